// Stand-alone driver for the AddressSanitizer / UndefinedBehaviorSanitizer build of
// getRouteFields' host route (DyMuPathPlanner::routeFieldsOnHost) through
// the flat C-ABI: a 97x61 map with obstacles from the oracle's FMM, every output with the
// speed map and a caller's field, subsets of outputs, the argument errors, and a goal set.
// The engine is tests/sanitize/engine_stub.c, so every call takes the host route.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "dymu_planner.h"
#include "oracle.h"

#define CHECK(c)                                                        \
  do {                                                                  \
    if (!(c)) {                                                         \
      std::fprintf(stderr, "CHECK failed: %s (line %d)\n", #c, __LINE__); \
      return 1;                                                         \
    }                                                                   \
  } while (0)

int main() {
  const uint32_t NX = 97, NY = 61, gi = 70, gj = 40;
  const size_t n = (size_t)NX * NY;
  const double inf = std::numeric_limits<double>::infinity();
  // U(1,5) speed with about 4 % obstacles, none next to the goals
  std::vector<double> u(n), u2(n), F(n), cost(n), T(n), elev(n);
  oracle_fill_u01(u.data(), n, 21);
  oracle_fill_u01(u2.data(), n, 22);
  for (size_t k = 0; k < n; ++k) {
    const long i = (long)(k % NX), j = (long)(k / NX);
    const bool near_goal = (std::labs(i - (long)gi) <= 3 && std::labs(j - (long)gj) <= 3) ||
                           (std::labs(i - 12) <= 1 && std::labs(j - 9) <= 1);
    F[k] = (u2[k] < 0.04 && !near_goal) ? inf : 1.0 + 4.0 * u[k];
    cost[k] = F[k] < inf ? F[k] : -1.0;
    elev[k] = 0.3 * std::sin(0.3 * (double)i) + 0.1 * std::cos(0.2 * (double)j) - 0.2;
  }
  uint64_t pops = 0;
  CHECK(oracle_fmm_heap(F.data(), NX, NY, gi, gj, -1, -1, T.data(), nullptr, &pops) >= 0);

  dymu_planner* h = nullptr;
  CHECK(dymu_planner_create(&h, 0.5, 1.0, 1.0, 1) == DYMU_OK);
  CHECK(dymu_planner_init_global_layer(h, 1.0, 0.5, NX, NY, 100.0, 200.0) == 1);
  CHECK(dymu_planner_set_cost_map(h, cost.data(), NX, NY) == 1);

  std::vector<uint32_t> sink(n), axis(n), diag(n);
  std::vector<double> length(n), integ[2], vmin[2], vmax[2];
  for (int f = 0; f < 2; ++f) integ[f].resize(n), vmin[f].resize(n), vmax[f].resize(n);
  dymu_route_out all{};
  all.sink = sink.data(), all.axis = axis.data(), all.diag = diag.data();
  all.length = length.data();
  for (int f = 0; f < 2; ++f)
    all.integral[f] = integ[f].data(), all.vmin[f] = vmin[f].data(), all.vmax[f] = vmax[f].data();
  const double* fields[2] = {nullptr, elev.data()};  // the speed map, the caller's field
  uint32_t rounds = 7;

  // without a goal nothing has a route
  CHECK(dymu_planner_get_route_fields(h, fields, 2, 0, &all, &rounds) == DYMU_OK);
  for (size_t k = 0; k < n; ++k)
    CHECK(sink[k] == DYMU_LABEL_NONE && axis[k] == 0 && std::isnan(length[k]) &&
          std::isnan(integ[1][k]) && vmin[0][k] == inf && vmax[1][k] == -inf);

  CHECK(dymu_planner_set_goal(h, 100.0 + gi, 200.0 + gj, 0, 1.25) == 1);
  CHECK(dymu_planner_load_total_cost_map(h, T.data()) == 1);
  CHECK(dymu_planner_get_route_fields(h, fields, 2, 0, &all, &rounds) == DYMU_OK);
  CHECK(rounds == 0 && dymu_planner_last_paths_on_device(h) == 0);
  size_t routed = 0;
  uint32_t longest = 0;
  for (size_t k = 0; k < n; ++k) {
    CHECK((sink[k] == 0) == (T[k] < inf) && (sink[k] == 0 || sink[k] == DYMU_LABEL_NONE));
    if (sink[k] != 0) {
      CHECK(axis[k] == 0 && diag[k] == 0 && std::isnan(length[k]) && std::isnan(integ[0][k]));
      continue;
    }
    ++routed;
    const uint32_t hops = axis[k] + diag[k];
    longest = hops > longest ? hops : longest;
    CHECK(length[k] == 1.0 * (double)axis[k] + (1.0 * 1.4142135623730951) * (double)diag[k]);
    CHECK(vmin[0][k] >= 1.0 && vmax[0][k] <= 5.0 && vmin[1][k] <= elev[k] && vmax[1][k] >= elev[k]);
    CHECK(integ[0][k] >= length[k] * (1 - 1e-12) && integ[0][k] <= 5.0 * length[k] * (1 + 1e-12));
    const long di = std::labs((long)(k % NX) - (long)gi), dj = std::labs((long)(k / NX) - (long)gj);
    CHECK((long)hops >= (di > dj ? di : dj));
  }
  CHECK(routed > n * 9 / 10 && longest >= 60);
  CHECK(axis[(size_t)gj * NX + gi] == 0 && length[(size_t)gj * NX + gi] == 0.0);

  // a subset of outputs leaves the other maps alone; host = 1 is the same route
  std::vector<uint32_t> sink2(n, 77u);
  std::vector<double> vmax2(n, -5.0);
  dymu_route_out part{};
  part.sink = sink2.data();
  part.vmax[0] = vmax2.data();
  const double* one[1] = {elev.data()};
  CHECK(dymu_planner_get_route_fields(h, one, 1, 1, &part, nullptr) == DYMU_OK);
  for (size_t k = 0; k < n; ++k) CHECK(sink2[k] == sink[k] && vmax2[k] == vmax[1][k]);
  dymu_route_out none{};
  CHECK(dymu_planner_get_route_fields(h, nullptr, 0, 0, &none, &rounds) == DYMU_OK);

  // argument errors: nothing is written
  dymu_route_out bad = part;
  bad.vmin[1] = vmax2.data();  // beyond n_fields
  CHECK(dymu_planner_get_route_fields(h, one, 1, 0, &bad, nullptr) == DYMU_ERR_ARG);
  CHECK(dymu_planner_get_route_fields(h, one, 5, 0, &part, nullptr) == DYMU_ERR_ARG);
  CHECK(dymu_planner_get_route_fields(h, nullptr, 1, 0, &part, nullptr) == DYMU_ERR_ARG);
  CHECK(dymu_planner_get_route_fields(h, one, 1, 0, nullptr, nullptr) == DYMU_ERR_ARG);
  CHECK(dymu_planner_get_route_fields(nullptr, one, 1, 0, &part, nullptr) == DYMU_ERR_ARG);
  CHECK(dymu_planner_get_route_fields_to(h, 0, one, 1, &part, nullptr) == DYMU_ERR_ARG);

  // a goal set with an offset and a dominated third goal, on the smaller of two maps (not
  // the seeded solve, but every node still has its parent)
  const double goals[12] = {100.0 + gi, 200.0 + gj, 0, 0.1, 112.0, 209.0, 0, 0.2,
                            100.0 + gi - 2, 200.0 + gj - 2, 0, 0.3};
  const double offsets[3] = {0.0, 0.0, 50.0};
  CHECK(dymu_planner_set_goals(h, goals, offsets, 3) == 1);
  std::vector<double> T2(n);
  CHECK(oracle_fmm_heap(F.data(), NX, NY, 12, 9, -1, -1, T2.data(), nullptr, &pops) >= 0);
  for (size_t k = 0; k < n; ++k) T2[k] = T2[k] < T[k] ? T2[k] : T[k];
  CHECK(dymu_planner_load_total_cost_map(h, T2.data()) == 1);
  CHECK(dymu_planner_get_route_fields(h, fields, 2, 0, &all, &rounds) == DYMU_OK);
  size_t per[2] = {0, 0};
  for (size_t k = 0; k < n; ++k) {
    CHECK((sink[k] != DYMU_LABEL_NONE) == (T2[k] < inf));
    if (sink[k] == DYMU_LABEL_NONE) continue;
    CHECK(sink[k] < 2);  // the third goal is dominated: no root
    ++per[sink[k]];
  }
  CHECK(per[0] > 500 && per[1] > 500);
  CHECK(sink[(size_t)9 * NX + 12] == 1 && axis[(size_t)9 * NX + 12] + diag[(size_t)9 * NX + 12] == 0);
  dymu_planner_destroy(h);
  std::printf("route sanitize driver ok: %zu of %zu cells routed, longest %u hops\n", routed, n,
              longest);
  return 0;
}
