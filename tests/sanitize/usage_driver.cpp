// Stand-alone driver for the AddressSanitizer / UndefinedBehaviorSanitizer build of
// getRouteUsage's host route (DyMuPathPlanner::routeUsageOnHost) through
// the flat C-ABI: a 97x61 map with obstacles from the oracle's FMM, unit and full weights,
// subsets of outputs, the argument errors, and a goal set with a dominated goal.
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
  std::vector<double> u(n), u2(n), F(n), cost(n), T(n);
  oracle_fill_u01(u.data(), n, 21);
  oracle_fill_u01(u2.data(), n, 22);
  for (size_t k = 0; k < n; ++k) {
    const long i = (long)(k % NX), j = (long)(k / NX);
    const bool near_goal = (std::labs(i - (long)gi) <= 3 && std::labs(j - (long)gj) <= 3) ||
                           (std::labs(i - 12) <= 1 && std::labs(j - 9) <= 1);
    F[k] = (u2[k] < 0.04 && !near_goal) ? inf : 1.0 + 4.0 * u[k];
    cost[k] = F[k] < inf ? F[k] : -1.0;
  }
  uint64_t pops = 0;
  CHECK(oracle_fmm_heap(F.data(), NX, NY, gi, gj, -1, -1, T.data(), nullptr, &pops) >= 0);

  dymu_planner* h = nullptr;
  CHECK(dymu_planner_create(&h, 0.5, 1.0, 1.0, 1) == DYMU_OK);
  CHECK(dymu_planner_init_global_layer(h, 1.0, 0.5, NX, NY, 100.0, 200.0) == 1);
  CHECK(dymu_planner_set_cost_map(h, cost.data(), NX, NY) == 1);

  std::vector<uint64_t> usage(n), cat(4, 99);
  std::vector<double> far(n);
  std::vector<uint32_t> sink(n);
  dymu_usage_out all{};
  all.usage = usage.data(), all.far = far.data(), all.sink = sink.data();
  uint32_t rounds = 7;

  // without a goal nothing has a route and there is no catchment
  CHECK(dymu_planner_get_route_usage(h, nullptr, 0, &all, cat.data(), 4, &rounds) == DYMU_OK);
  for (size_t k = 0; k < n; ++k)
    CHECK(sink[k] == DYMU_LABEL_NONE && usage[k] == 0 && std::isnan(far[k]));
  CHECK(cat[0] == 0 && cat[3] == 0);

  CHECK(dymu_planner_set_goal(h, 100.0 + gi, 200.0 + gj, 0, 1.25) == 1);
  CHECK(dymu_planner_load_total_cost_map(h, T.data()) == 1);
  CHECK(dymu_planner_get_route_usage(h, nullptr, 0, &all, cat.data(), 4, &rounds) == DYMU_OK);
  CHECK(rounds == 0 && dymu_planner_last_paths_on_device(h) == 0);
  size_t routed = 0;
  double tmax = 0.0;
  for (size_t k = 0; k < n; ++k) {
    CHECK((sink[k] == 0) == (T[k] < inf) && (sink[k] == 0 || sink[k] == DYMU_LABEL_NONE));
    if (sink[k] != 0) {
      CHECK(usage[k] == 0 && std::isnan(far[k]));
      continue;
    }
    ++routed;
    tmax = T[k] > tmax ? T[k] : tmax;
    CHECK(usage[k] >= 1 && far[k] >= T[k]);
  }
  const size_t g = (size_t)gj * NX + gi;
  CHECK(routed > n * 9 / 10 && usage[g] == routed && far[g] == tmax);
  CHECK(cat[0] == routed && cat[1] == 0 && cat[3] == 0);

  // every weight 2^32 - 1: the sums carry past 32 bits; a subset of outputs leaves the
  // other maps alone; host = 1 is the same route
  std::vector<uint32_t> w(n, 0xFFFFFFFFu);
  std::vector<uint64_t> usage2(n, 77u);
  dymu_usage_out part{};
  part.usage = usage2.data();
  CHECK(dymu_planner_get_route_usage(h, w.data(), 1, &part, nullptr, 0, nullptr) == DYMU_OK);
  for (size_t k = 0; k < n; ++k) CHECK(usage2[k] == usage[k] * 0xFFFFFFFFull);
  CHECK(usage2[g] > (1ull << 44));
  dymu_usage_out none{};
  CHECK(dymu_planner_get_route_usage(h, nullptr, 0, &none, cat.data(), 1, nullptr) == DYMU_OK);
  CHECK(cat[0] == routed);

  // argument errors: nothing is written
  std::fill(usage2.begin(), usage2.end(), 77u);
  cat.assign(4, 99);
  CHECK(dymu_planner_get_route_usage(h, nullptr, 0, &none, nullptr, 0, nullptr) == DYMU_ERR_ARG);
  CHECK(dymu_planner_get_route_usage(h, nullptr, 0, &part, cat.data(), 0, nullptr) == DYMU_ERR_ARG);
  CHECK(dymu_planner_get_route_usage(h, nullptr, 0, nullptr, cat.data(), 4, nullptr) == DYMU_ERR_ARG);
  CHECK(dymu_planner_get_route_usage(nullptr, nullptr, 0, &part, nullptr, 0, nullptr) == DYMU_ERR_ARG);
  CHECK(dymu_planner_get_route_usage_to(h, 0, nullptr, &part, nullptr, 0, nullptr) == DYMU_ERR_ARG);
  for (size_t k = 0; k < n; ++k) CHECK(usage2[k] == 77u);
  CHECK(cat[0] == 99 && cat[3] == 99);

  // a goal set with a dominated third goal, on the smaller of two maps (not the seeded
  // solve, but every node still has its parent)
  const double goals[12] = {100.0 + gi, 200.0 + gj, 0, 0.1, 112.0, 209.0, 0, 0.2,
                            100.0 + gi - 2, 200.0 + gj - 2, 0, 0.3};
  const double offsets[3] = {0.0, 0.0, 50.0};
  CHECK(dymu_planner_set_goals(h, goals, offsets, 3) == 1);
  std::vector<double> T2(n);
  CHECK(oracle_fmm_heap(F.data(), NX, NY, 12, 9, -1, -1, T2.data(), nullptr, &pops) >= 0);
  for (size_t k = 0; k < n; ++k) T2[k] = T2[k] < T[k] ? T2[k] : T[k];
  CHECK(dymu_planner_load_total_cost_map(h, T2.data()) == 1);
  CHECK(dymu_planner_get_route_usage(h, nullptr, 0, &all, cat.data(), 2, nullptr) == DYMU_ERR_ARG);
  CHECK(dymu_planner_get_route_usage(h, nullptr, 0, &all, cat.data(), 4, &rounds) == DYMU_OK);
  size_t per[2] = {0, 0};
  for (size_t k = 0; k < n; ++k) {
    CHECK((sink[k] != DYMU_LABEL_NONE) == (T2[k] < inf));
    if (sink[k] == DYMU_LABEL_NONE) continue;
    CHECK(sink[k] < 2);  // the third goal is dominated: no root
    ++per[sink[k]];
  }
  CHECK(per[0] > 500 && per[1] > 500);
  CHECK(cat[0] == per[0] && cat[1] == per[1] && cat[2] == 0 && cat[3] == 0);
  CHECK(usage[g] == per[0] && usage[(size_t)9 * NX + 12] == per[1]);
  dymu_planner_destroy(h);
  std::printf("usage sanitize driver ok: %zu of %zu cells routed\n", routed, n);
  return 0;
}
