// Stand-alone driver for the AddressSanitizer / UndefinedBehaviorSanitizer build of the
// arriving descent's host rule (DyMuPathPlanner::descendArriving) through
// the flat C-ABI: a map with obstacles from the oracle's FMM, starts inside, on the edges
// and off the grid, small max_wp, a stride, a goal set, and the two-call protocol.  The
// engine is tests/sanitize/engine_stub.c, so every call takes the host route.
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
  const uint32_t NX = 61, NY = 47, gi = 40, gj = 30;
  const size_t n = (size_t)NX * NY;
  const double inf = std::numeric_limits<double>::infinity();
  // U(1,5) speed with about 4 % obstacles, none next to the goals
  std::vector<double> u(n), u2(n), F(n), cost(n), T(n);
  oracle_fill_u01(u.data(), n, 21);
  oracle_fill_u01(u2.data(), n, 22);
  for (size_t k = 0; k < n; ++k) {
    const long i = (long)(k % NX), j = (long)(k / NX);
    const bool near_goal = (std::labs(i - (long)gi) <= 1 && std::labs(j - (long)gj) <= 1) ||
                           (std::labs(i - 10) <= 1 && std::labs(j - 8) <= 1);
    F[k] = (u2[k] < 0.04 && !near_goal) ? inf : 1.0 + 4.0 * u[k];
    cost[k] = F[k] < inf ? F[k] : -1.0;
  }
  uint64_t pops = 0;
  CHECK(oracle_fmm_heap(F.data(), NX, NY, gi, gj, -1, -1, T.data(), nullptr, &pops) >= 0);

  dymu_planner* h = nullptr;
  CHECK(dymu_planner_create(&h, 0.5, 1.0, 1.0, 1) == DYMU_OK);
  CHECK(dymu_planner_init_global_layer(h, 1.0, 0.5, NX, NY, 100.0, 200.0) == 1);
  CHECK(dymu_planner_set_cost_map(h, cost.data(), NX, NY) == 1);
  CHECK(dymu_planner_set_goal(h, 100.0 + gi, 200.0 + gj, 0, 1.25) == 1);
  CHECK(dymu_planner_load_total_cost_map(h, T.data()) == 1);

  std::vector<double> starts;
  auto add = [&](double x, double y) {
    starts.insert(starts.end(), {100.0 + x, 200.0 + y, 0.0, 0.0});
  };
  for (uint32_t q = 0; q < 60; ++q) add(1.0 + 58.0 * u[q], 1.0 + 44.0 * u2[q + 100]);
  add(0.0, 0.0), add(NX - 1.0, NY - 1.0), add(NX - 0.6, 3.2), add(7.7, NY - 0.51);  // edges
  add(-0.2, 5.0), add(5.0, NY - 0.4), add(std::nan(""), 5.0), add(1e300, 5.0), add(5.0, -1e300);
  const int M = (int)(starts.size() / 4);
  std::vector<int> cnt(M), st(M), sinks(M);
  std::vector<dymu_arrive_stat> rec(M), only(M);
  CHECK(dymu_planner_get_arriving_paths(h, starts.data(), M, 1 << 20, 1, nullptr, cnt.data(),
                                        st.data(), rec.data()) == M);
  CHECK(dymu_planner_last_path_sinks(h, sinks.data(), M) == M);
  CHECK(dymu_planner_last_paths_on_device(h) == 0);
  size_t total = 0;
  int arrived = 0;
  for (int q = 0; q < M; ++q) {
    CHECK(st[q] == rec[q].status && sinks[q] == rec[q].sink);
    CHECK(cnt[q] == (int)rec[q].count);
    CHECK(st[q] == 1 || st[q] == -1);
    if (q >= M - 5) CHECK(st[q] == -1 && cnt[q] == 0);
    total += (size_t)cnt[q];
    arrived += st[q] == 1;
  }
  CHECK(arrived >= 50);
  std::vector<double> out(4 * total + 4);
  CHECK(dymu_planner_get_arriving_paths(h, nullptr, M, 0, 0, out.data(), nullptr, nullptr,
                                        nullptr) == M);
  CHECK(dymu_planner_get_arriving_stats(h, starts.data(), M, 1 << 20, 1, only.data()) == M);
  for (int q = 0; q < M; ++q)
    CHECK(only[q].status == rec[q].status && only[q].count == rec[q].count &&
          only[q].hops == rec[q].hops && only[q].length == rec[q].length);
  // every path ends on the sink; small capacities and a stride
  size_t at = 0;
  for (int q = 0; q < M; ++q) {
    if (st[q] == 1) {
      const double* last = &out[4 * (at + (size_t)cnt[q] - 1)];
      CHECK(last[0] == 100.0 + gi && last[1] == 200.0 + gj && last[3] == 1.25);
    }
    at += (size_t)cnt[q];
  }
  for (int max_wp : {1, 2, 7}) {
    std::vector<double> few(4 * (size_t)max_wp * M);
    CHECK(dymu_planner_get_arriving_paths(h, starts.data(), M, max_wp, 1, few.data(), cnt.data(),
                                          st.data(), only.data()) == M);
    for (int q = 0; q < M; ++q)
      CHECK(cnt[q] <= max_wp && (st[q] == -3 || rec[q].count <= (uint32_t)max_wp));
  }
  std::vector<double> thin(4 * total + 4);
  CHECK(dymu_planner_get_arriving_paths(h, starts.data(), M, 1 << 20, 5, thin.data(), cnt.data(),
                                        st.data(), only.data()) == M);
  for (int q = 0; q < M; ++q) CHECK(only[q].count == rec[q].count && cnt[q] <= (int)rec[q].count);
  CHECK(dymu_planner_get_arriving_stats(h, starts.data(), M, 0, 1, only.data()) == DYMU_ERR_ARG);
  CHECK(dymu_planner_get_arriving_stats_to(h, 0, starts.data(), M, 16, only.data()) == DYMU_ERR_ARG);

  // a goal set: labels by the host routine, the sink follows the node's label
  const double goals[8] = {100.0 + gi, 200.0 + gj, 0, 0.1, 110.0, 208.0, 0, 0.2};
  CHECK(dymu_planner_set_goals(h, goals, nullptr, 2) == 1);
  std::vector<double> T2(n);
  CHECK(oracle_fmm_heap(F.data(), NX, NY, 10, 8, -1, -1, T2.data(), nullptr, &pops) >= 0);
  // the smaller of the two maps: not the seeded solve, but every node still has its parent
  for (size_t k = 0; k < n; ++k) T2[k] = T2[k] < T[k] ? T2[k] : T[k];
  CHECK(dymu_planner_load_total_cost_map(h, T2.data()) == 1);
  CHECK(dymu_planner_get_arriving_paths(h, starts.data(), M, 1 << 20, 1, nullptr, cnt.data(),
                                        st.data(), rec.data()) == M);
  CHECK(dymu_planner_last_path_sinks(h, sinks.data(), M) == M);
  for (int q = 0; q < M; ++q) CHECK((st[q] == 1) == (sinks[q] == 0 || sinks[q] == 1));
  dymu_planner_destroy(h);
  std::printf("arrive sanitize driver ok: %d of %d arrive, %zu waypoints\n", arrived, M, total);
  return 0;
}
