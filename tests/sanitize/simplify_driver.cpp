// Stand-alone driver for the AddressSanitizer / UndefinedBehaviorSanitizer build of
// getSimplifiedPaths' host route (DyMuPathPlanner::descendArriving with the rule of
// csrc/path_simplify.h) through the flat C-ABI: a map with obstacles from
// the oracle's FMM, starts inside, on the edges and off the grid, several eps, small walk
// limits, a goal set, and both forms of the two-call protocol.  The engine is
// tests/sanitize/engine_stub.c, so every call takes the host route.
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

  // the unsimplified paths, packed: what every simplified waypoint must be a copy of
  std::vector<int> fcnt(M), fst(M);
  std::vector<dymu_arrive_stat> frec(M);
  CHECK(dymu_planner_get_arriving_paths(h, starts.data(), M, 1 << 20, 1, nullptr, fcnt.data(),
                                        fst.data(), frec.data()) == M);
  size_t ftotal = 0;
  std::vector<size_t> fat(M);
  for (int q = 0; q < M; ++q) {
    fat[q] = ftotal;
    ftotal += (size_t)fcnt[q];
  }
  std::vector<double> full(4 * ftotal + 4);
  CHECK(dymu_planner_get_arriving_paths(h, nullptr, M, 0, 0, full.data(), nullptr, nullptr,
                                        nullptr) == M);

  std::vector<int> cnt(M), st(M), sinks(M);
  std::vector<dymu_arrive_stat> rec(M);
  size_t kept_all = 0;
  for (double eps : {1e-6, 0.05, 0.25, 1.0, 50.0}) {
    CHECK(dymu_planner_get_simplified_paths(h, starts.data(), M, eps, 1 << 20, nullptr, nullptr,
                                            cnt.data(), st.data(), rec.data()) == M);
    CHECK(dymu_planner_last_paths_on_device(h) == 0);
    CHECK(dymu_planner_last_path_sinks(h, sinks.data(), M) == M);
    uint64_t reruns = 1, bytes = 1;
    CHECK(dymu_planner_last_simplified(h, &reruns, &bytes) == DYMU_OK && !reruns && !bytes);
    size_t total = 0;
    for (int q = 0; q < M; ++q) {
      CHECK(st[q] == fst[q] && sinks[q] == rec[q].sink);
      CHECK(rec[q].status == frec[q].status && rec[q].count == frec[q].count &&
            rec[q].hops == frec[q].hops && rec[q].length == frec[q].length &&
            rec[q].start_cost == frec[q].start_cost);
      CHECK(cnt[q] >= 0 && cnt[q] <= fcnt[q]);
      if (q >= M - 5) CHECK(st[q] == -1 && cnt[q] == 0);
      total += (size_t)cnt[q];
    }
    std::vector<double> out(4 * total + 4);
    std::vector<uint32_t> idx(total + 1);
    CHECK(dymu_planner_get_simplified_paths(h, nullptr, M, 0, 0, out.data(), idx.data(), nullptr,
                                            nullptr, nullptr) == M);
    size_t at = 0;
    for (int q = 0; q < M; ++q) {
      for (int k = 0; k < cnt[q]; ++k) {
        const uint32_t i = idx[at + k];
        CHECK(i < (uint32_t)fcnt[q] && (k == 0 || i > idx[at + k - 1]));
        for (int c = 0; c < 4; ++c)
          CHECK(out[4 * (at + k) + c] == full[4 * (fat[q] + i) + c]);
      }
      if (cnt[q]) CHECK(idx[at] == 0 && idx[at + cnt[q] - 1] == (uint32_t)fcnt[q] - 1);
      at += (size_t)cnt[q];
    }
    kept_all += total;
  }
  // small walk limits; the one call that computes and copies, with and without indices
  for (int max_wp : {1, 2, 7}) {
    std::vector<double> few(4 * (size_t)max_wp * M + 4);
    std::vector<uint32_t> fidx((size_t)max_wp * M + 1);
    CHECK(dymu_planner_get_simplified_paths(h, starts.data(), M, 0.25, max_wp, few.data(),
                                            fidx.data(), cnt.data(), st.data(), rec.data()) == M);
    for (int q = 0; q < M; ++q)
      CHECK(cnt[q] <= max_wp && (st[q] == -3 || frec[q].count <= (uint32_t)max_wp));
    CHECK(dymu_planner_get_simplified_paths(h, starts.data(), M, 0.25, max_wp, few.data(), nullptr,
                                            nullptr, nullptr, nullptr) == M);
  }
  CHECK(dymu_planner_get_simplified_paths(h, starts.data(), M, 0.0, 16, nullptr, nullptr,
                                          cnt.data(), nullptr, nullptr) == DYMU_ERR_ARG);
  CHECK(dymu_planner_get_simplified_paths(h, starts.data(), M, std::nan(""), 16, nullptr, nullptr,
                                          cnt.data(), nullptr, nullptr) == DYMU_ERR_ARG);
  CHECK(dymu_planner_get_simplified_paths(h, starts.data(), M, 0.25, 0, nullptr, nullptr,
                                          cnt.data(), nullptr, nullptr) == DYMU_ERR_ARG);
  CHECK(dymu_planner_get_simplified_paths_to(h, 0, starts.data(), M, 0.25, 16, nullptr, nullptr,
                                             cnt.data(), nullptr, nullptr) == DYMU_ERR_ARG);
  // a result that is computed and never copied out is dropped with the handle
  CHECK(dymu_planner_get_simplified_paths(h, starts.data(), M, 0.25, 1 << 20, nullptr, nullptr,
                                          cnt.data(), st.data(), nullptr) == M);

  // a goal set: labels by the host routine, the sink follows the node's label
  const double goals[8] = {100.0 + gi, 200.0 + gj, 0, 0.1, 110.0, 208.0, 0, 0.2};
  CHECK(dymu_planner_set_goals(h, goals, nullptr, 2) == 1);
  std::vector<double> T2(n);
  CHECK(oracle_fmm_heap(F.data(), NX, NY, 10, 8, -1, -1, T2.data(), nullptr, &pops) >= 0);
  for (size_t k = 0; k < n; ++k) T2[k] = T2[k] < T[k] ? T2[k] : T[k];
  CHECK(dymu_planner_load_total_cost_map(h, T2.data()) == 1);
  CHECK(dymu_planner_get_simplified_paths(h, starts.data(), M, 0.25, 1 << 20, nullptr, nullptr,
                                          cnt.data(), st.data(), rec.data()) == M);
  CHECK(dymu_planner_last_path_sinks(h, sinks.data(), M) == M);
  int arrived = 0;
  for (int q = 0; q < M; ++q) {
    CHECK((st[q] == 1) == (sinks[q] == 0 || sinks[q] == 1));
    arrived += st[q] == 1;
  }
  CHECK(arrived >= 50);
  dymu_planner_destroy(h);
  std::printf("simplify sanitize driver ok: %d of %d arrive, %zu of %zu waypoints kept\n", arrived,
              M, kept_all, 5 * ftotal);
  return 0;
}
