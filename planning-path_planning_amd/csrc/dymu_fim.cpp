// dymu_fim.cpp -- C-ABI runtime (include/dymu_fim.h) around the HIP block-FIM
// kernels (fim_kernels.hip).  Owns the stream, events and the tile workspace;
// drives passes until the active-tile list drains.
//
// Replaces the host loop of computeEntireTotalCostMap
// (src/DyMu_GlobalPathPlanning.cpp:443-468): the reference pops one node per
// iteration from a linear-scan narrow band; here each pass relaxes every
// active tile in parallel and the device builds the next active list itself,
// so the host only reads a 4-byte counter every few passes.
#include "dymu_fim.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <chrono>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "fim_kernels.h"

using namespace dymu;

// The words of dymu_ctx::d_scratch, one name per use.  A use lives from the
// kernel that writes it to its read-back in the same call, so two names share a word only
// where no call has both live: the clearance entries read kScrObst / kScrFreed back before
// the edit's raise zeroes the same words for kScrEditStats; kScrCount, kScrRaiseStats and
// kScrReset belong to three other entries, and so do the probe and the box.  kScrTheta is
// live across the single-goal raise.  Word 1 is free.
enum ScratchSlot {
  kScrTheta = 0,       // smallest old value around the window / smallest key queued
  kScrProbe = 2,       // 2 words: the early-exit probe's (max T, min key)
  kScrBox = 2,         // 2 words: claimed_box's {x0, y0} and {x1, y1} in tiles
  kScrCount = 4,       // early-exit band / equal-value cells counted
  kScrObst = 4,        // obstacle cells seeded (clearance), added in a window
  kScrFreed = 5,       // obstacle cells a window frees; read back with kScrObst
  kScrEditStats = 4,   // 2 words: the clearance edit's raise [visits, cells]
  kScrRaiseStats = 5,  // 2 words: the single-goal raise [visits, cells]
  kScrReset = 5,       // cells the per-plane update reset
  kScrRoundTotal = 7,  // dom_round's tiles queued for its first pass (32 bits)
  kScrWords = 8
};

struct dymu_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  hipEvent_t ev_path0 = nullptr, ev_path1 = nullptr;  // around the last k_extract_paths
  bool path_timed = false;
  hipEvent_t ev_pstat0 = nullptr, ev_pstat1 = nullptr;  // around the last k_path_stats
  bool pstat_timed = false;
  hipEvent_t ev_arr0 = nullptr, ev_arr1 = nullptr;  // around the last k_arrive_paths
  bool arr_timed = false;
  hipEvent_t ev_simp0 = nullptr, ev_simp1 = nullptr;  // around the last simplified k_arrive_paths
  bool simp_timed = false;
  uint32_t* d_pq = nullptr;  // k_path_stats' work queue: the next path index
  hipEvent_t ev_lab0 = nullptr, ev_lab1 = nullptr;  // around the last dymu_goal_labels_device
  bool lab_timed = false;
  uint32_t* d_lab_cnt = nullptr;  // kLabelRounds + 1 counters of unresolved label entries
  // the last dymu_route_fields_device: before init, after it, after the rounds, after finalize
  hipEvent_t ev_route[4] = {nullptr, nullptr, nullptr, nullptr};
  bool route_timed = false;
  // the last dymu_route_usage_device: the same four stamps, and one before every round
  // launched with one behind the last
  hipEvent_t ev_usage[4] = {nullptr, nullptr, nullptr, nullptr};
  hipEvent_t ev_usage_round[kRouteRounds + 1] = {};
  uint32_t usage_rounds_timed = 0;
  bool usage_timed = false;
  dymu_opts opts{};
  int cu_count = 256;
  uint32_t* d_xchg = nullptr;  // k_exchange's block ticket (zero between launches)

  // 3: two 8x8 tiles per wave (red-black), 4: v3 body + priority passes;
  // 5: priority passes on 16x16 tiles (one per wave, 16-wave workgroups);
  // 0 (default): per domain, 5 from prio_min_tiles 8x8 tiles up, else 3.  Since the
  // checkerboard passes (v23) kernel 5 is the faster one at every size measured (256^2:
  // 0.45 vs 0.51 ms, 1024^2: 1.22 vs 1.63, 2048^2: 2.4-2.9 vs 4.1-4.3, 2896^2: 3.52 vs
  // 6.60; profiles/r02/small_grids.txt), so the threshold is 0.
  // DYMU_KERNEL overrides
  int variant = 0;
  uint32_t prio_min_tiles = 0;  // DYMU_PRIO_MIN_TILES
  uint32_t prio_target = 0;  // v4/v5: tiles relaxed per pass; 0 = per-variant default
  double prio_kappa = 0.5;   // v4: histogram bin width / mean F (DYMU_PRIO_KAPPA)
  float prio_frac = 0.0f;    // v4: ... or this fraction of the active list (DYMU_PRIO_FRAC)
  int prio_trace = -1;       // v4: stamp phases of this pass index (DYMU_PRIO_TRACE)
  unsigned long long* d_trace = nullptr;
  int prune = 1;             // v4/v5 exact activation pruning (DYMU_PRUNE=0 disables)
  int occupancy[6] = {0, 0, 0, 6, 5, 1};  // pass workgroups per CU (occupancy API)
  // passes before the first convergence read-back (then doubling to 64): 16 saves two
  // host round trips per solve (4096^2: 5.88 vs 5.96 ms; DYMU_FIRST_BATCH)
  uint64_t first_batch = 16;
  // convergence checks without host round trips: every pass posts the tiles queued for
  // it to a host-coherent mailbox and the host keeps max_batch passes queued ahead of the
  // running one (2, converge_stream; default), or the first pass of each batch posts and
  // the next batch is queued before the host reads it (1, converge_pipelined), or the
  // host synchronises on the counters after each batch (0, converge).  DYMU_PIPELINE,
  // DYMU_MAX_BATCH (passes queued ahead / batch size) override.  16384^2: 35.94 / 36.13 /
  // 36.58 ms, 4096^2: 5.85 / 5.91 / 5.96 ms (profiles/r02/pipe_*.log)
  int pipeline = 2;
  uint64_t max_batch = 4;
  unsigned long long* h_mail = nullptr;  // pinned, host-coherent: (seq << 32) | pending
  unsigned long long* d_mail = nullptr;  // its device address
  uint32_t mail_seq = 0;
  // a post armed by dymu_dom_post for the next launched pass (sharded loop)
  const int32_t* arm_src = nullptr;
  uint32_t arm_seq = 0;
  unsigned long long* arm_dst = nullptr;       // another post target (the peer status ring)
  const unsigned long long* arm_ext = nullptr;  // ... with these 4 status words
  int prio_debug = 0;        // v4: print the state after the first N passes (DYMU_PRIO_DEBUG)

  // tile workspace
  uint32_t tiles_cap = 0;
  uint32_t* d_lists = nullptr;       // 3 lists x kShards shards x tiles_cap
  uint32_t* d_counts = nullptr;      // 3 x kShards words, own block
  uint32_t* d_tile_epoch = nullptr;  // tiles_cap
  unsigned long long* d_stats = nullptr;  // kStatSlots
  // v4 priority state: keys 3 x tiles_cap, hist 3 x kShards x kBins,
  // prio = {minkey[3] (u64), base[3] (f64), delta (f64), 1 / delta (f64)}
  unsigned long long* d_keys = nullptr;
  uint32_t keys_cap = 0;
  uint32_t* d_hist = nullptr;
  unsigned long long* d_prio = nullptr;
  uint32_t epoch_base = 0;
  uint32_t* h_count = nullptr;  // pinned
  unsigned long long* h_probe = nullptr;  // pinned [2]: early-exit probe (max T, min key)
  uint64_t* d_band = nullptr;   // early-exit band indices (device)
  uint64_t band_cap = 0;
  // dymu_find_equal / dymu_scatter exchange indices and values through this pinned,
  // host-coherent, device-mapped buffer, which their kernels read and write in place
  void* h_xfer = nullptr;       // host address
  void* d_xfer = nullptr;       // its device address
  uint64_t xfer_cap = 0;        // bytes
  unsigned long long* d_region = nullptr;  // dymu_region_stats' 8 device words
  // dymu_batch_reduce_device / dymu_level_mask_device (reduce_kernels.hip):
  // the term list staged in pinned memory and copied to the device on the call's stream
  // (ev_red_copy: the copy has read the pinned list, which the next call rewrites); one
  // partial per workgroup, then the summary record and the level mask's words; 64 pinned
  // bytes for the results
  ReduceTerm* h_red_terms = nullptr;
  ReduceTerm* d_red_terms = nullptr;
  uint32_t red_cap = 0;
  ReducePartial* d_red_part = nullptr;
  uint32_t red_blocks = 0;
  void* h_red_res = nullptr;
  hipEvent_t ev_red_copy = nullptr, ev_red0 = nullptr, ev_red1 = nullptr;
  bool red_copy_pending = false, red_timed = false;
  unsigned long long* d_scratch = nullptr;  // kScrWords device scalars (ScratchSlot)
  double* d_lut = nullptr;      // computeCostMap LUT (device copy)
  size_t lut_cap = 0;

  // host-solve staging
  double* d_F = nullptr;
  double* d_T = nullptr;
  uint64_t cells_cap = 0;
  // the staged d_T holds the converged map of the last host solve of this grid
  bool host_valid = false;
  uint32_t host_nx = 0, host_ny = 0, host_gi = 0, host_gj = 0;

  // current domain (whole grid or one row slab) being solved
  struct Dom {
    bool live = false;
    int variant = 3;
    PassArgs a{};
    uint32_t ntiles = 0;
    uint32_t eb = 0;
    uint64_t p = 0;         // next pass index
    uint64_t launches = 0;
    uint64_t max_passes = 0;
    int blocks = 0;
    bool rehist = false;  // rebuild each list's histogram from its final keys
    uint32_t* lists[3] = {nullptr, nullptr, nullptr};
    uint32_t* counts[3] = {nullptr, nullptr, nullptr};
    size_t prof_used = 0;
  } dom;

  // per-pass statistics (kernel 5; dymu_set_pass_stats): kPassStatCap records of
  // kShards x kPsWords words, pass p at p % kPassStatCap
  int pass_stats = 0;
  uint32_t* d_pstat = nullptr;
  // kernel 5 edge columns (PassArgs::ec): 32 doubles per 16x16 tile; 1.5-2% per
  // 16384^2 solve against the per-row W / E halo loads (profiles/r03/ec)
  int use_ec = 1;
  // device memory kinds (dev_alloc): the maps (dymu_device_alloc, host-solve staging):
  // uncached -- a pass's write-backs leave no dirty L2 lines for its end-of-kernel
  // release (27.52-27.72 vs 28.06-28.28 ms per 16384^2 solve, profiles/r06/map_mem_ab.txt);
  // the tile workspace: cached (uncached lists / keys / edge columns cost +0.6%).
  // DYMU_MAP_MEM / DYMU_WS_MEM override (A/B)
  int map_mem = 2, ws_mem = 0, ec_mem = 0, key_mem = 0;
  double* d_ec = nullptr;
  uint64_t ec_cap = 0;  // tiles
  std::vector<void*> parked;  // outgrown device buffers, freed by dymu_destroy (park)
  // windowed updates with increases: theta reset (0, default) or the raise front (1,
  // DYMU_RAISE=1: exact dependency cone, measured slower on config 5 -- 9.5 vs 4.1 ms
  // at 4096^2, profiles/r03/configs_4096_r03c.json); the last
  // update's raise passes, raise visits, cells invalidated
  int raise = 0;
  uint64_t last_update[4] = {0, 0, 0, 0};
  // theta per plane of the seeded / stacked windowed update (update_planes_core)
  unsigned long long* d_theta = nullptr;
  uint32_t theta_cap = 0;
  // early exit on target cells (converge_targets): 2 + planes words the
  // probe kernel fills (max T, min key, max T per plane), and the passes between two
  // checks once the first first_batch passes have run (DYMU_UNTIL_BATCH overrides)
  unsigned long long* d_until = nullptr;
  uint32_t until_cap = 0;
  uint64_t until_batch = 16;
  // dymu_set_stepping: the device-resident entries return after their preparation with
  // the domain live (converge_auto); the caller runs the passes (tests of the stages)
  bool stepping = false;

  // profiling
  int profiling = 0;
  std::vector<hipEvent_t> prof_ev;
  double last_pass_ms = 0.0;
  uint64_t last_launches = 0;
  uint64_t last_timed = 0;  // sampled launches behind last_pass_ms

  std::string last_error;
};

namespace {

int fail_hip(dymu_ctx* c, hipError_t e, const char* what) {
  if (c) {
    char buf[256];
    std::snprintf(buf, sizeof buf, "%s: %s (%d)", what, hipGetErrorString(e), (int)e);
    c->last_error = buf;
  }
  return e == hipErrorOutOfMemory ? DYMU_ERR_NOMEM : DYMU_ERR_HIP;
}

#define HIPC(ctx, expr)                                  \
  do {                                                   \
    hipError_t _e = (expr);                              \
    if (_e != hipSuccess) return fail_hip(ctx, _e, #expr); \
  } while (0)

// Device memory by kind (A/B knobs): 0 hipMalloc (coarse-grained,
// L2-cached), 1 fine-grained, 2 uncached (no L2: nothing dirty for a kernel's
// end-of-pass release to write back)
hipError_t dev_alloc(void** p, size_t bytes, int kind) {
  if (kind == 1) return hipExtMallocWithFlags(p, bytes, hipDeviceMallocFinegrained);
  if (kind == 2) return hipExtMallocWithFlags(p, bytes, hipDeviceMallocUncached);
  return hipMalloc(p, bytes);
}
template <class P>
hipError_t dev_alloc(P** p, size_t bytes, int kind) {
  return dev_alloc(reinterpret_cast<void**>(p), bytes, kind);
}

// A buffer the engine has outgrown is kept until dymu_destroy, not freed: a solve whose
// buffers were allocated where device memory had just been freed has returned wrong maps
// (tools/history_probe.py, tests/test_gpu_engine_history.py).  A grown
// capacity is at least twice the old one, so the parked buffers of a kind together stay
// below the live one; if the doubled request does not fit, the exact one is tried.
void park(dymu_ctx* c, void* p) {
  if (p) c->parked.push_back(p);
}
uint64_t grown(uint64_t need, uint64_t cap, uint64_t limit) {
  return std::min(std::max(need, 2 * cap), limit);
}
// alloc(n) for n = want, then n = need (want >= need): the capacity obtained, 0 if neither fits
template <class Alloc>
uint64_t alloc_grown(uint64_t want, uint64_t need, Alloc alloc) {
  if (alloc(want) == hipSuccess) return want;
  (void)hipGetLastError();
  return want != need && alloc(need) == hipSuccess ? need : 0;
}

int ensure_tiles(dymu_ctx* c, uint32_t need, hipStream_t st) {
  if (need <= c->tiles_cap) return DYMU_OK;
  park(c, c->d_lists);
  park(c, c->d_tile_epoch);
  c->d_lists = nullptr;
  c->d_tile_epoch = nullptr;
  const uint64_t old = c->tiles_cap;
  c->tiles_cap = 0;
  const uint32_t ntiles = (uint32_t)alloc_grown(grown(need, old, (1ull << 31) - 1), need, [&](uint64_t n) {
    hipError_t e = dev_alloc(&c->d_lists, sizeof(uint32_t) * 3ull * kShards * n, c->ws_mem);
    if (e != hipSuccess) return e;
    e = dev_alloc(&c->d_tile_epoch, sizeof(uint32_t) * n, c->ws_mem);
    if (e != hipSuccess) {
      (void)hipFree(c->d_lists);  // never used: nothing was placed behind it
      c->d_lists = nullptr;
    }
    return e;
  });
  if (!ntiles) return fail_hip(c, hipErrorOutOfMemory, "tile workspace");
  HIPC(c, hipMemsetAsync(c->d_tile_epoch, 0, sizeof(uint32_t) * (uint64_t)ntiles, st));
  c->tiles_cap = ntiles;  // epoch_base stays: every stamp of the new array is 0, below any base
  return DYMU_OK;
}

int ensure_prio(dymu_ctx* c, uint32_t need) {
  // 3 list histograms + 2 rebuild buffers (deterministic mode)
  if (!c->d_hist) HIPC(c, hipMalloc(&c->d_hist, sizeof(uint32_t) * 5 * kShards * kBins));
  if (!c->d_prio) HIPC(c, hipMalloc(&c->d_prio, sizeof(unsigned long long) * 8));
  if (need <= c->keys_cap) return DYMU_OK;
  park(c, c->d_keys);
  c->d_keys = nullptr;
  const uint64_t old = c->keys_cap;
  c->keys_cap = 0;
  const uint32_t ntiles = (uint32_t)alloc_grown(grown(need, old, (1ull << 31) - 1), need, [&](uint64_t n) {
    return dev_alloc(&c->d_keys, sizeof(unsigned long long) * 3ull * n, c->key_mem);
  });
  if (!ntiles) return fail_hip(c, hipErrorOutOfMemory, "tile keys");
  c->keys_cap = ntiles;
  return DYMU_OK;
}

// The transfer buffer of dymu_find_equal / dymu_scatter: pinned host memory the
// kernels access in place, so no copy command stands between the host's data and
// the kernel.  Round 5's version staged through hipMallocAsync memory with copies; on
// this stack (ROCm 7.2, gfx950) a stream-ordered pool allocation is not seen alike by
// the copy paths and the kernels beyond its first 4 KiB page -- a kernel read an
// earlier allocation's bytes, whatever the copy's source, synchronicity or ordering
// (tools/copy_order_probe.hip, profiles/r06/copy_order_probe.jsonl).
// Callers synchronise the stream before the buffer is rewritten.
int ensure_xfer(dymu_ctx* c, uint64_t bytes) {
  if (bytes <= c->xfer_cap) return DYMU_OK;
  if (c->h_xfer) HIPC(c, hipHostFree(c->h_xfer));
  c->h_xfer = c->d_xfer = nullptr;
  c->xfer_cap = 0;
  bytes = std::max<uint64_t>(bytes, 1u << 16);
  HIPC(c, hipHostMalloc(&c->h_xfer, bytes, hipHostMallocCoherent | hipHostMallocMapped));
  c->xfer_cap = bytes;
  HIPC(c, hipHostGetDevicePointer(&c->d_xfer, c->h_xfer, 0));
  return DYMU_OK;
}

// the staged maps of the host path: outgrown ones are parked as well (see park)
int ensure_cells(dymu_ctx* c, uint64_t need) {
  if (need <= c->cells_cap) return DYMU_OK;
  c->host_valid = false;
  park(c, c->d_F);
  park(c, c->d_T);
  c->d_F = c->d_T = nullptr;
  const uint64_t old = c->cells_cap;
  c->cells_cap = 0;
  const uint64_t cells = alloc_grown(grown(need, old, ~0ull >> 4), need, [&](uint64_t n) {
    hipError_t e = dev_alloc(&c->d_F, sizeof(double) * n, c->map_mem);
    if (e != hipSuccess) return e;
    e = dev_alloc(&c->d_T, sizeof(double) * n, c->map_mem);
    if (e != hipSuccess) {
      (void)hipFree(c->d_F);  // never used
      c->d_F = nullptr;
    }
    return e;
  });
  if (!cells) return fail_hip(c, hipErrorOutOfMemory, "staged maps");
  c->cells_cap = cells;
  return DYMU_OK;
}

double* prio_delta(dymu_ctx* c) { return reinterpret_cast<double*>(c->d_prio + 6); }
double* prio_base(dymu_ctx* c, uint64_t q) { return reinterpret_cast<double*>(c->d_prio + 3 + q); }
unsigned long long* prio_minkey(dymu_ctx* c, uint64_t q) { return c->d_prio + q; }
uint32_t* prio_hist(dymu_ctx* c, uint64_t q) { return c->d_hist + q * kShards * kBins; }
unsigned long long* prio_keys(dymu_ctx* c, uint64_t q) {
  return c->d_keys + q * (uint64_t)c->dom.ntiles;
}

int tile_w(int variant) { return variant == 5 ? 16 : kWaveTile; }
int tile_h(int variant) { return variant == 5 ? 16 : kWaveTile; }
bool valid_variant(int v) { return v == 0 || (v >= 3 && v <= 5); }
bool is_prio(int variant) { return variant == 4 || variant == 5; }

// Passes a domain may run beyond max_passes: converge() checks the cap between
// batches of up to 64 launches (converge_pipelined has two such batches queued),
// so epochs up to eb + max_passes + kPassSlack + 2 can be stamped; the epoch-wrap
// guard in dom_begin reserves that many.
constexpr uint64_t kPassSlack = 128;

// Leave the live domain (error paths included): later domains stamp epochs
// above every epoch this one used, so no tile_epoch entry can block them.
void dom_retire(dymu_ctx* c) {
  auto& D = c->dom;
  c->arm_seq = 0;  // a post armed for a pass that will not run
  c->arm_src = nullptr;
  c->arm_dst = nullptr;
  c->arm_ext = nullptr;
  if (!D.live) return;
  c->epoch_base = D.eb + (uint32_t)D.p + 4u;
  D.live = false;
}

// ---- domain primitives (whole grid, or one row slab with ghost rows) ----
// cold = true: T := +inf (incl. ghost rows) and the goal seeded (a fresh solve);
// false: T is kept and the caller seeds list 0 (windowed re-propagation).
// need_keys: the caller needs tile keys (lower bounds on every value the passes can
// still produce, dymu_solve_until_device): the plain FIM kernel 3 has none, kernel 4
// runs instead.
// the pass kernel a domain of nx x nrows cells runs
int dom_variant(const dymu_ctx* c, uint32_t nx, uint32_t nrows, bool need_keys) {
  int variant = c->variant;
  if (variant == 0) {
    const uint64_t t8 = (uint64_t)((nx + kWaveTile - 1) / kWaveTile) *
                        (uint64_t)((nrows + kWaveTile - 1) / kWaveTile);
    variant = t8 >= c->prio_min_tiles ? 5 : 3;
  }
  if (need_keys && !is_prio(variant)) variant = 4;
  if (c->opts.deterministic) variant = 5;
  return variant;
}

int dom_begin(dymu_ctx* c, const double* dF, double* dT, uint32_t nx, uint32_t nrows, uint64_t ld,
              int ghost_lo, int ghost_hi, int64_t gi, int64_t gj, hipStream_t st,
              bool cold = true, bool need_keys = false) {
  if (!dF || !dT || nx == 0 || nrows == 0 || ld < nx) return DYMU_ERR_ARG;
  const int variant = dom_variant(c, nx, nrows, need_keys);
  const int TWd = tile_w(variant), THd = tile_h(variant);
  if (ghost_hi && (nrows % (uint32_t)THd) != 0) return DYMU_ERR_ARG;
  if (gj >= 0 && (gi < 0 || gi >= (int64_t)nx || gj >= (int64_t)nrows)) return DYMU_ERR_ARG;
  const uint32_t ntx = (uint32_t)((nx + TWd - 1) / TWd), nty = (uint32_t)((nrows + THd - 1) / THd);
  const uint64_t ntiles64 = (uint64_t)ntx * nty;
  if (ntiles64 >= (1ull << 31)) return DYMU_ERR_ARG;
  const uint32_t ntiles = (uint32_t)ntiles64;
  dom_retire(c);  // a domain abandoned mid-solve (an error, or no dom_finish)
  int rc = ensure_tiles(c, ntiles, st);
  if (rc) return rc;
  if (is_prio(variant) && (rc = ensure_prio(c, ntiles)) != DYMU_OK) return rc;
  auto& D = c->dom;
  D = dymu_ctx::Dom{};
  D.variant = variant;
  D.ntiles = ntiles;
  D.max_passes = c->opts.max_passes > 0 ? (uint64_t)c->opts.max_passes : 4ull * ntiles + 1024ull;
  if ((uint64_t)c->epoch_base + D.max_passes + kPassSlack + 8 >= 0xFFFFFFF0ull) {
    // the epochs wrap: every stamp of the array, not this domain's ntiles only -- a stamp
    // left beyond them would keep its tile out of every list of a later, larger domain
    HIPC(c, hipMemsetAsync(c->d_tile_epoch, 0, sizeof(uint32_t) * (uint64_t)c->tiles_cap, st));
    c->epoch_base = 0;
  }
  D.eb = c->epoch_base;
  c->epoch_base = D.eb + 4u;  // the seed's epoch stays used even if a step below fails
  const uint64_t lstride = (uint64_t)kShards * ntiles;
  for (int q = 0; q < 3; ++q) {
    D.lists[q] = c->d_lists + q * lstride;
    D.counts[q] = c->d_counts + q * kShards;
  }
  HIPC(c, hipMemsetAsync(c->d_counts, 0, sizeof(uint32_t) * 3 * kShards, st));
  HIPC(c, hipMemsetAsync(c->d_stats, 0, sizeof(unsigned long long) * kShards * kStatSlots, st));
  if (cold)
    HIPC(c, launch_fill_inf(dT, ld, nx, ghost_lo ? -1 : 0, (int64_t)nrows + (ghost_hi ? 1 : 0), st));
  PassArgs& a = D.a;
  if (is_prio(D.variant)) {
    HIPC(c, launch_prio_init(dF, (int64_t)ld, nx, nrows, c->d_keys, 3ull * ntiles, c->d_hist,
                             3ull * kShards * kBins, c->d_prio,
                             reinterpret_cast<double*>(c->d_prio + 3), prio_delta(c), c->prio_kappa,
                             st));
    // kernel 5 relaxes one colour of a checkerboard of tiles per pass (PassArgs::checker):
    // no visit then reads a halo another wave is writing, which cuts the tile visits
    // by a third (16384^2: 36.8 -> 33.8 ms, 4096^2: 5.98 -> 5.48 ms, v23,
    // profiles/r02/checker_sweep.txt).  DYMU_CHECKER=0 disables it.
    bool checker = D.variant == 5;
    if (const char* kv = std::getenv("DYMU_CHECKER")) checker = D.variant == 5 && std::atoi(kv);
    if (c->opts.deterministic) checker = true;
    // default per pass: 64 8x8 tiles per CU (v4) / 16x16 tiles per CU (v5), the measured
    // optima: with the checkerboard 6 / 12 / 14 per CU for whole grids below 2^17 /
    // below 2^20 / from 2^20 tiles (4096^2 / 8192^2 / 16384^2), 10 for slabs (8 without:
    // same pass time in the rehearsal, 6% fewer exchange rounds); without it 4 / 8 / 10
    // (v11, v18: profiles/r02/sweep_v18b.log)
    const bool whole5 = D.variant == 5 && !ghost_lo && !ghost_hi;
    const uint32_t per_cu = D.variant != 5                            ? 64u
                            : !whole5                                  ? (checker ? 10u : 8u)
                            : ntiles < (1u << 17)                      ? (checker ? 6u : 4u)
                            : ntiles >= (1u << 20)                     ? (checker ? 14u : 10u)
                                                                       : (checker ? 12u : 8u);
    a.checker = checker;
    a.target = c->prio_target ? c->prio_target : (uint32_t)c->cu_count * per_cu;
    a.target_frac = c->prio_frac;
    a.prune = c->prune;
    a.delta = prio_delta(c);
  }
  if (cold && gj >= 0) {
    const uint32_t gtile = (uint32_t)(gj / THd) * ntx + (uint32_t)(gi / TWd);
    // the goal's tile and, for the priority kernels, the tiles across the tile edges the
    // goal lies on (SeedTiles)
    SeedTiles gt{{gtile, 0u, 0u}, 1u};
    if (is_prio(D.variant)) {
      if (gi % TWd == 0 && gi > 0) gt.t[gt.n++] = gtile - 1u;
      if (gi % TWd == TWd - 1 && gi + 1 < (int64_t)nx) gt.t[gt.n++] = gtile + 1u;
      if (gj % THd == 0 && gj > 0) gt.t[gt.n++] = gtile - ntx;
      if (gj % THd == THd - 1 && gj + 1 < (int64_t)nrows) gt.t[gt.n++] = gtile + ntx;
    }
    HIPC(c, launch_seed(dT, ld, gi, gj, D.lists[0], D.counts[0], c->d_tile_epoch, D.eb + 1, gt, 1,
                        st));
    if (is_prio(D.variant))
      HIPC(c, launch_prio_seed(c->d_keys, c->d_hist, c->d_prio, gt, 0.0, st));
  }
  // kernel 5 edge columns: +inf (cold) plus the goal's tile; a warm domain
  // (resolve_core) rebuilds them from T once its seeding kernels have run (ec_sync)
  a.ec = nullptr;
  if (D.variant == 5 && c->use_ec) {
    if (c->ec_cap < ntiles) {
      park(c, c->d_ec);
      c->d_ec = nullptr;
      const uint64_t old = c->ec_cap;
      c->ec_cap = 0;
      const uint64_t cap = alloc_grown(grown(ntiles, old, (1ull << 31) - 1), ntiles, [&](uint64_t n) {
        return dev_alloc(&c->d_ec, sizeof(double) * 32 * n, c->ec_mem);
      });
      if (!cap) return fail_hip(c, hipErrorOutOfMemory, "edge columns");
      c->ec_cap = cap;
    }
    a.ec = c->d_ec;
    if (cold) {
      HIPC(c, launch_fill_inf(c->d_ec, 0, 32u * ntiles, 0, 1, st));
      if (gj >= 0) {
        const uint32_t gtile = (uint32_t)(gj / THd) * ntx + (uint32_t)(gi / TWd);
        HIPC(c, launch_ec_rebuild(dT, ld, nx, nrows, c->d_ec, ntx, gtile, gtile + 1, st));
      }
    }
  }
  a.F = dF;
  a.T = dT;
  a.ld = (int64_t)ld;
  a.nx = nx;
  a.ny = nrows;
  a.ntx = (int)ntx;
  {
    const TileDiv td = tile_div(ntx);
    a.ntx_mul = td.mul;
    a.ntx_shift = td.shift;
  }
  a.nty = (int)nty;
  a.ghost_lo = ghost_lo;
  a.ghost_hi = ghost_hi;
  // v5: a sweep cap of 16 bounds the visit (capped tiles re-queue themselves); on large
  // grids a pass is ended by the capped visits of the busiest SIMDs, so there a visit
  // also stops sweeping 14 us into the pass (re-queued like a capped one): 46.0 vs
  // 49.2 ms at 16384^2 (v9), 15.6 vs 16.0 ms at 8192^2 (v11).  Whole grids from 2^18
  // tiles; slabs (more exchange rounds with it) only from 2^20.
  // v33 (13 instead of 16.5 fp64 instructions per update) and the strided entries moved
  // the optimum for those grids to a cap of 18 and a deadline of 15 us: 28.48-28.54 vs
  // 29.90 ms at 16384^2, 1,392 vs 1,562 passes (profiles/r04/v34_knobs.txt)
  const bool big = ntiles >= (1u << 20) || (!ghost_lo && !ghost_hi && ntiles >= (1u << 18));
  a.max_inner = c->opts.max_inner > 0 ? c->opts.max_inner
                : variant == 5            ? (big ? 18 : 16)
                                          : 4 * (TWd + THd);
  if (const char* kv = std::getenv("DYMU_MAX_INNER")) a.max_inner = std::max(1, std::atoi(kv));

  a.sweep_deadline = (variant == 5 && big) ? 1500u : 0u;  // 10-ns s_memrealtime ticks
  if (const char* kv = std::getenv("DYMU_SWEEP_DEADLINE"))
    a.sweep_deadline = (uint32_t)std::max(0, std::atoi(kv));
  // at most 90% of the listed tiles per pass: a short list (the serpentine maze, the first
  // passes of an open grid) is otherwise relaxed whole, and every improvement behind the
  // front re-relaxes the tiles downstream of it; DYMU_PRIO_CAPFRAC=0: off
  a.cap_frac = 0.9f;
  if (const char* kv = std::getenv("DYMU_PRIO_CAPFRAC")) a.cap_frac = (float)std::atof(kv);
  // kernel 5: list entries carry their first-insertion key bin, so a key-deferred entry
  // skips its tile loads (PassArgs::pack_bins); tile indices must fit below the bin field,
  // and deterministic mode's histogram is rebuilt from the current keys instead
  a.pack_bins = variant == 5 && D.ntiles <= kTileMask + 1u && !c->opts.deterministic;
  if (const char* kv = std::getenv("DYMU_PACK_BINS")) a.pack_bins = a.pack_bins && std::atoi(kv);
  a.exact_sqrt = c->opts.exact_sqrt != 0;
  if (const char* kv = std::getenv("DYMU_EXACT_SQRT")) a.exact_sqrt = std::atoi(kv) != 0;
  if (c->opts.deterministic) {
    a.sweep_deadline = 0;  // the deadline makes the schedule timing-dependent
    D.rehist = true;       // and so do the first-insertion keys of the histogram
    HIPC(c, hipMemsetAsync(c->d_hist + (uint64_t)3 * kShards * kBins, 0,
                           sizeof(uint32_t) * 2 * kShards * kBins, st));
  }
  a.shard_cap = ntiles;
  a.tile_epoch = c->d_tile_epoch;
  a.stats = c->d_stats;
  a.goal_tx = gj >= 0 ? (int)(gi / TWd) : 0;
  a.goal_ty = gj >= 0 ? (int)(gj / THd) : 0;
  if (c->pass_stats && D.variant == 5) {
    const size_t bytes = sizeof(uint32_t) * (size_t)kPassStatCap * kShards * kPsWords;
    if (!c->d_pstat) HIPC(c, hipMalloc(&c->d_pstat, bytes));
    HIPC(c, hipMemsetAsync(c->d_pstat, 0, bytes, st));
  }
  // resident workgroups per CU at the kernel's register / LDS budget
  D.blocks = c->opts.grid_blocks > 0 ? c->opts.grid_blocks
                                      : c->cu_count * c->occupancy[D.variant];
  D.live = true;
  return DYMU_OK;
}

template <class A>
auto bind_hist(A& a, uint32_t* hist, int) -> decltype((void)(a.hist = hist)) {
  a.hist = hist;
}
template <class A>
void bind_hist(A&, uint32_t*, long) {}  // PlaneUpdateArgs: list 0 is re-binned, no histogram

// List 0 of the live domain in the argument struct of a seeding kernel (UpdateArgs,
// SeedArgs, PlaneUpdateArgs, MaskSeedArgs): the list, its counters and stamps, the tile
// geometry and, for the priority kernels, the keys and the histogram.  The epoch of list 0
// is eb + 1: dom_launch stamps eb + p + 2 for list p + 1, which pass p fills.
template <class A>
void bind_list0(dymu_ctx* c, A& a) {
  auto& D = c->dom;
  a.list = D.lists[0];
  a.counts = D.counts[0];
  a.shard_cap = D.ntiles;
  a.tile_epoch = c->d_tile_epoch;
  a.epoch = D.eb + 1;
  a.tw = (uint32_t)tile_w(D.variant);
  a.th = (uint32_t)tile_h(D.variant);
  a.ntx = (uint32_t)D.a.ntx;
  a.keys = is_prio(D.variant) ? prio_keys(c, 0) : nullptr;
  bind_hist(a, is_prio(D.variant) ? prio_hist(c, 0) : nullptr, 0);
}

// report_seq != 0: the batch's first pass posts (report_seq, tiles pending) to the mailbox
int dom_launch(dymu_ctx* c, uint64_t K, hipStream_t st, uint32_t report_seq = 0) {
  auto& D = c->dom;
  if (!D.live) return DYMU_ERR_STATE;
  if (D.p + K > D.max_passes + kPassSlack) {  // beyond the epochs dom_begin reserved
    c->last_error = "pass cap reached before convergence";
    dom_retire(c);
    return DYMU_ERR_NOT_CONVERGED;
  }
  PassArgs& a = D.a;
  const bool prof = c->profiling != 0;
  for (uint64_t k = 0; k < K; ++k, ++D.p) {
    const uint64_t p = D.p;
    a.list_in = D.lists[p % 3];
    a.count_in = D.counts[p % 3];
    a.list_out = D.lists[(p + 1) % 3];
    a.count_out = D.counts[(p + 1) % 3];
    a.count_clear = D.counts[(p + 2) % 3];
    a.epoch = D.eb + (uint32_t)p + 2u;
    a.checker_parity = (uint32_t)(p & 1u);
    if (is_prio(D.variant)) {
      a.key_in = prio_keys(c, p % 3);
      a.key_out = prio_keys(c, (p + 1) % 3);
      a.hist_in = prio_hist(c, p % 3);
      a.hist_out = prio_hist(c, (p + 1) % 3);
      a.hist_clear = prio_hist(c, (p + 2) % 3);
      a.minkey_in = prio_minkey(c, p % 3);
      a.minkey_out = prio_minkey(c, (p + 1) % 3);
      a.minkey_clear = prio_minkey(c, (p + 2) % 3);
      a.base_in = prio_base(c, p % 3);
      a.base_out = prio_base(c, (p + 1) % 3);
    }
    if (k == 0 && report_seq) {
      a.report = c->d_mail;
      a.report_seq = report_seq;
    } else if (c->arm_seq) {
      a.report = c->arm_dst ? c->arm_dst : c->d_mail;
      a.report_seq = c->arm_seq;
      a.report_src = c->arm_src;
      a.report_ext = c->arm_ext;
      c->arm_seq = 0;
      c->arm_src = nullptr;
      c->arm_dst = nullptr;
      c->arm_ext = nullptr;
    }
    a.pstat = (c->pass_stats && D.variant == 5 && c->d_pstat)
                  ? c->d_pstat + (p % kPassStatCap) * (uint64_t)kShards * kPsWords
                  : nullptr;
    const bool tr = is_prio(D.variant) && c->prio_trace >= 0 && p == (uint64_t)c->prio_trace;
    if (tr) {
      if (!c->d_trace)
        HIPC(c, hipMalloc(&c->d_trace, sizeof(unsigned long long) * kTracePts * 65536));
      HIPC(c, hipMemsetAsync(c->d_trace, 0, sizeof(unsigned long long) * kTracePts * D.blocks, st));
      a.trace = c->d_trace;
    }
    if (D.rehist) {  // deterministic mode: b* from the list's final keys
      uint32_t* rh = c->d_hist + (uint64_t)3 * kShards * kBins;  // 2 alternating buffers
      uint32_t* mine = rh + (p & 1u) * kShards * kBins;
      uint32_t* next = rh + ((p + 1) & 1u) * kShards * kBins;
      HIPC(c, launch_rehist(a.list_in, a.count_in, a.shard_cap, a.key_in, a.base_in, a.delta,
                            mine, next, st));
      a.hist_in = mine;
    }
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (prof && D.launches % (uint64_t)c->profiling == 0) {
      while (c->prof_ev.size() < D.prof_used + 2) {
        hipEvent_t e;
        HIPC(c, hipEventCreate(&e));
        c->prof_ev.push_back(e);
      }
      e0 = c->prof_ev[D.prof_used];
      e1 = c->prof_ev[D.prof_used + 1];
      D.prof_used += 2;
    }
    HIPC(c, D.variant == 4   ? launch_pass_prio(a, D.blocks, st, e0, e1)
            : D.variant == 5 ? launch_pass_prio16(a, D.blocks, st, e0, e1)
                             : launch_pass_rb(a, D.blocks, st, e0, e1));
    ++D.launches;
    a.report = nullptr;
    a.report_src = nullptr;
    a.report_ext = nullptr;
    if (tr) {
      a.trace = nullptr;
      std::vector<unsigned long long> h((size_t)kTracePts * D.blocks);
      HIPC(c, hipStreamSynchronize(st));
      HIPC(c, hipMemcpy(h.data(), c->d_trace, sizeof(unsigned long long) * h.size(),
                        hipMemcpyDeviceToHost));
      unsigned long long t0 = ~0ull;
      for (int b = 0; b < D.blocks; ++b) t0 = std::min(t0, h[(size_t)b * kTracePts]);
      std::fprintf(stderr, "TRACE pass %llu blocks %d (10ns ticks rel. first start)\n",
                   (unsigned long long)p, D.blocks);
      for (int b = 0; b < D.blocks; ++b) {
        const unsigned long long* t = &h[(size_t)b * kTracePts];
        auto rel = [&](int k) { return t[k] ? (long long)(t[k] - t0) : -1ll; };
        std::fprintf(stderr, "B %d %lld %lld %lld %lld %lld %llu %llu %lld %lld %lld %llu\n", b,
                     rel(0), rel(1), rel(2), rel(3), rel(4), t[5] >> 32, t[5] & 0xffffffffull,
                     rel(6), rel(7), rel(8), t[9]);
      }
    }
    if (is_prio(D.variant) && c->prio_debug && p < (uint64_t)c->prio_debug) {
      unsigned long long pr[8];
      uint32_t h[kShards * kBins], cnt[kShards];
      HIPC(c, hipStreamSynchronize(st));
      HIPC(c, hipMemcpy(pr, c->d_prio, sizeof pr, hipMemcpyDeviceToHost));
      HIPC(c, hipMemcpy(h, prio_hist(c, (p + 1) % 3), sizeof h, hipMemcpyDeviceToHost));
      HIPC(c, hipMemcpy(cnt, D.counts[(p + 1) % 3], sizeof cnt, hipMemcpyDeviceToHost));
      double dd[4];
      std::memcpy(dd, pr + 3, sizeof dd);
      uint32_t n = 0, hs[kBins] = {0};
      for (int q = 0; q < kShards; ++q) n += cnt[q];
      for (int q = 0; q < kShards * kBins; ++q) hs[q % kBins] += h[q];
      double mk[3];
      std::memcpy(mk, pr, sizeof mk);
      std::fprintf(stderr, "pass %llu n_out %u minkey %g %g %g base %g %g %g delta %g hist:",
                   (unsigned long long)p, n, mk[0], mk[1], mk[2], dd[0], dd[1], dd[2], dd[3]);
      for (int b = 0; b < kBins; ++b) if (hs[b]) std::fprintf(stderr, " %d:%u", b, hs[b]);
      std::fprintf(stderr, "\n");
    }
  }
  return DYMU_OK;
}

// tiles queued for the next pass (synchronises the stream)
int dom_pending(dymu_ctx* c, hipStream_t st, uint64_t* out) {
  auto& D = c->dom;
  if (!D.live) return DYMU_ERR_STATE;
  HIPC(c, hipMemcpyAsync(c->h_count, D.counts[D.p % 3], sizeof(uint32_t) * kShards,
                         hipMemcpyDeviceToHost, st));
  HIPC(c, hipStreamSynchronize(st));
  uint64_t pending = 0;
  for (int q = 0; q < kShards; ++q) pending += c->h_count[q];
  *out = pending;
  return DYMU_OK;
}

int dom_merge(dymu_ctx* c, const double* lo, const double* hi, int32_t* d_pending, hipStream_t st) {
  auto& D = c->dom;
  if (!D.live) return DYMU_ERR_STATE;
  if ((lo && !D.a.ghost_lo) || (hi && !D.a.ghost_hi)) return DYMU_ERR_ARG;
  const uint64_t p = D.p;
  if (lo || hi)
    HIPC(c, launch_merge_ghosts(D.a.T, D.a.ld, D.a.nx, D.a.ny, lo, hi, D.a.ntx, D.a.nty,
                                tile_w(D.variant), D.lists[p % 3], D.counts[p % 3], D.ntiles,
                                c->d_tile_epoch, D.eb + (uint32_t)p + 1u,
                                is_prio(D.variant) ? prio_keys(c, p % 3) : nullptr,
                                is_prio(D.variant) ? prio_hist(c, p % 3) : nullptr,
                                is_prio(D.variant) ? prio_minkey(c, p % 3) : nullptr,
                                is_prio(D.variant) ? prio_base(c, p % 3) : nullptr,
                                is_prio(D.variant) ? prio_delta(c) : nullptr, st));
  if (d_pending) HIPC(c, launch_sum_counts(D.counts[p % 3], d_pending, st));
  return DYMU_OK;
}

int dom_exchange(dymu_ctx* c, const double* lo, const double* hi, int32_t* d_total,
                 hipStream_t st) {
  auto& D = c->dom;
  if (!D.live) return DYMU_ERR_STATE;
  if (!d_total || (lo && !D.a.ghost_lo) || (hi && !D.a.ghost_hi)) return DYMU_ERR_ARG;
  const uint64_t p = D.p;
  HIPC(c, launch_exchange(D.a.T, D.a.ld, D.a.nx, D.a.ny, lo, hi, D.a.ntx, D.a.nty,
                          tile_w(D.variant), D.lists[p % 3], D.counts[p % 3], D.ntiles,
                          c->d_tile_epoch, D.eb + (uint32_t)p + 1u,
                          is_prio(D.variant) ? prio_keys(c, p % 3) : nullptr,
                          is_prio(D.variant) ? prio_hist(c, p % 3) : nullptr,
                          is_prio(D.variant) ? prio_minkey(c, p % 3) : nullptr,
                          is_prio(D.variant) ? prio_base(c, p % 3) : nullptr,
                          is_prio(D.variant) ? prio_delta(c) : nullptr, c->d_xchg, d_total, st));
  return DYMU_OK;
}

// One round of the sharded loop with the ghost merge inside the passes (kernel 5,
// K >= 2): the first pass min-merges the rows received after the previous round
// and queues the tiles under improved columns for the second; the second pass
// writes *d_total = tiles queued for the first + for the second pass.  0 on every
// rank is the fixed point: nothing was queued after the previous round, and the
// rows it produced improved no ghost.
bool dom_round_ok(const dymu_ctx* c, uint64_t K) {
  // not in deterministic mode: the in-pass merge writes ghost rows that the same
  // pass's boundary visits may be reading
  return c->dom.live && c->dom.variant == 5 && K >= 2 && !c->opts.deterministic;
}

int dom_round(dymu_ctx* c, uint64_t K, const double* lo, const double* hi, int32_t* d_total,
              hipStream_t st) {
  auto& D = c->dom;
  if (!dom_round_ok(c, K)) return DYMU_ERR_STATE;
  if (!d_total || (lo && !D.a.ghost_lo) || (hi && !D.a.ghost_hi)) return DYMU_ERR_ARG;
  uint32_t* scratch = reinterpret_cast<uint32_t*>(c->d_scratch + kScrRoundTotal);
  D.a.merge_lo = lo;
  D.a.merge_hi = hi;
  D.a.tot_save = scratch;
  int rc = dom_launch(c, 1, st);
  D.a.merge_lo = D.a.merge_hi = nullptr;
  D.a.tot_save = nullptr;
  if (rc) return rc;
  D.a.tot_prev = scratch;
  D.a.tot_out = d_total;
  rc = dom_launch(c, 1, st);
  D.a.tot_prev = nullptr;
  D.a.tot_out = nullptr;
  if (rc) return rc;
  return dom_launch(c, K - 2, st);
}

// The peer round (include/dymu_fim.h dymu_dom_round_peer): dom_round whose first pass
// also pushes the owned boundary rows into the neighbours' receive rows with a tag and
// reads its own receive rows after their tags; the second pass records the status.
int dom_round_peer(dymu_ctx* c, uint64_t K, const dymu_peer_links& L, hipStream_t st) {
  auto& D = c->dom;
  if (!dom_round_ok(c, K)) return DYMU_ERR_STATE;
  if (!L.ctl || (L.recv[0] && !D.a.ghost_lo) || (L.recv[1] && !D.a.ghost_hi)) return DYMU_ERR_ARG;
  for (int s = 0; s < 2; ++s)
    if ((L.recv[s] && !L.recv_tag[s]) || (L.send[s] && (!L.send_tag[s] || !L.last[s])))
      return DYMU_ERR_ARG;
  PeerCtl* pc = static_cast<PeerCtl*>(L.ctl);
  uint32_t* scratch = reinterpret_cast<uint32_t*>(c->d_scratch + kScrRoundTotal);
  PassArgs& a = D.a;
  a.merge_lo = L.recv[0];
  a.merge_hi = L.recv[1];
  for (int s = 0; s < 2; ++s) {
    a.merge_tag[s] = L.recv[s] ? L.recv_tag[s] : nullptr;
    a.push_dst[s] = L.send[s];
    a.push_tag[s] = L.send_tag[s];
    a.push_last[s] = L.last[s];
  }
  a.peer = pc;
  a.tot_save = scratch;
  int rc = dom_launch(c, 1, st);
  a.merge_lo = a.merge_hi = nullptr;
  for (int s = 0; s < 2; ++s) {
    a.merge_tag[s] = nullptr;
    a.push_dst[s] = nullptr;
    a.push_tag[s] = nullptr;
    a.push_last[s] = nullptr;
  }
  a.tot_save = nullptr;
  if (rc) {
    a.peer = nullptr;
    return rc;
  }
  a.tot_prev = scratch;
  a.tot_out = reinterpret_cast<int32_t*>(&pc->pend);
  rc = dom_launch(c, 1, st);
  a.tot_prev = nullptr;
  a.tot_out = nullptr;
  a.peer = nullptr;
  if (rc) return rc;
  return dom_launch(c, K - 2, st);
}

int dom_finish(dymu_ctx* c, hipStream_t st, dymu_stats* stats, double ms) {
  auto& D = c->dom;
  if (!D.live) return DYMU_ERR_STATE;
  dom_retire(c);
  HIPC(c, hipStreamSynchronize(st));
  c->last_launches = D.launches;
  c->last_pass_ms = 0.0;
  c->last_timed = 0;
  if (c->profiling) {
    c->last_timed = D.prof_used / 2;
    for (size_t q = 0; q + 1 < D.prof_used; q += 2) {
      float m = 0.f;
      HIPC(c, hipEventElapsedTime(&m, c->prof_ev[q], c->prof_ev[q + 1]));
      c->last_pass_ms += m;
    }
  }
  if (stats) {
    unsigned long long hs[kShards * kStatSlots];
    HIPC(c, hipMemcpy(hs, c->d_stats, sizeof hs, hipMemcpyDeviceToHost));
    unsigned long long h[kStatSlots] = {0};
    for (int q = 0; q < kShards; ++q)
      for (int k = 0; k < kStatSlots; ++k)
        h[k] = (k == kStatMaxActive) ? std::max(h[k], hs[q * kStatSlots + k])
                                     : h[k] + hs[q * kStatSlots + k];
    std::memset(stats, 0, sizeof *stats);
    stats->passes = h[kStatPasses];
    stats->launches = D.launches;
    stats->tile_visits = h[kStatVisits];
    stats->inner_sweeps = h[kStatSweeps];
    stats->max_active = h[kStatMaxActive];
    stats->deferred = h[kStatDeferred];
    stats->rounds = 0;
    stats->ms = ms;
    stats->tile_w = tile_w(D.variant);
    stats->tile_h = tile_h(D.variant);
    stats->kernel = D.variant;
  }
  return DYMU_OK;
}

// the time from event a to event b, once b has passed
int event_ms(dymu_ctx* c, hipEvent_t a, hipEvent_t b, double* ms) {
  HIPC(c, hipEventSynchronize(b));
  float f = 0.f;
  HIPC(c, hipEventElapsedTime(&f, a, b));
  *ms = (double)f;
  return DYMU_OK;
}

// a dymu_last_*_ms getter: the time between the event pair of the last call of its kind
int elapsed_ms(dymu_ctx* c, bool dymu_ctx::*timed, hipEvent_t dymu_ctx::*ev_a,
               hipEvent_t dymu_ctx::*ev_b, double* ms) {
  if (!c || !ms) return DYMU_ERR_ARG;
  if (!(c->*timed)) return DYMU_ERR_STATE;
  HIPC(c, hipSetDevice(c->device));
  return event_ms(c, c->*ev_a, c->*ev_b, ms);
}

// the getters of a call with four stamps (before init, after it, after the rounds, after
// finalize): the whole call, and its three stages
int total_ms(dymu_ctx* c, bool dymu_ctx::*timed, hipEvent_t (dymu_ctx::*ev)[4], double* ms) {
  if (!c || !ms) return DYMU_ERR_ARG;
  if (!(c->*timed)) return DYMU_ERR_STATE;
  HIPC(c, hipSetDevice(c->device));
  return event_ms(c, (c->*ev)[0], (c->*ev)[3], ms);
}
int stage_ms(dymu_ctx* c, bool dymu_ctx::*timed, hipEvent_t (dymu_ctx::*ev)[4], double out[3]) {
  if (!c || !out) return DYMU_ERR_ARG;
  if (!(c->*timed)) return DYMU_ERR_STATE;
  HIPC(c, hipSetDevice(c->device));
  for (int k = 0; k < 3; ++k) {
    const int rc = event_ms(c, (c->*ev)[k], (c->*ev)[k + 1], &out[k]);
    if (rc) return rc;
  }
  return DYMU_OK;
}

// launch() between the event pair of a dymu_last_*_ms getter (elapsed_ms): the events are
// created on first use, and the flag holds once both are recorded behind the launch
template <class Launch>
int timed_launch(dymu_ctx* c, hipStream_t st, bool dymu_ctx::*timed, hipEvent_t dymu_ctx::*ev_a,
                 hipEvent_t dymu_ctx::*ev_b, Launch launch) {
  if (!(c->*ev_a)) HIPC(c, hipEventCreate(&(c->*ev_a)));
  if (!(c->*ev_b)) HIPC(c, hipEventCreate(&(c->*ev_b)));
  c->*timed = false;
  HIPC(c, hipEventRecord(c->*ev_a, st));
  HIPC(c, launch());
  HIPC(c, hipEventRecord(c->*ev_b, st));
  c->*timed = true;
  return DYMU_OK;
}

// the end of a timed call: ev1 behind the work queued so far, the time since ev0, and the
// live domain's statistics
int finish_timed(dymu_ctx* c, hipStream_t st, dymu_stats* stats) {
  HIPC(c, hipEventRecord(c->ev1, st));
  double ms = 0.0;
  const int rc = event_ms(c, c->ev0, c->ev1, &ms);
  return rc ? rc : dom_finish(c, st, stats, ms);
}

// The host-checked convergence loop (the domain must be live): K passes, queue_test()
// puts the caller's stop test on the stream behind them, dom_pending synchronises, and
// stop(pending) -- with the words the test read back into c->h_probe -- decides.  Then the
// statistics.  Any error retires the domain.
// K: passes_per_check when given; else first_batch passes before the first check, then
// `later` between checks, or doubling up to 64 for later = kDoubling.
// record_ev0 = false: the caller has recorded ev0 before its preparation.
constexpr uint64_t kDoubling = 0;
template <class Queue, class Stop>
int converge_checked(dymu_ctx* c, hipStream_t st, dymu_stats* stats, uint64_t later,
                     bool record_ev0, const char* what, Queue queue_test, Stop stop) {
  if (record_ev0) HIPC(c, hipEventRecord(c->ev0, st));
  const bool fixed = c->opts.passes_per_check > 0;
  uint64_t K = fixed ? (uint64_t)c->opts.passes_per_check : c->first_batch;
  for (;;) {
    int rc = dom_launch(c, K, st);
    if (rc == DYMU_OK) {
      const hipError_t e = queue_test();
      if (e != hipSuccess) rc = fail_hip(c, e, what);
    }
    if (rc == DYMU_OK) {
      uint64_t pending = 0;
      rc = dom_pending(c, st, &pending);
      if (rc == DYMU_OK && stop(pending)) break;
    }
    if (rc == DYMU_OK && c->dom.p >= c->dom.max_passes) {
      c->last_error = "pass cap reached before convergence";
      rc = DYMU_ERR_NOT_CONVERGED;
    }
    if (rc) {
      dom_retire(c);
      return rc;
    }
    if (!fixed) K = later == kDoubling ? std::min<uint64_t>(K * 2, 64) : later;
  }
  return finish_timed(c, st, stats);
}

// passes until no tile is queued, then statistics.
// probe (priority kernels only): also stop as soon as the probe cells are final --
// every queued tile's key exceeds their largest value -- and return that value in
// *t_probe (+inf if a probe cell is unreachable; then the solve runs to the end).
int converge(dymu_ctx* c, hipStream_t st, dymu_stats* stats, const ProbeCells* probe = nullptr,
             double* t_probe = nullptr) {
  auto queue_test = [&]() -> hipError_t {
    if (!probe) return hipSuccess;
    auto& D = c->dom;
    const hipError_t e =
        launch_probe(D.a.T, D.a.ld, *probe, prio_minkey(c, D.p % 3), c->d_scratch + kScrProbe, st);
    if (e != hipSuccess) return e;
    return hipMemcpyAsync(c->h_probe, c->d_scratch + kScrProbe, 2 * sizeof(unsigned long long),
                          hipMemcpyDeviceToHost, st);
  };
  auto stop = [&](uint64_t pending) {
    if (probe) {
      double tmax, kmin;
      std::memcpy(&tmax, &c->h_probe[0], sizeof tmax);
      std::memcpy(&kmin, &c->h_probe[1], sizeof kmin);
      *t_probe = tmax;
      if (kmin > tmax) return true;  // no pass can lower a value <= tmax any more
    }
    return pending == 0;
  };
  return converge_checked(c, st, stats, kDoubling, /*record_ev0=*/true, "start probe", queue_test,
                          stop);
}

// Wait for the mailbox post seq (converge_pipelined, converge_stream).  The host spins on
// the coherent word; once a wait has lasted 20 ms (far beyond any batch) it asks
// every 5 ms whether the stream has drained, so a faulted or stopped stream ends
// the wait with an error instead of a hang.  (Not earlier: a query of a busy
// stream is not free.)
// Posts carry increasing sequence numbers; this returns the first one seen at or
// after seq (its number in *seen when seen is given).
int wait_mail(dymu_ctx* c, hipStream_t st, uint32_t seq, uint32_t* pending,
              uint32_t* seen = nullptr, double timeout_s = 0.0) {
  auto arrived = [&](unsigned long long v) {
    if ((int32_t)((uint32_t)(v >> 32) - seq) < 0) return false;
    *pending = (uint32_t)v;
    if (seen) *seen = (uint32_t)(v >> 32);
    return true;
  };
  using clk = std::chrono::steady_clock;
  const clk::time_point t0 = clk::now();
  clk::time_point next_query = t0 + std::chrono::milliseconds(20);
  for (uint64_t spin = 1;; ++spin) {
    if (arrived(__atomic_load_n(c->h_mail, __ATOMIC_ACQUIRE))) return DYMU_OK;
    if ((spin & 255) == 0 && clk::now() >= next_query) {
      next_query += std::chrono::milliseconds(5);
      if (timeout_s > 0.0 &&
          std::chrono::duration<double>(clk::now() - t0).count() > timeout_s) {
        c->last_error = "convergence mailbox: timed out waiting for a post";
        return DYMU_ERR_HIP;
      }
      const hipError_t e = hipStreamQuery(st);
      if (e == hipSuccess) {  // drained: the post, if made, is visible now
        if (arrived(__atomic_load_n(c->h_mail, __ATOMIC_ACQUIRE))) return DYMU_OK;
        c->last_error = "convergence mailbox: batch report missing";
        return DYMU_ERR_HIP;
      }
      if (e != hipErrorNotReady) return fail_hip(c, e, "hipStreamQuery");
    }
#if defined(__x86_64__)
    __builtin_ia32_pause();
#endif
  }
}

// converge() without host round trips between batches: batch b+1 is queued before
// the host learns batch b's outcome, which batch b+1's first pass posts to the
// mailbox as it starts -- the GPU never waits for the host, and the batch queued
// behind the converged one runs as empty passes (~3 us each).  Results are those of
// converge(): every pass after convergence finds no tile queued and changes nothing.
int converge_pipelined(dymu_ctx* c, hipStream_t st, dymu_stats* stats) {
  HIPC(c, hipEventRecord(c->ev0, st));
  auto& D = c->dom;
  uint64_t K = c->first_batch;
  int rc = dom_launch(c, K, st);
  while (rc == DYMU_OK) {
    const uint64_t done = D.p;  // passes whose outcome the next post reports
    K = std::min<uint64_t>(K * 2, c->max_batch);
    if (++c->mail_seq == 0) c->mail_seq = 1;
    const uint32_t seq = c->mail_seq;
    rc = dom_launch(c, K, st, seq);
    uint32_t pending = 0;
    if (rc == DYMU_OK) rc = wait_mail(c, st, seq, &pending);
    if (rc == DYMU_OK && pending == 0) break;
    if (rc == DYMU_OK && done >= D.max_passes) {
      c->last_error = "pass cap reached before convergence";
      rc = DYMU_ERR_NOT_CONVERGED;
    }
  }
  if (rc) {
    dom_retire(c);
    (void)hipStreamSynchronize(st);
    return rc;
  }
  return finish_timed(c, st, stats);
}

// Streaming variant (DYMU_PIPELINE=2): every pass posts, and the host keeps
// c->max_batch passes queued ahead of the one running -- the overshoot after
// convergence is at most that many passes.
// probe (priority kernels): the passes also post whether the probe cells are final
// (PassArgs::probe); the loop stops at the first such post, and *t_probe gets their
// largest value (+inf if one is unreachable: then the solve runs to the end).  The
// <= 4 passes queued behind that post only lower values above *t_probe (every key
// exceeds it), so the cells <= *t_probe are exactly those of converge()'s exit.
int converge_stream(dymu_ctx* c, hipStream_t st, dymu_stats* stats,
                    const ProbeCells* probe = nullptr, double* t_probe = nullptr) {
  HIPC(c, hipEventRecord(c->ev0, st));
  auto& D = c->dom;
  if (probe) D.a.probe = *probe;
  const uint64_t ahead = c->max_batch;
  const uint32_t base = c->mail_seq + 1;  // pass p posts base + p
  auto post_seq = [&](uint64_t p) { uint32_t s = base + (uint32_t)p; return s ? s : 1u; };
  int rc = DYMU_OK;
  for (uint64_t k = 0; k < ahead && rc == DYMU_OK; ++k) rc = dom_launch(c, 1, st, post_seq(D.p));
  uint64_t running = 0;  // pass whose post the host waits for
  while (rc == DYMU_OK) {
    uint32_t pending = 0, seen = 0;
    rc = wait_mail(c, st, post_seq(running), &pending, &seen);
    if (rc) break;
    running = (uint64_t)(uint32_t)(seen - base);
    if ((pending & 0x7FFFFFFFu) == 0 || (pending & 0x80000000u)) break;
    if (running > D.max_passes) {
      c->last_error = "pass cap reached before convergence";
      rc = DYMU_ERR_NOT_CONVERGED;
      break;
    }
    while (rc == DYMU_OK && D.p < running + 1 + ahead) rc = dom_launch(c, 1, st, post_seq(D.p));
    ++running;
  }
  c->mail_seq = base + (uint32_t)D.p + 1;
  D.a.probe.n = 0;
  if (rc) {
    dom_retire(c);
    (void)hipStreamSynchronize(st);
    return rc;
  }
  HIPC(c, hipEventRecord(c->ev1, st));
  if (probe) {
    HIPC(c, launch_probe(D.a.T, D.a.ld, *probe, nullptr, c->d_scratch + kScrProbe, st));
    HIPC(c, hipMemcpyAsync(c->h_probe, c->d_scratch + kScrProbe, 2 * sizeof(unsigned long long),
                           hipMemcpyDeviceToHost, st));
  }
  HIPC(c, hipEventSynchronize(c->ev1));
  HIPC(c, hipStreamSynchronize(st));
  if (probe) std::memcpy(t_probe, &c->h_probe[0], sizeof(double));
  float ms = 0.f;
  HIPC(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
  return dom_finish(c, st, stats, ms);
}

int converge_auto(dymu_ctx* c, hipStream_t st, dymu_stats* stats) {
  if (c->stepping) {  // the caller drives the live domain (dymu_set_stepping)
    HIPC(c, hipStreamSynchronize(st));
    return DYMU_OK;
  }
  if (c->pipeline == 2 && c->d_mail && c->opts.passes_per_check <= 0)
    return converge_stream(c, st, stats);
  if (c->pipeline && c->d_mail && c->opts.passes_per_check <= 0)
    return converge_pipelined(c, st, stats);
  return converge(c, st, stats);
}

int solve_core(dymu_ctx* c, const double* dF, double* dT, uint32_t nx, uint32_t ny, uint64_t ld,
               uint32_t gi, uint32_t gj, hipStream_t st, dymu_stats* stats) {
  if (gi >= nx || gj >= ny) return DYMU_ERR_ARG;
  int rc = dom_begin(c, dF, dT, nx, ny, ld, 0, 0, gi, gj, st);
  if (rc) return rc;
  return converge_auto(c, st, stats);
}

// The start cell and its in-grid 4-neighbours (isFullyClosedNode, :424-436).
ProbeCells start_probe(uint32_t nx, uint32_t ny, uint32_t si, uint32_t sj) {
  ProbeCells p{};
  auto add = [&](int64_t i, int64_t j) {
    if (i >= 0 && j >= 0 && i < (int64_t)nx && j < (int64_t)ny) {
      p.ij[p.n][0] = i;
      p.ij[p.n][1] = j;
      ++p.n;
    }
  };
  add(si, sj);
  add(si, (int64_t)sj - 1);
  add((int64_t)si - 1, sj);
  add((int64_t)si + 1, sj);
  add(si, (int64_t)sj + 1);
  return p;
}

int solve_until_core(dymu_ctx* c, const double* dF, double* dT, uint32_t nx, uint32_t ny,
                     uint64_t ld, uint32_t gi, uint32_t gj, uint32_t si, uint32_t sj,
                     hipStream_t st, double* t_closed, dymu_stats* stats) {
  if (gi >= nx || gj >= ny || si >= nx || sj >= ny || !t_closed) return DYMU_ERR_ARG;
  if (c->stepping) return DYMU_ERR_STATE;
  int rc = dom_begin(c, dF, dT, nx, ny, ld, 0, 0, gi, gj, st, true, /*need_keys=*/true);
  if (rc) return rc;
  const ProbeCells p = start_probe(nx, ny, si, sj);
  *t_closed = __builtin_inf();
  if (c->pipeline == 2 && c->d_mail && c->opts.passes_per_check <= 0)
    return converge_stream(c, st, stats, &p, t_closed);
  return converge(c, st, stats, &p, t_closed);
}

// The raise front (k_raise) on the live domain's map, its lists as plain lists
// of 16x16 tiles whatever the pass kernel's tile is (no keys, no histogram: the front has no
// order), stamps from eb + 1 on: from the tiles that meet the cells [win[0], win[2]) x
// [win[1], win[3]) until a pass queues nothing -- 4 passes, then doubling up to 64, between
// reads of the pending count.  The caller sets ra.F and ra.gi, ra.gj, or with seeded
// (k_raise<true>) the mask and ra.c.  The scratch words at stats_slot take [visits, cells],
// c->last_update[0..2] the passes and those two -- filled here, so they stand even if a later
// step of the caller (the clearance edit's box read-back) fails.  Any error retires the domain.
int run_raise(dymu_ctx* c, RaiseArgs ra, bool seeded, ScratchSlot stats_slot,
              const uint32_t win[4], hipStream_t st) {
  auto& D = c->dom;
  auto fail = [&](int rc) { return dom_retire(c), rc; };
  ra.T = D.a.T;
  ra.ld = D.a.ld;
  ra.nx = D.a.nx, ra.ny = D.a.ny;
  ra.ntx = (ra.nx + 15u) / 16u, ra.nty = (ra.ny + 15u) / 16u;
  ra.shard_cap = D.ntiles;
  ra.tile_epoch = c->d_tile_epoch;
  ra.tol = 1e-13;
  ra.stats = c->d_scratch + stats_slot;
  const int blocks = c->cu_count * 2;
  UpdateArgs u{};
  bind_list0(c, u);
  u.tw = u.th = 16, u.ntx = ra.ntx;
  u.keys = nullptr, u.hist = nullptr;
  hipError_t e = launch_seed_window(u, win[0], win[1], win[2], win[3], st);
  if (e == hipSuccess) e = hipMemsetAsync(ra.stats, 0, 2 * sizeof(unsigned long long), st);
  if (e != hipSuccess) return fail(fail_hip(c, e, "raise seeding"));
  uint64_t pending = 1, passes = 0;
  for (uint64_t K = 4; pending; K = std::min<uint64_t>(K * 2, 64)) {
    for (uint64_t k = 0; k < K; ++k, ++D.p, ++passes) {
      const uint64_t p = D.p;
      if (p > D.max_passes) {
        c->last_error = "raise: pass cap reached";
        return fail(DYMU_ERR_NOT_CONVERGED);
      }
      ra.list_in = D.lists[p % 3];
      ra.count_in = D.counts[p % 3];
      ra.list_out = D.lists[(p + 1) % 3];
      ra.count_out = D.counts[(p + 1) % 3];
      ra.count_clear = D.counts[(p + 2) % 3];
      ra.epoch = D.eb + (uint32_t)p + 2u;
      e = seeded ? launch_raise_seeded(ra, blocks, st) : launch_raise(ra, blocks, st);
      if (e != hipSuccess) return fail(fail_hip(c, e, "raise pass"));
    }
    if (const int rc = dom_pending(c, st, &pending)) return fail(rc);
  }
  unsigned long long hr[2];
  e = hipMemcpy(hr, ra.stats, sizeof hr, hipMemcpyDeviceToHost);
  if (e != hipSuccess) return fail(fail_hip(c, e, "raise statistics"));
  c->last_update[0] = passes;
  c->last_update[1] = hr[0];
  c->last_update[2] = hr[1];
  return DYMU_OK;
}

// Windowed re-propagation (update_kernels.hip): dT holds the converged map of
// the previous speed, dF the new speed, which differs only inside the window.
// decrease_only: the caller guarantees no speed in the window went up; then the
// old map is kept whole and only the window's tiles are seeded (k_seed_window).
// Otherwise (c->raise, default) the raise front invalidates the dependency cone of
// the window (k_raise passes) and the FIM re-solves the cone from
// its boundary plus the window when c->raise (DYMU_RAISE=1); by default every cell
// at or above theta is reset instead (k_reset_seed): a larger region, but one the
// FIM fills in key order from a single level set, where the cone is filled from
// its whole lateral boundary -- 4.1 ms / 192 K visits vs 9.5 ms (252 raise passes +
// 163 K visits) for config 5 at 4096^2.
int resolve_core(dymu_ctx* c, const double* dF, double* dT, uint32_t nx, uint32_t ny, uint64_t ld,
                 uint32_t gi, uint32_t gj, uint32_t i0, uint32_t j0, uint32_t w, uint32_t h,
                 hipStream_t st, dymu_stats* stats, bool decrease_only = false) {
  if (gi >= nx || gj >= ny || w == 0 || h == 0 || i0 >= nx || j0 >= ny) return DYMU_ERR_ARG;
  std::memset(c->last_update, 0, sizeof c->last_update);
  int rc = dom_begin(c, dF, dT, nx, ny, ld, 0, 0, -1, -1, st, /*cold=*/false);
  if (rc) return rc;
  auto& D = c->dom;
  // theta = min old T over the window plus its 1-cell ring (clipped)
  const uint32_t wi0 = i0 > 0 ? i0 - 1 : 0, wj0 = j0 > 0 ? j0 - 1 : 0;
  const uint32_t wi1 = (uint32_t)std::min<uint64_t>((uint64_t)i0 + w + 1, nx);
  const uint32_t wj1 = (uint32_t)std::min<uint64_t>((uint64_t)j0 + h + 1, ny);
  unsigned long long* theta = c->d_scratch + kScrTheta;
  HIPC(c, launch_store_u64(theta, 0x7FF0000000000000ull, st));  // +inf bits
  HIPC(c, launch_window_min(dT, (int64_t)ld, wi0, wj0, wi1, wj1, theta, st));
  UpdateArgs u{};
  u.T = dT;
  u.F = dF;
  u.ld = (int64_t)ld;
  u.nx = nx;
  u.ny = ny;
  u.gi = gi;
  u.gj = gj;
  u.theta_bits = theta;
  const bool raise = !decrease_only && c->raise;
  if (raise) {
    RaiseArgs ra{};
    ra.F = dF;
    ra.gi = gi;
    ra.gj = gj;
    const uint32_t win[4] = {i0, j0, i0 + w, j0 + h};
    rc = run_raise(c, ra, /*seeded=*/false, kScrRaiseStats, win, st);
    if (rc) return rc;
    // a fresh domain for the re-solve: epochs above every raise epoch (dom_retire)
    rc = dom_begin(c, dF, dT, nx, ny, ld, 0, 0, -1, -1, st, /*cold=*/false);
    if (rc) return rc;
  }
  bind_list0(c, u);
  if (raise) {  // the cone's boundary, then the window (decreases inside it)
    uint32_t* hist0 = u.hist;
    u.hist = nullptr;  // binned below from the final keys (they differ per tile)
    HIPC(c, launch_cone_seed(u, theta, st));
    HIPC(c, launch_seed_window(u, i0, j0, i0 + w, j0 + h, st));
    if (is_prio(D.variant)) {
      HIPC(c, launch_theta_state(theta, prio_minkey(c, 0), prio_base(c, 0), st));
      // list 0's histogram from its keys (origin theta', the smallest boundary value):
      // the first passes then relax the boundary tiles in key order, not all at once
      HIPC(c, launch_rehist(D.lists[0], D.counts[0], D.ntiles, prio_keys(c, 0), prio_base(c, 0),
                            prio_delta(c), hist0, c->d_hist + (uint64_t)4 * kShards * kBins, st));
    }
    if (D.a.ec)
      HIPC(c, launch_ec_rebuild(dT, ld, nx, ny, D.a.ec, (uint32_t)D.a.ntx, 0, D.ntiles, st));
    return converge_auto(c, st, stats);
  } else if (decrease_only) {
    HIPC(c, launch_seed_window(u, i0, j0, i0 + w, j0 + h, st));
  } else {
    HIPC(c, launch_reset_seed(u, st));
  }
  if (is_prio(D.variant))
    HIPC(c, launch_theta_state(theta, prio_minkey(c, 0), prio_base(c, 0), st));
  if (D.a.ec)  // the reset kernel wrote T
    HIPC(c, launch_ec_rebuild(dT, ld, nx, ny, D.a.ec, (uint32_t)D.a.ntx, 0, D.ntiles, st));
  return converge_auto(c, st, stats);
}

// ---- early exit on target cells (batch_kernels.hip) ----
static_assert(sizeof(dymu_batch_cell) == sizeof(ProbeTarget) &&
                  offsetof(dymu_batch_cell, j) == offsetof(ProbeTarget, j),
              "dymu_batch_cell is ProbeTarget");
// The targets of one call: tg (host, sorted by plane, each inside its plane) on a stack of
// `planes` maps of ny rows at a plane pitch of P rows (one plain map: planes = 1, P = ny).
struct UntilTargets {
  const ProbeTarget* tg;
  uint32_t n, ny, planes, P;
  double* t_closed;  // required
  double* t_plane;   // host [planes], or null
};

// converge() with the stop test over a target list: K passes, the probe (its words zeroed
// by a fill kernel first), two words read back, compare.  The solve ends at the first check
// at which every queued tile's key exceeds the largest value among the counting targets
// (then no pass can lower a value at or below it any more), or with nothing queued.
// K: passes_per_check when given, else first_batch passes before the first check and
// until_batch between the later ones -- no doubling to 64: the passes run behind the
// deciding one are the overshoot this entry exists to avoid.
int converge_targets(dymu_ctx* c, hipStream_t st, dymu_stats* stats, const UntilTargets& u,
                     const ProbeTarget* d_tg) {
  HIPC(c, hipEventRecord(c->ev0, st));
  const bool fixed = c->opts.passes_per_check > 0;
  uint64_t K = fixed ? (uint64_t)c->opts.passes_per_check : c->first_batch;
  const uint32_t words = u.planes + 2u;
  double tmax = __builtin_inf();
  for (;;) {
    int rc = dom_launch(c, K, st);
    if (rc == DYMU_OK) {
      auto& D = c->dom;
      hipError_t e = launch_fill_u64(c->d_until, words, 0ull, st);
      if (e == hipSuccess)
        e = launch_probe_targets(D.a.F, D.a.T, (uint64_t)D.a.ld, D.a.nx, u.ny, u.planes, u.P, d_tg,
                                 u.n, prio_minkey(c, D.p % 3), c->d_until, st);
      if (e == hipSuccess)
        e = hipMemcpyAsync(c->h_probe, c->d_until, 2 * sizeof(unsigned long long),
                           hipMemcpyDeviceToHost, st);
      if (e != hipSuccess) rc = fail_hip(c, e, "target probe");
    }
    if (rc == DYMU_OK) {
      uint64_t pending = 0;
      rc = dom_pending(c, st, &pending);  // synchronises: the probe words are here too
      if (rc == DYMU_OK) {
        double kmin;
        std::memcpy(&tmax, &c->h_probe[0], sizeof tmax);
        std::memcpy(&kmin, &c->h_probe[1], sizeof kmin);
        if (kmin > tmax || pending == 0) break;
      }
    }
    if (rc == DYMU_OK && c->dom.p >= c->dom.max_passes) {
      c->last_error = "pass cap reached before convergence";
      rc = DYMU_ERR_NOT_CONVERGED;
    }
    if (rc) {
      dom_retire(c);
      return rc;
    }
    if (!fixed) K = c->until_batch;
  }
  HIPC(c, hipEventRecord(c->ev1, st));
  HIPC(c, hipEventSynchronize(c->ev1));
  float ms = 0.f;
  HIPC(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
  *u.t_closed = tmax;
  if (u.t_plane) {  // the words of the last probe; the stream is idle
    std::vector<unsigned long long> h(u.planes);
    HIPC(c, hipMemcpy(h.data(), c->d_until + 2, sizeof(unsigned long long) * u.planes,
                      hipMemcpyDeviceToHost));
    std::memcpy(u.t_plane, h.data(), sizeof(double) * u.planes);
  }
  return dom_finish(c, st, stats, ms);
}

// ---- goal sets (goal_kernels.hip) ----
static_assert(sizeof(dymu_seed) == sizeof(GoalSeed) && offsetof(dymu_seed, t0) == offsetof(GoalSeed, t0),
              "dymu_seed is GoalSeed");
constexpr uint32_t kLabelRounds = 64;  // pointer-jumping rounds: ~log2 of the longest chain

// The seeds checked and copied into the pinned transfer buffer, where the kernels read
// them in place (ensure_xfer; the stream is drained first); *tmin = the smallest t0.
// t0 + 0.0 turns a -0.0 into +0.0, so that the values' bit patterns order like them.
// extra: bytes reserved behind the seeds in the same buffer (a second ensure_xfer could
// move it under the first, s5.8).
int stage_seeds(dymu_ctx* c, uint32_t nx, uint32_t ny, const dymu_seed* seeds, uint32_t n,
                hipStream_t st, const GoalSeed** d_seeds, double* tmin, uint64_t extra = 0) {
  if (!seeds || n == 0 || n >= (1u << 31)) return DYMU_ERR_ARG;
  double m = __builtin_inf();
  for (uint32_t k = 0; k < n; ++k) {
    const dymu_seed& s = seeds[k];
    if (s.i >= nx || s.j >= ny || !(s.t0 >= 0.0) || !(s.t0 < __builtin_inf())) return DYMU_ERR_ARG;
    m = std::min(m, s.t0);
  }
  HIPC(c, hipStreamSynchronize(st));  // no earlier kernel still uses the transfer buffer
  int rc = ensure_xfer(c, sizeof(GoalSeed) * (uint64_t)n + extra);
  if (rc) return rc;
  GoalSeed* h = static_cast<GoalSeed*>(c->h_xfer);
  for (uint32_t k = 0; k < n; ++k) h[k] = GoalSeed{seeds[k].i, seeds[k].j, seeds[k].t0 + 0.0};
  *d_seeds = static_cast<const GoalSeed*>(c->d_xfer);
  if (tmin) *tmin = m + 0.0;
  return DYMU_OK;
}

// A cold domain without a goal, every seed min-written into T and its tile queued in
// list 0 (priority kernels: key = the tile's smallest seed value, binned against
// base = min t0), then the unchanged passes to convergence.
// until: the early exit on target cells (s5.9) -- the targets staged behind the seeds, a
// priority kernel whatever the options say (need_keys), and converge_targets' stop test.
int solve_seeds_core(dymu_ctx* c, const double* dF, double* dT, uint32_t nx, uint32_t ny,
                     uint64_t ld, const dymu_seed* seeds, uint32_t n, hipStream_t st,
                     dymu_stats* stats, const UntilTargets* until = nullptr) {
  if (!dF || !dT || nx == 0 || ny == 0 || ld < nx) return DYMU_ERR_ARG;
  if (until && c->stepping) return DYMU_ERR_STATE;
  const GoalSeed* d_seeds = nullptr;
  double tmin = 0.0;
  const uint64_t tg_bytes = until ? sizeof(ProbeTarget) * (uint64_t)until->n : 0;
  int rc = stage_seeds(c, nx, ny, seeds, n, st, &d_seeds, &tmin, tg_bytes);
  if (rc) return rc;
  const ProbeTarget* d_tg = nullptr;
  if (until) {
    const uint64_t off = sizeof(GoalSeed) * (uint64_t)n;  // a multiple of 16
    std::memcpy(static_cast<char*>(c->h_xfer) + off, until->tg, (size_t)tg_bytes);
    d_tg = reinterpret_cast<const ProbeTarget*>(static_cast<const char*>(c->d_xfer) + off);
    if (c->until_cap < until->planes + 2u) {
      if (c->d_until) (void)hipFree(c->d_until);
      c->d_until = nullptr;
      c->until_cap = 0;
      HIPC(c, hipMalloc(&c->d_until, sizeof(unsigned long long) * ((uint64_t)until->planes + 2)));
      c->until_cap = until->planes + 2u;
    }
  }
  rc = dom_begin(c, dF, dT, nx, ny, ld, 0, 0, -1, -1, st, true, /*need_keys=*/until != nullptr);
  if (rc) return rc;
  auto& D = c->dom;
  SeedArgs a{};
  a.seeds = d_seeds;
  a.n = n;
  a.T = dT;
  a.ld = (int64_t)ld;
  a.nx = nx;
  a.ny = ny;
  a.tw = (uint32_t)tile_w(D.variant);
  a.th = (uint32_t)tile_h(D.variant);
  a.ntx = (uint32_t)D.a.ntx;
  a.list = D.lists[0];
  a.counts = D.counts[0];
  a.shard_cap = D.ntiles;
  a.tile_epoch = c->d_tile_epoch;
  a.epoch = D.eb + 1;  // the epoch of list 0 (dom_launch: eb + p + 2 for list p + 1)
  a.ec = D.a.ec;       // +inf after the cold dom_begin: the seeds on a tile's edge columns
  hipError_t e = hipSuccess;
  if (is_prio(D.variant)) {
    a.keys = prio_keys(c, 0);
    a.hist = prio_hist(c, 0);
    a.base = prio_base(c, 0);
    a.delta = prio_delta(c);
    unsigned long long tb;
    std::memcpy(&tb, &tmin, sizeof tb);
    e = launch_store_u64(prio_minkey(c, 0), tb, st);
    if (e == hipSuccess)
      e = launch_store_u64(reinterpret_cast<unsigned long long*>(prio_base(c, 0)), tb, st);
  }
  if (e == hipSuccess) e = launch_seed_goals(a, st);
  if (e != hipSuccess) {
    dom_retire(c);
    return fail_hip(c, e, "goal seeding");
  }
  if (until) return converge_targets(c, st, stats, *until, d_tg);
  return converge_auto(c, st, stats);
}

// ---- windowed re-propagation of seeded maps and stacks ----
// dT: `planes` converged maps of nx x ny cells at a plane pitch of P rows (one plain map:
// planes = 1, P = ny) under the old speed; dF: the new speed, changed only inside
// `wins` (plane-local, clipped, checked by the callers like the seeds, which are on
// stacked rows).  theta per plane, the reset with the seeds min-written back (or, for
// decrease_only, the windows' tiles), list 0 keyed by its plane's theta and binned from
// those keys, then the unchanged passes.  Seeds and windows share ONE reservation of
// the pinned transfer buffer: a second ensure_xfer may move it under the first.
int update_planes_core(dymu_ctx* c, const double* dF, double* dT, uint32_t nx, uint32_t ny,
                       uint32_t planes, uint32_t P, uint64_t ld, const dymu_seed* seeds,
                       uint32_t n_seeds, const BatchWindow* wins, uint32_t n_wins,
                       bool decrease_only, hipStream_t st, dymu_stats* stats) {
  std::memset(c->last_update, 0, sizeof c->last_update);
  const uint32_t rows = planes * P;  // fits (callers)
  const uint64_t seed_bytes = sizeof(GoalSeed) * (uint64_t)n_seeds;
  const GoalSeed* d_seeds = nullptr;  // on stacked rows, checked by the callers already
  int rc = stage_seeds(c, nx, rows, seeds, n_seeds, st, &d_seeds, nullptr,
                       sizeof(BatchWindow) * (uint64_t)n_wins);
  if (rc) return rc;
  std::memcpy(static_cast<char*>(c->h_xfer) + seed_bytes, wins, sizeof(BatchWindow) * (size_t)n_wins);
  const BatchWindow* d_wins =
      reinterpret_cast<const BatchWindow*>(static_cast<const char*>(c->d_xfer) + seed_bytes);
  uint64_t max_cells = 0;
  for (uint32_t k = 0; k < n_wins; ++k)
    max_cells = std::max<uint64_t>(
        max_cells, (uint64_t)(wins[k].i1 - wins[k].i0 + 2) * (wins[k].j1 - wins[k].j0 + 2));
  if (c->theta_cap < planes) {
    if (c->d_theta) (void)hipFree(c->d_theta);
    c->d_theta = nullptr;
    c->theta_cap = 0;
    HIPC(c, hipMalloc(&c->d_theta, sizeof(unsigned long long) * (uint64_t)planes));
    c->theta_cap = planes;
  }
  rc = dom_begin(c, dF, dT, nx, rows, ld, 0, 0, -1, -1, st, /*cold=*/false);
  if (rc) return rc;
  auto& D = c->dom;
  unsigned long long* n_reset = c->d_scratch + kScrReset;
  PlaneUpdateArgs u{};
  u.T = dT;
  u.F = dF;
  u.ld = (int64_t)ld;
  u.nx = nx;
  u.ny = ny;
  u.P = P;
  u.rows = rows;
  u.theta = c->d_theta;
  u.win = d_wins;
  u.n_win = n_wins;
  bind_list0(c, u);
  u.n_reset = n_reset;
  hipError_t e = launch_fill_u64(c->d_theta, planes, 0x7FF0000000000000ull, st);  // +inf bits
  if (e == hipSuccess) e = launch_store_u64(n_reset, 0ull, st);
  if (e == hipSuccess)
    e = launch_windows_min(dT, (int64_t)ld, nx, ny, P, d_wins, n_wins, max_cells, c->d_theta, st);
  if (e == hipSuccess && decrease_only) e = launch_seed_windows(u, max_cells, st);
  if (e == hipSuccess && !decrease_only) {
    e = launch_reset_planes(u, st);
    SeedArgs a{};  // the seeds back at their t0, their tiles queued (key: min t0 in the tile)
    a.seeds = d_seeds;
    a.n = n_seeds;
    a.T = dT;
    a.ld = (int64_t)ld;
    a.nx = nx;
    a.ny = rows;
    bind_list0(c, a);
    a.hist = nullptr;  // no histogram here: list 0 is binned below, the edge columns rebuilt
    if (e == hipSuccess) e = launch_seed_goals(a, st);
  }
  if (e == hipSuccess && is_prio(D.variant)) {
    // the keys differ between planes: list 0's histogram from its final keys against
    // base = the smallest theta, as the pass that reads it classifies its tiles
    e = launch_theta_min_state(c->d_theta, planes, prio_minkey(c, 0), prio_base(c, 0), st);
    if (e == hipSuccess)
      e = launch_rehist(D.lists[0], D.counts[0], D.ntiles, prio_keys(c, 0), prio_base(c, 0),
                        prio_delta(c), prio_hist(c, 0), c->d_hist + (uint64_t)4 * kShards * kBins,
                        st);
  }
  if (e == hipSuccess && D.a.ec)  // the reset and the seeds wrote T
    e = launch_ec_rebuild(dT, ld, nx, rows, D.a.ec, (uint32_t)D.a.ntx, 0, D.ntiles, st);
  if (e != hipSuccess) {
    dom_retire(c);
    return fail_hip(c, e, "windowed update seeding");
  }
  rc = converge_auto(c, st, stats);
  if (rc) return rc;
  if (!decrease_only) {
    unsigned long long h = 0;
    HIPC(c, hipMemcpyAsync(&h, n_reset, sizeof h, hipMemcpyDeviceToHost, st));
    HIPC(c, hipStreamSynchronize(st));
    c->last_update[2] = h;
  }
  return DYMU_OK;
}

// a window clipped to [0, nx) x [0, ny) (64-bit sums); false: an empty or off-grid one
bool clip_window(uint32_t plane, uint32_t i0, uint32_t j0, uint32_t w, uint32_t h, uint32_t nx,
                 uint32_t ny, BatchWindow* out) {
  if (w == 0 || h == 0 || i0 >= nx || j0 >= ny) return false;
  *out = BatchWindow{plane, i0, j0, (uint32_t)std::min<uint64_t>((uint64_t)i0 + w, nx),
                     (uint32_t)std::min<uint64_t>((uint64_t)j0 + h, ny), 0u};
  return true;
}

// The rounds of a pointer doubling (goal labels, route fields, route usage): launch_round(r)
// queues round r, which adds to d_cnt[r] the entries it left open.  Rounds in batches of 4
// between read-backs of the counters; a round launched behind the one that closed the last
// entry returns at once.  *launched: the rounds queued; *done: the rounds up to the first
// that left nothing open, 0 if `cap` rounds did not get there (the caller's error).
template <class Launch>
int doubling_rounds(dymu_ctx* c, hipStream_t st, const uint32_t* d_cnt, uint32_t cap,
                    Launch launch_round, uint32_t* launched, uint32_t* done) {
  uint32_t h_cnt[std::max(kLabelRounds, kRouteRounds)];
  if (cap > sizeof h_cnt / sizeof h_cnt[0]) return DYMU_ERR_ARG;
  uint32_t& n = *launched;
  for (n = *done = 0; *done == 0 && n < cap;) {
    const uint32_t r0 = n;
    for (uint32_t k = 0; k < 4 && n < cap; ++k, ++n) HIPC(c, launch_round(n));
    HIPC(c, hipStreamSynchronize(st));
    HIPC(c, hipMemcpy(h_cnt + r0, d_cnt + r0, sizeof(uint32_t) * (n - r0), hipMemcpyDeviceToHost));
    for (uint32_t r = r0; r < n && *done == 0; ++r)
      if (h_cnt[r] == 0) *done = r + 1;
  }
  return DYMU_OK;
}

int goal_labels_core(dymu_ctx* c, const double* dT, uint32_t nx, uint32_t ny, uint64_t ld,
                     const dymu_seed* seeds, uint32_t n_seeds, uint32_t* d_label, hipStream_t st,
                     uint32_t* rounds) {
  if (!dT || !d_label || nx == 0 || ny == 0 || ld < nx) return DYMU_ERR_ARG;
  if ((uint64_t)nx * ny >= (1ull << 31)) return DYMU_ERR_ARG;  // entries hold a cell index + tag
  const uint32_t n = nx * ny;
  const GoalSeed* d_seeds = nullptr;
  int rc = stage_seeds(c, nx, ny, seeds, n_seeds, st, &d_seeds, nullptr);
  if (rc) return rc;
  if (!c->ev_lab0) HIPC(c, hipEventCreate(&c->ev_lab0));
  if (!c->ev_lab1) HIPC(c, hipEventCreate(&c->ev_lab1));
  if (!c->d_lab_cnt) HIPC(c, hipMalloc(&c->d_lab_cnt, sizeof(uint32_t) * (kLabelRounds + 1)));
  c->lab_timed = false;
  HIPC(c, hipEventRecord(c->ev_lab0, st));
  HIPC(c, hipMemsetAsync(c->d_lab_cnt, 0, sizeof(uint32_t) * (kLabelRounds + 1), st));
  HIPC(c, launch_label_init(dT, (int64_t)ld, nx, ny, d_seeds, n_seeds, d_label, st));
  auto jump = [&](uint32_t r) { return launch_label_jump(d_label, n, c->d_lab_cnt, r, st); };
  uint32_t launched = 0, done = 0;
  rc = doubling_rounds(c, st, c->d_lab_cnt, kLabelRounds, jump, &launched, &done);
  if (rc) return rc;
  HIPC(c, launch_label_strip(d_label, n, st));
  HIPC(c, hipEventRecord(c->ev_lab1, st));
  HIPC(c, hipStreamSynchronize(st));
  c->lab_timed = true;
  if (rounds) *rounds = done ? done : launched;
  if (done == 0) {
    c->last_error = "goal labels: round cap reached";
    return DYMU_ERR_NOT_CONVERGED;
  }
  return DYMU_OK;
}

hipStream_t pick_stream(dymu_ctx* c, void* s) { return s ? (hipStream_t)s : c->stream; }

}  // namespace

extern "C" {

int dymu_abi_version(void) { return DYMU_ABI_VERSION; }

int dymu_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

void* dymu_get_stream(dymu_ctx* c) { return c ? static_cast<void*>(c->stream) : nullptr; }

const char* dymu_strerror(int s) {
  switch (s) {
    case DYMU_OK: return "ok";
    case DYMU_ERR_ARG: return "invalid argument";
    case DYMU_ERR_HIP: return "HIP runtime error";
    case DYMU_ERR_NOMEM: return "device out of memory";
    case DYMU_ERR_NOT_CONVERGED: return "pass cap reached before convergence";
    case DYMU_ERR_NO_DEVICE: return "no HIP device";
    case DYMU_ERR_RCCL: return "RCCL error";
    case DYMU_ERR_STATE: return "call out of sequence";
    default: return "unknown status";
  }
}

const char* dymu_last_error(dymu_ctx* c) { return c ? c->last_error.c_str() : ""; }

int dymu_create(dymu_ctx** out, const dymu_opts* opts) {
  if (!out) return DYMU_ERR_ARG;
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return DYMU_ERR_NO_DEVICE;
  dymu_ctx* c = new dymu_ctx();
  if (opts) c->opts = *opts;
  else c->opts.device = -1;
  int dev = c->opts.device;
  if (dev < 0) {
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
  }
  if (dev >= ndev) {
    delete c;
    return DYMU_ERR_ARG;
  }
  c->device = dev;
  hipError_t e = hipSetDevice(dev);
  if (e == hipSuccess) {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0)
      c->cu_count = prop.multiProcessorCount;
    e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
  }
  if (const char* kv = std::getenv("DYMU_MAP_MEM")) c->map_mem = std::atoi(kv);
  if (const char* kv = std::getenv("DYMU_WS_MEM")) c->ws_mem = c->ec_mem = c->key_mem = std::atoi(kv);
  if (const char* kv = std::getenv("DYMU_EC_MEM")) c->ec_mem = std::atoi(kv);
  if (const char* kv = std::getenv("DYMU_KEY_MEM")) c->key_mem = std::atoi(kv);
  if (const char* kv = std::getenv("DYMU_FIRST_BATCH"))
    c->first_batch = (uint64_t)std::max(1, std::atoi(kv));
  if (const char* kv = std::getenv("DYMU_PIPELINE")) c->pipeline = std::atoi(kv);
  if (const char* kv = std::getenv("DYMU_DETERMINISTIC")) c->opts.deterministic = std::atoi(kv);
  if (const char* kv = std::getenv("DYMU_MAX_BATCH"))
    c->max_batch = (uint64_t)std::min(64, std::max(1, std::atoi(kv)));
  if (const char* kv = std::getenv("DYMU_UNTIL_BATCH"))
    c->until_batch = (uint64_t)std::min(64, std::max(1, std::atoi(kv)));
  if (e == hipSuccess) {
    for (int v = 3; v <= 5; ++v) c->occupancy[v] = pass_blocks_per_cu(v);
  }
  if (e == hipSuccess) e = hipEventCreate(&c->ev0);
  if (e == hipSuccess) e = hipEventCreate(&c->ev1);
  if (!valid_variant(c->opts.kernel) || c->opts.prio_target < 0) {
    dymu_destroy(c);
    return DYMU_ERR_ARG;
  }
  c->variant = c->opts.kernel;
  if (const char* kv = std::getenv("DYMU_KERNEL")) {  // development override
    const int v = std::atoi(kv);
    c->variant = valid_variant(v) ? v : 0;
  }
  if (e == hipSuccess) {
    c->prio_target = (uint32_t)c->opts.prio_target;
    if (const char* kv = std::getenv("DYMU_PRIO_TARGET")) c->prio_target = (uint32_t)std::atol(kv);
    if (const char* kv = std::getenv("DYMU_PRIO_KAPPA")) c->prio_kappa = std::atof(kv);
    if (!(c->prio_kappa > 0.0)) c->prio_kappa = 0.5;
    if (const char* kv = std::getenv("DYMU_GRID_BLOCKS")) c->opts.grid_blocks = std::atoi(kv);
    if (const char* kv = std::getenv("DYMU_PRIO_MIN_TILES"))
      c->prio_min_tiles = (uint32_t)std::atol(kv);
    if (const char* kv = std::getenv("DYMU_PRIO_FRAC")) c->prio_frac = (float)std::atof(kv);
    if (const char* kv = std::getenv("DYMU_PRIO_TRACE")) c->prio_trace = std::atoi(kv);
    if (const char* kv = std::getenv("DYMU_PRUNE")) c->prune = std::atoi(kv);
    if (const char* kv = std::getenv("DYMU_PRIO_DEBUG")) c->prio_debug = std::atoi(kv);
    if (const char* kv = std::getenv("DYMU_RAISE")) c->raise = std::atoi(kv);
  }
  if (e == hipSuccess) e = hipMalloc(&c->d_counts, sizeof(uint32_t) * 4 * kShards);
  if (e == hipSuccess) e = hipMalloc(&c->d_scratch, sizeof(unsigned long long) * kScrWords);
  if (e == hipSuccess) e = hipMalloc(&c->d_xchg, sizeof(uint32_t));
  if (e == hipSuccess) e = hipMemset(c->d_xchg, 0, sizeof(uint32_t));
  if (e == hipSuccess)
    e = hipMalloc(&c->d_stats, sizeof(unsigned long long) * kShards * kStatSlots);
  if (e == hipSuccess) e = hipHostMalloc(&c->h_count, sizeof(uint32_t) * 4 * kShards, hipHostMallocDefault);
  if (e == hipSuccess)
    e = hipHostMalloc(&c->h_probe, sizeof(unsigned long long) * 2, hipHostMallocDefault);
  if (e == hipSuccess && c->pipeline) {  // without a mailbox: synchronous checks
    if (hipHostMalloc(&c->h_mail, 64, hipHostMallocCoherent | hipHostMallocMapped) == hipSuccess) {
      *c->h_mail = 0ull;
      void* d = nullptr;
      if (hipHostGetDevicePointer(&d, c->h_mail, 0) == hipSuccess)
        c->d_mail = static_cast<unsigned long long*>(d);
    }
    (void)hipGetLastError();
  }
  if (e != hipSuccess) {
    dymu_destroy(c);
    return e == hipErrorOutOfMemory ? DYMU_ERR_NOMEM : DYMU_ERR_HIP;
  }
  *out = c;
  return DYMU_OK;
}

int dymu_destroy(dymu_ctx* c) {
  if (!c) return DYMU_OK;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  for (hipEvent_t e : c->prof_ev) (void)hipEventDestroy(e);
  if (c->ev0) (void)hipEventDestroy(c->ev0);
  if (c->ev1) (void)hipEventDestroy(c->ev1);
  if (c->ev_path0) (void)hipEventDestroy(c->ev_path0);
  if (c->ev_path1) (void)hipEventDestroy(c->ev_path1);
  if (c->ev_pstat0) (void)hipEventDestroy(c->ev_pstat0);
  if (c->ev_pstat1) (void)hipEventDestroy(c->ev_pstat1);
  if (c->ev_arr0) (void)hipEventDestroy(c->ev_arr0);
  if (c->ev_arr1) (void)hipEventDestroy(c->ev_arr1);
  if (c->ev_simp0) (void)hipEventDestroy(c->ev_simp0);
  if (c->ev_simp1) (void)hipEventDestroy(c->ev_simp1);
  if (c->d_pq) (void)hipFree(c->d_pq);
  if (c->ev_lab0) (void)hipEventDestroy(c->ev_lab0);
  if (c->ev_lab1) (void)hipEventDestroy(c->ev_lab1);
  if (c->d_lab_cnt) (void)hipFree(c->d_lab_cnt);
  for (hipEvent_t e : c->ev_route)
    if (e) (void)hipEventDestroy(e);
  for (hipEvent_t e : c->ev_usage)
    if (e) (void)hipEventDestroy(e);
  for (hipEvent_t e : c->ev_usage_round)
    if (e) (void)hipEventDestroy(e);
  if (c->d_lists) (void)hipFree(c->d_lists);
  if (c->d_tile_epoch) (void)hipFree(c->d_tile_epoch);
  if (c->d_counts) (void)hipFree(c->d_counts);
  if (c->d_keys) (void)hipFree(c->d_keys);
  if (c->d_hist) (void)hipFree(c->d_hist);
  if (c->d_prio) (void)hipFree(c->d_prio);
  if (c->d_trace) (void)hipFree(c->d_trace);
  if (c->d_pstat) (void)hipFree(c->d_pstat);
  if (c->d_ec) (void)hipFree(c->d_ec);
  for (void* p : c->parked) (void)hipFree(p);
  if (c->d_lut) (void)hipFree(c->d_lut);
  if (c->d_scratch) (void)hipFree(c->d_scratch);
  if (c->d_theta) (void)hipFree(c->d_theta);
  if (c->d_until) (void)hipFree(c->d_until);
  if (c->d_xchg) (void)hipFree(c->d_xchg);
  if (c->d_stats) (void)hipFree(c->d_stats);
  if (c->d_F) (void)hipFree(c->d_F);
  if (c->d_T) (void)hipFree(c->d_T);
  if (c->h_count) (void)hipHostFree(c->h_count);
  if (c->h_probe) (void)hipHostFree(c->h_probe);
  if (c->h_mail) (void)hipHostFree(c->h_mail);
  if (c->d_band) (void)hipFree(c->d_band);
  if (c->h_xfer) (void)hipHostFree(c->h_xfer);
  if (c->d_region) (void)hipFree(c->d_region);
  if (c->ev_red_copy) (void)hipEventDestroy(c->ev_red_copy);
  if (c->ev_red0) (void)hipEventDestroy(c->ev_red0);
  if (c->ev_red1) (void)hipEventDestroy(c->ev_red1);
  if (c->h_red_terms) (void)hipHostFree(c->h_red_terms);
  if (c->h_red_res) (void)hipHostFree(c->h_red_res);
  if (c->d_red_terms) (void)hipFree(c->d_red_terms);
  if (c->d_red_part) (void)hipFree(c->d_red_part);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
  return DYMU_OK;
}

int dymu_solve_device(dymu_ctx* c, const double* dF, double* dT, uint32_t nx, uint32_t ny,
                      uint64_t ld, uint32_t gi, uint32_t gj, void* stream, dymu_stats* stats) {
  if (!c) return DYMU_ERR_ARG;
  HIPC(c, hipSetDevice(c->device));
  return solve_core(c, dF, dT, nx, ny, ld, gi, gj, pick_stream(c, stream), stats);
}

int dymu_solve(dymu_ctx* c, const double* F, uint32_t nx, uint32_t ny, uint32_t gi, uint32_t gj,
               double* T_out, dymu_stats* stats) {
  if (!c || !F || !T_out || nx == 0 || ny == 0) return DYMU_ERR_ARG;
  if (c->stepping) return DYMU_ERR_STATE;
  HIPC(c, hipSetDevice(c->device));
  const uint64_t cells = (uint64_t)nx * ny;
  int rc = ensure_cells(c, cells);
  if (rc) return rc;
  c->host_valid = false;
  HIPC(c, hipMemcpyAsync(c->d_F, F, sizeof(double) * cells, hipMemcpyHostToDevice, c->stream));
  rc = solve_core(c, c->d_F, c->d_T, nx, ny, nx, gi, gj, c->stream, stats);
  if (rc) return rc;
  HIPC(c, hipMemcpyAsync(T_out, c->d_T, sizeof(double) * cells, hipMemcpyDeviceToHost, c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));
  c->host_valid = true;
  c->host_nx = nx;
  c->host_ny = ny;
  c->host_gi = gi;
  c->host_gj = gj;
  return DYMU_OK;
}

int dymu_solve_until_device(dymu_ctx* c, const double* dF, double* dT, uint32_t nx, uint32_t ny,
                            uint64_t ld, uint32_t gi, uint32_t gj, uint32_t si, uint32_t sj,
                            void* stream, double* t_closed, dymu_stats* stats) {
  if (!c) return DYMU_ERR_ARG;
  HIPC(c, hipSetDevice(c->device));
  return solve_until_core(c, dF, dT, nx, ny, ld, gi, gj, si, sj, pick_stream(c, stream), t_closed,
                          stats);
}

int dymu_early_exit_mask(dymu_ctx* c, const double* dF, double* dT, uint32_t nx, uint32_t ny,
                         uint64_t ld, double t_closed, uint64_t* band_idx, uint64_t cap,
                         uint64_t* n_band, void* stream) {
  if (!c || !dF || !dT || !n_band || nx == 0 || ny == 0 || ld < nx || (cap && !band_idx))
    return DYMU_ERR_ARG;
  HIPC(c, hipSetDevice(c->device));
  hipStream_t st = pick_stream(c, stream);
  if (cap > c->band_cap) {
    if (c->d_band) HIPC(c, hipFree(c->d_band));
    c->d_band = nullptr;
    c->band_cap = 0;
    HIPC(c, hipMalloc(&c->d_band, sizeof(uint64_t) * cap));
    c->band_cap = cap;
  }
  unsigned long long* cnt = c->d_scratch + kScrCount;
  HIPC(c, hipMemsetAsync(cnt, 0, sizeof(unsigned long long), st));
  HIPC(c, launch_early_mask(dF, dT, (int64_t)ld, nx, ny, t_closed, c->d_band, cnt, cap, st));
  HIPC(c, hipMemcpyAsync(c->h_probe, cnt, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
  HIPC(c, hipStreamSynchronize(st));
  *n_band = c->h_probe[0];
  const uint64_t m = std::min<uint64_t>(*n_band, cap);
  if (m) HIPC(c, hipMemcpy(band_idx, c->d_band, sizeof(uint64_t) * m, hipMemcpyDeviceToHost));
  return DYMU_OK;
}

int dymu_count_equal(dymu_ctx* c, const double* dT, uint32_t nx, uint32_t ny, uint64_t ld,
                     double value, uint64_t* count, void* stream) {
  if (!c || !dT || !count || nx == 0 || ny == 0 || ld < nx) return DYMU_ERR_ARG;
  HIPC(c, hipSetDevice(c->device));
  hipStream_t st = pick_stream(c, stream);
  unsigned long long* cnt = c->d_scratch + kScrCount;
  HIPC(c, hipMemsetAsync(cnt, 0, sizeof(unsigned long long), st));
  HIPC(c, launch_count_equal(dT, (int64_t)ld, nx, ny, value, cnt, nullptr, 0, st));
  HIPC(c, hipMemcpyAsync(c->h_probe, cnt, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
  HIPC(c, hipStreamSynchronize(st));
  *count = c->h_probe[0];
  return DYMU_OK;
}

int dymu_find_equal(dymu_ctx* c, const double* dT, uint32_t nx, uint32_t ny, uint64_t ld,
                    double value, uint64_t* idx, uint64_t cap, uint64_t* count, void* stream) {
  if (!c || !dT || !count || nx == 0 || ny == 0 || ld < nx || (cap && !idx)) return DYMU_ERR_ARG;
  HIPC(c, hipSetDevice(c->device));
  hipStream_t st = pick_stream(c, stream);
  HIPC(c, hipStreamSynchronize(st));  // no earlier kernel still uses the transfer buffer
  int rc = ensure_xfer(c, sizeof(uint64_t) * (cap ? cap : 1));
  if (rc) return rc;
  uint64_t* di = static_cast<uint64_t*>(c->d_xfer);  // written by the kernel in host memory
  unsigned long long* cnt = c->d_scratch + kScrCount;
  HIPC(c, hipMemsetAsync(cnt, 0, sizeof(unsigned long long), st));
  HIPC(c, launch_count_equal(dT, (int64_t)ld, nx, ny, value, cnt, di, cap, st));
  HIPC(c, hipMemcpyAsync(c->h_probe, cnt, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
  HIPC(c, hipStreamSynchronize(st));
  *count = c->h_probe[0];
  const uint64_t m = std::min<uint64_t>(*count, cap);
  if (m) std::memcpy(idx, c->h_xfer, sizeof(uint64_t) * m);
  return DYMU_OK;
}

int dymu_region_stats(dymu_ctx* c, const double* dF, const double* dT, uint32_t nx, uint32_t ny,
                      uint64_t ld, uint32_t gi, uint32_t gj, double thr, double lo, double hi,
                      dymu_region* out, void* stream) {
  if (!c || !dF || !dT || !out || nx == 0 || ny == 0 || ld < nx || gi >= nx || gj >= ny)
    return DYMU_ERR_ARG;
  HIPC(c, hipSetDevice(c->device));
  hipStream_t st = pick_stream(c, stream);
  HIPC(c, hipStreamSynchronize(st));  // no earlier kernel still uses the transfer buffer
  int rc = ensure_xfer(c, sizeof(unsigned long long) * 8);
  if (rc) return rc;
  if (!c->d_region) HIPC(c, hipMalloc(&c->d_region, sizeof(unsigned long long) * 8));
  // atomics on device words (initialised by memsets), read back into pinned memory
  unsigned long long* d = c->d_region;
  auto* h = static_cast<unsigned long long*>(c->h_xfer);
  HIPC(c, hipMemsetAsync(d, 0xFF, 2 * sizeof(unsigned long long), st));  // min i, min j
  HIPC(c, hipMemsetAsync(d + 2, 0, 3 * sizeof(unsigned long long), st));  // max i, max j, count
  HIPC(c, hipMemsetAsync(d + 5, 0xFF, sizeof(unsigned long long), st));   // min distance^2
  double f0 = 0.0;  // the goal's speed
  HIPC(c, hipMemcpyAsync(h + 7, dF + (uint64_t)gj * ld + gi, sizeof(double), hipMemcpyDeviceToHost,
                         st));
  HIPC(c, launch_region_box(dT, (int64_t)ld, nx, ny, thr, lo, hi, d, st));
  HIPC(c, hipStreamSynchronize(st));
  std::memcpy(&f0, &h[7], sizeof f0);
  HIPC(c, launch_const_radius(dF, (int64_t)ld, nx, ny, gi, gj, f0, d + 5, st));
  HIPC(c, hipMemcpyAsync(h, d, 6 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
  HIPC(c, hipStreamSynchronize(st));
  std::memset(out, 0, sizeof *out);
  out->n_range = h[4];
  out->r_const = h[5] == ~0ull ? __builtin_inf() : std::sqrt((double)h[5]);
  if (h[0] > h[2]) {  // no cell at or below thr
    out->i0 = 1;
    out->i1 = 0;
    return DYMU_OK;
  }
  out->i0 = (uint32_t)h[0];
  out->j0 = (uint32_t)h[1];
  out->i1 = (uint32_t)h[2];
  out->j1 = (uint32_t)h[3];
  return DYMU_OK;
}

int dymu_scatter(dymu_ctx* c, double* dT, uint32_t nx, uint64_t ld, const uint64_t* idx,
                 const double* vals, uint64_t n, void* stream) {
  if (!c || !dT || nx == 0 || ld < nx || (n && (!idx || !vals))) return DYMU_ERR_ARG;
  if (n == 0) return DYMU_OK;
  HIPC(c, hipSetDevice(c->device));
  hipStream_t st = pick_stream(c, stream);
  // indices and values written into the pinned transfer buffer on the host and read
  // there by the kernel (ensure_xfer): no copy command, no device staging
  HIPC(c, hipStreamSynchronize(st));  // no earlier kernel still uses the transfer buffer
  int rc = ensure_xfer(c, (sizeof(uint64_t) + sizeof(double)) * n);
  if (rc) return rc;
  std::memcpy(c->h_xfer, idx, sizeof(uint64_t) * n);
  std::memcpy(static_cast<char*>(c->h_xfer) + sizeof(uint64_t) * n, vals, sizeof(double) * n);
  const uint64_t* di = static_cast<const uint64_t*>(c->d_xfer);
  const double* dv = reinterpret_cast<const double*>(di + n);
  HIPC(c, launch_scatter(dT, (int64_t)ld, nx, di, dv, n, st));
  HIPC(c, hipStreamSynchronize(st));
  return DYMU_OK;
}

// ---- the descent entries: paths, path summaries, arriving paths (descent_step.h) ----
namespace {
// What the three entries share: the checks of the shared arguments, the d_label / (gi, gj)
// branch (under a label map the single sink is unused: gi = gj = 0) and the argument block
// of the step.  Makes no HIP call.
int descent_args(dymu_ctx* c, const double* dT, uint32_t nx, uint32_t ny, uint64_t ld, double res,
                 uint32_t& gi, uint32_t& gj, const uint32_t* d_label, const double* d_goal_xy,
                 uint32_t n_goals, double tau, const double* d_start_xy, uint32_t n_paths,
                 uint32_t max_wp, DescentArgs& a) {
  if (!c || !dT || nx == 0 || ny == 0 || ld < nx) return DYMU_ERR_ARG;
  if (!(res > 0) || !(res < HUGE_VAL) || !(tau > 0) || !(tau < HUGE_VAL)) return DYMU_ERR_ARG;
  if (max_wp == 0 || max_wp > 0x7fffffffu) return DYMU_ERR_ARG;
  if (d_label) {
    if (!d_goal_xy || n_goals == 0 || n_goals >= (1u << 31)) return DYMU_ERR_ARG;
    if ((uint64_t)nx * ny >= (1ull << 31)) return DYMU_ERR_ARG;
    gi = gj = 0;
  } else if (gi >= nx || gj >= ny) {
    return DYMU_ERR_ARG;
  }
  if (n_paths && !d_start_xy) return DYMU_ERR_ARG;
  a.T = dT;
  a.ld = (int64_t)ld;
  a.nx = nx;
  a.ny = ny;
  a.res = res;
  // the host's expressions (planner.cpp computeGlobalPath / computeNextGlobalWaypoint)
  a.res_tau = res * tau;
  a.two_res = 2.0 * res;
  a.stall = 0.01 * tau * res;
  a.sink_x = res * (double)gi;
  a.sink_y = res * (double)gj;
  a.start_xy = d_start_xy;
  a.n_paths = n_paths;
  a.max_wp = max_wp;
  a.label = d_label;
  a.goal_xy = d_goal_xy;
  a.n_goals = n_goals;
  return DYMU_OK;
}

// dymu_extract_paths_device (d_label null: one sink, the goal (gi, gj)) and
// dymu_extract_paths_goals_device (the sink follows the label map)
int extract_paths(dymu_ctx* c, const double* dT, uint32_t nx, uint32_t ny, uint64_t ld, double res,
                  uint32_t gi, uint32_t gj, const uint32_t* d_label, const double* d_goal_xy,
                  uint32_t n_goals, double tau, const double* d_start_xy, uint32_t n_paths,
                  uint32_t max_wp, uint32_t stride, double* d_out, int32_t* d_count,
                  int32_t* d_status, int32_t* d_sink, void* stream) {
  PathArgs a{};
  const int rc = descent_args(c, dT, nx, ny, ld, res, gi, gj, d_label, d_goal_xy, n_goals, tau,
                              d_start_xy, n_paths, max_wp, a);
  if (rc) return rc;
  if (stride == 0 || (n_paths && (!d_out || !d_count || !d_status))) return DYMU_ERR_ARG;
  if (n_paths == 0) return DYMU_OK;
  a.stride = stride;
  a.out = d_out;
  a.count = d_count;
  a.status = d_status;
  a.sink = d_sink;
  HIPC(c, hipSetDevice(c->device));
  hipStream_t st = pick_stream(c, stream);
  return timed_launch(c, st, &dymu_ctx::path_timed, &dymu_ctx::ev_path0, &dymu_ctx::ev_path1, [&] {
    return d_label ? launch_extract_paths_goals(a, st) : launch_extract_paths(a, st);
  });
}
}  // namespace

int dymu_extract_paths_device(dymu_ctx* c, const double* dT, uint32_t nx, uint32_t ny, uint64_t ld,
                              double res, uint32_t gi, uint32_t gj, double tau,
                              const double* d_start_xy, uint32_t n_paths, uint32_t max_wp,
                              uint32_t stride, double* d_out, int32_t* d_count, int32_t* d_status,
                              void* stream) {
  return extract_paths(c, dT, nx, ny, ld, res, gi, gj, nullptr, nullptr, 0, tau, d_start_xy,
                       n_paths, max_wp, stride, d_out, d_count, d_status, nullptr, stream);
}

int dymu_extract_paths_goals_device(dymu_ctx* c, const double* dT, uint32_t nx, uint32_t ny,
                                    uint64_t ld, double res, const uint32_t* d_label,
                                    const double* d_goal_xy, uint32_t n_goals, double tau,
                                    const double* d_start_xy, uint32_t n_paths, uint32_t max_wp,
                                    uint32_t stride, double* d_out, int32_t* d_count,
                                    int32_t* d_status, void* stream, int32_t* d_sink) {
  if (!d_label || (n_paths && !d_sink)) return DYMU_ERR_ARG;
  return extract_paths(c, dT, nx, ny, ld, res, 0, 0, d_label, d_goal_xy, n_goals, tau, d_start_xy,
                       n_paths, max_wp, stride, d_out, d_count, d_status, d_sink, stream);
}

static_assert(sizeof(dymu_path_stat) == sizeof(PathStatRec) && DYMU_PATH_FIELDS == kPathFields &&
                  offsetof(dymu_path_stat, skipped) == offsetof(PathStatRec, skipped),
              "PathStatRec is dymu_path_stat's layout");

int dymu_path_stats_device(dymu_ctx* c, const double* dT, uint32_t nx, uint32_t ny, uint64_t ld,
                           double res, uint32_t gi, uint32_t gj, const uint32_t* d_label,
                           const double* d_goal_xy, uint32_t n_goals, double tau,
                           const double* d_start_xy, uint32_t n_paths, uint32_t max_wp,
                           const double* const* d_fields, const uint64_t* field_ld,
                           uint32_t n_fields, uint32_t n_lanes, dymu_path_stat* d_stats,
                           void* stream) {
  PathStatArgs a{};
  const int rc = descent_args(c, dT, nx, ny, ld, res, gi, gj, d_label, d_goal_xy, n_goals, tau,
                              d_start_xy, n_paths, max_wp, a);
  if (rc) return rc;
  if (n_paths > 0x7fffffffu || (n_paths && !d_stats)) return DYMU_ERR_ARG;
  if (n_fields > DYMU_PATH_FIELDS || (n_fields && (!d_fields || !field_ld))) return DYMU_ERR_ARG;
  for (uint32_t f = 0; f < n_fields; ++f)
    if (!d_fields[f] || field_ld[f] < nx) return DYMU_ERR_ARG;
  if (n_paths == 0) return DYMU_OK;
  for (uint32_t f = 0; f < n_fields; ++f) {
    a.field[f] = d_fields[f];
    a.field_ld[f] = (int64_t)field_ld[f];
  }
  a.out = reinterpret_cast<PathStatRec*>(d_stats);
  HIPC(c, hipSetDevice(c->device));
  hipStream_t st = pick_stream(c, stream);
  if (!c->d_pq) HIPC(c, hipMalloc(&c->d_pq, 256));
  a.next = c->d_pq;
  // The default is one lane per path: lanes that refill from the queue were slower than
  // that where measured.  More lanes than paths would only fetch and
  // leave; the fetches add at most n_paths + lanes < 2^32 to the counter.
  const uint32_t whole = (n_paths + 63u) / 64u * 64u;
  uint32_t lanes = n_lanes ? (n_lanes + 63u) / 64u * 64u : whole;
  if (n_lanes > 0xffffffc0u || lanes > whole) lanes = whole;
  c->pstat_timed = false;  // the queue's reset is outside the timed bracket
  HIPC(c, hipMemsetAsync(c->d_pq, 0, sizeof(uint32_t), st));
  return timed_launch(c, st, &dymu_ctx::pstat_timed, &dymu_ctx::ev_pstat0, &dymu_ctx::ev_pstat1,
                      [&] { return launch_path_stats(a, n_fields, lanes, st); });
}

int dymu_last_path_stats_ms(dymu_ctx* c, double* ms) {
  return elapsed_ms(c, &dymu_ctx::pstat_timed, &dymu_ctx::ev_pstat0, &dymu_ctx::ev_pstat1, ms);
}

// ---- the arriving descent (arrive_kernels.hip) ----
static_assert(sizeof(dymu_arrive_stat) == 32 && sizeof(dymu_arrive_stat) == sizeof(ArriveRec) &&
                  offsetof(dymu_arrive_stat, start_cost) == offsetof(ArriveRec, start_cost),
              "ArriveRec is dymu_arrive_stat's layout");

int dymu_arrive_paths_device(dymu_ctx* c, const double* dT, uint32_t nx, uint32_t ny, uint64_t ld,
                             double res, uint32_t gi, uint32_t gj, const uint32_t* d_label,
                             const double* d_goal_xy, uint32_t n_goals, double tau,
                             const double* d_start_xy, uint32_t n_paths, uint32_t max_wp,
                             uint32_t stride, double* d_out, int32_t* d_count,
                             dymu_arrive_stat* d_stats, void* stream) {
  ArriveArgs a{};
  const int rc = descent_args(c, dT, nx, ny, ld, res, gi, gj, d_label, d_goal_xy, n_goals, tau,
                              d_start_xy, n_paths, max_wp, a);
  if (rc) return rc;
  if (stride == 0 || (n_paths && (!d_stats || (d_out && !d_count)))) return DYMU_ERR_ARG;
  if (n_paths == 0) return DYMU_OK;
  a.goal_i = gi;
  a.goal_j = gj;
  a.stride = stride;
  a.out = d_out;
  a.count = d_count;
  a.stats = reinterpret_cast<ArriveRec*>(d_stats);
  HIPC(c, hipSetDevice(c->device));
  hipStream_t st = pick_stream(c, stream);
  return timed_launch(c, st, &dymu_ctx::arr_timed, &dymu_ctx::ev_arr0, &dymu_ctx::ev_arr1,
                      [&] { return launch_arrive_paths(a, st); });
}

int dymu_last_arrive_ms(dymu_ctx* c, double* ms) {
  return elapsed_ms(c, &dymu_ctx::arr_timed, &dymu_ctx::ev_arr0, &dymu_ctx::ev_arr1, ms);
}

// ---- the simplified arriving descent (path_simplify.h) ----
int dymu_arrive_simplified_device(dymu_ctx* c, const double* dT, uint32_t nx, uint32_t ny,
                                  uint64_t ld, double res, uint32_t gi, uint32_t gj,
                                  const uint32_t* d_label, const double* d_goal_xy,
                                  uint32_t n_goals, double tau, const double* d_start_xy,
                                  uint32_t n_paths, double eps, uint32_t max_steps,
                                  uint32_t max_kept, double* d_out, uint32_t* d_index,
                                  int32_t* d_count, dymu_arrive_stat* d_stats, void* stream) {
  ArriveArgs a{};
  const int rc = descent_args(c, dT, nx, ny, ld, res, gi, gj, d_label, d_goal_xy, n_goals, tau,
                              d_start_xy, n_paths, max_steps, a);
  if (rc) return rc;
  if (!(eps > 0) || !(eps < HUGE_VAL)) return DYMU_ERR_ARG;
  if (max_kept == 0 && (d_out || d_index)) return DYMU_ERR_ARG;
  if (n_paths && (!d_stats || !d_count)) return DYMU_ERR_ARG;
  if (n_paths == 0) return DYMU_OK;
  a.goal_i = gi;
  a.goal_j = gj;
  a.stride = 1;
  a.out = d_out;
  a.count = d_count;
  a.stats = reinterpret_cast<ArriveRec*>(d_stats);
  a.eps = eps;
  a.eps2 = eps * eps;
  a.max_kept = max_kept;
  a.index = d_index;
  HIPC(c, hipSetDevice(c->device));
  hipStream_t st = pick_stream(c, stream);
  return timed_launch(c, st, &dymu_ctx::simp_timed, &dymu_ctx::ev_simp0, &dymu_ctx::ev_simp1,
                      [&] { return launch_arrive_simplified(a, st); });
}

int dymu_last_arrive_simplified_ms(dymu_ctx* c, double* ms) {
  return elapsed_ms(c, &dymu_ctx::simp_timed, &dymu_ctx::ev_simp0, &dymu_ctx::ev_simp1, ms);
}

// ---- every cell's node route (route_kernels.hip) ----
namespace {
constexpr size_t kRouteAlign = 256;
constexpr size_t kRouteCntBytes = 256;  // kRouteRounds counters at the workspace's start
static_assert(sizeof(uint32_t) * kRouteRounds <= kRouteCntBytes, "the counters fit");

// which arrays the doubling carries for these outputs (null `out`: all of n_fields fields)
struct RouteCarry {
  bool cnt;
  bool integ[kPathFields], vmin[kPathFields], vmax[kPathFields];
};
RouteCarry route_carry(uint32_t n_fields, const dymu_route_out* out) {
  RouteCarry k{};
  k.cnt = !out || out->axis || out->diag || out->length;
  for (uint32_t f = 0; f < n_fields; ++f) {
    k.integ[f] = !out || out->integral[f];
    k.vmin[f] = !out || out->vmin[f];
    k.vmax[f] = !out || out->vmax[f];
  }
  return k;
}
// the workspace's layout: the counters, then per carried array its two buffers; returns
// the bytes used, and with ws the two states
size_t route_layout(uint64_t n, const RouteCarry& k, char* ws, RouteState st[2]) {
  size_t off = kRouteCntBytes;
  auto take = [&](size_t elem, void** a, void** b) {
    const size_t bytes = (elem * n + kRouteAlign - 1) / kRouteAlign * kRouteAlign;
    if (ws) {
      *a = ws + off;
      *b = ws + off + bytes;
    }
    off += 2 * bytes;
  };
  RouteState dummy[2]{};
  RouteState* s = st ? st : dummy;
  take(4, (void**)&s[0].next, (void**)&s[1].next);
  if (k.cnt) {
    take(4, (void**)&s[0].axis, (void**)&s[1].axis);
    take(4, (void**)&s[0].diag, (void**)&s[1].diag);
  }
  for (int f = 0; f < kPathFields; ++f) {
    if (k.integ[f]) take(8, (void**)&s[0].integ[f], (void**)&s[1].integ[f]);
    if (k.vmin[f]) take(8, (void**)&s[0].vmin[f], (void**)&s[1].vmin[f]);
    if (k.vmax[f]) take(8, (void**)&s[0].vmax[f], (void**)&s[1].vmax[f]);
  }
  return off;
}
bool route_out_ok(uint32_t n_fields, const dymu_route_out* out) {
  if (!out) return true;
  for (uint32_t f = n_fields; f < DYMU_PATH_FIELDS; ++f)
    if (out->integral[f] || out->vmin[f] || out->vmax[f]) return false;
  return true;
}
}  // namespace

size_t dymu_route_fields_workspace(uint32_t nx, uint32_t ny, uint32_t n_fields,
                                   const dymu_route_out* out) {
  const uint64_t n = (uint64_t)nx * ny;
  if (n == 0 || n >= (1ull << 31) || n_fields > DYMU_PATH_FIELDS || !route_out_ok(n_fields, out))
    return 0;
  return route_layout(n, route_carry(n_fields, out), nullptr, nullptr);
}

int dymu_route_fields_device(dymu_ctx* c, const double* dT, uint32_t nx, uint32_t ny, uint64_t ld,
                             double res, const dymu_seed* seeds, uint32_t n_seeds,
                             const double* const* d_fields, const uint64_t* field_ld,
                             uint32_t n_fields, const dymu_route_out* out, void* d_workspace,
                             size_t workspace_bytes, void* stream, uint32_t* rounds) {
  if (!c || !dT || !out || !d_workspace || nx == 0 || ny == 0 || ld < nx || out->ld < nx)
    return DYMU_ERR_ARG;
  if ((uint64_t)nx * ny >= (1ull << 31)) return DYMU_ERR_ARG;  // entries hold a cell index + tag
  if (!(res > 0) || !(res < HUGE_VAL)) return DYMU_ERR_ARG;
  if (n_fields > DYMU_PATH_FIELDS || (n_fields && (!d_fields || !field_ld))) return DYMU_ERR_ARG;
  for (uint32_t f = 0; f < n_fields; ++f)
    if (!d_fields[f] || field_ld[f] < nx) return DYMU_ERR_ARG;
  if (!route_out_ok(n_fields, out)) return DYMU_ERR_ARG;
  if (reinterpret_cast<uintptr_t>(d_workspace) % kRouteAlign) return DYMU_ERR_ARG;
  const uint32_t n = nx * ny;
  const RouteCarry carry = route_carry(n_fields, out);
  RouteState s[2]{};
  if (route_layout(n, carry, static_cast<char*>(d_workspace), s) > workspace_bytes)
    return DYMU_ERR_ARG;
  HIPC(c, hipSetDevice(c->device));
  hipStream_t st = pick_stream(c, stream);
  const GoalSeed* d_seeds = nullptr;
  int rc = stage_seeds(c, nx, ny, seeds, n_seeds, st, &d_seeds, nullptr);
  if (rc) return rc;
  for (hipEvent_t& e : c->ev_route)
    if (!e) HIPC(c, hipEventCreate(&e));
  uint32_t* d_cnt = static_cast<uint32_t*>(d_workspace);
  RouteInitArgs ia{};
  ia.T = dT;
  ia.ld = (int64_t)ld;
  ia.nx = nx;
  ia.ny = ny;
  ia.res = res;
  for (uint32_t f = 0; f < n_fields; ++f) {
    // a field none of whose aggregates is asked for is not sampled
    if (!carry.integ[f] && !carry.vmin[f] && !carry.vmax[f]) continue;
    ia.field[f] = d_fields[f];
    ia.field_ld[f] = (int64_t)field_ld[f];
  }
  ia.s0 = s[0];
  ia.s1 = s[1];
  c->route_timed = false;
  HIPC(c, hipEventRecord(c->ev_route[0], st));
  HIPC(c, hipMemsetAsync(d_cnt, 0, kRouteCntBytes, st));
  HIPC(c, launch_route_init(ia, d_seeds, n_seeds, st));
  HIPC(c, hipEventRecord(c->ev_route[1], st));
  auto launch_round = [&](uint32_t r) {  // round r reads buffer r & 1
    return launch_route_round(s[r & 1u], s[(r + 1u) & 1u], n, d_cnt, r, st);
  };
  uint32_t launched = 0, done = 0;
  rc = doubling_rounds(c, st, d_cnt, kRouteRounds, launch_round, &launched, &done);
  if (rc) return rc;
  HIPC(c, hipEventRecord(c->ev_route[2], st));
  const uint32_t ran = done ? done : launched;
  RouteFinalArgs fa{};
  fa.nx = nx;
  fa.ny = ny;
  fa.res = res;
  for (int f = 0; f < kPathFields; ++f) {
    fa.field[f] = ia.field[f];
    fa.field_ld[f] = ia.field_ld[f];
    fa.o_integ[f] = out->integral[f];
    fa.o_vmin[f] = out->vmin[f];
    fa.o_vmax[f] = out->vmax[f];
  }
  fa.s = s[ran & 1u];  // the state after `ran` rounds
  fa.seeds = d_seeds;
  fa.n_seeds = n_seeds;
  fa.o_sink = out->sink;
  fa.o_axis = out->axis;
  fa.o_diag = out->diag;
  fa.o_length = out->length;
  fa.o_ld = (int64_t)out->ld;
  HIPC(c, launch_route_final(fa, st));
  HIPC(c, hipEventRecord(c->ev_route[3], st));
  c->route_timed = true;
  if (rounds) *rounds = ran;
  if (done == 0) {
    c->last_error = "route fields: round cap reached";
    return DYMU_ERR_NOT_CONVERGED;
  }
  return DYMU_OK;
}

int dymu_last_route_fields_ms(dymu_ctx* c, double* ms) {
  return total_ms(c, &dymu_ctx::route_timed, &dymu_ctx::ev_route, ms);
}

int dymu_last_route_fields_stages(dymu_ctx* c, double out[3]) {
  return stage_ms(c, &dymu_ctx::route_timed, &dymu_ctx::ev_route, out);
}

// ---- how much of the map drains through every cell (usage_kernels.hip) ----
namespace {
constexpr size_t kUsageCntBytes = 512;  // 2 * kRouteRounds counters at the workspace's start
static_assert(sizeof(uint32_t) * 2 * kRouteRounds <= kUsageCntBytes, "the counters fit");
struct UsageState {
  uint32_t* next[2];
  unsigned long long* sum[2];
  unsigned long long* far;
};
// the workspace's layout: the counters, the two entry arrays, the two sums, the maximum;
// returns the bytes used, and with ws the arrays
size_t usage_layout(uint64_t n, bool sums, bool far, char* ws, UsageState* s) {
  size_t off = kUsageCntBytes;
  auto take = [&](size_t elem) {
    char* p = ws ? ws + off : nullptr;
    off += (elem * n + kRouteAlign - 1) / kRouteAlign * kRouteAlign;
    return p;
  };
  UsageState d{};
  d.next[0] = reinterpret_cast<uint32_t*>(take(4));
  d.next[1] = reinterpret_cast<uint32_t*>(take(4));
  if (sums) {
    d.sum[0] = reinterpret_cast<unsigned long long*>(take(8));
    d.sum[1] = reinterpret_cast<unsigned long long*>(take(8));
  }
  if (far) d.far = reinterpret_cast<unsigned long long*>(take(8));
  if (s) *s = d;
  return off;
}
}  // namespace

size_t dymu_route_usage_workspace(uint32_t nx, uint32_t ny, const dymu_usage_out* out) {
  const uint64_t n = (uint64_t)nx * ny;
  if (n == 0 || n >= (1ull << 31)) return 0;
  return usage_layout(n, !out || out->usage, !out || out->far, nullptr, nullptr);
}

int dymu_route_usage_device(dymu_ctx* c, const double* dT, uint32_t nx, uint32_t ny, uint64_t ld,
                            const dymu_seed* seeds, uint32_t n_seeds, const uint32_t* d_weight,
                            uint64_t weight_ld, const dymu_usage_out* out, uint64_t* catchment,
                            void* d_workspace, size_t workspace_bytes, void* stream,
                            uint32_t* rounds) {
  if (!c || !dT || !out || !d_workspace || nx == 0 || ny == 0 || ld < nx || out->ld < nx)
    return DYMU_ERR_ARG;
  if ((uint64_t)nx * ny >= (1ull << 31)) return DYMU_ERR_ARG;  // entries hold a cell index + tag
  if (d_weight && weight_ld < nx) return DYMU_ERR_ARG;
  if (!out->usage && !out->far && !out->sink && !catchment) return DYMU_ERR_ARG;
  if (reinterpret_cast<uintptr_t>(d_workspace) % kRouteAlign) return DYMU_ERR_ARG;
  const uint32_t n = nx * ny;
  const bool sums = out->usage || catchment;
  UsageState s{};
  if (usage_layout(n, sums, out->far != nullptr, static_cast<char*>(d_workspace), &s) >
      workspace_bytes)
    return DYMU_ERR_ARG;
  // round 0 by neighbour reads instead of atomics (the faster form at
  // 16384^2); development override: DYMU_USAGE_ROUND0=0 runs the plain atomic form, the
  // reference path
  bool gather0 = true;
  if (const char* kv = std::getenv("DYMU_USAGE_ROUND0")) gather0 = std::atoi(kv) != 0;
  HIPC(c, hipSetDevice(c->device));
  hipStream_t st = pick_stream(c, stream);
  const GoalSeed* d_seeds = nullptr;
  // the catchments come back through the transfer buffer, behind the seeds
  const uint64_t catch_bytes = catchment ? sizeof(uint64_t) * (uint64_t)n_seeds : 0;
  int rc = stage_seeds(c, nx, ny, seeds, n_seeds, st, &d_seeds, nullptr, catch_bytes);
  if (rc) return rc;
  const uint64_t catch_off = sizeof(GoalSeed) * (uint64_t)n_seeds;  // a multiple of 16
  for (hipEvent_t& e : c->ev_usage)
    if (!e) HIPC(c, hipEventCreate(&e));
  for (hipEvent_t& e : c->ev_usage_round)
    if (!e) HIPC(c, hipEventCreate(&e));
  uint32_t* d_cnt = static_cast<uint32_t*>(d_workspace);
  RouteInitArgs ia{};  // the entries only: no hop counts, no fields
  ia.T = dT;
  ia.ld = (int64_t)ld;
  ia.nx = nx;
  ia.ny = ny;
  ia.res = 1.0;
  ia.s0.next = s.next[0];
  ia.s1.next = s.next[1];
  c->usage_timed = false;
  HIPC(c, hipEventRecord(c->ev_usage[0], st));
  HIPC(c, hipMemsetAsync(d_cnt, 0, kUsageCntBytes, st));
  HIPC(c, launch_route_init(ia, d_seeds, n_seeds, st));
  HIPC(c, launch_usage_init(dT, (int64_t)ld, nx, ny, d_weight, (int64_t)weight_ld, s.sum[0], s.far,
                            st));
  HIPC(c, hipEventRecord(c->ev_usage[1], st));
  // round r reads buffer r & 1, behind its own time stamp
  auto launch_round = [&](uint32_t r) {
    UsageRoundArgs ra{};
    ra.nx = nx;
    ra.ny = ny;
    ra.nsrc = s.next[r & 1u];
    ra.ndst = s.next[(r + 1u) & 1u];
    ra.asrc = s.sum[r & 1u];
    ra.adst = s.sum[(r + 1u) & 1u];
    ra.far = s.far;
    const hipError_t e = hipEventRecord(c->ev_usage_round[r], st);
    return e != hipSuccess ? e : launch_usage_round(ra, d_cnt, r, gather0, st);
  };
  uint32_t launched = 0, done = 0;
  rc = doubling_rounds(c, st, d_cnt, kRouteRounds, launch_round, &launched, &done);
  if (rc) return rc;
  HIPC(c, hipEventRecord(c->ev_usage_round[launched], st));
  c->usage_rounds_timed = launched;
  HIPC(c, hipEventRecord(c->ev_usage[2], st));
  const uint32_t ran = done ? done : launched;
  UsageFinalArgs fa{};
  fa.nx = nx;
  fa.ny = ny;
  fa.next = s.next[ran & 1u];  // the state after `ran` rounds
  fa.sum = s.sum[ran & 1u];
  fa.far = s.far;
  fa.n_seeds = n_seeds;
  fa.o_usage = reinterpret_cast<unsigned long long*>(out->usage);
  fa.o_far = out->far;
  fa.o_sink = out->sink;
  fa.o_ld = (int64_t)out->ld;
  unsigned long long* d_catch =
      catchment ? reinterpret_cast<unsigned long long*>(static_cast<char*>(c->d_xfer) + catch_off)
                : nullptr;
  HIPC(c, launch_usage_final(fa, d_seeds, d_catch, st));
  HIPC(c, hipEventRecord(c->ev_usage[3], st));
  c->usage_timed = true;
  if (rounds) *rounds = ran;
  if (catchment) {  // written by the kernel in host memory
    HIPC(c, hipStreamSynchronize(st));
    std::memcpy(catchment, static_cast<const char*>(c->h_xfer) + catch_off, (size_t)catch_bytes);
  }
  if (done == 0) {
    c->last_error = "route usage: round cap reached";
    return DYMU_ERR_NOT_CONVERGED;
  }
  return DYMU_OK;
}

int dymu_last_route_usage_ms(dymu_ctx* c, double* ms) {
  return total_ms(c, &dymu_ctx::usage_timed, &dymu_ctx::ev_usage, ms);
}

int dymu_last_route_usage_stages(dymu_ctx* c, double out[3]) {
  return stage_ms(c, &dymu_ctx::usage_timed, &dymu_ctx::ev_usage, out);
}

int dymu_last_route_usage_round_ms(dymu_ctx* c, double round_ms[32], uint32_t* rounds) {
  if (!c || !round_ms || !rounds) return DYMU_ERR_ARG;
  if (!c->usage_timed) return DYMU_ERR_STATE;
  HIPC(c, hipSetDevice(c->device));
  for (uint32_t r = 0; r < c->usage_rounds_timed; ++r) {
    const int rc = event_ms(c, c->ev_usage_round[r], c->ev_usage_round[r + 1], &round_ms[r]);
    if (rc) return rc;
  }
  *rounds = c->usage_rounds_timed;
  return DYMU_OK;
}

int dymu_solve_seeds_device(dymu_ctx* c, const double* dF, double* dT, uint32_t nx, uint32_t ny,
                            uint64_t ld, const dymu_seed* seeds, uint32_t n_seeds, void* stream,
                            dymu_stats* stats) {
  if (!c) return DYMU_ERR_ARG;
  HIPC(c, hipSetDevice(c->device));
  return solve_seeds_core(c, dF, dT, nx, ny, ld, seeds, n_seeds, pick_stream(c, stream), stats);
}

// ---- batched solves (batch_kernels.hip) ----

uint32_t dymu_batch_plane_rows(uint32_t ny) {
  return (uint32_t)(16ull * (((uint64_t)ny + 1 + 15) / 16));
}

namespace {
// the stack's rows B * P when the arguments describe a stack the engine can address
bool batch_rows(uint32_t nx, uint32_t ny, uint32_t B, uint64_t ld, uint32_t* rows) {
  if (nx == 0 || ny == 0 || B == 0 || ld < nx) return false;
  const uint64_t r = (uint64_t)B * (16ull * (((uint64_t)ny + 16) / 16));  // B * P in 64 bits
  if (r > 0xFFFFFFFFull) return false;
  *rows = (uint32_t)r;
  return true;
}
}  // namespace

int dymu_stack_speed_device(dymu_ctx* c, const double* src, uint64_t src_ld,
                            uint64_t src_plane_stride, uint32_t nx, uint32_t ny, uint32_t B,
                            double* dF_stack, uint64_t ld, void* stream) {
  uint32_t rows = 0;
  if (!c || !src || !dF_stack || src_ld < nx || !batch_rows(nx, ny, B, ld, &rows))
    return DYMU_ERR_ARG;
  HIPC(c, hipSetDevice(c->device));
  HIPC(c, launch_stack_speed(src, src_ld, src_plane_stride, nx, ny, B, dymu_batch_plane_rows(ny),
                             dF_stack, ld, pick_stream(c, stream)));
  return DYMU_OK;
}

namespace {
// dymu_solve_batch_device; with targets (any order, checked here, sorted by plane for the
// probe's waves) dymu_solve_batch_until_device
int solve_batch(dymu_ctx* c, const double* dF_stack, double* dT_stack, uint32_t nx, uint32_t ny,
                uint32_t B, uint64_t ld, const dymu_batch_seed* seeds, uint32_t n_seeds,
                void* stream, dymu_stats* stats, const dymu_batch_cell* targets = nullptr,
                uint32_t n_targets = 0, double* t_closed = nullptr, double* t_plane = nullptr) {
  uint32_t rows = 0;
  if (!c || !dF_stack || !dT_stack || !seeds || n_seeds == 0 || n_seeds >= (1u << 31) ||
      !batch_rows(nx, ny, B, ld, &rows))
    return DYMU_ERR_ARG;
  const uint32_t P = dymu_batch_plane_rows(ny);
  // the seeds on stacked rows; every plane needs one (an unseeded plane would stay +inf)
  std::vector<dymu_seed> s(n_seeds);
  std::vector<uint8_t> seeded(B, 0);
  for (uint32_t k = 0; k < n_seeds; ++k) {
    const dymu_batch_seed& b = seeds[k];
    if (b.plane >= B || b.i >= nx || b.j >= ny || !(b.t0 >= 0.0) || !(b.t0 < __builtin_inf()))
      return DYMU_ERR_ARG;
    seeded[b.plane] = 1;
    s[k] = dymu_seed{b.i, b.plane * P + b.j, b.t0};
  }
  for (uint32_t b = 0; b < B; ++b)
    if (!seeded[b]) return DYMU_ERR_ARG;
  std::vector<ProbeTarget> tg;
  UntilTargets until{};
  if (targets) {
    std::vector<uint32_t> at(B + 1ull, 0u);  // counting sort by plane (stable)
    for (uint32_t k = 0; k < n_targets; ++k) {
      const dymu_batch_cell& q = targets[k];
      if (q.plane >= B || q.i >= nx || q.j >= ny) return DYMU_ERR_ARG;
      ++at[q.plane + 1ull];
    }
    for (uint32_t b = 0; b < B; ++b) at[b + 1ull] += at[b];
    tg.resize(n_targets);
    for (uint32_t k = 0; k < n_targets; ++k)
      tg[at[targets[k].plane]++] = ProbeTarget{targets[k].plane, targets[k].i, targets[k].j, 0u};
    until = UntilTargets{tg.data(), n_targets, ny, B, P, t_closed, t_plane};
  }
  HIPC(c, hipSetDevice(c->device));
  // The per-pass relax target is the one any solve of an nx x rows domain gets
  // (dom_begin); DYMU_BATCH_TARGET_PER_CU (tiles per CU, development) overrides it for
  // this entry point alone -- the measurements of DESIGN.md s5.7 found no better value.
  const uint32_t saved = c->prio_target;
  if (saved == 0)
    if (const char* kv = std::getenv("DYMU_BATCH_TARGET_PER_CU")) {
      const long v = std::atol(kv);
      if (v > 0 && v < 4096) c->prio_target = (uint32_t)c->cu_count * (uint32_t)v;
    }
  const int rc = solve_seeds_core(c, dF_stack, dT_stack, nx, rows, ld, s.data(), n_seeds,
                                  pick_stream(c, stream), stats, targets ? &until : nullptr);
  c->prio_target = saved;
  return rc;
}
}  // namespace

int dymu_solve_batch_device(dymu_ctx* c, const double* dF_stack, double* dT_stack, uint32_t nx,
                            uint32_t ny, uint32_t B, uint64_t ld, const dymu_batch_seed* seeds,
                            uint32_t n_seeds, void* stream, dymu_stats* stats) {
  return solve_batch(c, dF_stack, dT_stack, nx, ny, B, ld, seeds, n_seeds, stream, stats);
}

/* ---- early exit on target cells ---- */

int dymu_solve_batch_until_device(dymu_ctx* c, const double* dF_stack, double* dT_stack,
                                  uint32_t nx, uint32_t ny, uint32_t B, uint64_t ld,
                                  const dymu_batch_seed* seeds, uint32_t n_seeds,
                                  const dymu_batch_cell* targets, uint32_t n_targets, void* stream,
                                  double* t_closed, double* t_plane, dymu_stats* stats) {
  if (!c || !targets || n_targets == 0 || n_targets >= (1u << 31) || !t_closed)
    return DYMU_ERR_ARG;
  return solve_batch(c, dF_stack, dT_stack, nx, ny, B, ld, seeds, n_seeds, stream, stats, targets,
                     n_targets, t_closed, t_plane);
}

int dymu_solve_seeds_until_device(dymu_ctx* c, const double* dF, double* dT, uint32_t nx,
                                  uint32_t ny, uint64_t ld, const dymu_seed* seeds,
                                  uint32_t n_seeds, const dymu_cell* targets, uint32_t n_targets,
                                  void* stream, double* t_closed, dymu_stats* stats) {
  if (!c || !dF || !dT || !seeds || !targets || n_targets == 0 || n_targets >= (1u << 31) ||
      !t_closed)
    return DYMU_ERR_ARG;
  std::vector<ProbeTarget> tg(n_targets);
  for (uint32_t k = 0; k < n_targets; ++k) {
    if (targets[k].i >= nx || targets[k].j >= ny) return DYMU_ERR_ARG;
    tg[k] = ProbeTarget{0u, targets[k].i, targets[k].j, 0u};
  }
  const UntilTargets until{tg.data(), n_targets, ny, 1u, ny, t_closed, nullptr};
  HIPC(c, hipSetDevice(c->device));
  return solve_seeds_core(c, dF, dT, nx, ny, ld, seeds, n_seeds, pick_stream(c, stream), stats,
                          &until);
}

/* ---- obstacle clearance field and risk-inflated speed ---- */

namespace {
// converge_targets with a constant level instead of a probe over target cells: the key
// bound read back with the counters, compare.  Ends at the first check at which every
// queued tile's key exceeds `level` (no pass can lower a value at or below it any more),
// or with nothing queued.  The caller has recorded ev0 before its preparation.
int converge_level(dymu_ctx* c, hipStream_t st, dymu_stats* stats, double level) {
  auto queue_test = [&]() {
    return hipMemcpyAsync(c->h_probe + 1, prio_minkey(c, c->dom.p % 3),
                          sizeof(unsigned long long), hipMemcpyDeviceToHost, st);
  };
  auto stop = [&](uint64_t pending) {
    double kmin;
    std::memcpy(&kmin, &c->h_probe[1], sizeof kmin);
    return kmin > level || pending == 0;
  };
  return converge_checked(c, st, stats, c->until_batch, /*record_ev0=*/false,
                          "key bound read-back", queue_test, stop);
}
}  // namespace

int dymu_clearance_device(dymu_ctx* c, const double* dF, double* dW, double* dS, uint32_t nx,
                          uint32_t ny, uint64_t ld, double step, void* stream, dymu_stats* stats) {
  if (!c || !dF || !dW || !dS || nx == 0 || ny == 0 || ld < nx) return DYMU_ERR_ARG;
  if (!(step > 0.0) || !(step < __builtin_inf())) return DYMU_ERR_ARG;
  if (c->stepping) return DYMU_ERR_STATE;
  HIPC(c, hipSetDevice(c->device));
  hipStream_t st = pick_stream(c, stream);
  HIPC(c, hipEventRecord(c->ev0, st));  // the fill and the seeding count as the call's time
  HIPC(c, launch_fill_const(dW, ld, nx, ny, step, st));
  int rc = dom_begin(c, dW, dS, nx, ny, ld, 0, 0, -1, -1, st, true, /*need_keys=*/true);
  if (rc) return rc;
  auto& D = c->dom;
  MaskSeedArgs a{};
  a.T = dS;
  a.ld = (int64_t)ld;
  a.nx = nx;
  a.ny = ny;
  bind_list0(c, a);  // a priority kernel (need_keys): keys and histogram
  a.ec = D.a.ec;
  a.n_obst = c->d_scratch + kScrObst;
  // list 0's smallest key and histogram origin: +0.0, the value of every seed
  hipError_t e = launch_store_u64(prio_minkey(c, 0), 0ull, st);
  if (e == hipSuccess)
    e = launch_store_u64(reinterpret_cast<unsigned long long*>(prio_base(c, 0)), 0ull, st);
  if (e == hipSuccess) e = launch_store_u64(a.n_obst, 0ull, st);
  // 8 workgroups of at most 256 lanes per CU: all resident, their claims' latencies overlap
  if (e == hipSuccess) e = launch_seed_mask(dF, a, D.ntiles, (uint32_t)c->cu_count * 8u, st);
  if (e == hipSuccess)
    e = hipMemcpyAsync(c->h_probe, a.n_obst, sizeof(unsigned long long), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) {
    dom_retire(c);
    return fail_hip(c, e, "obstacle seeding");
  }
  // no obstacle: the field is +inf everywhere, no pass runs
  if (c->h_probe[0] == 0ull) return finish_timed(c, st, stats);
  return converge_level(c, st, stats, 1.0);
}

// The field after obstacles were added inside a window: a warm, decrease-only start on
// (dW, dS) -- the old field bounds the new one from above, so nothing is reset -- from the
// new obstacle cells, the passes under converge_level, then the box of the claimed tiles.
//
// edit (dymu_clearance_edit_device): the window may free obstacle cells
// too.  Every state the passes leave is a supersolution (a cell's value was the update of its
// neighbours when it was written, and they only fell since), so after the freed cells are
// set to +inf and every cell whose value its current neighbours no longer support followed
// them (run_raise, seeded), what is left bounds the new field from above and the warm start
// above fills the cone: from the added cells and from the cone's boundary inside the tiles
// the raise claimed.  The box is the union of what the raise and the passes each claimed.
namespace {
// what the stages of a windowed clearance call share
struct ClearanceCall {
  const double* dF;  // the mask
  double* dW;        // the constant speed map
  double step;
  int variant;       // the pass kernel (dom_variant): a's tile geometry anticipates its domain
  MaskSeedArgs a;    // the field (T, ld, nx, ny); list 0 is bound once the pass domain is live
  MaskWindow win;
  uint32_t blocks;   // 8 workgroups per CU, as dymu_clearance_device seeds
  bool added, freed;  // what the count found
};

// The box {x0, y0, x1, y1}, in tiles, of the first `ntiles` tiles (ntx per row) whose stamp
// is at least stamp_lo; x1 = 0: none.  Synchronises the stream.
hipError_t claimed_box(dymu_ctx* c, uint32_t ntiles, uint32_t ntx, uint32_t stamp_lo,
                       hipStream_t st, uint32_t out[4]) {
  unsigned long long* dbox = c->d_scratch + kScrBox;
  hipError_t e = launch_store_u64(dbox, ~0ull, st);
  if (e == hipSuccess) e = launch_store_u64(dbox + 1, 0ull, st);
  uint32_t* box32 = reinterpret_cast<uint32_t*>(dbox);
  if (e == hipSuccess) e = launch_claimed_box(c->d_tile_epoch, ntiles, ntx, stamp_lo, box32, st);
  if (e == hipSuccess)
    e = hipMemcpyAsync(c->h_probe, dbox, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e == hipSuccess) std::memcpy(out, c->h_probe, 4 * sizeof(uint32_t));
  return e;
}

// Count first: the new obstacle cells and the freed ones (k.added, k.freed), nothing written.
// Neither: the field stands, and the call ends here -- the empty box, its time, no domain.
int clearance_count_window(dymu_ctx* c, ClearanceCall& k, bool edit, hipStream_t st,
                           uint32_t box[4], dymu_stats* stats) {
  unsigned long long* cnt = c->d_scratch + kScrObst;  // and kScrFreed behind it
  hipError_t e = hipMemsetAsync(cnt, 0, 2 * sizeof(unsigned long long), st);
  if (e == hipSuccess) e = launch_seed_mask_window(k.dF, k.a, k.win, k.blocks, st);
  if (e == hipSuccess)
    e = hipMemcpyAsync(c->h_probe, cnt, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return fail_hip(c, e, "obstacle window count");
  k.added = c->h_probe[0] != 0ull, k.freed = c->h_probe[1] != 0ull;
  if (k.freed && !edit) {
    c->last_error = "clearance update: the window frees an obstacle cell";
    return DYMU_ERR_STATE;
  }
  if (k.added || k.freed) return DYMU_OK;
  HIPC(c, hipEventRecord(c->ev1, st));
  double ms = 0.0;
  const int rc = event_ms(c, c->ev0, c->ev1, &ms);
  if (rc) return rc;
  if (box) box[0] = k.win.i0, box[1] = k.win.j0, box[2] = box[3] = 0u;
  if (stats) {
    std::memset(stats, 0, sizeof *stats);
    stats->ms = ms;
    stats->tile_w = (int)k.a.tw;
    stats->tile_h = (int)k.a.th;
    stats->kernel = k.variant;
  }
  return DYMU_OK;
}

// The raise from the window, on a domain of its own (run_raise; its statistics take the words
// of the count, which was read back), then what it claimed, before the pass domain's claims
// go to the same stamps: rt = its box {x0, y0, x1, y1} in 16x16 tiles, *raise_lo = its first stamp.
int clearance_raise(dymu_ctx* c, const ClearanceCall& k, hipStream_t st, uint32_t rt[4],
                    uint32_t* raise_lo) {
  const uint32_t ntx16 = (k.a.nx + 15u) / 16u, nty16 = (k.a.ny + 15u) / 16u;
  int rc = dom_begin(c, k.dW, k.a.T, k.a.nx, k.a.ny, (uint64_t)k.a.ld, 0, 0, -1, -1, st,
                     /*cold=*/false, /*need_keys=*/true);
  if (rc) return rc;
  *raise_lo = c->dom.eb + 1u;
  RaiseArgs ra{};
  ra.F = k.dF;  // the mask; the speed is the constant
  ra.c = k.step;
  const uint32_t win[4] = {k.win.i0, k.win.j0, k.win.i1, k.win.j1};
  rc = run_raise(c, ra, /*seeded=*/true, kScrEditStats, win, st);
  if (rc) return rc;
  const hipError_t e = claimed_box(c, ntx16 * nty16, ntx16, *raise_lo, st, rt);
  if (e == hipSuccess) return DYMU_OK;
  dom_retire(c);
  return fail_hip(c, e, "raise box");
}

// List 0 of the live pass domain (bound in k.a): the new obstacle cells, and after a raise
// the cone's boundary inside the tiles it claimed (rt, raise_lo: clearance_raise's).
hipError_t clearance_seed(dymu_ctx* c, ClearanceCall& k, const uint32_t rt[4], uint32_t raise_lo,
                          hipStream_t st) {
  auto& D = c->dom;
  MaskSeedArgs& a = k.a;
  // the edge columns belong to whatever domain ran last: from the old field (after the raise
  // wrote it), then the seeding kernel adds the new cells'
  hipError_t e = !D.a.ec ? hipSuccess : launch_ec_rebuild(a.T, (uint64_t)a.ld, a.nx, a.ny, D.a.ec,
                                                          (uint32_t)D.a.ntx, 0, D.ntiles, st);
  if (!k.freed) {  // list 0's smallest key and histogram origin: +0.0, the value of every seed
    if (e == hipSuccess) e = launch_store_u64(prio_minkey(c, 0), 0ull, st);
    if (e == hipSuccess)
      e = launch_store_u64(reinterpret_cast<unsigned long long*>(prio_base(c, 0)), 0ull, st);
    if (e == hipSuccess) e = launch_seed_mask_window(k.dF, a, k.win, k.blocks, st);
    return e;
  }
  // The cone's boundary joins the added cells in list 0, keyed with the boundary's values:
  // the keys first (they read the raise's stamps), then the claims.  theta: the smallest
  // key queued, +0.0 with an added cell; the histogram is binned from the final keys, as
  // after the single-goal raise (resolve_core).
  unsigned long long* theta = c->d_scratch + kScrTheta;
  uint32_t* hist0 = a.hist;
  a.hist = nullptr;
  ConeArgs cone{};
  cone.S = a.T;
  cone.F = k.dF;
  cone.ld = a.ld;
  cone.nx = a.nx;
  cone.ny = a.ny;
  cone.ntx16 = (a.nx + 15u) / 16u;
  cone.bx0 = rt[0], cone.by0 = rt[1];
  cone.nbx = rt[2] > rt[0] ? rt[2] - rt[0] : 0u;
  cone.nby = rt[3] > rt[1] ? rt[3] - rt[1] : 0u;
  // dom_begin restarted the epochs (its wrap guard zeroed every stamp, the raise's too):
  // every tile of the raise's box is scanned then.  The box was reduced before that, and
  // a tile the raise did not claim holds the old solve's stop at the level: a visit of it
  // writes values above the level at most, inside the box.
  cone.stamp_lo = D.eb < raise_lo ? 0u : raise_lo;
  cone.tw = a.tw, cone.th = a.th, cone.ntx = a.ntx;
  cone.list = a.list;
  cone.counts = a.counts;
  cone.shard_cap = a.shard_cap;
  cone.tile_epoch = a.tile_epoch;
  cone.epoch = a.epoch;
  cone.keys = a.keys;
  cone.theta_bits = theta;
  if (e == hipSuccess) e = launch_store_u64(theta, k.added ? 0ull : 0x7FF0000000000000ull, st);
  if (e == hipSuccess) e = launch_cone_keys(cone, k.blocks, st);
  if (e == hipSuccess && k.added) e = launch_seed_mask_window(k.dF, a, k.win, k.blocks, st);
  if (e == hipSuccess) e = launch_cone_queue(cone, st);
  if (e == hipSuccess) e = launch_theta_state(theta, prio_minkey(c, 0), prio_base(c, 0), st);
  if (e == hipSuccess)
    e = launch_rehist(D.lists[0], D.counts[0], D.ntiles, prio_keys(c, 0), prio_base(c, 0),
                      prio_delta(c), hist0, c->d_hist + (uint64_t)4 * kShards * kBins, st);
  return e;
}

// count -> raise (if cells were freed) -> pass domain -> seed -> passes -> box -> join
int clearance_window(dymu_ctx* c, const double* dF, double* dW, double* dS, uint32_t nx,
                     uint32_t ny, uint64_t ld, double step, uint32_t i0, uint32_t j0, uint32_t w,
                     uint32_t h, void* stream, uint32_t box[4], dymu_stats* stats, bool edit) {
  if (!c || !dF || !dW || !dS || nx == 0 || ny == 0 || ld < nx) return DYMU_ERR_ARG;
  if (!(step > 0.0) || !(step < __builtin_inf())) return DYMU_ERR_ARG;
  if (w == 0 || h == 0 || i0 >= nx || j0 >= ny) return DYMU_ERR_ARG;
  if (c->stepping) return DYMU_ERR_STATE;
  if (edit) std::memset(c->last_update, 0, sizeof c->last_update);
  HIPC(c, hipSetDevice(c->device));
  hipStream_t st = pick_stream(c, stream);
  HIPC(c, hipEventRecord(c->ev0, st));
  ClearanceCall k{dF, dW, step, dom_variant(c, nx, ny, /*need_keys=*/true)};
  MaskSeedArgs& a = k.a;
  a.T = dS;
  a.ld = (int64_t)ld;
  a.nx = nx;
  a.ny = ny;
  a.tw = (uint32_t)tile_w(k.variant);
  a.th = (uint32_t)tile_h(k.variant);
  a.ntx = (nx + a.tw - 1u) / a.tw;
  a.n_obst = c->d_scratch + kScrObst;
  MaskWindow& win = k.win;
  win.i0 = i0;
  win.j0 = j0;
  win.i1 = (uint32_t)std::min<uint64_t>((uint64_t)i0 + w, nx);
  win.j1 = (uint32_t)std::min<uint64_t>((uint64_t)j0 + h, ny);
  win.tx0 = i0 / a.tw;
  win.ty0 = j0 / a.th;
  win.ntwx = (win.i1 - 1u) / a.tw - win.tx0 + 1u;
  win.ntwy = (win.j1 - 1u) / a.th - win.ty0 + 1u;
  win.n_freed = c->d_scratch + kScrFreed;
  if ((uint64_t)win.ntwx * win.ntwy >= (1ull << 31)) return DYMU_ERR_ARG;  // as dom_begin's tiles
  k.blocks = (uint32_t)c->cu_count * 8u;
  int rc = clearance_count_window(c, k, edit, st, box, stats);
  if (rc || (!k.added && !k.freed)) return rc;
  uint32_t rt[4] = {0u, 0u, 0u, 0u}, raise_lo = 0u;  // no raise: an empty box
  if (k.freed && (rc = clearance_raise(c, k, st, rt, &raise_lo)) != DYMU_OK) return rc;
  // A per-pass target of one tile: every pass relaxes the lowest non-empty key bin only
  // (pass_scan's b*), so the tiles are visited in key order and none whose key lies above
  // the bin of the level is visited before the stop test sees it.  With the solves' target
  // a list shorter than the target is relaxed whole, whatever its keys: every pass then
  // lowers one more ring of tiles of a field that is +inf beyond the level, and the box
  // grows by a tile per pass (512x64 wall map, a block at column 300: 54 visits and a box
  // of 13 tiles instead of the 4 tiles within the level's reach plus their ring).
  const uint32_t saved_target = c->prio_target;
  c->prio_target = 1u;
  rc = dom_begin(c, dW, dS, nx, ny, ld, 0, 0, -1, -1, st, /*cold=*/false, /*need_keys=*/true);
  c->prio_target = saved_target;
  if (rc) return rc;
  auto& D = c->dom;
  bind_list0(c, a);  // tw, th, ntx: the domain's, which the count above anticipated
  a.ec = D.a.ec;
  win.seed = 1u;
  const uint32_t eb = D.eb, ntiles = D.ntiles, ntx = (uint32_t)D.a.ntx;
  hipError_t e = clearance_seed(c, k, rt, raise_lo, st);
  if (e != hipSuccess) {
    dom_retire(c);
    return fail_hip(c, e, "obstacle window seeding");
  }
  rc = converge_level(c, st, stats, 1.0);
  if (rc) return rc;
  // every tile a list of this domain held carries a stamp above eb; the stamps are left to
  // the next domain, whose epochs lie above them
  uint32_t t[4];
  e = claimed_box(c, ntiles, ntx, eb + 1u, st, t);
  if (e != hipSuccess) return fail_hip(c, e, "claimed-tile box");
  if (box) {
    // in cells: the pass domain's tiles (none when nothing was queued), then the raise's
    uint64_t b[4] = {~0ull, ~0ull, 0ull, 0ull};
    auto join = [&](const uint32_t q[4], uint32_t tw, uint32_t th) {
      if (q[2] == 0u) return;
      b[0] = std::min<uint64_t>(b[0], (uint64_t)q[0] * tw);
      b[1] = std::min<uint64_t>(b[1], (uint64_t)q[1] * th);
      b[2] = std::max<uint64_t>(b[2], std::min<uint64_t>((uint64_t)q[2] * tw, nx));
      b[3] = std::max<uint64_t>(b[3], std::min<uint64_t>((uint64_t)q[3] * th, ny));
    };
    join(t, a.tw, a.th);
    join(rt, 16u, 16u);
    if (b[2] == 0ull) {
      box[0] = i0, box[1] = j0, box[2] = box[3] = 0u;
    } else {
      box[0] = (uint32_t)b[0], box[1] = (uint32_t)b[1];
      box[2] = (uint32_t)(b[2] - b[0]), box[3] = (uint32_t)(b[3] - b[1]);
    }
  }
  return DYMU_OK;
}
}  // namespace

int dymu_clearance_update_device(dymu_ctx* c, const double* dF, double* dW, double* dS,
                                 uint32_t nx, uint32_t ny, uint64_t ld, double step, uint32_t i0,
                                 uint32_t j0, uint32_t w, uint32_t h, void* stream,
                                 uint32_t box[4], dymu_stats* stats) {
  return clearance_window(c, dF, dW, dS, nx, ny, ld, step, i0, j0, w, h, stream, box, stats,
                          /*edit=*/false);
}

int dymu_clearance_edit_device(dymu_ctx* c, const double* dF, double* dW, double* dS, uint32_t nx,
                               uint32_t ny, uint64_t ld, double step, uint32_t i0, uint32_t j0,
                               uint32_t w, uint32_t h, void* stream, uint32_t box[4],
                               dymu_stats* stats) {
  return clearance_window(c, dF, dW, dS, nx, ny, ld, step, i0, j0, w, h, stream, box, stats,
                          /*edit=*/true);
}

int dymu_inflate_speed_device(dymu_ctx* c, const double* dF, const double* dS, double* dOut,
                              uint32_t nx, uint32_t ny, uint64_t ld, double risk_ratio,
                              void* stream) {
  if (!c || !dF || !dS || !dOut || nx == 0 || ny == 0 || ld < nx) return DYMU_ERR_ARG;
  if (!(risk_ratio >= 0.0) || !(risk_ratio < __builtin_inf())) return DYMU_ERR_ARG;
  HIPC(c, hipSetDevice(c->device));
  HIPC(c, launch_inflate_speed(dF, dS, dOut, ld, nx, ny, risk_ratio, pick_stream(c, stream)));
  return DYMU_OK;
}

int dymu_gather_costs_device(dymu_ctx* c, const double* dT_stack, uint32_t nx, uint32_t ny,
                             uint32_t B, uint64_t ld, double res, const double* d_xy, uint32_t M,
                             double* d_out, void* stream) {
  uint32_t rows = 0;
  if (!c || !dT_stack || !batch_rows(nx, ny, B, ld, &rows)) return DYMU_ERR_ARG;
  if (!(res > 0) || !(res < HUGE_VAL) || (M && (!d_xy || !d_out))) return DYMU_ERR_ARG;
  if (M == 0) return DYMU_OK;
  HIPC(c, hipSetDevice(c->device));
  HIPC(c, launch_gather_costs(dT_stack, ld, nx, ny, B, dymu_batch_plane_rows(ny), res, d_xy, M,
                              d_out, pick_stream(c, stream)));
  return DYMU_OK;
}

/* ---- plane reduction and level mask (reduce_kernels.hip) ---- */

namespace {
// the pinned result words, the partials (one per workgroup of the largest grid, then the
// summary record, then the level mask's words) and the events
int ensure_reduce(dymu_ctx* c) {
  if (!c->ev_red_copy) HIPC(c, hipEventCreateWithFlags(&c->ev_red_copy, hipEventDisableTiming));
  if (!c->ev_red0) HIPC(c, hipEventCreate(&c->ev_red0));
  if (!c->ev_red1) HIPC(c, hipEventCreate(&c->ev_red1));
  if (!c->h_red_res) HIPC(c, hipHostMalloc(&c->h_red_res, 64, hipHostMallocDefault));
  if (!c->d_red_part) {
    c->red_blocks = (uint32_t)std::max(c->cu_count, 1) * 8u;
    HIPC(c, hipMalloc(&c->d_red_part, sizeof(ReducePartial) * (c->red_blocks + 2ull)));
  }
  return DYMU_OK;
}
// [a, a + na) and [b, b + nb) share a byte
bool ranges_overlap(const void* a, uint64_t na, const void* b, uint64_t nb) {
  const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
  return pa < pb + nb && pb < pa + na;
}
// bytes from a pitched map's first cell to the end of its last row's nx cells
uint64_t map_span(uint64_t rows, uint64_t ld, uint32_t nx, uint64_t elem) {
  return ((rows - 1) * ld + nx) * elem;
}
}  // namespace

int dymu_batch_reduce_device(dymu_ctx* c, const double* dT_stack, uint32_t nx, uint32_t ny,
                             uint32_t B, uint64_t ld, int op, const uint32_t* planes,
                             uint32_t n_planes, const double* weights, const double* offsets,
                             double* d_out, uint64_t out_ld, uint32_t* d_arg, uint64_t arg_ld,
                             dymu_reduce_summary* summary, void* stream) {
  uint32_t rows = 0;
  if (!c || !dT_stack || !d_out || !batch_rows(nx, ny, B, ld, &rows)) return DYMU_ERR_ARG;
  if (out_ld < nx || (d_arg && arg_ld < nx)) return DYMU_ERR_ARG;
  if (op != DYMU_REDUCE_SUM && op != DYMU_REDUCE_MAX && op != DYMU_REDUCE_MIN) return DYMU_ERR_ARG;
  const uint32_t n = planes ? n_planes : B;
  if (n == 0 || n > 65536u) return DYMU_ERR_ARG;
  for (uint32_t k = 0; k < n; ++k) {
    if (planes && planes[k] >= B) return DYMU_ERR_ARG;
    if (weights && (!(weights[k] > 0.0) || !(weights[k] < __builtin_inf()))) return DYMU_ERR_ARG;
    if (offsets && (!(offsets[k] >= 0.0) || !(offsets[k] < __builtin_inf()))) return DYMU_ERR_ARG;
  }
  const uint64_t stack_bytes = map_span(rows, ld, nx, sizeof(double));
  if (ranges_overlap(d_out, map_span(ny, out_ld, nx, sizeof(double)), dT_stack, stack_bytes) ||
      (d_arg && ranges_overlap(d_arg, map_span(ny, arg_ld, nx, sizeof(uint32_t)), dT_stack,
                               stack_bytes)))
    return DYMU_ERR_ARG;
  HIPC(c, hipSetDevice(c->device));
  hipStream_t st = pick_stream(c, stream);
  int rc = ensure_reduce(c);
  if (rc) return rc;
  // the previous call's copy has read the pinned list
  if (c->red_copy_pending) HIPC(c, hipEventSynchronize(c->ev_red_copy));
  c->red_copy_pending = false;
  if (n > c->red_cap) {
    const uint32_t cap = std::max<uint32_t>(n, std::max<uint32_t>(2 * c->red_cap, 64u));
    if (c->h_red_terms) HIPC(c, hipHostFree(c->h_red_terms));
    c->h_red_terms = nullptr;
    park(c, c->d_red_terms);  // a queued kernel may still read it
    c->d_red_terms = nullptr;
    c->red_cap = 0;
    HIPC(c, hipHostMalloc(&c->h_red_terms, sizeof(ReduceTerm) * cap, hipHostMallocDefault));
    HIPC(c, hipMalloc(&c->d_red_terms, sizeof(ReduceTerm) * cap));
    c->red_cap = cap;
  }
  const uint64_t plane_elems = (uint64_t)dymu_batch_plane_rows(ny) * ld;
  for (uint32_t k = 0; k < n; ++k) {
    const uint32_t p = planes ? planes[k] : k;
    c->h_red_terms[k] = ReduceTerm{p * plane_elems, weights ? weights[k] : 1.0,
                                   offsets ? offsets[k] : 0.0, p, 0u};
  }
  HIPC(c, hipMemcpyAsync(c->d_red_terms, c->h_red_terms, sizeof(ReduceTerm) * n,
                         hipMemcpyHostToDevice, st));
  HIPC(c, hipEventRecord(c->ev_red_copy, st));
  c->red_copy_pending = true;
  ReduceArgs a{};
  a.T = dT_stack;
  a.ld = ld;
  a.nx = nx;
  a.ny = ny;
  a.terms = c->d_red_terms;
  a.n = n;
  a.flags = (weights ? 1u : 0u) | (offsets ? 2u : 0u);
  a.out = d_out;
  a.out_ld = out_ld;
  a.arg = d_arg;
  a.arg_ld = arg_ld;
  a.part = summary ? c->d_red_part : nullptr;
  a.walk = tile_walk(dT_stack, ld, nx, ny);
  const uint32_t blocks = (uint32_t)std::min<uint64_t>(a.walk.ntiles, c->red_blocks);
  ReducePartial* d_sum = c->d_red_part + c->red_blocks;
  c->red_timed = false;
  HIPC(c, hipEventRecord(c->ev_red0, st));
  HIPC(c, launch_batch_reduce(a, op, blocks, d_sum, st));
  HIPC(c, hipEventRecord(c->ev_red1, st));
  c->red_timed = true;
  if (!summary) return DYMU_OK;
  HIPC(c, hipMemcpyAsync(c->h_red_res, d_sum, sizeof(ReducePartial), hipMemcpyDeviceToHost, st));
  HIPC(c, hipStreamSynchronize(st));
  ReducePartial r;
  std::memcpy(&r, c->h_red_res, sizeof r);
  std::memset(summary, 0, sizeof *summary);
  summary->min_value = r.v;
  summary->n_finite = r.n;
  summary->min_i = summary->min_j = summary->min_plane = 0xFFFFFFFFu;
  if (r.cell != ~0ull) {
    summary->min_i = (uint32_t)(r.cell % nx);
    summary->min_j = (uint32_t)(r.cell / nx);
    if (op != DYMU_REDUCE_SUM) summary->min_plane = r.arg;
  }
  return DYMU_OK;
}

int dymu_last_reduce_ms(dymu_ctx* c, double* ms) {
  return elapsed_ms(c, &dymu_ctx::red_timed, &dymu_ctx::ev_red0, &dymu_ctx::ev_red1, ms);
}

int dymu_level_mask_device(dymu_ctx* c, const double* d_map, uint32_t nx, uint32_t ny, uint64_t ld,
                           double bound, uint8_t* d_mask, uint64_t mask_ld, dymu_region* out,
                           void* stream) {
  if (!c || !d_map || !d_mask || nx == 0 || ny == 0 || ld < nx || mask_ld < nx)
    return DYMU_ERR_ARG;
  if (!(bound > -__builtin_inf()) || !(bound < __builtin_inf())) return DYMU_ERR_ARG;
  HIPC(c, hipSetDevice(c->device));
  hipStream_t st = pick_stream(c, stream);
  int rc = ensure_reduce(c);
  if (rc) return rc;
  const TileWalk walk = tile_walk(d_map, ld, nx, ny);
  const uint32_t blocks = (uint32_t)std::min<uint64_t>(walk.ntiles, c->red_blocks);
  uint32_t* box = reinterpret_cast<uint32_t*>(c->d_red_part + c->red_blocks + 1);
  unsigned long long* cnt = reinterpret_cast<unsigned long long*>(box + 4);
  if (out) {
    HIPC(c, hipMemsetAsync(box, 0xFF, 2 * sizeof(uint32_t), st));
    HIPC(c, hipMemsetAsync(box + 2, 0, 2 * sizeof(uint32_t) + sizeof(unsigned long long), st));
  }
  HIPC(c, launch_level_mask(d_map, ld, nx, ny, bound, d_mask, mask_ld, walk, blocks,
                            out ? box : nullptr, cnt, st));
  if (!out) return DYMU_OK;
  char* h = static_cast<char*>(c->h_red_res) + 32;
  HIPC(c, hipMemcpyAsync(h, box, 24, hipMemcpyDeviceToHost, st));
  HIPC(c, hipStreamSynchronize(st));
  uint32_t b[4];
  unsigned long long m = 0;
  std::memcpy(b, h, sizeof b);
  std::memcpy(&m, h + 16, sizeof m);
  std::memset(out, 0, sizeof *out);
  out->n_range = m;
  if (m == 0) {  // no cell at or below the bound
    out->i0 = 1;
    return DYMU_OK;
  }
  out->i0 = b[0], out->j0 = b[1], out->i1 = b[2], out->j1 = b[3];
  return DYMU_OK;
}

/* ---- windowed updates of seeded maps and of stacks ---- */

int dymu_update_seeds_window_device(dymu_ctx* c, const double* dF, double* dT, uint32_t nx,
                                    uint32_t ny, uint64_t ld, const dymu_seed* seeds,
                                    uint32_t n_seeds, uint32_t i0, uint32_t j0, uint32_t w,
                                    uint32_t h, int decrease_only, void* stream,
                                    dymu_stats* stats) {
  if (!c || !dF || !dT || !seeds || nx == 0 || ny == 0 || ld < nx || n_seeds == 0 ||
      n_seeds >= (1u << 31))
    return DYMU_ERR_ARG;
  for (uint32_t k = 0; k < n_seeds; ++k) {
    const dymu_seed& s = seeds[k];
    if (s.i >= nx || s.j >= ny || !(s.t0 >= 0.0) || !(s.t0 < __builtin_inf())) return DYMU_ERR_ARG;
  }
  BatchWindow win;
  if (!clip_window(0, i0, j0, w, h, nx, ny, &win)) return DYMU_ERR_ARG;
  HIPC(c, hipSetDevice(c->device));
  return update_planes_core(c, dF, dT, nx, ny, 1, ny, ld, seeds, n_seeds, &win, 1,
                            decrease_only != 0, pick_stream(c, stream), stats);
}

int dymu_update_batch_window_device(dymu_ctx* c, const double* dF_stack, double* dT_stack,
                                    uint32_t nx, uint32_t ny, uint32_t B, uint64_t ld,
                                    const dymu_batch_seed* seeds, uint32_t n_seeds,
                                    const dymu_batch_window* windows, uint32_t n_windows,
                                    int decrease_only, void* stream, dymu_stats* stats) {
  uint32_t rows = 0;
  if (!c || !dF_stack || !dT_stack || !seeds || n_seeds == 0 || n_seeds >= (1u << 31) ||
      !windows || n_windows == 0 || n_windows >= (1u << 31) || !batch_rows(nx, ny, B, ld, &rows))
    return DYMU_ERR_ARG;
  const uint32_t P = dymu_batch_plane_rows(ny);
  std::vector<dymu_seed> s(n_seeds);
  std::vector<uint8_t> seeded(B, 0);
  for (uint32_t k = 0; k < n_seeds; ++k) {
    const dymu_batch_seed& b = seeds[k];
    if (b.plane >= B || b.i >= nx || b.j >= ny || !(b.t0 >= 0.0) || !(b.t0 < __builtin_inf()))
      return DYMU_ERR_ARG;
    seeded[b.plane] = 1;
    s[k] = dymu_seed{b.i, b.plane * P + b.j, b.t0};
  }
  for (uint32_t b = 0; b < B; ++b)
    if (!seeded[b]) return DYMU_ERR_ARG;
  std::vector<BatchWindow> wv(n_windows);
  for (uint32_t k = 0; k < n_windows; ++k) {
    const dymu_batch_window& q = windows[k];
    if (q.plane >= B || !clip_window(q.plane, q.i0, q.j0, q.w, q.h, nx, ny, &wv[k]))
      return DYMU_ERR_ARG;
  }
  HIPC(c, hipSetDevice(c->device));
  return update_planes_core(c, dF_stack, dT_stack, nx, ny, B, P, ld, s.data(), n_seeds, wv.data(),
                            n_windows, decrease_only != 0, pick_stream(c, stream), stats);
}

int dymu_goal_labels_device(dymu_ctx* c, const double* dT, uint32_t nx, uint32_t ny, uint64_t ld,
                            const dymu_seed* seeds, uint32_t n_seeds, uint32_t* d_label,
                            void* stream, uint32_t* rounds) {
  if (!c) return DYMU_ERR_ARG;
  HIPC(c, hipSetDevice(c->device));
  return goal_labels_core(c, dT, nx, ny, ld, seeds, n_seeds, d_label, pick_stream(c, stream),
                          rounds);
}

int dymu_last_labels_ms(dymu_ctx* c, double* ms) {
  return elapsed_ms(c, &dymu_ctx::lab_timed, &dymu_ctx::ev_lab0, &dymu_ctx::ev_lab1, ms);
}

int dymu_last_paths_ms(dymu_ctx* c, double* ms) {
  if (!c || !ms) return DYMU_ERR_ARG;
  if (!c->path_timed) return DYMU_ERR_STATE;
  HIPC(c, hipSetDevice(c->device));
  HIPC(c, hipEventSynchronize(c->ev_path1));
  float f = 0.0f;
  HIPC(c, hipEventElapsedTime(&f, c->ev_path0, c->ev_path1));
  *ms = (double)f;
  return DYMU_OK;
}

int dymu_memcpy2d_d2h(dymu_ctx* c, void* dst, size_t dpitch, const void* src, size_t spitch,
                      size_t width, size_t height) {
  if (!c || !dst || !src) return DYMU_ERR_ARG;
  HIPC(c, hipSetDevice(c->device));
  HIPC(c, hipMemcpy2DAsync(dst, dpitch, src, spitch, width, height, hipMemcpyDeviceToHost,
                           c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));
  return DYMU_OK;
}

int dymu_memcpy2d_h2d(dymu_ctx* c, void* dst, size_t dpitch, const void* src, size_t spitch,
                      size_t width, size_t height) {
  if (!c || !dst || !src) return DYMU_ERR_ARG;
  HIPC(c, hipSetDevice(c->device));
  HIPC(c, hipMemcpy2DAsync(dst, dpitch, src, spitch, width, height, hipMemcpyHostToDevice,
                           c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));
  return DYMU_OK;
}

int dymu_host_register(dymu_ctx* c, void* p, size_t bytes) {
  if (!c || !p || bytes == 0) return DYMU_ERR_ARG;
  HIPC(c, hipSetDevice(c->device));
  HIPC(c, hipHostRegister(p, bytes, hipHostRegisterDefault));
  return DYMU_OK;
}

int dymu_host_unregister(dymu_ctx* c, void* p) {
  if (!c || !p) return DYMU_ERR_ARG;
  HIPC(c, hipSetDevice(c->device));
  HIPC(c, hipHostUnregister(p));
  return DYMU_OK;
}

int dymu_resolve_window_device(dymu_ctx* c, const double* dF, double* dT, uint32_t nx,
                               uint32_t ny, uint64_t ld, uint32_t gi, uint32_t gj, uint32_t i0,
                               uint32_t j0, uint32_t w, uint32_t h, void* stream,
                               dymu_stats* stats) {
  if (!c || !dF || !dT || nx == 0 || ny == 0 || ld < nx) return DYMU_ERR_ARG;
  HIPC(c, hipSetDevice(c->device));
  w = (uint32_t)std::min<uint64_t>(w, nx > i0 ? nx - i0 : 0);
  h = (uint32_t)std::min<uint64_t>(h, ny > j0 ? ny - j0 : 0);
  return resolve_core(c, dF, dT, nx, ny, ld, gi, gj, i0, j0, w, h, pick_stream(c, stream), stats);
}

int dymu_update_window_device(dymu_ctx* c, const double* dF, double* dT, uint32_t nx,
                              uint32_t ny, uint64_t ld, uint32_t gi, uint32_t gj, uint32_t i0,
                              uint32_t j0, uint32_t w, uint32_t h, int decrease_only, void* stream,
                              dymu_stats* stats) {
  if (!c || !dF || !dT || nx == 0 || ny == 0 || ld < nx) return DYMU_ERR_ARG;
  HIPC(c, hipSetDevice(c->device));
  w = (uint32_t)std::min<uint64_t>(w, nx > i0 ? nx - i0 : 0);
  h = (uint32_t)std::min<uint64_t>(h, ny > j0 ? ny - j0 : 0);
  return resolve_core(c, dF, dT, nx, ny, ld, gi, gj, i0, j0, w, h, pick_stream(c, stream), stats,
                      decrease_only != 0);
}

int dymu_resolve_window(dymu_ctx* c, const double* F, uint32_t nx, uint32_t ny, uint32_t gi,
                        uint32_t gj, uint32_t i0, uint32_t j0, uint32_t w, uint32_t h,
                        double* T_out, dymu_stats* stats) {
  if (!c || !F || !T_out || nx == 0 || ny == 0) return DYMU_ERR_ARG;
  if (c->stepping) return DYMU_ERR_STATE;
  if (!c->host_valid || c->host_nx != nx || c->host_ny != ny || c->host_gi != gi ||
      c->host_gj != gj) {
    c->last_error = "dymu_resolve_window: no previous dymu_solve of this grid and goal";
    return DYMU_ERR_STATE;
  }
  if (i0 >= nx || j0 >= ny || w == 0 || h == 0) return DYMU_ERR_ARG;
  HIPC(c, hipSetDevice(c->device));
  w = (uint32_t)std::min<uint64_t>(w, nx - i0);
  h = (uint32_t)std::min<uint64_t>(h, ny - j0);
  c->host_valid = false;
  // only the window of F changed: upload those rows' columns
  const uint64_t off = (uint64_t)j0 * nx + i0;
  HIPC(c, hipMemcpy2DAsync(c->d_F + off, sizeof(double) * nx, F + off, sizeof(double) * nx,
                           sizeof(double) * w, h, hipMemcpyHostToDevice, c->stream));
  int rc = resolve_core(c, c->d_F, c->d_T, nx, ny, nx, gi, gj, i0, j0, w, h, c->stream, stats);
  if (rc) return rc;
  const uint64_t cells = (uint64_t)nx * ny;
  HIPC(c, hipMemcpyAsync(T_out, c->d_T, sizeof(double) * cells, hipMemcpyDeviceToHost, c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));
  c->host_valid = true;
  return DYMU_OK;
}

int dymu_synth_speed(dymu_ctx* c, double* dF, uint32_t nx, uint32_t ny, uint64_t ld, uint64_t row0,
                     uint64_t seed, double obst_frac, uint64_t obst_seed, uint32_t gi, uint32_t gj,
                     void* stream) {
  if (!c || !dF || ld < nx) return DYMU_ERR_ARG;
  HIPC(c, hipSetDevice(c->device));
  hipStream_t st = pick_stream(c, stream);
  HIPC(c, launch_synth(dF, ld, nx, ny, row0, seed, obst_frac, obst_seed, gi, gj, st));
  HIPC(c, hipStreamSynchronize(st));
  return DYMU_OK;
}

int dymu_device_alloc(dymu_ctx* c, size_t bytes, void** p) {
  if (!c || !p) return DYMU_ERR_ARG;
  HIPC(c, hipSetDevice(c->device));
  HIPC(c, dev_alloc(p, bytes, c->map_mem));
  return DYMU_OK;
}

int dymu_device_alloc_cached(dymu_ctx* c, size_t bytes, void** p) {
  if (!c || !p) return DYMU_ERR_ARG;
  HIPC(c, hipSetDevice(c->device));
  HIPC(c, dev_alloc(p, bytes, 0));
  return DYMU_OK;
}

int dymu_device_free(dymu_ctx* c, void* p) {
  if (!c) return DYMU_ERR_ARG;
  HIPC(c, hipSetDevice(c->device));
  HIPC(c, hipFree(p));
  return DYMU_OK;
}

int dymu_memcpy_d2h(dymu_ctx* c, void* dst, const void* src, size_t bytes) {
  if (!c) return DYMU_ERR_ARG;
  HIPC(c, hipSetDevice(c->device));
  // ordered after the work queued on the context stream, complete on return
  HIPC(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));
  return DYMU_OK;
}

int dymu_memcpy_h2d(dymu_ctx* c, void* dst, const void* src, size_t bytes) {
  if (!c) return DYMU_ERR_ARG;
  HIPC(c, hipSetDevice(c->device));
  HIPC(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));
  return DYMU_OK;
}

int dymu_dom_begin(dymu_ctx* c, const dymu_domain* d, int64_t goal_i, int64_t goal_j_local,
                   void* stream) {
  if (!c || !d) return DYMU_ERR_ARG;
  HIPC(c, hipSetDevice(c->device));
  return dom_begin(c, d->F, d->T, d->nx, d->nrows, d->ld, d->ghost_lo, d->ghost_hi, goal_i,
                   goal_j_local, pick_stream(c, stream));
}

int dymu_dom_run(dymu_ctx* c, uint32_t passes, void* stream) {
  if (!c) return DYMU_ERR_ARG;
  HIPC(c, hipSetDevice(c->device));
  return dom_launch(c, passes, pick_stream(c, stream));
}

int dymu_dom_merge_ghosts(dymu_ctx* c, const double* new_lo, const double* new_hi,
                          int32_t* d_pending, void* stream) {
  if (!c) return DYMU_ERR_ARG;
  HIPC(c, hipSetDevice(c->device));
  return dom_merge(c, new_lo, new_hi, d_pending, pick_stream(c, stream));
}

int dymu_dom_exchange(dymu_ctx* c, const double* new_lo, const double* new_hi,
                      int32_t* d_total, void* stream) {
  if (!c) return DYMU_ERR_ARG;
  HIPC(c, hipSetDevice(c->device));
  return dom_exchange(c, new_lo, new_hi, d_total, pick_stream(c, stream));
}

int dymu_dom_round_supported(dymu_ctx* c, uint32_t passes) {
  return c && dom_round_ok(c, passes) ? 1 : 0;
}

int dymu_dom_round_capable(dymu_ctx* c, uint32_t nx, uint32_t nrows, uint32_t passes) {
  if (!c || nx == 0 || nrows == 0) return 0;
  return dom_variant(c, nx, nrows, false) == 5 && passes >= 2 && !c->opts.deterministic ? 1 : 0;
}

int dymu_dom_round(dymu_ctx* c, uint32_t passes, const double* new_lo, const double* new_hi,
                   int32_t* d_total, void* stream) {
  if (!c) return DYMU_ERR_ARG;
  HIPC(c, hipSetDevice(c->device));
  return dom_round(c, passes, new_lo, new_hi, d_total, pick_stream(c, stream));
}

int dymu_dom_round_peer(dymu_ctx* c, uint32_t passes, const dymu_peer_links* links,
                        void* stream) {
  if (!c || !links) return DYMU_ERR_ARG;
  static_assert(sizeof(PeerCtl) <= DYMU_PEER_CTL_BYTES, "peer control block");
  // the initial state include/dymu_fim.h documents: zeros, bytes 32 .. 47 all ones
  static_assert(offsetof(PeerCtl, rmin) == 32 && sizeof(PeerCtl::rmin) == 16, "documented rmin");
  HIPC(c, hipSetDevice(c->device));
  return dom_round_peer(c, passes, *links, pick_stream(c, stream));
}

int dymu_dom_post_status(dymu_ctx* c, const void* ctl, unsigned long long* dst, uint32_t seq) {
  if (!c || !ctl || !dst || seq == 0) return DYMU_ERR_ARG;
  if (!c->dom.live) return DYMU_ERR_STATE;
  const PeerCtl* pc = static_cast<const PeerCtl*>(ctl);
  c->arm_src = reinterpret_cast<const int32_t*>(&pc->pend);
  c->arm_ext = pc->ext;
  c->arm_dst = dst;
  c->arm_seq = seq;
  return DYMU_OK;
}

int dymu_dom_post(dymu_ctx* c, const int32_t* d_src, uint32_t* seq) {
  if (!c || !d_src || !seq) return DYMU_ERR_ARG;
  if (!c->d_mail || !c->dom.live) return DYMU_ERR_STATE;
  if (++c->mail_seq == 0) c->mail_seq = 1;
  c->arm_dst = nullptr;
  c->arm_ext = nullptr;
  c->arm_src = d_src;
  c->arm_seq = c->mail_seq;
  *seq = c->mail_seq;
  return DYMU_OK;
}

int dymu_dom_wait_post(dymu_ctx* c, uint32_t seq, double timeout_s, int32_t* value,
                       void* stream) {
  if (!c || !value || seq == 0) return DYMU_ERR_ARG;
  if (!c->d_mail) return DYMU_ERR_STATE;
  uint32_t v = 0;
  const int rc = wait_mail(c, pick_stream(c, stream), seq, &v, nullptr, timeout_s);
  if (rc) return rc;
  *value = (int32_t)v;
  return DYMU_OK;
}

int dymu_dom_pending(dymu_ctx* c, void* stream, uint64_t* pending) {
  if (!c || !pending) return DYMU_ERR_ARG;
  HIPC(c, hipSetDevice(c->device));
  return dom_pending(c, pick_stream(c, stream), pending);
}

int dymu_set_stepping(dymu_ctx* c, int on) {
  if (!c) return DYMU_ERR_ARG;
  c->stepping = on != 0;
  return DYMU_OK;
}

int dymu_dom_min_key(dymu_ctx* c, void* stream, double* key) {
  if (!c || !key) return DYMU_ERR_ARG;
  auto& D = c->dom;
  if (!D.live || !is_prio(D.variant)) return DYMU_ERR_STATE;
  HIPC(c, hipSetDevice(c->device));
  hipStream_t st = pick_stream(c, stream);
  HIPC(c, hipMemcpyAsync(c->h_probe, prio_minkey(c, D.p % 3), sizeof(unsigned long long),
                         hipMemcpyDeviceToHost, st));
  HIPC(c, hipStreamSynchronize(st));
  std::memcpy(key, &c->h_probe[0], sizeof *key);
  return DYMU_OK;
}

int dymu_dom_snapshot(dymu_ctx* c, void* stream, dymu_dom_state* s) {
  if (!c || !s) return DYMU_ERR_ARG;
  auto& D = c->dom;
  if (!D.live) return DYMU_ERR_STATE;
  HIPC(c, hipSetDevice(c->device));
  hipStream_t st = pick_stream(c, stream);
  HIPC(c, hipStreamSynchronize(st));
  const uint32_t nt = D.ntiles;
  const bool keys = is_prio(D.variant);
  s->eb = D.eb;
  s->ntiles = nt;
  s->tiles_cap = c->tiles_cap;
  s->variant = D.variant;
  s->p = D.p;
  s->F = D.a.F;
  s->T = D.a.T;
  s->ld = (uint64_t)D.a.ld;
  s->nx = (uint32_t)D.a.nx;
  s->ny = (uint32_t)D.a.ny;
  s->has_keys = keys ? 1 : 0;
  s->has_ec = D.a.ec ? 1 : 0;
  if ((s->tile_epoch && s->tile_epoch_cap < c->tiles_cap) ||
      (s->keys && keys && s->keys_cap < 3ull * nt) || (s->ec && D.a.ec && s->ec_cap < 32ull * nt))
    return DYMU_ERR_ARG;
  auto d2h = [&](void* dst, const void* src, size_t bytes) {
    return bytes ? hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost) : hipSuccess;
  };
  uint32_t cnt[3 * kShards];
  HIPC(c, d2h(cnt, c->d_counts, sizeof cnt));
  if (s->counts) std::memcpy(s->counts, cnt, sizeof cnt);
  const uint32_t* cin = cnt + (D.p % 3) * kShards;
  s->list_n = 0;
  for (int q = 0; q < kShards; ++q) {
    if (cin[q] > nt) {
      c->last_error = "snapshot: a shard counter exceeds the shard's capacity";
      return DYMU_ERR_STATE;
    }
    s->list_n += cin[q];
  }
  if (s->list_raw || s->list_tile) {
    if (s->list_cap < s->list_n) return DYMU_ERR_ARG;
    std::vector<uint32_t> tmp;
    uint32_t* raw = s->list_raw;
    if (!raw) {
      tmp.resize((size_t)s->list_n);
      raw = tmp.data();
    }
    uint64_t at = 0;
    for (int q = 0; q < kShards; ++q) {
      HIPC(c, d2h(raw + at, D.lists[D.p % 3] + (uint64_t)q * nt, sizeof(uint32_t) * cin[q]));
      at += cin[q];
    }
    if (s->list_tile)
      for (uint64_t k = 0; k < s->list_n; ++k) s->list_tile[k] = raw[k] & kTileMask;
  }
  if (s->tile_epoch)
    HIPC(c, d2h(s->tile_epoch, c->d_tile_epoch, sizeof(uint32_t) * (size_t)c->tiles_cap));
  std::memset(s->minkey, 0, sizeof s->minkey);
  std::memset(s->base, 0, sizeof s->base);
  s->delta = 0.0;
  if (keys) {
    unsigned long long pr[8];
    HIPC(c, d2h(pr, c->d_prio, sizeof pr));
    std::memcpy(s->minkey, pr, sizeof s->minkey);
    std::memcpy(s->base, pr + 3, sizeof s->base);
    std::memcpy(&s->delta, pr + 6, sizeof s->delta);
    if (s->keys) HIPC(c, d2h(s->keys, c->d_keys, sizeof(unsigned long long) * 3 * (size_t)nt));
    if (s->hist) HIPC(c, d2h(s->hist, c->d_hist, sizeof(uint32_t) * 3 * kShards * kBins));
  }
  if (s->ec && D.a.ec) HIPC(c, d2h(s->ec, D.a.ec, sizeof(double) * 32 * (size_t)nt));
  return DYMU_OK;
}

int dymu_debug_raise_epoch_base(dymu_ctx* c, uint32_t value) {
  if (!c) return DYMU_ERR_ARG;
  if (c->dom.live) return DYMU_ERR_STATE;
  c->epoch_base = std::max(c->epoch_base, value);
  return DYMU_OK;
}

int dymu_dom_finish(dymu_ctx* c, void* stream, dymu_stats* stats) {
  if (!c) return DYMU_ERR_ARG;
  HIPC(c, hipSetDevice(c->device));
  return dom_finish(c, pick_stream(c, stream), stats, 0.0);
}

int dymu_slab_rows(uint32_t ny, uint32_t nranks, uint32_t rank, uint32_t* row0, uint32_t* nrows) {
  if (!row0 || !nrows || nranks == 0 || rank >= nranks) return DYMU_ERR_ARG;
  // slab boundaries on multiples of 32 rows (a whole number of tile rows for
  // every kernel variant), so every slab but the last satisfies ghost_hi.
  const uint32_t A = 32;
  const uint64_t blocks = ((uint64_t)ny + A - 1) / A;
  const uint64_t b0 = blocks * rank / nranks, b1 = blocks * (rank + 1) / nranks;
  uint64_t r0 = b0 * A, r1 = b1 * A;
  if (r1 > ny) r1 = ny;
  if (r0 > ny) r0 = ny;
  *row0 = (uint32_t)r0;
  *nrows = (uint32_t)(r1 - r0);
  return DYMU_OK;
}

int dymu_eikonal_batch(dymu_ctx* c, const double* tx, const double* ty, const double* cc,
                       double* out, uint64_t n, int fast) {
  if (!c || !tx || !ty || !cc || !out) return DYMU_ERR_ARG;
  HIPC(c, hipSetDevice(c->device));
  HIPC(c, launch_eikonal_batch(tx, ty, cc, out, n, fast, c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));
  return DYMU_OK;
}

int dymu_pass_scan_probe(dymu_ctx* c, const uint32_t* counts, const uint32_t* hist,
                         uint32_t target, float target_frac, float cap_frac, uint32_t* prefix,
                         int32_t* bstar) {
  if (!c || !counts || !hist || !prefix || !bstar) return DYMU_ERR_ARG;
  HIPC(c, hipSetDevice(c->device));
  constexpr size_t n_in = kShards + (size_t)kShards * kBins, n_out = kShards + 2;
  uint32_t* d = nullptr;
  HIPC(c, hipMalloc(&d, sizeof(uint32_t) * (n_in + n_out)));
  uint32_t out[n_out];
  hipError_t e = hipMemcpyAsync(d, counts, sizeof(uint32_t) * kShards, hipMemcpyHostToDevice,
                                c->stream);
  if (e == hipSuccess)
    e = hipMemcpyAsync(d + kShards, hist, sizeof(uint32_t) * kShards * kBins,
                       hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess)
    e = launch_pass_scan_probe(d, d + kShards, target, target_frac, cap_frac, d + n_in, c->stream);
  if (e == hipSuccess)
    e = hipMemcpyAsync(out, d + n_in, sizeof out, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  (void)hipFree(d);
  HIPC(c, e);
  std::memcpy(prefix, out, sizeof(uint32_t) * (kShards + 1));
  *bstar = (int32_t)out[kShards + 1];
  return DYMU_OK;
}

namespace {
dymu::CostState cost_state(const dymu_cost_state* s) {
  return dymu::CostState{s->cost,        s->raw_cost, s->slope, s->terrain,
                         s->is_obstacle, s->hazard,   s->traff, s->loc_mode};
}
bool cost_state_ok(const dymu_cost_state* s) {
  return s && s->cost && s->raw_cost && s->slope && s->terrain && s->is_obstacle && s->hazard &&
         s->traff && s->loc_mode;
}
}  // namespace

int dymu_compute_cost_map(dymu_ctx* c, uint32_t nx, uint32_t ny, uint64_t ld, double global_res,
                          const double* lut, int lut_len, const double* slopes, int n_slopes,
                          int n_locs, const double* elevation, const double* terrain_map,
                          const dymu_cost_state* st, double* dF, void* stream) {
  if (!c || !lut || lut_len <= 0 || !slopes || n_slopes <= 0 || n_locs <= 0 || !elevation ||
      !terrain_map || !cost_state_ok(st) || nx < 2 || ny < 2 || ld < nx || !(global_res > 0))
    return DYMU_ERR_ARG;
  HIPC(c, hipSetDevice(c->device));
  hipStream_t s = pick_stream(c, stream);
  if ((size_t)lut_len > c->lut_cap) {
    if (c->d_lut) HIPC(c, hipFree(c->d_lut));
    c->d_lut = nullptr;
    c->lut_cap = 0;
    HIPC(c, hipMalloc(&c->d_lut, sizeof(double) * (size_t)lut_len));
    c->lut_cap = (size_t)lut_len;
  }
  // the previous launch reading d_lut must be done before it is overwritten
  HIPC(c, hipStreamSynchronize(s));
  HIPC(c, hipMemcpy(c->d_lut, lut, sizeof(double) * (size_t)lut_len, hipMemcpyHostToDevice));
  dymu::CostArgs a{};
  a.nx = nx;
  a.ny = ny;
  a.ld = (int64_t)ld;
  a.res = global_res;
  a.cmax = lut[0];  // std::max_element (:221)
  for (int k = 1; k < lut_len; ++k)
    if (a.cmax < lut[k]) a.cmax = lut[k];
  a.slope_lo = slopes[0];
  a.slope_hi = slopes[n_slopes - 1];
  a.n_slopes = n_slopes;
  a.n_locs = n_locs;
  a.lut_len = lut_len;
  a.lut = c->d_lut;
  a.elevation = elevation;
  a.terrain_map = terrain_map;
  a.st = cost_state(st);
  a.F = dF;
  HIPC(c, dymu::launch_cost_map(a, s));
  return DYMU_OK;
}

int dymu_pack_speed(dymu_ctx* c, uint32_t nx, uint32_t ny, uint64_t ld, double global_res,
                    const dymu_cost_state* st, double* dF, void* stream) {
  if (!c || !cost_state_ok(st) || !dF || nx == 0 || ny == 0 || ld < nx) return DYMU_ERR_ARG;
  HIPC(c, hipSetDevice(c->device));
  dymu::CostArgs a{};
  a.nx = nx;
  a.ny = ny;
  a.ld = (int64_t)ld;
  a.res = global_res;
  a.st = cost_state(st);
  a.F = dF;
  HIPC(c, dymu::launch_pack_speed(a, pick_stream(c, stream)));
  return DYMU_OK;
}

int dymu_last_update_stats(dymu_ctx* c, uint64_t out[4]) {
  if (!c || !out) return DYMU_ERR_ARG;
  std::memcpy(out, c->last_update, sizeof c->last_update);
  return DYMU_OK;
}

int dymu_set_pass_stats(dymu_ctx* c, int enable) {
  if (!c) return DYMU_ERR_ARG;
  c->pass_stats = enable != 0;
  return DYMU_OK;
}

int dymu_last_pass_stats(dymu_ctx* c, uint32_t* out, uint64_t cap, uint64_t* n) {
  if (!c || !n || (cap && !out)) return DYMU_ERR_ARG;
  *n = 0;
  if (!c->d_pstat || !c->pass_stats) return DYMU_ERR_STATE;
  HIPC(c, hipSetDevice(c->device));
  const uint64_t passes = std::min<uint64_t>(c->last_launches, kPassStatCap);
  *n = passes;
  const uint64_t m = std::min(passes, cap);
  if (!m) return DYMU_OK;
  std::vector<uint32_t> h((size_t)m * kShards * kPsWords);
  HIPC(c, hipMemcpy(h.data(), c->d_pstat, sizeof(uint32_t) * h.size(), hipMemcpyDeviceToHost));
  for (uint64_t p = 0; p < m; ++p) {
    uint32_t* o = out + p * kPsWords;
    std::memset(o, 0, sizeof(uint32_t) * kPsWords);
    for (int q = 0; q < kShards; ++q) {
      const uint32_t* r = &h[(p * kShards + q) * kPsWords];
      for (int w = 0; w < kPsWords; ++w) {
        if (w == kPsRadiusMax || w == kPsRadiusMin) o[w] = std::max(o[w], r[w]);
        else o[w] += r[w];
      }
    }
    o[kPsRadiusMin] = o[kPsRadiusMin] ? ~o[kPsRadiusMin] : 0u;  // stored as ~radius
  }
  return DYMU_OK;
}

int dymu_set_profiling(dymu_ctx* c, int period) {
  if (!c || period < 0) return DYMU_ERR_ARG;
  c->profiling = period;
  return DYMU_OK;
}

int dymu_last_pass_timing(dymu_ctx* c, double* ms, uint64_t* n) {
  if (!c) return DYMU_ERR_ARG;
  if (ms) *ms = c->last_pass_ms;
  if (n) *n = c->last_timed;
  return DYMU_OK;
}

}  // extern "C"
