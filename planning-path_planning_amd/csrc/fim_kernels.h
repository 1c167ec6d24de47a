// fim_kernels.h -- internal interface between the HIP kernels and the
// C-ABI runtime (dymu_fim.cpp).  Not installed; not part of the C-ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dymu {

constexpr int kWaveTile = 8;  // kernels 3/4: 8x8 tiles, two per 64-lane wave (half-wave each)
constexpr int kShards = 16;   // active lists are split in shards to spread the append atomics

enum StatSlot : int {
  kStatPasses = 0,
  kStatVisits = 1,
  kStatSweeps = 2,
  kStatMaxActive = 3,
  kStatDeferred = 4,
  kStatSlots = 8
};

struct ProbeCells {
  int64_t ij[5][2];  // (i, j) of the start cell and its in-grid 4-neighbours
  int n;
};

// Counters of the peer rounds (dymu_dom_round_peer, DESIGN.md s5 "Peer transport"),
// in the rank's own device memory, zeroed at the start of a solve (rmin: all ones).
// side 0 = the link to rank-1, side 1 = the link to rank+1.
struct PeerCtl {
  uint32_t done[2];               // workgroups that finished this pass's push of a side
  uint32_t changed[2];            // some pushed column of the side decreased this pass
  unsigned long long sent[2];     // S: pushes that carried a decrease (= the tags written)
  unsigned long long rmin[2];     // smallest tag a merging workgroup read this round
  unsigned long long merged[2];   // R: the tag of the last complete merge (status pass)
  uint32_t pend;                  // P: tiles queued for the round's first + second pass
  uint32_t pad;
  unsigned long long ext[4];      // the posted status: S0, S1, R0, R1 (with pend)
};

struct PassArgs {
  const double* F;  // speed, pitch ld
  double* T;        // total cost, pitch ld (row -1 / row ny are ghost rows when flagged)
  int64_t ld;
  int64_t nx, ny;   // local domain
  int ntx, nty;     // tiles
  // kernel 5: tile / ntx = (tile * ntx_mul) >> ntx_shift for every tile < 2^25 (tile_div)
  uint32_t ntx_mul, ntx_shift;
  int ghost_lo;     // row -1 exists in memory (read-only halo)
  int ghost_hi;     // row ny exists in memory (requires ny % tile height == 0)
  int max_inner;    // cap on in-tile sweeps per visit
  uint32_t epoch;   // epoch stamped on tiles enqueued for the NEXT pass
  uint32_t shard_cap;  // capacity of one shard (= number of tiles)
  const uint32_t* list_in;   // kShards shards of shard_cap entries
  const uint32_t* count_in;  // kShards counters
  uint32_t* list_out;
  uint32_t* count_out;
  uint32_t* count_clear;
  uint32_t* tile_epoch;
  unsigned long long* stats;  // kShards x kStatSlots
  // ---- v4 (priority passes) only ----
  unsigned long long* key_in;   // per-tile key of list p (double bits), reset to +inf by its reader
  unsigned long long* key_out;  // keys of list p+1 (atomicMin)
  const uint32_t* hist_in;      // kShards x kBins key histogram of list p
  uint32_t* hist_out;           // ... of list p+1
  uint32_t* hist_clear;         // ... of list p+2 (zeroed by block 0)
  const unsigned long long* minkey_in;  // min key of list p
  unsigned long long* minkey_out;
  unsigned long long* minkey_clear;
  const double* base_in;  // histogram origin of list p
  double* base_out;       // ... of list p+1 (= min key of list p, written by block 0)
  const double* delta;    // histogram bin width, and in delta[1] its reciprocal (k_prio_init)
  uint32_t target;        // tiles to relax per pass; 0 = all (plain FIM)
  float target_frac;      // ... at least this fraction of the active list
  float cap_frac;         // kernel 5: ... and at most this fraction (>= 256 tiles); 0 = off
  int prune;              // activate a neighbour only through edge cells below its halo value
  unsigned long long* trace;  // debug: kTracePts s_memrealtime stamps per block, or null
  uint32_t sweep_deadline;  // kernel 5 (dyn): > 0: a visit stops sweeping this many 10-ns ticks
                            // after its workgroup started the pass (re-queued as if capped)
  int checker;              // kernel 5: relax only tiles with (tx + ty + checker_parity) even
  uint32_t checker_parity;  // (deterministic mode: no tile reads a halo being written)
  int exact_sqrt;  // kernel 5 (dyn): 1 = correctly rounded sweep sqrt (10 VALU), 0 = one
                   // Goldschmidt step (5 VALU, <= 36 ulp)
  // convergence mailbox: when set, block 0 stores (report_seq << 32) | n_active -- the
  // tiles queued by the previous pass -- into this word of host-coherent pinned memory,
  // so the host learns a batch's outcome without a stream synchronisation
  unsigned long long* report;
  uint32_t report_seq;
  const int32_t* report_src;  // post *report_src instead of the pass's count (sharded loop)
  // with report_src: these 4 words are stored at report[1..4] before the (seq | count)
  // word at report[0] (a fresh slot per post: the peer loop's status ring)
  const unsigned long long* report_ext;
  // priority kernels, with report: bit 31 of the posted count is set when every queued
  // tile's key (min key of the input list) exceeds the largest T over these cells -- they
  // are final (the early exit of dymu_solve_until_device); n = 0: off
  ProbeCells probe;
  // ---- kernel 5, sharded rounds (dom_round) ----
  // received neighbour rows (nx doubles, device) min-merged into the ghost rows by this
  // pass; the tiles under improved columns are queued for the NEXT pass
  const double* merge_lo;
  const double* merge_hi;
  uint32_t* tot_save;       // block 0 stores the pass's count here ...
  const uint32_t* tot_prev;  // ... and a later pass stores *tot_prev + its count
  int32_t* tot_out;          //     into *tot_out (the round's termination count)
  // peer rounds (dymu_dom_round_peer): the merge reads merge_tag[s] (the sequence tag
  // the neighbour writes after its push, system scope) before its share of the row,
  // and the pass pushes the owned first (0) / last (1) row's decreased values into the
  // neighbour's receive row push_dst[s] (peer-mapped) and, from the last workgroup,
  // the new tag into push_tag[s]; push_last[s] holds the values last pushed.  With
  // peer set, the status pass (tot_out) also records S / R in *peer.
  const unsigned long long* merge_tag[2];
  double* push_dst[2];
  unsigned long long* push_tag[2];
  double* push_last[2];
  PeerCtl* peer;
  // ---- kernel 5: edge columns (required) ----
  // ec[t * 32 + 0..15] = column 0 (W edge) of tile t's T, ec[t * 32 + 16..31] = column
  // 15 (E edge): an interior tile reads its W / E halo as ONE 128-byte line of its
  // neighbour's edge instead of one line per row; every visit writes its decreased
  // edge cells here too ("Edge columns")
  double* ec;
  // ---- kernel 5, per-pass statistics (dymu_set_pass_stats; off = null) ----
  // this pass's record: kShards rows of kPsWords words (PassStat), one row per
  // workgroup shard, summed (max / min for the radii) by the host
  uint32_t* pstat;
  int goal_tx, goal_ty;  // the goal's tile (radius = Manhattan tile distance from it)
  // ---- kernel 5: list entries carry their first-insertion key bin (kPackShift) ----
  // 1: this pass's enqueues write tile | (bin + 1) << kPackShift; an entry with a bin
  // above the pass's threshold is then deferred on its CURRENT key before any tile
  // load, one at or below it is relaxed without waiting on the key (the current key
  // is never above the first-insertion one, so the decision is the key gate's)
  int pack_bins;
};
// list entries: the tile index in the low kPackShift bits; bits above: 0 = no bin
// (seeding kernels, merges), else the key bin + 1 the entry was first inserted with
constexpr int kPackShift = 25;
constexpr uint32_t kTileMask = (1u << kPackShift) - 1u;

// Division of a tile index by the tiles per row without a divider: with l =
// ceil(log2 d), s = kPackShift + l and m = floor(2^s / d) + 1,
//   floor(n * m / 2^s) = floor(n / d)   for every 0 <= n < 2^25, 1 <= d <= 2^25.
// Proof: m = 2^s / d + e with 0 < e <= 1, so n * m / 2^s = n / d + n * e / 2^s, and the
// excess n * e / 2^s < 2^25 / 2^s = 2^-l <= 1 / d; n / d lies at least 1 / d below the next
// integer, so the floor does not change.  m <= 2^25 * (2^l / d) + 1 < 2^26 + 1 fits 32
// bits and n * m < 2^52 fits 64.  tools/tile_div_check.cpp checks it against / and %.
struct TileDiv {
  uint32_t mul, shift;
};
inline TileDiv tile_div(uint32_t d) {
  uint32_t l = 0;
  while ((1ull << l) < d) ++l;
  const uint32_t s = (uint32_t)kPackShift + l;
  return TileDiv{(uint32_t)((1ull << s) / d + 1ull), s};
}

// per-pass statistics words (kernel 5)
enum PassStat : int {
  kPsActive = 0,    // listed entries (block 0)
  kPsVisited = 1,   // tiles relaxed
  kPsColour = 2,    // entries deferred by the checkerboard colour (no tile load)
  kPsKey = 3,       // entries deferred by the key threshold (tile loaded, then skipped)
  kPsCapped = 4,    // visits stopped by the sweep cap (re-queued)
  kPsDeadline = 5,  // visits stopped by the pass deadline (re-queued)
  kPsRadiusMax = 6, // largest tile radius relaxed (atomicMax; 0 = none or the goal tile)
  kPsSweeps = 7,    // in-tile sweeps
  kPsBstar = 8,     // threshold bin (block 0)
  kPsRadiusMin = 9, // ~smallest tile radius relaxed (atomicMin of ~r... stored as 0xFFFFFFFF - r)
  kPsEnqueued = 10, // entries appended to the next list (activations + deferrals)
  kPsWords = 12
};
constexpr uint32_t kPassStatCap = 16384;  // passes kept (a ring; pass p at p % cap)

constexpr int kBins = 64;  // v4/v5 key histogram bins
constexpr int kTracePts = 10;
// resident workgroups per CU of pass kernel variant 3/4/5 (occupancy API)
int pass_blocks_per_cu(int variant);

hipError_t launch_fill_inf(double* T, uint64_t ld, uint32_t nx, int64_t row_lo, int64_t row_hi,
                           hipStream_t st);
// The tiles a seeded cell queues: its own and, where the cell lies on a tile edge, the
// tile across that edge.  A cell across the edge is updated from the seed's value, which
// no visit of the seed's tile changes, and a visit queues its neighbours (and keys them)
// for the edge values it CHANGED only: without these entries the tile across would be
// keyed above the value its cell ends at, or, with every in-tile neighbour of the seed
// blocked, never be queued at all.  Priority kernels (4, 5) only: the plain FIM (kernel 3)
// queues the seed's own tile, as before.
struct SeedTiles {
  uint32_t t[3];
  uint32_t n;
};
hipError_t launch_seed(double* T, uint64_t ld, int64_t gi, int64_t gj, uint32_t* list,
                       uint32_t* count, uint32_t* tile_epoch, uint32_t epoch,
                       const SeedTiles& tiles, int set_goal, hipStream_t st);
hipError_t launch_pass_prio(const PassArgs& a, int blocks, hipStream_t st,
                           hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr);
hipError_t launch_pass_prio16(const PassArgs& a, int blocks, hipStream_t st,
                             hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr);  // kernel 5
hipError_t launch_pass_rb(const PassArgs& a, int blocks, hipStream_t st,
                      hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr);     // v3: 2 x 8x8 tiles / wave, red-black
hipError_t launch_merge_ghosts(double* T, int64_t ld, int64_t nx, int64_t nrows,
                               const double* new_lo, const double* new_hi, int ntx, int nty,
                               int tile_w, uint32_t* list, uint32_t* counts, uint32_t cap,
                               uint32_t* tile_epoch, uint32_t epoch, unsigned long long* keys,
                               uint32_t* hist, unsigned long long* minkey, const double* base,
                               const double* delta, hipStream_t st);
hipError_t launch_exchange(double* T, int64_t ld, int64_t nx, int64_t nrows, const double* new_lo,
                           const double* new_hi, int ntx, int nty, int tile_w, uint32_t* list,
                           uint32_t* counts, uint32_t cap, uint32_t* tile_epoch, uint32_t epoch,
                           unsigned long long* keys, uint32_t* hist, unsigned long long* minkey,
                           const double* base, const double* delta, uint32_t* ticket,
                           int32_t* total, hipStream_t st);
hipError_t launch_eikonal_batch(const double* tx, const double* ty, const double* c, double* out,
                                uint64_t n, int fast, hipStream_t st);
hipError_t launch_sum_counts(const uint32_t* counts, int32_t* out, hipStream_t st);
// one wave runs the priority passes' list scan (pass_scan) on kShards counts and a
// kShards x kBins histogram: out[0 .. kShards] = the shard prefixes (s_pref),
// out[kShards + 1] = the threshold bin b*
hipError_t launch_pass_scan_probe(const uint32_t* counts, const uint32_t* hist, uint32_t target,
                                  float target_frac, float cap_frac, uint32_t* out,
                                  hipStream_t st);
// edge columns of tiles [t0, t1) (16x16 tiles, ntx per row) from T (see PassArgs::ec)
hipError_t launch_ec_rebuild(const double* T, uint64_t ld, uint32_t nx, uint32_t ny, double* ec,
                             uint32_t ntx, uint32_t t0, uint32_t t1, hipStream_t st);
// deterministic mode: rebuild the key histogram of a list from its FINAL keys (the
// enqueue path bins a tile by the key of its first insertion, which depends on the
// order of the insertions) into shard 0's row of `out`; `zero` (the other of two
// alternating buffers) is cleared for the next rebuild
hipError_t launch_rehist(const uint32_t* list, const uint32_t* counts, uint32_t cap,
                         const unsigned long long* keys, const double* base, const double* delta,
                         uint32_t* out, uint32_t* zero, hipStream_t st);
// computeCostMap state (SoA planner node fields, row-major pitch ld)
struct CostState {
  double* cost;
  double* raw_cost;
  double* slope;
  uint32_t* terrain;
  uint8_t* is_obstacle;
  double* hazard;
  double* traff;
  int32_t* loc_mode;
};
struct CostArgs {
  uint32_t nx, ny;
  int64_t ld;
  double res, cmax, slope_lo, slope_hi;
  int n_slopes, n_locs, lut_len;
  const double* lut;  // device copy
  const double* elevation;
  const double* terrain_map;
  CostState st;
  double* F;  // speed output (may be null for launch_cost_map)
};
hipError_t launch_cost_map(const CostArgs& a, hipStream_t st);
hipError_t launch_pack_speed(const CostArgs& a, hipStream_t st);

// windowed re-propagation (update_kernels.hip)
struct UpdateArgs {
  double* T;
  const double* F;
  int64_t ld;
  uint32_t nx, ny, gi, gj;
  const unsigned long long* theta_bits;
  uint32_t* list;    // list 0 (kShards x shard_cap)
  uint32_t* counts;  // its kShards counters
  uint32_t shard_cap;
  uint32_t* tile_epoch;
  uint32_t epoch;
  uint32_t tw, th, ntx;
  unsigned long long* keys;  // priority kernels: keys / histogram of list 0, else null
  uint32_t* hist;
};
hipError_t launch_window_min(const double* T, int64_t ld, uint32_t i0, uint32_t j0, uint32_t i1,
                             uint32_t j1, unsigned long long* out, hipStream_t st);
hipError_t launch_reset_seed(const UpdateArgs& a, hipStream_t st);
// *out += the number of cells of T (nx x ny, pitch ld) whose bits equal value's;
// with idx (device, cap entries) also the first cap of their indices j*nx + i
hipError_t launch_count_equal(const double* T, int64_t ld, uint32_t nx, uint32_t ny, double value,
                              unsigned long long* out, uint64_t* idx, uint64_t cap,
                              hipStream_t st);
// decrease-only window [i0,i1) x [j0,j1): seed the tiles that intersect it, no reset
hipError_t launch_seed_window(const UpdateArgs& a, uint32_t i0, uint32_t j0, uint32_t i1,
                              uint32_t j1, hipStream_t st);
hipError_t launch_theta_state(const unsigned long long* theta_bits, unsigned long long* minkey0,
                              double* base0, hipStream_t st);

// windowed re-propagation of seeded maps and of stacks of planes (update_kernels.hip,
// DESIGN.md s5.8): planes of nx x ny cells at a plane pitch of P rows (one plain map:
// one plane, P = ny), theta per plane
struct BatchWindow {  // plane-local [i0, i1) x [j0, j1), clipped to the plane
  uint32_t plane, i0, j0, i1, j1, pad;
};
struct PlaneUpdateArgs {
  double* T;
  const double* F;
  int64_t ld;
  uint32_t nx, ny, P, rows;         // rows = planes * P
  const unsigned long long* theta;  // per plane (double bits; +inf: no window)
  const BatchWindow* win;           // device-readable
  uint32_t n_win;
  uint32_t* list;    // list 0 (kShards x shard_cap)
  uint32_t* counts;  // its kShards counters
  uint32_t shard_cap;
  uint32_t* tile_epoch;
  uint32_t epoch;
  uint32_t tw, th, ntx;
  unsigned long long* keys;     // priority kernels: keys of list 0, else null
  unsigned long long* n_reset;  // += finite cells at or above their plane's theta
};
hipError_t launch_fill_u64(unsigned long long* p, uint32_t n, unsigned long long v,
                           hipStream_t st);
// theta[plane] = min(theta[plane], min T over each of the plane's windows and its 1-cell
// ring, clipped to the plane); max_cells: the largest window's cells (grid sizing)
hipError_t launch_windows_min(const double* T, int64_t ld, uint32_t nx, uint32_t ny, uint32_t P,
                              const BatchWindow* win, uint32_t n_win, uint64_t max_cells,
                              unsigned long long* theta, hipStream_t st);
// every finite cell at or above its plane's theta <- +inf; the tiles where such a cell
// of finite speed touches a kept finite cell into list 0 with key theta[plane]
hipError_t launch_reset_planes(const PlaneUpdateArgs& a, hipStream_t st);
// decrease-only: the tiles that intersect each window into list 0, key theta[plane]
hipError_t launch_seed_windows(const PlaneUpdateArgs& a, uint64_t max_cells, hipStream_t st);
// list 0's minkey / histogram origin <- min over the planes' theta (0 if none is finite)
hipError_t launch_theta_min_state(const unsigned long long* theta, uint32_t planes,
                                  unsigned long long* minkey0, double* base0, hipStream_t st);

// raise front of a windowed update with speed increases (update_kernels.hip): one
// pass over the listed 16x16 tiles; every cell whose converged value is no longer
// supported by the update of its current neighbours under the new speed (u >
// T (1 + tol)) becomes +inf, inside the tile until nothing changes; the tiles
// across an edge with an invalidated cell are listed for the next pass
struct RaiseArgs {
  double* T;
  const double* F;
  int64_t ld;
  uint32_t nx, ny, gi, gj;
  uint32_t ntx, nty;  // 16x16 tiles
  const uint32_t* list_in;
  const uint32_t* count_in;
  uint32_t* list_out;
  uint32_t* count_out;
  uint32_t* count_clear;
  uint32_t shard_cap;
  uint32_t* tile_epoch;
  uint32_t epoch;
  double tol;
  unsigned long long* stats;  // [0] tile visits, [1] cells invalidated
  double c;                   // launch_raise_seeded: the constant speed
};
hipError_t launch_raise(const RaiseArgs& a, int blocks, hipStream_t st);
// The raise of a seeded constant-speed field (the clearance field after obstacle cells were
// freed): the speed is a.c everywhere, a.F is the mask whose obstacle cells (+inf or NaN) are
// the seeds and exempt (a.gi, a.gj are not read), and a cell that is free in the mask and
// holds +0.0 becomes +inf whatever its neighbours hold.
hipError_t launch_raise_seeded(const RaiseArgs& a, int blocks, hipStream_t st);
// after the raise: list 0 <- every tile holding a finite-speed +inf cell (not the goal)
// next to a finite cell, key = the smallest such neighbour value of the tile (a
// scheduling hint), histogram bin 0; *theta_bits lowered to the smallest key
hipError_t launch_cone_seed(const UpdateArgs& a, unsigned long long* theta_bits, hipStream_t st);

// early exit of computeTotalCostMap (update_kernels.hip)
// out[0] = bits of max T over the probe cells, out[1] = *minkey (or +inf bits if null)
hipError_t launch_probe(const double* T, int64_t ld, const ProbeCells& cells,
                        const unsigned long long* minkey, unsigned long long* out,
                        hipStream_t st);
// reference node states after the early exit: T > t_closed -> +inf unless the cell is a
// finite-speed 4-neighbour of a cell with T <= t_closed (the band: index appended to band)
hipError_t launch_early_mask(const double* F, double* T, int64_t ld, uint32_t nx, uint32_t ny,
                             double t_closed, uint64_t* band, unsigned long long* n_band,
                             uint64_t cap, hipStream_t st);
// the early exit's region: bbox of the cells with T <= thr into out[0..3] (atomic
// min i, min j, max i, max j: initialise to ~0, ~0, 0, 0) and the count of cells with
// lo <= T <= hi added to out[4]
hipError_t launch_region_box(const double* T, int64_t ld, uint32_t nx, uint32_t ny, double thr,
                             double lo, double hi, unsigned long long* out, hipStream_t st);
// least squared distance from (gi, gj) to a cell of speed != f0 into *out (atomic min:
// initialise to ~0)
hipError_t launch_const_radius(const double* F, int64_t ld, uint32_t nx, uint32_t ny, uint32_t gi,
                               uint32_t gj, double f0, unsigned long long* out, hipStream_t st);
// *p = v, in stream order (no host-to-device copy for a per-call scalar)
hipError_t launch_store_u64(unsigned long long* p, unsigned long long v, hipStream_t st);
// T[(idx / nx) * ld + idx % nx] = vals[k]
hipError_t launch_scatter(double* T, int64_t ld, uint32_t nx, const uint64_t* idx,
                          const double* vals, uint64_t n, hipStream_t st);

// The argument block of the continuous descent step (descent_step.h), which the three
// path kernels' blocks begin with: the reference's gradient descent on T from start_xy[p]
// (grid-local metres) towards the sink.  dymu_fim.cpp's descent_args fills it.
struct DescentArgs {
  const double* T;  // total cost, pitch ld
  int64_t ld;
  uint32_t nx, ny;
  double res;              // global_res
  double res_tau;          // res * tau: the step length
  double two_res;          // 2 * res: within this of the sink the descent ends
  double stall;            // 0.01 * tau * res: a shorter step is "ERROR in trajectory"
  double sink_x, sink_y;   // res * goal_i, res * goal_j
  const double* start_xy;  // n_paths x 2
  uint32_t n_paths, max_wp;
  // ---- goal sets: label null is the single sink (sink_x, sink_y) ----
  const uint32_t* label;  // nearest-goal label per cell, pitch nx (0xFFFFFFFF: none)
  const double* goal_xy;  // n_goals x 2: the sinks (res * i, res * j)
  uint32_t n_goals;
};

// batched path extraction (path_kernels.hip): one lane per path runs the descent
struct PathArgs : DescentArgs {
  uint32_t stride;
  double* out;      // [path][slot][4]: x, y and the (dcx, dcy) that produced the waypoint
  int32_t* count;   // slots written per path
  int32_t* status;  // 1 sink appended, 0 stalled, -1 first step NaN / off the grid, -3 max_wp
  int32_t* sink;    // goal sets: per path the goal whose sink was appended, or -1
};
hipError_t launch_extract_paths(const PathArgs& a, hipStream_t st);
// the same descent with a per-path sink: the goal labelled on the cell the path is in
hipError_t launch_extract_paths_goals(const PathArgs& a, hipStream_t st);

// per-path summaries (path_stats_kernels.hip): the same descent, no
// waypoint stored, one record per path.  PathStatRec is dymu_path_stat's layout.
constexpr int kPathFields = 4;
struct PathStatRec {
  int32_t status, sink;
  uint32_t count, reserved;
  double length, last_hop;
  double integral[kPathFields], vmin[kPathFields], vmax[kPathFields];
  uint32_t skipped[kPathFields];
};
struct PathStatArgs : DescentArgs {
  const double* field[kPathFields];  // the sampled fields, pitch field_ld
  int64_t field_ld[kPathFields];
  uint32_t* next;    // the work queue: the next path index to hand out (zero at launch)
  PathStatRec* out;  // n_paths records
};
// n_fields <= kPathFields fields; lanes: a multiple of 64, the size of the grid
hipError_t launch_path_stats(const PathStatArgs& a, uint32_t n_fields, uint32_t lanes,
                             hipStream_t st);

// the arriving descent (arrive_kernels.hip): the continuous step where
// it is valid, a node-to-node step on T where it is not.  ArriveRec is dymu_arrive_stat's
// layout.
struct ArriveRec {
  int32_t status, sink;
  uint32_t count, hops;
  double length, start_cost;
};
struct ArriveArgs : DescentArgs {  // the label is looked up at the node; two_res is unused
  uint32_t goal_i, goal_j;         // the single sink's node
  uint32_t stride;
  double* out;       // null: no waypoint is stored; else PathArgs' slots
  int32_t* count;    // slots kept per path (may be null with out)
  ArriveRec* stats;  // n_paths records
  // ---- the simplified form only (path_simplify.h) ----
  double eps, eps2;    // the bound and eps * eps
  uint32_t max_kept;   // slots per path in out and index; count = waypoints kept, stored or not
  uint32_t* index;     // null, or per kept waypoint its number in the walk
};
hipError_t launch_arrive_paths(const ArriveArgs& a, hipStream_t st);
// the same walk at stride 1 with only the waypoints the rule keeps stored: max_wp bounds
// the walk, max_kept the slots
hipError_t launch_arrive_simplified(const ArriveArgs& a, hipStream_t st);

// goal sets (goal_kernels.hip)
struct GoalSeed {  // dymu_seed's layout
  uint32_t i, j;
  double t0;
};
struct SeedArgs {
  const GoalSeed* seeds;  // device-readable
  uint32_t n;
  double* T;
  int64_t ld;
  uint32_t nx, ny;
  uint32_t tw, th, ntx;
  uint32_t* list;    // list 0 (kShards x shard_cap)
  uint32_t* counts;  // its kShards counters
  uint32_t shard_cap;
  uint32_t* tile_epoch;
  uint32_t epoch;
  unsigned long long* keys;  // priority kernels: keys / histogram of list 0, else null
  uint32_t* hist;
  const double* base;   // histogram origin of list 0 (= min t0) and bin width
  const double* delta;
  double* ec;  // kernel 5 edge columns, else null
};
// T[seed] = min(T, t0) for every seed; each seeded tile (a seed's own and the tile across
// each tile edge its cell lies on, see SeedTiles) once into list 0, its key the smallest
// value of the seeds that queued it, binned against *base
hipError_t launch_seed_goals(const SeedArgs& a, hipStream_t st);
// L (nx * ny entries, pitch nx): per cell a resolved label (top bit set) or its parent's
// cell index; then in-place pointer-jumping rounds (cnt[round] = entries still
// unresolved after it; a round after a 0 does nothing) and the tag bit's removal
hipError_t launch_label_init(const double* T, int64_t ld, uint32_t nx, uint32_t ny,
                             const GoalSeed* seeds, uint32_t n_seeds, uint32_t* L,
                             hipStream_t st);
hipError_t launch_label_jump(uint32_t* L, uint32_t n, uint32_t* cnt, uint32_t round,
                             hipStream_t st);
hipError_t launch_label_strip(uint32_t* L, uint32_t n, hipStream_t st);

// every cell's node route to the goal (route_kernels.hip): the hop of the
// arriving descent at every node, its aggregates by synchronous pointer doubling.
// RouteState is one of the two buffers of the doubling, SoA over the nx * ny cells (pitch
// nx); an array that is not carried is null.
constexpr uint32_t kRouteRounds = 32;  // 31 suffice for nx * ny < 2^31
struct RouteState {
  uint32_t* next;  // a cell index, or a terminal entry (top bit set: seed index / NONE)
  uint32_t *axis, *diag;
  double* integ[kPathFields];
  double* vmin[kPathFields];
  double* vmax[kPathFields];
};
struct RouteInitArgs {
  const double* T;  // total cost, pitch ld
  int64_t ld;
  uint32_t nx, ny;
  double res;
  const double* field[kPathFields];  // null: not sampled
  int64_t field_ld[kPathFields];
  RouteState s0, s1;
};
struct RouteFinalArgs {
  uint32_t nx, ny;
  double res;
  const double* field[kPathFields];
  int64_t field_ld[kPathFields];
  RouteState s;  // the final state
  const GoalSeed* seeds;
  uint32_t n_seeds;
  // the outputs, pitch o_ld elements; null: not written
  uint32_t *o_sink, *o_axis, *o_diag;
  double* o_length;
  double* o_integ[kPathFields];
  double* o_vmin[kPathFields];
  double* o_vmax[kPathFields];
  int64_t o_ld;
};
// state 0 into s0, what a round needs of it into s1, the roots marked in both
hipError_t launch_route_init(const RouteInitArgs& a, const GoalSeed* seeds, uint32_t n_seeds,
                             hipStream_t st);
// dst = one doubling of src; cnt[round] = entries still open after it; a round after a 0
// does nothing
hipError_t launch_route_round(const RouteState& src, const RouteState& dst, uint32_t n,
                              uint32_t* cnt, uint32_t round, hipStream_t st);
hipError_t launch_route_final(const RouteFinalArgs& a, hipStream_t st);

// how much of the map drains through every cell (usage_kernels.hip): the
// reverse of the doubling above on the same entries (launch_route_init with the `next`
// arrays only).  All arrays are workspace, pitch nx; a null sum or far array is not carried.
struct UsageRoundArgs {
  uint32_t nx, ny;
  const uint32_t* nsrc;  // the entries of state r
  uint32_t* ndst;        // ... of state r + 1
  const unsigned long long* asrc;  // A_r
  unsigned long long* adst;        // A_{r+1}
  unsigned long long* far;         // M, bit patterns of doubles >= +0.0, in place
};
struct UsageFinalArgs {
  uint32_t nx, ny;
  const uint32_t* next;  // the final entries
  const unsigned long long* sum;
  const unsigned long long* far;
  uint32_t n_seeds;
  // the outputs, pitch o_ld elements; null: not written
  unsigned long long* o_usage;
  double* o_far;
  uint32_t* o_sink;
  int64_t o_ld;
};
// A_0 = w (W null: 1), M_0 = T for the cells with T < +inf, 0 elsewhere
hipError_t launch_usage_init(const double* T, int64_t ld, uint32_t nx, uint32_t ny,
                             const uint32_t* W, int64_t w_ld, unsigned long long* sum,
                             unsigned long long* far, hipStream_t st);
// one round: adst <- asrc, then every open entry sends.  cnt[round] = entries still open
// after it, cnt[kRouteRounds + round] = entries that sent in it; a round after a 0 does
// nothing.  gather0: round 0 by reads of the eight neighbours instead of atomics.
hipError_t launch_usage_round(const UsageRoundArgs& a, uint32_t* cnt, uint32_t round,
                              bool gather0, hipStream_t st);
// the masked outputs, and with catchment (n_seeds words, device-visible) the roots' sums
hipError_t launch_usage_final(const UsageFinalArgs& a, const GoalSeed* seeds,
                              unsigned long long* catchment, hipStream_t st);

// batched solves (batch_kernels.hip): `planes` maps of nx x ny stacked at
// a plane pitch of P rows (dymu_batch_plane_rows), rows ny .. P-1 of each being +inf walls
// dst (pitch ld, planes * P rows) <- plane b from src + b * src_plane_stride (pitch src_ld;
// stride 0: one map for all planes), every wall row +inf
hipError_t launch_stack_speed(const double* src, uint64_t src_ld, uint64_t src_plane_stride,
                              uint32_t nx, uint32_t ny, uint32_t planes, uint32_t P, double* dst,
                              uint64_t ld, hipStream_t st);
// out[b * M + m] = DyMuPathPlanner::getTotalCost of point xy[m] (grid-local metres) on
// plane b of the solved stack T, bit-identical to the host's on the same values
hipError_t launch_gather_costs(const double* T, uint64_t ld, uint32_t nx, uint32_t ny,
                               uint32_t planes, uint32_t P, double res, const double* xy,
                               uint32_t M, double* out, hipStream_t st);

// early exit on target cells (batch_kernels.hip)
struct ProbeTarget {  // dymu_batch_cell's layout: cell (i, j) of plane `plane`
  uint32_t plane, i, j, pad;
};
// The stop test's inputs over `n` targets (device-readable, sorted by plane) of a stack of
// `planes` maps at a plane pitch of P rows (one plain map: one plane, P = ny).  A target
// counts when its speed is finite.  out (2 + planes words, zeroed before the launch):
// out[0] = bits of max T over the counting targets, out[1] = *minkey, out[2 + b] = bits of
// max T over plane b's counting targets (0: none).
hipError_t launch_probe_targets(const double* F, const double* T, uint64_t ld, uint32_t nx,
                                uint32_t ny, uint32_t planes, uint32_t P, const ProbeTarget* tg,
                                uint32_t n, const unsigned long long* minkey,
                                unsigned long long* out, hipStream_t st);

// obstacle clearance field and risk-inflated speed (clearance_kernels.hip)
struct MaskSeedArgs {
  double* T;  // the field: +inf after the cold dom_begin
  int64_t ld;
  uint32_t nx, ny;
  uint32_t tw, th, ntx;
  uint32_t* list;    // list 0 (kShards x shard_cap)
  uint32_t* counts;  // its kShards counters
  uint32_t shard_cap;
  uint32_t* tile_epoch;
  uint32_t epoch;
  unsigned long long* keys;  // priority kernels: keys / histogram of list 0, else null
  uint32_t* hist;
  double* ec;                   // kernel 5 edge columns, else null
  unsigned long long* n_obst;  // += the obstacle cells found (one atomic per workgroup)
};
// W (nx x ny, pitch ld) <- v
hipError_t launch_fill_const(double* W, uint64_t ld, uint32_t nx, uint32_t ny, double v,
                             hipStream_t st);
// T = 0 at every cell whose F is +inf or NaN; each tile that holds one (and, with keys, the
// tile across each tile edge such a cell lies on, see SeedTiles) once into list 0, key 0,
// bin 0.  `blocks` workgroups, each on one tile at a time.
hipError_t launch_seed_mask(const double* F, const MaskSeedArgs& a, uint32_t ntiles, uint32_t blocks,
                            hipStream_t st);
// The window of dymu_clearance_update_device: cells [i0, i1) x [j0, j1), clipped to the
// grid, and the ntwx x ntwy tiles from (tx0, ty0) that meet it.
struct MaskWindow {
  uint32_t i0, j0, i1, j1;
  uint32_t tx0, ty0, ntwx, ntwy;
  uint32_t seed;                // 0: count only; 1: seed the new obstacle cells
  unsigned long long* n_freed;  // count only: += the cells finite in F that hold +0.0
};
// seed = 0: *a.n_obst += the window's cells that are obstacles in F and do not hold +0.0 in
// a.T, *w.n_freed += its cells finite in F that hold +0.0; nothing else is written.
// seed = 1: k_seed_mask's seeding for exactly the former cells (a.n_obst is not used).
hipError_t launch_seed_mask_window(const double* F, const MaskSeedArgs& a, const MaskWindow& w,
                                   uint32_t blocks, hipStream_t st);
// box[0..3] (from {~0, ~0, 0, 0}) = min tx, min ty, max tx + 1, max ty + 1 over the tiles with
// tile_epoch >= epoch_lo
hipError_t launch_claimed_box(const uint32_t* tile_epoch, uint32_t ntiles, uint32_t ntx,
                              uint32_t epoch_lo, uint32_t* box, hipStream_t st);
// The boundary of the cone a seeded raise left (dymu_clearance_edit_device), from the 16x16
// raise tiles of the box [bx0, bx0 + nbx) x [by0, by0 + nby) whose stamp is at least stamp_lo
// (the tiles the raise claimed) and from no other tile: the old field's own stop at the level
// is a +inf cell beside a finite one too, map-wide.
struct ConeArgs {
  const double* S;
  const double* F;  // the mask
  int64_t ld;
  uint32_t nx, ny;
  uint32_t ntx16;                  // raise tiles per row
  uint32_t bx0, by0, nbx, nby;     // the raise's box, in raise tiles
  uint32_t stamp_lo;               // the raise's first epoch; 0 (every tile of the box) when
                                   // the epochs restarted behind the raise and took its stamps
  uint32_t tw, th, ntx;            // the pass kernel's tiles (8 or 16 cells), bind_list0
  uint32_t* list;                  // list 0 (kShards x shard_cap)
  uint32_t* counts;
  uint32_t shard_cap;
  uint32_t* tile_epoch;
  uint32_t epoch;
  unsigned long long* keys;        // keys of list 0: +inf bits wherever no seeding kernel wrote
  unsigned long long* theta_bits;  // lowered to the smallest key
};
// keys[t] = min(keys[t], v) for every pass tile t that holds a cell with S = +inf, finite F
// and a finite in-grid 4-neighbour, v the smallest such neighbour value; reads the stamps,
// writes none
hipError_t launch_cone_keys(const ConeArgs& a, uint32_t blocks, hipStream_t st);
// list 0 <- every pass tile under the raise's box whose key is finite, claimed once
hipError_t launch_cone_queue(const ConeArgs& a, hipStream_t st);
// out = F * (risk_ratio * max(1 - S, 0) + 1) per cell, operation by operation; out may be F
hipError_t launch_inflate_speed(const double* F, const double* S, double* out, uint64_t ld,
                                uint32_t nx, uint32_t ny, double risk_ratio, hipStream_t st);

// ---- plane reduction and level mask (reduce_kernels.hip) ----
// How 256-thread workgroups walk an nx x ny map at `base` with pitch ld two cells at a time:
// a row takes 2^lanes_log2 lanes of a tile (256: `chunks` tiles per row), ntiles in all.
struct TileWalk {
  uint64_t ntiles;
  uint32_t chunks, lanes_log2;
};
TileWalk tile_walk(const void* base, uint64_t ld, uint32_t nx, uint32_t ny);
// one listed plane: its offset in the stack in elements (plane * P * ld), weight, offset
struct ReduceTerm {
  uint64_t off;
  double w, o;
  uint32_t plane, reserved;
};
// a workgroup's share of the summary, and the summary itself: the smallest value below +inf,
// its cell j * nx + i (~0: none; the lowest among equals), the cells below +inf, the arg there
struct ReducePartial {
  double v;
  uint64_t cell, n;
  uint32_t arg, reserved;
};
struct ReduceArgs {
  const double* T;          // the stack, plane 0
  uint64_t ld;
  uint32_t nx, ny;
  const ReduceTerm* terms;  // device, n entries
  uint32_t n, flags;        // flags: 1 weights, 2 offsets
  double* out;
  uint64_t out_ld;
  uint32_t* arg;            // may be null
  uint64_t arg_ld;
  ReducePartial* part;      // one record per workgroup, or null: no summary
  TileWalk walk;
};
// op: 0 sum, 1 max, 2 min.  With a.part the partials are folded into *d_sum by a second launch.
hipError_t launch_batch_reduce(const ReduceArgs& a, int op, uint32_t blocks, ReducePartial* d_sum,
                               hipStream_t st);
// mask = map <= bound; box (null: none) = {min i, min j, max i, max j} from {~0, ~0, 0, 0} and
// *cnt += the marked cells
hipError_t launch_level_mask(const double* map, uint64_t ld, uint32_t nx, uint32_t ny, double bound,
                             uint8_t* mask, uint64_t mask_ld, const TileWalk& walk, uint32_t blocks,
                             uint32_t* box, unsigned long long* cnt, hipStream_t st);

hipError_t launch_prio_init(const double* F, int64_t ld, int64_t nx, int64_t ny,
                           unsigned long long* keys, uint64_t nkeys, uint32_t* hist, uint64_t nhist,
                           unsigned long long* minkey, double* base, double* delta, double kappa,
                           hipStream_t st);
hipError_t launch_prio_seed(unsigned long long* key0, uint32_t* hist0, unsigned long long* minkey0,
                           const SeedTiles& tiles, double keyv, hipStream_t st);
hipError_t launch_synth(double* F, uint64_t ld, uint32_t nx, uint32_t ny, uint64_t row0,
                        uint64_t seed, double frac, uint64_t oseed, int64_t gi, int64_t gj,
                        hipStream_t st);

}  // namespace dymu
