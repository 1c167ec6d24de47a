/*
 * dymu_fim.h -- C-ABI of the MI355X (gfx950) total-cost propagation engine.
 *
 * This is the drop-in boundary for the DyMu global total-cost propagation
 * (ESA-PRL/planning-path_planning).  It replaces, for the host C++ planner
 * (include/DyMu.hpp), the hot loop of:
 *   - DyMuPathPlanner::computeEntireTotalCostMap   src/DyMu_GlobalPathPlanning.cpp:443-468
 *   - DyMuPathPlanner::computeTotalCostMap         src/DyMu_GlobalPathPlanning.cpp:364-408
 *   - propagateGlobalNode (Eikonal update)          src/DyMu_GlobalPathPlanning.cpp:500-546
 *   - minCostGlobalNode (narrow band)               src/DyMu_GlobalPathPlanning.cpp:551-568
 *   - resetTotalCostMap / resetGlobalNarrowBand     src/DyMu_GlobalPathPlanning.cpp:473-496
 * The reference has no FFI; its boundary is the C++ class in src/DyMu.hpp:397-609.
 * This header is the C surface that class (our include/DyMu.hpp) calls, and
 * the one a cgo / JNI / ctypes binding would bind.
 *
 * Data model: row-major fp64 grids, index = j*ld + i (j = y row, i = x col,
 * reference :52-58).  F[k] is the per-node speed C of reference :527-528,
 *   F = global_res * cost * (2 + hazard_density - trafficability),
 * and +inf (or NaN) for an obstacle.  F must be >= 0 or +inf.  T[k] receives
 * the converged total cost; +inf marks unreachable cells and obstacles; the
 * goal holds 0.  Results equal the reference FMM within |dT| <= 1e-12*max(1,T)
 * with an identical +inf mask for speeds with 2*F*F finite
 * (F < 1.34e154); beyond that the reference update itself is order-dependent.
 *
 * All functions return DYMU_OK (0) or a negative dymu_status.  Contexts are
 * not thread-safe; use one context per host thread.
 */
#ifndef DYMU_FIM_H
#define DYMU_FIM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DYMU_ABI_VERSION 5

typedef enum dymu_status {
  DYMU_OK = 0,
  DYMU_ERR_ARG = -1,           /* bad argument (null pointer, size, goal off-grid) */
  DYMU_ERR_HIP = -2,           /* HIP runtime error (see dymu_last_error) */
  DYMU_ERR_NOMEM = -3,         /* device allocation failed */
  DYMU_ERR_NOT_CONVERGED = -4, /* pass cap reached (dymu_opts.max_passes) */
  DYMU_ERR_NO_DEVICE = -5,     /* no HIP device / extension unusable */
  DYMU_ERR_RCCL = -6,          /* RCCL error in the sharded solver */
  DYMU_ERR_STATE = -7          /* call out of sequence (e.g. comm not initialised) */
} dymu_status;

typedef struct dymu_ctx dymu_ctx;

typedef struct dymu_opts {
  int device;           /* HIP device ordinal; -1 = current device */
  int passes_per_check; /* passes launched between convergence read-backs; 0 = adaptive */
  int max_passes;       /* safety cap on FIM passes; 0 = derived from the grid size */
  int max_inner;        /* cap on in-tile sweeps per tile visit; 0 = default */
  int grid_blocks;      /* workgroups per pass launch; 0 = derived from the device */
  int kernel;           /* pass kernel: 0 = auto (by grid size), 3 = plain block FIM
                           (8x8 tiles), 4 = priority passes on 8x8 tiles, 5 = priority
                           passes on 16x16 tiles */
  int prio_target;      /* kernels 4/5: tiles relaxed per pass; 0 = default
                           (64 per CU for 4, 8 per CU for 5) */
  int exact_sqrt;       /* kernel 5: 1 = correctly rounded sqrt in the sweeps; 0 = default:
                           one Goldschmidt step folded into the candidate.  Both use the
                           monotone combine min(Tx,Ty) + h (one rounding at the scale of T,
                           within 1 ulp of the reference candidate plus the sqrt's error),
                           so the FIM's min over history does not accumulate a rounding
                           bias along long paths (DESIGN.md s3, s4 "Monotone combine") */
  int deterministic;    /* 1 = bit-reproducible maps: kernel 5 with checkerboard passes (a
                           pass relaxes tiles of one colour only, so no tile reads a halo
                           another wave is writing) and no sweep deadline; ~2x the passes.
                           0 = default (the last ulps depend on the schedule) */
} dymu_opts;

typedef struct dymu_stats {
  uint64_t passes;       /* FIM passes that had active tiles ("iterations to converge") */
  uint64_t launches;     /* pass kernels launched (incl. speculative empty ones) */
  uint64_t tile_visits;  /* sum over passes of active tiles */
  uint64_t inner_sweeps; /* sum over tile visits of in-tile sweeps */
  uint64_t max_active;   /* largest active-tile list */
  uint64_t rounds;       /* sharded solver: halo-exchange rounds (0 single GPU) */
  double ms;             /* device time of the solve (HIP events), ms */
  int tile_w, tile_h;    /* tile geometry used */
  int kernel;            /* pass kernel that ran (see dymu_opts.kernel) */
  int reserved;
  uint64_t deferred;     /* kernel 5: list entries deferred to a later pass (key above the
                            pass's threshold bin); entries drawn = tile_visits + deferred */
} dymu_stats;

/* Context: owns a HIP stream, events and workspace on one device. */
int dymu_create(dymu_ctx** out, const dymu_opts* opts); /* opts may be NULL */
int dymu_destroy(dymu_ctx* ctx);

/* Host-buffer solve: copies F in, solves, copies T out (the planner path).
 * F, T_out: nx*ny doubles, row-major, caller-owned host memory. */
int dymu_solve(dymu_ctx* ctx, const double* F, uint32_t nx, uint32_t ny, uint32_t goal_i,
               uint32_t goal_j, double* T_out, dymu_stats* stats);

/* Device-resident solve: dF, dT are device pointers with row pitch `ld`
 * elements (ld >= nx).  dT is overwritten (initialised to +inf, goal 0).
 * `stream` is a hipStream_t or NULL for the context's own stream.  Blocks
 * until converged. */
int dymu_solve_device(dymu_ctx* ctx, const double* dF, double* dT, uint32_t nx, uint32_t ny,
                      uint64_t ld, uint32_t goal_i, uint32_t goal_j, void* stream,
                      dymu_stats* stats);

/* ---- computeTotalCostMap's early exit (reference src/DyMu_GlobalPathPlanning.cpp:364-408) ----
 * The reference stops its FMM as soon as the start node and its 4-neighbours
 * are CLOSED (isFullyClosedNode :424-436).  dymu_solve_until_device is
 * dymu_solve_device with that stop: it returns as soon as every queued tile's
 * priority key -- a lower bound on any value the remaining passes can produce: the key
 * bound stated at dymu_dom_min_key, which holds before every pass --
 * exceeds t = max T over the start (start_i, start_j) and its in-grid
 * 4-neighbours, or when the map has converged.  On return every cell whose
 * converged value is <= *t_closed = t holds that value (the reference's CLOSED
 * set); other cells hold upper bounds.  *t_closed = +inf when the start is
 * unreachable (the whole map is then converged).  Runs a priority kernel (4 or
 * 5) whatever dymu_opts.kernel says. */
int dymu_solve_until_device(dymu_ctx* ctx, const double* dF, double* dT, uint32_t nx,
                            uint32_t ny, uint64_t ld, uint32_t goal_i, uint32_t goal_j,
                            uint32_t start_i, uint32_t start_j, void* stream, double* t_closed,
                            dymu_stats* stats);
/* The node states after that early exit: a cell is CLOSED iff T <= t_closed and
 * keeps T; a finite-speed 4-neighbour of a CLOSED cell is in the narrow band
 * (the reference propagated into it, :462-465) and keeps its current T for the
 * caller to replace with the reference's tentative value; every other cell
 * gets +inf (never reached: -1 in getTotalCostMatrix).  band_idx: host buffer
 * of `cap` entries receiving the band cells' indices j*nx + i (unordered);
 * *n_band = their number -- if it exceeds cap only cap were written, and the
 * call may be repeated with a larger buffer (it is idempotent). */
int dymu_early_exit_mask(dymu_ctx* ctx, const double* dF, double* dT, uint32_t nx, uint32_t ny,
                         uint64_t ld, double t_closed, uint64_t* band_idx, uint64_t cap,
                         uint64_t* n_band, void* stream);
/* *count = the number of cells of dT whose value is bitwise `value` (the early
 * exit's tie test: cells of exactly t_closed other than the last one the
 * reference closes make its CLOSED set depend on its insertion order).
 * Synchronises `stream`.  DYMU_ERR_ARG (here and in dymu_find_equal): a null pointer,
 * nx or ny = 0, ld < nx. */
int dymu_count_equal(dymu_ctx* ctx, const double* dT, uint32_t nx, uint32_t ny, uint64_t ld,
                     double value, uint64_t* count, void* stream);
/* dymu_count_equal that also lists the cells: *count = their number, idx (host,
 * cap entries) their indices j*nx + i (the first cap found, unordered).  The
 * planner's early exit resolves the reference's order among them. */
int dymu_find_equal(dymu_ctx* ctx, const double* dT, uint32_t nx, uint32_t ny, uint64_t ld,
                    double value, uint64_t* idx, uint64_t cap, uint64_t* count, void* stream);
/* The early exit's region, for the planner's near-tie guard and its exact host
 * replay: the bounding box of the cells with T <= thr (i0, j0, i1, j1
 * inclusive; i0 > i1 when there is none), the number of cells with lo <= T <= hi (the
 * engine's near ties with the exit value), and r_const, the Euclidean distance from
 * the goal (goal_i, goal_j) to the nearest cell whose speed differs from the goal's
 * (+inf: constant speed everywhere).  Synchronises `stream`. */
typedef struct dymu_region {
  uint32_t i0, j0, i1, j1;
  uint64_t n_range;
  double r_const;
} dymu_region;
int dymu_region_stats(dymu_ctx* ctx, const double* dF, const double* dT, uint32_t nx, uint32_t ny,
                      uint64_t ld, uint32_t goal_i, uint32_t goal_j, double thr, double lo,
                      double hi, dymu_region* out, void* stream);
/* dT[(idx[k] / nx) * ld + idx[k] % nx] = vals[k] for k < n (idx, vals: host). */
int dymu_scatter(dymu_ctx* ctx, double* dT, uint32_t nx, uint64_t ld, const uint64_t* idx,
                 const double* vals, uint64_t n, void* stream);

/* ---- batched path extraction (DyMuPathPlanner::getPaths) ----
 * The reference's gradient descent on T (computeGlobalPath and its helpers,
 * src/DyMu_GlobalPathPlanning.cpp:615-784), one GPU lane per path.  dT: total cost
 * (device, pitch ld, as a solve leaves it); res: global_res; (goal_i, goal_j): the sink;
 * tau: the step in cells (the planner's min(0.4, risk_distance)); d_start_xy: n_paths
 * (x, y) starts in grid-local metres (device).  Path p writes at most max_wp slots of 4
 * doubles at d_out + p * max_wp * 4: x, y and the descent direction (dcx, dcy) that
 * produced the waypoint (0, 0 for the start and the sink) -- heading = atan2(-dcy, -dcx)
 * and z are the caller's, so that they are the host libm's and the host's elevation.  x,
 * y and the counts are bit-identical to the host loop on the same T.  stride >= 1 keeps
 * waypoints 0, stride, 2 stride, ... and always the sink.  d_count[p] = slots written;
 * d_status[p] = 1 sink appended; 0 stalled ("ERROR in trajectory": the waypoints so far
 * are kept); -1 the first step is NaN or off the grid (nothing written); -3 max_wp
 * reached (the first max_wp kept).  A lane stops after max_wp * stride steps, and a
 * coordinate off the grid (negative, huge, NaN) ends its path before any load.
 * Asynchronous on `stream` (NULL: the context's stream). */
int dymu_extract_paths_device(dymu_ctx* ctx, const double* dT, uint32_t nx, uint32_t ny,
                              uint64_t ld, double res, uint32_t goal_i, uint32_t goal_j,
                              double tau, const double* d_start_xy, uint32_t n_paths,
                              uint32_t max_wp, uint32_t stride, double* d_out, int32_t* d_count,
                              int32_t* d_status, void* stream);
/* Device time (ms, HIP events) of the last dymu_extract_paths_device kernel; waits for
 * it.  DYMU_ERR_STATE before the first one. */
int dymu_last_paths_ms(dymu_ctx* ctx, double* ms);

/* ---- goal sets: multi-source solve, nearest-goal labels and paths ----
 * A seed is a source cell (i, j) with a start value t0 >= 0, finite (an offset: the
 * cost already paid when the route ends there).  seeds: HOST array. */
typedef struct dymu_seed {
  uint32_t i, j;
  double t0;
} dymu_seed;
#define DYMU_LABEL_NONE 0xFFFFFFFFu
/* dymu_solve_device for a seed list: dT = +inf, then T[seed] = the smallest t0 given for
 * that cell, then the converged solve -- the discrete upwind solution of all sources
 * together (not the cellwise minimum of single-source solves, which only bounds it from
 * above).  Any pass kernel, deterministic and exact_sqrt as for a single goal; one seed
 * with t0 = 0 in deterministic mode is bitwise dymu_solve_device.  DYMU_ERR_ARG:
 * n_seeds = 0, a seed off the grid, t0 negative, NaN or infinite.  A seed on a
 * +inf-speed cell keeps its value and spreads from there, like a goal on one. */
int dymu_solve_seeds_device(dymu_ctx* ctx, const double* dF, double* dT, uint32_t nx, uint32_t ny,
                            uint64_t ld, const dymu_seed* seeds, uint32_t n_seeds, void* stream,
                            dymu_stats* stats);
/* d_label[j*nx + i] (device, nx*ny words, pitch nx; plain cached device memory serves the
 * random gathers best) = the index of the seed the cell's optimal route drains to, a
 * function of dT alone:
 *   parent(c) = among the in-grid 4-neighbours in the order (i,j-1), (i-1,j), (i+1,j),
 *     (i,j+1) the first one holding the smallest T, if that is strictly below T[c];
 *   c is a root with label k if it is seed k's cell and T[c] is bitwise t0_k (duplicate
 *     cells: the smallest t0, the lowest k among equal ones; a seed whose cell ended
 *     below its t0 is dominated and no root);
 *   DYMU_LABEL_NONE for T = +inf, for a non-root without a strictly smaller neighbour,
 *     and for every cell that drains to such a cell; else label(c) = label(parent(c)).
 * Requires nx*ny < 2^31 and n_seeds < 2^31.  *rounds (may be NULL) = pointer-jumping
 * rounds run (about log2 of the longest chain; DYMU_ERR_NOT_CONVERGED beyond 64).
 * Blocks until done. */
int dymu_goal_labels_device(dymu_ctx* ctx, const double* dT, uint32_t nx, uint32_t ny, uint64_t ld,
                            const dymu_seed* seeds, uint32_t n_seeds, uint32_t* d_label,
                            void* stream, uint32_t* rounds);
/* dymu_extract_paths_device with a sink per path: whenever the path enters another
 * cell (cx, cy) its sink becomes goal d_label[cy*nx + cx] at d_goal_xy[2k], [2k+1]
 * (device, n_goals x 2: res*i, res*j); DYMU_LABEL_NONE keeps the previous sink, and a
 * path whose first cell has none gets status -1.  The end test and the appended sink
 * waypoint use the current sink; d_sink[p] = the goal appended, or -1. */
int dymu_extract_paths_goals_device(dymu_ctx* ctx, const double* dT, uint32_t nx, uint32_t ny,
                                    uint64_t ld, double res, const uint32_t* d_label,
                                    const double* d_goal_xy, uint32_t n_goals, double tau,
                                    const double* d_start_xy, uint32_t n_paths, uint32_t max_wp,
                                    uint32_t stride, double* d_out, int32_t* d_count,
                                    int32_t* d_status, void* stream, int32_t* d_sink);
/* ---- per-path summaries (DyMuPathPlanner::getPathStats) ----
 * The record of one path.  Let w_0 .. w_{n-1} be the waypoints dymu_extract_paths_device
 * (stride 1) writes for the start, in grid-local metres, seg_k = dist(w_k, w_{k+1}) =
 * sqrt(dx*dx + dy*dy), and for a sampled field f let v_k = f at w_k's nearest node
 * (i, j) = (uint)(x / res + 0.5), (uint)(y / res + 0.5), a sample that counts when the
 * node is on the grid (tested before the load) and v_k is finite.  Sums run in the order
 * k = 0, 1, ... from 0.0, so host and device agree bit for bit.
 *   status, sink  as dymu_extract_paths[_goals]_device (sink: 0 with a single sink, -1
 *                 where status != 1); -3: the record covers the first max_wp waypoints
 *   count         n (0 with status -1, and the record is then the empty one)
 *   length        seg_0 + seg_1 + ...
 *   last_hop      seg_{n-2} (0 for n < 2): at most (2 + tau) * res where the descent
 *                 arrived, longer where it was cut short and jumped to the sink
 *   integral[f]   the sum over k <= n-2 of v_k * seg_k, counting samples only
 *   vmin[f], vmax[f]  over the counting samples, from +inf / -inf
 *   skipped[f]    waypoints whose sample does not count
 * A field slot that is not used keeps 0 / +inf / -inf / 0. */
#define DYMU_PATH_FIELDS 4
typedef struct dymu_path_stat {
  int32_t status, sink;
  uint32_t count, reserved;
  double length, last_hop;
  double integral[DYMU_PATH_FIELDS], vmin[DYMU_PATH_FIELDS], vmax[DYMU_PATH_FIELDS];
  uint32_t skipped[DYMU_PATH_FIELDS];
} dymu_path_stat;
/* The descent of dymu_extract_paths_device (d_label NULL: the sink is (goal_i, goal_j))
 * or of dymu_extract_paths_goals_device (d_label, d_goal_xy, n_goals as there; goal_i,
 * goal_j ignored) for n_paths starts, storing no waypoint: d_stats[p] (device) = the
 * record of path p over the fields d_fields[f] (HOST array of n_fields <= DYMU_PATH_FIELDS
 * device maps of nx x ny doubles, pitch field_ld[f] >= nx, HOST array).  A batch plane is
 * an ordinary map pointer.  The kernel runs n_lanes lanes (rounded up to whole waves, at
 * most one per path; 0: the default, one lane per path); a lane that finishes a path
 * takes the next one from a device counter, so any n_lanes gives the same records.  One call at a time per context (the counter and the timer are the context's).
 * Asynchronous on `stream`.  DYMU_ERR_ARG: max_wp = 0, n_fields > DYMU_PATH_FIELDS, a
 * NULL field or a pitch below nx, and what dymu_extract_paths[_goals]_device reject. */
int dymu_path_stats_device(dymu_ctx* ctx, const double* dT, uint32_t nx, uint32_t ny, uint64_t ld,
                           double res, uint32_t goal_i, uint32_t goal_j, const uint32_t* d_label,
                           const double* d_goal_xy, uint32_t n_goals, double tau,
                           const double* d_start_xy, uint32_t n_paths, uint32_t max_wp,
                           const double* const* d_fields, const uint64_t* field_ld,
                           uint32_t n_fields, uint32_t n_lanes, dymu_path_stat* d_stats,
                           void* stream);
/* Device time (ms, HIP events) of the last dymu_path_stats_device kernel; waits for it.
 * DYMU_ERR_STATE before the first one. */
int dymu_last_path_stats_ms(dymu_ctx* ctx, double* ms);
/* ---- the arriving descent (DyMuPathPlanner::getArrivingPaths) ----
 * A descent that passes obstacles and ends on the sink's node: the continuous step of
 * dymu_extract_paths_device wherever it is valid, a node-to-node step on T wherever it is
 * not.  node(p) = ((uint)(x / res + 0.5), (uint)(y / res + 0.5)), on the grid iff i < nx
 * and j < ny (a negative or NaN coordinate is off it; tested before any load).  Per path:
 * the position p, its node n, and `same`, the accepted continuous steps since n changed.
 *   start   n = node(start) off the grid, T[n] = +inf, or (goal set) n without a label:
 *           status -1, the empty record, no waypoint.  Else waypoint 0 is the start.
 *   loop    at most max_wp * stride steps, each:
 *     1. n is the sink's node (goal set: label[n] = k < n_goals and goal k's node is n):
 *        the sink is appended, status 1.
 *     2. c = the continuous step from p and m = node(c).  c is taken iff it is not NaN,
 *        dist(p, c) >= 0.01 tau res, m is on the grid with T[m] finite and within one
 *        node of n in i and in j; for m = n, same < 8; for m != n, T[m] < T[n]; for a
 *        diagonal m, T is finite on both side nodes (m.i, n.j) and (n.i, m.j).
 *        Then p = c, same = (m == n) ? same + 1 : 0, n = m; the stored direction is the
 *        step's (dcx, dcy).
 *     3. else a hop: among the in-grid 8-neighbours m of n in the order (i,j-1), (i-1,j),
 *        (i+1,j), (i,j+1), (i-1,j-1), (i+1,j-1), (i-1,j+1), (i+1,j+1) with T[m] < T[n], a
 *        diagonal only with both side nodes finite, the first one of the largest score
 *        T[n] - T[m] (a diagonal: (T[n] - T[m]) * 0.7071067811865476).  None: status 0,
 *        the waypoints so far kept.  Else p = (res m.i, res m.j), n = m, same = 0, one more
 *        hop; the stored direction is (n_old.i - m.i, n_old.j - m.j).
 *     4. p is kept under dymu_extract_paths_device's stride rule; status -3 when max_wp
 *        waypoints are kept before the sink.
 * T[n] never rises and falls whenever n changes, so the walk ends; on a converged map a
 * start on a finite node arrives.  The record (count, hops and length are those of
 * stride 1, whatever the stride; -3: it covers the waypoints walked): */
typedef struct dymu_arrive_stat { /* 32 bytes */
  int32_t status, sink;  /* as dymu_extract_paths[_goals]_device; sink -1 where status != 1 */
  uint32_t count, hops;  /* waypoints at stride 1 (sink included); node-to-node steps */
  double length;         /* seg_0 + seg_1 + ... from 0.0 in order, sqrt(dx*dx + dy*dy) each */
  double start_cost;     /* T at the start's node (0 with status -1) */
} dymu_arrive_stat;
/* d_label NULL: the sink is (goal_i, goal_j); else d_label, d_goal_xy, n_goals as for
 * dymu_extract_paths_goals_device (goal_i, goal_j ignored; the label is read at the node).
 * d_out NULL: no waypoint is stored (records only, d_count may be NULL); else the slot
 * layout of dymu_extract_paths_device (x, y, dcx, dcy; max_wp slots per path) and
 * d_count[p] = slots written.  d_stats[p] (device) = the record.  A batch plane is an
 * ordinary map pointer.  Built like the host rule (no contraction): x, y, the counts, the
 * hops and the length are bit-identical to DyMuPathPlanner's host loop on the same T.
 * Argument errors are those of dymu_extract_paths[_goals]_device.  Asynchronous on
 * `stream`; one call at a time per context (the timer is the context's). */
int dymu_arrive_paths_device(dymu_ctx* ctx, const double* dT, uint32_t nx, uint32_t ny, uint64_t ld,
                             double res, uint32_t goal_i, uint32_t goal_j,
                             const uint32_t* d_label, const double* d_goal_xy, uint32_t n_goals,
                             double tau, const double* d_start_xy, uint32_t n_paths,
                             uint32_t max_wp, uint32_t stride, double* d_out, int32_t* d_count,
                             dymu_arrive_stat* d_stats, void* stream);
/* Device time (ms, HIP events) of the last dymu_arrive_paths_device kernel; waits for it.
 * DYMU_ERR_STATE before the first one. */
int dymu_last_arrive_ms(dymu_ctx* ctx, double* ms);
/* ---- the simplified arriving descent (DyMuPathPlanner::getSimplifiedPaths) ----
 * The walk of dymu_arrive_paths_device at stride 1, thinned while it runs: a dropped
 * waypoint is never stored or moved.  The rule (csrc/path_simplify.h, one header for the
 * kernel and the host) runs on the waypoints w_0 .. w_{n-1} walked, the sink excluded,
 * with eps > 0 in map units and cross(a, b) = a.x*b.y - a.y*b.x.  Its state is the anchor
 * A (a kept waypoint), the previous waypoint, a cone (l, h) with a flag `open` (no
 * constraint yet) and far2.  w_0 is kept: A = w_0, open, far2 = 0.  For each further P:
 *   1. v = P - A, d2 = v.x*v.x + v.y*v.y.
 *   2. P is admissible iff d2 >= far2 and (open, or cross(l, v) >= 0 and cross(v, h) >= 0).
 *   3. not admissible: the previous waypoint is kept and becomes A, open, far2 = 0, and P
 *      is taken again from step 1 (the first waypoint after an anchor is admissible).
 *   4. admissible: far2 = d2; if d2 > eps*eps, with c = sqrt(d2 - eps*eps),
 *        tl = (v.x*c + v.y*eps, v.y*c - v.x*eps), th = (v.x*c - v.y*eps, v.y*c + v.x*eps);
 *      open: l = tl, h = th, not open; else l = tl if cross(l, tl) > 0 and h = th if
 *      cross(th, h) > 0.
 *   5. when the walk ends, for whatever reason, the last waypoint walked is kept if it is
 *      not yet; with status 1 the sink follows it, as in dymu_arrive_paths_device.
 * Guarantee: every dropped waypoint lies within eps of the SEGMENT between the kept
 * waypoints on either side of it -- the cone bounds its distance to the ray from A, the
 * far2 rule (distances from A never fall inside a window) puts the foot on the segment.
 * It is one-sided: it bounds the dropped waypoints' distance to the polyline, not the
 * polyline's distance to the waypoints walked or to anything else; a caller who needs the
 * polyline to clear obstacles chooses eps below the clearance they rely on.
 * A kept waypoint's slot is the slot dymu_arrive_paths_device(stride 1) writes for it
 * (x, y, dcx, dcy): the output is a subsequence of that call's, element for element, and
 * d_index (optional) gives each kept waypoint's number in it (the sink's included).
 *   max_steps  the walk limit, dymu_arrive_paths_device's max_wp at stride 1: status -3
 *              beyond it, and the record covers the waypoints walked
 *   max_kept   slots per path in d_out and d_index
 *   d_out      NULL: count only; else [n_paths][max_kept][4]
 *   d_index    NULL or [n_paths][max_kept]
 *   d_count    [n_paths], required: the waypoints the rule keeps (the sink included),
 *              WHETHER STORED OR NOT.  Only the first max_kept are stored; d_count[p] >
 *              max_kept is an overflow, which changes neither the status nor the record.
 *   d_stats    [n_paths], required: byte for byte dymu_arrive_paths_device's record with
 *              max_wp = max_steps
 * Argument errors are dymu_arrive_paths_device's, and eps not finite or <= 0, max_steps
 * == 0, max_kept == 0 with d_out or d_index: DYMU_ERR_ARG.  Bit-identical to the host
 * rule like dymu_arrive_paths_device.  Asynchronous on `stream`; one call at a time per
 * context. */
int dymu_arrive_simplified_device(dymu_ctx* ctx, const double* dT, uint32_t nx, uint32_t ny,
                                  uint64_t ld, double res, uint32_t goal_i, uint32_t goal_j,
                                  const uint32_t* d_label, const double* d_goal_xy,
                                  uint32_t n_goals, double tau, const double* d_start_xy,
                                  uint32_t n_paths, double eps, uint32_t max_steps,
                                  uint32_t max_kept, double* d_out, uint32_t* d_index,
                                  int32_t* d_count, dymu_arrive_stat* d_stats, void* stream);
/* Device time (ms, HIP events) of the last dymu_arrive_simplified_device kernel; waits for
 * it.  DYMU_ERR_STATE before the first one. */
int dymu_last_arrive_simplified_ms(dymu_ctx* ctx, double* ms);
/* Device time (ms, HIP events) of the last dymu_goal_labels_device, first kernel to last.
 * DYMU_ERR_STATE before the first one. */
int dymu_last_labels_ms(dymu_ctx* ctx, double* ms);
/* ---- every cell's node route to the goal (DyMuPathPlanner::getRouteFields) ----
 * The per-path record of every cell at once, along a route that provably arrives.  The
 * definition is a function of T alone (nx x ny, pitch ld, nx*ny < 2^31) and of a seed list
 * (a single goal is one seed with t0 = 0), the same on host and device:
 *   root      dymu_goal_labels_device's rule: seed k's cell is a root iff its T is bitwise
 *             t0_k (duplicate cells: the smallest t0, the lowest k among equal ones; a
 *             dominated seed is no root).  A root is terminal even with a lower neighbour.
 *   rp(c)     the route parent of a non-root node c with T[c] < +inf: the hop target of
 *             dymu_arrive_paths_device's step 3 evaluated at n = c -- among the in-grid
 *             8-neighbours m in the order (i,j-1), (i-1,j), (i+1,j), (i,j+1), (i-1,j-1),
 *             (i+1,j-1), (i-1,j+1), (i+1,j+1) with T[m] < T[c] strictly, a diagonal only with
 *             both side nodes finite, the first one of the largest score T[c] - T[m] (a
 *             diagonal: (T[c] - T[m]) * 0.7071067811865476).  None: c is a dead end.
 *   route(c)  c, rp(c), rp(rp(c)), ... up to a root or a dead end; T falls strictly along
 *             it, so it has no cycle.
 *   no route  T[c] is +inf or NaN, or the route ends in a dead end.
 * Per cell with a route n_0 = c -> n_1 -> ... -> n_h that ends on root k:
 *   sink         k
 *   axis, diag   hops between axis and between diagonal neighbours; h = axis + diag
 *   length       res * axis + (res * 1.4142135623730951) * diag, in exactly that form
 *   integral[f]  the sum over k < h of v_f(n_k) * seg_k, seg_k = res or
 *                res * 1.4142135623730951, counting finite samples only (a sample that does
 *                not count adds 0.0): dymu_path_stat's left sum on the node route.  The
 *                order of the additions is the implementation's; a host that sums each cell
 *                from its parent and the device differ by rounding (at most
 *                h * 2^-52 * sum |v_f(n_k)| seg_k), and two device calls not at all.
 *   vmin[f], vmax[f]  over the finite samples at n_0 .. n_h (-0.0 below +0.0); +inf / -inf
 *                if there are none
 * A cell without a route gets sink = DYMU_LABEL_NONE, axis = diag = 0, length and integral
 * NaN, vmin = +inf and vmax = -inf.
 * What this route is: the hop-only walk, a chain of grid nodes.  It is not the mostly
 * continuous path dymu_arrive_paths_device returns; length follows the octile metric and
 * overstates a straight run by up to 8.2 %; and with a goal set, sink can differ from the
 * 4-neighbour label of dymu_goal_labels_device. */
typedef struct dymu_route_out {
  /* maps of nx x ny elements, pitch ld elements (>= nx); any may be NULL: not computed */
  uint32_t *sink, *axis, *diag;
  double* length;
  double* integral[DYMU_PATH_FIELDS];
  double* vmin[DYMU_PATH_FIELDS];
  double* vmax[DYMU_PATH_FIELDS];
  uint64_t ld;
} dymu_route_out;
/* The bytes of workspace dymu_route_fields_device needs for these outputs (the pointers of
 * `out` are only tested against NULL; out NULL: every output of n_fields fields).  0 for
 * nx*ny = 0 or >= 2^31 and for n_fields > DYMU_PATH_FIELDS.  The doubling keeps two copies
 * of a 4-byte entry per cell, of the two hop counts if axis, diag or length is asked for,
 * and per field of the 8-byte aggregates asked for: at most 2 * (12 + 24 n_fields) bytes a
 * cell.  An integral, vmin or vmax beyond n_fields must be NULL. */
size_t dymu_route_fields_workspace(uint32_t nx, uint32_t ny, uint32_t n_fields,
                                   const dymu_route_out* out);
/* The routes of all cells of dT for the seeds (HOST array) over the fields d_fields[f]
 * (HOST array of n_fields <= DYMU_PATH_FIELDS device maps, pitch field_ld[f] >= nx, HOST
 * array; as dymu_path_stats_device takes them) into the device maps of *out.  A NULL output
 * is not carried through the rounds and costs nothing.  d_workspace: device memory of at
 * least dymu_route_fields_workspace(...) bytes, 256-byte aligned, the caller's (plain
 * cached device memory, dymu_device_alloc_cached, serves the random gathers best); the call
 * allocates and frees nothing map-sized.  *rounds (may be NULL) = doubling rounds run,
 * about log2 of the longest route (DYMU_ERR_NOT_CONVERGED beyond 32; 31 always suffice).
 * A batch plane is an ordinary map pointer.  Asynchronous on `stream` but for the reads of
 * the round counters (one every four rounds): the outputs are complete once the stream
 * has drained.  One call at a time per context.  DYMU_ERR_ARG: what dymu_goal_labels_device
 * rejects, dymu_path_stats_device's field-list errors, a NULL out or workspace, out->ld <
 * nx, a per-field output beyond n_fields, workspace_bytes too small. */
int dymu_route_fields_device(dymu_ctx* ctx, const double* dT, uint32_t nx, uint32_t ny,
                             uint64_t ld, double res, const dymu_seed* seeds, uint32_t n_seeds,
                             const double* const* d_fields, const uint64_t* field_ld,
                             uint32_t n_fields, const dymu_route_out* out, void* d_workspace,
                             size_t workspace_bytes, void* stream, uint32_t* rounds);
/* Device time (ms, HIP events) of the last dymu_route_fields_device, first kernel to last;
 * waits for it.  DYMU_ERR_STATE before the first one. */
int dymu_last_route_fields_ms(dymu_ctx* ctx, double* ms);
/* ... and its parts: stage_ms[0] the init and root kernels, [1] the rounds (the counter
 * reads between them included), [2] the finalize kernel. */
int dymu_last_route_fields_stages(dymu_ctx* ctx, double stage_ms[3]);
/* ---- how much of the map drains through every cell (DyMuPathPlanner::getRouteUsage) ----
 * The upstream question on the forest of dymu_route_fields_device.  A function of T (nx x
 * ny, pitch ld, nx*ny < 2^31), of the seed list and of an optional weight map alone, the
 * same on host and device.  root, rp(c), route(c) and "no route" are
 * dymu_route_fields_device's, word for word.  w(c) = d_weight[j*weight_ld + i] (uint32);
 * with a NULL weight map w(c) = 1 for every cell.  sub(c) = the cells d that have a route
 * and whose route contains c (c itself if it has a route).
 * Per cell with a route:
 *   usage   the sum over d in sub(c) of w(d), uint64: integers, below 2^31 * 2^32, no
 *           overflow; a leaf holds w(c)
 *   far     the maximum over d in sub(c) of T[d]: the cost-to-go of the costliest start
 *           that passes through c, so far[c] >= T[c]
 *   sink    the root k the route ends on, as dymu_route_out.sink
 * A cell without a route (a dead-end tree is entirely without one) gets usage 0, far NaN,
 * sink DYMU_LABEL_NONE.  catchment[k] (HOST, n_seeds entries) = usage at root k's cell, 0
 * for a seed that is no root (dominated, or a duplicate that lost its cell).
 * Two calls give identical bytes, and device and host are equal bit for bit.  far is
 * specified for maps whose routed cells have T >= +0.0 and finite, which every solve
 * leaves; the contract ends there (a -0.0 or a negative T in a routed cell leaves far
 * unspecified; usage and sink hold for every map). */
typedef struct dymu_usage_out {
  /* maps of nx x ny elements, pitch ld elements (>= nx); any may be NULL: not computed,
   * and what only it needs is not carried */
  uint64_t* usage;
  double* far;
  uint32_t* sink;
  uint64_t ld;
} dymu_usage_out;
/* The bytes of workspace dymu_route_usage_device needs for these outputs (the pointers of
 * `out` are only tested against NULL; out NULL: every output).  0 for nx*ny = 0 or >= 2^31.
 * 512 bytes of counters, two 4-byte entries a cell, two 8-byte sums a cell if usage is
 * asked for, one 8-byte maximum a cell if far is: at most 32 bytes a cell.  The catchment
 * needs the sums: size a call that wants it with a non-NULL usage. */
size_t dymu_route_usage_workspace(uint32_t nx, uint32_t ny, const dymu_usage_out* out);
/* usage, far and sink of all cells of dT for the seeds (HOST array) and the weights
 * (device, pitch weight_ld >= nx; NULL: unit weights) into the device maps of *out, and
 * the catchments into the HOST array catchment (may be NULL).  d_workspace: device memory
 * of at least dymu_route_usage_workspace(...) bytes (with the sums if catchment is given),
 * 256-byte aligned, the caller's (dymu_device_alloc_cached); the call allocates and frees
 * nothing map-sized.  Its first 64 uint32 hold, after the call, per round r the entries
 * still open after it ([r]) and the entries that sent -- one 8-byte atomic per carried
 * array each -- in it ([32 + r]).  *rounds (may be NULL) = doubling rounds run
 * (DYMU_ERR_NOT_CONVERGED beyond 32; 31 always suffice).  A batch plane is an ordinary map
 * pointer.  Asynchronous on `stream` but for the reads of the round counters (one every
 * four rounds) and, with a catchment, a final wait: the outputs are complete once the
 * stream has drained.  One call at a time per context.  DYMU_ERR_ARG, before any device
 * work: what dymu_route_fields_device rejects that applies here (a NULL ctx, map, out or
 * workspace, nx or ny 0, ld or out->ld < nx, nx*ny >= 2^31, a bad seed list, a misaligned
 * workspace), weight_ld < nx with a weight map, all of usage, far, sink and catchment
 * NULL, workspace_bytes too small. */
int dymu_route_usage_device(dymu_ctx* ctx, const double* dT, uint32_t nx, uint32_t ny,
                            uint64_t ld, const dymu_seed* seeds, uint32_t n_seeds,
                            const uint32_t* d_weight, uint64_t weight_ld,
                            const dymu_usage_out* out, uint64_t* catchment, void* d_workspace,
                            size_t workspace_bytes, void* stream, uint32_t* rounds);
/* Device time (ms, HIP events) of the last dymu_route_usage_device, first kernel to last;
 * waits for it.  DYMU_ERR_STATE before the first one. */
int dymu_last_route_usage_ms(dymu_ctx* ctx, double* ms);
/* ... and its parts: stage_ms[0] the init and root kernels, [1] the rounds (the counter
 * reads between them included), [2] the final kernels. */
int dymu_last_route_usage_stages(dymu_ctx* ctx, double stage_ms[3]);
/* ... and round by round: round_ms[r] for r < *rounds (the rounds launched, those behind
 * the closing one included; round_ms holds 32 entries).  A counter read falls into the
 * round after it. */
int dymu_last_route_usage_round_ms(dymu_ctx* ctx, double round_ms[32], uint32_t* rounds);

/* ---- batched solves: many maps in one pass sequence ----
 * A batch is B planes of nx x ny cells stacked into ONE domain of nx x (B * P) cells with
 * pitch ld, where P = dymu_batch_plane_rows(ny) = 16 * ceil((ny + 1) / 16) is the plane
 * pitch in rows: plane b, row j lives at stacked row b * P + j.  Rows ny .. P-1 of every
 * plane (at least one, and every plane starts on a tile boundary of the 8- and the
 * 16-cell tiles) are wall rows: F = +inf there, hence T = +inf after a solve.  The update
 * ignores a +inf neighbour, so the planes cannot influence each other, while their fronts
 * advance in the same passes: the pass count stays about that of one map and each pass
 * does B times the work.  A stack costs 16 * B * nx * P bytes for F and T together.
 * A plane is an ordinary map at dT_stack + b * P * ld (pitch ld): dymu_extract_paths_device,
 * dymu_goal_labels_device and the copy helpers work on it unchanged.
 * dymu_batch_plane_rows returns 0 where P does not fit in uint32_t (ny >= 2^32 - 16). */
uint32_t dymu_batch_plane_rows(uint32_t ny);
/* A seed of a batch: cell (i, j) of plane `plane` with start value t0 (as dymu_seed). */
typedef struct dymu_batch_seed {
  uint32_t plane, i, j, reserved;
  double t0;
} dymu_batch_seed;
/* The stacked speed: plane b of dF_stack <- the nx x ny map at src + b * src_plane_stride
 * (device, pitch src_ld; src_plane_stride = 0: one shared map replicated B times), every
 * wall row +inf.  Asynchronous on `stream`.  DYMU_ERR_ARG: B = 0, ld or src_ld < nx,
 * B * P not fitting in uint32_t. */
int dymu_stack_speed_device(dymu_ctx* ctx, const double* src, uint64_t src_ld,
                            uint64_t src_plane_stride, uint32_t nx, uint32_t ny, uint32_t B,
                            double* dF_stack, uint64_t ld, void* stream);
/* The cold multi-source solve (dymu_solve_seeds_device) of the whole stack: every plane
 * converges to the map its own seeds give on its own speed.  seeds: HOST array; several
 * seeds with offsets per plane are allowed (a batch of goal sets).  deterministic and
 * exact_sqrt as for any solve; stats are those of the stacked domain.  DYMU_ERR_ARG: B = 0,
 * ld < nx, a seed with plane >= B or off its plane, t0 negative, NaN or infinite, a plane
 * without a seed, B * P not fitting in uint32_t.  Blocks until converged. */
int dymu_solve_batch_device(dymu_ctx* ctx, const double* dF_stack, double* dT_stack, uint32_t nx,
                            uint32_t ny, uint32_t B, uint64_t ld, const dymu_batch_seed* seeds,
                            uint32_t n_seeds, void* stream, dymu_stats* stats);
/* DyMuPathPlanner::getTotalCost on the device: d_out[b * M + m] (device) = what the
 * planner returns for point d_xy[2m], d_xy[2m+1] (device; grid-local metres) on plane b
 * taken as a converged map of resolution res -- the nearest node (or +inf) where a corner
 * of the point's cell is off the grid, the nearest node where a corner is not finite, else
 * the reference's bilinear expression; bit-identical to the host's on the same values.
 * Asynchronous on `stream`. */
int dymu_gather_costs_device(dymu_ctx* ctx, const double* dT_stack, uint32_t nx, uint32_t ny,
                             uint32_t B, uint64_t ld, double res, const double* d_xy, uint32_t M,
                             double* d_out, void* stream);

/* ---- combining the planes of a stack: via fields, rendezvous, nearest plane ----
 * d_out[j * out_ld + i] = one left-to-right fold over the listed planes p_0 .. p_{n-1} of
 * cell (i, j), in fp64, operation by operation:
 *   term_k = T[p_k]                    neither weights nor offsets
 *            w_k * T[p_k]              weights only
 *            T[p_k] + o_k              offsets only
 *            w_k * T[p_k] + o_k        both (two roundings)
 *   acc = term_0, arg = p_0; then for k = 1 .. n-1
 *     SUM  acc = acc + term_k
 *     MAX  if (term_k > acc) acc = term_k, arg = p_k
 *     MIN  if (term_k < acc) acc = term_k, arg = p_k
 * so equal terms keep the earlier listed plane, +inf propagates by arithmetic, and the same
 * loop on the host gives the same bits.  A MIN cell that ends at +inf gets arg = 0xFFFFFFFF
 * (no plane reaches it, as DYMU_LABEL_NONE).  d_arg (MAX / MIN only; may be NULL; not
 * written for SUM) receives arg.  planes: HOST list of n_planes <= 65536 plane indices < B,
 * duplicates and any order allowed (the order is part of a SUM's bits); NULL: 0 .. B-1.
 * weights (finite, > 0) and offsets (finite, >= 0): HOST, one per listed plane, or NULL.
 * Only rows 0 .. ny-1 of a plane are read -- never a wall row -- and only columns
 * 0 .. nx-1 of d_out and d_arg are written.  The stack is read only.
 * summary (HOST, may be NULL) describes d_out; equal minima resolve to the lowest row-major
 * cell whatever order the workgroups finish in (per-workgroup partials and a final pass, no
 * atomics).  Without it the call is asynchronous on `stream`; with it, it synchronises.  One
 * call at a time per context (the staged list and the partials are the context's).
 * DYMU_ERR_ARG, before any device work: a null ctx, dT_stack or d_out; nx, ny or B = 0; ld,
 * out_ld or (with d_arg) arg_ld below nx; an unknown op; n_planes = 0 with a list, or above
 * 65536 (B above 65536 without one); a listed plane >= B; a weight not finite or not > 0; an
 * offset negative, NaN or infinite; B * P not fitting in uint32_t; d_out or d_arg overlapping
 * the stack's address range. */
typedef enum { DYMU_REDUCE_SUM = 0, DYMU_REDUCE_MAX = 1, DYMU_REDUCE_MIN = 2 } dymu_reduce_op;
typedef struct dymu_reduce_summary {
  double   min_value;      /* smallest value of out below +inf; +inf when there is none          */
  uint32_t min_i, min_j;   /* its cell: the lowest j*nx+i among equals; 0xFFFFFFFF when none      */
  uint32_t min_plane;      /* d_arg at that cell (MAX/MIN); 0xFFFFFFFF for SUM or when none       */
  uint32_t reserved;
  uint64_t n_finite;       /* cells of out below +inf                                             */
} dymu_reduce_summary;
int dymu_batch_reduce_device(dymu_ctx* ctx, const double* dT_stack, uint32_t nx, uint32_t ny,
                             uint32_t B, uint64_t ld, int op, const uint32_t* planes,
                             uint32_t n_planes, const double* weights, const double* offsets,
                             double* d_out, uint64_t out_ld, uint32_t* d_arg, uint64_t arg_ld,
                             dymu_reduce_summary* summary, void* stream);
/* Device time (ms, HIP events) of the last dymu_batch_reduce_device's kernels; waits for
 * them.  DYMU_ERR_STATE before the first one. */
int dymu_last_reduce_ms(dymu_ctx* ctx, double* ms);
/* The sub-level set of a map: d_mask[j * mask_ld + i] = d_map[j * ld + i] <= bound ? 1 : 0
 * (device bytes, columns 0 .. nx-1 only).  out (HOST, may be NULL): the inclusive box i0, j0,
 * i1, j1 of the marked cells (i0 > i1 when there is none), n_range = their number,
 * r_const = 0.  Asynchronous on `stream` without out, synchronises with it.  DYMU_ERR_ARG: a
 * null ctx, d_map or d_mask, nx or ny = 0, ld or mask_ld below nx, bound NaN or infinite. */
int dymu_level_mask_device(dymu_ctx* ctx, const double* d_map, uint32_t nx, uint32_t ny,
                           uint64_t ld, double bound, uint8_t* d_mask, uint64_t mask_ld,
                           dymu_region* out, void* stream);

/* ---- early exit on target cells for seeded and batched solves ----
 * The cold solves of dymu_solve_seeds_device / dymu_solve_batch_device with a stop test
 * over a list of target cells (HOST array, like the seeds).  A target COUNTS when its
 * speed is finite; a target on a +inf-speed cell is final from the start (its value is
 * +inf by definition) and is ignored.  (This differs from dymu_solve_until_device's
 * five-cell probe, where an obstacle among the start's neighbours reads +inf and makes
 * the solve run to the end.)  The solve returns at the first check at which the smallest
 * key of any queued tile (the key bound of dymu_dom_min_key) exceeds t = max T over all counting targets of all planes, or
 * when the domain has converged; *t_closed = t.  On return every cell of every plane
 * whose converged value is <= *t_closed holds that value (dymu_solve_until_device's
 * contract); other cells hold upper bounds or +inf.  t_plane (host, B doubles, or NULL):
 * t_plane[b] = the maximum over plane b's counting targets -- +inf when one of them is
 * unreachable, 0.0 for a plane with none (such a plane imposes no condition);
 * t_plane[b] <= *t_closed.  A finite-speed target that is unreachable in its plane keeps
 * the whole stack running to convergence: *t_closed = +inf and the result is the full
 * solve's.  Runs a priority kernel (4 or 5) whatever dymu_opts.kernel says;
 * deterministic and exact_sqrt as for any solve; dymu_opts.passes_per_check > 0 checks
 * every that many passes, 0 checks after 16 passes and then every 16.
 * A plane is an ordinary map: dymu_early_exit_mask on plane b with level t_plane[b] (or
 * *t_closed, for everything known final) cuts it back to the reference's exit state.
 * DYMU_ERR_ARG, before any device work: a null pointer (t_plane excepted), n_targets = 0,
 * a target with plane >= B or off its plane, and every argument rule of the solve
 * extended.  Block until the exit. */
typedef struct dymu_cell {
  uint32_t i, j;
} dymu_cell;
typedef struct dymu_batch_cell {
  uint32_t plane, i, j, reserved;
} dymu_batch_cell;
int dymu_solve_seeds_until_device(dymu_ctx* ctx, const double* dF, double* dT, uint32_t nx,
                                  uint32_t ny, uint64_t ld, const dymu_seed* seeds,
                                  uint32_t n_seeds, const dymu_cell* targets, uint32_t n_targets,
                                  void* stream, double* t_closed, dymu_stats* stats);
int dymu_solve_batch_until_device(dymu_ctx* ctx, const double* dF_stack, double* dT_stack,
                                  uint32_t nx, uint32_t ny, uint32_t B, uint64_t ld,
                                  const dymu_batch_seed* seeds, uint32_t n_seeds,
                                  const dymu_batch_cell* targets, uint32_t n_targets, void* stream,
                                  double* t_closed, double* t_plane, dymu_stats* stats);

/* ---- obstacle clearance field and risk-inflated speed ----
 * The clearance field of a speed map: the multi-source solution on the CONSTANT speed c
 * with every obstacle cell of dF -- a cell with !(F < +inf): +inf or NaN -- seeded at 0,
 * i.e. dymu_solve_seeds_device on a map of c with one seed (i, j, 0) per obstacle cell,
 * taken from the device-resident map itself and stopped at the level 1.  With
 * c = global_res / risk_distance the field is the distance to the nearest obstacle in
 * units of the risk distance, and risk = max(1 - S, 0) is the reference's risk
 * (src/DyMu_LocalPathRepairing.cpp:493-576), here for the global layer.
 * dF: read only (by the seeding kernel alone).  dW: a caller-provided work map of nx x ny
 * doubles at pitch ld; the call fills it with c in every cell, obstacles included, and
 * solves on it; the solve never writes the speed map, so on return it still holds c in every
 * cell (what dymu_clearance_update_device starts from).  dS: the output.  On return every
 * cell whose converged value is <= 1 holds that value (within the parity bound
 * 1e-12 * max(1, S); an obstacle cell holds +0.0 exactly); every other cell holds an upper
 * bound of its converged value or +inf -- dymu_solve_seeds_until_device's contract with the
 * level fixed at 1: the solve ends at the first check at which the key bound of
 * dymu_dom_min_key exceeds 1.0, or with nothing queued (checks every
 * dymu_opts.passes_per_check passes when given, else after 16 passes and then every 16).
 * A map without an obstacle cell: dS = +inf everywhere, stats->passes = 0, DYMU_OK.
 * Runs a priority kernel (4 or 5) whatever dymu_opts.kernel says; deterministic and
 * exact_sqrt as for any solve.  stats->ms covers the fill, the seeding and the passes.
 * DYMU_ERR_ARG, before any device work: a null pointer (stats excepted), nx or ny = 0,
 * ld < nx, c not > 0, NaN or infinite.  DYMU_ERR_STATE while stepping is on.  Blocks
 * until the exit. */
int dymu_clearance_device(dymu_ctx* ctx, const double* dF, double* dW, double* dS, uint32_t nx,
                          uint32_t ny, uint64_t ld, double c, void* stream, dymu_stats* stats);
/* The field after obstacles were ADDED inside a window, without a whole solve.
 * Preconditions: dS meets dymu_clearance_device's contract for an old mask on the same grid,
 * pitch and c; dW holds c in every cell, as that call left it; the obstacle set of dF
 * (!(F < +inf)) is the old one plus cells inside the window [i0, i0+w) x [j0, j0+h), which
 * is clipped to the grid.  Adding obstacles can only lower the field, so the old field is an
 * upper bound of the new one and nothing is reset: the window's cells that are obstacles in
 * dF and do not hold +0.0 yet are seeded at +0.0 (their tiles and, on a tile edge, the tiles
 * across it queued with key 0, as the cold seeding does), and the priority passes run to the
 * level 1 as in dymu_clearance_device.  They reach exactly as far as values change.
 * Postcondition: dS meets the same contract for the new mask.  box (may be NULL) receives
 * {i0, j0, w, h} in cells: the bounding box of the tiles (8 x 8 cells for kernel 4, 16 x 16
 * for kernel 5) that a list of the call held, clipped to the grid; every cell of dS outside
 * it is bit for bit what it was, the columns nx .. ld-1 included, and dF and dW are not
 * written at all.  The box is reported, not derived: no geometric bound on how far a value
 * <= 1 can change is proven for the discrete scheme.  With no new obstacle cell in the
 * window: box = {i0, j0, 0, 0}, stats->passes = 0, nothing written.
 * A cell of the window that is finite in dF but holds +0.0 in dS is a freed obstacle, which
 * a decrease-only update cannot handle: DYMU_ERR_STATE, nothing written (the window is
 * counted before it is seeded).  Obstacles freed or added outside the window are not seen.
 * Always runs a priority kernel; deterministic and exact_sqrt as for any solve.  stats->ms
 * covers the count, the seeding and the passes.  DYMU_ERR_ARG, before any device work: a
 * null pointer (box and stats excepted), nx or ny = 0, ld < nx, c not > 0, NaN or infinite,
 * w or h = 0, i0 >= nx, j0 >= ny.  DYMU_ERR_STATE while stepping is on.  Blocks until the
 * exit. */
int dymu_clearance_update_device(dymu_ctx* ctx, const double* dF, double* dW, double* dS,
                                 uint32_t nx, uint32_t ny, uint64_t ld, double c, uint32_t i0,
                                 uint32_t j0, uint32_t w, uint32_t h, void* stream,
                                 uint32_t box[4], dymu_stats* stats);
/* The field after the obstacle set changed in ANY way inside a window -- cells added, cells
 * freed, or both -- without a whole solve.  Arguments, preconditions and
 * argument errors are dymu_clearance_update_device's, except that the obstacle set of dF may
 * differ from the old one in any way inside the clipped window.
 * Every state the passes leave is a supersolution: a cell's value was the update of its
 * neighbours when it was written, and they only fell afterwards.  The call sets the freed
 * cells (finite in dF, +0.0 in dS) to +inf and then every finite cell, obstacle cells of dF
 * excepted, whose update from its current neighbours exceeds its value by more than 1e-13
 * relative, until nothing changes (a raise front on 16 x 16 tiles from the window's tiles,
 * whatever the pass kernel's tile is).  What is left bounds the new field from above, and a
 * kept converged value <= 1 is the new value.  The added cells are then seeded at +0.0, the
 * tiles the raise claimed that hold a +inf cell of finite dF beside a finite cell are queued
 * with the smallest such neighbour value as their key, and the priority passes run to the
 * level 1 as in dymu_clearance_update_device.
 * Postcondition: dS meets dymu_clearance_device's contract for the mask of dF; a freed cell
 * no longer holds +0.0.  box as in dymu_clearance_update_device, over the tiles the raise
 * and the passes each claimed: every cell of dS outside it is bit for bit what it was, every
 * cell either wrote lies inside it; dF, dW and the columns nx .. ld-1 are not written.  The
 * raise ends where the values of the old solve end: no bound short of that is proven.  With
 * no added and no freed cell in the window: box = {i0, j0, 0, 0}, stats->passes = 0, nothing
 * written.  dymu_last_update_stats afterwards: {raise passes, raise tile visits, cells
 * invalidated, 0}, zeros when nothing was freed.  stats->ms covers the count, the raise, the
 * seeding and the passes.  Always runs a priority kernel; deterministic and exact_sqrt as
 * for any solve, and in deterministic mode two calls from the same state give the same
 * bytes.  DYMU_ERR_STATE while stepping is on.  Blocks until the exit. */
int dymu_clearance_edit_device(dymu_ctx* ctx, const double* dF, double* dW, double* dS,
                               uint32_t nx, uint32_t ny, uint64_t ld, double c, uint32_t i0,
                               uint32_t j0, uint32_t w, uint32_t h, void* stream,
                               uint32_t box[4], dymu_stats* stats);
/* The risk folded into the speed, per cell and operation by operation:
 *   R = fmax(1.0 - S, 0.0);  out = F * (risk_ratio * R + 1.0)
 * so S > 1, S = +inf and risk_ratio = 0 give F bit for bit, and an obstacle stays +inf or
 * NaN by arithmetic.  dOut may be dF.  Asynchronous on `stream`.  DYMU_ERR_ARG: a null
 * pointer, nx or ny = 0, ld < nx, risk_ratio negative, NaN or infinite. */
int dymu_inflate_speed_device(dymu_ctx* ctx, const double* dF, const double* dS, double* dOut,
                              uint32_t nx, uint32_t ny, uint64_t ld, double risk_ratio,
                              void* stream);

/* ---- row-slab domains (multi-GPU sharding; also single-GPU virtual slabs) ----
 * A rank owns rows [row0, row0+nrows) of an nx-wide global grid.  T points at
 * its first owned row; with ghost_lo the row above it (T - ld) holds the
 * neighbour rank's last row, with ghost_hi the row T + nrows*ld holds the
 * next rank's first row (then nrows must be a multiple of the tile height: 8 for
 * kernels 3 and 4, 16 for kernel 5; dymu_slab_rows cuts on multiples of 32).  Ghost
 * rows are read-only halo for the kernels: only dymu_dom_begin (+inf) and the merges
 * below write them, and no call touches the columns nx .. ld-1 of any row, a row
 * beyond a ghost row, or the ghost slot of a side whose flag is 0.
 * Protocol (bench_sharded.py / dymu.sharded):
 *   dymu_dom_begin -> repeat { dymu_dom_run(K passes); exchange boundary rows
 *   (RCCL); dymu_dom_merge_ghosts(received rows) } until the all-reduced
 *   pending count is 0 -> dymu_dom_finish.
 * or, on kernel-5 slabs (include/dymu_dist.h's native loop):
 *   dymu_dom_begin -> repeat { dymu_dom_round(K passes, merging the rows the
 *   previous exchange received); exchange boundary rows } until 0 -> finish.
 * All calls except dymu_dom_pending / dymu_dom_finish are asynchronous on
 * `stream`. */
typedef struct dymu_domain {
  const double* F; /* owned rows, pitch ld (device) */
  double* T;       /* owned row 0 (device); ghost rows at T - ld / T + nrows*ld */
  uint64_t ld;
  uint32_t nx, nrows;
  int32_t ghost_lo, ghost_hi;
} dymu_domain;

/* Partition ny rows over nranks slabs (boundaries on multiples of 32 rows). */
int dymu_slab_rows(uint32_t ny, uint32_t nranks, uint32_t rank, uint32_t* row0, uint32_t* nrows);
/* Initialise T (owned + ghost rows = +inf) and seed the goal if it lies in
 * this slab (goal_j_local = goal row - row0, or -1). */
int dymu_dom_begin(dymu_ctx* ctx, const dymu_domain* dom, int64_t goal_i, int64_t goal_j_local,
                   void* stream);
/* Launch `passes` FIM passes (speculative passes with no active tile are cheap). */
int dymu_dom_run(dymu_ctx* ctx, uint32_t passes, void* stream);
/* Min-merge received neighbour rows (device pointers, nx doubles, or NULL)
 * into the ghost rows and queue the tiles under improved columns; if
 * d_pending != NULL also write the number of queued tiles there (int32).
 * The merge rule (also dymu_dom_exchange's and the fused rounds'): a ghost value
 * is replaced only by a received value STRICTLY below it.  An equal value and a
 * NaN write nothing and queue nothing, so merging the same rows again is a no-op.
 * Tile trow * ntx + i / tile_w is queued when a column i of it improved, trow = 0
 * for new_lo and the last tile row for new_hi (tiles are 8 x 8 cells for kernels 3
 * and 4, 16 x 16 for kernel 5); a tile is in the list at most once per pass,
 * whichever sides and however many merges reach it.  A NULL side leaves its ghost
 * row alone.  The count is that of the whole list the next pass reads: tiles the
 * passes queued plus merged ones.  DYMU_ERR_STATE without a live domain;
 * DYMU_ERR_ARG for a row on a side without a ghost. */
int dymu_dom_merge_ghosts(dymu_ctx* ctx, const double* new_lo, const double* new_hi,
                          int32_t* d_pending, void* stream);
/* dymu_dom_merge_ghosts with the queued-tile count in the SAME launch (the
 * native sharded loop's per-round step, include/dymu_dist.h): *d_total (device
 * int32, required) receives the number of tiles queued for the next pass. */
int dymu_dom_exchange(dymu_ctx* ctx, const double* new_lo, const double* new_hi,
                      int32_t* d_total, void* stream);
/* One round with the ghost merge inside the passes: `passes` (>= 2) FIM passes,
 * the first of which min-merges the received rows (device, nx doubles, or NULL)
 * into the ghost rows; *d_total (device int32) receives the tiles queued for
 * the round's first pass plus those queued for its second (0 on every rank =
 * fixed point).  Replaces dymu_dom_run + dymu_dom_exchange for the rows of the
 * PREVIOUS round (one launch per round fewer).  Only for domains on kernel 5:
 * DYMU_ERR_STATE otherwise; dymu_dom_round_supported says which (1 / 0). */
int dymu_dom_round_supported(dymu_ctx* ctx, uint32_t passes);
/* 1 if a domain of nx x nrows cells would support fused rounds of `passes` (the
 * check dymu_dom_round_supported makes after dymu_dom_begin), before any domain
 * exists: the sharded solver's pre-flight rejects an unsupported peer-transport
 * solve on every rank with DYMU_ERR_ARG instead of aborting the communicator. */
int dymu_dom_round_capable(dymu_ctx* ctx, uint32_t nx, uint32_t nrows, uint32_t passes);
int dymu_dom_round(dymu_ctx* ctx, uint32_t passes, const double* new_lo, const double* new_hi,
                   int32_t* d_total, void* stream);
/* Arm a post for the next launched pass: its block 0 stores *d_src (device
 * int32) into the context's host-coherent mailbox with sequence *seq, so the
 * host can read a device value (the all-reduced count) without a copy or a
 * stream synchronisation; dymu_dom_wait_post spins for it (timeout_s > 0:
 * DYMU_ERR_HIP after that long).  DYMU_ERR_STATE without a mailbox. */
int dymu_dom_post(dymu_ctx* ctx, const int32_t* d_src, uint32_t* seq);
int dymu_dom_wait_post(dymu_ctx* ctx, uint32_t seq, double timeout_s, int32_t* value,
                       void* stream);
/* Peer rounds (include/dymu_dist.h's GPU-initiated peer transport):
 * dymu_dom_round whose first pass also PUSHES this rank's first / last owned row
 * into the neighbours' receive rows (peer-mapped device memory) -- only the
 * values below those last pushed -- and, from the pass's last workgroup, writes a
 * sequence tag after them (system-scope release); the merge of the same pass reads
 * this rank's own receive rows after their tags.  No host involvement and no wait
 * on a neighbour: rows arrive whenever the neighbour's pass runs, and any mix of
 * old and new values is a valid upper bound.  The round's second pass records in
 * `ctl` the status a termination check needs: P (tiles queued for the round's two
 * first passes), S per side (pushes that carried a decrease) and R per side (the
 * smallest tag the round's merge read).  Kernel-5 domains, passes >= 2.
 * Initial state, set by the caller before the first round of a solve: `ctl` all
 * zero bytes except bytes 32 .. 47 (the two words holding the smallest tag read per
 * side), which are all ones; every `last` row and every receive row +inf; every
 * tag 0.  A tag counts the pushes that carried a decrease: it stays 0 for a
 * boundary row that never becomes finite, and +inf is never pushed. */
#define DYMU_PEER_CTL_BYTES 128
typedef struct dymu_peer_links {
  const double* recv[2];                 /* own receive rows: from rank-1 (0) / rank+1 (1) */
  const unsigned long long* recv_tag[2]; /* their tags (written by the neighbours) */
  double* send[2];                       /* the neighbours' receive rows for the first (0) /
                                            last (1) owned row (peer-mapped), NULL = none */
  unsigned long long* send_tag[2];       /* ... and their tags */
  double* last[2];                       /* nx values last pushed per side (device) */
  void* ctl;                             /* DYMU_PEER_CTL_BYTES of device memory */
} dymu_peer_links;
int dymu_dom_round_peer(dymu_ctx* ctx, uint32_t passes, const dymu_peer_links* links,
                        void* stream);
/* Arm a status post for the next launched pass: its block 0 stores the status of
 * `ctl` (S0, S1, R0, R1) at dst[1..4], then (seq << 32) | P at dst[0] (release,
 * system scope).  dst: device address of 5 words of host-coherent memory. */
int dymu_dom_post_status(dymu_ctx* ctx, const void* ctl, unsigned long long* dst, uint32_t seq);
/* Tiles queued for the next pass (synchronises `stream`). */
int dymu_dom_pending(dymu_ctx* ctx, void* stream, uint64_t* pending);
/* End the domain solve; fills stats (passes, visits, sweeps). */
int dymu_dom_finish(dymu_ctx* ctx, void* stream, dymu_stats* stats);

/* ---- stepping: a device-resident entry stopped after its preparation ----
 * With stepping on, dymu_solve_device, dymu_solve_seeds_device, dymu_solve_batch_device,
 * dymu_resolve_window_device, dymu_update_window_device, dymu_update_seeds_window_device
 * and dymu_update_batch_window_device do everything up to their first pass -- the fill
 * and the seeds of a cold solve; theta, the reset (or the raise front) and the queued
 * tiles of an update -- then synchronise `stream` and return DYMU_OK with the domain
 * LIVE and *stats untouched.  The caller runs the passes with dymu_dom_run, reads
 * dymu_dom_pending / dymu_dom_min_key between them and ends with dymu_dom_finish
 * (stats.ms = 0); the map after the pass at which nothing is pending is the one the
 * entry would have returned.  dymu_last_update_stats is valid as soon as the entry has
 * returned.  The entries that cannot leave a domain behind return DYMU_ERR_STATE while
 * stepping is on: dymu_solve, dymu_resolve_window (host buffers) and the *_until_*
 * entries.  Off (the default) nothing changes.  For tests and diagnostics. */
int dymu_set_stepping(dymu_ctx* ctx, int on);
/* *key = the smallest priority key of the list the next pass reads, +inf when no tile is
 * queued (synchronises `stream`).  The key bound every early exit rests on: before every
 * pass, every cell whose value a later pass will still change ends at a value >= *key
 * (within the parity bound 1e-12 * max(1, *key), which covers kernel 5's sweep sqrt).
 * So once *key exceeds a value v, every cell whose converged value is <= v already holds
 * it.  The keys: a seed (the goal: value 0) queues its own tile and (kernels 4 and 5; kernel
 * 3 has no keys and queues the seed's tile only), where its cell lies on a tile edge, the
 * tile across that edge -- whose cell next to the seed is updated
 * from a value no visit changes -- each keyed with its smallest such seed value; a tile queued
 * by a visit of its neighbour has the smallest value that visit changed on the shared
 * edge; a tile deferred by key or by colour, or re-queued after a capped visit, keeps the
 * key it had; the tiles an update queues have theta (below), a seed's tile its smallest
 * t0 if that is lower.  A tile's key is the minimum over everything that queued it.
 * DYMU_ERR_STATE without a live domain and for a domain on kernel 3 (no keys). */
int dymu_dom_min_key(dymu_ctx* ctx, void* stream, double* key);

/* ---- the state a domain starts from and carries between passes (tests, diagnostics) ----
 * What an engine keeps from one solve to the next -- the tile-epoch stamps, the three
 * lists with their counters, keys and histograms, the edge columns -- copied out of the
 * LIVE domain (the one a stepped entry or dymu_dom_begin left) after a synchronisation
 * of `stream`.  Read-only: the domain runs on as if the call had not been made.
 * Scalars are always filled.  Each array goes to the host buffer given for it, or is
 * skipped when that pointer is null; a buffer shorter than the array (its *_cap, in
 * elements) is DYMU_ERR_ARG, so call once without buffers to learn the sizes. */
typedef struct dymu_dom_state {
  /* out */
  uint32_t eb;         /* the domain's epoch base: the seed's tiles carry eb + 1, the tiles
                          listed for pass p carry eb + p + 1, no stamp exceeds that */
  uint32_t ntiles;     /* tiles of the domain */
  uint32_t tiles_cap;  /* entries of the tile-epoch array (>= ntiles) */
  int32_t variant;     /* pass kernel: 3, 4 or 5 */
  uint64_t p;          /* index of the next pass; it reads list p % 3 */
  const double* F;     /* device addresses and shape the passes use */
  double* T;
  uint64_t ld;
  uint32_t nx, ny;
  int32_t has_keys;    /* kernels 4 and 5: keys, hist, minkey, base, delta are valid */
  int32_t has_ec;      /* kernel 5 with edge columns: ec is valid */
  uint64_t list_n;     /* entries of the list the next pass reads (sum of its counters) */
  uint64_t minkey[3];  /* per list: bits of its smallest key (+inf: none) */
  double base[3];      /* per list: origin of its histogram */
  double delta;        /* histogram bin width */
  /* in: host buffers (null: skipped) and their capacities in elements */
  uint32_t* tile_epoch;     /* tiles_cap stamps */
  uint64_t tile_epoch_cap;
  uint32_t* counts;         /* 3 lists x 16 shards, list-major (always 48 words) */
  uint32_t* list_raw;       /* the next pass's list, shard after shard: entries as stored */
  uint32_t* list_tile;      /* ... and their tile indices (the key-bin field masked off) */
  uint64_t list_cap;        /* of each of the two; 16 * ntiles always suffices */
  uint64_t* keys;           /* 3 lists x ntiles key bits, list-major */
  uint64_t keys_cap;
  uint32_t* hist;           /* 3 lists x 16 shards x 64 bins (always 3072 words) */
  double* ec;               /* 32 * ntiles: per tile its column 0, then its column 15 */
  uint64_t ec_cap;
} dymu_dom_state;
/* DYMU_ERR_STATE without a live domain, and (with nothing copied from the lists, the
 * reason in dymu_last_error) if a shard counter exceeds the shard's capacity. */
int dymu_dom_snapshot(dymu_ctx* ctx, void* stream, dymu_dom_state* state);
/* epoch_base = max(epoch_base, value): the next domain's eb.  Only while no domain is
 * live (else DYMU_ERR_STATE), and only ever upwards, so it cannot by itself leave a
 * stamp above the base.  Its one purpose: 4 * 10^9 passes on one engine bring the base
 * to the wrap guard of the 32-bit epochs (a domain that could reach 0xFFFFFFF0 clears
 * the stamps and restarts at 0); this brings the guard within reach of a test. */
int dymu_debug_raise_epoch_base(dymu_ctx* ctx, uint32_t value);

/* Synthetic input generator on the device (bench/test data):
 *   F[k] = 1 + 4*u(seed, k),  u(s,k) = (splitmix64(s ^ k) >> 11) * 2^-53,
 *   obstacle (F = +inf) where u(obst_seed, k) < obst_frac, except the 3x3
 *   block around (goal_i, goal_j).  k = j*nx + i is the GLOBAL cell index, so
 *   shards generate identical values: rows [row0, row0+ny) of a grid nx wide. */
int dymu_synth_speed(dymu_ctx* ctx, double* dF, uint32_t nx, uint32_t ny, uint64_t ld,
                     uint64_t row0, uint64_t seed, double obst_frac, uint64_t obst_seed,
                     uint32_t goal_i, uint32_t goal_j, void* stream);

/* Arithmetic self-test: out[k] = the kernels' Eikonal candidate for
 * (Tx[k], Ty[k], C[k]) (reference :531-535), computed by the same device code
 * the pass kernels use (fast = 1: the range-restricted correctly rounded sqrt in
 * the reference's combine, kernels 3/4; fast = 2: kernel 5's default sweep
 * candidate, monotone combine + one Goldschmidt step; fast = 3: kernel 5 with
 * exact_sqrt, monotone combine + correctly rounded sqrt; fast = 4: the v31 sweep
 * candidate, kept for A/B).
 * Device pointers; blocks until done. */
int dymu_eikonal_batch(dymu_ctx* ctx, const double* tx, const double* ty, const double* c,
                       double* out, uint64_t n, int fast);

/* Scheduling self-test: one wave runs the list scan every priority pass starts with
 * (the shard prefix sums and the threshold bin b*) on the given inputs.
 * counts: 16 shard counts; hist: the 16 x 64 key histogram (shard-major); target,
 * target_frac, cap_frac: the pass's target in tiles, as at least this fraction of
 * the listed tiles, and as at most this fraction (not below 256 tiles; 0 = no cap).
 * prefix[0..16]: prefix[k] = counts[0] + .. + counts[k-1] (mod 2^32); *bstar: the
 * first of bins 0..62 whose inclusive histogram prefix reaches the target, or 64 when
 * target is 0, the list is no longer than the target, or no bin reaches it.
 * Host pointers; blocks until done. */
int dymu_pass_scan_probe(dymu_ctx* ctx, const uint32_t* counts, const uint32_t* hist,
                         uint32_t target, float target_frac, float cap_frac, uint32_t* prefix,
                         int32_t* bstar);

/* Device memory helpers (so a host without torch can run the device path).
 * dymu_device_alloc returns uncached device memory (hipDeviceMallocUncached: no L2
 * lines of the maps are left dirty for each pass's end-of-kernel release to write
 * back -- 27.5 vs 28.1 ms per 16384^2 solve); DYMU_MAP_MEM=0 gives
 * plain hipMalloc memory, 1 fine-grained.  Any device memory works with the solve
 * entry points.  The copies are ordered after the work queued on the context stream
 * and are complete on return. */
int dymu_device_alloc(dymu_ctx* ctx, size_t bytes, void** dptr);
int dymu_device_free(dymu_ctx* ctx, void* dptr);
/* plain hipMalloc memory (L2-cached), whatever DYMU_MAP_MEM says: for buffers read by
 * random gathers, such as dymu_goal_labels_device's d_label.  Freed by dymu_device_free. */
int dymu_device_alloc_cached(dymu_ctx* ctx, size_t bytes, void** dptr);
int dymu_memcpy_d2h(dymu_ctx* ctx, void* dst, const void* src, size_t bytes);
int dymu_memcpy_h2d(dymu_ctx* ctx, void* dst, const void* src, size_t bytes);
/* pitched copies (hipMemcpy2D: width bytes per row, height rows) */
int dymu_memcpy2d_d2h(dymu_ctx* ctx, void* dst, size_t dpitch, const void* src, size_t spitch,
                      size_t width, size_t height);
int dymu_memcpy2d_h2d(dymu_ctx* ctx, void* dst, size_t dpitch, const void* src, size_t spitch,
                      size_t width, size_t height);
/* page-lock a host buffer for full-speed DMA (hipHostRegister) / undo it */
int dymu_host_register(dymu_ctx* ctx, void* p, size_t bytes);
int dymu_host_unregister(dymu_ctx* ctx, void* p);

/* ---- dynamic update: windowed re-propagation ----
 * After the speed changed only inside the window [i0, i0+w) x [j0, j0+h)
 * (the local layer's hazard / trafficability writes, reference
 * src/DyMu_LocalPathRepairing.cpp:264-274, :389-394, entering F through
 * src/DyMu_GlobalPathPlanning.cpp:527-528), bring T from the converged map of
 * the old speed to that of the new one without a cold solve: cells whose old
 * T is below theta = min(old T over the window and its 1-cell ring) provably
 * keep their value; the rest is reset and re-propagated from the boundary of
 * the kept region.  With DYMU_RAISE=1 a raise front instead
 * sets to +inf exactly the cells whose converged value is no longer supported
 * under the new speed (the window's dependency cone; cells supported within
 * 1e-13 relative keep their value) and the FIM re-propagates the cone from its
 * boundary -- exact and smaller, but slower on config 5.
 * Increases and decreases are both handled; the result is the fixed point a
 * cold dymu_solve of the new speed reaches.
 * The window is clipped to the grid.
 *
 * The preparation, exactly (what dymu_set_stepping exposes; tiles are 8 x 8 cells for
 * kernels 3 and 4, 16 x 16 for kernel 5; a tile is queued at most once):
 * Theta reset (decrease_only = 0, no DYMU_RAISE).  theta = the minimum of old T over the
 *   clipped window grown by one cell on every side and clipped again (+inf when all of
 *   it is +inf).  A cell with old T >= theta is set to +inf, except the goal and cells
 *   that already hold +inf; every other cell is not written (kept bit for bit, the
 *   columns nx .. ld-1 included).  A tile is queued when it holds a cell with old
 *   T >= theta (the goal excepted) of finite new speed that has an in-grid 4-neighbour
 *   which is kept: old T < theta, or the goal.  The queued tiles are keyed theta.
 * Decrease-only.  Nothing is written.  The tiles that meet the clipped window are
 *   queued, keyed theta.
 * Raise (DYMU_RAISE=1, decrease_only = 0).  The invalidated set S is the largest set of
 *   live cells (finite old T, not the goal) such that every cell of S has new speed +inf
 *   (or NaN), or has u > T * (1 + 1e-13), u being the reference update (:531-535) under
 *   the new speed of its in-grid 4-neighbours' values with the cells of S (and off-grid
 *   neighbours) at +inf.  The front starts from the window's cells and follows
 *   4-neighbours, which finds all of S when T is a fixed point of the update under the
 *   old speed within that tolerance.  S is set to +inf, nothing else is written.  A tile
 *   is queued when it meets the clipped window, or holds a non-goal cell with T = +inf
 *   and finite new speed that has a finite in-grid 4-neighbour; such a tile's key is the
 *   smallest such neighbour value, and the list's smallest key is min(theta, those).
 * dymu_last_update_stats after these single-goal forms: {raise passes, raise tile
 * visits, |S|, 0} for the raise; all zeros for the theta reset (its reset cells are not
 * counted, unlike the seeded form's below) and for decrease-only. */
int dymu_resolve_window_device(dymu_ctx* ctx, const double* dF, double* dT, uint32_t nx,
                               uint32_t ny, uint64_t ld, uint32_t goal_i, uint32_t goal_j,
                               uint32_t i0, uint32_t j0, uint32_t w, uint32_t h, void* stream,
                               dymu_stats* stats);
/* The same with the caller's knowledge of the change: decrease_only != 0
 * promises that no F in the window increased (F grows with hazard density and
 * falls with trafficability, reference :527-528: e.g. a hazard cleared or a
 * trafficability restored after src/DyMu_LocalPathRepairing.cpp:389-394).  Then
 * the old map is a valid upper bound everywhere and no cell is reset: only the
 * window's tiles are seeded and the passes lower what the cheaper window
 * reaches.  decrease_only = 0 is dymu_resolve_window_device. */
int dymu_update_window_device(dymu_ctx* ctx, const double* dF, double* dT, uint32_t nx,
                              uint32_t ny, uint64_t ld, uint32_t goal_i, uint32_t goal_j,
                              uint32_t i0, uint32_t j0, uint32_t w, uint32_t h, int decrease_only,
                              void* stream, dymu_stats* stats);
/* What the last windowed update did before its re-solve: out[0] raise passes,
 * out[1] tiles visited by them, out[2] cells invalidated (the dependency cone of
 * the window's speed increases; 0s for decrease-only updates and for the single-goal
 * theta reset, which does not count the cells it resets), out[3] reserved.  Filled by the
 * update's preparation: valid after a stepped entry has returned (dymu_set_stepping). */
int dymu_last_update_stats(dymu_ctx* ctx, uint64_t out[4]);
/* ---- windowed updates of seeded maps and of stacks ----
 * dymu_update_window_device for a seed list: dT holds the converged multi-source map of
 * `seeds` (dymu_solve_seeds_device) under the old speed, dF the new speed, changed only
 * inside the window; the result is the fixed point dymu_solve_seeds_device reaches on
 * the new speed.  theta = min(old T over the window and its 1-cell ring); cells below it
 * keep their value, every other finite cell is reset -- a seed cell to the smallest t0
 * given for it (a seed is a boundary value, not a goal at 0: a dominated seed in the
 * reset region comes back as min(t0, what propagates)), any other cell to +inf -- and
 * re-propagated from the kept region's boundary and the seeds.  decrease_only != 0 as for
 * dymu_update_window_device: nothing is reset, the window's tiles are queued.  Always
 * the theta reset (DYMU_RAISE is not consulted: the raise front is single-goal).
 * dymu_last_update_stats afterwards: out[0] = out[1] = 0, out[2] = the cells whose finite
 * old value was at or above theta (0 for decrease_only).  seeds: HOST array.  The window
 * is clipped to the grid.
 * The preparation, exactly: the theta reset of dymu_resolve_window_device without an
 * exempt cell -- every finite cell with old T >= theta is set to +inf, every other cell is
 * not written; a tile is queued, keyed theta, when it holds a cell with old T >= theta of
 * finite new speed with an in-grid 4-neighbour of old T < theta -- then every seed is
 * min-written (T = min(T, t0): a kept seed cell is not changed) and every seed's tile,
 * with (kernels 4 and 5) the tile across each tile edge the seed's cell lies on (tile
 * edges of the whole stacked domain), is queued with the smallest t0 of those seeds as a key (a tile's key
 * is the minimum of both; a seed in the reset region has t0 >= theta).  Nothing else is written; a tile is queued
 * at most once; the list's smallest key is theta.  theta = +inf (a window on +inf cells
 * only): no cell is reset and only the seeds' tiles are queued.  DYMU_ERR_ARG, before any device work: a null pointer, ld < nx,
 * dymu_solve_seeds_device's seed rules, w or h = 0, i0 >= nx, j0 >= ny. */
int dymu_update_seeds_window_device(dymu_ctx* ctx, const double* dF, double* dT, uint32_t nx,
                                    uint32_t ny, uint64_t ld, const dymu_seed* seeds,
                                    uint32_t n_seeds, uint32_t i0, uint32_t j0, uint32_t w,
                                    uint32_t h, int decrease_only, void* stream,
                                    dymu_stats* stats);
/* A changed window [i0, i0+w) x [j0, j0+h) of plane `plane` of a batch. */
typedef struct dymu_batch_window {
  uint32_t plane, i0, j0, w, h, reserved;
} dymu_batch_window;
/* The same for the stack of dymu_solve_batch_device (same layout, same seeds), whose
 * speed changed only inside `windows` (HOST array; any number per plane, none included;
 * each clipped to its plane).  The planes are independent, so theta is taken per plane
 * -- the minimum over all of the plane's windows and their rings -- and keys that
 * plane's queued tiles; a plane without a window is not read beyond its theta slot and
 * not written: its map stays bit for bit.  decrease_only != 0 promises it for every
 * window.  dymu_last_update_stats: out[2] = the reset cells summed over the planes, each
 * counted against its own plane's theta.  DYMU_ERR_ARG, before any device work: a null
 * pointer, B = 0, ld < nx, dymu_solve_batch_device's seed rules (a plane without a seed
 * included), B * P not fitting in uint32_t, n_windows = 0, a window with plane >= B,
 * w or h = 0, i0 >= nx or j0 >= ny.  Blocks until converged. */
int dymu_update_batch_window_device(dymu_ctx* ctx, const double* dF_stack, double* dT_stack,
                                    uint32_t nx, uint32_t ny, uint32_t B, uint64_t ld,
                                    const dymu_batch_seed* seeds, uint32_t n_seeds,
                                    const dymu_batch_window* windows, uint32_t n_windows,
                                    int decrease_only, void* stream, dymu_stats* stats);
/* Host-buffer form: requires that the previous dymu_solve / dymu_resolve_window
 * on this context solved the same grid size and goal (DYMU_ERR_STATE otherwise);
 * only the window of F is uploaded, the whole new T is written to T_out. */
int dymu_resolve_window(dymu_ctx* ctx, const double* F, uint32_t nx, uint32_t ny, uint32_t goal_i,
                        uint32_t goal_j, uint32_t i0, uint32_t j0, uint32_t w, uint32_t h,
                        double* T_out, dymu_stats* stats);

/* ---- computeCostMap on the device ----
 * Planner node state (the globalNode fields of reference src/DyMu.hpp:69-108
 * that the global layer uses) as device SoA arrays, row-major, pitch ld. */
typedef struct dymu_cost_state {
  double* cost;         /* smoothed cost; its previous value feeds the smoothing (Q1) */
  double* raw_cost;     /* nominal cost before smoothing */
  double* slope;        /* rad */
  uint32_t* terrain;    /* terrain class, 0 on the border */
  uint8_t* is_obstacle; /* sticky */
  double* hazard;       /* hazard_density */
  double* traff;        /* trafficability */
  int32_t* loc_mode;    /* -1 = "DONT_CARE", else the locomotion index */
} dymu_cost_state;

/* computeCostMap (reference src/DyMu_GlobalPathPlanning.cpp:145-181 with
 * calculateSlope :186-210, calculateNominalCost :217-293, smoothCost
 * :297-308; quirks Q1-Q4) over device arrays elevation / terrain_map (class
 * as double, like the reference's vector<vector<double>>); lut and slopes are
 * HOST arrays (the reference's cost_data / slope_values).  If dF is not NULL
 * the speed F = (res*cost)*((2+hazard)-traff), +inf for obstacles (:527-528),
 * is written too.  Asynchronous on `stream` (NULL: the context's stream).
 * nx, ny >= 2.  A terrain class beyond the LUT marks the cell as an obstacle
 * (the reference reads out of bounds there). */
int dymu_compute_cost_map(dymu_ctx* ctx, uint32_t nx, uint32_t ny, uint64_t ld, double global_res,
                          const double* lut, int lut_len, const double* slopes, int n_slopes,
                          int n_locs, const double* elevation, const double* terrain_map,
                          const dymu_cost_state* st, double* dF, void* stream);

/* The speed alone from the state (after hazard / trafficability updates). */
int dymu_pack_speed(dymu_ctx* ctx, uint32_t nx, uint32_t ny, uint64_t ld, double global_res,
                    const dymu_cost_state* st, double* dF, void* stream);

/* Profiling: period > 0 times every period-th pass launch with HIP events
 * (start/stop taken by the dispatch itself); 0 turns it off.  Sampling keeps
 * the event overhead out of the timed region (period 1 costs ~4 us/launch). */
int dymu_set_profiling(dymu_ctx* ctx, int period);

/* Per-pass statistics of kernel 5 (diagnostics; off by default, costs a few
 * atomics per workgroup per pass when on): enable, then after a solve read one
 * record of DYMU_PASS_STAT_WORDS words per pass (the first min(launches, 16384)
 * passes; *n = their number):
 *   [0] listed entries   [1] tiles relaxed    [2] colour-deferred entries
 *   [3] key-deferred entries (tile loaded, key above the pass threshold)
 *   [4] visits stopped by the sweep cap   [5] ... by the pass deadline
 *   [6] largest / [9] smallest Manhattan tile distance from the goal's tile relaxed
 *   [7] in-tile sweeps   [8] threshold bin   [10] entries appended to the next list */
#define DYMU_PASS_STAT_WORDS 12
int dymu_set_pass_stats(dymu_ctx* ctx, int enable);
int dymu_last_pass_stats(dymu_ctx* ctx, uint32_t* out, uint64_t cap_passes, uint64_t* n);

/* Summed kernel time (ms, HIP events on the launch stream) of the most recent
 * solve's SAMPLED pass launches and their count: the mean launch duration is
 * pass_ms_total / n_pass_launches -- the bench's roofline source. */
int dymu_last_pass_timing(dymu_ctx* ctx, double* pass_ms_total, uint64_t* n_pass_launches);

/* The context's own stream (the hipStream_t that NULL `stream` arguments mean). */
void* dymu_get_stream(dymu_ctx* ctx);

const char* dymu_strerror(int status);
const char* dymu_last_error(dymu_ctx* ctx); /* last HIP/RCCL error text */
int dymu_abi_version(void);
int dymu_device_count(void);

#ifdef __cplusplus
}
#endif
#endif
