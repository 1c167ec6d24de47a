/*
 * dymu_planner.h -- flat C-ABI over PathPlanning_lib::DyMuPathPlanner
 * (include/DyMu.hpp) for non-C++ callers (ctypes, cgo, JNI).
 *
 * Each entry point forwards to the class method of the same name, which in
 * turn follows the reference method cited in DyMu.hpp.  Boolean methods
 * return 1 (true) / 0 (false); a negative value is a dymu_status error (for
 * example DYMU_ERR_NO_DEVICE when the HIP engine cannot run).  Grids are
 * row-major ny*nx doubles, index j*nx + i.  Waypoints are (x, y, z, heading).
 */
#ifndef DYMU_PLANNER_H
#define DYMU_PLANNER_H

#include <stdint.h>

#include "dymu_fim.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dymu_planner dymu_planner;

/* DyMuPathPlanner(risk_distance, reconnect_distance, risk_ratio, approach)
 * (reference src/DyMu_GlobalPathPlanning.cpp:22-33); approach 0 CONSERVATIVE, 1 SWEEPING */
int dymu_planner_create(dymu_planner** out, double risk_distance, double reconnect_distance,
                        double risk_ratio, int approach);
void dymu_planner_destroy(dymu_planner* p);
int dymu_planner_set_engine_options(dymu_planner* p, const dymu_opts* opts);

/* initGlobalLayer (:39-104) */
int dymu_planner_init_global_layer(dymu_planner* p, double globalres, double localres,
                                   uint32_t nx, uint32_t ny, double offx, double offy);
/* setCostMap (:109-126); cost_map: ny*nx */
int dymu_planner_set_cost_map(dymu_planner* p, const double* cost_map, uint32_t nx, uint32_t ny);
/* computeCostMap (:145-181); loc_modes: n_locs C strings */
int dymu_planner_compute_cost_map(dymu_planner* p, const double* lut, int lut_len,
                                  const double* slopes, int n_slopes, const char* const* loc_modes,
                                  int n_locs, const double* elevation, const double* terrain);
/* setGoal (:322-357) */
int dymu_planner_set_goal(dymu_planner* p, double x, double y, double z, double heading);
/* computeTotalCostMap (:364-408) */
int dymu_planner_compute_total_cost_map(dymu_planner* p, double x, double y, double z,
                                        double heading);
/* computeEntireTotalCostMap (:443-468) */
int dymu_planner_compute_entire_total_cost_map(dymu_planner* p);

/* getTotalCostMatrix (:799-811, +inf -> -1), getGlobalCostMatrix (:815-829),
 * getHazardDensityMatrix (:833-842), getTrafficabilityMatrix (:846-855) */
int dymu_planner_get_total_cost_matrix(dymu_planner* p, double* out);
int dymu_planner_get_global_cost_matrix(dymu_planner* p, double* out);
int dymu_planner_get_hazard_density_matrix(dymu_planner* p, double* out);
int dymu_planner_get_trafficability_matrix(dymu_planner* p, double* out);
/* raw total cost (+inf unreachable), ny*nx */
int dymu_planner_get_total_cost_raw(dymu_planner* p, double* out);
/* getTotalCost(Waypoint) (:860-890) */
int dymu_planner_get_total_cost(dymu_planner* p, double x, double y, double z, double heading,
                                double* out);
/* getPath (:589-611): writes up to max_wp waypoints (x,y,z,heading); returns
 * the number of waypoints (>= 0) or a negative status */
int dymu_planner_get_path(dymu_planner* p, double x, double y, double z, double heading,
                          double* out_xyzh, int max_wp);
/* getPaths (extension, DyMu.hpp): the global path of each of n starts (starts_xyzh: n x
 * (x, y, z, heading)) on the current total-cost map -- on the GPU next to the map while
 * the device copy is current, else by the host descent per start.  No evaluatePath, and
 * current_path is not touched.  counts[q] (may be NULL) = waypoints of path q, at most
 * max_wp; status[q] (may be NULL) = 1 sink appended, 0 stalled ("ERROR in trajectory",
 * the waypoints so far kept), -1 first step NaN / start off the grid (empty), -3 more
 * than max_wp waypoints (the first max_wp kept).  stride >= 1 keeps waypoints 0, stride,
 * 2 stride, ... and the sink.  out_xyzh receives the paths PACKED one after another
 * (sum of counts waypoints; n * max_wp in the worst case).  As the sizes are not known
 * before the call, out_xyzh may be NULL: the result is then kept in the handle, and a
 * second call with starts_xyzh = NULL and the same n copies it into out_xyzh (sized
 * from the first call's counts) and drops it.  Returns n or a negative status. */
int dymu_planner_get_paths(dymu_planner* p, const double* starts_xyzh, int n, int max_wp,
                           int stride, double* out_xyzh, int* counts, int* status);
/* ---- goal sets (DyMuPathPlanner::setGoals) ----
 * n goals (x, y, z, heading each) with offsets (n costs >= 0, finite) or NULL for none;
 * each goal validated as dymu_planner_set_goal validates its one.  1 = set, 0 = rejected
 * (nothing changed).  dymu_planner_set_goal clears the set. */
int dymu_planner_set_goals(dymu_planner* p, const double* goals_xyzh, const double* offsets,
                           int n);
/* goals in force: 0 none, 1 after dymu_planner_set_goal, n after dymu_planner_set_goals */
int dymu_planner_goal_count(dymu_planner* p);
/* the nearest-goal label of every node (ny*nx, row-major; 0xFFFFFFFF = none) */
int dymu_planner_get_goal_labels(dymu_planner* p, uint32_t* out);
/* the label of the node nearest (x, y): >= 0, -1 for none (or off the grid, or a NULL
 * handle); an engine failure returns its status (<= -2) */
int dymu_planner_goal_label(dymu_planner* p, double x, double y);
/* the goal each path of the last dymu_planner_get_paths ended on (-1: status != 1);
 * n = that call's n.  Returns n or a negative status. */
int dymu_planner_last_path_sinks(dymu_planner* p, int* out, int n);
/* 1 if the last dymu_planner_get_paths ran on the device, 0 on the host threads */
int dymu_planner_last_paths_on_device(dymu_planner* p);
/* its kernel time (HIP events, ms; 0 on the host route) */
int dymu_planner_last_paths_kernel_ms(dymu_planner* p, double* ms);
/* ---- batched total-cost maps (DyMuPathPlanner::computeTotalCostMaps) ----
 * One map per goal (n x (x, y, z, heading)) on the current speed, solved together and
 * kept on the device, next to -- not instead of -- the single goal's map.  1 = solved,
 * 0 = rejected (a goal dymu_planner_set_goal would reject, or no device engine: nothing
 * changed). */
int dymu_planner_compute_total_cost_maps(dymu_planner* p, const double* goals_xyzh, int n);
/* maps in the batch (0: none, or dropped by a speed change / a new grid) */
int dymu_planner_batch_count(dymu_planner* p);
/* map b (ny*nx, row-major): raw != 0 +inf for unreachable cells, else -1.  1 = copied,
 * 0 = no such map. */
int dymu_planner_copy_batch_total_cost(dymu_planner* p, uint32_t b, double* out, int raw);
/* out[b * n + m] = dymu_planner_get_total_cost of point m (n x (x, y)) on map b, for
 * every map of the batch (out: batch_count * n doubles).  1 = written, 0 = no batch. */
int dymu_planner_get_total_costs(dymu_planner* p, const double* points_xy, int n, double* out);
/* both of the above in one call: out (n_goals * n_targets) = the traverse-cost matrix */
int dymu_planner_cost_matrix(dymu_planner* p, const double* goals_xyzh, int n_goals,
                             const double* targets_xy, int n_targets, double* out);
/* DyMuPathPlanner::costMatrixUntil: dymu_planner_cost_matrix whose batch
 * solve stops once the cells the targets read are final in every map -- the same matrix
 * for less work when the targets lie near the goals.  It leaves a TRUNCATED batch:
 * dymu_planner_batch_level is finite, and the batch readers (get_total_costs,
 * copy_batch_total_cost, get_paths_to) and compute_total_cost_maps of the same goals
 * first complete it with the cold solve.  0 (nothing changed) also without a device
 * engine or with an engine that lacks the entry. */
int dymu_planner_cost_matrix_until(dymu_planner* p, const double* goals_xyzh, int n_goals,
                                   const double* targets_xy, int n_targets, double* out);
/* batchLevel(): the level up to which the held batch's maps are final; +inf for a
 * complete batch and with no batch */
int dymu_planner_batch_level(dymu_planner* p, double* level);
/* dymu_planner_get_paths on map b with goal b as the sink: same arguments, same
 * two-call protocol, same status values.  DYMU_ERR_ARG for b >= batch_count. */
int dymu_planner_get_paths_to(dymu_planner* p, uint32_t b, const double* starts_xyzh, int n,
                              int max_wp, int stride, double* out_xyzh, int* counts, int* status);
/* getPathStats (extension, DyMu.hpp): out[q] = the dymu_path_stat record
 * (include/dymu_fim.h) of the path dymu_planner_get_paths would return for start q, with
 * no waypoint stored or moved.  Field slot 0 is the speed map the solve used, slot 1 the
 * optional row-major ny x nx `field` (NULL: none).  The route is get_paths' unless host is
 * non-zero, which runs the host descent; dymu_planner_last_paths_on_device / _kernel_ms
 * report the call.  Returns n or a negative status (DYMU_ERR_ARG for max_wp <= 0). */
int dymu_planner_get_path_stats(dymu_planner* p, const double* starts_xyzh, int n, int max_wp,
                                const double* field, int host, dymu_path_stat* out);
/* ... on map b of the batch with goal b as the sink (always on the device).
 * DYMU_ERR_ARG for b >= batch_count. */
int dymu_planner_get_path_stats_to(dymu_planner* p, uint32_t b, const double* starts_xyzh, int n,
                                   int max_wp, const double* field, dymu_path_stat* out);
/* getArrivingPaths (extension, DyMu.hpp): dymu_planner_get_paths with the
 * arriving descent -- paths that pass obstacles and end on the goal's node (the rule is
 * stated with dymu_arrive_stat in include/dymu_fim.h).  Same arguments, same two-call
 * protocol, same status values (-1: the start's node is off the grid, an obstacle or
 * without a label); stats (may be NULL; first call only) receives n records.
 * dymu_planner_last_path_sinks / _last_paths_on_device / _kernel_ms report the call. */
int dymu_planner_get_arriving_paths(dymu_planner* p, const double* starts_xyzh, int n, int max_wp,
                                    int stride, double* out_xyzh, int* counts, int* status,
                                    dymu_arrive_stat* stats);
/* ... on map b of the batch with goal b as the sink (always on the device).
 * DYMU_ERR_ARG for b >= batch_count. */
int dymu_planner_get_arriving_paths_to(dymu_planner* p, uint32_t b, const double* starts_xyzh,
                                       int n, int max_wp, int stride, double* out_xyzh,
                                       int* counts, int* status, dymu_arrive_stat* stats);
/* getArrivingStats: out[q] = the record of start q, no waypoint stored or moved.  The route
 * is get_paths' unless host is non-zero.  Returns n or a negative status. */
int dymu_planner_get_arriving_stats(dymu_planner* p, const double* starts_xyzh, int n, int max_wp,
                                    int host, dymu_arrive_stat* out);
int dymu_planner_get_arriving_stats_to(dymu_planner* p, uint32_t b, const double* starts_xyzh,
                                       int n, int max_wp, dymu_arrive_stat* out);
/* getSimplifiedPaths (extension, DyMu.hpp): the arriving paths thinned
 * while the descent runs -- every dropped waypoint lies within eps (map units) of the
 * segment between the kept waypoints on either side of it (the rule and its one-sided
 * guarantee are stated with dymu_arrive_simplified_device in include/dymu_fim.h).  max_wp
 * bounds the walk as in dymu_planner_get_arriving_stats.  The two-call protocol of
 * dymu_planner_get_arriving_paths: with starts the call computes, fills counts / status /
 * stats (each may be NULL) and keeps the result; with starts NULL (n as before) it copies
 * the held result out and releases it -- out_xyzh packed path after path, and index (may
 * be NULL) packed the same way: each waypoint's number in the path
 * dymu_planner_get_arriving_paths(stride 1) returns, of which it is the exact copy.  A
 * first call with out_xyzh does both.  DYMU_ERR_ARG for eps not finite or <= 0 and for
 * max_wp <= 0.  dymu_planner_last_path_sinks / _last_paths_on_device / _kernel_ms report
 * the call. */
int dymu_planner_get_simplified_paths(dymu_planner* p, const double* starts_xyzh, int n,
                                      double eps, int max_wp, double* out_xyzh, uint32_t* index,
                                      int* counts, int* status, dymu_arrive_stat* stats);
/* ... on map b of the batch with goal b as the sink (always on the device).
 * DYMU_ERR_ARG for b >= batch_count. */
int dymu_planner_get_simplified_paths_to(dymu_planner* p, uint32_t b, const double* starts_xyzh,
                                         int n, double eps, int max_wp, double* out_xyzh,
                                         uint32_t* index, int* counts, int* status,
                                         dymu_arrive_stat* stats);
/* the last dymu_planner_get_simplified_paths[_to]: the paths that ran a second time on the
 * device because they kept more waypoints than the first slot capacity (0 on the host
 * route), and the bytes it downloaded (either may be NULL) */
int dymu_planner_last_simplified(dymu_planner* p, uint64_t* reruns, uint64_t* bytes);
/* getRouteFields (extension, DyMu.hpp): every cell's node route to the
 * goal at once, as include/dymu_fim.h defines it with dymu_route_out.  fields: n_fields <=
 * DYMU_PATH_FIELDS row-major ny x nx arrays, a NULL entry being the speed map the solve
 * used.  out: HOST maps of nx * ny elements (out->ld is ignored: the pitch is nx); a NULL
 * map is not computed, an integral / vmin / vmax beyond n_fields must be NULL.  The route
 * is get_paths' unless host is non-zero; dymu_planner_last_paths_on_device / _kernel_ms
 * report the call.  *rounds (may be NULL) = doubling rounds on the device, 0 on the host.
 * Returns DYMU_OK or a negative status. */
int dymu_planner_get_route_fields(dymu_planner* p, const double* const* fields, int n_fields,
                                  int host, const dymu_route_out* out, uint32_t* rounds);
/* ... on map b of the batch with goal b as the root (always on the device).  DYMU_ERR_ARG
 * for b >= batch_count. */
int dymu_planner_get_route_fields_to(dymu_planner* p, uint32_t b, const double* const* fields,
                                     int n_fields, const dymu_route_out* out, uint32_t* rounds);
/* getRouteUsage (extension, DyMu.hpp): how much of the map drains through
 * every cell, as include/dymu_fim.h defines it with dymu_usage_out.  weights: a row-major
 * ny x nx uint32 array, or NULL for 1 a cell.  out: HOST maps of nx * ny elements (out->ld
 * is ignored: the pitch is nx); a NULL map is not computed.  catchment: n_catchment HOST
 * entries, one per goal (dymu_planner_goal_count; entries beyond the goals are set to 0),
 * or NULL.  DYMU_ERR_ARG if nothing is asked for, or if n_catchment is below the number of
 * goals.  The route is get_paths' unless host is non-zero;
 * dymu_planner_last_paths_on_device / _kernel_ms report the call.  *rounds (may be NULL) =
 * doubling rounds on the device, 0 on the host.  Returns DYMU_OK or a negative status. */
int dymu_planner_get_route_usage(dymu_planner* p, const uint32_t* weights, int host,
                                 const dymu_usage_out* out, uint64_t* catchment,
                                 uint32_t n_catchment, uint32_t* rounds);
/* ... on map b of the batch with goal b as the root (always on the device; one catchment
 * entry).  DYMU_ERR_ARG for b >= batch_count. */
int dymu_planner_get_route_usage_to(dymu_planner* p, uint32_t b, const uint32_t* weights,
                                    const dymu_usage_out* out, uint64_t* catchment,
                                    uint32_t n_catchment, uint32_t* rounds);
/* goalI() / goalJ(): the single goal's cell (goal 0 of a goal set); 1 = written, 0 = no
 * goal set yet */
int dymu_planner_goal_cell(dymu_planner* p, uint32_t* i, uint32_t* j);
/* statistics of the last batch solve (those of the stacked domain) */
int dymu_planner_last_batch_stats(dymu_planner* p, dymu_stats* out);
/* DyMuPathPlanner::trackSpeedChanges (off by default): with it on a
 * synchronised speed change keeps the batch and the goal set's map, and the next
 * compute_total_cost_maps of the same goals / compute_entire_total_cost_map under the
 * same goal set re-propagates them from the changed box instead of solving cold. */
int dymu_planner_track_speed_changes(dymu_planner* p, int on);
/* lastBatchSolveKind(): 0 cold solve, 1 windowed re-propagation, 2 batch reused */
int dymu_planner_last_batch_solve_kind(dymu_planner* p);
/* ---- combining the maps of the batch (DyMuPathPlanner::combineTotalCostMaps, DESIGN.md
 * s5.14; the fold, its order and its tie rules: dymu_batch_reduce_device) ----
 * op (dymu_reduce_op) over the listed maps -- planes: n_planes indices, NULL: all maps in
 * order -- with optional weights and offsets, one per listed map (per map of the batch
 * without a list), or NULL.  The combined map and the MAX / MIN plane map stay on the
 * device; summary (may be NULL) describes the combined map.  1 = combined, 0 = refused
 * (no batch, no device engine, a bad list: nothing changed). */
int dymu_planner_combine_total_cost_maps(dymu_planner* p, int op, const uint32_t* planes,
                                         uint32_t n_planes, const double* weights,
                                         const double* offsets, dymu_reduce_summary* summary);
/* the combined map (ny*nx doubles; raw != 0: +inf, else -1) and the plane map of the last
 * MAX / MIN (ny*nx words).  1 = copied, 0 = none that belongs to the held batch: it ends
 * with the batch and with every solve or refresh that rewrites the stack. */
int dymu_planner_copy_combined_total_cost(dymu_planner* p, double* out, int raw);
int dymu_planner_copy_combined_planes(dymu_planner* p, uint32_t* out);
/* viaCorridor: mask (ny*nx bytes) = 1 where T_a + T_b <= bound = D_min * (1 + slack), D_min
 * the minimum of that sum; info as DyMuPathPlanner::CorridorInfo.  1 = written, 0 = refused
 * (a or b >= batch_count, slack negative or not finite, no finite cell: nothing written). */
typedef struct dymu_corridor_info {
  double d_min;
  uint32_t min_i, min_j;
  uint64_t count;
  uint32_t i0, j0, i1, j1;
  double bound;
} dymu_corridor_info;
int dymu_planner_via_corridor(dymu_planner* p, uint32_t a, uint32_t b, double slack, uint8_t* mask,
                              dymu_corridor_info* info);
/* rendezvous: the cell minimising the MAX (minimax != 0) or the SUM of the listed maps
 * (lists as for combine) and that value.  1 = written, 0 = refused or no finite cell. */
int dymu_planner_rendezvous(dymu_planner* p, const uint32_t* planes, uint32_t n_planes,
                            const double* weights, const double* offsets, int minimax, uint32_t* i,
                            uint32_t* j, double* value);
/* kernel time (HIP events, ms) of the last combine; 0 before the first */
int dymu_planner_last_combine_kernel_ms(dymu_planner* p, double* ms);
/* getLocomotionMode (:788-795) into buf (NUL-terminated) */
int dymu_planner_get_locomotion_mode(dymu_planner* p, double x, double y, double z, double heading,
                                     char* buf, int buflen);
/* dynamic feedback (extension): hazard_density / trafficability, ny*nx */
int dymu_planner_set_hazard_density(dymu_planner* p, const double* hd);
int dymu_planner_set_trafficability(dymu_planner* p, const double* tr);
/* windowed forms: w*h values (row-major) for cells [i0, i0+w) x [j0, j0+h) */
int dymu_planner_set_hazard_density_window(dymu_planner* p, uint32_t i0, uint32_t j0, uint32_t w,
                                           uint32_t h, const double* hd);
int dymu_planner_set_trafficability_window(dymu_planner* p, uint32_t i0, uint32_t j0, uint32_t w,
                                           uint32_t h, const double* tr);
/* setCostMapWindow: setCostMap's per-cell rule for the cells [i0, i0+w) x [j0, j0+h) only
 * (w*h costs, row-major).  1 = set; 0 = rejected, nothing changed (a box not inside the
 * grid); DYMU_ERR_ARG for a null pointer.  Only the box's rows are re-packed at the next
 * solve; with the global risk on, added obstacles update R incrementally, and freed ones
 * too once dymu_planner_track_obstacle_removal is on (else by the whole clearance solve). */
int dymu_planner_set_cost_map_window(dymu_planner* p, uint32_t i0, uint32_t j0, uint32_t w,
                                     uint32_t h, const double* cost);
/* trackObstacleRemoval(on != 0): off by default.  On: an obstacle that a later
 * dymu_planner_set_cost_map_window frees joins the pending box of the incremental update
 * (dymu_clearance_edit_device) instead of sending R through the whole clearance solve,
 * provided the global risk is on, R is current and the engine has the entry.  DYMU_OK;
 * DYMU_ERR_ARG for a null handle. */
int dymu_planner_track_obstacle_removal(dymu_planner* p, int on);
/* DyMuPathPlanner::setGlobalRisk (off by default): the obstacle clearance
 * of the global map as one more factor of the speed, F * (risk_ratio * R + 1) with
 * R = max(1 - distance to the nearest obstacle / risk_distance, 0).  Either argument 0
 * switches it off.  1 = set; 0 = rejected, nothing changed (a negative, NaN or infinite
 * argument; a non-zero setting without a device engine). */
int dymu_planner_set_global_risk(dymu_planner* p, double risk_distance, double risk_ratio);
/* getGlobalRiskMatrix(): R, ny*nx (recomputed first when stale; zeros while off) */
int dymu_planner_get_global_risk(dymu_planner* p, double* out);
/* lastRiskUpdateKind(): how R was last brought up to date: 0 not yet, 1 the whole clearance
 * solve, 2 the incremental update after setCostMapWindow added obstacles, 3 the incremental
 * update after it freed some (dymu_planner_track_obstacle_removal) */
int dymu_planner_last_risk_update_kind(dymu_planner* p);
/* ... the engine's statistics of that clearance solve or update (either may be NULL) and the
 * box {i0, j0, w, h} of R it rewrote: the whole grid, or the box the update reported */
int dymu_planner_last_risk_update(dymu_planner* p, dymu_stats* out, uint32_t box[4]);
/* ... and, after an update of kind 3, the raise's figures as dymu_last_update_stats gives
 * them: {raise passes, raise tile visits, cells invalidated, 0}; zeros after any other kind */
int dymu_planner_last_risk_raise(dymu_planner* p, uint64_t out[4]);
/* narrow-band cells left by the last computeTotalCostMap's early exit (0 after
 * computeEntireTotalCostMap) */
int64_t dymu_planner_last_band_size(dymu_planner* p);
/* statistics of the last solve */
int dymu_planner_last_stats(dymu_planner* p, dymu_stats* out);
/* the last computeTotalCostMap's exit-order resolution: out[0] cells
 * of exactly the exit value, out[1] how many of them the reference had not closed,
 * out[2] 1 if the exact host replay ran (degenerate ties only), out[3] host ms,
 * out[4] reference updates the band replay evaluated, out[5] 1 if every band value
 * is the reference's (0: the replay hit its work bound) */
int dymu_planner_last_early_exit(dymu_planner* p, double out[6]);
/* the same, n values of: tied, open_at_limit, exact_replay, resolve_ms, replay_updates,
 * band_exact, near_ties (comparisons of engine values rounding could flip: any sends
 * the exit to the exact host replay), replay_threads (round 6) */
int dymu_planner_last_early_exit_ex(dymu_planner* p, double* out, uint32_t n);
/* how the last solve ran: 0 cold, 1 windowed re-propagation from the window
 * where the speed changed (dymu_resolve_window), 2 previous map reused */
int dymu_planner_last_solve_kind(dymu_planner* p);

/* ---- node-level access (src/DyMu.hpp:500-518, extension of the flat ABI) ---- */
typedef struct dymu_global_node {
  double elevation, slope, raw_cost, cost, hazard_density, trafficability, total_cost;
  uint32_t terrain;
  int32_t state;        /* 0 OPEN, 1 CLOSED */
  int32_t is_obstacle;
  int32_t has_local_map;
} dymu_global_node;
/* getGlobalNode (:313-317): 1 and *out, or 0 (NULL) */
int dymu_planner_get_global_node(dymu_planner* p, uint32_t i, uint32_t j, dymu_global_node* out);
int dymu_planner_is_safe_node(dymu_planner* p, uint32_t i, uint32_t j);          /* :410-422 */
int dymu_planner_is_fully_closed_node(dymu_planner* p, uint32_t i, uint32_t j);  /* :424-436 */
int dymu_planner_reset_total_cost_map(dymu_planner* p);                          /* :473-485 */
/* every node's state in bulk (ny*nx bytes, row-major: 1 CLOSED, 0 OPEN), as
 * dymu_planner_get_global_node reports it one node at a time */
int dymu_planner_get_node_states(dymu_planner* p, uint8_t* out);
/* global_narrowband (:445) as the last computeTotalCostMap left it: the band
 * size; up to max (i, j) pairs written to ij in the reference's insertion order */
int64_t dymu_planner_global_narrowband(dymu_planner* p, uint32_t* ij, int64_t max);
/* minCostGlobalNode (:548-567): 1, the band node of lowest total cost (removed
 * from the band list) in ij[2] and *total_cost; 0 on an empty band */
int dymu_planner_min_cost_global_node(dymu_planner* p, uint32_t* ij, double* total_cost);
int dymu_planner_reset_global_narrow_band(dymu_planner* p);                      /* :487-498 */
/* gradientNode (:718-772): the normalised descent direction at (i, j) in d[2] */
int dymu_planner_gradient_node(dymu_planner* p, uint32_t i, uint32_t j, double* d);
/* propagateGlobalNode (:500-546): the reference update of node (i, j) from its
 * nb4's current total costs on the host copy of the map; a node whose total cost
 * was +inf joins the band (appended) and global_propagated_nodes */
int dymu_planner_propagate_global_node(dymu_planner* p, uint32_t i, uint32_t j);
/* the public globalNode::state (0 OPEN, 1 CLOSED) written by a caller */
int dymu_planner_set_global_node_state(dymu_planner* p, uint32_t i, uint32_t j, int state);
/* global_propagated_nodes (:447): the count (max <= 0: cheap); up to max (i, j) pairs in
 * ij, in the reference's insertion order (DyMuPathPlanner::globalPropagatedIndices) --
 * rebuilt from the values, or from the exact host replay of the reference's FMM where
 * near ties leave it open (from ~2^22 reached nodes: ~34 s for the whole list at 16384^2) */
int64_t dymu_planner_global_propagated_nodes(dymu_planner* p, uint32_t* ij, int64_t max);
/* install a total-cost map (ny*nx, +inf unreachable) as a converged
 * computeEntireTotalCostMap leaves it (every finite node CLOSED) */
int dymu_planner_load_total_cost_map(dymu_planner* p, const double* T);
/* current_path (public member, src/DyMu.hpp:456): n waypoints (x, y, z, heading) */
int dymu_planner_set_current_path(dymu_planner* p, const double* xyzh, int n);
int dymu_planner_get_current_path(dymu_planner* p, double* out_xyzh, int max_wp);

/* ---- local layer (src/DyMu_LocalPathRepairing.cpp) ---- */
/* computeLocalPlanning (:193-291).  image: height rows of row_size bytes, pixel
 * (i, j) at image[j*row_size + i*pixel_size], nonzero = obstacle.  Returns 1
 * when the path was repaired (trajectory = current_path, *n_traj waypoints, at
 * most max_traj written; *local_time_s = repair time), 0 when not blocked. */
int dymu_planner_compute_local_planning(dymu_planner* p, double x, double y, double z,
                                        double heading, const uint8_t* image, uint32_t width,
                                        uint32_t height, uint32_t row_size, uint32_t pixel_size,
                                        double res, double* traj_xyzh, int max_traj,
                                        int* n_traj, double* local_time_s);
/* repairPath (:298-435): the reconnecting index or -1 */
int dymu_planner_repair_path(dymu_planner* p, double x, double y, double z, double heading,
                             uint32_t index);
/* evaluatePath (:1027-1109) */
int dymu_planner_evaluate_path(dymu_planner* p, uint32_t starting_index);
/* expandRisk (:493-523) */
int dymu_planner_expand_risk(dymu_planner* p);
/* computeLocalPropagation (:578-698): 1 and the set node's global pose, or 0 (NULL) */
int dymu_planner_compute_local_propagation(dymu_planner* p, const double* start_xyzh,
                                           const double* overtake_xyzh, double* set_xy);
/* computeLocalWaypointDijkstra (L:851-869) from the sub-cell at waypoint xyzh
 * (getLocalNode: subdivides): 1 and the step's (x, y, z, heading), 0 (NULL) */
int dymu_planner_local_waypoint_dijkstra(dymu_planner* p, const double* xyzh, double* out_xyzh);
/* local_agent (src/DyMu.hpp:460): 1 and its global pose (x, y), or 0 (NULL) */
int dymu_planner_local_agent(dymu_planner* p, double* global_xy);
/* computeLocalPropagation's wall-clock limit (the reference's 5 s, :685-696;
 * <= 0 disables it); it then returns 0 (NULL) like the reference */
int dymu_planner_set_local_timeout(dymu_planner* p, double seconds);
/* getRiskMatrix / getDeviationMatrix (:1111-1211): (21*r)^2 doubles, r = res ratio */
int dymu_planner_get_risk_matrix(dymu_planner* p, double x, double y, double z, double heading,
                                 double* out);
int dymu_planner_get_deviation_matrix(dymu_planner* p, double x, double y, double z,
                                      double heading, double* out);
int dymu_planner_get_reconnecting_index(dymu_planner* p);
int dymu_planner_res_ratio(dymu_planner* p);
/* subdivided global nodes: count, and a ny*nx byte mask (may be NULL) */
int64_t dymu_planner_local_map_mask(dymu_planner* p, uint8_t* mask);
/* a local-layer sub-cell (the reference's localNode, src/DyMu.hpp:42-67); id names
 * it for the calls below (stable while the local map lives) */
typedef struct dymu_local_node {
  double global_x, global_y;  /* global_pose (global units) */
  double deviation, total_cost, risk;
  uint32_t parent_i, parent_j; /* the subdivided global node */
  uint32_t li, lj;             /* the sub-cell inside it */
  int32_t state, is_obstacle;  /* 0 OPEN / 1 CLOSED; 0 / 1 */
  uint64_t id;
} dymu_local_node;
/* getLocalNode(Waypoint) (L:177-189; subdivides): 1 and *out, or 0 (NULL) */
int dymu_planner_get_local_node(dymu_planner* p, double x, double y, dymu_local_node* out);
/* localNode::nb4List[d] of sub-cell id (d: 0 (i,j-1), 1 (i-1,j), 2 (i+1,j),
 * 3 (i,j+1)): 1 and *out, or 0 (NULL) */
int dymu_planner_local_neighbour(dymu_planner* p, uint64_t id, int d, dymu_local_node* out);
/* maxRiskNode (L:525-548): 1 and the popped node, or 0 (empty queue: NULL) */
int dymu_planner_max_risk_node(dymu_planner* p, dymu_local_node* out);
/* propagateRisk (L:550-576) / propagateLocalNode (L:700-750) on sub-cell id */
int dymu_planner_propagate_risk(dymu_planner* p, uint64_t id);
int dymu_planner_propagate_local_node(dymu_planner* p, uint64_t id);
/* the public localNode::state (0 OPEN, 1 CLOSED) written by a caller */
int dymu_planner_set_local_node_state(dymu_planner* p, uint64_t id, int state);
/* minCostLocalNode(Tovertake, minC) (L:752-775) / minCostLocalNode(reachNode)
 * (L:777-805): 1 and the popped band node, or 0 (empty band) */
int dymu_planner_min_cost_local_node(dymu_planner* p, double Tovertake, double minC,
                                     dymu_local_node* out);
int dymu_planner_min_cost_local_node_reach(dymu_planner* p, uint64_t reach_id,
                                           dymu_local_node* out);
/* the public local lists (src/DyMu.hpp:448-454): which = 0 local_narrowband, 1
 * local_expandable_obstacles, 2 local_propagated_nodes; the count, up to max
 * written to out in the list's order */
int64_t dymu_planner_local_list(dymu_planner* p, int which, dymu_local_node* out, int64_t max);
/* one subdivided node's r*r sub-cells ([j][i]); 0 if (i, j) has no local map */
int dymu_planner_local_block(dymu_planner* p, uint32_t i, uint32_t j, double* dev, double* tc,
                             double* risk, uint8_t* state, uint8_t* obst);

#ifdef __cplusplus
}
#endif
#endif
