// planner_capi.cpp -- extern "C" forwarding layer (include/dymu_planner.h)
// over PathPlanning_lib::DyMuPathPlanner.  Exceptions never cross the ABI:
// an engine failure becomes DYMU_ERR_NO_DEVICE / DYMU_ERR_HIP.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <exception>
#include <functional>
#include <new>
#include <stdexcept>
#include <string>
#include <vector>

#include "DyMu.hpp"
#include "dymu_planner.h"

using PathPlanning_lib::DyMuPathPlanner;
using PathPlanning_lib::localNode;
using PathPlanning_lib::CLOSED;
using PathPlanning_lib::OPEN;

struct dymu_planner {
  DyMuPathPlanner pl;
  // the last dymu_planner_get_paths result, kept until it is copied out
  std::vector<std::vector<base::Waypoint>> paths;
  std::vector<int> paths_status;
  std::vector<int> paths_sinks;  // the goal each of those paths ended on (-1: none)
  // dymu_planner_get_simplified_paths: each kept waypoint's number in the unsimplified path
  std::vector<std::vector<uint32_t>> paths_index;
  dymu_planner(double a, double b, double c, PathPlanning_lib::repairingAproach r)
      : pl(a, b, c, r) {}
};

namespace {

base::Waypoint wp(double x, double y, double z, double h) {
  base::Waypoint w;
  w.position[0] = x;
  w.position[1] = y;
  w.position[2] = z;
  w.heading = h;
  return w;
}

int engine_error(const std::exception& e) {
  const std::string m = e.what();
  return m.find("cannot create") != std::string::npos ? DYMU_ERR_NO_DEVICE : DYMU_ERR_HIP;
}

template <class F>
int guarded(F&& f) {
  try {
    return f();
  } catch (const std::bad_alloc&) {
    return DYMU_ERR_NOMEM;
  } catch (const std::exception& e) {
    return engine_error(e);
  }
}

std::vector<std::vector<double>> to_rows(const double* a, unsigned nx, unsigned ny) {
  std::vector<std::vector<double>> m(ny, std::vector<double>(nx));
  for (unsigned j = 0; j < ny; ++j) std::memcpy(m[j].data(), a + (size_t)j * nx, sizeof(double) * nx);
  return m;
}

void from_rows(const std::vector<std::vector<double>>& m, double* out) {
  size_t off = 0;
  for (const auto& r : m) {
    std::memcpy(out + off, r.data(), sizeof(double) * r.size());
    off += r.size();
  }
}

}  // namespace

extern "C" {

int dymu_planner_create(dymu_planner** out, double risk_distance, double reconnect_distance,
                        double risk_ratio, int approach) {
  if (!out) return DYMU_ERR_ARG;
  return guarded([&] {
    *out = new dymu_planner(risk_distance, reconnect_distance, risk_ratio,
                            approach == 1 ? PathPlanning_lib::SWEEPING
                                          : PathPlanning_lib::CONSERVATIVE);
    return DYMU_OK;
  });
}

void dymu_planner_destroy(dymu_planner* p) { delete p; }

int dymu_planner_set_engine_options(dymu_planner* p, const dymu_opts* o) {
  if (!p || !o) return DYMU_ERR_ARG;
  p->pl.setEngineOptions(*o);
  return DYMU_OK;
}

int dymu_planner_init_global_layer(dymu_planner* p, double globalres, double localres,
                                   uint32_t nx, uint32_t ny, double offx, double offy) {
  if (!p || nx == 0 || ny == 0) return DYMU_ERR_ARG;
  return guarded([&] { return (int)p->pl.initGlobalLayer(globalres, localres, nx, ny, {offx, offy}); });
}

int dymu_planner_set_cost_map(dymu_planner* p, const double* cost_map, uint32_t nx, uint32_t ny) {
  if (!p || !cost_map) return DYMU_ERR_ARG;
  return guarded([&] { return (int)p->pl.setCostMap(to_rows(cost_map, nx, ny)); });
}

int dymu_planner_compute_cost_map(dymu_planner* p, const double* lut, int lut_len,
                                  const double* slopes, int n_slopes, const char* const* loc_modes,
                                  int n_locs, const double* elevation, const double* terrain) {
  if (!p || !lut || !slopes || !loc_modes || !elevation || !terrain || lut_len <= 0 ||
      n_slopes <= 0 || n_locs <= 0)
    return DYMU_ERR_ARG;
  return guarded([&] {
    std::vector<std::string> modes;
    for (int k = 0; k < n_locs; ++k) modes.emplace_back(loc_modes[k] ? loc_modes[k] : "");
    return (int)p->pl.computeCostMap(std::vector<double>(lut, lut + lut_len),
                                     std::vector<double>(slopes, slopes + n_slopes), modes,
                                     elevation, terrain);
  });
}

int dymu_planner_set_goal(dymu_planner* p, double x, double y, double z, double h) {
  if (!p) return DYMU_ERR_ARG;
  return guarded([&] { return (int)p->pl.setGoal(wp(x, y, z, h)); });
}

int dymu_planner_compute_total_cost_map(dymu_planner* p, double x, double y, double z, double h) {
  if (!p) return DYMU_ERR_ARG;
  return guarded([&] { return (int)p->pl.computeTotalCostMap(wp(x, y, z, h)); });
}

int dymu_planner_compute_entire_total_cost_map(dymu_planner* p) {
  if (!p) return DYMU_ERR_ARG;
  return guarded([&] { return (int)p->pl.computeEntireTotalCostMap(); });
}

int dymu_planner_get_total_cost_matrix(dymu_planner* p, double* out) {
  if (!p || !out) return DYMU_ERR_ARG;
  return guarded([&] { p->pl.copyTotalCost(out, false); return DYMU_OK; });
}

int dymu_planner_get_global_cost_matrix(dymu_planner* p, double* out) {
  if (!p || !out) return DYMU_ERR_ARG;
  return guarded([&] { from_rows(p->pl.getGlobalCostMatrix(), out); return DYMU_OK; });
}

int dymu_planner_get_hazard_density_matrix(dymu_planner* p, double* out) {
  if (!p || !out) return DYMU_ERR_ARG;
  return guarded([&] { from_rows(p->pl.getHazardDensityMatrix(), out); return DYMU_OK; });
}

int dymu_planner_get_trafficability_matrix(dymu_planner* p, double* out) {
  if (!p || !out) return DYMU_ERR_ARG;
  return guarded([&] { from_rows(p->pl.getTrafficabilityMatrix(), out); return DYMU_OK; });
}

int dymu_planner_get_total_cost_raw(dymu_planner* p, double* out) {
  if (!p || !out) return DYMU_ERR_ARG;
  return guarded([&] { p->pl.copyTotalCost(out, true); return DYMU_OK; });
}

int dymu_planner_get_total_cost(dymu_planner* p, double x, double y, double z, double h,
                                double* out) {
  if (!p || !out) return DYMU_ERR_ARG;
  return guarded([&] { *out = p->pl.getTotalCost(wp(x, y, z, h)); return DYMU_OK; });
}

int dymu_planner_get_path(dymu_planner* p, double x, double y, double z, double h,
                          double* out, int max_wp) {
  if (!p || !out || max_wp < 0) return DYMU_ERR_ARG;
  return guarded([&] {
    const std::vector<base::Waypoint> path = p->pl.getPath(wp(x, y, z, h));
    const int n = (int)path.size();
    for (int k = 0; k < n && k < max_wp; ++k) {
      out[4 * k + 0] = path[k].position[0];
      out[4 * k + 1] = path[k].position[1];
      out[4 * k + 2] = path[k].position[2];
      out[4 * k + 3] = path[k].heading;
    }
    return n;
  });
}

int dymu_planner_get_locomotion_mode(dymu_planner* p, double x, double y, double z, double h,
                                     char* buf, int buflen) {
  if (!p || !buf || buflen <= 0) return DYMU_ERR_ARG;
  return guarded([&] {
    const std::string m = p->pl.getLocomotionMode(wp(x, y, z, h));
    std::strncpy(buf, m.c_str(), (size_t)buflen - 1);
    buf[buflen - 1] = '\0';
    return (int)m.size();
  });
}

int dymu_planner_set_hazard_density(dymu_planner* p, const double* hd) {
  if (!p || !hd) return DYMU_ERR_ARG;
  const size_t n = (size_t)p->pl.sizeX() * p->pl.sizeY();
  return guarded([&] { return (int)p->pl.setHazardDensity(std::vector<double>(hd, hd + n)); });
}

int dymu_planner_set_trafficability(dymu_planner* p, const double* tr) {
  if (!p || !tr) return DYMU_ERR_ARG;
  const size_t n = (size_t)p->pl.sizeX() * p->pl.sizeY();
  return guarded([&] { return (int)p->pl.setTrafficability(std::vector<double>(tr, tr + n)); });
}

int dymu_planner_set_global_risk(dymu_planner* p, double risk_distance, double risk_ratio) {
  if (!p) return DYMU_ERR_ARG;
  return guarded([&] { return (int)p->pl.setGlobalRisk(risk_distance, risk_ratio); });
}

int dymu_planner_get_global_risk(dymu_planner* p, double* out) {
  if (!p || !out) return DYMU_ERR_ARG;
  return guarded([&] { from_rows(p->pl.getGlobalRiskMatrix(), out); return DYMU_OK; });
}

int dymu_planner_last_stats(dymu_planner* p, dymu_stats* out) {
  if (!p || !out) return DYMU_ERR_ARG;
  *out = p->pl.lastStats();
  return DYMU_OK;
}

int dymu_planner_last_early_exit(dymu_planner* p, double out[6]) {
  if (!p || !out) return DYMU_ERR_ARG;
  const auto& e = p->pl.lastEarlyExitInfo();
  out[0] = (double)e.tied;
  out[1] = (double)e.open_at_limit;
  out[2] = (double)e.exact_replay;
  out[3] = e.resolve_ms;
  out[4] = (double)e.replay_updates;
  out[5] = (double)e.band_exact;
  return DYMU_OK;
}

int dymu_planner_last_early_exit_ex(dymu_planner* p, double* out, uint32_t n) {
  if (!p || (n && !out)) return DYMU_ERR_ARG;
  const auto& e = p->pl.lastEarlyExitInfo();
  const double v[8] = {(double)e.tied,           (double)e.open_at_limit, (double)e.exact_replay,
                       e.resolve_ms,             (double)e.replay_updates, (double)e.band_exact,
                       (double)e.near_ties,      (double)e.replay_threads};
  for (uint32_t q = 0; q < n && q < 8; ++q) out[q] = v[q];
  return DYMU_OK;
}

int dymu_planner_last_solve_kind(dymu_planner* p) {
  if (!p) return DYMU_ERR_ARG;
  return p->pl.lastSolveKind();
}

int dymu_planner_set_hazard_density_window(dymu_planner* p, uint32_t i0, uint32_t j0, uint32_t w,
                                           uint32_t h, const double* hd) {
  if (!p || !hd) return DYMU_ERR_ARG;
  return guarded([&] { return (int)p->pl.setHazardDensityWindow(i0, j0, w, h, hd); });
}

int dymu_planner_set_cost_map_window(dymu_planner* p, uint32_t i0, uint32_t j0, uint32_t w,
                                     uint32_t h, const double* cost) {
  if (!p || !cost) return DYMU_ERR_ARG;
  return guarded([&] { return (int)p->pl.setCostMapWindow(i0, j0, w, h, cost); });
}

int dymu_planner_track_obstacle_removal(dymu_planner* p, int on) {
  if (!p) return DYMU_ERR_ARG;
  p->pl.trackObstacleRemoval(on != 0);
  return DYMU_OK;
}

int dymu_planner_last_risk_raise(dymu_planner* p, uint64_t out[4]) {
  if (!p || !out) return DYMU_ERR_ARG;
  std::copy(p->pl.lastRiskRaise(), p->pl.lastRiskRaise() + 4, out);
  return DYMU_OK;
}

int dymu_planner_last_risk_update_kind(dymu_planner* p) {
  if (!p) return DYMU_ERR_ARG;
  return p->pl.lastRiskUpdateKind();
}

int dymu_planner_last_risk_update(dymu_planner* p, dymu_stats* out, uint32_t box[4]) {
  if (!p) return DYMU_ERR_ARG;
  if (out) *out = p->pl.lastRiskStats();
  if (box) std::copy(p->pl.lastRiskBox(), p->pl.lastRiskBox() + 4, box);
  return DYMU_OK;
}

int dymu_planner_set_trafficability_window(dymu_planner* p, uint32_t i0, uint32_t j0, uint32_t w,
                                           uint32_t h, const double* tr) {
  if (!p || !tr) return DYMU_ERR_ARG;
  return guarded([&] { return (int)p->pl.setTrafficabilityWindow(i0, j0, w, h, tr); });
}

int64_t dymu_planner_last_band_size(dymu_planner* p) {
  if (!p) return DYMU_ERR_ARG;
  return (int64_t)p->pl.lastBandSize();
}

int dymu_planner_get_global_node(dymu_planner* p, uint32_t i, uint32_t j, dymu_global_node* out) {
  if (!p || !out) return DYMU_ERR_ARG;
  return guarded([&] {
    const auto n = p->pl.getGlobalNode(i, j);
    if (!n) return 0;
    out->elevation = n->elevation;
    out->slope = n->slope;
    out->raw_cost = n->raw_cost;
    out->cost = n->cost;
    out->hazard_density = n->hazard_density;
    out->trafficability = n->trafficability;
    out->total_cost = n->total_cost;
    out->terrain = n->terrain;
    out->state = n->state == PathPlanning_lib::CLOSED ? 1 : 0;
    out->is_obstacle = n->isObstacle ? 1 : 0;
    out->has_local_map = n->hasLocalMap ? 1 : 0;
    return 1;
  });
}

int dymu_planner_is_safe_node(dymu_planner* p, uint32_t i, uint32_t j) {
  if (!p) return DYMU_ERR_ARG;
  return guarded([&] { return (int)p->pl.isSafeNode(i, j); });
}

int dymu_planner_is_fully_closed_node(dymu_planner* p, uint32_t i, uint32_t j) {
  if (!p) return DYMU_ERR_ARG;
  return guarded([&] { return (int)p->pl.isFullyClosedNode(i, j); });
}

int64_t dymu_planner_global_narrowband(dymu_planner* p, uint32_t* ij, int64_t max) {
  if (!p || (max > 0 && !ij)) return DYMU_ERR_ARG;
  int64_t n = 0;
  const int rc = guarded([&] {
    const auto band = p->pl.globalNarrowband();
    n = (int64_t)band.size();
    for (int64_t q = 0; q < n && q < max; ++q) {
      ij[2 * q] = (uint32_t)band[q].pose.position[0];
      ij[2 * q + 1] = (uint32_t)band[q].pose.position[1];
    }
    return DYMU_OK;
  });
  return rc < 0 ? rc : n;
}

int dymu_planner_min_cost_global_node(dymu_planner* p, uint32_t* ij, double* total_cost) {
  if (!p || !ij) return DYMU_ERR_ARG;
  return guarded([&] {
    const auto n = p->pl.minCostGlobalNode();
    if (!n) return 0;
    ij[0] = (uint32_t)n->pose.position[0];
    ij[1] = (uint32_t)n->pose.position[1];
    if (total_cost) *total_cost = n->total_cost;
    return 1;
  });
}

int dymu_planner_reset_global_narrow_band(dymu_planner* p) {
  if (!p) return DYMU_ERR_ARG;
  return guarded([&] { p->pl.resetGlobalNarrowBand(); return DYMU_OK; });
}

int dymu_planner_gradient_node(dymu_planner* p, uint32_t i, uint32_t j, double* d) {
  if (!p || !d) return DYMU_ERR_ARG;
  return guarded([&] {
    if (i >= p->pl.sizeX() || j >= p->pl.sizeY()) return (int)DYMU_ERR_ARG;
    p->pl.gradientNode(i, j, d[0], d[1]);
    return (int)DYMU_OK;
  });
}

int dymu_planner_propagate_global_node(dymu_planner* p, uint32_t i, uint32_t j) {
  if (!p) return DYMU_ERR_ARG;
  return guarded([&] {
    if (i >= p->pl.sizeX() || j >= p->pl.sizeY()) return (int)DYMU_ERR_ARG;
    p->pl.propagateGlobalNode(i, j);
    return (int)DYMU_OK;
  });
}

int dymu_planner_set_global_node_state(dymu_planner* p, uint32_t i, uint32_t j, int state) {
  if (!p || (state != 0 && state != 1)) return DYMU_ERR_ARG;
  return guarded([&] {
    if (i >= p->pl.sizeX() || j >= p->pl.sizeY()) return (int)DYMU_ERR_ARG;
    p->pl.setGlobalNodeState(i, j, state ? CLOSED : OPEN);
    return (int)DYMU_OK;
  });
}

int64_t dymu_planner_global_propagated_nodes(dymu_planner* p, uint32_t* ij, int64_t max) {
  if (!p || (max > 0 && !ij)) return DYMU_ERR_ARG;
  int64_t n = 0;
  const int rc = guarded([&] {
    if (max <= 0) {
      n = (int64_t)p->pl.globalPropagatedCount();
      return DYMU_OK;
    }
    const std::vector<uint64_t> ks = p->pl.globalPropagatedIndices();
    const uint64_t nx = p->pl.sizeX();
    n = (int64_t)ks.size();
    for (int64_t q = 0; q < n && q < max; ++q) {
      ij[2 * q] = (uint32_t)(ks[q] % nx);
      ij[2 * q + 1] = (uint32_t)(ks[q] / nx);
    }
    return DYMU_OK;
  });
  return rc < 0 ? rc : n;
}

int dymu_planner_get_node_states(dymu_planner* p, uint8_t* out) {
  if (!p || !out) return DYMU_ERR_ARG;
  return guarded([&] {
    p->pl.copyNodeStates(out);
    return (int)DYMU_OK;
  });
}

int dymu_planner_reset_total_cost_map(dymu_planner* p) {
  if (!p) return DYMU_ERR_ARG;
  p->pl.resetTotalCostMap();
  return DYMU_OK;
}

int dymu_planner_load_total_cost_map(dymu_planner* p, const double* T) {
  if (!p || !T) return DYMU_ERR_ARG;
  return guarded([&] { return (int)p->pl.loadTotalCostMap(T); });
}

int dymu_planner_set_current_path(dymu_planner* p, const double* xyzh, int n) {
  if (!p || n < 0 || (n > 0 && !xyzh)) return DYMU_ERR_ARG;
  return guarded([&] {
    p->pl.current_path.clear();
    for (int k = 0; k < n; ++k)
      p->pl.current_path.push_back(wp(xyzh[4 * k], xyzh[4 * k + 1], xyzh[4 * k + 2], xyzh[4 * k + 3]));
    return DYMU_OK;
  });
}

namespace {
int put_path(const std::vector<base::Waypoint>& path, double* out, int max_wp) {
  const int n = (int)path.size();
  for (int k = 0; k < n && k < max_wp; ++k) {
    out[4 * k + 0] = path[k].position[0];
    out[4 * k + 1] = path[k].position[1];
    out[4 * k + 2] = path[k].position[2];
    out[4 * k + 3] = path[k].heading;
  }
  return n;
}
}  // namespace

int dymu_planner_get_current_path(dymu_planner* p, double* out, int max_wp) {
  if (!p || !out || max_wp < 0) return DYMU_ERR_ARG;
  return put_path(p->pl.current_path, out, max_wp);
}

int dymu_planner_get_paths(dymu_planner* p, const double* starts, int n, int max_wp, int stride,
                           double* out, int* counts, int* status) {
  if (!p || n < 0) return DYMU_ERR_ARG;
  if (starts && (max_wp <= 0 || stride <= 0)) return DYMU_ERR_ARG;
  if (!starts && (!out || (size_t)n != p->paths.size())) return DYMU_ERR_ARG;
  return guarded([&] {
    if (starts) {
      std::vector<base::Waypoint> s((size_t)n);
      for (int q = 0; q < n; ++q)
        s[q] = wp(starts[4 * q], starts[4 * q + 1], starts[4 * q + 2], starts[4 * q + 3]);
      p->paths = p->pl.getPaths(s, &p->paths_status, (unsigned)max_wp, (unsigned)stride,
                                &p->paths_sinks);
    }
    for (int q = 0; q < n; ++q) {
      if (counts) counts[q] = (int)p->paths[q].size();
      if (status) status[q] = p->paths_status[q];
    }
    if (out) {
      for (const auto& path : p->paths) out += 4 * put_path(path, out, (int)path.size());
      p->paths.clear();
      p->paths.shrink_to_fit();
      p->paths_status.clear();
    }
    return n;
  });
}

namespace {
std::vector<base::Waypoint> wps(const double* a, int n, int width) {
  std::vector<base::Waypoint> v((size_t)n);
  for (int q = 0; q < n; ++q)
    v[q] = width == 4 ? wp(a[4 * q], a[4 * q + 1], a[4 * q + 2], a[4 * q + 3])
                      : wp(a[2 * q], a[2 * q + 1], 0, 0);
  return v;
}
}  // namespace

int dymu_planner_compute_total_cost_maps(dymu_planner* p, const double* xyzh, int n) {
  if (!p || !xyzh || n <= 0) return DYMU_ERR_ARG;
  return guarded([&] { return (int)p->pl.computeTotalCostMaps(wps(xyzh, n, 4)); });
}

int dymu_planner_batch_count(dymu_planner* p) {
  if (!p) return DYMU_ERR_ARG;
  return (int)p->pl.batchCount();
}

int dymu_planner_copy_batch_total_cost(dymu_planner* p, uint32_t b, double* out, int raw) {
  if (!p || !out) return DYMU_ERR_ARG;
  return guarded([&] { return (int)p->pl.copyBatchTotalCost(b, out, raw != 0); });
}

int dymu_planner_get_total_costs(dymu_planner* p, const double* xy, int n, double* out) {
  if (!p || n < 0 || (n > 0 && (!xy || !out))) return DYMU_ERR_ARG;
  return guarded([&] {
    std::vector<double> v;
    if (!p->pl.getTotalCosts(wps(xy, n, 2), v)) return 0;
    if (!v.empty()) std::memcpy(out, v.data(), sizeof(double) * v.size());
    return 1;
  });
}

int dymu_planner_cost_matrix(dymu_planner* p, const double* goals_xyzh, int n_goals,
                             const double* targets_xy, int n_targets, double* out) {
  if (!p || !goals_xyzh || n_goals <= 0 || n_targets < 0 || (n_targets > 0 && (!targets_xy || !out)))
    return DYMU_ERR_ARG;
  return guarded([&] {
    std::vector<double> v;
    if (!p->pl.costMatrix(wps(goals_xyzh, n_goals, 4), wps(targets_xy, n_targets, 2), v)) return 0;
    if (!v.empty()) std::memcpy(out, v.data(), sizeof(double) * v.size());
    return 1;
  });
}

int dymu_planner_cost_matrix_until(dymu_planner* p, const double* goals_xyzh, int n_goals,
                                   const double* targets_xy, int n_targets, double* out) {
  if (!p || !goals_xyzh || n_goals <= 0 || n_targets < 0 || (n_targets > 0 && (!targets_xy || !out)))
    return DYMU_ERR_ARG;
  return guarded([&] {
    std::vector<double> v;
    if (!p->pl.costMatrixUntil(wps(goals_xyzh, n_goals, 4), wps(targets_xy, n_targets, 2), v))
      return 0;
    if (!v.empty()) std::memcpy(out, v.data(), sizeof(double) * v.size());
    return 1;
  });
}

int dymu_planner_batch_level(dymu_planner* p, double* level) {
  if (!p || !level) return DYMU_ERR_ARG;
  *level = p->pl.batchLevel();
  return DYMU_OK;
}

int dymu_planner_get_paths_to(dymu_planner* p, uint32_t b, const double* starts, int n, int max_wp,
                              int stride, double* out, int* counts, int* status) {
  if (!starts) return dymu_planner_get_paths(p, nullptr, n, max_wp, stride, out, counts, status);
  if (!p || n < 0 || max_wp <= 0 || stride <= 0 || b >= p->pl.batchCount()) return DYMU_ERR_ARG;
  const int rc = guarded([&] {
    p->paths = p->pl.getPathsTo(b, wps(starts, n, 4), &p->paths_status, (unsigned)max_wp,
                                (unsigned)stride);
    p->paths_sinks.assign((size_t)n, 0);
    for (int q = 0; q < n; ++q)
      if (p->paths_status[q] != 1) p->paths_sinks[q] = -1;
    return DYMU_OK;
  });
  if (rc != DYMU_OK) return rc;
  // counts / status / the packed copy as dymu_planner_get_paths' second half does them
  for (int q = 0; q < n; ++q) {
    if (counts) counts[q] = (int)p->paths[q].size();
    if (status) status[q] = p->paths_status[q];
  }
  if (out) return dymu_planner_get_paths(p, nullptr, n, 0, 0, out, nullptr, nullptr);
  return n;
}

int dymu_planner_get_path_stats(dymu_planner* p, const double* starts, int n, int max_wp,
                                const double* field, int host, dymu_path_stat* out) {
  if (!p || n < 0 || max_wp <= 0 || (n > 0 && (!starts || !out))) return DYMU_ERR_ARG;
  return guarded([&] {
    const auto v = p->pl.getPathStats(wps(starts, n, 4), (unsigned)max_wp, field, host != 0);
    std::copy(v.begin(), v.end(), out);
    return n;
  });
}

int dymu_planner_get_path_stats_to(dymu_planner* p, uint32_t b, const double* starts, int n,
                                   int max_wp, const double* field, dymu_path_stat* out) {
  if (!p || n < 0 || max_wp <= 0 || (n > 0 && (!starts || !out)) || b >= p->pl.batchCount())
    return DYMU_ERR_ARG;
  return guarded([&] {
    const auto v = p->pl.getPathStatsTo(b, wps(starts, n, 4), (unsigned)max_wp, field);
    std::copy(v.begin(), v.end(), out);
    return n;
  });
}

namespace {
// the first half of the two-call protocol for a result `run` leaves in the handle
// (p->paths, p->paths_status, p->paths_sinks); the second half is dymu_planner_get_paths'
int arriving_paths(dymu_planner* p, int n, double* out, int* counts, int* status,
                   const std::function<void()>& run) {
  const int rc = guarded([&] {
    run();
    return DYMU_OK;
  });
  if (rc != DYMU_OK) return rc;
  for (int q = 0; q < n; ++q) {
    if (counts) counts[q] = (int)p->paths[q].size();
    if (status) status[q] = p->paths_status[q];
  }
  if (out) return dymu_planner_get_paths(p, nullptr, n, 0, 0, out, nullptr, nullptr);
  return n;
}
}  // namespace

int dymu_planner_get_arriving_paths(dymu_planner* p, const double* starts, int n, int max_wp,
                                    int stride, double* out, int* counts, int* status,
                                    dymu_arrive_stat* stats) {
  if (!starts) return dymu_planner_get_paths(p, nullptr, n, max_wp, stride, out, counts, status);
  if (!p || n < 0 || max_wp <= 0 || stride <= 0) return DYMU_ERR_ARG;
  return arriving_paths(p, n, out, counts, status, [&] {
    std::vector<DyMuPathPlanner::ArriveStats> rec;
    p->paths = p->pl.getArrivingPaths(wps(starts, n, 4), &p->paths_status, (unsigned)max_wp,
                                      (unsigned)stride, &p->paths_sinks, &rec);
    if (stats) std::copy(rec.begin(), rec.end(), stats);
  });
}

int dymu_planner_get_arriving_paths_to(dymu_planner* p, uint32_t b, const double* starts, int n,
                                       int max_wp, int stride, double* out, int* counts,
                                       int* status, dymu_arrive_stat* stats) {
  if (!starts) return dymu_planner_get_paths(p, nullptr, n, max_wp, stride, out, counts, status);
  if (!p || n < 0 || max_wp <= 0 || stride <= 0 || b >= p->pl.batchCount()) return DYMU_ERR_ARG;
  return arriving_paths(p, n, out, counts, status, [&] {
    std::vector<DyMuPathPlanner::ArriveStats> rec;
    p->paths = p->pl.getArrivingPathsTo(b, wps(starts, n, 4), &p->paths_status, (unsigned)max_wp,
                                        (unsigned)stride, &rec);
    p->paths_sinks.assign((size_t)n, 0);
    for (int q = 0; q < n; ++q)
      if (p->paths_status[q] != 1) p->paths_sinks[q] = -1;
    if (stats) std::copy(rec.begin(), rec.end(), stats);
  });
}

namespace {
// dymu_planner_get_simplified_paths[_to]: `run` leaves the result in the handle (first
// call), or the held result is copied out -- the indices packed like the waypoints
int simplified_paths(dymu_planner* p, bool first, int n, double* out, uint32_t* index,
                     int* counts, int* status, const std::function<void()>& run) {
  if (first) {
    const int rc = guarded([&] {
      run();
      return DYMU_OK;
    });
    if (rc != DYMU_OK) return rc;
    for (int q = 0; q < n; ++q) {
      if (counts) counts[q] = (int)p->paths[q].size();
      if (status) status[q] = p->paths_status[q];
    }
    if (!out) return n;
  }
  if (!out || (size_t)n != p->paths.size() || p->paths_index.size() != p->paths.size())
    return DYMU_ERR_ARG;
  if (index)
    for (const auto& v : p->paths_index) index = std::copy(v.begin(), v.end(), index);
  p->paths_index.clear();
  p->paths_index.shrink_to_fit();
  return dymu_planner_get_paths(p, nullptr, n, 0, 0, out, nullptr, nullptr);
}
}  // namespace

int dymu_planner_get_simplified_paths(dymu_planner* p, const double* starts, int n, double eps,
                                      int max_wp, double* out, uint32_t* index, int* counts,
                                      int* status, dymu_arrive_stat* stats) {
  if (!p || n < 0) return DYMU_ERR_ARG;
  if (starts && (max_wp <= 0 || !(eps > 0) || !(eps < HUGE_VAL))) return DYMU_ERR_ARG;
  return simplified_paths(p, starts != nullptr, n, out, index, counts, status, [&] {
    std::vector<DyMuPathPlanner::ArriveStats> rec;
    p->paths = p->pl.getSimplifiedPaths(wps(starts, n, 4), eps, &p->paths_status,
                                        (unsigned)max_wp, &p->paths_sinks, &rec, &p->paths_index);
    if (stats) std::copy(rec.begin(), rec.end(), stats);
  });
}

int dymu_planner_get_simplified_paths_to(dymu_planner* p, uint32_t b, const double* starts, int n,
                                         double eps, int max_wp, double* out, uint32_t* index,
                                         int* counts, int* status, dymu_arrive_stat* stats) {
  if (!p || n < 0) return DYMU_ERR_ARG;
  if (starts && (max_wp <= 0 || !(eps > 0) || !(eps < HUGE_VAL) || b >= p->pl.batchCount()))
    return DYMU_ERR_ARG;
  return simplified_paths(p, starts != nullptr, n, out, index, counts, status, [&] {
    std::vector<DyMuPathPlanner::ArriveStats> rec;
    p->paths = p->pl.getSimplifiedPathsTo(b, wps(starts, n, 4), eps, &p->paths_status,
                                          (unsigned)max_wp, &rec, &p->paths_index);
    p->paths_sinks.assign((size_t)n, 0);
    for (int q = 0; q < n; ++q)
      if (p->paths_status[q] != 1) p->paths_sinks[q] = -1;
    if (stats) std::copy(rec.begin(), rec.end(), stats);
  });
}

int dymu_planner_last_simplified(dymu_planner* p, uint64_t* reruns, uint64_t* bytes) {
  if (!p) return DYMU_ERR_ARG;
  if (reruns) *reruns = p->pl.lastSimplifiedReruns();
  if (bytes) *bytes = p->pl.lastSimplifiedBytes();
  return DYMU_OK;
}

int dymu_planner_get_arriving_stats(dymu_planner* p, const double* starts, int n, int max_wp,
                                    int host, dymu_arrive_stat* out) {
  if (!p || n < 0 || max_wp <= 0 || (n > 0 && (!starts || !out))) return DYMU_ERR_ARG;
  return guarded([&] {
    const auto v = p->pl.getArrivingStats(wps(starts, n, 4), (unsigned)max_wp, host != 0);
    std::copy(v.begin(), v.end(), out);
    return n;
  });
}

int dymu_planner_get_arriving_stats_to(dymu_planner* p, uint32_t b, const double* starts, int n,
                                       int max_wp, dymu_arrive_stat* out) {
  if (!p || n < 0 || max_wp <= 0 || (n > 0 && (!starts || !out)) || b >= p->pl.batchCount())
    return DYMU_ERR_ARG;
  return guarded([&] {
    const auto v = p->pl.getArrivingStatsTo(b, wps(starts, n, 4), (unsigned)max_wp);
    std::copy(v.begin(), v.end(), out);
    return n;
  });
}

namespace {
// a flat route request: the outputs are the non-NULL maps of `out`; false: rejected
bool route_request(const double* const* fields, int n_fields, const dymu_route_out* out,
                   DyMuPathPlanner::RouteRequest& rq) {
  typedef DyMuPathPlanner P;
  if (!out || n_fields < 0 || n_fields > DYMU_PATH_FIELDS || (n_fields && !fields)) return false;
  rq.outputs = (out->sink ? P::kRouteSink : 0u) | (out->axis ? P::kRouteAxis : 0u) |
               (out->diag ? P::kRouteDiag : 0u) | (out->length ? P::kRouteLength : 0u);
  for (int f = 0; f < DYMU_PATH_FIELDS; ++f) {
    if (f >= n_fields && (out->integral[f] || out->vmin[f] || out->vmax[f])) return false;
    if (f >= n_fields) continue;
    // a per-field output is computed for every field or for none
    if (out->integral[f]) rq.outputs |= P::kRouteIntegral;
    if (out->vmin[f]) rq.outputs |= P::kRouteMin;
    if (out->vmax[f]) rq.outputs |= P::kRouteMax;
  }
  rq.fields.assign(fields, fields + n_fields);
  return true;
}
void route_copy(const DyMuPathPlanner::RouteFields& r, int n_fields, const dymu_route_out* out) {
  if (out->sink) std::copy(r.sink.begin(), r.sink.end(), out->sink);
  if (out->axis) std::copy(r.axis.begin(), r.axis.end(), out->axis);
  if (out->diag) std::copy(r.diag.begin(), r.diag.end(), out->diag);
  if (out->length) std::copy(r.length.begin(), r.length.end(), out->length);
  for (int f = 0; f < n_fields; ++f) {
    if (out->integral[f]) std::copy(r.integral[f].begin(), r.integral[f].end(), out->integral[f]);
    if (out->vmin[f]) std::copy(r.vmin[f].begin(), r.vmin[f].end(), out->vmin[f]);
    if (out->vmax[f]) std::copy(r.vmax[f].begin(), r.vmax[f].end(), out->vmax[f]);
  }
}
}  // namespace

int dymu_planner_get_route_fields(dymu_planner* p, const double* const* fields, int n_fields,
                                  int host, const dymu_route_out* out, uint32_t* rounds) {
  DyMuPathPlanner::RouteRequest rq;
  if (!p || !route_request(fields, n_fields, out, rq)) return DYMU_ERR_ARG;
  rq.host = host != 0;
  return guarded([&] {
    const auto r = p->pl.getRouteFields(rq);
    route_copy(r, n_fields, out);
    if (rounds) *rounds = r.rounds;
    return DYMU_OK;
  });
}

int dymu_planner_get_route_fields_to(dymu_planner* p, uint32_t b, const double* const* fields,
                                     int n_fields, const dymu_route_out* out, uint32_t* rounds) {
  DyMuPathPlanner::RouteRequest rq;
  if (!p || !route_request(fields, n_fields, out, rq) || b >= p->pl.batchCount())
    return DYMU_ERR_ARG;
  return guarded([&] {
    const auto r = p->pl.getRouteFieldsTo(b, rq);
    route_copy(r, n_fields, out);
    if (rounds) *rounds = r.rounds;
    return DYMU_OK;
  });
}

namespace {
// a flat usage request: the outputs are the non-NULL maps of `out` and the catchment;
// false: rejected
bool usage_request(const uint32_t* weights, const dymu_usage_out* out, const uint64_t* catchment,
                   DyMuPathPlanner::RouteUsageRequest& rq) {
  typedef DyMuPathPlanner P;
  if (!out) return false;
  rq.outputs = (out->usage ? P::kUsageUsage : 0u) | (out->far ? P::kUsageFar : 0u) |
               (out->sink ? P::kUsageSink : 0u) | (catchment ? P::kUsageCatchment : 0u);
  rq.weights = weights;
  return rq.outputs != 0;
}
int usage_copy(const DyMuPathPlanner::RouteUsage& r, const dymu_usage_out* out,
               uint64_t* catchment, uint32_t n_catchment) {
  if (catchment && r.catchment.size() > n_catchment) return DYMU_ERR_ARG;
  if (out->usage) std::copy(r.usage.begin(), r.usage.end(), out->usage);
  if (out->far) std::copy(r.far.begin(), r.far.end(), out->far);
  if (out->sink) std::copy(r.sink.begin(), r.sink.end(), out->sink);
  if (catchment) {
    std::fill(catchment, catchment + n_catchment, (uint64_t)0);
    std::copy(r.catchment.begin(), r.catchment.end(), catchment);
  }
  return DYMU_OK;
}
}  // namespace

int dymu_planner_get_route_usage(dymu_planner* p, const uint32_t* weights, int host,
                                 const dymu_usage_out* out, uint64_t* catchment,
                                 uint32_t n_catchment, uint32_t* rounds) {
  DyMuPathPlanner::RouteUsageRequest rq;
  if (!p || !usage_request(weights, out, catchment, rq)) return DYMU_ERR_ARG;
  if (catchment && p->pl.hasGoal() && p->pl.goalCount() > n_catchment) return DYMU_ERR_ARG;
  rq.host = host != 0;
  return guarded([&] {
    const auto r = p->pl.getRouteUsage(rq);
    const int rc = usage_copy(r, out, catchment, n_catchment);
    if (rc == DYMU_OK && rounds) *rounds = r.rounds;
    return rc;
  });
}

int dymu_planner_get_route_usage_to(dymu_planner* p, uint32_t b, const uint32_t* weights,
                                    const dymu_usage_out* out, uint64_t* catchment,
                                    uint32_t n_catchment, uint32_t* rounds) {
  DyMuPathPlanner::RouteUsageRequest rq;
  if (!p || !usage_request(weights, out, catchment, rq) || b >= p->pl.batchCount() ||
      (catchment && n_catchment < 1))
    return DYMU_ERR_ARG;
  return guarded([&] {
    const auto r = p->pl.getRouteUsageTo(b, rq);
    const int rc = usage_copy(r, out, catchment, n_catchment);
    if (rc == DYMU_OK && rounds) *rounds = r.rounds;
    return rc;
  });
}

int dymu_planner_goal_cell(dymu_planner* p, uint32_t* i, uint32_t* j) {
  if (!p || !i || !j) return DYMU_ERR_ARG;
  if (!p->pl.hasGoal()) return 0;
  *i = p->pl.goalI();
  *j = p->pl.goalJ();
  return 1;
}

int dymu_planner_last_batch_stats(dymu_planner* p, dymu_stats* out) {
  if (!p || !out) return DYMU_ERR_ARG;
  *out = p->pl.lastBatchStats();
  return DYMU_OK;
}

int dymu_planner_track_speed_changes(dymu_planner* p, int on) {
  if (!p) return DYMU_ERR_ARG;
  p->pl.trackSpeedChanges(on != 0);
  return DYMU_OK;
}

int dymu_planner_last_batch_solve_kind(dymu_planner* p) {
  if (!p) return DYMU_ERR_ARG;
  return p->pl.lastBatchSolveKind();
}

namespace {
// the flat lists of the combine entries as the vectors the planner takes (planes NULL: all
// maps, one weight / offset per map of the batch)
struct CombineLists {
  std::vector<uint32_t> planes;
  std::vector<double> weights, offsets;
  CombineLists(dymu_planner* p, const uint32_t* pl, uint32_t n_planes, const double* w,
               const double* o) {
    const size_t n = pl ? n_planes : p->pl.batchCount();
    if (pl) planes.assign(pl, pl + n);
    if (w) weights.assign(w, w + n);
    if (o) offsets.assign(o, o + n);
  }
};
}  // namespace

int dymu_planner_combine_total_cost_maps(dymu_planner* p, int op, const uint32_t* planes,
                                         uint32_t n_planes, const double* weights,
                                         const double* offsets, dymu_reduce_summary* summary) {
  if (!p || op < 0 || op > 2 || (planes && n_planes == 0)) return DYMU_ERR_ARG;
  return guarded([&] {
    const CombineLists l(p, planes, n_planes, weights, offsets);
    return (int)p->pl.combineTotalCostMaps((DyMuPathPlanner::CombineOp)op, l.planes, l.weights,
                                           l.offsets, summary);
  });
}

int dymu_planner_copy_combined_total_cost(dymu_planner* p, double* out, int raw) {
  if (!p || !out) return DYMU_ERR_ARG;
  return guarded([&] { return (int)p->pl.copyCombinedTotalCost(out, raw != 0); });
}

int dymu_planner_copy_combined_planes(dymu_planner* p, uint32_t* out) {
  if (!p || !out) return DYMU_ERR_ARG;
  return guarded([&] { return (int)p->pl.copyCombinedPlanes(out); });
}

int dymu_planner_via_corridor(dymu_planner* p, uint32_t a, uint32_t b, double slack, uint8_t* mask,
                              dymu_corridor_info* info) {
  if (!p || !mask || !info) return DYMU_ERR_ARG;
  return guarded([&] {
    DyMuPathPlanner::CorridorInfo ci{};
    if (!p->pl.viaCorridor(a, b, slack, mask, &ci)) return 0;
    *info = dymu_corridor_info{ci.D_min, ci.min_i, ci.min_j, ci.count, ci.i0,
                               ci.j0,    ci.i1,    ci.j1,    ci.bound};
    return 1;
  });
}

int dymu_planner_rendezvous(dymu_planner* p, const uint32_t* planes, uint32_t n_planes,
                            const double* weights, const double* offsets, int minimax, uint32_t* i,
                            uint32_t* j, double* value) {
  if (!p || !i || !j || !value || (planes && n_planes == 0)) return DYMU_ERR_ARG;
  return guarded([&] {
    const CombineLists l(p, planes, n_planes, weights, offsets);
    unsigned ci = 0, cj = 0;
    double v = 0.0;
    if (!p->pl.rendezvous(l.planes, l.weights, l.offsets, minimax != 0, &ci, &cj, &v)) return 0;
    *i = ci, *j = cj, *value = v;
    return 1;
  });
}

int dymu_planner_last_combine_kernel_ms(dymu_planner* p, double* ms) {
  if (!p || !ms) return DYMU_ERR_ARG;
  *ms = p->pl.lastCombineKernelMs();
  return DYMU_OK;
}

int dymu_planner_set_goals(dymu_planner* p, const double* xyzh, const double* offsets, int n) {
  if (!p || !xyzh || n <= 0) return DYMU_ERR_ARG;
  return guarded([&] {
    std::vector<base::Waypoint> g((size_t)n);
    for (int q = 0; q < n; ++q)
      g[q] = wp(xyzh[4 * q], xyzh[4 * q + 1], xyzh[4 * q + 2], xyzh[4 * q + 3]);
    std::vector<double> off;
    if (offsets) off.assign(offsets, offsets + n);
    return (int)p->pl.setGoals(g, off);
  });
}

int dymu_planner_goal_count(dymu_planner* p) {
  if (!p) return DYMU_ERR_ARG;
  return (int)p->pl.goalCount();
}

int dymu_planner_get_goal_labels(dymu_planner* p, uint32_t* out) {
  if (!p || !out) return DYMU_ERR_ARG;
  return guarded([&] { p->pl.copyGoalLabels(out); return DYMU_OK; });
}

int dymu_planner_goal_label(dymu_planner* p, double x, double y) {
  if (!p) return -1;
  int lab = -1;
  const int rc = guarded([&] { lab = p->pl.goalLabel(wp(x, y, 0, 0)); return DYMU_OK; });
  return rc < 0 ? rc : lab;
}

int dymu_planner_last_path_sinks(dymu_planner* p, int* out, int n) {
  if (!p || !out || n < 0 || (size_t)n != p->paths_sinks.size()) return DYMU_ERR_ARG;
  std::copy(p->paths_sinks.begin(), p->paths_sinks.end(), out);
  return n;
}

int dymu_planner_last_paths_on_device(dymu_planner* p) {
  if (!p) return DYMU_ERR_ARG;
  return p->pl.lastPathsOnDevice() ? 1 : 0;
}

int dymu_planner_last_paths_kernel_ms(dymu_planner* p, double* ms) {
  if (!p || !ms) return DYMU_ERR_ARG;
  *ms = p->pl.lastPathsKernelMs();
  return DYMU_OK;
}

int dymu_planner_compute_local_planning(dymu_planner* p, double x, double y, double z, double h,
                                        const uint8_t* image, uint32_t width, uint32_t height,
                                        uint32_t row_size, uint32_t pixel_size, double res,
                                        double* traj, int max_traj, int* n_traj,
                                        double* local_time_s) {
  if (!p || (!image && width && height) || max_traj < 0 || (max_traj > 0 && !traj) ||
      (height > 0 && width > 0 && (uint64_t)(height - 1) * row_size + (uint64_t)(width - 1) * pixel_size >= (uint64_t)height * row_size))
    return DYMU_ERR_ARG;
  return guarded([&] {
    base::samples::frame::Frame f;
    f.width = width;
    f.height = height;
    f.row_size = row_size;
    f.pixel_size = pixel_size;
    f.image.assign(image, image + (size_t)height * row_size);
    std::vector<base::Waypoint> trajectory;
    base::Time t;
    const bool r = p->pl.computeLocalPlanning(wp(x, y, z, h), f, res, trajectory, t);
    if (r) {
      const int n = put_path(trajectory, traj, max_traj);
      if (n_traj) *n_traj = n;
      if (local_time_s) *local_time_s = t.toSeconds();
    } else if (n_traj) {
      *n_traj = 0;
    }
    return (int)r;
  });
}

int dymu_planner_repair_path(dymu_planner* p, double x, double y, double z, double h,
                             uint32_t index) {
  if (!p) return DYMU_ERR_ARG;
  return guarded([&] { return p->pl.repairPath(wp(x, y, z, h), index); });
}

int dymu_planner_evaluate_path(dymu_planner* p, uint32_t starting_index) {
  if (!p) return DYMU_ERR_ARG;
  return guarded([&] { return (int)p->pl.evaluatePath(starting_index); });
}

int dymu_planner_expand_risk(dymu_planner* p) {
  if (!p) return DYMU_ERR_ARG;
  return guarded([&] { p->pl.expandRisk(); return DYMU_OK; });
}

int dymu_planner_set_local_timeout(dymu_planner* p, double seconds) {
  if (!p) return DYMU_ERR_ARG;
  p->pl.setLocalPropagationTimeout(seconds);
  return DYMU_OK;
}

int dymu_planner_local_waypoint_dijkstra(dymu_planner* p, const double* s, double* out) {
  if (!p || !s || !out) return DYMU_ERR_ARG;
  return guarded([&] {
    const auto n = p->pl.getLocalNode(wp(s[0], s[1], s[2], s[3]));
    if (!n) return 0;
    const base::Waypoint w = p->pl.computeLocalWaypointDijkstra(*n);
    out[0] = w.position[0];
    out[1] = w.position[1];
    out[2] = w.position[2];
    out[3] = w.heading;
    return 1;
  });
}

int dymu_planner_local_agent(dymu_planner* p, double* xy) {
  if (!p || !xy) return DYMU_ERR_ARG;
  return guarded([&] {
    const auto n = p->pl.localAgent();
    if (!n) return 0;
    xy[0] = n->global_pose.position[0];
    xy[1] = n->global_pose.position[1];
    return 1;
  });
}

namespace {
void flat_local(const localNode& n, dymu_local_node* out) {
  out->global_x = n.global_pose.position[0];
  out->global_y = n.global_pose.position[1];
  out->deviation = n.deviation;
  out->total_cost = n.total_cost;
  out->risk = n.risk;
  out->parent_i = (uint32_t)n.parent_pose.position[0];
  out->parent_j = (uint32_t)n.parent_pose.position[1];
  out->li = (uint32_t)n.pose.position[0];
  out->lj = (uint32_t)n.pose.position[1];
  out->state = n.state == CLOSED ? 1 : 0;
  out->is_obstacle = n.isObstacle ? 1 : 0;
  out->id = n.id;
}
localNode by_id(uint64_t id) {
  localNode n;
  n.id = id;
  return n;
}
}  // namespace

int dymu_planner_get_local_node(dymu_planner* p, double x, double y, dymu_local_node* out) {
  if (!p || !out) return DYMU_ERR_ARG;
  return guarded([&] {
    const auto n = p->pl.getLocalNode(wp(x, y, 0.0, 0.0));
    if (!n) return 0;
    flat_local(*n, out);
    return 1;
  });
}

int dymu_planner_local_neighbour(dymu_planner* p, uint64_t id, int d, dymu_local_node* out) {
  if (!p || !out || d < 0 || d > 3) return DYMU_ERR_ARG;
  return guarded([&] {
    const auto n = p->pl.localNeighbour(by_id(id), d);
    if (!n) return 0;
    flat_local(*n, out);
    return 1;
  });
}

int dymu_planner_max_risk_node(dymu_planner* p, dymu_local_node* out) {
  if (!p || !out) return DYMU_ERR_ARG;
  return guarded([&] {
    const auto n = p->pl.maxRiskNode();
    if (!n) return 0;
    flat_local(*n, out);
    return 1;
  });
}

int dymu_planner_propagate_risk(dymu_planner* p, uint64_t id) {
  if (!p) return DYMU_ERR_ARG;
  return guarded([&] { p->pl.propagateRisk(by_id(id)); return (int)DYMU_OK; });
}

int dymu_planner_propagate_local_node(dymu_planner* p, uint64_t id) {
  if (!p) return DYMU_ERR_ARG;
  return guarded([&] { p->pl.propagateLocalNode(by_id(id)); return (int)DYMU_OK; });
}

int dymu_planner_set_local_node_state(dymu_planner* p, uint64_t id, int state) {
  if (!p || (state != 0 && state != 1)) return DYMU_ERR_ARG;
  return guarded([&] {
    p->pl.setLocalNodeState(by_id(id), state ? CLOSED : OPEN);
    return (int)DYMU_OK;
  });
}

int dymu_planner_min_cost_local_node(dymu_planner* p, double Tovertake, double minC,
                                     dymu_local_node* out) {
  if (!p || !out) return DYMU_ERR_ARG;
  return guarded([&] {
    const auto n = p->pl.minCostLocalNode(Tovertake, minC);
    if (!n) return 0;
    flat_local(*n, out);
    return 1;
  });
}

int dymu_planner_min_cost_local_node_reach(dymu_planner* p, uint64_t reach_id,
                                           dymu_local_node* out) {
  if (!p || !out) return DYMU_ERR_ARG;
  return guarded([&] {
    const auto n = p->pl.minCostLocalNode(by_id(reach_id));
    if (!n) return 0;
    flat_local(*n, out);
    return 1;
  });
}

int64_t dymu_planner_local_list(dymu_planner* p, int which, dymu_local_node* out, int64_t max) {
  if (!p || which < 0 || which > 2 || (max > 0 && !out)) return DYMU_ERR_ARG;
  int64_t n = 0;
  const int rc = guarded([&] {
    const auto v = which == 0   ? p->pl.localNarrowband()
                   : which == 1 ? p->pl.localExpandableObstacles()
                                : p->pl.localPropagatedNodes();
    n = (int64_t)v.size();
    for (int64_t q = 0; q < n && q < max; ++q) flat_local(v[q], &out[q]);
    return DYMU_OK;
  });
  return rc < 0 ? rc : n;
}

int dymu_planner_compute_local_propagation(dymu_planner* p, const double* s, const double* o,
                                           double* set_xy) {
  if (!p || !s || !o) return DYMU_ERR_ARG;
  return guarded([&] {
    const auto n = p->pl.computeLocalPropagation(wp(s[0], s[1], s[2], s[3]), wp(o[0], o[1], o[2], o[3]));
    if (!n) return 0;
    if (set_xy) {
      set_xy[0] = n->global_pose.position[0];
      set_xy[1] = n->global_pose.position[1];
    }
    return 1;
  });
}

int dymu_planner_get_risk_matrix(dymu_planner* p, double x, double y, double z, double h,
                                 double* out) {
  if (!p || !out) return DYMU_ERR_ARG;
  return guarded([&] { from_rows(p->pl.getRiskMatrix(wp(x, y, z, h)), out); return DYMU_OK; });
}

int dymu_planner_get_deviation_matrix(dymu_planner* p, double x, double y, double z, double h,
                                      double* out) {
  if (!p || !out) return DYMU_ERR_ARG;
  return guarded([&] { from_rows(p->pl.getDeviationMatrix(wp(x, y, z, h)), out); return DYMU_OK; });
}

int dymu_planner_get_reconnecting_index(dymu_planner* p) {
  if (!p) return DYMU_ERR_ARG;
  return p->pl.getReconnectingIndex();
}

int dymu_planner_res_ratio(dymu_planner* p) {
  if (!p) return DYMU_ERR_ARG;
  return (int)p->pl.resRatio();
}

int64_t dymu_planner_local_map_mask(dymu_planner* p, uint8_t* mask) {
  if (!p) return DYMU_ERR_ARG;
  return (int64_t)p->pl.localMapMask(mask);
}

int dymu_planner_local_block(dymu_planner* p, uint32_t i, uint32_t j, double* dev, double* tc,
                             double* risk, uint8_t* state, uint8_t* obst) {
  if (!p) return DYMU_ERR_ARG;
  return (int)p->pl.localBlock(i, j, dev, tc, risk, state, obst);
}

}  // extern "C"
