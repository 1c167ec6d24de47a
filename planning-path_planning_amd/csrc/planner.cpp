// planner.cpp -- PathPlanning_lib::DyMuPathPlanner over SoA arrays (DyMu.hpp).
//
// Host C++ around the MI355X engine: cost-map ingestion, goal validation and
// path extraction run on the host exactly as the reference computes them
// (compiled with -ffp-contract=off so each operation rounds where the
// reference's does); the total-cost propagation -- the reference's FMM loop
// -- runs on the GPU over a device-resident speed / total-cost map:
//   * the speed F is packed on the host only for the rows whose node fields
//     changed, and only the rows whose speed changed are uploaded;
//   * the total cost stays on the device; the host mirror fetches blocks of it
//     on first read (path extraction reads a narrow band around the path) or
//     all of it for the matrix getters.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <cstdio>
#include <limits>
#include <stdexcept>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "DyMu.hpp"
#include "local_layer.hpp"
#include "path_simplify.h"
#include "pop_order.hpp"

namespace PathPlanning_lib {

namespace {
constexpr double kInf = std::numeric_limits<double>::infinity();

void log_warn(const char* m) { std::fprintf(stderr, "[dymu] WARN: %s\n", m); }
void log_error(const char* m) { std::fprintf(stderr, "[dymu] ERROR: %s\n", m); }
}  // namespace

DyMuPathPlanner::DyMuPathPlanner(double risk_distance, double reconnect_distance,
                                 double risk_ratio, repairingAproach input_approach)
    : risk_distance_(risk_distance),
      reconnect_distance_(reconnect_distance),
      risk_ratio_(risk_ratio),
      repairing_approach_(input_approach) {}

namespace {
void release_engine(dymu_ctx*& ctx, double*& dF, double*& dT, void*& reg, uint64_t& cells) {
  if (!ctx) return;
  if (reg) (void)dymu_host_unregister(ctx, reg);
  if (dF) (void)dymu_device_free(ctx, dF);
  if (dT) (void)dymu_device_free(ctx, dT);
  dymu_destroy(ctx);
  ctx = nullptr;
  dF = dT = nullptr;
  reg = nullptr;
  cells = 0;
}
}  // namespace

DyMuPathPlanner::~DyMuPathPlanner() {
  dropLabels();
  dropBatch();
  dropCombined();
  dropRiskMaps();
  release_engine(ctx_, dF_, dT_, registered_, dcells_);
}

void DyMuPathPlanner::setEngineOptions(const dymu_opts& o) {
  opts_ = o;
  // the solved map lives in dT_: bring the host mirror up to date before the
  // device buffers go, so T(), getPath and the matrix getters keep working
  if (ctx_ && dT_ && blk_missing_) fetchAll();
  dropLabels();
  dropBatch();
  dropCombined();
  dropRiskMaps();
  release_engine(ctx_, dF_, dT_, registered_, dcells_);
  dev_map_current_ = false;
  solved_ = false, gs_seeds_.clear();
  speed_valid_ = false;
  markDirty(0, ny_);
}

// :39-104.  Node fields start as the globalNode constructor sets them
// (src/DyMu.hpp:88-107): cost 0, raw_cost 0, hazard 0, traff 1, T = +inf,
// OPEN, not an obstacle, locomotion "DONT_CARE".  Neighbour lists are implicit
// in the row-major layout.
bool DyMuPathPlanner::initGlobalLayer(double globalres, double localres, unsigned num_nodes_X,
                                      unsigned num_nodes_Y, std::vector<double> offset) {
  global_res_ = globalres;
  local_res_ = localres;
  {
    const double rr = global_res_ / local_res_;  // :49 res_ratio = (uint)(global_res / local_res)
    res_ratio_ = grid_u32(rr);
  }
  if (!local_) local_ = std::make_unique<LocalLayer>();
  local_->reset(res_ratio_);
  local_agent_ = -1;
  reconnecting_index = 0;
  solved_ = false, gs_seeds_.clear();
  nx_ = num_nodes_X;
  ny_ = num_nodes_Y;
  global_offset_ = offset;
  if (global_offset_.size() < 2) global_offset_.resize(2, 0.0);
  const uint64_t n = (uint64_t)nx_ * ny_;
  elevation_.assign(n, 0.0);
  slope_.assign(n, 0.0);
  raw_cost_.assign(n, 0.0);
  cost_.assign(n, 0.0);
  hazard_.assign(n, 0.0);
  traff_.assign(n, 1.0);
  terrain_.assign(n, 0u);
  is_obstacle_.assign(n, 0);
  loc_mode_.assign(n, -1);
  has_goal_ = false;
  goals_.clear();
  dropLabels();
  dropBatch();
  dropCombined();
  pend_ = false;
  current_path.clear();
  // a new grid: new device buffers and an empty total-cost map (every node
  // OPEN at +inf, as the globalNode constructor leaves it)
  release_engine(ctx_, dF_, dT_, registered_, dcells_);
  dev_map_current_ = false;
  total_cost_.assign(n, kInf);
  nbx_ = (nx_ + kBlk - 1) / kBlk;
  nby_ = (ny_ + kBlk - 1) / kBlk;
  blk_ok_.assign((uint64_t)nbx_ * nby_, 1);
  blk_missing_ = 0;
  closed_limit_ = 0.0;
  band_cells_.clear();
  band_unordered_ = false;
  band_values_checked_ = true;
  open_at_limit_.clear();
  node_state_.clear();
  propagated_extra_.clear();
  manual_list_ = false;
  speed_.clear();
  speed_valid_ = false;
  if (globalRiskOn()) global_risk_.assign(n, 0.0);
  risk_stale_ = true;
  markDirty(0, ny_);
  return true;
}

// :109-126
bool DyMuPathPlanner::setCostMap(std::vector<std::vector<double>> cost_map) {
  if (cost_map.size() != ny_ || cost_map.empty() || cost_map[0].size() != nx_) return false;
  for (unsigned j = 0; j < ny_; ++j) {
    if (cost_map[j].size() != nx_) return false;
    for (unsigned i = 0; i < nx_; ++i) {
      const double c = cost_map[j][i];
      const uint64_t k = idx(i, j);
      cost_[k] = c;
      if (c <= 0) {
        is_obstacle_[k] = 1;
        traff_[k] = 0.0;
        hazard_[k] = 1.0;
      }
    }
  }
  risk_stale_ = true;
  markDirty(0, ny_);
  return true;
}

#pragma weak dymu_clearance_update_device
#pragma weak dymu_clearance_edit_device
#pragma weak dymu_last_update_stats

// setCostMap's per-cell rule on the cells of the box alone.  With the global risk on, the
// obstacle mask is that of the raw speed (refreshGlobalRisk): a cell the box turns into an
// obstacle joins the pending box of the incremental update, and so does a cell it frees
// while trackObstacleRemoval is on and the engine has the edit entry; otherwise a freed
// cell, or a field on the device that is not the one R belongs to, leaves the whole
// recompute.
bool DyMuPathPlanner::setCostMapWindow(unsigned i0, unsigned j0, unsigned w, unsigned h,
                                       const double* cost) {
  if (!cost || (uint64_t)i0 + w > nx_ || (uint64_t)j0 + h > ny_) return false;
  const bool risk = globalRiskOn();
  bool added = false, freed = false;
  for (unsigned r = 0; r < h; ++r)
    for (unsigned q = 0; q < w; ++q) {
      const double c = cost[(uint64_t)r * w + q];
      const uint64_t k = idx(i0 + q, j0 + r);
      const bool was = risk && !(rawSpeed(k) < kInf);
      cost_[k] = c;
      if (c <= 0) {
        is_obstacle_[k] = 1;
        traff_[k] = 0.0;
        hazard_[k] = 1.0;
      }
      if (risk) {
        const bool now = !(rawSpeed(k) < kInf);
        added = added || (now && !was);
        freed = freed || (was && !now);
      }
    }
  markDirty(j0, j0 + h);
  const bool can_free = track_removal_ && &dymu_clearance_edit_device;
  if ((freed && !can_free) ||
      ((added || freed) && (risk_stale_ || !risk_dev_valid_ || !&dymu_clearance_update_device))) {
    risk_stale_ = true;
  } else if (added || freed) {
    risk_pend_freed_ = (risk_pend_ && risk_pend_freed_) || freed;
    if (!risk_pend_) {
      rpend_i0_ = i0, rpend_i1_ = i0 + w, rpend_j0_ = j0, rpend_j1_ = j0 + h;
    } else {
      rpend_i0_ = std::min(rpend_i0_, i0), rpend_i1_ = std::max(rpend_i1_, i0 + w);
      rpend_j0_ = std::min(rpend_j0_, j0), rpend_j1_ = std::max(rpend_j1_, j0 + h);
    }
    risk_pend_ = true;
  }
  return true;
}

namespace {

// Host threads for the per-node loops of computeCostMap: DYMU_HOST_THREADS, else
// OMP_NUM_THREADS, else the hardware's, at most 64.
unsigned host_threads() {
  for (const char* v : {"DYMU_HOST_THREADS", "OMP_NUM_THREADS"})
    if (const char* kv = std::getenv(v)) {
      const int t = std::atoi(kv);
      if (t > 0) return (unsigned)std::min(t, 64);
    }
  const unsigned h = std::thread::hardware_concurrency();
  return h ? std::min(h, 64u) : 1u;
}

// body(t) for t in [0, nt) on nt threads (the caller's among them).  Exceptions
// thrown by body on a worker thread are carried back and rethrown on the calling
// thread (a throw escaping a std::thread would std::terminate); the started threads
// are joined on every path, a failed thread start included.
template <class Body>
void parallel_tasks(unsigned nt, Body&& body) {
  if (nt <= 1) {
    body(0u);
    return;
  }
  std::vector<std::exception_ptr> errs(nt);
  struct Joiner {
    std::vector<std::thread> pool;
    ~Joiner() {
      for (auto& th : pool)
        if (th.joinable()) th.join();
    }
  } J;
  J.pool.reserve(nt - 1);
  auto run = [&body, &errs](unsigned t) {
    try {
      body(t);
    } catch (...) {
      errs[t] = std::current_exception();
    }
  };
  try {
    for (unsigned t = 1; t < nt; ++t) J.pool.emplace_back(run, t);
  } catch (...) {  // std::system_error from a thread start: finish what started, rethrow
    for (auto& th : J.pool) th.join();
    J.pool.clear();
    throw;
  }
  run(0u);
  for (auto& th : J.pool) th.join();
  J.pool.clear();
  for (auto& e : errs)
    if (e) std::rethrow_exception(e);
}

// body(q) for every q in [0, n) on up to host_threads() threads; a thread takes the next
// index when it is done with one, so starts of unequal cost balance
template <class Body>
void for_each_start(size_t n, Body&& body) {
  const unsigned nt = (unsigned)std::min<size_t>(host_threads(), n);
  std::atomic<size_t> next{0};
  parallel_tasks(nt, [&](unsigned) {
    for (size_t q = next++; q < n; q = next++) body(q);
  });
}

// body(j0, j1) over row ranges of [0, ny) on up to host_threads() threads (at
// least 64 rows each).  Every loop run this way writes only the node it visits
// and reads fields no iteration of the same loop writes, so the split changes no
// value -- the results are those of the reference's single raster loop.
template <class Body>
void parallel_rows(unsigned ny, Body&& body) {
  const unsigned nt = std::max(1u, std::min(host_threads(), ny / 64));
  const unsigned step = (ny + nt - 1) / nt;
  parallel_tasks(nt, [&](unsigned t) {
    const unsigned j0 = t * step, j1 = std::min(ny, j0 + step);
    if (t == 0 || j0 < j1) body(j0, j1);
  });
}

// std::sort over up to host_threads() threads: sorted runs, merged pairwise (the merges
// of a round in parallel).  The elements sorted here are distinct (they hold a cell
// index), so the result is the one std::sort gives.
template <class E>
void parallel_sort(std::vector<E>& v) {
  const uint64_t n = v.size();
  const unsigned nt = std::max(1u, std::min(host_threads(), (unsigned)std::min<uint64_t>(n >> 16, 64)));
  if (nt <= 1) {
    std::sort(v.begin(), v.end());
    return;
  }
  std::vector<uint64_t> b(nt + 1);
  for (unsigned t = 0; t <= nt; ++t) b[t] = n * t / nt;
  parallel_tasks(nt, [&](unsigned t) { std::sort(v.begin() + b[t], v.begin() + b[t + 1]); });
  std::vector<E> tmp(n);
  std::vector<E>*src = &v, *dst = &tmp;
  for (unsigned w = 1; w < nt; w *= 2) {
    const unsigned pairs = (nt + 2 * w - 1) / (2 * w);
    parallel_tasks(pairs, [&](unsigned q) {
      const unsigned lo = q * 2 * w, mid = std::min(lo + w, nt), hi = std::min(lo + 2 * w, nt);
      std::merge(src->begin() + b[lo], src->begin() + b[mid], src->begin() + b[mid],
                 src->begin() + b[hi], dst->begin() + b[lo]);
    });
    std::swap(src, dst);
  }
  if (src != &v) v.swap(*src);
}

}  // namespace

// :145-181, with :186-210 (slope), :217-293 (nominal cost) and :297-308
// (smoothing).  Quirks kept: Q1 smoothing starts from the previous cost; Q2
// locomotion mode 0 skipped when several modes exist; Q3 the neighbour
// "Cmax" loops never run; Q4 LUT indexing differs between range==1 and >1.
bool DyMuPathPlanner::computeCostMap(std::vector<double> cost_data,
                                     std::vector<double> slope_values,
                                     std::vector<std::string> locomotionModes,
                                     std::vector<std::vector<double>> elevation,
                                     std::vector<std::vector<double>> terrainMap) {
  cost_lutable = cost_data;
  slope_range_ = slope_values;
  locomotion_modes_ = locomotionModes;
  if (elevation.size() != ny_ || terrainMap.size() != ny_) return false;
  for (unsigned j = 0; j < ny_; ++j)
    if (elevation[j].size() != nx_ || terrainMap[j].size() != nx_) return false;
  return costMapFromRows([&](unsigned j) { return elevation[j].data(); },
                         [&](unsigned j) { return terrainMap[j].data(); });
}

bool DyMuPathPlanner::computeCostMap(const std::vector<double>& cost_data,
                                     const std::vector<double>& slope_values,
                                     const std::vector<std::string>& locomotionModes,
                                     const double* elevation, const double* terrainMap) {
  cost_lutable = cost_data;
  slope_range_ = slope_values;
  locomotion_modes_ = locomotionModes;
  if (!elevation || !terrainMap) return false;
  const uint64_t nx = nx_;
  return costMapFromRows([=](unsigned j) { return elevation + j * nx; },
                         [=](unsigned j) { return terrainMap + j * nx; });
}

template <class ERows, class TRows>
bool DyMuPathPlanner::costMapFromRows(const ERows& elev_row, const TRows& terr_row) {
  if (cost_lutable.empty() || slope_range_.empty() || locomotion_modes_.empty()) return false;
  const int range = (int)slope_range_.size();
  const int num_locs = (int)locomotion_modes_.size();
  const double cmax = *std::max_element(cost_lutable.begin(), cost_lutable.end());
  parallel_rows(ny_, [&](unsigned j0, unsigned j1) {
    for (unsigned j = j0; j < j1; ++j) {
      const double* e = elev_row(j);
      const double* t = terr_row(j);
      for (unsigned i = 0; i < nx_; ++i) {
        const uint64_t k = idx(i, j);
        raw_cost_[k] = 0;
        elevation_[k] = e[i];
        terrain_[k] = (i == 0 || j == 0 || i == nx_ - 1 || j == ny_ - 1) ? 0u : (uint32_t)t[i];
      }
    }
  });
  // slope reads the elevation only; the nominal cost its own node
  parallel_rows(ny_, [&](unsigned j0, unsigned j1) {
    for (unsigned j = j0; j < j1; ++j)
      for (unsigned i = 0; i < nx_; ++i) {
        calculateSlope(i, j);
        nominalCost(i, j, range, num_locs, cmax);
        const uint64_t k = idx(i, j);
        if (is_obstacle_[k]) {
          traff_[k] = 0.0;
          hazard_[k] = 1.0;
        }
      }
  });
  // smoothing writes cost and reads only raw costs (Q1: its own previous cost)
  parallel_rows(ny_, [&](unsigned j0, unsigned j1) {
    for (unsigned j = j0; j < j1; ++j)
      for (unsigned i = 0; i < nx_; ++i) smoothCost(i, j);
  });
  risk_stale_ = true;
  markDirty(0, ny_);
  return true;
}

// :186-210 (off-grid neighbours: one-sided differences; a 1-wide axis reads
// slope 0 there instead of the reference's NULL dereference)
void DyMuPathPlanner::calculateSlope(unsigned i, unsigned j) {
  if (i >= nx_ || j >= ny_) return;
  const uint64_t k = idx(i, j);
  double dx = 0, dy = 0;
  if (nx_ > 1) {
    if (i == 0)
      dx = (elevation_[k + 1] - elevation_[k]) / global_res_;
    else if (i == nx_ - 1)
      dx = (elevation_[k] - elevation_[k - 1]) / global_res_;
    else
      dx = (elevation_[k + 1] - elevation_[k - 1]) * 0.5 / global_res_;
  }
  if (ny_ > 1) {
    if (j == 0)
      dy = (elevation_[k + nx_] - elevation_[k]) / global_res_;
    else if (j == ny_ - 1)
      dy = (elevation_[k] - elevation_[k - nx_]) / global_res_;
    else
      dy = (elevation_[k + nx_] - elevation_[k - nx_]) * 0.5 / global_res_;
  }
  slope_[k] = std::atan(std::sqrt(dx * dx + dy * dy));
}

// :217-293 (Cmax recomputed per call, as there)
void DyMuPathPlanner::calculateNominalCost(unsigned i, unsigned j, int range, int numLocs) {
  if (i >= nx_ || j >= ny_ || cost_lutable.empty()) return;
  nominalCost(i, j, range, numLocs, *std::max_element(cost_lutable.begin(), cost_lutable.end()));
}

// Q2: locomotion mode 0 is skipped when there are several; Q3: the neighbours'
// "Cmax" loops never run (isObstacle was just set); Q4: range == 1 indexes the
// LUT as terrain * numLocs + m.  A terrain class the LUT does not cover (an
// out-of-bounds read in the reference) makes the cell an obstacle, as the
// device kernel does (cost_kernels.hip).
void DyMuPathPlanner::nominalCost(unsigned i, unsigned j, int range, int num_locs, double cmax) {
  const uint64_t k = idx(i, j);
  const uint32_t t = terrain_[k];
  const size_t nl = cost_lutable.size();
  auto lut = [&](size_t q) { return q < nl ? cost_lutable[q] : cmax; };
  if (t == 0 || (uint64_t)(t + 1) * (uint64_t)range * (uint64_t)num_locs > nl) {
    raw_cost_[k] = cmax;
    is_obstacle_[k] = 1;
  } else if (range == 1) {
    double cdef = lut((size_t)t * num_locs);
    for (int m = 0; m < (int)locomotion_modes_.size(); ++m)
      cdef = std::min(cdef, lut((size_t)t * num_locs + m));
    raw_cost_[k] = std::max(raw_cost_[k], cdef);
  } else {
    const double si = slope_[k] * 180 / M_PI / (slope_range_.back() - slope_range_.front()) *
                      (double)(slope_range_.size() - 1);
    if (si > (double)(slope_range_.size() - 1)) {
      raw_cost_[k] = cmax;
      is_obstacle_[k] = 1;
    } else {
      const double smin = std::floor(si), smax = std::ceil(si);
      double cdef = cmax;
      if (num_locs > 1) {
        for (int m = 1; m < (int)locomotion_modes_.size(); ++m) {
          const double c1 = lut((size_t)t * range * num_locs + (size_t)m * range + (int)smin);
          const double c2 = lut((size_t)t * range * num_locs + (size_t)m * range + (int)smax);
          const double cc = c1 + (c2 - c1) * (si - smin);
          if (cc < cdef) {
            cdef = cc;
            raw_cost_[k] = std::max(raw_cost_[k], cdef);
            loc_mode_[k] = m;
          }
        }
      } else {
        const double c1 = lut((size_t)t * range + (int)smin);
        const double c2 = lut((size_t)t * range + (int)smax);
        cdef = c1 + (c2 - c1) * (si - smin);
        raw_cost_[k] = std::max(raw_cost_[k], cdef);
        loc_mode_[k] = 0;
      }
    }
  }
}

// :297-308 (Q1: starts from the node's previous cost)
void DyMuPathPlanner::smoothCost(unsigned i, unsigned j) {
  if (i >= nx_ || j >= ny_) return;
  const uint64_t k = idx(i, j);
  double csum = cost_[k], n = 5;
  if (j == 0) n--; else csum += raw_cost_[k - nx_];
  if (i == 0) n--; else csum += raw_cost_[k - 1];
  if (i == nx_ - 1) n--; else csum += raw_cost_[k + 1];
  if (j == ny_ - 1) n--; else csum += raw_cost_[k + nx_];
  cost_[k] = csum / n;
}

// :322-357
bool DyMuPathPlanner::setGoal(base::Waypoint wGoal) {
  const double px = (wGoal.position[0] - global_offset_[0]) / global_res_;
  const double py = (wGoal.position[1] - global_offset_[1]) / global_res_;
  if (px < 0 || py < 0) return false;
  const unsigned i = grid_u32(px + 0.5), j = grid_u32(py + 0.5);
  if (i >= nx_ || j >= ny_) return false;
  if (i == 0 || j == 0 || i + 1 >= nx_ || j + 1 >= ny_) return false;  // an nb4 is NULL
  const uint64_t k = idx(i, j);
  if (is_obstacle_[k] || is_obstacle_[k - nx_] || is_obstacle_[k - 1] || is_obstacle_[k + 1] ||
      is_obstacle_[k + nx_])
    return false;
  has_goal_ = true;
  goal_i_ = i;
  goal_j_ = j;
  goal_heading_ = wGoal.heading;
  goals_.clear();
  gs_seeds_.clear();
  invalidateLabels();
  return true;
}

namespace {
// rows of a vs b (ny rows of nx) that differ: [*j0, *j1), empty if none
void diff_rows(const double* a, const double* b, unsigned nx, unsigned ny, unsigned* j0,
               unsigned* j1) {
  *j0 = ny;
  *j1 = 0;
  for (unsigned j = 0; j < ny; ++j)
    if (std::memcmp(a + (uint64_t)j * nx, b + (uint64_t)j * nx, sizeof(double) * nx) != 0) {
      if (*j0 == ny) *j0 = j;
      *j1 = j + 1;
    }
}
}  // namespace

void DyMuPathPlanner::markDirty(unsigned j0, unsigned j1) {
  if (j0 >= j1) return;
  if (dirty_j0_ >= dirty_j1_) {
    dirty_j0_ = j0;
    dirty_j1_ = j1;
  } else {
    dirty_j0_ = std::min(dirty_j0_, j0);
    dirty_j1_ = std::max(dirty_j1_, j1);
  }
}

bool DyMuPathPlanner::setHazardDensity(const std::vector<double>& hd) {
  if (hd.size() != hazard_.size()) return false;
  unsigned j0, j1;
  diff_rows(hd.data(), hazard_.data(), nx_, ny_, &j0, &j1);
  if (j0 < j1) {
    std::memcpy(&hazard_[idx(0, j0)], &hd[idx(0, j0)], sizeof(double) * (uint64_t)(j1 - j0) * nx_);
    markDirty(j0, j1);
  }
  return true;
}

bool DyMuPathPlanner::setTrafficability(const std::vector<double>& tr) {
  if (tr.size() != traff_.size()) return false;
  unsigned j0, j1;
  diff_rows(tr.data(), traff_.data(), nx_, ny_, &j0, &j1);
  if (j0 < j1) {
    std::memcpy(&traff_[idx(0, j0)], &tr[idx(0, j0)], sizeof(double) * (uint64_t)(j1 - j0) * nx_);
    markDirty(j0, j1);
  }
  return true;
}

bool DyMuPathPlanner::setHazardDensityWindow(unsigned i0, unsigned j0, unsigned w, unsigned h,
                                             const double* hd) {
  if (!hd || (uint64_t)i0 + w > nx_ || (uint64_t)j0 + h > ny_) return false;
  for (unsigned r = 0; r < h; ++r)
    std::memcpy(&hazard_[idx(i0, j0 + r)], hd + (uint64_t)r * w, sizeof(double) * w);
  markDirty(j0, j0 + h);
  return true;
}

bool DyMuPathPlanner::setTrafficabilityWindow(unsigned i0, unsigned j0, unsigned w, unsigned h,
                                              const double* tr) {
  if (!tr || (uint64_t)i0 + w > nx_ || (uint64_t)j0 + h > ny_) return false;
  for (unsigned r = 0; r < h; ++r)
    std::memcpy(&traff_[idx(i0, j0 + r)], tr + (uint64_t)r * w, sizeof(double) * w);
  markDirty(j0, j0 + h);
  return true;
}

// ---- the device-resident map ----

void DyMuPathPlanner::ensureEngine() {
  const uint64_t n = (uint64_t)nx_ * ny_;
  if (!ctx_) {
    const int rc = dymu_create(&ctx_, &opts_);
    if (rc != DYMU_OK) {
      ctx_ = nullptr;
      throw std::runtime_error(std::string("dymu: cannot create the HIP engine: ") +
                               dymu_strerror(rc));
    }
    solved_ = false, gs_seeds_.clear();
    speed_valid_ = false;
  }
  if (dcells_ != n) {
    if (dF_) (void)dymu_device_free(ctx_, dF_);
    if (dT_) (void)dymu_device_free(ctx_, dT_);
    dF_ = dT_ = nullptr;
    dropLabels();
    dropBatch();
    dropCombined();
    dropRiskMaps();
    dcells_ = 0;
    dev_map_current_ = false;
    void *f = nullptr, *t = nullptr;
    if (dymu_device_alloc(ctx_, sizeof(double) * n, &f) != DYMU_OK ||
        dymu_device_alloc(ctx_, sizeof(double) * n, &t) != DYMU_OK) {
      if (f) (void)dymu_device_free(ctx_, f);
      throw std::runtime_error("dymu: cannot allocate the device map");
    }
    dF_ = static_cast<double*>(f);
    dT_ = static_cast<double*>(t);
    dcells_ = n;
    solved_ = false, gs_seeds_.clear();
    speed_valid_ = false;
    // page-lock the host mirror for full-rate downloads (optional: pageable works)
    if (registered_) (void)dymu_host_unregister(ctx_, registered_);
    registered_ = nullptr;
    if (dymu_host_register(ctx_, total_cost_.data(), sizeof(double) * n) == DYMU_OK)
      registered_ = total_cost_.data();
  }
  if (!speed_valid_) {
    speed_.assign(n, 0.0);
    markDirty(0, ny_);
  }
}

// F = global_res * cost * (2 + hazard - traff) (:527-528), +inf for obstacles,
// re-packed for the dirty rows; the rows whose F changed are uploaded.
bool DyMuPathPlanner::syncSpeed(unsigned& i0, unsigned& i1, unsigned& j0, unsigned& j1) {
  syncGlobalRisk();
  i0 = nx_;
  i1 = 0;
  j0 = ny_;
  j1 = 0;
  decrease_only_ = speed_valid_;
  if (dirty_j0_ >= dirty_j1_ && speed_valid_) return false;
  const unsigned d0 = speed_valid_ ? dirty_j0_ : 0, d1 = speed_valid_ ? dirty_j1_ : ny_;
  row_.resize(nx_);
  for (unsigned j = d0; j < d1; ++j) {
    const uint64_t k0 = idx(0, j);
    for (unsigned i = 0; i < nx_; ++i) {
      const uint64_t k = k0 + i;
      row_[i] = is_obstacle_[k] ? kInf : nodeSpeed(k);
    }
    double* old = &speed_[k0];
    if (speed_valid_ && std::memcmp(row_.data(), old, sizeof(double) * nx_) == 0) continue;
    unsigned a = 0, b = nx_;
    if (speed_valid_) {
      while (std::memcmp(&row_[a], old + a, sizeof(double)) == 0) ++a;
      while (std::memcmp(&row_[b - 1], old + b - 1, sizeof(double)) == 0) --b;
      for (unsigned i = a; i < b && decrease_only_; ++i)
        if (!(row_[i] <= old[i])) decrease_only_ = false;
    }
    std::memcpy(old, row_.data(), sizeof(double) * nx_);
    i0 = std::min(i0, a);
    i1 = std::max(i1, b);
    if (j0 == ny_) j0 = j;
    j1 = j + 1;
  }
  dirty_j0_ = dirty_j1_ = 0;
  if (!speed_valid_) {
    i0 = 0, i1 = nx_, j0 = 0, j1 = ny_;
  }
  speed_valid_ = true;
  if (j0 >= j1) return false;
  const int rc = dymu_memcpy_h2d(ctx_, dF_ + idx(0, j0), &speed_[idx(0, j0)],
                                 sizeof(double) * (uint64_t)(j1 - j0) * nx_);
  if (rc != DYMU_OK) {
    speed_valid_ = false;
    throw std::runtime_error(std::string("dymu: speed upload failed: ") + dymu_last_error(ctx_));
  }
  return true;
}

// ---- obstacle clearance for the global plan ----
#pragma weak dymu_clearance_device

bool DyMuPathPlanner::setGlobalRisk(double risk_distance, double risk_ratio) {
  if (!(risk_distance >= 0) || !(risk_ratio >= 0) || !(risk_distance < kInf) ||
      !(risk_ratio < kInf))
    return false;
  const bool on = risk_distance > 0 && risk_ratio > 0;
  if (on) {  // computeTotalCostMaps' rule: no device engine, no change
    if (!&dymu_clearance_device) return false;
    try {
      ensureEngine();
    } catch (const std::exception&) {
      return false;
    }
  }
  if (risk_distance == grisk_distance_ && risk_ratio == grisk_ratio_) return true;
  const bool was_on = globalRiskOn();
  grisk_distance_ = risk_distance;
  grisk_ratio_ = risk_ratio;
  if (on) {
    global_risk_.assign((uint64_t)nx_ * ny_, 0.0);
    risk_stale_ = true;
  } else {
    std::vector<double>().swap(global_risk_);
    dropRiskMaps();
  }
  if (on || was_on) markDirty(0, ny_);
  return true;
}

void DyMuPathPlanner::dropRiskMaps() {
  for (double** p : {&dMask_, &dW_, &dS_}) {
    if (*p && ctx_) (void)dymu_device_free(ctx_, *p);
    *p = nullptr;
  }
  risk_dev_valid_ = false;
  if (risk_pend_) risk_stale_ = true;  // the field the pending box would update is gone
  risk_pend_ = risk_pend_freed_ = false;
}

void DyMuPathPlanner::refreshGlobalRisk() {
  ensureEngine();
  const uint64_t n = (uint64_t)nx_ * ny_;
  risk_pend_ = risk_pend_freed_ = false;  // the whole recompute sees every obstacle
  if (n == 0) {
    risk_stale_ = false;
    return;
  }
  // the raw speed, through R's own buffer, into the mask map: the obstacle mask the
  // seeding kernel reads.  dF_ is not touched: it stays the upload of speed_, the speed
  // the solved maps belong to and the next diff is taken against
  global_risk_.resize(n);
  for (uint64_t k = 0; k < n; ++k) global_risk_[k] = rawSpeed(k);
  risk_dev_valid_ = false;
  int rc = DYMU_OK;
  for (double** p : {&dMask_, &dW_, &dS_}) {
    void* q = *p;
    if (!q && rc == DYMU_OK) rc = dymu_device_alloc(ctx_, sizeof(double) * n, &q);
    *p = static_cast<double*>(q);
  }
  if (rc == DYMU_OK) rc = dymu_memcpy_h2d(ctx_, dMask_, global_risk_.data(), sizeof(double) * n);
  dymu_stats st{};
  if (rc == DYMU_OK)
    rc = dymu_clearance_device(ctx_, dMask_, dW_, dS_, nx_, ny_, nx_,
                               global_res_ / grisk_distance_, nullptr, &st);
  if (rc == DYMU_OK) rc = dymu_memcpy_d2h(ctx_, global_risk_.data(), dS_, sizeof(double) * n);
  if (rc != DYMU_OK) {  // still stale: the next synchronisation tries again
    const std::string err = dymu_last_error(ctx_);
    std::fill(global_risk_.begin(), global_risk_.end(), 0.0);
    throw std::runtime_error(std::string("dymu: global risk: ") + dymu_strerror(rc) + " " + err);
  }
  for (uint64_t k = 0; k < n; ++k) global_risk_[k] = std::fmax(1.0 - global_risk_[k], 0.0);
  risk_stale_ = false;
  risk_dev_valid_ = true;
  risk_update_kind_ = 1;
  std::fill(risk_raise_, risk_raise_ + 4, 0ull);
  risk_stats_ = st;
  risk_box_[0] = risk_box_[1] = 0, risk_box_[2] = nx_, risk_box_[3] = ny_;
  markDirty(0, ny_);
}

// R after setCostMapWindow added obstacles inside the pending box, R being current but for
// them: the box's rows of the raw speed into the mask map, the field re-propagated from the new
// cells (dymu_clearance_update_device), and the box the engine reports -- no cell of the
// field outside it moved -- downloaded, turned into R and re-packed.  Whatever the engine
// refuses (a freed cell it finds itself, an error) leaves the whole recompute.  A pending box
// that freed obstacles (trackObstacleRemoval) goes through dymu_clearance_edit_device
// instead, which raises the field where the freed cells supported it first: R can fall as
// well as rise inside the reported box, which the row diff of syncSpeed sees by itself.
void DyMuPathPlanner::updateGlobalRisk() {
  ensureEngine();  // a new grid or engine drops the maps and turns the box into risk_stale_
  const bool edit = risk_pend_freed_;
  if (risk_stale_ || !risk_pend_ || !risk_dev_valid_ || !&dymu_clearance_update_device ||
      (edit && !&dymu_clearance_edit_device)) {
    risk_stale_ = true;
    refreshGlobalRisk();
    return;
  }
  risk_pend_ = risk_pend_freed_ = false;
  const unsigned i0 = rpend_i0_, j0 = rpend_j0_, w = rpend_i1_ - i0, h = rpend_j1_ - j0;
  // whole rows, one contiguous copy: outside the box they differ from the mask map in
  // finite values at most, and the engine reads the window's cells only
  std::vector<double> raw((uint64_t)nx_ * h);
  for (uint64_t k = 0; k < raw.size(); ++k) raw[k] = rawSpeed(idx(0, j0) + k);
  int rc = dymu_memcpy_h2d(ctx_, dMask_ + idx(0, j0), raw.data(), sizeof(double) * raw.size());
  uint32_t box[4] = {0, 0, 0, 0};
  dymu_stats st{};
  if (rc == DYMU_OK)
    rc = (edit ? dymu_clearance_edit_device : dymu_clearance_update_device)(
        ctx_, dMask_, dW_, dS_, nx_, ny_, nx_, global_res_ / grisk_distance_, i0, j0, w, h, nullptr,
        box, &st);
  if (rc == DYMU_OK && box[2] && box[3]) {
    const uint64_t o = idx(box[0], box[1]);
    rc = dymu_memcpy2d_d2h(ctx_, &global_risk_[o], sizeof(double) * nx_, dS_ + o,
                           sizeof(double) * nx_, sizeof(double) * box[2], box[3]);
    if (rc != DYMU_OK) {  // R's box holds a partial download
      risk_dev_valid_ = false;
    } else {
      for (unsigned r = 0; r < box[3]; ++r) {
        double* g = &global_risk_[idx(box[0], box[1] + r)];
        for (unsigned q = 0; q < box[2]; ++q) g[q] = std::fmax(1.0 - g[q], 0.0);
      }
      markDirty(box[1], box[1] + box[3]);
    }
  }
  if (rc != DYMU_OK) {
    risk_stale_ = true;
    refreshGlobalRisk();
    return;
  }
  risk_update_kind_ = edit ? 3 : 2;
  std::fill(risk_raise_, risk_raise_ + 4, 0ull);
  if (edit && &dymu_last_update_stats) (void)dymu_last_update_stats(ctx_, risk_raise_);
  risk_stats_ = st;
  std::copy(box, box + 4, risk_box_);
}

std::vector<std::vector<double>> DyMuPathPlanner::getGlobalRiskMatrix() {
  std::vector<std::vector<double>> m(ny_, std::vector<double>(nx_, 0.0));
  if (!globalRiskOn()) return m;
  syncGlobalRisk();
  for (unsigned j = 0; j < ny_; ++j)
    for (unsigned i = 0; i < nx_; ++i) m[j][i] = global_risk_[idx(i, j)];
  return m;
}

// Thread-safe (the band replay's threads read through it): a block's flag is read
// with acquire and set with release after its download, downloads one at a time.
double DyMuPathPlanner::T(uint64_t k) const {
  if (__atomic_load_n(&blk_missing_, __ATOMIC_ACQUIRE)) {
    const unsigned j = (unsigned)(k / nx_), i = (unsigned)(k % nx_);
    const uint64_t b = (uint64_t)(j / kBlk) * nbx_ + i / kBlk;
    if (!__atomic_load_n(&blk_ok_[b], __ATOMIC_ACQUIRE)) {
      std::lock_guard<std::mutex> lock(fetch_mu_);
      if (!__atomic_load_n(&blk_ok_[b], __ATOMIC_RELAXED)) {
        const unsigned bi = (i / kBlk) * kBlk, bj = (j / kBlk) * kBlk;
        const unsigned w = std::min(kBlk, nx_ - bi), h = std::min(kBlk, ny_ - bj);
        const uint64_t o = idx(bi, bj);
        if (dymu_memcpy2d_d2h(ctx_, &total_cost_[o], sizeof(double) * nx_, dT_ + o,
                              sizeof(double) * nx_, sizeof(double) * w, h) != DYMU_OK)
          throw std::runtime_error(std::string("dymu: total-cost download failed: ") +
                                   dymu_last_error(ctx_));
        __atomic_store_n(&blk_ok_[b], (uint8_t)1, __ATOMIC_RELEASE);
        __atomic_sub_fetch(&blk_missing_, 1, __ATOMIC_RELEASE);
      }
    }
  }
  return total_cost_[k];
}

void DyMuPathPlanner::fetchAll() const {
  if (!blk_missing_) return;
  if (dymu_memcpy_d2h(ctx_, total_cost_.data(), dT_, sizeof(double) * dcells_) != DYMU_OK)
    throw std::runtime_error(std::string("dymu: total-cost download failed: ") +
                             dymu_last_error(ctx_));
  std::fill(blk_ok_.begin(), blk_ok_.end(), 1);
  blk_missing_ = 0;
}

const double* DyMuPathPlanner::totalCostData() const {
  fetchAll();
  return total_cost_.data();
}

// One pass over the host mirror split in row ranges: at 16384^2 a single-thread
// copy into a caller's fresh buffer (first-touch faults on 2 GiB) costs several
// times the solve itself.
// A stale mirror is downloaded in row chunks and each chunk is handed on while
// the next one downloads.
template <class Body>
void DyMuPathPlanner::streamTotalCost(Body&& body) const {
  constexpr unsigned kChunks = 16;
  if (!blk_missing_ || ny_ < 64 * kChunks) {
    fetchAll();
    body(0u, ny_);
    return;
  }
  const unsigned step = (ny_ + kChunks - 1) / kChunks;
  // the return code is the failure flag (some failures leave no error text)
  int rc = DYMU_OK;
  std::exception_ptr body_err;
  struct Joiner {
    std::thread th;
    ~Joiner() {
      if (th.joinable()) th.join();
    }
  } worker;
  // body_err is written by the worker thread: it is read only after that thread's
  // join (the join is the synchronisation), never while the worker may still run
  for (unsigned r0 = 0; r0 < ny_ && rc == DYMU_OK; r0 += step) {
    const unsigned r1 = std::min(ny_, r0 + step);
    const uint64_t o = idx(0, r0);
    rc = dymu_memcpy_d2h(ctx_, &total_cost_[o], dT_ + o, sizeof(double) * (idx(0, r1) - o));
    if (worker.th.joinable()) worker.th.join();
    if (body_err) break;
    if (rc == DYMU_OK)
      worker.th = std::thread([&body, &body_err, r0, r1] {
        try {
          body(r0, r1);
        } catch (...) {
          body_err = std::current_exception();
        }
      });
  }
  if (worker.th.joinable()) worker.th.join();
  if (rc != DYMU_OK) {
    const char* msg = ctx_ ? dymu_last_error(ctx_) : "";
    throw std::runtime_error(std::string("dymu: total-cost download failed: ") +
                             (msg && *msg ? msg : dymu_strerror(rc)));
  }
  if (body_err) std::rethrow_exception(body_err);
  std::fill(blk_ok_.begin(), blk_ok_.end(), 1);
  blk_missing_ = 0;
}

void DyMuPathPlanner::copyTotalCost(double* out, bool raw) const {
  const double* t = total_cost_.data();
  streamTotalCost([&](unsigned r0, unsigned r1) {
    parallel_rows(r1 - r0, [&](unsigned j0, unsigned j1) {
      const uint64_t a = idx(0, r0 + j0), b = idx(0, r0 + j1);
      if (raw) {
        std::memcpy(out + a, t + a, sizeof(double) * (b - a));
      } else {
        for (uint64_t k = a; k < b; ++k) out[k] = t[k] == kInf ? -1.0 : t[k];
      }
    });
  });
}

bool DyMuPathPlanner::closedCell(uint64_t k) const {
  if (!node_state_.empty()) return node_state_[k] != 0;
  const double t = T(k);
  if (!(t < kInf) || t > closed_limit_) return false;
  return t < closed_limit_ || open_at_limit_.empty() ||
         !std::binary_search(open_at_limit_.begin(), open_at_limit_.end(), k);
}

// One propagation on the engine.  early = computeTotalCostMap (:364-408): stop
// once (si, sj) and its nb4 are final, then rebuild the reference's node states
// (CLOSED / band / never reached) and the band's tentative values.  Otherwise
// computeEntireTotalCostMap (:443-468), incremental where possible: when dT_
// holds the converged map of the same grid and goal and the speed changed only
// inside a window (the local layer's hazard / trafficability writes), the engine
// re-propagates from that window (dymu_update_window_device; without any reset
// when every changed speed went down); unchanged speed
// reuses the map.  Both give the cold solve's fixed point.
// Returns false iff the early exit left an empty band (the reference's "goal
// unreachable" return, :399-403).
bool DyMuPathPlanner::propagate(bool early, unsigned si, unsigned sj) {
  ensureEngine();
  unsigned i0, i1, j0, j1;
  bool changed = syncSpeed(i0, i1, j0, j1);
  if (changed) batchSpeedChanged(i0, i1, j0, j1);  // its maps are those of the old speed
  if (pend_) {  // a change a batch solve synchronised: dT_ has not seen it yet
    i0 = std::min(i0, pend_i0_), i1 = std::max(i1, pend_i1_);
    j0 = std::min(j0, pend_j0_), j1 = std::max(j1, pend_j1_);
    decrease_only_ = decrease_only_ && pend_dec_;
    changed = true;
    pend_ = false;
  }
  const uint64_t n = (uint64_t)nx_ * ny_;
  int rc = DYMU_ERR_STATE;
  if (!early && solved_ && solved_gi_ == goal_i_ && solved_gj_ == goal_j_) {
    if (!changed) {
      incremental_ = 2;
      return true;
    }
    if ((uint64_t)(i1 - i0) * (j1 - j0) * 4 <= n) {
      rc = dymu_update_window_device(ctx_, dF_, dT_, nx_, ny_, nx_, goal_i_, goal_j_, i0, j0,
                                     i1 - i0, j1 - j0, decrease_only_ ? 1 : 0, nullptr, &stats_);
      if (rc == DYMU_OK) incremental_ = 1;
    }
  }
  double t_closed = kInf;
  dev_map_current_ = false;  // until the engine call below succeeds
  invalidateLabels();
  if (rc != DYMU_OK) {
    solved_ = false, gs_seeds_.clear();
    rc = early ? dymu_solve_until_device(ctx_, dF_, dT_, nx_, ny_, nx_, goal_i_, goal_j_, si, sj,
                                         nullptr, &t_closed, &stats_)
               : dymu_solve_device(ctx_, dF_, dT_, nx_, ny_, nx_, goal_i_, goal_j_, nullptr,
                                   &stats_);
    if (rc != DYMU_OK)
      throw std::runtime_error(std::string("dymu solve failed: ") + dymu_strerror(rc) + " " +
                               dymu_last_error(ctx_));
    incremental_ = 0;
  }
  // the host mirror is stale (its blocks are fetched from dT_ on first read); node
  // states and the propagated list follow the new map
  dev_map_current_ = true;
  std::fill(blk_ok_.begin(), blk_ok_.end(), 0);
  blk_missing_ = blk_ok_.size();
  band_cells_.clear();
  band_unordered_ = false;
  band_values_checked_ = true;
  open_at_limit_.clear();
  node_state_.clear();
  propagated_extra_.clear();
  manual_list_ = false;
  early_info_ = EarlyExitInfo{};
  if (!early) {
    closed_limit_ = kInf;
    solved_ = true;
    solved_gi_ = goal_i_;
    solved_gj_ = goal_j_;
    return true;
  }
  // early exit: the reference's CLOSED set is {T <= t_closed}; the band gets its
  // tentative values; every other cell +inf.  dT_ is no longer a converged map.
  solved_ = false, gs_seeds_.clear();
  closed_limit_ = t_closed;
  const auto t0 = std::chrono::steady_clock::now();
  const uint64_t g = idx(goal_i_, goal_j_), s = idx(si, sj);
  // The region the exit is decided on: the cells of T <= t_closed (a margin far above
  // the engine's error) and their band, one cell around; and the near-tie guard over it
  // (pop_order.hpp): the engine's values order cells as the reference's do only where
  // no rounding can flip the order
  dymu_region reg{};
  reg.i0 = 1;
  reg.i1 = 0;
  const double thr = t_closed < kInf ? t_closed * (1 + kRegionMargin) : kInf;
  if (dymu_region_stats(ctx_, dF_, dT_, nx_, ny_, nx_, goal_i_, goal_j_, thr,
                        t_closed * (1 - kTieEps), t_closed * (1 + kTieEps), &reg,
                        nullptr) != DYMU_OK)
    throw std::runtime_error(std::string("dymu_region_stats failed: ") + dymu_last_error(ctx_));
  int64_t box[4] = {0, 0, -1, -1};  // inclusive; empty when nothing was reached
  if (reg.i0 <= reg.i1) {
    box[0] = reg.i0 > 0 ? reg.i0 - 1 : 0;
    box[1] = reg.j0 > 0 ? reg.j0 - 1 : 0;
    box[2] = std::min<int64_t>((int64_t)reg.i1 + 1, nx_ - 1);
    box[3] = std::min<int64_t>((int64_t)reg.j1 + 1, ny_ - 1);
  }
  TieGuard guard(nx_, goal_i_, goal_j_, speed_[g], reg.r_const);
  have_start_ = true;  // for insertionOrder's / minCostGlobalNode's exact fallback
  exit_r_const_ = reg.r_const;
  start_i_ = si;
  start_j_ = sj;
  std::copy(box, box + 4, exit_box_);
  std::vector<uint64_t> band(std::max<uint64_t>(4096, 4 * (uint64_t)(nx_ + ny_)));
  uint64_t nb = 0;
  for (;;) {
    rc = dymu_early_exit_mask(ctx_, dF_, dT_, nx_, ny_, nx_, t_closed, band.data(), band.size(),
                              &nb, nullptr);
    if (rc != DYMU_OK)
      throw std::runtime_error(std::string("dymu_early_exit_mask failed: ") +
                               dymu_last_error(ctx_));
    if (nb <= band.size()) break;
    band.resize(nb);
  }
  band.resize(nb);
  std::sort(band.begin(), band.end());
  PopOrder<MapT> po(MapT{this}, nx_, ny_, g, &guard);
  // the exit moment: the last of the start and its nb4 the reference pops (all five
  // CLOSED; the latest has the largest value, t_closed)
  const uint64_t probes[5] = {s, s - nx_, s - 1, s + 1, s + nx_};
  uint64_t last = s;
  for (int q = 1; q < 5; ++q)
    if (po.popBefore(last, probes[q])) last = probes[q];
  // Cells of exactly t_closed: the reference pops them in insertion order and stops
  // right after `last`, so those it pops later stay in the band (with their value).
  // Resolve which, from the values (pop_order.hpp).  An engine tie with the exit value
  // is the reference's only as a mirror image of a probe of that value; a cell the
  // engine puts within eps of it, but not on it, is a near tie.
  if (t_closed < kInf) {
    std::vector<uint64_t> eq(256);
    uint64_t n_eq = 0;
    for (;;) {
      if (dymu_find_equal(ctx_, dT_, nx_, ny_, nx_, t_closed, eq.data(), eq.size(), &n_eq,
                          nullptr) != DYMU_OK)
        throw std::runtime_error(std::string("dymu_find_equal failed: ") + dymu_last_error(ctx_));
      if (n_eq <= eq.size()) break;
      eq.resize(n_eq);
    }
    eq.resize(n_eq);
    early_info_.tied = n_eq;
    for (const uint64_t x : eq) {
      bool trusted = false;
      for (const uint64_t q : probes)
        trusted = trusted || (T(q) == t_closed && (q == x || guard.mirror(x, q)));
      if (!trusted) ++guard.near;
    }
    guard.near += reg.n_range > n_eq ? reg.n_range - n_eq : 0;
    if (n_eq > 1) {
      for (const uint64_t x : eq)
        if (x != last && po.popBefore(last, x)) open_at_limit_.push_back(x);
      std::sort(open_at_limit_.begin(), open_at_limit_.end());
    }
  }
  const double ms_order =
      std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  // an undetermined or near-tied order: the exact host replay decides the exit
  // (DYMU_EXACT_EXIT=1 forces it: measurement and tests of that path)
  static const bool force_exact = [] {
    const char* kv = std::getenv("DYMU_EXACT_EXIT");
    return kv && std::atoi(kv) != 0;
  }();
  bool exact = po.degenerate() || guard.near > 0 || force_exact;
  // the band with the cells the reference left OPEN at t_closed: they join it, and
  // a neighbour of theirs stays in it only if it has another CLOSED neighbour
  // (otherwise it was never reached: +inf)
  std::vector<uint64_t> unreached;
  if (!exact && !open_at_limit_.empty()) {
    std::vector<uint64_t> add(open_at_limit_);
    for (const uint64_t x : open_at_limit_) {
      const unsigned i = (unsigned)(x % nx_), j = (unsigned)(x / nx_);
      const int64_t nb4[4][2] = {{i, (int64_t)j - 1}, {(int64_t)i - 1, j}, {i + 1, j}, {i, j + 1}};
      for (const auto& q : nb4) {
        if (q[0] < 0 || q[1] < 0 || q[0] >= nx_ || q[1] >= ny_) continue;
        const uint64_t y = idx((unsigned)q[0], (unsigned)q[1]);
        if (!std::binary_search(band.begin(), band.end(), y) || T(y) <= t_closed) continue;
        bool reached = false;
        const unsigned yi = (unsigned)q[0], yj = (unsigned)q[1];
        if (yj > 0) reached |= closedCell(y - nx_);
        if (yi > 0) reached |= closedCell(y - 1);
        if (yi + 1 < nx_) reached |= closedCell(y + 1);
        if (yj + 1 < ny_) reached |= closedCell(y + nx_);
        if (!reached) unreached.push_back(y);
      }
    }
    std::sort(unreached.begin(), unreached.end());
    unreached.erase(std::unique(unreached.begin(), unreached.end()), unreached.end());
    std::vector<uint64_t> kept;
    kept.reserve(band.size() + add.size());
    for (const uint64_t y : band)
      if (!std::binary_search(unreached.begin(), unreached.end(), y)) kept.push_back(y);
    kept.insert(kept.end(), add.begin(), add.end());
    std::sort(kept.begin(), kept.end());
    band.swap(kept);
    nb = band.size();
  }
  std::vector<double> vals;
  if (nb && !exact) {
    exact = replayBand(last, band, vals, guard);
  }
  early_info_.near_ties = guard.near;
  early_info_.open_at_limit = open_at_limit_.size();
  if (exact) {
    // the reference replayed exactly on the host over the region (no size limit)
    early_info_.exact_replay = 1;
    if (std::getenv("DYMU_ORDER_DEBUG"))
      std::fprintf(stderr,
                   "[dymu] exact exit: near ties %llu (first (%llu,%llu) %.17g vs (%llu,%llu) "
                   "%.17g; mirror below %.17g), degenerate %d (reason %d)\n",
                   (unsigned long long)guard.near, (unsigned long long)(guard.first[0] % nx_),
                   (unsigned long long)(guard.first[0] / nx_), guard.first_t[0],
                   (unsigned long long)(guard.first[1] % nx_),
                   (unsigned long long)(guard.first[1] / nx_), guard.first_t[1],
                   guard.trust_below, (int)po.degenerate(), po.why());
    const bool r = exactEarlyExit(si, sj, box);
    early_info_.resolve_ms =
        std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return r;
  }
  if (!unreached.empty()) {
    const std::vector<double> inf(unreached.size(), kInf);
    if (dymu_scatter(ctx_, dT_, nx_, nx_, unreached.data(), inf.data(), unreached.size(),
                     nullptr) != DYMU_OK)
      throw std::runtime_error(std::string("dymu_scatter failed: ") + dymu_last_error(ctx_));
    for (const uint64_t y : unreached) {
      (void)T(y);
      total_cost_[y] = kInf;
    }
  }
  if (nb) {
    rc = dymu_scatter(ctx_, dT_, nx_, nx_, band.data(), vals.data(), nb, nullptr);
    if (rc != DYMU_OK)
      throw std::runtime_error(std::string("dymu_scatter failed: ") + dymu_last_error(ctx_));
    // blocks fetched during the replay hold the pre-replay band values
    for (uint64_t q = 0; q < nb; ++q) {
      (void)T(band[q]);
      total_cost_[band[q]] = vals[q];
    }
  }
  early_info_.resolve_ms =
      std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (std::getenv("DYMU_ORDER_DEBUG"))
    std::fprintf(stderr, "[dymu] early exit: t_closed %.17g band %llu tied %llu open %llu, "
                 "%.1f ms order + %.1f ms band on %u threads\n", t_closed,
                 (unsigned long long)nb, (unsigned long long)early_info_.tied,
                 (unsigned long long)open_at_limit_.size(), ms_order,
                 early_info_.resolve_ms - ms_order, early_info_.replay_threads);
  band_cells_ = std::move(band);
  band_unordered_ = band_cells_.size() > 1;
  band_values_checked_ = false;  // minCostGlobalNode checks them for near ties first
  return nb > 0;
}

// The reference's tentative band values at its early exit, from the CLOSED
// values.  A pop of node m updates its OPEN nb4 x from the values x's neighbours
// hold at that moment (:462-465, :500-546), so with "moment c" = just after the pop
// of node c:
//   val(x, c) = min over nb4 m of x CLOSED by moment c of cand(x, m),
// where cand(x, m) is the update with each neighbour n of x at its value at moment
// m: T(n) if n is CLOSED by then (popped no later than m, in the reference's pop
// order -- pop_order.hpp -- which decides ties), else val(n, m).  The band values at
// the exit are val(x, last), last = the last of the start and its nb4 popped.  An
// OPEN value at moment m is >= T(m) >= any CLOSED value then (the FMM invariant), so
// an axis with a CLOSED side takes that side and the recursion only follows axes
// whose two sides are OPEN -- cells next to the front, at strictly earlier pops (x's
// neighbours are not adjacent to each other).
// The band cells are independent given the CLOSED values: host threads take
// contiguous runs of them, each with its own memo and order cache (a walk back stays
// near its band cell, so little work is repeated across threads).  Every comparison
// of two cells' values goes through a copy of the guard; their near ties are summed
// into `guard`.  Returns true when the values are not to be used: the pop order was
// undetermined or near-tied, or a replay hit its work bound -- the caller then
// replays the reference exactly.
bool DyMuPathPlanner::replayBand(uint64_t last, const std::vector<uint64_t>& band,
                                 std::vector<double>& out, TieGuard& guard) {
  using Order = PopOrder<MapT>;
  // open-addressing map uint64 -> double, keys != 0
  struct Memo {
    std::vector<uint64_t> key;
    std::vector<double> v;
    uint64_t n = 0, mask = 0;
    Memo() : key(1u << 12, 0), v(1u << 12), mask((1u << 12) - 1) {}
    static uint64_t h(uint64_t x) { return (x * 0x9E3779B97F4A7C15ull) >> 17; }
    double* find(uint64_t k) {
      for (uint64_t q = h(k) & mask;; q = (q + 1) & mask) {
        if (key[q] == k) return &v[q];
        if (key[q] == 0) return nullptr;
      }
    }
    void put(uint64_t k, double x) {
      if (2 * (n + 1) > key.size()) grow();
      uint64_t q = h(k) & mask;
      while (key[q] != 0 && key[q] != k) q = (q + 1) & mask;
      if (key[q] == 0) ++n;
      key[q] = k;
      v[q] = x;
    }
    void grow() {
      std::vector<uint64_t> ok(key.size() * 2, 0);
      std::vector<double> ov(key.size() * 2);
      ok.swap(key);
      ov.swap(v);
      mask = key.size() - 1;
      n = 0;
      for (size_t q = 0; q < ok.size(); ++q)
        if (ok[q]) put(ok[q], ov[q]);
    }
  };
  struct Replay {
    DyMuPathPlanner& pl;
    TieGuard guard;                // this thread's copy (near ties counted here)
    Order po;
    const double* F;
    int64_t NX, NY;
    uint64_t last;                 // the exit moment
    double lim;                    // closed_limit_ (T(last))
    const std::vector<uint64_t>& open;  // open_at_limit_
    uint64_t budget;               // upd evaluations left before giving up
    Memo memo;                     // upd(k, s), keyed k * 4 + s + 1
    Memo bmemo;                    // band values at the exit, keyed k + 1
    uint64_t band_k = ~0ull;       // the band cell being evaluated at the exit
    bool overrun = false;          // the budget or the depth bound was hit

    Replay(DyMuPathPlanner& p, const TieGuard& g, uint64_t gl, uint64_t lst, uint64_t b)
        : pl(p), guard(g), po(MapT{&p}, p.nx_, p.ny_, gl, &guard),
          F(p.speed_.data()), NX(p.nx_), NY(p.ny_), last(lst), lim(p.closed_limit_),
          open(p.open_at_limit_), budget(b) {
      guard.near = 0;
    }
    bool in_grid(int64_t i, int64_t j) const { return i >= 0 && j >= 0 && i < NX && j < NY; }
    double tv(int64_t i, int64_t j) const { return pl.T((uint64_t)(j * NX + i)); }
    // closedCell with T already loaded (node_state_ is empty here: propagate cleared it)
    bool closed(uint64_t k, double t) {
      if (!(t < kInf)) return false;
      const int c = guard.cmp(k, t, last, lim);
      if (c != 0) return c < 0;
      return open.empty() || !std::binary_search(open.begin(), open.end(), k);
    }
    // value of (i, j) if it is CLOSED by moment c (value tc), else +inf
    double closed_by(int64_t i, int64_t j, uint64_t c, double tc) {
      if (!in_grid(i, j)) return kInf;
      const uint64_t k = (uint64_t)(j * NX + i);
      const double t = tv(i, j);
      if (!closed(k, t)) return kInf;
      if (k == c) return t;
      const int r = guard.cmp(k, t, c, tc);
      if (r != 0) return r < 0 ? t : kInf;
      return po.popBefore(k, c) ? t : kInf;
    }
    // the reference update (:504-535), -ffp-contract=off
    static double eikonal(double tx, double ty, double C) {
      if ((std::fabs(tx - ty) < C) && (tx < kInf) && (ty < kInf))
        return (tx + ty + std::sqrt(2 * (C * C) - (tx - ty) * (tx - ty))) / 2;
      return std::fmin(tx, ty) + C;
    }
    double axis(int64_t ia, int64_t ja, int64_t ib, int64_t jb, uint64_t m, double tm,
                int depth) {
      const double a = closed_by(ia, ja, m, tm), b = closed_by(ib, jb, m, tm);
      if (a < kInf || b < kInf) return std::fmin(a, b);  // OPEN sides are >= T(m) >= it
      const double va = in_grid(ia, ja) ? val(ia, ja, m, tm, depth + 1) : kInf;
      const double vb = in_grid(ib, jb) ? val(ib, jb, m, tm, depth + 1) : kInf;
      return std::fmin(va, vb);
    }
    // val(k, c) = min over the nb4 m of k popped by moment c of upd(k, m): the update
    // of k by m's pop depends on m alone, so it is memoised per (k, m) -- at most four
    // per cell -- and a value at any moment is a min over at most four of them.  When
    // every neighbour that updates k before k's own pop (a CLOSED k) or before the exit
    // (a band k) has been popped by c, the value at c is that final one: T(k), or k's
    // band value -- which cuts the walk back through the front's history short
    double val(int64_t i, int64_t j, uint64_t c, double tc, int depth) {
      const uint64_t k = (uint64_t)(j * NX + i);
      if (!(F[k] < kInf)) return kInf;  // obstacles are never updated
      const int64_t nb[4][2] = {{i, j - 1}, {i - 1, j}, {i + 1, j}, {i, j + 1}};
      const double tk = tv(i, j);
      const bool kc = closed(k, tk);
      bool all = true;
      double byc[4];
      for (int s = 0; s < 4; ++s) {
        byc[s] = closed_by(nb[s][0], nb[s][1], c, tc);
        if (byc[s] < kInf || !all || !in_grid(nb[s][0], nb[s][1])) continue;
        // a neighbour not popped by c: does it update k before k's value is final?
        const uint64_t n = (uint64_t)(nb[s][1] * NX + nb[s][0]);
        if (kc ? n != k && closed_by(nb[s][0], nb[s][1], k, tk) < kInf
               : closed(n, tv(nb[s][0], nb[s][1])))
          all = false;
      }
      if (all && kc) return tk;
      if (all && k != band_k) return bandval(i, j, depth);
      double v = kInf;
      for (int s = 0; s < 4; ++s)
        if (byc[s] < kInf) v = std::fmin(v, upd(i, j, s, depth));
      return v;
    }
    // a band cell's value at the exit, memoised
    double bandval(int64_t i, int64_t j, int depth) {
      const uint64_t k = (uint64_t)(j * NX + i);
      if (const double* hit = bmemo.find(k + 1)) return *hit;
      const uint64_t saved = band_k;
      band_k = k;
      const double v = val(i, j, last, lim, depth + 1);
      band_k = saved;
      bmemo.put(k + 1, v);
      return v;
    }
    // the reference update of k at the pop of its neighbour in nb4 slot s (:462-465)
    double upd(int64_t i, int64_t j, int s, int depth) {
      const uint64_t k = (uint64_t)(j * NX + i);
      const uint64_t key = k * 4 + (uint64_t)s + 1;
      if (const double* hit = memo.find(key)) return *hit;
      if (depth > 3000 || budget == 0) {  // give up (~1 MB of stack)
        overrun = true;
        return tv(i, j);
      }
      --budget;
      memo.put(key, kInf);  // (pops only go back in time: never re-entered)
      const int64_t mi = s == 1 ? i - 1 : s == 2 ? i + 1 : i;
      const int64_t mj = s == 0 ? j - 1 : s == 3 ? j + 1 : j;
      const uint64_t m = (uint64_t)(mj * NX + mi);
      const double tm = tv(mi, mj);
      const double tx = axis(i - 1, j, i + 1, j, m, tm, depth);
      const double ty = axis(i, j - 1, i, j + 1, m, tm, depth);
      const double v = eikonal(tx, ty, F[k]);
      memo.put(key, v);
      return v;
    }
  };
  const uint64_t g = idx(goal_i_, goal_j_);
  // the work bound (DYMU_REPLAY_BUDGET overrides it: tests of the overrun path)
  static const uint64_t budget = [] {
    const char* kv = std::getenv("DYMU_REPLAY_BUDGET");
    return kv && std::atoll(kv) > 0 ? (uint64_t)std::atoll(kv) : kReplayBudget;
  }();
  out.assign(band.size(), kInf);
  // threads: at least 64 band cells each; the work bound is shared out per thread
  const unsigned nt = std::max(1u, std::min(host_threads(), (unsigned)std::min<uint64_t>(
                                                                 band.size() / 64, 1u << 16)));
  std::vector<uint64_t> used(nt, 0);
  std::vector<TieGuard> tg(nt, guard);  // each thread's guard at its end
  std::vector<uint8_t> bad(nt, 0);
  // runs of band cells taken from a shared counter: the work per cell varies by orders
  // of magnitude along the front (where a staircase front walks far back), so static
  // shares leave most threads idle; a thread keeps its memo across its runs
  const uint64_t run = std::max<uint64_t>(16, band.size() / ((uint64_t)nt * 16));
  std::atomic<uint64_t> next_run{0};
  std::vector<double> tms(nt, 0.0);
  const auto tp0 = std::chrono::steady_clock::now();
  parallel_tasks(nt, [&](unsigned t) {
    const auto tt0 = std::chrono::steady_clock::now();
    struct Stamp {
      double& ms;
      std::chrono::steady_clock::time_point t0;
      ~Stamp() {
        ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
      }
    } stamp{tms[t], tt0};
    Replay rec(*this, guard, g, last, std::max<uint64_t>(1, budget / nt));
    for (;;) {
      const uint64_t q0 = next_run.fetch_add(run, std::memory_order_relaxed);
      if (q0 >= band.size() || rec.overrun || rec.po.degenerate()) break;
      const uint64_t q1 = std::min<uint64_t>(band.size(), q0 + run);
      for (uint64_t q = q0; q < q1 && !rec.overrun && !rec.po.degenerate(); ++q)
        out[q] = rec.bandval((int64_t)(band[q] % nx_), (int64_t)(band[q] / nx_), 0);
    }
    used[t] = std::max<uint64_t>(1, budget / nt) - rec.budget;
    tg[t] = rec.guard;
    bad[t] = rec.overrun || rec.po.degenerate();
    if (rec.po.degenerate() && std::getenv("DYMU_ORDER_DEBUG")) {
      const uint64_t k = rec.po.whyCell();
      std::fprintf(stderr, "[dymu] order undetermined: reason %d at (%llu, %llu)\n",
                   rec.po.why(), (unsigned long long)(k % nx_), (unsigned long long)(k / nx_));
    }
  });
  if (std::getenv("DYMU_ORDER_DEBUG")) {
    std::fprintf(stderr, "[dymu] band replay %.1f ms, per thread:",
                 std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tp0)
                     .count());
    for (unsigned t = 0; t < nt; ++t) std::fprintf(stderr, " %.1f/%llu", tms[t], (unsigned long long)used[t]);
    std::fprintf(stderr, "\n");
  }
  early_info_.replay_threads = nt;
  early_info_.replay_updates = 0;
  bool give_up = false;
  for (unsigned t = 0; t < nt; ++t) {
    early_info_.replay_updates += used[t];
    if (!guard.near && tg[t].near) {
      std::copy(tg[t].first, tg[t].first + 2, guard.first);
      std::copy(tg[t].first_t, tg[t].first_t + 2, guard.first_t);
    }
    guard.near += tg[t].near;
    give_up = give_up || bad[t];
  }
  return give_up || guard.near > 0;
}

// band_cells_ after a GPU early exit are in grid order: put them in the reference's
// insertion order (pop_order.hpp) before anyone reads the order.  (The exit has
// already checked the order for near ties: the exact replay ran otherwise.)
void DyMuPathPlanner::orderBand() {
  if (!band_unordered_) return;
  band_unordered_ = false;
  PopOrder<MapT> po(MapT{this}, nx_, ny_, idx(goal_i_, goal_j_));
  std::vector<uint64_t> b(band_cells_);
  std::stable_sort(b.begin(), b.end(),
                   [&po](uint64_t x, uint64_t y) { return po.insBefore(x, y); });
  if (!po.degenerate()) band_cells_.swap(b);  // else keep grid order
}

// The reference FMM replayed exactly on the host: its band as a heap keyed (T,
// first-insertion sequence) -- the pops of the first-strict-minimum scan (:551-568) in
// the same order -- from the goal until the start (si, sj) and its nb4 are CLOSED
// (computeTotalCostMap :364-408; si < 0: until the band empties, :443-468).  It runs
// over a box (inclusive; empty: the whole grid): every cell the reference pops at the
// exit has a value at most t_closed, and the caller's box holds every cell the engine
// puts below t_closed (1 + kRegionMargin) plus a ring; a pop whose neighbour lies
// outside it means the box was short, and the replay restarts on the whole grid.
// The box is stored with a one-cell ring at +inf: off the grid that is the reference's
// "the other neighbour alone" (:504-523, fmin(+inf, x) = x), off the box "never
// reached"; the ring's state says which (4: off the grid, never a neighbour; 3: outside
// the box).  The band is a radix heap (BandQueue below); each pop prefetches the next
// one's neighbourhood while it updates its own.
// O(m log m) for the m cells the reference reaches.
namespace {
// The band in the reference's pop order -- least value, equal values by first insertion
// -- as a radix heap on the values' bit patterns (a non-negative double orders as its
// bits): bucket b > 0 holds the keys whose highest bit differing from the last popped
// key is bit b - 1; `eq` (a heap on the sequence) the keys equal to it.  Every value the
// replay inserts is at least the last popped one in exact arithmetic; one rounded below
// it goes to `below` (a heap on value, then sequence), popped first.  A lowered value
// is pushed again and the entry it supersedes is skipped when popped (its value is no
// longer the cell's).
struct BandQueue {
  struct E {
    uint64_t key, seq, p, k;  // value bits, first insertion, box-local index, grid index
  };
  std::vector<E> b[65], eq, below;
  uint64_t last = 0;
  static bool seq_after(const E& x, const E& y) { return x.seq > y.seq; }
  static bool after(const E& x, const E& y) {
    return x.key > y.key || (x.key == y.key && x.seq > y.seq);
  }
  void push(const E& e) {
    if (e.key < last) {
      below.push_back(e);
      std::push_heap(below.begin(), below.end(), after);
    } else if (e.key == last) {
      eq.push_back(e);
      std::push_heap(eq.begin(), eq.end(), seq_after);
    } else {
      b[64 - __builtin_clzll(e.key ^ last)].push_back(e);
    }
  }
  // the entry the next pop returns (nullptr: empty); the least key's bucket is spread
  // over the lower ones when `eq` has run dry
  const E* next() {
    if (!below.empty()) return &below.front();
    if (eq.empty()) {
      int i = 1;
      while (i <= 64 && b[i].empty()) ++i;
      if (i > 64) return nullptr;
      uint64_t mn = ~0ull;
      for (const E& e : b[i]) mn = std::min(mn, e.key);
      last = mn;
      std::vector<E> v;
      v.swap(b[i]);
      for (const E& e : v) push(e);  // each goes to a bucket below i, or to eq
      v.clear();
      b[i].swap(v);  // the bucket keeps its buffer
    }
    return &eq.front();
  }
  bool pop(E& out) {
    if (!next()) return false;
    const bool lo = !below.empty();
    std::vector<E>& h = lo ? below : eq;
    std::pop_heap(h.begin(), h.end(), lo ? after : seq_after);
    out = h.back();
    h.pop_back();
    return true;
  }
};

uint64_t value_bits(double t) {
  uint64_t u;
  std::memcpy(&u, &t, sizeof u);
  return u;
}
}  // namespace

DyMuPathPlanner::HostFmm DyMuPathPlanner::hostFmm(int64_t si, int64_t sj,
                                                  const int64_t box_in[4]) const {
  const double* F = speed_.data();
  HostFmm r;
  r.bx[0] = r.bx[1] = 0;
  r.bx[2] = (int64_t)nx_ - 1;
  r.bx[3] = (int64_t)ny_ - 1;
  if (box_in && box_in[0] <= box_in[2]) {  // the region grown by two more cells
    r.bx[0] = std::max<int64_t>(0, box_in[0] - 2);
    r.bx[1] = std::max<int64_t>(0, box_in[1] - 2);
    r.bx[2] = std::min<int64_t>(nx_ - 1, box_in[2] + 2);
    r.bx[3] = std::min<int64_t>(ny_ - 1, box_in[3] + 2);
  }
  for (;;) {
    const int64_t* bx = r.bx;
    const int64_t W = bx[2] - bx[0] + 1, H = bx[3] - bx[1] + 1, PW = W + 2;
    r.W = W;
    r.PW = PW;
    const uint64_t m = (uint64_t)PW * (uint64_t)(H + 2);
    r.T.assign(m, kInf);
    r.st.assign(m, 0);  // 1 CLOSED, 2 in the band; the ring 3 / 4
    {
      const uint8_t s_lo = bx[1] > 0 ? 3 : 4, s_hi = bx[3] + 1 < (int64_t)ny_ ? 3 : 4;
      const uint8_t w_lo = bx[0] > 0 ? 3 : 4, w_hi = bx[2] + 1 < (int64_t)nx_ ? 3 : 4;
      for (int64_t c = 0; c < PW; ++c) {
        r.st[(uint64_t)c] = s_lo;
        r.st[(uint64_t)(H + 1) * PW + c] = s_hi;
      }
      for (int64_t q = 1; q <= H; ++q) {
        r.st[(uint64_t)q * PW] = w_lo;
        r.st[(uint64_t)q * PW + W + 1] = w_hi;
      }
    }
    r.order.clear();
    // each band cell's first-insertion sequence (32 bits while the box allows)
    const bool wide = m >= (1ull << 32);
    std::vector<uint32_t> seq32(wide ? 0 : m);
    std::vector<uint64_t> seq64(wide ? m : 0);
    BandQueue band;
    double* T = r.T.data();
    uint8_t* st = r.st.data();
    const uint64_t g = r.at(goal_i_, goal_j_);
    T[g] = 0.0;
    r.order.push_back(idx(goal_i_, goal_j_));
    st[g] = 2;
    band.push({value_bits(0.0), 0, g, idx(goal_i_, goal_j_)});
    r.band = 1;
    bool short_box = false;
    const bool early = si >= 0;
    const uint64_t sl = early ? r.at(si, sj) : 0;
    auto fully_closed = [&] {  // :424-436 (the start is interior: safeNode)
      return early && st[sl] == 1 && st[sl - PW] == 1 && st[sl - 1] == 1 && st[sl + 1] == 1 &&
             st[sl + PW] == 1;
    };
    const int64_t dp[4] = {-PW, -1, 1, PW};  // nb4 order (:76-80)
    const int64_t dk[4] = {-(int64_t)nx_, -1, 1, (int64_t)nx_};
    BandQueue::E top;
    while (r.band > 0 && !fully_closed() && !short_box && band.pop(top)) {
      const uint64_t p = top.p, kp = top.k;
      if (st[p] != 2 || value_bits(T[p]) != top.key) continue;  // a superseded entry
      st[p] = 1;
      --r.band;
      if (const BandQueue::E* nx = band.next()) {  // its neighbourhood, fetched meanwhile
        const uint64_t np = nx->p, nk = nx->k;
        const int64_t NX = (int64_t)nx_, mb = (int64_t)m - 1, ng = (int64_t)nx_ * ny_ - 1;
        auto in = [](int64_t x, int64_t hi) { return x < 0 ? 0 : x > hi ? hi : x; };
        const int64_t dt[8] = {-2 * PW, -PW - 1, -PW + 1, -1, 1, PW - 1, PW + 1, 2 * PW};
        for (const int64_t d : dt) __builtin_prefetch(T + in((int64_t)np + d, mb));
        const int64_t ds[3] = {-PW, 0, PW}, df[3] = {-NX, 0, NX};
        for (const int64_t d : ds) __builtin_prefetch(st + in((int64_t)np + d, mb));
        for (const int64_t d : df) __builtin_prefetch(F + in((int64_t)nk + d, ng));
      }
      for (int s = 0; s < 4; ++s) {
        const uint64_t q = p + dp[s];
        const uint8_t sq = st[q];
        if (sq == 1 || sq == 4) continue;
        if (sq == 3) {
          short_box = true;  // the reference reaches beyond the box
          break;
        }
        const uint64_t kq = kp + dk[s];
        const double C = F[kq];
        if (!(C < kInf)) continue;
        // propagateGlobalNode (:500-546) from the current values
        const double Ty = std::fmin(T[q + PW], T[q - PW]);
        const double Tx = std::fmin(T[q - 1], T[q + 1]);
        double u;
        if ((std::fabs(Tx - Ty) < C) && (Tx < kInf) && (Ty < kInf))
          u = (Tx + Ty + std::sqrt(2 * (C * C) - ((Tx - Ty) * (Tx - Ty)))) / 2;
        else
          u = std::fmin(Tx, Ty) + C;
        if (!(u < T[q])) continue;
        uint64_t seq;
        if (T[q] == kInf) {  // first reached: into the band and the propagated list
          seq = r.order.size();
          if (wide)
            seq64[q] = seq;
          else
            seq32[q] = (uint32_t)seq;
          r.order.push_back(kq);
          st[q] = 2;
          ++r.band;
        } else {
          seq = wide ? seq64[q] : seq32[q];
        }
        T[q] = u;
        band.push({value_bits(u), seq, q, kq});
      }
    }
    if (short_box && !(bx[0] == 0 && bx[1] == 0 && bx[2] == nx_ - 1 && bx[3] == ny_ - 1)) {
      if (std::getenv("DYMU_ORDER_DEBUG"))
        std::fprintf(stderr, "[dymu] exact replay: box short, restarting on the whole grid\n");
      r.bx[0] = r.bx[1] = 0;
      r.bx[2] = (int64_t)nx_ - 1;
      r.bx[3] = (int64_t)ny_ - 1;
      continue;
    }
    return r;
  }
}

// computeTotalCostMap's exit replayed exactly on the host (hostFmm) over the region
// box -- when the values cannot decide the reference's order at the exit (near ties,
// degenerate ties) or the band replay hit its work bound.  The map, the node states,
// the band (insertion order) and global_propagated_nodes become the reference's.
bool DyMuPathPlanner::exactEarlyExit(unsigned si, unsigned sj, const int64_t box[4]) {
  const uint64_t n = (uint64_t)nx_ * ny_;
  HostFmm r = hostFmm(si, sj, box);
  const int64_t* bx = r.bx;
  invalidateLabels();
  std::fill(total_cost_.begin(), total_cost_.end(), kInf);
  node_state_.assign(n, 0);
  for (int64_t j = bx[1]; j <= bx[3]; ++j)
    for (int64_t i = bx[0]; i <= bx[2]; ++i) {
      const uint64_t k = r.at(i, j);
      const uint64_t kg = idx((unsigned)i, (unsigned)j);
      total_cost_[kg] = r.T[k];
      node_state_[kg] = r.st[k] == 1 ? 1 : 0;
    }
  std::fill(blk_ok_.begin(), blk_ok_.end(), 1);
  blk_missing_ = 0;
  if (dymu_memcpy_h2d(ctx_, dT_, total_cost_.data(), sizeof(double) * n) != DYMU_OK)
    throw std::runtime_error(std::string("dymu: total-cost upload failed: ") +
                             dymu_last_error(ctx_));
  dev_map_current_ = true;
  band_cells_.clear();
  band_unordered_ = false;
  band_values_checked_ = true;
  open_at_limit_.clear();
  for (const uint64_t kg : r.order)
    if (!node_state_[kg]) band_cells_.push_back(kg);  // the reference's band vector, in order
  propagated_extra_.swap(r.order);
  manual_list_ = true;
  solved_ = false, gs_seeds_.clear();
  return r.band > 0;  // :399-407
}

// global_propagated_nodes (:447, :537-545) after a GPU solve: every reached node in
// the order the reference inserted it, rebuilt from the values like the band's order
// (pop_order.hpp) but for all nodes at once -- the popped (CLOSED) nodes ranked by value,
// equal values by insertion; a node's insertion keyed by the rank of its first-popped
// neighbour (its least CLOSED one) and its slot in that neighbour's nb4 list.  Near ties
// (TieGuard) or an undetermined order: the reference's FMM is replayed on the host for
// the order (hostFmm; its values are not installed).
std::vector<uint64_t> DyMuPathPlanner::insertionOrder() {
  fetchAll();
  const uint64_t n = (uint64_t)nx_ * ny_;
  const double* t = total_cost_.data();
  const uint64_t g = idx(goal_i_, goal_j_);
  std::vector<uint64_t> reached;
  for (uint64_t k = 0; k < n; ++k)
    if (t[k] < kInf) reached.push_back(k);
  // the constant-speed radius around the goal (TieGuard): mirror ties trusted within
  const double f0 = speed_[g];
  double d2 = kInf;
  for (uint64_t k = 0; k < n; ++k)
    if (speed_[k] != f0) {
      const double di = (double)(k % nx_) - goal_i_, dj = (double)(k / nx_) - goal_j_;
      d2 = std::fmin(d2, di * di + dj * dj);
    }
  TieGuard guard(nx_, goal_i_, goal_j_, f0, std::sqrt(d2));
  // DYMU_EXACT_EXIT=1 sends the list to the exact replay too (tests of that path).  So
  // does a list of more than 2^23 nodes: among that many values some two lie within 1e-12
  // of each other (tens of such pairs are expected; none has been seen missing), so the
  // sort below would only find that out
  static const bool force_exact = [] {
    const char* kv = std::getenv("DYMU_EXACT_EXIT");
    return kv && std::atoi(kv) != 0;
  }();
  std::vector<std::pair<double, uint64_t>> popped;
  const bool large = reached.size() > (1ull << 23);
  if (!force_exact && !large) {
    for (const uint64_t k : reached)
      if (closedCell(k)) popped.push_back({t[k], k});
    parallel_sort(popped);
  }
  bool undetermined = force_exact || large || popped.empty() || popped[0].second != g;
  // near ties between consecutive values first (on the host threads): any one of them
  // leaves the pop order to the exact replay, and the keys below would be wasted (the
  // sorted values' mean spacing falls with the cell count: from ~2^22 reached cells on
  // generic terrain some pair lies within 1e-12 of each other)
  {
    const uint64_t m = popped.size();
    const unsigned nt = std::max(1u, std::min(host_threads(), (unsigned)std::min<uint64_t>(m >> 16, 64)));
    std::vector<uint64_t> near(nt, 0);
    parallel_tasks(nt, [&](unsigned th) {
      TieGuard gd(guard);
      gd.near = 0;
      const uint64_t q0 = std::max<uint64_t>(1, m * th / nt), q1 = m * (th + 1) / nt;
      for (uint64_t q = q0; q < q1; ++q)
        if (popped[q].first != popped[q - 1].first)
          (void)gd.cmp(popped[q - 1].second, popped[q - 1].first, popped[q].second, popped[q].first);
      near[th] = gd.near;
    });
    for (const uint64_t x : near) guard.near += x;
  }
  if (guard.near > 0) undetermined = true;
  std::vector<uint64_t> rank(undetermined ? 0 : n, ~0ull);
  // x's first-popped neighbour (least value, equal ones by rank) and x's slot in its list;
  // false when none is ranked (x ties with its least neighbour: undetermined)
  auto first_popped = [&](uint64_t x, uint64_t& key, TieGuard& gd) {
    const unsigned i = (unsigned)(x % nx_), j = (unsigned)(x / nx_);
    uint64_t nb[4];
    int slot[4], m = 0;  // x's slot in nb's list: (i,j-1) sees x as its (i,j+1): 3, ...
    if (j > 0) nb[m] = x - nx_, slot[m++] = 3;
    if (i > 0) nb[m] = x - 1, slot[m++] = 2;
    if (i + 1 < nx_) nb[m] = x + 1, slot[m++] = 1;
    if (j + 1 < ny_) nb[m] = x + nx_, slot[m++] = 0;
    int best = -1;
    for (int q = 0; q < m; ++q) {
      if (rank[nb[q]] == ~0ull) continue;
      if (best < 0) {
        best = q;
        continue;
      }
      const int c = gd.cmp(nb[q], t[nb[q]], nb[best], t[nb[best]]);
      if (c < 0 || (c == 0 && rank[nb[q]] < rank[nb[best]])) best = q;
    }
    if (best < 0) return false;
    if (gd.cmp(nb[best], t[nb[best]], x, t[x]) >= 0) return false;
    key = rank[nb[best]] * 4 + (uint64_t)slot[best];
    return true;
  };
  // pop ranks: value order; a group of equal values in insertion order (a lone value
  // needs no key: its checks run with every node's below)
  uint64_t next = 0;
  std::vector<std::pair<uint64_t, uint64_t>> grp;
  for (size_t a = 0; a < popped.size() && !undetermined;) {
    size_t b = a + 1;
    while (b < popped.size() && popped[b].first == popped[a].first) ++b;
    if (b == a + 1) {
      rank[popped[a].second] = next++;
      a = b;
      continue;
    }
    grp.clear();
    for (size_t q = a; q < b; ++q) {
      const uint64_t x = popped[q].second;
      if (q > a) (void)guard.cmp(popped[a].second, popped[a].first, x, popped[q].first);
      uint64_t key = 0;
      if (x != g && !first_popped(x, key, guard)) undetermined = true;
      grp.push_back({x == g ? 0 : key + 1, x});
    }
    std::sort(grp.begin(), grp.end());
    for (const auto& e : grp) rank[e.second] = next++;
    a = b;
  }
  popped = {};
  // every reached node keyed by its first-popped neighbour's rank and slot, on the host
  // threads (each with its own guard; their near ties are summed)
  std::vector<std::pair<uint64_t, uint64_t>> ins;
  if (!undetermined) {
    ins.resize(reached.size());
    const unsigned nt = std::max(
        1u, std::min(host_threads(), (unsigned)std::min<uint64_t>(reached.size() >> 16, 64)));
    std::vector<TieGuard> tg(nt, guard);
    for (auto& gd : tg) gd.near = 0;
    std::vector<uint8_t> und(nt, 0);
    std::atomic<bool> stop{false};
    parallel_tasks(nt, [&](unsigned th) {
      const uint64_t q0 = reached.size() * th / nt, q1 = reached.size() * (th + 1) / nt;
      for (uint64_t q = q0; q < q1 && !stop.load(std::memory_order_relaxed); ++q) {
        const uint64_t x = reached[q];
        uint64_t key = 0;
        if (x != g && !first_popped(x, key, tg[th])) {
          und[th] = 1;
          stop.store(true, std::memory_order_relaxed);
        }
        ins[q] = {x == g ? 0 : key + 1, x};
      }
    });
    for (unsigned th = 0; th < nt; ++th) {
      guard.near += tg[th].near;
      undetermined = undetermined || und[th];
    }
  }
  std::vector<uint64_t> order;
  if (undetermined || guard.near > 0) {  // the reference's own order, replayed
    const int64_t none[4] = {0, 0, -1, -1};
    const bool early = closed_limit_ < kInf && have_start_;
    HostFmm r = hostFmm(early ? (int64_t)start_i_ : -1, early ? (int64_t)start_j_ : -1,
                        early ? exit_box_ : none);
    order.swap(r.order);
  } else {
    parallel_sort(ins);
    order.reserve(ins.size());
    for (const auto& e : ins) order.push_back(e.second);
  }
  return order;
}

void DyMuPathPlanner::copyNodeStates(uint8_t* out) {
  const uint64_t n = (uint64_t)nx_ * ny_;
  if (!node_state_.empty()) {
    std::memcpy(out, node_state_.data(), n);
    return;
  }
  fetchAll();
  for (uint64_t k = 0; k < n; ++k) out[k] = closedCell(k) ? 1 : 0;
}

// :443-468
bool DyMuPathPlanner::computeEntireTotalCostMap() {
  if (!has_goal_ || is_obstacle_[idx(goal_i_, goal_j_)]) {
    log_warn("The goal is not valid");
    return false;
  }
  if (!goals_.empty()) return propagateGoals();
  return propagate(false, 0, 0);
}

// :410-422 (start and its 8 neighbours must be free; border -> false here,
// where the reference dereferences NULL)
bool DyMuPathPlanner::safeNode(unsigned i, unsigned j) const {
  if (i == 0 || j == 0 || i + 1 >= nx_ || j + 1 >= ny_) return false;
  for (int dj = -1; dj <= 1; ++dj)
    for (int di = -1; di <= 1; ++di)
      if (is_obstacle_[idx(i + di, j + dj)]) return false;
  return true;
}

// :364-408.  The propagation stops once the start node and its nb4 are final
// (dymu_solve_until_device); the return value is the reference's: false iff
// the narrow band is empty at that moment (the start is unreachable, or its
// neighbourhood closed last of all the reachable nodes).
bool DyMuPathPlanner::computeTotalCostMap(base::Waypoint wPos) {
  const double x = wPos.position[0] - global_offset_[0];
  const double y = wPos.position[1] - global_offset_[1];
  if (!has_goal_ || is_obstacle_[idx(goal_i_, goal_j_)]) {
    log_warn("The goal is not valid");
    return false;
  }
  const double fx = x / global_res_ + 0.5, fy = y / global_res_ + 0.5;
  if (!(fx >= 0) || !(fy >= 0) || fx >= (double)nx_ || fy >= (double)ny_) {
    log_error("PLANNER: The rover is located too close to an obstacle");
    return false;
  }
  const unsigned si = grid_u32(fx), sj = grid_u32(fy);
  if (!safeNode(si, sj)) {
    log_error("PLANNER: The rover is located too close to an obstacle");
    return false;
  }
  // a goal set has no early exit (the reference's tie and insertion-order rules are
  // single-goal): the whole map, and "unreachable" read from it
  if (!goals_.empty() ? !(propagateGoals() && T(idx(si, sj)) < kInf) : !propagate(true, si, sj)) {
    log_error("The goal is unreachable");
    return false;
  }
  return true;
}

// :589-611 (evaluatePath(0) repairs the segments through local risk; it is the
// identity while no global node is subdivided)
std::vector<base::Waypoint> DyMuPathPlanner::getPath(base::Waypoint wPos) {
  wPos.position[0] -= global_offset_[0];
  wPos.position[1] -= global_offset_[1];
  computeGlobalPath(wPos);
  evaluatePath(0);
  std::vector<base::Waypoint> out = current_path;
  for (auto& w : out) {
    w.position[0] += global_offset_[0];
    w.position[1] += global_offset_[1];
  }
  return out;
}

// :615-662 (gradient descent on T; Q5: a NaN position ends the loop and the
// sink is appended)
bool DyMuPathPlanner::computeGlobalPath(base::Waypoint wPos) {
  current_path.clear();
  if (!has_goal_) return false;
  if (!goals_.empty()) ensureHostLabels();
  const int st = descend(wPos, current_path, std::numeric_limits<uint64_t>::max(), 1);
  if (st == -1) log_error("PLANNER: Gradient Descent Method failed");
  if (st == 0) log_error("ERROR in trajectory");
  return st == 1;
}

namespace {
// The cell of grid coordinate g on an axis of n nodes: the reference's (uint) cast of
// an in-range value (grid_u32), tested in 64-bit so that nothing wraps; false when the
// cell or its +1 neighbour is off the grid -- negative (below -1), huge and NaN
// coordinates included.  k_extract_paths (path_kernels.hip) makes the same test.
bool path_cell(double g, unsigned n, unsigned& c) {
  if (!(g > -9.2e18 && g < 9.2e18)) return false;
  const int64_t t = (int64_t)g;
  if (t < 0 || t + 1 >= (int64_t)n) return false;
  c = (unsigned)t;
  return true;
}
// :776-784 (interpolate)
double bilinear(double a, double b, double g00, double g01, double g10, double g11) {
  return g00 + (g10 - g00) * a + (g01 - g00) * b + (g11 + g00 - g10 - g01) * a * b;
}
}  // namespace

// The record of one path while the host descent builds it (include/dymu_fim.h,
// dymu_path_stat): k_path_stats (path_stats_kernels.hip) forms the same sums in the same
// order.  Field f at node k is speed (slot 0: the packed speed the solve used, or the
// node fields' speed where none was packed yet) or the caller's array (slot 1).
struct DyMuPathPlanner::PathAccum {
  dymu_path_stat r;
  unsigned nf = 0;
  const double* f[DYMU_PATH_FIELDS] = {nullptr, nullptr, nullptr, nullptr};
  double px = 0, py = 0;
  double pv[DYMU_PATH_FIELDS] = {0, 0, 0, 0};  // the previous waypoint's samples ...
  unsigned ok = 0;                             // ... and which of them count
  static dymu_path_stat empty() {
    dymu_path_stat e{};
    e.status = -1;
    e.sink = -1;
    for (int q = 0; q < DYMU_PATH_FIELDS; ++q) {
      e.vmin[q] = kInf;
      e.vmax[q] = -kInf;
    }
    return e;
  }
  PathAccum() : r(empty()) {}
  void add(const DyMuPathPlanner& pl, double x, double y) {
    if (r.count > 0) {
      const double dx = px - x, dy = py - y;
      const double seg = std::sqrt(dx * dx + dy * dy);
      r.length = r.length + seg;
      r.last_hop = seg;
      for (unsigned q = 0; q < nf; ++q)
        if (ok >> q & 1u) r.integral[q] = r.integral[q] + pv[q] * seg;
    }
    // nearestIndex's rule; nothing is read before the node is known to be on the grid
    const uint32_t i = grid_u32(x / pl.global_res_ + 0.5), j = grid_u32(y / pl.global_res_ + 0.5);
    const bool in = i < pl.nx_ && j < pl.ny_;
    ok = 0;
    for (unsigned q = 0; q < nf; ++q) {
      double v = 0;
      if (in) {
        const uint64_t k = pl.idx(i, j);
        v = f[q] ? f[q][k] : pl.is_obstacle_[k] ? kInf : pl.nodeSpeed(k);
      }
      if (in && v < kInf && v > -kInf) {
        r.vmin[q] = v < r.vmin[q] ? v : r.vmin[q];
        r.vmax[q] = v > r.vmax[q] ? v : r.vmax[q];
        pv[q] = v;
        ok |= 1u << q;
      } else {
        ++r.skipped[q];
      }
    }
    px = x;
    py = y;
    ++r.count;
  }
};

// The loop of computeGlobalPath into `path`, without member writes.  Returns getPaths'
// status: 1 sink appended, 0 "ERROR in trajectory" (the waypoints so far kept), -1 the
// first step is NaN (empty path), -3 more than max_wp waypoints (the first max_wp
// kept).  Waypoint w of the reference's path is kept when w % stride == 0, the sink
// always; the loop runs at most max_wp * stride steps (k_extract_paths' bound).
// With a goal set (labels_ valid: ensureHostLabels) the sink follows the label map as in
// k_extract_paths<true>: before each step, when the position is in another cell than the
// last one looked up, the sink becomes the goal labelled on that cell's node (no label:
// the previous sink stays; none yet at the first step: -1).  *sink_out = the goal whose
// sink was appended, -1 otherwise.
// With acc the kept waypoints join its record (grid-local x, y) and `path` stays empty.
int DyMuPathPlanner::descend(base::Waypoint wPos, std::vector<base::Waypoint>& path,
                             uint64_t max_wp, unsigned stride, int* sink_out,
                             PathAccum* acc) const {
  path.clear();
  if (sink_out) *sink_out = -1;
  if (!has_goal_) return -1;
  const uint64_t limit = max_wp > std::numeric_limits<uint64_t>::max() / stride
                             ? std::numeric_limits<uint64_t>::max()
                             : max_wp * stride;
  base::Waypoint sink = nodeSink(goal_i_, goal_j_, goal_heading_);
  const bool gs = !goals_.empty();
  int sink_k = gs ? -1 : 0;
  bool held = false;
  unsigned hcx = 0, hcy = 0;
  auto track = [&](const base::Waypoint& p) {
    if (!gs) return;
    unsigned cx = 0, cy = 0;
    if (!path_cell(p.position[0] / global_res_, nx_, cx) ||
        !path_cell(p.position[1] / global_res_, ny_, cy))
      return;
    if (held && cx == hcx && cy == hcy) return;
    held = true;
    hcx = cx;
    hcy = cy;
    const uint32_t lab = labels_[idx(cx, cy)];
    if (lab < goals_.size()) {
      sink = sinkWaypoint(lab);
      sink_k = (int)lab;
    }
  };
  const double tau = std::min(0.4, risk_distance_);
  track(wPos);
  base::Waypoint wNext = nextWaypoint(wPos, tau);
  if (std::isnan(wNext.position[0]) || std::isnan(wNext.position[1])) return -1;
  if (sink_k < 0) return -1;
  unsigned phase = 0;
  auto keep = [&](const base::Waypoint& w) {
    if (acc) acc->add(*this, w.position[0], w.position[1]);
    else path.push_back(w);
  };
  auto push = [&](const base::Waypoint& w) {
    if (phase == 0) keep(w);
    if (++phase == stride) phase = 0;
  };
  push(wPos);
  wPos = wNext;
  auto dist = [](const base::Waypoint& a, const base::Waypoint& b) {
    const double dx = a.position[0] - b.position[0], dy = a.position[1] - b.position[1];
    return std::sqrt(dx * dx + dy * dy);
  };
  for (uint64_t w = 1; dist(wPos, sink) > 2.0 * global_res_; ++w) {
    if (w == limit) return -3;
    track(wPos);
    wNext = nextWaypoint(wPos, tau);
    push(wPos);
    if (dist(wPos, wNext) < 0.01 * tau * global_res_) return 0;
    wPos = wNext;
  }
  if ((acc ? (uint64_t)acc->r.count : (uint64_t)path.size()) >= max_wp) return -3;
  keep(sink);
  if (sink_out) *sink_out = sink_k;
  return 1;
}

// :666-714 (wPos.position[2] is written: elevation, bilinear, with the
// reference's argument order at :699-704)
base::Waypoint DyMuPathPlanner::computeNextGlobalWaypoint(base::Waypoint& wPos, double tau) {
  return nextWaypoint(wPos, tau);
}

base::Waypoint DyMuPathPlanner::nextWaypoint(base::Waypoint& wPos, double tau) const {
  base::Waypoint wNext;
  const double gx = wPos.position[0] / global_res_, gy = wPos.position[1] / global_res_;
  unsigned cx = 0, cy = 0;
  if (!path_cell(gx, nx_, cx) || !path_cell(gy, ny_, cy)) {  // reference: NULL dereference
    wNext.position[0] = wNext.position[1] = std::numeric_limits<double>::quiet_NaN();
    return wNext;
  }
  const double ax = gx - (double)cx, ay = gy - (double)cy;
  double gx00, gx10, gx01, gx11, gy00, gy10, gy01, gy11;
  gradientNode(cx, cy, gx00, gy00);
  gradientNode(cx + 1, cy, gx10, gy10);
  gradientNode(cx, cy + 1, gx01, gy01);
  gradientNode(cx + 1, cy + 1, gx11, gy11);
  const double dcx = bilinear(ax, ay, gx00, gx01, gx10, gx11);
  const double dcy = bilinear(ax, ay, gy00, gy01, gy10, gy11);
  const uint64_t k = idx(cx, cy);
  wPos.position[2] =
      bilinear(ax, ay, elevation_[k], elevation_[k + 1], elevation_[k + nx_],
                  elevation_[k + nx_ + 1]);
  wNext.position[0] = wPos.position[0] - global_res_ * tau * dcx;
  wNext.position[1] = wPos.position[1] - global_res_ * tau * dcy;
  wNext.heading = std::atan2(-dcy, -dcx);
  return wNext;
}

void DyMuPathPlanner::gradientNode(const globalNode& n, double& dnx, double& dny) const {
  const double i = n.pose.position[0], j = n.pose.position[1];
  if (!(i >= 0 && j >= 0 && i < nx_ && j < ny_)) {
    dnx = dny = 0;
    return;
  }
  gradientNode((unsigned)i, (unsigned)j, dnx, dny);
}

// :718-772
void DyMuPathPlanner::gradientNode(unsigned i, unsigned j, double& dnx, double& dny) const {
  const uint64_t k = idx(i, j);
  const bool hw = i > 0, he = i + 1 < nx_, hs = j > 0, hn = j + 1 < ny_;
  const double tw = hw ? T(k - 1) : kInf, te = he ? T(k + 1) : kInf;
  const double ts = hs ? T(k - nx_) : kInf, tn = hn ? T(k + nx_) : kInf;
  const double t = T(k);
  double dx, dy;
  if ((!hw && !he) || (hw && he && tw == kInf && te == kInf)) dx = 0;
  else if (!hw || tw == kInf) dx = te - t;
  else if (!he || te == kInf) dx = t - tw;
  else dx = (te - tw) * 0.5;
  if ((!hs && !hn) || (hs && hn && ts == kInf && tn == kInf)) dy = 0;
  else if (!hs || ts == kInf) dy = tn - t;
  else if (!hn || tn == kInf) dy = t - ts;
  else dy = (tn - ts) * 0.5;
  if (dx == 0 && dy == 0) {
    dnx = 0;
    dny = 0;
  } else {
    dnx = dx / std::sqrt(dx * dx + dy * dy);
    dny = dy / std::sqrt(dx * dx + dy * dy);
  }
}

// :776-784
double DyMuPathPlanner::interpolate(double a, double b, double g00, double g01, double g10,
                                    double g11) {
  return bilinear(a, b, g00, g01, g10, g11);
}

// ---- getPaths: batched path extraction (extension) ----

// The planner runs over any implementation of the engine C-ABI (tests/hostengine is a
// host one).  One that predates the path entries leaves these two references null,
// and getPaths then takes its host route (lastPathsOnDevice() says which ran);
// libdymu_fim.so always has them.
#pragma weak dymu_extract_paths_device
#pragma weak dymu_last_paths_ms

std::vector<std::vector<base::Waypoint>> DyMuPathPlanner::getPaths(
    const std::vector<base::Waypoint>& starts, std::vector<int>* status, unsigned max_wp,
    unsigned stride, std::vector<int>* sinks) {
  if (max_wp == 0 || stride == 0) throw std::invalid_argument("getPaths: max_wp, stride >= 1");
  const size_t n = starts.size();
  std::vector<std::vector<base::Waypoint>> out(n);
  std::vector<int> st(n, -1), sk(n, -1);
  last_paths_device_ = false;
  last_paths_kernel_ms_ = 0.0;
  if (n && has_goal_) {
    if (descentOnDevice() && n <= 0xffffffffull && &dymu_extract_paths_device &&
        &dymu_last_paths_ms) {
      pathsOnDevice(starts, out, st, sk, max_wp, stride);
      last_paths_device_ = true;
    } else {
      if (!goals_.empty()) ensureHostLabels();
      // the host descent per start (T() is thread-safe; descend writes no member)
      for_each_start(n, [&](size_t q) {
        base::Waypoint w = starts[q];
        w.position[0] -= global_offset_[0];
        w.position[1] -= global_offset_[1];
        st[q] = descend(w, out[q], max_wp, stride, &sk[q]);
        for (auto& p : out[q]) {
          p.position[0] += global_offset_[0];
          p.position[1] += global_offset_[1];
        }
      });
    }
  }
  if (status) status->swap(st);
  if (sinks) sinks->swap(sk);
  return out;
}

bool DyMuPathPlanner::descentOnDevice() const {
  return ctx_ && dT_ && dev_map_current_ && (goals_.empty() || goalsOnDevice());
}

base::Waypoint DyMuPathPlanner::nodeSink(unsigned gi, unsigned gj, double heading) const {
  base::Waypoint w;
  w.position[0] = global_res_ * (double)gi;
  w.position[1] = global_res_ * (double)gj;
  w.position[2] = elevation_.empty() ? 0.0 : elevation_[idx(gi, gj)];
  w.heading = heading;
  return w;
}

namespace {
// device buffers of one call of `entry`, freed on every path out of it
struct DeviceScratch {
  dymu_ctx* ctx;
  const char* entry;
  std::vector<void*> ptrs;
  DeviceScratch(dymu_ctx* c, const char* name) : ctx(c), entry(name) {}
  ~DeviceScratch() {
    for (void* p : ptrs) (void)dymu_device_free(ctx, p);
  }
  template <class P>
  P* alloc(uint64_t count) {
    void* p = nullptr;
    if (dymu_device_alloc(ctx, sizeof(P) * std::max<uint64_t>(count, 1), &p) != DYMU_OK)
      throw std::runtime_error(std::string("dymu: ") + entry + " device allocation failed: " +
                               dymu_last_error(ctx));
    ptrs.push_back(p);
    return static_cast<P*>(p);
  }
  void release(void* p) {
    ptrs.erase(std::remove(ptrs.begin(), ptrs.end(), p), ptrs.end());
    (void)dymu_device_free(ctx, p);
  }
};
}  // namespace

// One call of a device descent entry (pathsOnDevice, arriveStatsOnDevice,
// pathStatsOnDevice): the map and the sink it runs on -- `target`, else dT_ with the goal
// or, gs, the goal set, whose label map and sinks (grid-local) it puts on the device.
struct DyMuPathPlanner::DeviceQuery {
  DyMuPathPlanner& p;
  const char* entry;
  const double* map;
  const unsigned gi, gj;
  const bool gs;
  const double tau;
  DeviceScratch dev;
  double* d_gxy = nullptr;
  std::vector<double> xy;

  DeviceQuery(DyMuPathPlanner& planner, const char* name, const PathTarget* target)
      : p(planner), entry(name), map(target ? target->map : p.dT_),
        gi(target ? target->gi : p.goal_i_), gj(target ? target->gj : p.goal_j_),
        gs(!target && !p.goals_.empty()), tau(std::min(0.4, p.risk_distance_)),
        dev(p.ctx_, name) {
    if (!gs) return;
    p.ensureDeviceLabels();
    std::vector<double> gxy(2 * p.goals_.size());
    for (size_t k = 0; k < p.goals_.size(); ++k) {
      const base::Waypoint w = p.sinkWaypoint(k);
      gxy[2 * k] = w.position[0];
      gxy[2 * k + 1] = w.position[1];
    }
    d_gxy = dev.alloc<double>(gxy.size());
    check(dymu_memcpy_h2d(p.ctx_, d_gxy, gxy.data(), sizeof(double) * gxy.size()), "upload");
  }
  void check(int rc, const char* what) const {
    if (rc != DYMU_OK)
      throw std::runtime_error(std::string("dymu: ") + entry + " " + what + " failed: " +
                               dymu_strerror(rc) + " " + dymu_last_error(p.ctx_));
  }
  const uint32_t* labels() const { return gs ? p.d_label_ : nullptr; }
  uint32_t goals() const { return gs ? (uint32_t)p.goals_.size() : 0u; }
  // the m starts ids[0 .. m) (ids null: the first m), grid-local, on the device
  double* uploadStarts(const std::vector<base::Waypoint>& starts, const uint32_t* ids, size_t m) {
    xy.resize(2 * m);
    for (size_t q = 0; q < m; ++q) {
      const base::Waypoint& s = starts[ids ? ids[q] : q];
      xy[2 * q] = s.position[0] - p.global_offset_[0];
      xy[2 * q + 1] = s.position[1] - p.global_offset_[1];
    }
    double* d_xy = dev.alloc<double>(2 * (uint64_t)m);
    check(dymu_memcpy_h2d(p.ctx_, d_xy, xy.data(), sizeof(double) * xy.size()), "upload");
    return d_xy;
  }
  // the last launch's time joins the call's kernel time
  void addKernelMs(int (*last_ms)(dymu_ctx*, double*)) {
    double ms = 0.0;
    if (last_ms(p.ctx_, &ms) == DYMU_OK) p.last_paths_kernel_ms_ += ms;
  }
};

namespace {
// The download of per-path rows of a device array with one fixed pitch (pathsOnDevice,
// simplifiedOnDevice): runs of consecutive paths, each downloaded by one pitched copy as
// wide as its longest row -- a run grows while that moves at most twice its elements (plus
// 1024), so few commands move little more than the counts.  len[q] = the elements of row
// q; off[q] = where it lands in the host buffer; returns that buffer's elements.
struct RowRun {
  uint32_t q0, n;
  uint64_t width, base;
};
uint64_t planRowRuns(const std::vector<uint64_t>& len, std::vector<uint64_t>& off,
                     std::vector<RowRun>& runs) {
  const uint32_t m = (uint32_t)len.size();
  off.assign(m, 0);
  runs.clear();
  uint64_t total = 0;
  for (uint32_t q0 = 0; q0 < m;) {
    uint64_t width = len[q0], sum = len[q0];
    uint32_t q1 = q0 + 1;
    for (; q1 < m; ++q1) {
      const uint64_t w2 = std::max(width, len[q1]), s2 = sum + len[q1];
      if (w2 * (q1 + 1 - q0) > 2 * s2 + 1024) break;
      width = w2;
      sum = s2;
    }
    for (uint32_t q = q0; q < q1; ++q) off[q] = total + (uint64_t)(q - q0) * width;
    runs.push_back({q0, q1 - q0, width, total});
    total += width * (q1 - q0);
    q0 = q1;
  }
  return total;
}
}  // namespace

// getPaths' host post-pass: z from the elevation with the host's interpolate call and its
// argument order (nextWaypoint), heading = atan2(-dcy, -dcx) with the host libm
void DyMuPathPlanner::slotsToPath(const double* r, uint64_t c, int status,
                                  const base::Waypoint& start, const base::Waypoint& sink,
                                  std::vector<base::Waypoint>& path) const {
  path.assign(c, base::Waypoint());
  for (uint64_t k = 0; k < c; ++k, r += 4) {
    base::Waypoint& w = path[k];
    if (status == 1 && k + 1 == c) {
      w = sink;
      continue;
    }
    if (k == 0) w = start;
    else w.heading = std::atan2(-r[3], -r[2]);
    w.position[0] = r[0];
    w.position[1] = r[1];
    const double gx = r[0] / global_res_, gy = r[1] / global_res_;
    unsigned cx = 0, cy = 0;
    if (path_cell(gx, nx_, cx) && path_cell(gy, ny_, cy)) {
      const double ax = gx - (double)cx, ay = gy - (double)cy;
      const uint64_t e = idx(cx, cy);
      w.position[2] = bilinear(ax, ay, elevation_[e], elevation_[e + 1], elevation_[e + nx_],
                               elevation_[e + nx_ + 1]);
    } else if (k > 0) {
      w.position[2] = 0.0;  // nextWaypoint left the default waypoint's z
    }
    w.position[0] += global_offset_[0];
    w.position[1] += global_offset_[1];
  }
}

// The device route: upload the starts, k_extract_paths, download the counts and
// statuses, then the waypoints written (runs of paths by pitched copies); z and the
// heading on the host threads.  The kernel's output has one fixed number of slots per path, and a caller's
// max_wp (2^20 by default) times thousands of paths is more memory than a path needs:
// the paths run in batches with a slot capacity sized from the grid, and those that
// overflow it (status -3 below max_wp) run again with four times the capacity.
void DyMuPathPlanner::pathsOnDevice(const std::vector<base::Waypoint>& starts,
                                    std::vector<std::vector<base::Waypoint>>& out,
                                    std::vector<int>& st, std::vector<int>& sinks,
                                    unsigned max_wp, unsigned stride,
                                    const PathTarget* target,
                                    std::vector<ArriveStats>* arrive) {
  constexpr uint64_t kOutBytes = 4ull << 30;  // device output of one batch, at most
  const size_t n = starts.size();
  DeviceQuery dq(*this, "getPaths", target);
  DeviceScratch& dev = dq.dev;
  auto check = [&](int rc, const char* what) { dq.check(rc, what); };
  const double* map = dq.map;
  const unsigned gi = dq.gi, gj = dq.gj;
  const bool gs = dq.gs;
  // the waypoints a path can end on, offsets added: the sink, or with a goal set (one sink
  // per path back) every goal's
  auto shifted = [&](base::Waypoint w) {
    w.position[0] += global_offset_[0];
    w.position[1] += global_offset_[1];
    return w;
  };
  const base::Waypoint sink = shifted(nodeSink(gi, gj, target ? target->heading : goal_heading_));
  std::vector<base::Waypoint> gsinks;
  if (gs)
    for (size_t k = 0; k < goals_.size(); ++k) gsinks.push_back(shifted(sinkWaypoint(k)));
  std::vector<int32_t> snk;
  // a straight descent across the grid is (nx + ny) / tau waypoints at most
  uint64_t cap = std::max<uint64_t>(1024, 4 * ((uint64_t)nx_ + ny_) / stride);
  cap = std::min<uint64_t>(cap, max_wp);
  std::vector<uint32_t> pending(n), again;
  for (size_t q = 0; q < n; ++q) pending[q] = (uint32_t)q;
  std::vector<double> raw;
  std::vector<int32_t> cnt, sts;
  std::vector<ArriveStats> recs;  // arrive: the batch's records (status and sink are theirs)
  std::vector<uint64_t> off, len;  // per path: its row in `raw` (waypoints), its count
  std::vector<RowRun> runs;
  while (!pending.empty()) {
    const uint64_t per_batch = std::max<uint64_t>(1, kOutBytes / (32 * cap));
    again.clear();
    for (size_t b0 = 0; b0 < pending.size(); b0 += per_batch) {
      const uint32_t m = (uint32_t)std::min<uint64_t>(per_batch, pending.size() - b0);
      const uint32_t* ids = &pending[b0];
      double* d_xy = dq.uploadStarts(starts, ids, m);
      int32_t* d_cnt = dev.alloc<int32_t>(m);
      int32_t* d_st = dev.alloc<int32_t>(m);
      double* d_out = dev.alloc<double>(4 * cap * m);
      int32_t* d_snk = gs && !arrive ? dev.alloc<int32_t>(m) : nullptr;
      ArriveStats* d_rec = arrive ? dev.alloc<ArriveStats>(m) : nullptr;
      if (arrive)
        check(dymu_arrive_paths_device(ctx_, map, nx_, ny_, nx_, global_res_, gi, gj, dq.labels(),
                                       dq.d_gxy, dq.goals(), dq.tau, d_xy, m, (uint32_t)cap,
                                       stride, d_out, d_cnt, d_rec, nullptr),
              "kernel");
      else if (gs)
        check(dymu_extract_paths_goals_device(ctx_, map, nx_, ny_, nx_, global_res_, dq.labels(),
                                              dq.d_gxy, dq.goals(), dq.tau, d_xy, m,
                                              (uint32_t)cap, stride, d_out, d_cnt, d_st, nullptr,
                                              d_snk),
              "kernel");
      else
        check(dymu_extract_paths_device(ctx_, map, nx_, ny_, nx_, global_res_, gi, gj, dq.tau,
                                        d_xy, m, (uint32_t)cap, stride, d_out, d_cnt, d_st,
                                        nullptr),
              "kernel");
      cnt.resize(m);
      sts.resize(m);
      snk.assign(m, 0);
      if (d_snk) check(dymu_memcpy_d2h(ctx_, snk.data(), d_snk, sizeof(int32_t) * m), "download");
      check(dymu_memcpy_d2h(ctx_, cnt.data(), d_cnt, sizeof(int32_t) * m), "download");
      if (arrive) {
        recs.resize(m);
        check(dymu_memcpy_d2h(ctx_, recs.data(), d_rec, sizeof(ArriveStats) * m), "download");
        for (uint32_t q = 0; q < m; ++q) {
          sts[q] = recs[q].status;
          snk[q] = recs[q].sink;
        }
      } else {
        check(dymu_memcpy_d2h(ctx_, sts.data(), d_st, sizeof(int32_t) * m), "download");
      }
      dq.addKernelMs(arrive ? &dymu_last_arrive_ms : &dymu_last_paths_ms);
      // the waypoints: runs of consecutive paths, each downloaded by one pitched copy
      // as wide as its longest path -- a run grows while that moves at most twice its
      // waypoints (plus 1024), so few commands move little more than the counts
      len.assign(m, 0);
      off.assign(m, 0);
      for (uint32_t q = 0; q < m; ++q) {
        const bool rerun = sts[q] == -3 && cap < max_wp;
        len[q] = rerun ? 0 : (uint64_t)std::max(cnt[q], 0);
        if (rerun) again.push_back(ids[q]);
      }
      const uint64_t total = planRowRuns(len, off, runs);
      raw.resize(4 * total);
      for (const RowRun& r : runs)
        if (r.width)
          check(dymu_memcpy2d_d2h(ctx_, &raw[4 * r.base], 32 * r.width, d_out + 4 * cap * r.q0,
                                  32 * cap, 32 * r.width, r.n),
                "download");
      for (void* p : {(void*)d_xy, (void*)d_cnt, (void*)d_st, (void*)d_out}) dev.release(p);
      if (d_snk) dev.release(d_snk);
      if (d_rec) dev.release(d_rec);
      // host post-pass (slotsToPath) on the host threads
      for_each_start(m, [&](size_t q) {
        const uint32_t id = ids[q];
        st[id] = sts[q];
        if (sts[q] == -3 && cap < max_wp) return;
        sinks[id] = sts[q] == 1 ? snk[q] : -1;
        if (arrive) (*arrive)[id] = recs[q];
        slotsToPath(raw.data() + 4 * off[q], len[q], sts[q], starts[id],
                    gs ? gsinks[(size_t)std::max(snk[q], 0)] : sink, out[id]);
      });
    }
    pending.swap(again);
    cap = std::min<uint64_t>(cap * 4, max_wp);
  }
}

// ---- the arriving descent (extension) ----
// null with an engine that predates the entry (tests/hostengine): the host route runs
#pragma weak dymu_arrive_paths_device
#pragma weak dymu_last_arrive_ms

namespace {
// The node of coordinate v (nearestIndex's rounding) on an axis of n nodes; false off the
// grid -- a negative or NaN coordinate included.  k_arrive_paths makes the same test.
bool arrive_node(double v, double res, unsigned n, unsigned& i) {
  if (!(v >= 0.0)) return false;
  const double h = v / res + 0.5;
  if (!(h < 4294967296.0)) return false;
  i = (unsigned)h;
  return i < n;
}
constexpr DyMuPathPlanner::ArriveStats kNoArrival{-1, -1, 0u, 0u, 0.0, 0.0};
}  // namespace

// The rule of include/dymu_fim.h (dymu_arrive_stat), which k_arrive_paths
// (arrive_kernels.hip) follows statement for statement: every expression here is formed
// there in the same order.
int DyMuPathPlanner::descendArriving(double x, double y, uint64_t max_wp, unsigned stride,
                                     std::vector<double>* slots, ArriveStats& rec,
                                     const double* eps, std::vector<uint32_t>* index) const {
  rec = kNoArrival;
  if (slots) slots->clear();
  if (index) index->clear();
  // eps: the rule of path_simplify.h as k_arrive_paths' simplified form applies it
  dymu::PathSimplifier sim;
  const double eps1 = eps ? *eps : 0.0, eps2 = eps1 * eps1;
  double qdx = 0, qdy = 0;  // the direction of the previous waypoint's slot
  auto keep = [&](double ex, double ey, double edx, double edy, uint32_t i) {
    if (slots) slots->insert(slots->end(), {ex, ey, edx, edy});
    if (index) index->push_back(i);
  };
  if (!has_goal_) return -1;
  const double res = global_res_, tau = std::min(0.4, risk_distance_);
  const double res_tau = res * tau, stall = 0.01 * tau * res;
  const uint64_t limit = max_wp > std::numeric_limits<uint64_t>::max() / stride
                             ? std::numeric_limits<uint64_t>::max()
                             : max_wp * stride;
  unsigned ni = 0, nj = 0;
  if (!arrive_node(x, res, nx_, ni) || !arrive_node(y, res, ny_, nj)) return -1;
  const bool gs = !goals_.empty();
  // T at the node (dj, di) away from (ni, nj); +inf off the grid, which no test accepts
  auto at = [&](int di, int dj) {
    const int64_t i = (int64_t)ni + di, j = (int64_t)nj + dj;
    return i < 0 || j < 0 || i >= (int64_t)nx_ || j >= (int64_t)ny_ ? kInf
                                                                    : T(idx((unsigned)i, (unsigned)j));
  };
  auto dist = [](double ax, double ay, double bx, double by) {
    const double dx = ax - bx, dy = ay - by;
    return std::sqrt(dx * dx + dy * dy);
  };
  // the sink of the node the path is on: the goal, or the goal labelled there (-1: none)
  double sink_x = res * (double)goal_i_, sink_y = res * (double)goal_j_;
  unsigned sni = goal_i_, snj = goal_j_;
  int sink_k = gs ? -1 : 0;
  auto track = [&] {
    if (!gs) return;
    const uint32_t lab = labels_[idx(ni, nj)];
    sink_k = lab < goals_.size() ? (int)lab : -1;
    if (sink_k < 0) return;
    const base::Waypoint s = sinkWaypoint(lab);
    sink_x = s.position[0];
    sink_y = s.position[1];
    if (!arrive_node(sink_x, res, nx_, sni) || !arrive_node(sink_y, res, ny_, snj))
      sni = snj = 0xffffffffu;  // a goal off the grid is no node's sink
  };
  track();
  if (!(at(0, 0) < kInf) || sink_k < 0) return -1;
  rec.start_cost = at(0, 0);
  int status = 0;
  uint64_t kept = 0;
  unsigned phase = 0, same = 0;
  double px = 0, py = 0, pdx = 0, pdy = 0;
  for (uint64_t w = 0;; ++w) {
    // waypoint w joins the record and, under the stride rule, the slots
    if (w > 0) rec.length = rec.length + dist(px, py, x, y);
    ++rec.count;
    if (phase == 0) {
      if (eps) {
        if (w == 0) {
          sim.anchor(x, y);
          keep(x, y, pdx, pdy, 0u);
        } else if (sim.next(px, py, x, y, eps1, eps2)) {
          keep(px, py, qdx, qdy, (uint32_t)w - 1u);
        }
        qdx = pdx;
        qdy = pdy;
      } else if (slots) {
        slots->insert(slots->end(), {x, y, pdx, pdy});
      }
      ++kept;
    }
    if (++phase == stride) phase = 0;
    px = x;
    py = y;
    // 1. arrived
    if (ni == sni && nj == snj && sink_k >= 0) {
      status = 1;
      break;
    }
    if (w + 1 == limit) {
      status = -3;
      break;
    }
    const double tn = at(0, 0);
    // 2. the continuous candidate (nextWaypoint's expressions) and its node m
    const double gx = x / res, gy = y / res;
    double cx_ = std::numeric_limits<double>::quiet_NaN(), cy_ = cx_, dcx = 0, dcy = 0;
    unsigned cx = 0, cy = 0;
    if (path_cell(gx, nx_, cx) && path_cell(gy, ny_, cy)) {
      const double ax = gx - (double)cx, ay = gy - (double)cy;
      double gx00, gx10, gx01, gx11, gy00, gy10, gy01, gy11;
      gradientNode(cx, cy, gx00, gy00);
      gradientNode(cx + 1, cy, gx10, gy10);
      gradientNode(cx, cy + 1, gx01, gy01);
      gradientNode(cx + 1, cy + 1, gx11, gy11);
      dcx = bilinear(ax, ay, gx00, gx01, gx10, gx11);
      dcy = bilinear(ax, ay, gy00, gy01, gy10, gy11);
      cx_ = x - res_tau * dcx;
      cy_ = y - res_tau * dcy;
    }
    unsigned mi = 0, mj = 0;
    bool take = dist(x, y, cx_, cy_) >= stall;  // false for a NaN candidate
    take = take && arrive_node(cx_, res, nx_, mi) && arrive_node(cy_, res, ny_, mj);
    int di = 0, dj = 0;
    if (take) {
      const int64_t ddi = (int64_t)mi - (int64_t)ni, ddj = (int64_t)mj - (int64_t)nj;
      take = ddi >= -1 && ddi <= 1 && ddj >= -1 && ddj <= 1;
      di = (int)ddi;
      dj = (int)ddj;
    }
    if (take) {
      const double tm = at(di, dj);
      take = tm < kInf;
      if (di == 0 && dj == 0) take = take && same < 8u;
      else take = take && tm < tn;
      if (di != 0 && dj != 0)  // no corner is cut: both side nodes are finite
        take = take && at(di, 0) < kInf && at(0, dj) < kInf;
    }
    if (take) {
      x = cx_;
      y = cy_;
      pdx = dcx;
      pdy = dcy;
      if (di == 0 && dj == 0) {
        ++same;
      } else {
        same = 0;
        ni = mi;
        nj = mj;
        track();
      }
      continue;
    }
    // 3. a hop to the neighbour of the steepest fall of T; the first of equal scores
    static const int kHop[8][2] = {{0, -1}, {-1, 0}, {1, 0}, {0, 1},
                                   {-1, -1}, {1, -1}, {-1, 1}, {1, 1}};
    double best = -1.0;
    int bi = 0, bj = 0;
    for (const auto& h : kHop) {
      const bool diag = h[0] != 0 && h[1] != 0;
      if (diag && !(at(h[0], 0) < kInf && at(0, h[1]) < kInf)) continue;
      const double tm = at(h[0], h[1]);
      if (!(tm < tn)) continue;
      const double s = diag ? (tn - tm) * 0.7071067811865476 : tn - tm;
      if (s > best) {
        best = s;
        bi = h[0];
        bj = h[1];
      }
    }
    if (bi == 0 && bj == 0) break;  // stalled: status 0
    ni = (unsigned)((int64_t)ni + bi);
    nj = (unsigned)((int64_t)nj + bj);
    x = res * (double)ni;
    y = res * (double)nj;
    pdx = (double)-bi;
    pdy = (double)-bj;
    same = 0;
    ++rec.hops;
    track();
  }
  // the last waypoint walked is kept; it is the anchor only where it is waypoint 0
  if (eps && rec.count >= 2u) keep(px, py, qdx, qdy, rec.count - 1u);
  if (status == 1) {
    if (kept < max_wp) {
      rec.length = rec.length + dist(px, py, sink_x, sink_y);
      ++rec.count;
      if (eps) keep(sink_x, sink_y, 0.0, 0.0, rec.count - 1u);
      else if (slots) slots->insert(slots->end(), {sink_x, sink_y, 0.0, 0.0});
    } else {
      status = -3;
    }
  }
  rec.status = status;
  rec.sink = status == 1 ? sink_k : -1;
  return status;
}

std::vector<std::vector<base::Waypoint>> DyMuPathPlanner::getArrivingPaths(
    const std::vector<base::Waypoint>& starts, std::vector<int>* status, unsigned max_wp,
    unsigned stride, std::vector<int>* sinks, std::vector<ArriveStats>* stats) {
  if (max_wp == 0 || stride == 0)
    throw std::invalid_argument("getArrivingPaths: max_wp, stride >= 1");
  const size_t n = starts.size();
  std::vector<std::vector<base::Waypoint>> out(n);
  std::vector<int> st(n, -1), sk(n, -1);
  std::vector<ArriveStats> rec(n, kNoArrival);
  last_paths_device_ = false;
  last_paths_kernel_ms_ = 0.0;
  if (n && has_goal_) {
    if (descentOnDevice() && n <= 0xffffffffull && &dymu_arrive_paths_device &&
        &dymu_last_arrive_ms) {
      pathsOnDevice(starts, out, st, sk, max_wp, stride, nullptr, &rec);
      last_paths_device_ = true;
    } else {
      if (!goals_.empty()) ensureHostLabels();
      for_each_start(n, [&](size_t q) {
        std::vector<double> slots;
        st[q] = descendArriving(starts[q].position[0] - global_offset_[0],
                                starts[q].position[1] - global_offset_[1], max_wp, stride, &slots,
                                rec[q]);
        sk[q] = rec[q].sink;
        base::Waypoint end = !goals_.empty() && sk[q] >= 0
                                 ? sinkWaypoint((size_t)sk[q])
                                 : nodeSink(goal_i_, goal_j_, goal_heading_);
        end.position[0] += global_offset_[0];
        end.position[1] += global_offset_[1];
        slotsToPath(slots.data(), slots.size() / 4, st[q], starts[q], end, out[q]);
      });
    }
  }
  if (status) status->swap(st);
  if (sinks) sinks->swap(sk);
  if (stats) stats->swap(rec);
  return out;
}

std::vector<DyMuPathPlanner::ArriveStats> DyMuPathPlanner::getArrivingStats(
    const std::vector<base::Waypoint>& starts, unsigned max_wp, bool host) {
  if (max_wp == 0) throw std::invalid_argument("getArrivingStats: max_wp >= 1");
  const size_t n = starts.size();
  std::vector<ArriveStats> out(n, kNoArrival);
  last_paths_device_ = false;
  last_paths_kernel_ms_ = 0.0;
  if (!n || !has_goal_) return out;
  if (!host && descentOnDevice() && n <= 0xffffffffull && max_wp <= 0x7fffffffu &&
      &dymu_arrive_paths_device && &dymu_last_arrive_ms) {
    arriveStatsOnDevice(starts, out, max_wp, nullptr);
    last_paths_device_ = true;
    return out;
  }
  if (!goals_.empty()) ensureHostLabels();
  for_each_start(n, [&](size_t q) {
    (void)descendArriving(starts[q].position[0] - global_offset_[0],
                          starts[q].position[1] - global_offset_[1], max_wp, 1, nullptr, out[q]);
  });
  return out;
}

// The device route of the records: the starts up, one k_arrive_paths launch that stores
// no waypoint, the records down.
void DyMuPathPlanner::arriveStatsOnDevice(const std::vector<base::Waypoint>& starts,
                                          std::vector<ArriveStats>& out, unsigned max_wp,
                                          const PathTarget* target) {
  const size_t n = starts.size();
  DeviceQuery dq(*this, "getArrivingStats", target);
  double* d_xy = dq.uploadStarts(starts, nullptr, n);
  ArriveStats* d_rec = dq.dev.alloc<ArriveStats>(n);
  dq.check(dymu_arrive_paths_device(ctx_, dq.map, nx_, ny_, nx_, global_res_, dq.gi, dq.gj,
                                    dq.labels(), dq.d_gxy, dq.goals(), dq.tau, d_xy, (uint32_t)n,
                                    max_wp, 1, nullptr, nullptr, d_rec, nullptr),
           "kernel");
  dq.check(dymu_memcpy_d2h(ctx_, out.data(), d_rec, sizeof(ArriveStats) * n), "download");
  dq.addKernelMs(&dymu_last_arrive_ms);
}

// ---- getSimplifiedPaths: arriving paths thinned within a bound (extension) ----
// null with an engine that predates the entry (tests/hostengine): the host route runs
#pragma weak dymu_arrive_simplified_device
#pragma weak dymu_last_arrive_simplified_ms

namespace {
void simplified_check(const char* who, double eps, unsigned max_wp) {
  if (!(eps > 0) || !(eps < std::numeric_limits<double>::infinity()) || max_wp == 0)
    throw std::invalid_argument(std::string(who) + ": eps > 0 and finite, max_wp >= 1");
}
}  // namespace

std::vector<std::vector<base::Waypoint>> DyMuPathPlanner::getSimplifiedPaths(
    const std::vector<base::Waypoint>& starts, double eps, std::vector<int>* status,
    unsigned max_wp, std::vector<int>* sinks, std::vector<ArriveStats>* stats,
    std::vector<std::vector<uint32_t>>* index) {
  simplified_check("getSimplifiedPaths", eps, max_wp);
  const size_t n = starts.size();
  std::vector<std::vector<base::Waypoint>> out(n);
  std::vector<int> st(n, -1), sk(n, -1);
  std::vector<ArriveStats> rec(n, kNoArrival);
  if (index) index->assign(n, std::vector<uint32_t>());
  last_paths_device_ = false;
  last_paths_kernel_ms_ = 0.0;
  last_simplified_reruns_ = last_simplified_bytes_ = 0;
  if (n && has_goal_) {
    if (descentOnDevice() && n <= 0xffffffffull && max_wp <= 0x7fffffffu &&
        &dymu_arrive_simplified_device && &dymu_last_arrive_simplified_ms) {
      simplifiedOnDevice(starts, eps, out, st, sk, max_wp, nullptr, rec, index);
      last_paths_device_ = true;
    } else {
      if (!goals_.empty()) ensureHostLabels();
      for_each_start(n, [&](size_t q) {
        std::vector<double> slots;
        st[q] = descendArriving(starts[q].position[0] - global_offset_[0],
                                starts[q].position[1] - global_offset_[1], max_wp, 1, &slots,
                                rec[q], &eps, index ? &(*index)[q] : nullptr);
        sk[q] = rec[q].sink;
        base::Waypoint end = !goals_.empty() && sk[q] >= 0
                                 ? sinkWaypoint((size_t)sk[q])
                                 : nodeSink(goal_i_, goal_j_, goal_heading_);
        end.position[0] += global_offset_[0];
        end.position[1] += global_offset_[1];
        slotsToPath(slots.data(), slots.size() / 4, st[q], starts[q], end, out[q]);
      });
    }
  }
  if (status) status->swap(st);
  if (sinks) sinks->swap(sk);
  if (stats) stats->swap(rec);
  return out;
}

// The device route: the starts up, one simplified k_arrive_paths launch per batch, the
// records and the counts down, then only the slots (and numbers) the rule kept, by
// pathsOnDevice's pitched copies; z and the heading on the host threads.  The kernel
// counts every waypoint the rule keeps and stores the first `cap` of them.  The first cap
// is a guess from the grid and eps (below), and a path that kept more runs once more, with
// the largest count reported as the capacity: the rule is deterministic, so the second run
// fits exactly.
void DyMuPathPlanner::simplifiedOnDevice(const std::vector<base::Waypoint>& starts, double eps,
                                         std::vector<std::vector<base::Waypoint>>& out,
                                         std::vector<int>& st, std::vector<int>& sinks,
                                         unsigned max_wp, const PathTarget* target,
                                         std::vector<ArriveStats>& rec,
                                         std::vector<std::vector<uint32_t>>* index) {
  constexpr uint64_t kOutBytes = 4ull << 30;  // device output of one batch, at most
  const size_t n = starts.size();
  DeviceQuery dq(*this, "getSimplifiedPaths", target);
  DeviceScratch& dev = dq.dev;
  auto check = [&](int rc, const char* what) { dq.check(rc, what); };
  auto shifted = [&](base::Waypoint w) {
    w.position[0] += global_offset_[0];
    w.position[1] += global_offset_[1];
    return w;
  };
  const base::Waypoint sink =
      shifted(nodeSink(dq.gi, dq.gj, target ? target->heading : goal_heading_));
  std::vector<base::Waypoint> gsinks;
  if (dq.gs)
    for (size_t k = 0; k < goals_.size(); ++k) gsinks.push_back(shifted(sinkWaypoint(k)));
  // The first capacity, a guess: a long path walks about nx + ny waypoints (a diagonal
  // from a corner to the middle at 0.4 cell a step) and the rule keeps about one in
  // 16 sqrt(eps in cells) of them on the maps measured, eps taken between
  // 1/64 and 64 cells; 64 slots at the least.  A path keeps at most max_wp waypoints: the
  // sink follows fewer than max_wp walked.
  const double eps_cells = std::min(64.0, std::max(1.0 / 64.0, eps / global_res_));
  uint64_t cap = (uint64_t)((double)((uint64_t)nx_ + ny_) / (16.0 * std::sqrt(eps_cells)));
  cap = std::min<uint64_t>(std::max<uint64_t>(64, cap), max_wp);
  const uint64_t slot_bytes = 32 + (index ? 4 : 0);
  std::vector<uint32_t> pending(n), again, idx;
  for (size_t q = 0; q < n; ++q) pending[q] = (uint32_t)q;
  std::vector<double> raw;
  std::vector<int32_t> cnt;
  std::vector<ArriveStats> recs;
  std::vector<uint64_t> off, len;
  std::vector<RowRun> runs;
  for (int round = 0; !pending.empty(); ++round) {
    const uint64_t per_batch = std::max<uint64_t>(1, kOutBytes / (slot_bytes * cap));
    again.clear();
    uint64_t next_cap = 0;
    for (size_t b0 = 0; b0 < pending.size(); b0 += per_batch) {
      const uint32_t m = (uint32_t)std::min<uint64_t>(per_batch, pending.size() - b0);
      const uint32_t* ids = &pending[b0];
      double* d_xy = dq.uploadStarts(starts, ids, m);
      int32_t* d_cnt = dev.alloc<int32_t>(m);
      ArriveStats* d_rec = dev.alloc<ArriveStats>(m);
      double* d_out = dev.alloc<double>(4 * cap * m);
      uint32_t* d_idx = index ? dev.alloc<uint32_t>(cap * m) : nullptr;
      check(dymu_arrive_simplified_device(ctx_, dq.map, nx_, ny_, nx_, global_res_, dq.gi, dq.gj,
                                          dq.labels(), dq.d_gxy, dq.goals(), dq.tau, d_xy, m, eps,
                                          max_wp, (uint32_t)cap, d_out, d_idx, d_cnt, d_rec,
                                          nullptr),
            "kernel");
      cnt.resize(m);
      recs.resize(m);
      check(dymu_memcpy_d2h(ctx_, cnt.data(), d_cnt, sizeof(int32_t) * m), "download");
      check(dymu_memcpy_d2h(ctx_, recs.data(), d_rec, sizeof(ArriveStats) * m), "download");
      last_simplified_bytes_ += (sizeof(int32_t) + sizeof(ArriveStats)) * (uint64_t)m;
      dq.addKernelMs(&dymu_last_arrive_simplified_ms);
      len.assign(m, 0);
      for (uint32_t q = 0; q < m; ++q) {
        const uint64_t c = (uint64_t)std::max(cnt[q], 0);
        if (c > cap) {
          if (round > 0) throw std::runtime_error("dymu: getSimplifiedPaths: a rerun overflowed");
          again.push_back(ids[q]);
          next_cap = std::max(next_cap, c);
        } else {
          len[q] = c;
        }
      }
      const uint64_t total = planRowRuns(len, off, runs);
      raw.resize(4 * total);
      if (index) idx.resize(total);
      for (const RowRun& r : runs) {
        if (!r.width) continue;
        check(dymu_memcpy2d_d2h(ctx_, &raw[4 * r.base], 32 * r.width, d_out + 4 * cap * r.q0,
                                32 * cap, 32 * r.width, r.n),
              "download");
        if (index)
          check(dymu_memcpy2d_d2h(ctx_, &idx[r.base], 4 * r.width, d_idx + cap * r.q0, 4 * cap,
                                  4 * r.width, r.n),
                "download");
        last_simplified_bytes_ += slot_bytes * r.width * r.n;
      }
      for (void* p : {(void*)d_xy, (void*)d_cnt, (void*)d_rec, (void*)d_out}) dev.release(p);
      if (d_idx) dev.release(d_idx);
      for_each_start(m, [&](size_t q) {
        if ((uint64_t)std::max(cnt[q], 0) > cap) return;
        const uint32_t id = ids[q];
        st[id] = recs[q].status;
        sinks[id] = recs[q].sink;
        rec[id] = recs[q];
        slotsToPath(raw.data() + 4 * off[q], len[q], st[id], starts[id],
                    dq.gs ? gsinks[(size_t)std::max(sinks[id], 0)] : sink, out[id]);
        if (index) (*index)[id].assign(idx.begin() + off[q], idx.begin() + off[q] + len[q]);
      });
    }
    last_simplified_reruns_ += again.size();
    pending.swap(again);
    cap = next_cap;
  }
}

// ---- getPathStats: per-path summaries (extension) ----
#pragma weak dymu_path_stats_device
#pragma weak dymu_last_path_stats_ms

std::vector<DyMuPathPlanner::PathStats> DyMuPathPlanner::getPathStats(
    const std::vector<base::Waypoint>& starts, unsigned max_wp, const double* field, bool host) {
  if (max_wp == 0) throw std::invalid_argument("getPathStats: max_wp >= 1");
  const size_t n = starts.size();
  std::vector<PathStats> out(n, PathAccum::empty());
  last_paths_device_ = false;
  last_paths_kernel_ms_ = 0.0;
  if (!n || !has_goal_) return out;
  if (!host && descentOnDevice() && dF_ && speed_valid_ && n <= 0x7fffffffull &&
      max_wp <= 0x7fffffffu && &dymu_path_stats_device && &dymu_last_path_stats_ms) {
    pathStatsOnDevice(starts, out, max_wp, field, nullptr);
    last_paths_device_ = true;
    return out;
  }
  if (!goals_.empty()) ensureHostLabels();
  if (!speed_valid_) syncGlobalRisk();
  const double* f0 = speed_valid_ ? speed_.data() : nullptr;
  for_each_start(n, [&](size_t q) {
    std::vector<base::Waypoint> none;  // stays empty: the waypoints join acc
    base::Waypoint w = starts[q];
    w.position[0] -= global_offset_[0];
    w.position[1] -= global_offset_[1];
    PathAccum acc;
    acc.nf = field ? 2u : 1u;
    acc.f[0] = f0;
    acc.f[1] = field;
    int sink = -1;
    const int st = descend(w, none, max_wp, 1, &sink, &acc);
    if (st == -1) return;  // the empty record
    acc.r.status = st;
    acc.r.sink = st == 1 ? sink : -1;
    out[q] = acc.r;
  });
  return out;
}

// The device route: the starts up, one k_path_stats launch, the records down.  The
// caller's field goes through d_pfield_, a buffer of the map's size that is allocated
// once and lives as long as the map buffers.
void DyMuPathPlanner::pathStatsOnDevice(const std::vector<base::Waypoint>& starts,
                                        std::vector<PathStats>& out, unsigned max_wp,
                                        const double* field, const PathTarget* target) {
  const size_t n = starts.size();
  DeviceQuery dq(*this, "getPathStats", target);
  if (field) {
    if (!d_pfield_) {
      void* p = nullptr;
      dq.check(dymu_device_alloc(ctx_, sizeof(double) * dcells_, &p), "field allocation");
      d_pfield_ = static_cast<double*>(p);
    }
    dq.check(dymu_memcpy_h2d(ctx_, d_pfield_, field, sizeof(double) * dcells_), "field upload");
  }
  double* d_xy = dq.uploadStarts(starts, nullptr, n);
  PathStats* d_rec = dq.dev.alloc<PathStats>(n);
  const double* fields[2] = {dF_, d_pfield_};
  const uint64_t pitch[2] = {nx_, nx_};
  dq.check(dymu_path_stats_device(ctx_, dq.map, nx_, ny_, nx_, global_res_, dq.gi, dq.gj,
                                  dq.labels(), dq.d_gxy, dq.goals(), dq.tau, d_xy, (uint32_t)n,
                                  max_wp, fields, pitch, field ? 2u : 1u, 0u, d_rec, nullptr),
           "kernel");
  dq.check(dymu_memcpy_d2h(ctx_, out.data(), d_rec, sizeof(PathStats) * n), "download");
  dq.addKernelMs(&dymu_last_path_stats_ms);
}

// ---- getRouteFields: every cell's node route at once (extension) ----
#pragma weak dymu_route_fields_device
#pragma weak dymu_route_fields_workspace
#pragma weak dymu_last_route_fields_ms
#pragma weak dymu_device_alloc_cached

namespace {
// include/dymu_fim.h's minimum and maximum: -0.0 below +0.0, so the order of folds does not show
inline double route_min(double a, double b) { return (b < a || (b == a && std::signbit(b))) ? b : a; }
inline double route_max(double a, double b) { return (b > a || (b == a && !std::signbit(b))) ? b : a; }
inline bool route_finite(double v) { return v > -kInf && v < kInf; }
// include/dymu_fim.h's rp(c) on a row-major nx x ny map t, for a node with t[c] < +inf: the
// hop target of the arriving descent evaluated at c, or -1 for a dead end; *diag = whether
// the hop is diagonal.  getRouteFields' and getRouteUsage's host routes share it.
int64_t route_parent(const double* t, int64_t nx, int64_t ny, uint64_t c, bool* diag) {
  const int64_t i = (int64_t)(c % (uint64_t)nx), j = (int64_t)(c / (uint64_t)nx);
  const double tn = t[c];
  // a neighbour off the grid is +inf: no test accepts it
  auto at = [&](int di, int dj) {
    const int64_t a = i + di, b = j + dj;
    return a >= 0 && a < nx && b >= 0 && b < ny ? t[b * nx + a] : kInf;
  };
  double best = -1.0;
  int bi = 0, bj = 0;
  auto hop_try = [&](bool ok, int di, int dj) {
    const double tm = at(di, dj);
    if (ok && tm < tn) {
      const double s = (di && dj) ? (tn - tm) * 0.7071067811865476 : tn - tm;
      if (s > best) best = s, bi = di, bj = dj;
    }
  };
  const bool w = at(-1, 0) < kInf, ea = at(1, 0) < kInf, s = at(0, -1) < kInf,
             no = at(0, 1) < kInf;
  hop_try(true, 0, -1);
  hop_try(true, -1, 0);
  hop_try(true, 1, 0);
  hop_try(true, 0, 1);
  hop_try(w && s, -1, -1);
  hop_try(ea && s, 1, -1);
  hop_try(w && no, -1, 1);
  hop_try(ea && no, 1, 1);
  if (bi == 0 && bj == 0) return -1;
  *diag = bi != 0 && bj != 0;
  return (j + bj) * nx + (i + bi);
}
void route_check_request(const DyMuPathPlanner::RouteRequest& rq) {
  if (rq.fields.size() > DYMU_PATH_FIELDS)
    throw std::invalid_argument("getRouteFields: at most DYMU_PATH_FIELDS fields");
}
// the output maps of a request, every cell without a route
void route_empty(const DyMuPathPlanner::RouteRequest& rq, uint64_t n,
                 DyMuPathPlanner::RouteFields& out) {
  typedef DyMuPathPlanner P;
  const size_t nf = rq.fields.size();
  if (rq.outputs & P::kRouteSink) out.sink.assign(n, DYMU_LABEL_NONE);
  if (rq.outputs & P::kRouteAxis) out.axis.assign(n, 0u);
  if (rq.outputs & P::kRouteDiag) out.diag.assign(n, 0u);
  if (rq.outputs & P::kRouteLength) out.length.assign(n, std::nan(""));
  if (rq.outputs & P::kRouteIntegral)
    out.integral.assign(nf, std::vector<double>(n, std::nan("")));
  if (rq.outputs & P::kRouteMin) out.vmin.assign(nf, std::vector<double>(n, kInf));
  if (rq.outputs & P::kRouteMax) out.vmax.assign(nf, std::vector<double>(n, -kInf));
}
}  // namespace

DyMuPathPlanner::RouteFields DyMuPathPlanner::getRouteFields(const RouteRequest& rq) {
  route_check_request(rq);
  RouteFields out;
  last_paths_device_ = false;
  last_paths_kernel_ms_ = 0.0;
  const uint64_t n = (uint64_t)nx_ * ny_;
  if (!n || !has_goal_) {
    route_empty(rq, n, out);
    return out;
  }
  bool speed = false;
  for (const double* f : rq.fields) speed = speed || !f;
  if (!rq.host && ctx_ && dT_ && dev_map_current_ && n < (1ull << 31) &&
      (!speed || (dF_ && speed_valid_)) && &dymu_route_fields_device &&
      &dymu_route_fields_workspace && &dymu_last_route_fields_ms && &dymu_device_alloc_cached) {
    routeFieldsOnDevice(rq, dT_, seedList(), out);
    last_paths_device_ = true;
    return out;
  }
  routeFieldsOnHost(rq, out);
  return out;
}

// The definition of include/dymu_fim.h on the host mirror: roots first, then the finite
// cells in ascending total cost, each from its parent (a parent is strictly lower, so it
// is done by then) -- the integral as w(c) + integral[rp(c)].
void DyMuPathPlanner::routeFieldsOnHost(const RouteRequest& rq, RouteFields& out) {
  const uint64_t n = (uint64_t)nx_ * ny_;
  const size_t nf = rq.fields.size();
  fetchAll();
  const double* t = total_cost_.data();
  // a null field is the speed map the solve used (getPathStats' slot 0): the packed copy,
  // or without one the node's own speed, as the host descent's record takes it
  bool speed = false;
  for (const double* f : rq.fields) speed = speed || !f;
  if (speed && !speed_valid_) syncGlobalRisk();
  const double* f0 = speed_valid_ ? speed_.data() : nullptr;
  std::vector<const double*> fld(rq.fields);
  for (const double*& f : fld)
    if (!f) f = f0;
  // the whole record is kept while the pass runs; what was not asked for is dropped after
  std::vector<uint32_t> sink(n, DYMU_LABEL_NONE), axis(n, 0u), diag(n, 0u);
  std::vector<std::vector<double>> integ(nf, std::vector<double>(n, 0.0)),
      vmin(nf, std::vector<double>(n, kInf)), vmax(nf, std::vector<double>(n, -kInf));
  auto sample = [&](size_t f, uint64_t c, double& v) {
    v = fld[f] ? fld[f][c] : is_obstacle_[c] ? kInf : nodeSpeed(c);
    return route_finite(v);
  };
  const std::vector<dymu_seed> seeds = seedList();
  std::vector<uint8_t> root(n, 0);
  for (size_t k = seeds.size(); k-- > 0;) {  // descending: the lowest k is written last
    const uint64_t c = idx(seeds[k].i, seeds[k].j);
    if (std::memcmp(&t[c], &seeds[k].t0, sizeof(double)) != 0) continue;  // dominated
    sink[c] = (uint32_t)k;
    root[c] = 1;
  }
  for (uint64_t c = 0; c < n; ++c)
    if (root[c])
      for (size_t f = 0; f < nf; ++f) {
        double v;
        if (sample(f, c, v)) vmin[f][c] = vmax[f][c] = v;
      }
  std::vector<std::pair<double, uint64_t>> order;
  for (uint64_t c = 0; c < n; ++c)
    if (t[c] < kInf && !root[c]) order.emplace_back(t[c], c);
  parallel_sort(order);
  const double seg_d = global_res_ * 1.4142135623730951;
  const int64_t nx = nx_, ny = ny_;
  for (const auto& e : order) {
    const uint64_t c = e.second;
    bool dg = false;
    const int64_t rp = route_parent(t, nx, ny, c, &dg);
    if (rp < 0) continue;  // a dead end
    const uint64_t p = (uint64_t)rp;
    if (sink[p] == DYMU_LABEL_NONE) continue;  // drains to a dead end
    sink[c] = sink[p];
    axis[c] = axis[p] + (dg ? 0u : 1u);
    diag[c] = diag[p] + (dg ? 1u : 0u);
    const double seg = dg ? seg_d : global_res_;
    for (size_t f = 0; f < nf; ++f) {
      double v = 0.0;
      const bool cnt = sample(f, c, v);
      integ[f][c] = (cnt ? v * seg : 0.0) + integ[f][p];
      vmin[f][c] = route_min(cnt ? v : kInf, vmin[f][p]);
      vmax[f][c] = route_max(cnt ? v : -kInf, vmax[f][p]);
    }
  }
  if (rq.outputs & kRouteLength) {
    out.length.resize(n);
    for (uint64_t c = 0; c < n; ++c)
      out.length[c] = sink[c] == DYMU_LABEL_NONE
                          ? std::nan("")
                          : global_res_ * (double)axis[c] + seg_d * (double)diag[c];
  }
  for (uint64_t c = 0; c < n; ++c)
    if (sink[c] == DYMU_LABEL_NONE)
      for (size_t f = 0; f < nf; ++f) {
        integ[f][c] = std::nan("");
        vmin[f][c] = kInf;
        vmax[f][c] = -kInf;
      }
  if (rq.outputs & kRouteSink) out.sink.swap(sink);
  if (rq.outputs & kRouteAxis) out.axis.swap(axis);
  if (rq.outputs & kRouteDiag) out.diag.swap(diag);
  if (rq.outputs & kRouteIntegral) out.integral.swap(integ);
  if (rq.outputs & kRouteMin) out.vmin.swap(vmin);
  if (rq.outputs & kRouteMax) out.vmax.swap(vmax);
}

// The device route: the caller's fields up, dymu_route_fields_device into the planner's
// output maps, the requested maps down.
void DyMuPathPlanner::routeFieldsOnDevice(const RouteRequest& rq, const double* map,
                                          const std::vector<dymu_seed>& seeds, RouteFields& out) {
  const uint64_t n = (uint64_t)nx_ * ny_;
  const uint32_t nf = (uint32_t)rq.fields.size();
  auto check = [&](int rc, const char* what) {
    if (rc != DYMU_OK)
      throw std::runtime_error(std::string("dymu: getRouteFields ") + what + " failed: " +
                               dymu_strerror(rc) + " " + dymu_last_error(ctx_));
  };
  auto ensure = [&](auto*& p, size_t elem) {
    if (p) return;
    void* q = nullptr;
    check(dymu_device_alloc_cached(ctx_, elem * dcells_, &q), "allocation");
    p = static_cast<std::remove_reference_t<decltype(p)>>(q);
  };
  const double* fields[DYMU_PATH_FIELDS] = {};
  uint64_t pitch[DYMU_PATH_FIELDS] = {};
  for (uint32_t f = 0; f < nf; ++f) {
    pitch[f] = nx_;
    if (!rq.fields[f]) {
      fields[f] = dF_;
      continue;
    }
    ensure(d_rfield_[f], sizeof(double));
    check(dymu_memcpy_h2d(ctx_, d_rfield_[f], rq.fields[f], sizeof(double) * n), "field upload");
    fields[f] = d_rfield_[f];
  }
  dymu_route_out o{};
  o.ld = nx_;
  const uint32_t ubit[3] = {kRouteSink, kRouteAxis, kRouteDiag};
  uint32_t** const uout[3] = {&o.sink, &o.axis, &o.diag};
  for (int k = 0; k < 3; ++k)
    if (rq.outputs & ubit[k]) {
      ensure(d_rout_u_[k], sizeof(uint32_t));
      *uout[k] = d_rout_u_[k];
    }
  if (rq.outputs & kRouteLength) {
    ensure(d_rout_len_, sizeof(double));
    o.length = d_rout_len_;
  }
  const uint32_t fbit[3] = {kRouteIntegral, kRouteMin, kRouteMax};
  double** const fout[3] = {o.integral, o.vmin, o.vmax};
  for (int k = 0; k < 3; ++k)
    for (uint32_t f = 0; f < nf; ++f)
      if (rq.outputs & fbit[k]) {
        ensure(d_rout_f_[k][f], sizeof(double));
        fout[k][f] = d_rout_f_[k][f];
      }
  const size_t need = dymu_route_fields_workspace(nx_, ny_, nf, &o);
  if (!need) check(DYMU_ERR_ARG, "workspace query");
  if (need > route_ws_bytes_) {
    if (d_route_ws_) (void)dymu_device_free(ctx_, d_route_ws_);
    d_route_ws_ = nullptr;
    route_ws_bytes_ = 0;
    check(dymu_device_alloc_cached(ctx_, need, &d_route_ws_), "workspace allocation");
    route_ws_bytes_ = need;
  }
  check(dymu_route_fields_device(ctx_, map, nx_, ny_, nx_, global_res_, seeds.data(),
                                 (uint32_t)seeds.size(), fields, pitch, nf, &o, d_route_ws_,
                                 route_ws_bytes_, nullptr, &out.rounds),
        "kernels");
  auto down = [&](auto& v, const void* d) {
    v.resize(n);
    check(dymu_memcpy_d2h(ctx_, v.data(), d, sizeof(v[0]) * n), "download");
  };
  if (o.sink) down(out.sink, o.sink);
  if (o.axis) down(out.axis, o.axis);
  if (o.diag) down(out.diag, o.diag);
  if (o.length) down(out.length, o.length);
  std::vector<std::vector<double>>* const hv[3] = {&out.integral, &out.vmin, &out.vmax};
  for (int k = 0; k < 3; ++k)
    if (rq.outputs & fbit[k]) {
      hv[k]->resize(nf);
      for (uint32_t f = 0; f < nf; ++f) down((*hv[k])[f], fout[k][f]);
    }
  double ms = 0.0;
  if (dymu_last_route_fields_ms(ctx_, &ms) == DYMU_OK) last_paths_kernel_ms_ = ms;
}

void DyMuPathPlanner::dropRouteBuffers() {
  auto drop = [&](auto*& p) {
    if (p && ctx_) (void)dymu_device_free(ctx_, p);
    p = nullptr;
  };
  for (auto& p : d_rfield_) drop(p);
  for (auto& p : d_rout_u_) drop(p);
  drop(d_rout_len_);
  for (auto& row : d_rout_f_)
    for (auto& p : row) drop(p);
  drop(d_route_ws_);
  route_ws_bytes_ = 0;
  drop(d_uweight_);
  drop(d_uout_usage_);
  drop(d_uout_far_);
  drop(d_uout_sink_);
  drop(d_usage_ws_);
  usage_ws_bytes_ = 0;
}

// ---- getRouteUsage: how much of the map drains through every cell (extension) ----
#pragma weak dymu_route_usage_device
#pragma weak dymu_route_usage_workspace
#pragma weak dymu_last_route_usage_ms

DyMuPathPlanner::RouteUsage DyMuPathPlanner::getRouteUsage(const RouteUsageRequest& rq) {
  RouteUsage out;
  last_paths_device_ = false;
  last_paths_kernel_ms_ = 0.0;
  const uint64_t n = (uint64_t)nx_ * ny_;
  if (!n || !has_goal_) {  // every cell is without a route; no goal, no catchment
    if (rq.outputs & kUsageUsage) out.usage.assign(n, 0u);
    if (rq.outputs & kUsageFar) out.far.assign(n, std::nan(""));
    if (rq.outputs & kUsageSink) out.sink.assign(n, DYMU_LABEL_NONE);
    return out;
  }
  if (!rq.host && (rq.outputs & kUsageAll) && ctx_ && dT_ && dev_map_current_ &&
      n < (1ull << 31) && &dymu_route_usage_device && &dymu_route_usage_workspace &&
      &dymu_last_route_usage_ms && &dymu_device_alloc_cached) {
    routeUsageOnDevice(rq, dT_, seedList(), out);
    last_paths_device_ = true;
    return out;
  }
  routeUsageOnHost(rq, out);
  return out;
}

// The definition of include/dymu_fim.h on the host mirror: the finite cells in descending
// total cost, each added into its parent (a child is strictly higher, so it is complete by
// then); the same order backwards hands the sinks down from the roots.
void DyMuPathPlanner::routeUsageOnHost(const RouteUsageRequest& rq, RouteUsage& out) {
  const uint64_t n = (uint64_t)nx_ * ny_;
  fetchAll();
  const double* t = total_cost_.data();
  const std::vector<dymu_seed> seeds = seedList();
  std::vector<uint32_t> sink(n, DYMU_LABEL_NONE);
  std::vector<uint8_t> root(n, 0);
  for (size_t k = seeds.size(); k-- > 0;) {  // descending: the lowest k is written last
    const uint64_t c = idx(seeds[k].i, seeds[k].j);
    if (std::memcmp(&t[c], &seeds[k].t0, sizeof(double)) != 0) continue;  // dominated
    sink[c] = (uint32_t)k;
    root[c] = 1;
  }
  std::vector<std::pair<double, uint64_t>> order;
  for (uint64_t c = 0; c < n; ++c)
    if (t[c] < kInf && !root[c]) order.emplace_back(t[c], c);
  parallel_sort(order);
  std::vector<uint64_t> usage(n, 0u);
  std::vector<double> far(n, 0.0);
  for (uint64_t c = 0; c < n; ++c)
    if (t[c] < kInf) {
      usage[c] = rq.weights ? rq.weights[c] : 1u;
      far[c] = t[c];
    }
  // parent[k] of order[k]; n: none
  std::vector<uint64_t> parent(order.size(), n);
  const int64_t nx = nx_, ny = ny_;
  for (size_t k = order.size(); k-- > 0;) {
    const uint64_t c = order[k].second;
    bool dg = false;
    const int64_t p = route_parent(t, nx, ny, c, &dg);
    if (p < 0) continue;  // a dead end
    parent[k] = (uint64_t)p;
    usage[p] += usage[c];
    if (far[c] > far[p]) far[p] = far[c];
  }
  for (size_t k = 0; k < order.size(); ++k)
    if (parent[k] != n) sink[order[k].second] = sink[parent[k]];
  for (uint64_t c = 0; c < n; ++c)
    if (sink[c] == DYMU_LABEL_NONE) {
      usage[c] = 0u;
      far[c] = std::nan("");
    }
  if (rq.outputs & kUsageCatchment) {
    out.catchment.assign(seeds.size(), 0u);
    for (size_t k = 0; k < seeds.size(); ++k) {
      const uint64_t c = idx(seeds[k].i, seeds[k].j);
      if (root[c] && sink[c] == (uint32_t)k) out.catchment[k] = usage[c];
    }
  }
  if (rq.outputs & kUsageUsage) out.usage.swap(usage);
  if (rq.outputs & kUsageFar) out.far.swap(far);
  if (rq.outputs & kUsageSink) out.sink.swap(sink);
}

// The device route: the caller's weights up, dymu_route_usage_device into the planner's
// output maps, the requested maps down.
void DyMuPathPlanner::routeUsageOnDevice(const RouteUsageRequest& rq, const double* map,
                                         const std::vector<dymu_seed>& seeds, RouteUsage& out) {
  const uint64_t n = (uint64_t)nx_ * ny_;
  auto check = [&](int rc, const char* what) {
    if (rc != DYMU_OK)
      throw std::runtime_error(std::string("dymu: getRouteUsage ") + what + " failed: " +
                               dymu_strerror(rc) + " " + dymu_last_error(ctx_));
  };
  auto ensure = [&](auto*& p, size_t elem) {
    if (p) return;
    void* q = nullptr;
    check(dymu_device_alloc_cached(ctx_, elem * dcells_, &q), "allocation");
    p = static_cast<std::remove_reference_t<decltype(p)>>(q);
  };
  if (rq.weights) {
    ensure(d_uweight_, sizeof(uint32_t));
    check(dymu_memcpy_h2d(ctx_, d_uweight_, rq.weights, sizeof(uint32_t) * n), "weight upload");
  }
  dymu_usage_out o{};
  o.ld = nx_;
  if (rq.outputs & kUsageUsage) {
    ensure(d_uout_usage_, sizeof(uint64_t));
    o.usage = d_uout_usage_;
  }
  if (rq.outputs & kUsageFar) {
    ensure(d_uout_far_, sizeof(double));
    o.far = d_uout_far_;
  }
  if (rq.outputs & kUsageSink) {
    ensure(d_uout_sink_, sizeof(uint32_t));
    o.sink = d_uout_sink_;
  }
  const bool want_catch = (rq.outputs & kUsageCatchment) != 0;
  dymu_usage_out sized = o;  // the catchment needs the sums: size the workspace with them
  uint64_t dummy = 0;
  if (want_catch && !sized.usage) sized.usage = &dummy;
  const size_t need = dymu_route_usage_workspace(nx_, ny_, &sized);
  if (!need) check(DYMU_ERR_ARG, "workspace query");
  if (need > usage_ws_bytes_) {
    if (d_usage_ws_) (void)dymu_device_free(ctx_, d_usage_ws_);
    d_usage_ws_ = nullptr;
    usage_ws_bytes_ = 0;
    check(dymu_device_alloc_cached(ctx_, need, &d_usage_ws_), "workspace allocation");
    usage_ws_bytes_ = need;
  }
  if (want_catch) out.catchment.assign(seeds.size(), 0u);
  check(dymu_route_usage_device(ctx_, map, nx_, ny_, nx_, seeds.data(), (uint32_t)seeds.size(),
                                rq.weights ? d_uweight_ : nullptr, nx_, &o,
                                want_catch ? out.catchment.data() : nullptr, d_usage_ws_,
                                usage_ws_bytes_, nullptr, &out.rounds),
        "kernels");
  auto down = [&](auto& v, const void* d) {
    v.resize(n);
    check(dymu_memcpy_d2h(ctx_, v.data(), d, sizeof(v[0]) * n), "download");
  };
  if (o.usage) down(out.usage, o.usage);
  if (o.far) down(out.far, o.far);
  if (o.sink) down(out.sink, o.sink);
  double ms = 0.0;
  if (dymu_last_route_usage_ms(ctx_, &ms) == DYMU_OK) last_paths_kernel_ms_ = ms;
}

// ---- goal sets (extension) ----

// The goal-set entries of the engine C-ABI: null with an engine that predates them
// (see the path entries above); the solve then fails, labels and paths take the host route.
#pragma weak dymu_solve_seeds_device
#pragma weak dymu_goal_labels_device
#pragma weak dymu_extract_paths_goals_device
#pragma weak dymu_device_alloc_cached
// ... and the windowed updates of seeded maps and stacks: without them
// trackSpeedChanges changes nothing
#pragma weak dymu_update_seeds_window_device
#pragma weak dymu_update_batch_window_device

bool DyMuPathPlanner::goalsOnDevice() const {
  return &dymu_goal_labels_device && &dymu_extract_paths_goals_device &&
         &dymu_device_alloc_cached && (uint64_t)nx_ * ny_ < (1ull << 31);
}

bool DyMuPathPlanner::setGoals(const std::vector<base::Waypoint>& goals,
                               const std::vector<double>& offsets) {
  if (goals.empty() || (!offsets.empty() && offsets.size() != goals.size())) return false;
  std::vector<Goal> gs;
  for (size_t q = 0; q < goals.size(); ++q) {
    const double t0 = offsets.empty() ? 0.0 : offsets[q];
    if (!(t0 >= 0.0) || !(t0 < kInf)) return false;
    // setGoal's tests (:322-357)
    const double px = (goals[q].position[0] - global_offset_[0]) / global_res_;
    const double py = (goals[q].position[1] - global_offset_[1]) / global_res_;
    if (!(px >= 0) || !(py >= 0)) return false;
    const unsigned i = grid_u32(px + 0.5), j = grid_u32(py + 0.5);
    if (i >= nx_ || j >= ny_) return false;
    if (i == 0 || j == 0 || i + 1 >= nx_ || j + 1 >= ny_) return false;
    const uint64_t k = idx(i, j);
    if (is_obstacle_[k] || is_obstacle_[k - nx_] || is_obstacle_[k - 1] || is_obstacle_[k + 1] ||
        is_obstacle_[k + nx_])
      return false;
    gs.push_back(Goal{i, j, goals[q].heading, t0 + 0.0});
  }
  goals_.swap(gs);
  has_goal_ = true;
  goal_i_ = goals_[0].i;
  goal_j_ = goals_[0].j;
  goal_heading_ = goals_[0].heading;
  solved_ = false;  // no single-goal map is reused under a goal set (gs_seeds_: compared
                    // with the new list by propagateGoals)
  invalidateLabels();
  return true;
}

std::vector<dymu_seed> DyMuPathPlanner::seedList() const {
  std::vector<dymu_seed> s;
  if (goals_.empty()) {
    if (has_goal_) s.push_back(dymu_seed{goal_i_, goal_j_, 0.0});
  } else {
    for (const Goal& g : goals_) s.push_back(dymu_seed{g.i, g.j, g.t0});
  }
  return s;
}

base::Waypoint DyMuPathPlanner::sinkWaypoint(size_t k) const {
  const Goal& g = goals_[k];
  return nodeSink(g.i, g.j, g.heading);
}

// computeEntireTotalCostMap for a goal set: the cold multi-source solve -- always,
// unless trackSpeedChanges is on and dT_ holds the converged map of the same seed list:
// then the map is re-propagated from the changed box (at most a quarter of the grid,
// propagate's rule) or reused.  The state is a converged full solve's (every finite
// node CLOSED, no band), and solved_ stays false so that no single-goal window reuse is
// keyed on this map.
bool DyMuPathPlanner::propagateGoals() {
  for (const Goal& g : goals_)
    if (is_obstacle_[idx(g.i, g.j)]) {
      log_warn("The goal is not valid");
      return false;
    }
  ensureEngine();
  if (!&dymu_solve_seeds_device)
    throw std::runtime_error("dymu: the engine has no multi-source solve (dymu_solve_seeds_device)");
  unsigned i0, i1, j0, j1;
  bool changed = syncSpeed(i0, i1, j0, j1);
  if (changed) batchSpeedChanged(i0, i1, j0, j1);
  if (pend_) {  // a change a batch solve synchronised: dT_ has not seen it yet
    i0 = std::min(i0, pend_i0_), i1 = std::max(i1, pend_i1_);
    j0 = std::min(j0, pend_j0_), j1 = std::max(j1, pend_j1_);
    decrease_only_ = decrease_only_ && pend_dec_;
    changed = true;
    pend_ = false;  // and solved_ stays false: no single-goal window is reused after this
  }
  const std::vector<dymu_seed> seeds = seedList();
  // trackSpeedChanges: dT_ holds the converged map of this very seed list
  const bool held = track_ && &dymu_update_seeds_window_device && dev_map_current_ &&
                    gs_seeds_.size() == seeds.size() &&
                    std::equal(seeds.begin(), seeds.end(), gs_seeds_.begin(),
                               [](const dymu_seed& a, const dymu_seed& b) {
                                 return a.i == b.i && a.j == b.j && a.t0 == b.t0;
                               });
  if (held && !changed) {
    incremental_ = 2;
    return true;
  }
  int rc = DYMU_ERR_STATE;
  dev_map_current_ = false;
  solved_ = false, gs_seeds_.clear();
  invalidateLabels();
  if (held && (uint64_t)(i1 - i0) * (j1 - j0) * 4 <= (uint64_t)nx_ * ny_) {
    rc = dymu_update_seeds_window_device(ctx_, dF_, dT_, nx_, ny_, nx_, seeds.data(),
                                         (uint32_t)seeds.size(), i0, j0, i1 - i0, j1 - j0,
                                         decrease_only_ ? 1 : 0, nullptr, &stats_);
    if (rc == DYMU_OK) incremental_ = 1;
  }
  if (rc != DYMU_OK) {
    rc = dymu_solve_seeds_device(ctx_, dF_, dT_, nx_, ny_, nx_, seeds.data(),
                                 (uint32_t)seeds.size(), nullptr, &stats_);
    if (rc != DYMU_OK)
      throw std::runtime_error(std::string("dymu solve failed: ") + dymu_strerror(rc) + " " +
                               dymu_last_error(ctx_));
    incremental_ = 0;
  }
  gs_seeds_ = seeds;
  dev_map_current_ = true;
  std::fill(blk_ok_.begin(), blk_ok_.end(), 0);
  blk_missing_ = blk_ok_.size();
  band_cells_.clear();
  band_unordered_ = false;
  band_values_checked_ = true;
  open_at_limit_.clear();
  node_state_.clear();
  propagated_extra_.clear();
  manual_list_ = false;
  early_info_ = EarlyExitInfo{};
  have_start_ = false;
  closed_limit_ = kInf;
  return true;
}

// global_propagated_nodes under a goal set: the finite cells by (total cost, grid index)
std::vector<uint64_t> DyMuPathPlanner::sortedFinite() {
  fetchAll();
  std::vector<std::pair<double, uint64_t>> v;
  for (uint64_t k = 0; k < total_cost_.size(); ++k)
    if (total_cost_[k] < kInf) v.emplace_back(total_cost_[k], k);
  parallel_sort(v);
  std::vector<uint64_t> out;
  out.reserve(v.size());
  for (const auto& e : v) out.push_back(e.second);
  return out;
}

void DyMuPathPlanner::dropLabels() {
  invalidateLabels();
  if (d_label_ && ctx_) (void)dymu_device_free(ctx_, d_label_);
  d_label_ = nullptr;
  // getPathStats' field buffer goes where the label map goes: with the map buffers
  if (d_pfield_ && ctx_) (void)dymu_device_free(ctx_, d_pfield_);
  d_pfield_ = nullptr;
  dropRouteBuffers();  // ... and getRouteFields' buffers
}

void DyMuPathPlanner::ensureDeviceLabels() {
  if (d_label_valid_) return;
  const uint64_t n = (uint64_t)nx_ * ny_;
  if (!d_label_) {
    void* p = nullptr;
    if (dymu_device_alloc_cached(ctx_, sizeof(uint32_t) * n, &p) != DYMU_OK)
      throw std::runtime_error(std::string("dymu: cannot allocate the label map: ") +
                               dymu_last_error(ctx_));
    d_label_ = static_cast<uint32_t*>(p);
  }
  const std::vector<dymu_seed> seeds = seedList();
  const int rc = dymu_goal_labels_device(ctx_, dT_, nx_, ny_, nx_, seeds.data(),
                                         (uint32_t)seeds.size(), d_label_, nullptr, &label_rounds_);
  if (rc != DYMU_OK)
    throw std::runtime_error(std::string("dymu: goal labels failed: ") + dymu_strerror(rc) + " " +
                             dymu_last_error(ctx_));
  d_label_valid_ = true;
}

// The label rule of include/dymu_fim.h on the host mirror: roots first, then the cells
// in ascending total cost, each taking its parent's label (a parent is strictly lower,
// so it is labelled by then).
void DyMuPathPlanner::ensureHostLabels() {
  if (labels_valid_) return;
  const uint64_t n = (uint64_t)nx_ * ny_;
  labels_.assign(n, DYMU_LABEL_NONE);
  const std::vector<dymu_seed> seeds = seedList();
  if (seeds.empty()) {
    labels_valid_ = true;
    return;
  }
  if (ctx_ && dT_ && dev_map_current_ && goalsOnDevice()) {
    ensureDeviceLabels();
    if (dymu_memcpy_d2h(ctx_, labels_.data(), d_label_, sizeof(uint32_t) * n) != DYMU_OK)
      throw std::runtime_error(std::string("dymu: label download failed: ") +
                               dymu_last_error(ctx_));
    labels_valid_ = true;
    return;
  }
  label_rounds_ = 0;
  fetchAll();
  const double* t = total_cost_.data();
  std::vector<uint8_t> root(n, 0);
  for (size_t k = seeds.size(); k-- > 0;) {  // descending: the lowest k is written last
    const uint64_t c = idx(seeds[k].i, seeds[k].j);
    if (std::memcmp(&t[c], &seeds[k].t0, sizeof(double)) != 0) continue;  // dominated
    labels_[c] = (uint32_t)k;
    root[c] = 1;
  }
  std::vector<std::pair<double, uint64_t>> order;
  for (uint64_t c = 0; c < n; ++c)
    if (t[c] < kInf && !root[c]) order.emplace_back(t[c], c);
  parallel_sort(order);
  for (const auto& e : order) {
    const uint64_t c = e.second;
    const unsigned i = (unsigned)(c % nx_), j = (unsigned)(c / nx_);
    double best = e.first;
    uint64_t par = n;
    if (j > 0 && t[c - nx_] < best) { best = t[c - nx_]; par = c - nx_; }
    if (i > 0 && t[c - 1] < best) { best = t[c - 1]; par = c - 1; }
    if (i + 1 < nx_ && t[c + 1] < best) { best = t[c + 1]; par = c + 1; }
    if (j + 1 < ny_ && t[c + nx_] < best) { best = t[c + nx_]; par = c + nx_; }
    if (par < n) labels_[c] = labels_[par];
  }
  labels_valid_ = true;
}

void DyMuPathPlanner::copyGoalLabels(uint32_t* out) {
  ensureHostLabels();
  std::memcpy(out, labels_.data(), sizeof(uint32_t) * labels_.size());
}

int DyMuPathPlanner::goalLabel(base::Waypoint w) {
  const double x = w.position[0] - global_offset_[0], y = w.position[1] - global_offset_[1];
  if (!(x / global_res_ + 0.5 >= 0) || !(y / global_res_ + 0.5 >= 0)) return -1;
  const int64_t k = nearestIndex(x, y);
  if (k < 0) return -1;
  ensureHostLabels();
  const uint32_t lab = labels_[(uint64_t)k];
  return lab == DYMU_LABEL_NONE ? -1 : (int)lab;
}

// :788-795
std::string DyMuPathPlanner::getLocomotionMode(base::Waypoint wPos) {
  const double x = wPos.position[0] - global_offset_[0];
  const double y = wPos.position[1] - global_offset_[1];
  const unsigned i = grid_u32(x / global_res_ + 0.5), j = grid_u32(y / global_res_ + 0.5);
  if (i >= nx_ || j >= ny_) return "DONT_CARE";
  const int m = loc_mode_[idx(i, j)];
  if (m < 0 || m >= (int)locomotion_modes_.size()) return "DONT_CARE";
  return locomotion_modes_[m];
}

// :799-811
std::vector<std::vector<double>> DyMuPathPlanner::getTotalCostMatrix() {
  std::vector<std::vector<double>> m(ny_);
  parallel_rows(ny_, [&](unsigned j0, unsigned j1) {
    for (unsigned j = j0; j < j1; ++j) m[j].resize(nx_);
  });
  streamTotalCost([&](unsigned r0, unsigned r1) {
    parallel_rows(r1 - r0, [&](unsigned j0, unsigned j1) {
      for (unsigned j = r0 + j0; j < r0 + j1; ++j) {
        const double* t = &total_cost_[idx(0, j)];
        std::vector<double>& r = m[j];
        for (unsigned i = 0; i < nx_; ++i) r[i] = (t[i] == kInf) ? -1.0 : t[i];
      }
    });
  });
  return m;
}

// :815-829
std::vector<std::vector<double>> DyMuPathPlanner::getGlobalCostMatrix() {
  std::vector<std::vector<double>> m(ny_, std::vector<double>(nx_));
  for (unsigned j = 0; j < ny_; ++j)
    for (unsigned i = 0; i < nx_; ++i) {
      const uint64_t k = idx(i, j);
      m[j][i] = is_obstacle_[k] ? -1.0 : cost_[k] * (2 + hazard_[k] - traff_[k]);
    }
  return m;
}

// :833-842
std::vector<std::vector<double>> DyMuPathPlanner::getHazardDensityMatrix() {
  std::vector<std::vector<double>> m(ny_, std::vector<double>(nx_));
  for (unsigned j = 0; j < ny_; ++j)
    for (unsigned i = 0; i < nx_; ++i) m[j][i] = hazard_[idx(i, j)];
  return m;
}

// :846-855
std::vector<std::vector<double>> DyMuPathPlanner::getTrafficabilityMatrix() {
  std::vector<std::vector<double>> m(ny_, std::vector<double>(nx_));
  for (unsigned j = 0; j < ny_; ++j)
    for (unsigned i = 0; i < nx_; ++i) m[j][i] = traff_[idx(i, j)];
  return m;
}

// :860-890 (Q6 kept: a = x - i, not x/res - i)
double DyMuPathPlanner::getTotalCost(base::Waypoint wInt) {
  const double x = wInt.position[0] - global_offset_[0];
  const double y = wInt.position[1] - global_offset_[1];
  const unsigned i = grid_u32(x / global_res_), j = grid_u32(y / global_res_);
  const double a = x - (double)i, b = y - (double)j;
  if (i >= nx_ || j >= ny_ || i + 1 >= nx_ || j + 1 >= ny_) {  // a corner is NULL
    const unsigned ni = grid_u32(x / global_res_ + 0.5), nj = grid_u32(y / global_res_ + 0.5);
    if (ni >= nx_ || nj >= ny_) return kInf;
    return T(idx(ni, nj));
  }
  const uint64_t k = idx(i, j);
  const uint64_t k10 = k + 1, k01 = k + nx_, k11 = k + nx_ + 1;
  if (!closedCell(k) || !closedCell(k10) || !closedCell(k01) || !closedCell(k11)) {
    const unsigned ni = grid_u32(x / global_res_ + 0.5), nj = grid_u32(y / global_res_ + 0.5);
    return T(idx(ni, nj));
  }
  const double w00 = T(k), w10 = T(k10);
  const double w01 = T(k01), w11 = T(k11);
  return w00 + (w10 - w00) * a + (w01 - w00) * b + (w11 + w00 - w10 - w01) * a * b;
}

// ---- node-level access (src/DyMu.hpp:500-518) ----

std::optional<globalNode> DyMuPathPlanner::snapshot(uint64_t k) {
  globalNode n;
  const unsigned i = (unsigned)(k % nx_), j = (unsigned)(k / nx_);
  n.pose.position[0] = (double)i;
  n.pose.position[1] = (double)j;
  if (has_goal_ && i == goal_i_ && j == goal_j_) n.pose.orientation = goal_heading_;
  n.world_pose.position[0] = (double)i * global_res_;  // globalNode ctor (src/DyMu.hpp:92-93)
  n.world_pose.position[1] = (double)j * global_res_;
  n.elevation = elevation_[k];
  n.slope = slope_[k];
  n.state = closedCell(k) ? CLOSED : OPEN;
  n.isObstacle = is_obstacle_[k] != 0;
  n.hasLocalMap = local_ && local_->block(k) >= 0;
  n.raw_cost = raw_cost_[k];
  n.cost = cost_[k];
  n.hazard_density = hazard_[k];
  n.trafficability = traff_[k];
  n.total_cost = T(k);
  n.terrain = terrain_[k];
  const int m = loc_mode_[k];
  n.nodeLocMode = (m < 0 || m >= (int)locomotion_modes_.size()) ? "DONT_CARE" : locomotion_modes_[m];
  return n;
}

// :313-317
std::optional<globalNode> DyMuPathPlanner::getGlobalNode(unsigned i, unsigned j) {
  if (i >= nx_ || j >= ny_) return std::nullopt;
  return snapshot(idx(i, j));
}

// :570-584
std::optional<globalNode> DyMuPathPlanner::getNearestGlobalNode(base::Pose2D pos) {
  const int64_t k = nearestIndex(pos.position[0], pos.position[1]);
  if (k < 0) return std::nullopt;
  return snapshot((uint64_t)k);
}

std::optional<globalNode> DyMuPathPlanner::getNearestGlobalNode(base::Waypoint wPos) {
  const int64_t k = nearestIndex(wPos.position[0], wPos.position[1]);
  if (k < 0) return std::nullopt;
  return snapshot((uint64_t)k);
}

std::optional<globalNode> DyMuPathPlanner::globalGoal() {
  if (!has_goal_) return std::nullopt;
  return snapshot(idx(goal_i_, goal_j_));
}

bool DyMuPathPlanner::isSafeNode(unsigned i, unsigned j) { return safeNode(i, j); }

// :424-436 (a border node returns false where the reference dereferences NULL)
bool DyMuPathPlanner::isFullyClosedNode(unsigned i, unsigned j) {
  if (i == 0 || j == 0 || i + 1 >= nx_ || j + 1 >= ny_) return false;
  const uint64_t k = idx(i, j);
  return closedCell(k) && closedCell(k - nx_) && closedCell(k - 1) && closedCell(k + 1) &&
         closedCell(k + nx_);
}

// :473-485: every node OPEN at +inf, global_propagated_nodes cleared
void DyMuPathPlanner::resetTotalCostMap() {
  std::fill(total_cost_.begin(), total_cost_.end(), kInf);
  std::fill(blk_ok_.begin(), blk_ok_.end(), 1);
  blk_missing_ = 0;
  closed_limit_ = 0.0;
  band_cells_.clear();
  band_unordered_ = false;
  band_values_checked_ = true;
  open_at_limit_.clear();
  node_state_.assign(total_cost_.size(), 0);
  propagated_extra_.clear();
  manual_list_ = true;
  solved_ = false, gs_seeds_.clear();
  dev_map_current_ = false;  // the host copy alone was written
  invalidateLabels();
}

// the node states of the last solve made explicit, so a caller can change some
void DyMuPathPlanner::materializeStates() {
  if (!node_state_.empty()) return;
  fetchAll();
  std::vector<uint8_t> st(total_cost_.size());
  for (uint64_t k = 0; k < st.size(); ++k) st[k] = closedCell(k) ? 1 : 0;
  node_state_ = std::move(st);
}

void DyMuPathPlanner::setGlobalNodeState(unsigned i, unsigned j, node_state s) {
  if (i >= nx_ || j >= ny_) return;
  settleBand();
  materializeStates();
  node_state_[idx(i, j)] = s == CLOSED ? 1 : 0;
}

// :500-546, on the host copy of the map (made whole first, so no later download
// of device blocks can overwrite what this writes)
void DyMuPathPlanner::propagateGlobalNode(unsigned i, unsigned j) {
  if (i >= nx_ || j >= ny_) return;
  settleBand();
  orderBand();  // from the solve's values, before this changes any
  fetchAll();
  const uint64_t k = idx(i, j);
  const double* t = total_cost_.data();
  const bool n0 = j > 0, n3 = j + 1 < ny_, n1 = i > 0, n2 = i + 1 < nx_;
  // a NULL neighbour: the other one alone (:504-523); none at all (a 1-wide grid, a
  // NULL dereference in the reference): +inf
  double Ty, Tx;
  if (n0 && n3)
    Ty = std::fmin(t[k + nx_], t[k - nx_]);
  else if (!n0)
    Ty = n3 ? t[k + nx_] : kInf;
  else
    Ty = t[k - nx_];
  if (n1 && n2)
    Tx = std::fmin(t[k - 1], t[k + 1]);
  else if (!n1)
    Tx = n2 ? t[k + 1] : kInf;
  else
    Tx = t[k - 1];
  syncGlobalRisk();
  const double C = nodeSpeed(k);  // :527-528, times the global risk's factor (s5.11)
  double Tn;
  if ((std::fabs(Tx - Ty) < C) && (Tx < kInf) && (Ty < kInf))
    Tn = (Tx + Ty + std::sqrt(2 * (C * C) - ((Tx - Ty) * (Tx - Ty)))) / 2;  // pow(., 2.0) == x*x
  else
    Tn = std::fmin(Tx, Ty) + C;
  if (Tn < total_cost_[k]) {
    if (total_cost_[k] == kInf) {
      propagated_extra_.push_back(k);
      band_cells_.push_back(k);  // insertion order, as the reference's vector
    }
    total_cost_[k] = Tn;
    solved_ = false, gs_seeds_.clear();  // the device map no longer matches the host's
    dev_map_current_ = false;
    invalidateLabels();
  }
}

void DyMuPathPlanner::propagateGlobalNode(const globalNode& n) {
  propagateGlobalNode(grid_u32(n.pose.position[0]), grid_u32(n.pose.position[1]));
}

uint64_t DyMuPathPlanner::globalPropagatedCount() {
  if (manual_list_) return propagated_extra_.size();
  uint64_t c = propagated_extra_.size();
  streamTotalCost([&](unsigned r0, unsigned r1) {
    const double* t = total_cost_.data();
    for (uint64_t k = idx(0, r0); k < idx(0, r1); ++k) c += t[k] < kInf ? 1 : 0;
  });
  // nodes propagateGlobalNode made finite are counted in the map already
  return c - propagated_extra_.size();
}

// the reached nodes in the reference's insertion order (insertionOrder: rebuilt from
// the values, or replayed on the host when they cannot decide it), then those
// propagateGlobalNode added since, in the order it added them
std::vector<uint64_t> DyMuPathPlanner::globalPropagatedIndices() {
  std::vector<uint64_t> out;
  if (!manual_list_) {
    out = goals_.empty() ? insertionOrder() : sortedFinite();
    if (!propagated_extra_.empty()) {
      std::vector<uint8_t> extra(total_cost_.size(), 0);
      for (const uint64_t k : propagated_extra_) extra[k] = 1;
      out.erase(std::remove_if(out.begin(), out.end(), [&](uint64_t k) { return extra[k] != 0; }),
                out.end());
    }
  }
  out.insert(out.end(), propagated_extra_.begin(), propagated_extra_.end());
  return out;
}

std::vector<globalNode> DyMuPathPlanner::globalPropagatedNodes() {
  const std::vector<uint64_t> ks = globalPropagatedIndices();
  std::vector<globalNode> out;
  out.reserve(ks.size());
  for (const uint64_t k : ks) out.push_back(*snapshot(k));
  return out;
}

std::vector<globalNode> DyMuPathPlanner::globalNarrowband() {
  orderBand();
  std::vector<globalNode> out;
  out.reserve(band_cells_.size());
  for (const uint64_t k : band_cells_) out.push_back(*snapshot(k));
  return out;
}

// The band's values after a GPU early exit are the reference's update arithmetic on the
// engine's CLOSED values: equal to the reference's within rounding, so the order of
// minCostGlobalNode's pops is decided by them only if no two are near-tied (TieGuard).
// Checked once, before the first pop or change of the band (it costs a sort); on a near
// tie the exit is replayed exactly on the host and the band and its values become the
// reference's.
void DyMuPathPlanner::settleBand() {
  if (band_values_checked_) return;
  band_values_checked_ = true;
  if (band_cells_.size() < 2) return;
  const uint64_t g = idx(goal_i_, goal_j_);
  TieGuard guard(nx_, goal_i_, goal_j_, speed_[g], exit_r_const_);
  std::vector<std::pair<double, uint64_t>> bv(band_cells_.size());
  for (size_t q = 0; q < bv.size(); ++q) bv[q] = {T(band_cells_[q]), band_cells_[q]};
  std::sort(bv.begin(), bv.end());
  for (size_t q = 1; q < bv.size(); ++q)
    (void)guard.cmp(bv[q - 1].second, bv[q - 1].first, bv[q].second, bv[q].first);
  early_info_.near_ties += guard.near;
  if (guard.near) {
    early_info_.exact_replay = 1;
    (void)exactEarlyExit(start_i_, start_j_, exit_box_);
  }
}

// :548-567 (first strict minimum, then erased from the band)
std::optional<globalNode> DyMuPathPlanner::minCostGlobalNode() {
  settleBand();
  if (band_cells_.empty()) return std::nullopt;
  orderBand();
  size_t best = 0;
  double tmin = T(band_cells_[0]);
  for (size_t q = 1; q < band_cells_.size(); ++q) {
    const double t = T(band_cells_[q]);
    if (t < tmin) {
      tmin = t;
      best = q;
    }
  }
  const uint64_t k = band_cells_[best];
  band_cells_.erase(band_cells_.begin() + (std::ptrdiff_t)best);
  return snapshot(k);
}

// :487-498
void DyMuPathPlanner::resetGlobalNarrowBand() {
  band_cells_.clear();
  band_unordered_ = false;
  band_values_checked_ = true;
  if (!has_goal_ || nx_ == 0) return;
  if (!goals_.empty()) {  // every root goal: not dominated, once per cell, at its offset
    fetchAll();
    const std::vector<dymu_seed> seeds = seedList();
    std::vector<std::pair<uint64_t, double>> roots;
    for (const dymu_seed& sd : seeds) {
      const uint64_t k = idx(sd.i, sd.j);
      if (total_cost_[k] < sd.t0) continue;  // dominated by another goal
      auto it = std::find_if(roots.begin(), roots.end(), [&](const auto& r) { return r.first == k; });
      if (it == roots.end()) roots.emplace_back(k, sd.t0);
      else it->second = std::min(it->second, sd.t0);
    }
    dev_map_current_ = false;
    invalidateLabels();
    for (const auto& r : roots) {
      total_cost_[r.first] = r.second;
      band_cells_.push_back(r.first);
      propagated_extra_.push_back(r.first);
    }
    return;
  }
  const uint64_t k = idx(goal_i_, goal_j_);
  (void)T(k);  // the goal's block in the host mirror before the write
  total_cost_[k] = 0.0;
  dev_map_current_ = false;  // written on the host alone
  invalidateLabels();
  band_cells_.push_back(k);
  propagated_extra_.push_back(k);  // global_propagated_nodes.push_back(global_goal)
}

bool DyMuPathPlanner::loadTotalCostMap(const double* Tin) {
  const uint64_t n = (uint64_t)nx_ * ny_;
  if (!Tin || n == 0) return false;
  std::memcpy(total_cost_.data(), Tin, sizeof(double) * n);
  std::fill(blk_ok_.begin(), blk_ok_.end(), 1);
  blk_missing_ = 0;
  closed_limit_ = kInf;
  band_cells_.clear();
  band_unordered_ = false;
  band_values_checked_ = true;
  open_at_limit_.clear();
  node_state_.clear();
  propagated_extra_.clear();
  manual_list_ = false;
  solved_ = false, gs_seeds_.clear();
  dev_map_current_ = false;
  invalidateLabels();
  if (ctx_ && dT_ && dcells_ == n) {
    if (dymu_memcpy_h2d(ctx_, dT_, total_cost_.data(), sizeof(double) * n) != DYMU_OK)
      throw std::runtime_error(std::string("dymu: total-cost upload failed: ") +
                               dymu_last_error(ctx_));
    dev_map_current_ = true;
  }
  return true;
}

// ---- batched total-cost maps (extension) ----

// The batch entries of the engine C-ABI: null with an engine that predates them (see the
// path entries above); computeTotalCostMaps then returns false.
#pragma weak dymu_batch_plane_rows
#pragma weak dymu_stack_speed_device
#pragma weak dymu_solve_batch_device
#pragma weak dymu_gather_costs_device
#pragma weak dymu_solve_batch_until_device

// trackSpeedChanges: a pending box is re-propagated through the batch when it covers at
// most 1 / kBatchWindowDiv of the grid (propagate's rule; DESIGN.md s5.8 has the
// measurements it rests on), else the batch is solved cold
constexpr uint64_t kBatchWindowDiv = 4;

void DyMuPathPlanner::dropBatch() {
  if (dT_batch_ && ctx_) (void)dymu_device_free(ctx_, dT_batch_);
  dT_batch_ = nullptr;
  batch_goals_.clear();
  batch_stats_ = dymu_stats{};
  batch_kind_ = 0;
  batch_level_ = kInf;
  bpend_ = false;
  comb_valid_ = comb_arg_valid_ = false;  // the combined map was that of this stack
}

void DyMuPathPlanner::trackSpeedChanges(bool on) {
  track_ = on;
  if (!on && bpend_) dropBatch();  // untracked, a batch never outlives a change
}

void DyMuPathPlanner::batchSpeedChanged(unsigned i0, unsigned i1, unsigned j0, unsigned j1) {
  if (!dT_batch_) return;
  // a truncated batch (costMatrixUntil) is never carried across a change
  if (!track_ || !&dymu_update_batch_window_device || batch_level_ < kInf) {
    dropBatch();
    return;
  }
  bpend_i0_ = bpend_ ? std::min(bpend_i0_, i0) : i0;
  bpend_i1_ = bpend_ ? std::max(bpend_i1_, i1) : i1;
  bpend_j0_ = bpend_ ? std::min(bpend_j0_, j0) : j0;
  bpend_j1_ = bpend_ ? std::max(bpend_j1_, j1) : j1;
  bpend_dec_ = (bpend_ ? bpend_dec_ : true) && decrease_only_;
  bpend_ = true;
}

// setGoal's tests (:322-357)
bool DyMuPathPlanner::goalCell(const base::Waypoint& w, unsigned& i, unsigned& j) const {
  const double px = (w.position[0] - global_offset_[0]) / global_res_;
  const double py = (w.position[1] - global_offset_[1]) / global_res_;
  if (!(px >= 0) || !(py >= 0)) return false;
  i = grid_u32(px + 0.5), j = grid_u32(py + 0.5);
  if (i >= nx_ || j >= ny_) return false;
  if (i == 0 || j == 0 || i + 1 >= nx_ || j + 1 >= ny_) return false;
  const uint64_t k = idx(i, j);
  return !(is_obstacle_[k] || is_obstacle_[k - nx_] || is_obstacle_[k - 1] || is_obstacle_[k + 1] ||
           is_obstacle_[k + nx_]);
}

bool DyMuPathPlanner::prepareBatch(const std::vector<base::Waypoint>& goals,
                                   std::vector<BatchGoal>& bg) {
  if (goals.empty() || goals.size() > 0xffffffffull || nx_ == 0 || ny_ == 0) return false;
  if (!&dymu_batch_plane_rows || !&dymu_stack_speed_device || !&dymu_solve_batch_device ||
      !&dymu_gather_costs_device)
    return false;
  for (const base::Waypoint& w : goals) {
    unsigned i = 0, j = 0;
    if (!goalCell(w, i, j)) return false;
    bg.push_back(BatchGoal{i, j, w.heading});
  }
  const uint64_t P = dymu_batch_plane_rows(ny_);
  if (P == 0 || (uint64_t)bg.size() * P > 0xffffffffull) return false;
  try {
    ensureEngine();
    unsigned i0, i1, j0, j1;
    if (syncSpeed(i0, i1, j0, j1)) {
      // the batch at hand is that of the old speed (dropped, or kept with the box pending:
      // trackSpeedChanges); dT_ keeps the old speed's map, so the changed box waits for
      // the next single-goal solve (propagate)
      batchSpeedChanged(i0, i1, j0, j1);
      pend_i0_ = pend_ ? std::min(pend_i0_, i0) : i0;
      pend_i1_ = pend_ ? std::max(pend_i1_, i1) : i1;
      pend_j0_ = pend_ ? std::min(pend_j0_, j0) : j0;
      pend_j1_ = pend_ ? std::max(pend_j1_, j1) : j1;
      pend_dec_ = (pend_ ? pend_dec_ : true) && decrease_only_;
      pend_ = true;
    }
  } catch (const std::exception&) {
    return false;  // no device engine
  }
  return true;
}

bool DyMuPathPlanner::computeTotalCostMaps(const std::vector<base::Waypoint>& goals) {
  std::vector<BatchGoal> bg;
  if (!prepareBatch(goals, bg)) return false;
  // trackSpeedChanges: the held batch of these very goals is reused, or re-propagated
  // from the pending box where that box is small enough (refreshBatch); a truncated
  // batch (costMatrixUntil) is not: the cold solve below replaces it
  if (track_ && dT_batch_ && !(batch_level_ < kInf) && bg.size() == batch_goals_.size() &&
      std::equal(bg.begin(), bg.end(), batch_goals_.begin(),
                 [](const BatchGoal& a, const BatchGoal& b) { return a.i == b.i && a.j == b.j; })) {
    if (!bpend_) {
      batch_goals_.swap(bg);  // the headings given now
      batch_kind_ = 2;
      return true;
    }
    if ((uint64_t)(bpend_i1_ - bpend_i0_) * (bpend_j1_ - bpend_j0_) * kBatchWindowDiv <=
        (uint64_t)nx_ * ny_) {
      if (!refreshBatch()) return false;
      batch_goals_.swap(bg);
      return true;
    }
  }
  return solveBatchCold(bg);
}

bool DyMuPathPlanner::solveBatchCold(std::vector<BatchGoal>& bg) {
  const uint32_t B = (uint32_t)bg.size();
  const uint64_t P = dymu_batch_plane_rows(ny_);
  std::vector<dymu_batch_seed> seeds;
  for (const BatchGoal& g : bg) seeds.push_back(dymu_batch_seed{(uint32_t)seeds.size(), g.i, g.j, 0u, 0.0});
  double *f = nullptr, *t = nullptr;
  const uint64_t bytes = sizeof(double) * (uint64_t)B * P * nx_;
  void *pf = nullptr, *pt = nullptr;
  dymu_stats st{};
  int rc = dymu_device_alloc(ctx_, bytes, &pf);
  if (rc == DYMU_OK) rc = dymu_device_alloc(ctx_, bytes, &pt);
  f = static_cast<double*>(pf);
  t = static_cast<double*>(pt);
  if (rc == DYMU_OK) rc = dymu_stack_speed_device(ctx_, dF_, nx_, 0, nx_, ny_, B, f, nx_, nullptr);
  if (rc == DYMU_OK)
    rc = dymu_solve_batch_device(ctx_, f, t, nx_, ny_, B, nx_, seeds.data(), B, nullptr, &st);
  if (f) (void)dymu_device_free(ctx_, f);  // the solved stack alone stays resident
  if (rc != DYMU_OK) {
    if (t) (void)dymu_device_free(ctx_, t);
    return false;
  }
  dropBatch();
  dT_batch_ = t;
  batch_goals_.swap(bg);
  batch_stats_ = st;
  return true;
}

// The held batch on the current speed.  A pending box of at most 1 / kBatchWindowDiv of
// the grid: F re-stacked from dF_ (temporary) and every plane re-propagated from the box
// in one call; a larger box, or an update that fails: the cold solve of the same goals.
bool DyMuPathPlanner::refreshBatch() {
  if (batch_level_ < kInf) {  // truncated (costMatrixUntil): completed by the cold solve
    if (!ctx_ || !dT_batch_) return false;
    std::vector<BatchGoal> bg = batch_goals_;
    if (solveBatchCold(bg)) return true;
    dropBatch();
    return false;
  }
  if (!bpend_) return true;
  if (!ctx_ || !dT_batch_) return false;
  const uint32_t B = (uint32_t)batch_goals_.size();
  const uint64_t P = dymu_batch_plane_rows(ny_);
  if (&dymu_update_batch_window_device &&
      (uint64_t)(bpend_i1_ - bpend_i0_) * (bpend_j1_ - bpend_j0_) * kBatchWindowDiv <=
          (uint64_t)nx_ * ny_) {
    std::vector<dymu_batch_seed> seeds;
    std::vector<dymu_batch_window> wins;
    for (uint32_t b = 0; b < B; ++b) {
      seeds.push_back(dymu_batch_seed{b, batch_goals_[b].i, batch_goals_[b].j, 0u, 0.0});
      wins.push_back(dymu_batch_window{b, bpend_i0_, bpend_j0_, bpend_i1_ - bpend_i0_,
                                       bpend_j1_ - bpend_j0_, 0u});
    }
    void* pf = nullptr;
    dymu_stats st{};
    int rc = dymu_device_alloc(ctx_, sizeof(double) * (uint64_t)B * P * nx_, &pf);
    double* f = static_cast<double*>(pf);
    if (rc == DYMU_OK) rc = dymu_stack_speed_device(ctx_, dF_, nx_, 0, nx_, ny_, B, f, nx_, nullptr);
    if (rc == DYMU_OK)
      rc = dymu_update_batch_window_device(ctx_, f, dT_batch_, nx_, ny_, B, nx_, seeds.data(), B,
                                           wins.data(), B, bpend_dec_ ? 1 : 0, nullptr, &st);
    if (f) (void)dymu_device_free(ctx_, f);
    if (rc == DYMU_OK) {
      bpend_ = false;
      batch_stats_ = st;
      batch_kind_ = 1;
      comb_valid_ = comb_arg_valid_ = false;  // the stack was rewritten
      return true;
    }
  }
  std::vector<BatchGoal> bg = batch_goals_;
  if (solveBatchCold(bg)) return true;
  dropBatch();  // its planes are those of an older speed
  return false;
}

bool DyMuPathPlanner::copyBatchTotalCost(unsigned b, double* out, bool raw) {
  if (b >= batch_goals_.size() || !out || !ctx_ || !dT_batch_ || !refreshBatch()) return false;
  const uint64_t n = (uint64_t)nx_ * ny_;
  const double* plane = dT_batch_ + (uint64_t)b * dymu_batch_plane_rows(ny_) * nx_;
  if (dymu_memcpy_d2h(ctx_, out, plane, sizeof(double) * n) != DYMU_OK)
    throw std::runtime_error(std::string("dymu: batch download failed: ") + dymu_last_error(ctx_));
  if (!raw)
    for (uint64_t k = 0; k < n; ++k)
      if (out[k] == kInf) out[k] = -1.0;
  return true;
}

// ---- combining the planes of the batch (extension) ----

// null with an engine that predates them: the methods below then return false
#pragma weak dymu_batch_reduce_device
#pragma weak dymu_level_mask_device
#pragma weak dymu_last_reduce_ms

void DyMuPathPlanner::dropCombined() {
  if (ctx_) {
    if (d_comb_) (void)dymu_device_free(ctx_, d_comb_);
    if (d_comb_arg_) (void)dymu_device_free(ctx_, d_comb_arg_);
    if (d_comb_mask_) (void)dymu_device_free(ctx_, d_comb_mask_);
  }
  d_comb_ = nullptr;
  d_comb_arg_ = nullptr;
  d_comb_mask_ = nullptr;
  comb_valid_ = comb_arg_valid_ = false;
}

bool DyMuPathPlanner::combineOnDevice(int op, const std::vector<uint32_t>& planes,
                                      const std::vector<double>& weights,
                                      const std::vector<double>& offsets, dymu_reduce_summary& s) {
  if (batch_goals_.empty() || !ctx_ || !dT_batch_ || !&dymu_batch_reduce_device) return false;
  const size_t B = batch_goals_.size(), n = planes.empty() ? B : planes.size();
  if (op < 0 || op > 2 || n > 65536 || (!weights.empty() && weights.size() != n) ||
      (!offsets.empty() && offsets.size() != n))
    return false;
  for (uint32_t p : planes)
    if (p >= B) return false;
  for (double w : weights)
    if (!(w > 0.0) || !(w < kInf)) return false;
  for (double o : offsets)
    if (!(o >= 0.0) || !(o < kInf)) return false;
  if (!refreshBatch()) return false;
  const uint64_t cells = (uint64_t)nx_ * ny_;
  if (!d_comb_) {
    void* q = nullptr;
    if (dymu_device_alloc(ctx_, sizeof(double) * cells, &q) != DYMU_OK) return false;
    d_comb_ = static_cast<double*>(q);
  }
  if (op != 0 && !d_comb_arg_) {
    void* q = nullptr;
    if (dymu_device_alloc(ctx_, sizeof(uint32_t) * cells, &q) != DYMU_OK) return false;
    d_comb_arg_ = static_cast<uint32_t*>(q);
  }
  comb_valid_ = comb_arg_valid_ = false;
  const int rc = dymu_batch_reduce_device(
      ctx_, dT_batch_, nx_, ny_, (uint32_t)B, nx_, op, planes.empty() ? nullptr : planes.data(),
      (uint32_t)n, weights.empty() ? nullptr : weights.data(),
      offsets.empty() ? nullptr : offsets.data(), d_comb_, nx_, op != 0 ? d_comb_arg_ : nullptr,
      nx_, &s, nullptr);
  if (rc != DYMU_OK) return false;
  comb_valid_ = true;
  comb_arg_valid_ = op != 0;
  double ms = 0.0;
  if (&dymu_last_reduce_ms && dymu_last_reduce_ms(ctx_, &ms) == DYMU_OK) last_combine_ms_ = ms;
  return true;
}

bool DyMuPathPlanner::combineTotalCostMaps(CombineOp op, const std::vector<uint32_t>& planes,
                                           const std::vector<double>& weights,
                                           const std::vector<double>& offsets,
                                           CombineSummary* summary) {
  dymu_reduce_summary s{};
  if (!combineOnDevice((int)op, planes, weights, offsets, s)) return false;
  if (summary) *summary = s;
  return true;
}

bool DyMuPathPlanner::copyCombinedTotalCost(double* out, bool raw) {
  // with a change pending the combined map is that of an older speed
  if (!out || !ctx_ || !dT_batch_ || !d_comb_ || !comb_valid_ || bpend_) return false;
  const uint64_t n = (uint64_t)nx_ * ny_;
  if (dymu_memcpy_d2h(ctx_, out, d_comb_, sizeof(double) * n) != DYMU_OK)
    throw std::runtime_error(std::string("dymu: combined map download failed: ") +
                             dymu_last_error(ctx_));
  if (!raw)
    for (uint64_t k = 0; k < n; ++k)
      if (out[k] == kInf) out[k] = -1.0;
  return true;
}

bool DyMuPathPlanner::copyCombinedPlanes(uint32_t* out) {
  if (!out || !ctx_ || !dT_batch_ || !d_comb_arg_ || !comb_valid_ || !comb_arg_valid_ || bpend_)
    return false;
  if (dymu_memcpy_d2h(ctx_, out, d_comb_arg_, sizeof(uint32_t) * (uint64_t)nx_ * ny_) != DYMU_OK)
    throw std::runtime_error(std::string("dymu: plane map download failed: ") +
                             dymu_last_error(ctx_));
  return true;
}

bool DyMuPathPlanner::viaCorridor(unsigned a, unsigned b, double slack, uint8_t* mask,
                                  CorridorInfo* info) {
  if (!mask || a >= batch_goals_.size() || b >= batch_goals_.size() || !(slack >= 0.0) ||
      !(slack < kInf) || !&dymu_level_mask_device)
    return false;
  dymu_reduce_summary s{};
  if (!combineOnDevice(0, {a, b}, {}, {}, s) || s.n_finite == 0) return false;
  const double bound = s.min_value * (1.0 + slack);
  if (!(bound < kInf)) return false;
  const uint64_t cells = (uint64_t)nx_ * ny_;
  if (!d_comb_mask_) {
    void* q = nullptr;
    if (dymu_device_alloc(ctx_, cells, &q) != DYMU_OK) return false;
    d_comb_mask_ = static_cast<uint8_t*>(q);
  }
  dymu_region box{};
  if (dymu_level_mask_device(ctx_, d_comb_, nx_, ny_, nx_, bound, d_comb_mask_, nx_, &box,
                             nullptr) != DYMU_OK)
    return false;
  if (dymu_memcpy_d2h(ctx_, mask, d_comb_mask_, cells) != DYMU_OK)
    throw std::runtime_error(std::string("dymu: corridor mask download failed: ") +
                             dymu_last_error(ctx_));
  if (info)
    *info = CorridorInfo{s.min_value, s.min_i, s.min_j, box.n_range, box.i0,
                         box.j0,      box.i1,  box.j1,  bound};
  return true;
}

bool DyMuPathPlanner::rendezvous(const std::vector<uint32_t>& planes,
                                 const std::vector<double>& weights,
                                 const std::vector<double>& offsets, bool minimax, unsigned* i,
                                 unsigned* j, double* value) {
  dymu_reduce_summary s{};
  if (!combineOnDevice(minimax ? 1 : 0, planes, weights, offsets, s) || s.n_finite == 0)
    return false;
  if (i) *i = s.min_i;
  if (j) *j = s.min_j;
  if (value) *value = s.min_value;
  return true;
}

bool DyMuPathPlanner::getTotalCosts(const std::vector<base::Waypoint>& points,
                                    std::vector<double>& out) {
  if (batch_goals_.empty() || !ctx_ || !dT_batch_ || points.size() > 0xffffffffull) return false;
  if (!refreshBatch()) return false;
  gatherBatch(points, out);
  return true;
}

void DyMuPathPlanner::gatherBatch(const std::vector<base::Waypoint>& points,
                                  std::vector<double>& out) {
  const uint32_t B = (uint32_t)batch_goals_.size(), M = (uint32_t)points.size();
  std::vector<double> res((uint64_t)B * M);
  if (M) {
    std::vector<double> xy(2 * (size_t)M);
    for (uint32_t m = 0; m < M; ++m) {
      xy[2 * m] = points[m].position[0] - global_offset_[0];
      xy[2 * m + 1] = points[m].position[1] - global_offset_[1];
    }
    auto check = [&](int rc, const char* what) {
      if (rc != DYMU_OK)
        throw std::runtime_error(std::string("dymu: getTotalCosts ") + what + " failed: " +
                                 dymu_strerror(rc) + " " + dymu_last_error(ctx_));
    };
    DeviceScratch dev(ctx_, "getTotalCosts");
    double* d_xy = dev.alloc<double>(xy.size());
    double* d_out = dev.alloc<double>(res.size());
    check(dymu_memcpy_h2d(ctx_, d_xy, xy.data(), sizeof(double) * xy.size()), "upload");
    check(dymu_gather_costs_device(ctx_, dT_batch_, nx_, ny_, B, nx_, global_res_, d_xy, M, d_out,
                                   nullptr),
          "kernel");
    check(dymu_memcpy_d2h(ctx_, res.data(), d_out, sizeof(double) * res.size()), "download");
  }
  out.swap(res);
}

bool DyMuPathPlanner::costMatrix(const std::vector<base::Waypoint>& goals,
                                 const std::vector<base::Waypoint>& targets,
                                 std::vector<double>& out) {
  return computeTotalCostMaps(goals) && getTotalCosts(targets, out);
}

// costMatrix with the batch solve stopped once the matrix's inputs are final (DESIGN.md
// s5.9).  The targets of the solve are the cells k_gather_costs / getTotalCost may read
// for each point, in every plane: the nearest node alone where a corner of the point's
// cell is off the grid, else the four corners (the nearest node is one of them).  A
// corner on an obstacle is ignored by the stop test and reads +inf either way; every
// other one is final on return, so the gather sees what it would see on converged maps.
bool DyMuPathPlanner::costMatrixUntil(const std::vector<base::Waypoint>& goals,
                                      const std::vector<base::Waypoint>& targets,
                                      std::vector<double>& out) {
  if (!&dymu_solve_batch_until_device || targets.size() > 0xffffffffull) return false;
  if (targets.empty()) return costMatrix(goals, targets, out);  // nothing to stop on
  std::vector<BatchGoal> bg;
  if (!prepareBatch(goals, bg)) return false;
  const uint32_t B = (uint32_t)bg.size();
  const uint64_t P = dymu_batch_plane_rows(ny_);
  std::vector<dymu_cell> cells;
  for (const base::Waypoint& w : targets) {
    const double x = w.position[0] - global_offset_[0], y = w.position[1] - global_offset_[1];
    const uint64_t i = grid_u32(x / global_res_), j = grid_u32(y / global_res_);
    const uint64_t ni = grid_u32(x / global_res_ + 0.5), nj = grid_u32(y / global_res_ + 0.5);
    if (i >= nx_ || j >= ny_ || i + 1 >= nx_ || j + 1 >= ny_) {
      if (ni < nx_ && nj < ny_) cells.push_back(dymu_cell{(uint32_t)ni, (uint32_t)nj});
    } else {
      for (uint32_t q = 0; q < 4; ++q)
        cells.push_back(dymu_cell{(uint32_t)i + (q & 1u), (uint32_t)j + (q >> 1)});
    }
  }
  if (cells.empty() || (uint64_t)cells.size() * B >= (1ull << 31))
    return costMatrix(goals, targets, out);  // every point reads +inf / too many cells
  std::vector<dymu_batch_seed> seeds;
  std::vector<dymu_batch_cell> tg;
  tg.reserve(cells.size() * B);
  for (uint32_t b = 0; b < B; ++b) {
    seeds.push_back(dymu_batch_seed{b, bg[b].i, bg[b].j, 0u, 0.0});
    for (const dymu_cell& c : cells) tg.push_back(dymu_batch_cell{b, c.i, c.j, 0u});
  }
  const uint64_t bytes = sizeof(double) * (uint64_t)B * P * nx_;
  void *pf = nullptr, *pt = nullptr;
  dymu_stats st{};
  double level = kInf;
  int rc = dymu_device_alloc(ctx_, bytes, &pf);
  if (rc == DYMU_OK) rc = dymu_device_alloc(ctx_, bytes, &pt);
  double* f = static_cast<double*>(pf);
  double* t = static_cast<double*>(pt);
  if (rc == DYMU_OK) rc = dymu_stack_speed_device(ctx_, dF_, nx_, 0, nx_, ny_, B, f, nx_, nullptr);
  if (rc == DYMU_OK)
    rc = dymu_solve_batch_until_device(ctx_, f, t, nx_, ny_, B, nx_, seeds.data(), B, tg.data(),
                                       (uint32_t)tg.size(), nullptr, &level, nullptr, &st);
  if (f) (void)dymu_device_free(ctx_, f);
  if (rc != DYMU_OK) {
    if (t) (void)dymu_device_free(ctx_, t);
    return false;
  }
  dropBatch();
  dT_batch_ = t;
  batch_goals_.swap(bg);
  batch_stats_ = st;
  batch_level_ = level;  // +inf: the solve ran to convergence, the batch is complete
  gatherBatch(targets, out);
  return true;
}

std::vector<std::vector<base::Waypoint>> DyMuPathPlanner::getPathsTo(
    unsigned b, const std::vector<base::Waypoint>& starts, std::vector<int>* status,
    unsigned max_wp, unsigned stride) {
  if (max_wp == 0 || stride == 0) throw std::invalid_argument("getPathsTo: max_wp, stride >= 1");
  if (b >= batch_goals_.size() || !ctx_ || !dT_batch_ || starts.size() > 0xffffffffull ||
      !refreshBatch())
    throw std::invalid_argument("getPathsTo: no such map in the batch");
  const size_t n = starts.size();
  std::vector<std::vector<base::Waypoint>> out(n);
  std::vector<int> st(n, -1), sk(n, -1);
  last_paths_device_ = false;
  last_paths_kernel_ms_ = 0.0;
  if (n) {
    const BatchGoal& g = batch_goals_[b];
    const PathTarget tgt{dT_batch_ + (uint64_t)b * dymu_batch_plane_rows(ny_) * nx_, g.i, g.j,
                         g.heading};
    pathsOnDevice(starts, out, st, sk, max_wp, stride, &tgt);
    last_paths_device_ = true;
  }
  if (status) status->swap(st);
  return out;
}

std::vector<DyMuPathPlanner::PathStats> DyMuPathPlanner::getPathStatsTo(
    unsigned b, const std::vector<base::Waypoint>& starts, unsigned max_wp, const double* field) {
  if (max_wp == 0) throw std::invalid_argument("getPathStatsTo: max_wp >= 1");
  if (b >= batch_goals_.size() || !ctx_ || !dT_batch_ || starts.size() > 0x7fffffffull ||
      max_wp > 0x7fffffffu || !&dymu_path_stats_device || !&dymu_last_path_stats_ms ||
      !refreshBatch())
    throw std::invalid_argument("getPathStatsTo: no such map in the batch");
  std::vector<PathStats> out(starts.size(), PathAccum::empty());
  last_paths_device_ = false;
  last_paths_kernel_ms_ = 0.0;
  if (!starts.empty()) {
    const BatchGoal& g = batch_goals_[b];
    const PathTarget tgt{dT_batch_ + (uint64_t)b * dymu_batch_plane_rows(ny_) * nx_, g.i, g.j,
                         g.heading};
    pathStatsOnDevice(starts, out, max_wp, field, &tgt);
    last_paths_device_ = true;
  }
  return out;
}

std::vector<std::vector<base::Waypoint>> DyMuPathPlanner::getArrivingPathsTo(
    unsigned b, const std::vector<base::Waypoint>& starts, std::vector<int>* status,
    unsigned max_wp, unsigned stride, std::vector<ArriveStats>* stats) {
  if (max_wp == 0 || stride == 0)
    throw std::invalid_argument("getArrivingPathsTo: max_wp, stride >= 1");
  if (b >= batch_goals_.size() || !ctx_ || !dT_batch_ || starts.size() > 0xffffffffull ||
      !&dymu_arrive_paths_device || !&dymu_last_arrive_ms || !refreshBatch())
    throw std::invalid_argument("getArrivingPathsTo: no such map in the batch");
  const size_t n = starts.size();
  std::vector<std::vector<base::Waypoint>> out(n);
  std::vector<int> st(n, -1), sk(n, -1);
  std::vector<ArriveStats> rec(n, kNoArrival);
  last_paths_device_ = false;
  last_paths_kernel_ms_ = 0.0;
  if (n) {
    const BatchGoal& g = batch_goals_[b];
    const PathTarget tgt{dT_batch_ + (uint64_t)b * dymu_batch_plane_rows(ny_) * nx_, g.i, g.j,
                         g.heading};
    pathsOnDevice(starts, out, st, sk, max_wp, stride, &tgt, &rec);
    last_paths_device_ = true;
  }
  if (status) status->swap(st);
  if (stats) stats->swap(rec);
  return out;
}

std::vector<std::vector<base::Waypoint>> DyMuPathPlanner::getSimplifiedPathsTo(
    unsigned b, const std::vector<base::Waypoint>& starts, double eps, std::vector<int>* status,
    unsigned max_wp, std::vector<ArriveStats>* stats, std::vector<std::vector<uint32_t>>* index) {
  simplified_check("getSimplifiedPathsTo", eps, max_wp);
  if (b >= batch_goals_.size() || !ctx_ || !dT_batch_ || starts.size() > 0xffffffffull ||
      max_wp > 0x7fffffffu || !&dymu_arrive_simplified_device ||
      !&dymu_last_arrive_simplified_ms || !refreshBatch())
    throw std::invalid_argument("getSimplifiedPathsTo: no such map in the batch");
  const size_t n = starts.size();
  std::vector<std::vector<base::Waypoint>> out(n);
  std::vector<int> st(n, -1), sk(n, -1);
  std::vector<ArriveStats> rec(n, kNoArrival);
  if (index) index->assign(n, std::vector<uint32_t>());
  last_paths_device_ = false;
  last_paths_kernel_ms_ = 0.0;
  last_simplified_reruns_ = last_simplified_bytes_ = 0;
  if (n) {
    const BatchGoal& g = batch_goals_[b];
    const PathTarget tgt{dT_batch_ + (uint64_t)b * dymu_batch_plane_rows(ny_) * nx_, g.i, g.j,
                         g.heading};
    simplifiedOnDevice(starts, eps, out, st, sk, max_wp, &tgt, rec, index);
    last_paths_device_ = true;
  }
  if (status) status->swap(st);
  if (stats) stats->swap(rec);
  return out;
}

std::vector<DyMuPathPlanner::ArriveStats> DyMuPathPlanner::getArrivingStatsTo(
    unsigned b, const std::vector<base::Waypoint>& starts, unsigned max_wp) {
  if (max_wp == 0) throw std::invalid_argument("getArrivingStatsTo: max_wp >= 1");
  if (b >= batch_goals_.size() || !ctx_ || !dT_batch_ || starts.size() > 0xffffffffull ||
      max_wp > 0x7fffffffu || !&dymu_arrive_paths_device || !&dymu_last_arrive_ms ||
      !refreshBatch())
    throw std::invalid_argument("getArrivingStatsTo: no such map in the batch");
  std::vector<ArriveStats> out(starts.size(), kNoArrival);
  last_paths_device_ = false;
  last_paths_kernel_ms_ = 0.0;
  if (!starts.empty()) {
    const BatchGoal& g = batch_goals_[b];
    const PathTarget tgt{dT_batch_ + (uint64_t)b * dymu_batch_plane_rows(ny_) * nx_, g.i, g.j,
                         g.heading};
    arriveStatsOnDevice(starts, out, max_wp, &tgt);
    last_paths_device_ = true;
  }
  return out;
}

DyMuPathPlanner::RouteFields DyMuPathPlanner::getRouteFieldsTo(unsigned b,
                                                              const RouteRequest& rq) {
  route_check_request(rq);
  if (b >= batch_goals_.size() || !ctx_ || !dT_batch_ || !dF_ ||
      (uint64_t)nx_ * ny_ >= (1ull << 31) || !&dymu_route_fields_device ||
      !&dymu_route_fields_workspace || !&dymu_last_route_fields_ms ||
      !&dymu_device_alloc_cached || !refreshBatch())
    throw std::invalid_argument("getRouteFieldsTo: no such map in the batch");
  RouteFields out;
  last_paths_device_ = false;
  last_paths_kernel_ms_ = 0.0;
  const BatchGoal& g = batch_goals_[b];
  routeFieldsOnDevice(rq, dT_batch_ + (uint64_t)b * dymu_batch_plane_rows(ny_) * nx_,
                      {dymu_seed{g.i, g.j, 0.0}}, out);
  last_paths_device_ = true;
  return out;
}

DyMuPathPlanner::RouteUsage DyMuPathPlanner::getRouteUsageTo(unsigned b,
                                                            const RouteUsageRequest& rq) {
  if (b >= batch_goals_.size() || !ctx_ || !dT_batch_ || !(rq.outputs & kUsageAll) ||
      (uint64_t)nx_ * ny_ >= (1ull << 31) || !&dymu_route_usage_device ||
      !&dymu_route_usage_workspace || !&dymu_last_route_usage_ms ||
      !&dymu_device_alloc_cached || !refreshBatch())
    throw std::invalid_argument("getRouteUsageTo: no such map in the batch");
  RouteUsage out;
  last_paths_device_ = false;
  last_paths_kernel_ms_ = 0.0;
  const BatchGoal& g = batch_goals_[b];
  routeUsageOnDevice(rq, dT_batch_ + (uint64_t)b * dymu_batch_plane_rows(ny_) * nx_,
                     {dymu_seed{g.i, g.j, 0.0}}, out);
  last_paths_device_ = true;
  return out;
}

}  // namespace PathPlanning_lib
