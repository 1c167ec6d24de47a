// descent_step.h -- the one continuous descent step of the path kernels
// (path_kernels.hip, path_stats_kernels.hip, arrive_kernels.hip) on the device-resident
// total cost, and the grid-coordinate casts they share with batch_kernels.hip.
//
// The step is the reference's computeNextGlobalWaypoint / gradientNode / interpolate
// (src/DyMu_GlobalPathPlanning.cpp:666-784 as restated in planner.cpp).  Every expression
// is the host's, in the host's order, and the files that include this header are built
// with -ffp-contract=off like the host code: fp64 add / sub / mul / div / sqrt round the
// same on both sides, so a kernel's x, y and counts come out bit-identical to the host
// loop on the same T.  A change to an expression here changes all three
// kernels at once and must be made in planner.cpp's nextWaypoint / gradientNode too.
//
// A step touches the 4x4 block of cells around (cx, cy) without its corners (the stencils
// of the cell's four corner nodes).  A step is 0.4 cell, so most steps stay in their cell:
// the 12 values are loaded together when the cell changes (one latency per reload) and the
// four corner gradients -- functions of those values alone -- are kept in registers until
// it changes again (HeldCell).  Everything here is __forceinline__ and takes values, not
// argument blocks: the state stays in registers, no array is indexed at run time.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace dymu {

constexpr double kInfD = __builtin_huge_val();

// planner.cpp's path_cell: the cell index of grid coordinate g (truncation like
// the reference's (uint) cast of an in-range value), tested in 64-bit; false
// when the cell or its +1 neighbour is off a grid of n nodes (negative, huge
// and NaN coordinates included)
__device__ __forceinline__ bool path_cell(double g, uint32_t n, int64_t& c) {
  if (!(g > -9.2e18 && g < 9.2e18)) return false;
  c = (int64_t)g;
  return c >= 0 && c + 1 < (int64_t)n;
}

// local_layer.hpp's grid_u32: the reference's (uint) cast of an in-range value
__device__ __forceinline__ uint32_t grid_u32(double d) {
  return (d > -9.2e18 && d < 9.2e18) ? (uint32_t)(int64_t)d : 0u;
}

// gradientNode (:718-772) of a node from its values: h* = the neighbour exists
__device__ __forceinline__ void gradient_node(bool hw, bool he, bool hs, bool hn, double tw,
                                              double te, double ts, double tn, double t,
                                              double& dnx, double& dny) {
  double dx, dy;
  if ((!hw && !he) || (hw && he && tw == kInfD && te == kInfD)) dx = 0;
  else if (!hw || tw == kInfD) dx = te - t;
  else if (!he || te == kInfD) dx = t - tw;
  else dx = (te - tw) * 0.5;
  if ((!hs && !hn) || (hs && hn && ts == kInfD && tn == kInfD)) dy = 0;
  else if (!hs || ts == kInfD) dy = tn - t;
  else if (!hn || tn == kInfD) dy = t - ts;
  else dy = (tn - ts) * 0.5;
  if (dx == 0 && dy == 0) {
    dnx = 0;
    dny = 0;
  } else {
    const double r = sqrt(dx * dx + dy * dy);
    dnx = dx / r;
    dny = dy / r;
  }
}

// interpolate (:776-784)
__device__ __forceinline__ double interpolate(double a, double b, double g00, double g01,
                                              double g10, double g11) {
  return g00 + (g10 - g00) * a + (g01 - g00) * b + (g11 + g00 - g10 - g01) * a * b;
}

__device__ __forceinline__ double dist2d(double ax, double ay, double bx, double by) {
  const double dx = ax - bx, dy = ay - by;
  return sqrt(dx * dx + dy * dy);
}

// The 4x4 block around cell (cx, cy), which is inside the grid: rows cy-1 .. cy+2
// (r0 .. r3) and columns cx-1 .. cx+2 (i0, cx, cx + 1, i3).  An index off the grid is
// clamped for the load and its value never used: *_ok = the row or column exists.
struct Stencil {
  const double *r0, *r1, *r2, *r3;
  int64_t i0, i3;
  bool w_ok, e_ok, s_ok, n_ok;
};
__device__ __forceinline__ Stencil stencil_of(const double* T, int64_t ld, int64_t nx, int64_t ny,
                                              int64_t cx, int64_t cy) {
  Stencil s;
  s.i0 = cx > 0 ? cx - 1 : 0, s.i3 = cx + 2 < nx ? cx + 2 : nx - 1;
  const int64_t j0 = cy > 0 ? cy - 1 : 0, j3 = cy + 2 < ny ? cy + 2 : ny - 1;
  s.r0 = T + j0 * ld;
  s.r1 = T + cy * ld;
  s.r2 = s.r1 + ld;
  s.r3 = T + j3 * ld;
  s.w_ok = cx > 0, s.e_ok = cx + 2 < nx, s.s_ok = cy > 0, s.n_ok = cy + 2 < ny;
  return s;
}

// The cell whose four corner gradients a lane holds, and the gradients
struct HeldCell {
  int64_t ccx = -1, ccy = -1;
  double gx00 = 0, gx10 = 0, gx01 = 0, gx11 = 0, gy00 = 0, gy10 = 0, gy01 = 0, gy11 = 0;

  __device__ __forceinline__ bool holds(int64_t cx, int64_t cy) const {
    return cx == ccx && cy == ccy;
  }
  __device__ __forceinline__ void drop() { ccx = ccy = -1; }

  // cell (cx, cy) from the block without its corners, t<row><column> as Stencil names them
  __device__ __forceinline__ void set(int64_t cx, int64_t cy, bool w_ok, bool e_ok, bool s_ok,
                                      bool n_ok, double t01, double t02, double t10, double t11,
                                      double t12, double t13, double t20, double t21, double t22,
                                      double t23, double t31, double t32) {
    gradient_node(w_ok, true, s_ok, true, t10, t12, t01, t21, t11, gx00, gy00);
    gradient_node(true, e_ok, s_ok, true, t11, t13, t02, t22, t12, gx10, gy10);
    gradient_node(w_ok, true, true, n_ok, t20, t22, t11, t31, t21, gx01, gy01);
    gradient_node(true, e_ok, true, n_ok, t21, t23, t12, t32, t22, gx11, gy11);
    ccx = cx;
    ccy = cy;
  }

  // the same with the 12 loads, issued together
  __device__ __forceinline__ void load(const double* T, int64_t ld, int64_t nx, int64_t ny,
                                       int64_t cx, int64_t cy) {
    const Stencil s = stencil_of(T, ld, nx, ny, cx, cy);
    const double t01 = s.r0[cx], t02 = s.r0[cx + 1];
    const double t10 = s.r1[s.i0], t11 = s.r1[cx], t12 = s.r1[cx + 1], t13 = s.r1[s.i3];
    const double t20 = s.r2[s.i0], t21 = s.r2[cx], t22 = s.r2[cx + 1], t23 = s.r2[s.i3];
    const double t31 = s.r3[cx], t32 = s.r3[cx + 1];
    set(cx, cy, s.w_ok, s.e_ok, s.s_ok, s.n_ok, t01, t02, t10, t11, t12, t13, t20, t21, t22, t23,
        t31, t32);
  }

  // the candidate of computeNextGlobalWaypoint (:666-714) from (x, y) with grid coordinates
  // (gx, gy) in the held cell (cx, cy): the direction and the next waypoint
  __device__ __forceinline__ void candidate(double x, double y, double gx, double gy, int64_t cx,
                                            int64_t cy, double res_tau, double& dcx, double& dcy,
                                            double& nxt_x, double& nxt_y) const {
    const double ax = gx - (double)cx, ay = gy - (double)cy;
    dcx = interpolate(ax, ay, gx00, gx01, gx10, gx11);
    dcy = interpolate(ax, ay, gy00, gy01, gy10, gy11);
    nxt_x = x - res_tau * dcx;
    nxt_y = y - res_tau * dcy;
  }
};

// Goal sets: the sink follows the label map.  When the held cell changes,
// the sink becomes the goal labelled on that cell (index `cell` of the pitch-nx map, inside
// the grid); a cell without a label keeps the previous sink.
__device__ __forceinline__ void label_sink(const uint32_t* label, const double* goal_xy,
                                           uint32_t n_goals, int64_t cell, double& sink_x,
                                           double& sink_y, int32_t& sink_k) {
  const uint32_t lab = label[cell];
  if (lab < n_goals) {
    sink_x = goal_xy[2 * (uint64_t)lab];
    sink_y = goal_xy[2 * (uint64_t)lab + 1];
    sink_k = (int32_t)lab;
  }
}

}  // namespace dymu
