// path_kernels.hip -- batched path extraction on the device-resident total cost.
//
// k_extract_paths: one lane per path, each running the reference's gradient
// descent (computeGlobalPath / computeNextGlobalWaypoint / gradientNode /
// interpolate, src/DyMu_GlobalPathPlanning.cpp:615-784 as restated in
// planner.cpp) on the row-major fp64 T.  Every expression is the host's, in the
// host's order, and this file is built with -ffp-contract=off like the host
// code: fp64 add / sub / mul / div / sqrt round the same on both sides, so x, y
// and the waypoint count come out bit-identical to the host loop on the same T
// (DESIGN.md s5.3).  The heading (atan2) and z are left to the host: a waypoint
// carries the (dcx, dcy) that produced it in its two spare slots.
//
// A step touches the 4x4 block of cells around (cx, cy) without its corners
// (the stencils of the cell's four corner nodes).  A step is 0.4 cell, so most
// steps stay in their cell: the 12 values are loaded together when the cell
// changes (one latency per reload) and the four corner gradients -- functions
// of those values alone -- are kept in registers until it changes again.
#include "fim_kernels.h"

namespace dymu {
namespace {

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

// GOALS: the sink is per path and follows the label map (goal sets):
// whenever the cell the lane holds gradients for changes, the sink becomes the goal
// labelled on that cell; a cell without a label keeps the previous sink, and a path
// whose first cell has none ends with status -1.  GOALS = false is the single-sink
// kernel, unchanged.
template <bool GOALS>
__global__ __launch_bounds__(64) void k_extract_paths(PathArgs a) {
  const uint32_t p = blockIdx.x * 64u + threadIdx.x;
  if (p >= a.n_paths) return;
  double x = a.start_xy[2 * (uint64_t)p], y = a.start_xy[2 * (uint64_t)p + 1];
  double* out = a.out + (uint64_t)p * a.max_wp * 4;
  const int64_t nx = a.nx, ny = a.ny, ld = a.ld;
  // every lane's loop ends after at most max_wp * stride steps
  const uint64_t limit = (uint64_t)a.max_wp * a.stride;
  uint32_t n = 0, phase = 0;
  int32_t status = 1;
  double pdx = 0, pdy = 0;  // the direction that produced the current waypoint
  int64_t ccx = -1, ccy = -1;  // the cell whose corner gradients are held
  double gx00 = 0, gx10 = 0, gx01 = 0, gx11 = 0, gy00 = 0, gy10 = 0, gy01 = 0, gy11 = 0;
  double sink_x = a.sink_x, sink_y = a.sink_y;
  int32_t sink_k = -1;  // GOALS: the goal of the current sink
  for (uint64_t w = 0;; ++w) {
    // (x, y) is the path's waypoint w unless the descent ends here
    if (w > 0 && !(dist2d(x, y, sink_x, sink_y) > a.two_res)) break;  // NaN ends it too (Q5)
    if (w == limit) {
      status = -3;
      break;
    }
    // computeNextGlobalWaypoint (:666-714)
    const double gx = x / a.res, gy = y / a.res;
    int64_t cx = 0, cy = 0;
    double nxt_x = __builtin_nan(""), nxt_y = nxt_x, dcx = 0, dcy = 0;
    // no load before both indices are proven inside the grid
    const bool in_x = path_cell(gx, a.nx, cx), in_y = path_cell(gy, a.ny, cy);
    if (in_x && in_y) {
      if (cx != ccx || cy != ccy) {
        // rows cy-1 .. cy+2, columns cx-1 .. cx+2 without the corners; an index off
        // the grid is clamped for the load and its value never used
        const int64_t i0 = cx > 0 ? cx - 1 : 0, i3 = cx + 2 < nx ? cx + 2 : nx - 1;
        const int64_t j0 = cy > 0 ? cy - 1 : 0, j3 = cy + 2 < ny ? cy + 2 : ny - 1;
        const double* r0 = a.T + j0 * ld;
        const double* r1 = a.T + cy * ld;
        const double* r2 = r1 + ld;
        const double* r3 = a.T + j3 * ld;
        const double t01 = r0[cx], t02 = r0[cx + 1];
        const double t10 = r1[i0], t11 = r1[cx], t12 = r1[cx + 1], t13 = r1[i3];
        const double t20 = r2[i0], t21 = r2[cx], t22 = r2[cx + 1], t23 = r2[i3];
        const double t31 = r3[cx], t32 = r3[cx + 1];
        const bool w_ok = cx > 0, e_ok = cx + 2 < nx, s_ok = cy > 0, n_ok = cy + 2 < ny;
        gradient_node(w_ok, true, s_ok, true, t10, t12, t01, t21, t11, gx00, gy00);
        gradient_node(true, e_ok, s_ok, true, t11, t13, t02, t22, t12, gx10, gy10);
        gradient_node(w_ok, true, true, n_ok, t20, t22, t11, t31, t21, gx01, gy01);
        gradient_node(true, e_ok, true, n_ok, t21, t23, t12, t32, t22, gx11, gy11);
        ccx = cx;
        ccy = cy;
        if (GOALS) {  // the cell is inside the grid: cy * nx + cx < nx * ny
          const uint32_t lab = a.label[cy * nx + cx];
          if (lab < a.n_goals) {
            sink_x = a.goal_xy[2 * (uint64_t)lab];
            sink_y = a.goal_xy[2 * (uint64_t)lab + 1];
            sink_k = (int32_t)lab;
          }
        }
      }
      const double ax = gx - (double)cx, ay = gy - (double)cy;
      dcx = interpolate(ax, ay, gx00, gx01, gx10, gx11);
      dcy = interpolate(ax, ay, gy00, gy01, gy10, gy11);
      nxt_x = x - a.res_tau * dcx;
      nxt_y = y - a.res_tau * dcy;
    }
    if (w == 0 && (nxt_x != nxt_x || nxt_y != nxt_y)) {  // :628-633
      status = -1;
      break;
    }
    if (GOALS && w == 0 && sink_k < 0) {  // no goal drains the start's cell
      status = -1;
      break;
    }
    if (phase == 0) {  // n < max_wp: w < max_wp * stride
      double* o = out + 4 * (uint64_t)n;
      o[0] = x;
      o[1] = y;
      o[2] = pdx;
      o[3] = pdy;
      ++n;
    }
    if (++phase == a.stride) phase = 0;
    if (w > 0 && dist2d(x, y, nxt_x, nxt_y) < a.stall) {  // "ERROR in trajectory" (:650-656)
      status = 0;
      break;
    }
    x = nxt_x;
    y = nxt_y;
    pdx = dcx;
    pdy = dcy;
  }
  if (status == 1) {
    if (n < a.max_wp) {
      double* o = out + 4 * (uint64_t)n;
      o[0] = sink_x;
      o[1] = sink_y;
      o[2] = 0;
      o[3] = 0;
      ++n;
    } else {
      status = -3;
    }
  }
  a.count[p] = (int32_t)n;
  a.status[p] = status;
  if (GOALS) a.sink[p] = status == 1 ? sink_k : -1;
}

}  // namespace

hipError_t launch_extract_paths(const PathArgs& a, hipStream_t st) {
  if (a.n_paths == 0) return hipSuccess;
  const uint32_t blocks = (a.n_paths + 63u) / 64u;
  hipLaunchKernelGGL(k_extract_paths<false>, dim3(blocks), dim3(64), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_extract_paths_goals(const PathArgs& a, hipStream_t st) {
  if (a.n_paths == 0) return hipSuccess;
  const uint32_t blocks = (a.n_paths + 63u) / 64u;
  hipLaunchKernelGGL(k_extract_paths<true>, dim3(blocks), dim3(64), 0, st, a);
  return hipGetLastError();
}

}  // namespace dymu
