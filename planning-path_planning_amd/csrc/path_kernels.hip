// path_kernels.hip -- batched path extraction on the device-resident total cost.
//
// k_extract_paths: one lane per path, each running the reference's gradient
// descent (computeGlobalPath, src/DyMu_GlobalPathPlanning.cpp:615-660 as restated in
// planner.cpp) with the step of descent_step.h, which states the bit-identity
// contract with the host loop and how a lane holds its cell's gradients.  The
// heading (atan2) and z are left to the host: a waypoint carries the (dcx, dcy)
// that produced it in its two spare slots.
#include "descent_step.h"
#include "fim_kernels.h"

namespace dymu {
namespace {

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
  HeldCell cell;
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
      if (!cell.holds(cx, cy)) {
        cell.load(a.T, ld, nx, ny, cx, cy);
        // the cell is inside the grid: cy * nx + cx < nx * ny
        if (GOALS) label_sink(a.label, a.goal_xy, a.n_goals, cy * nx + cx, sink_x, sink_y, sink_k);
      }
      cell.candidate(x, y, gx, gy, cx, cy, a.res_tau, dcx, dcy, nxt_x, nxt_y);
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
