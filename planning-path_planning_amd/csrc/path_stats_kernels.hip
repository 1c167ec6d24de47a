// path_stats_kernels.hip -- per-path summaries of the reference's descent on the
// device-resident total cost (DyMuPathPlanner::getPathStats).
//
// k_path_stats runs k_extract_paths' descent (the step of descent_step.h, which states
// the bit-identity contract with the host loop) and stores no waypoint.  It keeps the previous waypoint in registers and accumulates one record per
// path: outcome, waypoint count, length, last hop, and for up to kPathFields sampled
// fields the integral along the path, the minimum, the maximum and the number of
// samples skipped.  The record is defined on the host loop (planner.cpp, PathAccum) and
// every sum is taken in that loop's order, so host and device agree bit for bit.
//
// A sample is the field at the waypoint's nearest node (nearestIndex's rule).  That
// node changes about as rarely as the cell, so the node's field values stay in
// registers and are loaded again only when the node changes; those loads are issued
// ahead of the stencil's, and their values are first used after the stencil block, so
// a step that changes both waits once.
//
// Work queue: the grid is a fixed number of lanes.  A lane that finishes a path takes
// the next path index from a device counter and goes on in the same loop -- the idle
// lanes of a wave fetch together, one atomic add for all of them.  A record depends on
// its path alone, never on the lane that ran it.
#include "descent_step.h"
#include "fim_kernels.h"

namespace dymu {
namespace {

// The record of one path while it is built (planner.cpp's PathAccum): everything stays
// in registers, NF is a compile-time count so that no array is indexed at run time.
template <int NF>
struct Accum {
  double px, py;  // the previous waypoint
  double length, last_hop;
  double fv[NF ? NF : 1];  // the held node's field values: the previous waypoint's samples
  double integral[NF ? NF : 1], vmin[NF ? NF : 1], vmax[NF ? NF : 1];
  uint32_t skipped[NF ? NF : 1];
  uint32_t ok;  // bit f: the previous waypoint's sample of field f counts
  uint32_t n;   // waypoints so far

  __device__ __forceinline__ void reset() {
    px = py = length = last_hop = 0;
    ok = n = 0;
#pragma unroll
    for (int f = 0; f < NF; ++f) {
      fv[f] = integral[f] = 0;
      vmin[f] = kInfD;
      vmax[f] = -kInfD;
      skipped[f] = 0;
    }
  }

  // waypoint (x, y) joins the record.  in: its nearest node is on the grid; fresh: that
  // node is not the held one and nv[] holds its values (else fv[] are the node's)
  __device__ __forceinline__ void add(double x, double y, bool in, bool fresh,
                                      const double (&nv)[NF ? NF : 1]) {
    if (n > 0) {
      const double seg = dist2d(px, py, x, y);
      length = length + seg;
      last_hop = seg;
#pragma unroll
      for (int f = 0; f < NF; ++f)
        if (ok >> f & 1u) integral[f] = integral[f] + fv[f] * seg;
    }
    ok = 0;
#pragma unroll
    for (int f = 0; f < NF; ++f) {
      if (fresh) fv[f] = nv[f];
      const double v = fv[f];
      if (in && v < kInfD && v > -kInfD) {
        vmin[f] = v < vmin[f] ? v : vmin[f];
        vmax[f] = v > vmax[f] ? v : vmax[f];
        ok |= 1u << f;
      } else {
        ++skipped[f];
      }
    }
    px = x;
    py = y;
    ++n;
  }
};

template <bool GOALS, int NF>
__global__ __launch_bounds__(64) void k_path_stats(PathStatArgs a) {
  const int64_t nx = a.nx, ny = a.ny, ld = a.ld;
  uint32_t p = 0;
  bool idle = true;
  double x = 0, y = 0;
  int32_t status = 1;
  HeldCell cell;
  double sink_x = a.sink_x, sink_y = a.sink_y;
  int32_t sink_k = -1;
  uint32_t hni = 0xffffffffu, hnj = 0xffffffffu;  // the node whose field values are held
  Accum<NF> acc;
  acc.reset();
  for (;;) {
    if (idle) {
      // the idle lanes of the wave take consecutive path indices with one atomic add
      const unsigned long long m = __ballot(1);
      const uint32_t rank = __builtin_amdgcn_mbcnt_hi(
          (uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
      uint32_t base = 0;
      if (rank == 0) base = atomicAdd(a.next, (uint32_t)__popcll(m));
      p = (uint32_t)__builtin_amdgcn_readfirstlane((int)base) + rank;
      if (p >= a.n_paths) break;  // every later fetch would be past the end too
      x = a.start_xy[2 * (uint64_t)p];
      y = a.start_xy[2 * (uint64_t)p + 1];
      status = 1;
      cell.drop();
      hni = hnj = 0xffffffffu;
      sink_x = a.sink_x;
      sink_y = a.sink_y;
      sink_k = GOALS ? -1 : 0;
      acc.reset();
      idle = false;
    }
    // (x, y) is the path's waypoint acc.n unless the descent ends here; every path ends
    // after at most max_wp steps
    bool done = false;
    if (acc.n > 0 && !(dist2d(x, y, sink_x, sink_y) > a.two_res)) {  // NaN ends it too (Q5)
      done = true;
    } else if (acc.n == a.max_wp) {
      status = -3;
      done = true;
    } else {
      // computeNextGlobalWaypoint (:666-714), as k_extract_paths
      const double gx = x / a.res, gy = y / a.res;
      int64_t cx = 0, cy = 0;
      double nxt_x = __builtin_nan(""), nxt_y = nxt_x, dcx = 0, dcy = 0;
      // no load before its indices are proven inside the grid
      const bool in_x = path_cell(gx, a.nx, cx), in_y = path_cell(gy, a.ny, cy);
      // the nearest node (nearestIndex): its field values, ahead of the stencil's loads
      const uint32_t ni = grid_u32(gx + 0.5), nj = grid_u32(gy + 0.5);
      const bool node_in = ni < a.nx && nj < a.ny;
      const bool fresh = node_in && (ni != hni || nj != hnj);
      double nv[NF ? NF : 1] = {};
      if (fresh) {
#pragma unroll
        for (int f = 0; f < NF; ++f) nv[f] = a.field[f][(int64_t)nj * a.field_ld[f] + ni];
        hni = ni;
        hnj = nj;
      }
      if (in_x && in_y) {
        if (!cell.holds(cx, cy)) {
          cell.load(a.T, ld, nx, ny, cx, cy);
          // the cell is inside the grid: cy * nx + cx < nx * ny
          if (GOALS)
            label_sink(a.label, a.goal_xy, a.n_goals, cy * nx + cx, sink_x, sink_y, sink_k);
        }
        cell.candidate(x, y, gx, gy, cx, cy, a.res_tau, dcx, dcy, nxt_x, nxt_y);
      }
      if (acc.n == 0 && ((nxt_x != nxt_x || nxt_y != nxt_y) || (GOALS && sink_k < 0))) {
        status = -1;  // :628-633, or no goal drains the start's cell: an empty record
        done = true;
      } else {
        const bool first = acc.n == 0;
        acc.add(x, y, node_in, fresh, nv);
        if (!first && dist2d(x, y, nxt_x, nxt_y) < a.stall) {  // "ERROR in trajectory"
          status = 0;
          done = true;
        }
        x = nxt_x;
        y = nxt_y;
      }
    }
    if (done) {
      if (status == 1) {
        if (acc.n < a.max_wp) {  // the sink is the last waypoint; its node's samples
          const uint32_t ni = grid_u32(sink_x / a.res + 0.5), nj = grid_u32(sink_y / a.res + 0.5);
          const bool node_in = ni < a.nx && nj < a.ny;
          const bool fresh = node_in && (ni != hni || nj != hnj);
          double nv[NF ? NF : 1] = {};
          if (fresh) {
#pragma unroll
            for (int f = 0; f < NF; ++f) nv[f] = a.field[f][(int64_t)nj * a.field_ld[f] + ni];
          }
          acc.add(sink_x, sink_y, node_in, fresh, nv);
        } else {
          status = -3;
        }
      }
      PathStatRec* o = a.out + p;
      o->status = status;
      o->sink = status == 1 ? sink_k : -1;
      o->count = acc.n;
      o->reserved = 0;
      o->length = acc.length;
      o->last_hop = acc.last_hop;
#pragma unroll
      for (int f = 0; f < kPathFields; ++f) {
        o->integral[f] = f < NF ? acc.integral[f < NF ? f : 0] : 0.0;
        o->vmin[f] = f < NF ? acc.vmin[f < NF ? f : 0] : kInfD;
        o->vmax[f] = f < NF ? acc.vmax[f < NF ? f : 0] : -kInfD;
        o->skipped[f] = f < NF ? acc.skipped[f < NF ? f : 0] : 0u;
      }
      idle = true;
    }
  }
}

template <bool GOALS>
hipError_t launch_nf(const PathStatArgs& a, uint32_t n_fields, uint32_t blocks, hipStream_t st) {
  switch (n_fields) {
    case 0: hipLaunchKernelGGL((k_path_stats<GOALS, 0>), dim3(blocks), dim3(64), 0, st, a); break;
    case 1: hipLaunchKernelGGL((k_path_stats<GOALS, 1>), dim3(blocks), dim3(64), 0, st, a); break;
    case 2: hipLaunchKernelGGL((k_path_stats<GOALS, 2>), dim3(blocks), dim3(64), 0, st, a); break;
    case 3: hipLaunchKernelGGL((k_path_stats<GOALS, 3>), dim3(blocks), dim3(64), 0, st, a); break;
    case 4: hipLaunchKernelGGL((k_path_stats<GOALS, 4>), dim3(blocks), dim3(64), 0, st, a); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace

hipError_t launch_path_stats(const PathStatArgs& a, uint32_t n_fields, uint32_t lanes,
                             hipStream_t st) {
  if (a.n_paths == 0) return hipSuccess;
  const uint32_t blocks = (lanes + 63u) / 64u;
  if (blocks == 0) return hipErrorInvalidValue;
  return a.label ? launch_nf<true>(a, n_fields, blocks, st) : launch_nf<false>(a, n_fields, blocks, st);
}

}  // namespace dymu
