// arrive_kernels.hip -- the arriving descent on the device-resident total cost
// (DyMuPathPlanner::getArrivingPaths / getArrivingStats).
//
// k_arrive_paths: one lane per path.  A path takes k_extract_paths' continuous step
// (descent_step.h, which states the bit-identity contract) wherever that step is valid,
// and a node-to-node step on T wherever it is not; it never enters an obstacle node's
// square and ends on the sink's node.  The rule is DyMuPathPlanner::descendArriving (planner.cpp), statement for
// statement, so x, y, the counts, the hops and the length are the host's bits.
//
// A lane holds two things between steps, each renewed only when it changes:
//   - the four corner gradients of the cell it is in (from the 12 stencil values of
//     k_extract_paths), and
//   - the 3x3 block of T around its node n: every test of a step -- the candidate's node,
//     the two side nodes of a diagonal move, the eight neighbours of a hop -- reads that
//     block and nothing else.
// A node is a corner of the cell its position is in, so its 3x3 block lies inside the 4x4
// block around that cell: the cell change loads all 16 values together (the stencil and
// the four corners), the lane keeps them, and a node change inside the cell takes its
// nine values from them by selects -- no load, no array indexed at run time.  Only a node
// that is in no cell (a hop along the last row or column) loads its own nine.  Every
// index is clamped for its load and a value from outside the grid is replaced by +inf,
// which no test accepts.
#include "descent_step.h"
#include "fim_kernels.h"
#include "path_simplify.h"

namespace dymu {
namespace {

constexpr double kDiag = 0.7071067811865476;  // a diagonal hop's score per unit of T

// planner.cpp's arrive_node: the node of coordinate v with grid coordinate g = v / res
// (nearestIndex's rounding); false off a grid of n nodes -- negative and NaN included
__device__ __forceinline__ bool arrive_node(double v, double g, uint32_t n, uint32_t& i) {
  if (!(v >= 0.0)) return false;
  const double h = g + 0.5;
  if (!(h < 4294967296.0)) return false;
  i = (uint32_t)h;
  return i < n;
}

// one of three named values by d in {-1, 0, +1}: no array is indexed at run time
__device__ __forceinline__ double pick3(int d, double m, double z, double p) {
  return d < 0 ? m : d > 0 ? p : z;
}

// a hop's candidate (di, dj) with value tm and score factor: the largest score wins, the
// first in the order among equals
__device__ __forceinline__ void hop_try(bool ok, double tn, double tm, bool diag, int di, int dj,
                                        double& best, int& bi, int& bj) {
  if (ok && tm < tn) {
    const double s = diag ? (tn - tm) * kDiag : tn - tm;
    if (s > best) {
      best = s;
      bi = di;
      bj = dj;
    }
  }
}

// GOALS: the sink is the goal labelled on the path's node, looked up when the node
// changes; STORE: the kept waypoints go to a.out (else only the record is written);
// SIMPLIFY: the waypoints walked (stride 1, at most max_wp) pass through the rule of
// path_simplify.h, and only those it keeps -- the first max_kept of them -- take a slot
template <bool GOALS, bool STORE, bool SIMPLIFY>
__global__ __launch_bounds__(64) void k_arrive_paths(ArriveArgs a) {
  const uint32_t p = blockIdx.x * 64u + threadIdx.x;
  if (p >= a.n_paths) return;
  double x = a.start_xy[2 * (uint64_t)p], y = a.start_xy[2 * (uint64_t)p + 1];
  double* out = STORE ? a.out + (uint64_t)p * (SIMPLIFY ? a.max_kept : a.max_wp) * 4 : nullptr;
  // SIMPLIFY: the rule's state, the direction of the previous waypoint's slot (its
  // position is (px, py)), the waypoints the rule kept, and where their numbers go
  PathSimplifier sim;
  double qdx = 0, qdy = 0;
  uint32_t skept = 0;
  uint32_t* index = SIMPLIFY && a.index ? a.index + (uint64_t)p * a.max_kept : nullptr;
  // the rule keeps waypoint i of the walk, whose slot is (ex, ey, edx, edy)
  auto keep = [&](double ex, double ey, double edx, double edy, uint32_t i) {
    if (skept < a.max_kept) {
      if (STORE) {
        double* o = out + 4 * (uint64_t)skept;
        o[0] = ex;
        o[1] = ey;
        o[2] = edx;
        o[3] = edy;
      }
      if (index) index[skept] = i;
    }
    ++skept;
  };
  const int64_t nx = a.nx, ny = a.ny, ld = a.ld;
  // every lane's loop ends after at most max_wp * stride steps
  const uint64_t limit = (uint64_t)a.max_wp * a.stride;
  int32_t status = -1, sink_k = GOALS ? -1 : 0;
  uint32_t count = 0, hops = 0, kept = 0, phase = 0, same = 0;
  double length = 0, start_cost = 0;
  double sink_x = a.sink_x, sink_y = a.sink_y;
  uint32_t sni = a.goal_i, snj = a.goal_j;  // the sink's node
  uint32_t ni = 0, nj = 0;
  // no load before the start's node is proven on the grid
  double gx = x / a.res, gy = y / a.res;  // the grid coordinates of (x, y)
  bool alive = arrive_node(x, gx, a.nx, ni) && arrive_node(y, gy, a.ny, nj);
  // the 3x3 block of T around (ni, nj): t<column><row>, m / 0 / p = -1 / 0 / +1
  double tmm = kInfD, t0m = kInfD, tpm = kInfD, tm0 = kInfD, t00 = kInfD, tp0 = kInfD,
         tmp = kInfD, t0p = kInfD, tpp = kInfD;
  bool fresh = alive;  // the block is not that of (ni, nj) yet
  uint32_t lab_held = 0xffffffffu;  // GOALS: the label whose goal (sni, snj) is
  double px = 0, py = 0;            // the previous waypoint
  double pdx = 0, pdy = 0;          // the direction that produced the current waypoint
  HeldCell cell;
  // the 4x4 block of T around the held cell, b<row><column>: rows ccy-1 .. ccy+2, columns
  // ccx-1 .. ccx+2 (where the grid ends, a copy of the clamped row or column)
  double b00 = 0, b01 = 0, b02 = 0, b03 = 0, b10 = 0, b11 = 0, b12 = 0, b13 = 0, b20 = 0, b21 = 0,
         b22 = 0, b23 = 0, b30 = 0, b31 = 0, b32 = 0, b33 = 0;
  for (uint64_t w = 0; alive; ++w) {
    // (x, y) is the path's waypoint w and (ni, nj), on the grid, its node
    uint32_t lab = 0xffffffffu;
    // the node is inside the grid; issued ahead of the block's loads, used after them
    if (GOALS && fresh) lab = a.label[(int64_t)nj * nx + ni];
    // the continuous candidate: computeNextGlobalWaypoint (:666-714), as k_extract_paths
    int64_t cx = 0, cy = 0;
    double nxt_x = __builtin_nan(""), nxt_y = nxt_x, dcx = 0, dcy = 0;
    const bool in_x = path_cell(gx, a.nx, cx), in_y = path_cell(gy, a.ny, cy);
    if (in_x && in_y) {
      if (!cell.holds(cx, cy)) {
        // the whole 4x4 block, loaded together.  The gradients take it without its
        // corners (k_extract_paths' 12 values); the corners serve the nodes.
        const Stencil s = stencil_of(a.T, ld, nx, ny, cx, cy);
        b00 = s.r0[s.i0], b01 = s.r0[cx], b02 = s.r0[cx + 1], b03 = s.r0[s.i3];
        b10 = s.r1[s.i0], b11 = s.r1[cx], b12 = s.r1[cx + 1], b13 = s.r1[s.i3];
        b20 = s.r2[s.i0], b21 = s.r2[cx], b22 = s.r2[cx + 1], b23 = s.r2[s.i3];
        b30 = s.r3[s.i0], b31 = s.r3[cx], b32 = s.r3[cx + 1], b33 = s.r3[s.i3];
        cell.set(cx, cy, s.w_ok, s.e_ok, s.s_ok, s.n_ok, b01, b02, b10, b11, b12, b13, b20, b21,
                 b22, b23, b31, b32);
      }
      cell.candidate(x, y, gx, gy, cx, cy, a.res_tau, dcx, dcy, nxt_x, nxt_y);
    }
    if (fresh) {
      // the 3x3 block of the new node, before the grid's edge is applied
      double bmm, b0m, bpm, bm0, bz0, bp0, bmp, b0p, bpp;
      const uint32_t ox = ni - (uint32_t)cx, oy = nj - (uint32_t)cy;
      if (in_x && in_y && ox <= 1u && oy <= 1u) {
        // the node is a corner of the held cell (the rounding and the truncation of one
        // coordinate differ by 0 or 1): its 3x3 block lies inside the 4x4 one -- no load
        const bool sx = ox != 0u, sy = oy != 0u;
        const double u0m = sx ? b01 : b00, u00 = sx ? b02 : b01, u0p = sx ? b03 : b02;
        const double u1m = sx ? b11 : b10, u10 = sx ? b12 : b11, u1p = sx ? b13 : b12;
        const double u2m = sx ? b21 : b20, u20 = sx ? b22 : b21, u2p = sx ? b23 : b22;
        const double u3m = sx ? b31 : b30, u30 = sx ? b32 : b31, u3p = sx ? b33 : b32;
        bmm = sy ? u1m : u0m, b0m = sy ? u10 : u00, bpm = sy ? u1p : u0p;
        bm0 = sy ? u2m : u1m, bz0 = sy ? u20 : u10, bp0 = sy ? u2p : u1p;
        bmp = sy ? u3m : u2m, b0p = sy ? u30 : u20, bpp = sy ? u3p : u2p;
      } else {
        // a node that is in no cell (the last row or column): rows nj-1 .. nj+1, columns
        // ni-1 .. ni+1, clamped; 0 <= ni < nx and 0 <= nj < ny
        const int64_t i1 = ni, j1 = nj;
        const int64_t i0 = i1 > 0 ? i1 - 1 : 0, i2 = i1 + 1 < nx ? i1 + 1 : nx - 1;
        const int64_t j0 = j1 > 0 ? j1 - 1 : 0, j2 = j1 + 1 < ny ? j1 + 1 : ny - 1;
        const double* q0 = a.T + j0 * ld;
        const double* q1 = a.T + j1 * ld;
        const double* q2 = a.T + j2 * ld;
        bmm = q0[i0], b0m = q0[i1], bpm = q0[i2];
        bm0 = q1[i0], bz0 = q1[i1], bp0 = q1[i2];
        bmp = q2[i0], b0p = q2[i1], bpp = q2[i2];
      }
      // a neighbour off the grid is +inf: no test accepts it
      const bool hw = ni > 0, he = (int64_t)ni + 1 < nx, hs = nj > 0, hn = (int64_t)nj + 1 < ny;
      tmm = hw && hs ? bmm : kInfD, t0m = hs ? b0m : kInfD, tpm = he && hs ? bpm : kInfD;
      tm0 = hw ? bm0 : kInfD, t00 = bz0, tp0 = he ? bp0 : kInfD;
      tmp = hw && hn ? bmp : kInfD, t0p = hn ? b0p : kInfD, tpp = he && hn ? bpp : kInfD;
      fresh = false;
      if (GOALS && lab < a.n_goals && lab != lab_held) {
        const double sx = a.goal_xy[2 * (uint64_t)lab], sy = a.goal_xy[2 * (uint64_t)lab + 1];
        sni = snj = 0xffffffffu;  // a goal off the grid is no node's sink
        uint32_t gi = 0, gj = 0;
        if (arrive_node(sx, sx / a.res, a.nx, gi) && arrive_node(sy, sy / a.res, a.ny, gj)) {
          sni = gi;
          snj = gj;
        }
        sink_x = sx;
        sink_y = sy;
        lab_held = lab;
      }
      if (GOALS) sink_k = lab < a.n_goals ? (int32_t)lab : -1;
    }
    if (w == 0) {  // the start: on a finite node, and under a goal set on a labelled one
      if (!(t00 < kInfD) || (GOALS && sink_k < 0)) break;
      start_cost = t00;
      status = 0;
    }
    // waypoint w joins the record and, under the stride rule, the output
    if (w > 0) length = length + dist2d(px, py, x, y);
    ++count;
    if (phase == 0) {  // kept < max_wp: w < max_wp * stride
      if (SIMPLIFY) {
        if (w == 0) {
          sim.anchor(x, y);
          keep(x, y, pdx, pdy, 0u);
        } else if (sim.next(px, py, x, y, a.eps, a.eps2)) {
          keep(px, py, qdx, qdy, (uint32_t)w - 1u);
        }
        qdx = pdx;
        qdy = pdy;
      } else if (STORE) {
        double* o = out + 4 * (uint64_t)kept;
        o[0] = x;
        o[1] = y;
        o[2] = pdx;
        o[3] = pdy;
      }
      ++kept;
    }
    if (++phase == a.stride) phase = 0;
    px = x;
    py = y;
    // 1. arrived: the node is the sink's
    if (ni == sni && nj == snj && (!GOALS || sink_k >= 0)) {
      status = 1;
      break;
    }
    if (w + 1 == limit) {
      status = -3;
      break;
    }
    // 2. the continuous candidate and its node m
    uint32_t mi = 0, mj = 0;
    const double gnx = nxt_x / a.res, gny = nxt_y / a.res;
    bool take = dist2d(x, y, nxt_x, nxt_y) >= a.stall;  // false for a NaN candidate
    take = take && arrive_node(nxt_x, gnx, a.nx, mi) && arrive_node(nxt_y, gny, a.ny, mj);
    int di = 0, dj = 0;
    if (take) {
      const int64_t ddi = (int64_t)mi - (int64_t)ni, ddj = (int64_t)mj - (int64_t)nj;
      take = ddi >= -1 && ddi <= 1 && ddj >= -1 && ddj <= 1;
      di = (int)ddi;
      dj = (int)ddj;
    }
    if (take) {
      const double tm = pick3(dj, pick3(di, tmm, t0m, tpm), pick3(di, tm0, t00, tp0),
                              pick3(di, tmp, t0p, tpp));
      take = tm < kInfD;
      if (di == 0 && dj == 0) take = take && same < 8u;
      else take = take && tm < t00;
      if (di != 0 && dj != 0)  // no corner is cut: both side nodes are finite
        take = take && pick3(di, tm0, t00, tp0) < kInfD && pick3(dj, t0m, t00, t0p) < kInfD;
    }
    if (take) {
      x = nxt_x;
      y = nxt_y;
      gx = gnx;
      gy = gny;
      pdx = dcx;
      pdy = dcy;
      if (di == 0 && dj == 0) {
        ++same;
      } else {
        same = 0;
        ni = mi;
        nj = mj;
        fresh = true;
      }
    } else {
      // 3. a hop to the neighbour of the steepest fall of T
      double best = -1.0;
      int bi = 0, bj = 0;
      hop_try(true, t00, t0m, false, 0, -1, best, bi, bj);
      hop_try(true, t00, tm0, false, -1, 0, best, bi, bj);
      hop_try(true, t00, tp0, false, 1, 0, best, bi, bj);
      hop_try(true, t00, t0p, false, 0, 1, best, bi, bj);
      hop_try(tm0 < kInfD && t0m < kInfD, t00, tmm, true, -1, -1, best, bi, bj);
      hop_try(tp0 < kInfD && t0m < kInfD, t00, tpm, true, 1, -1, best, bi, bj);
      hop_try(tm0 < kInfD && t0p < kInfD, t00, tmp, true, -1, 1, best, bi, bj);
      hop_try(tp0 < kInfD && t0p < kInfD, t00, tpp, true, 1, 1, best, bi, bj);
      if (bi == 0 && bj == 0) break;  // stalled: status 0
      // the neighbour's value is not the +inf of a node off the grid: it is on the grid
      ni = (uint32_t)((int64_t)ni + bi);
      nj = (uint32_t)((int64_t)nj + bj);
      x = a.res * (double)ni;
      y = a.res * (double)nj;
      gx = x / a.res;
      gy = y / a.res;
      pdx = (double)-bi;
      pdy = (double)-bj;
      same = 0;
      ++hops;
      fresh = true;
    }
  }
  // the last waypoint walked is kept; it is the anchor only where it is waypoint 0
  if (SIMPLIFY && count >= 2u) keep(px, py, qdx, qdy, count - 1u);
  if (status == 1) {
    if (kept < a.max_wp) {
      length = length + dist2d(px, py, sink_x, sink_y);
      ++count;
      if (SIMPLIFY) {
        keep(sink_x, sink_y, 0, 0, count - 1u);
      } else if (STORE) {
        double* o = out + 4 * (uint64_t)kept;
        o[0] = sink_x;
        o[1] = sink_y;
        o[2] = 0;
        o[3] = 0;
      }
      ++kept;
    } else {
      status = -3;
    }
  }
  if (a.count) a.count[p] = (int32_t)(SIMPLIFY ? skept : kept);
  ArriveRec* o = a.stats + p;
  o->status = status;
  o->sink = status == 1 ? sink_k : -1;
  o->count = count;
  o->hops = hops;
  o->length = length;
  o->start_cost = start_cost;
}

}  // namespace

hipError_t launch_arrive_paths(const ArriveArgs& a, hipStream_t st) {
  if (a.n_paths == 0) return hipSuccess;
  const dim3 grid((a.n_paths + 63u) / 64u), block(64);
  if (a.label) {
    if (a.out) hipLaunchKernelGGL((k_arrive_paths<true, true, false>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((k_arrive_paths<true, false, false>), grid, block, 0, st, a);
  } else {
    if (a.out) hipLaunchKernelGGL((k_arrive_paths<false, true, false>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((k_arrive_paths<false, false, false>), grid, block, 0, st, a);
  }
  return hipGetLastError();
}

// the simplified form: a.stride is 1, a.max_wp bounds the walk, a.out may be null
hipError_t launch_arrive_simplified(const ArriveArgs& a, hipStream_t st) {
  if (a.n_paths == 0) return hipSuccess;
  const dim3 grid((a.n_paths + 63u) / 64u), block(64);
  if (a.label) {
    if (a.out) hipLaunchKernelGGL((k_arrive_paths<true, true, true>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((k_arrive_paths<true, false, true>), grid, block, 0, st, a);
  } else {
    if (a.out) hipLaunchKernelGGL((k_arrive_paths<false, true, true>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((k_arrive_paths<false, false, true>), grid, block, 0, st, a);
  }
  return hipGetLastError();
}

}  // namespace dymu
