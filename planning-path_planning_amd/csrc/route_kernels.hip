// route_kernels.hip -- every cell's node route to the goal at once
// (DyMuPathPlanner::getRouteFields, dymu_route_fields_device).
//
// The route of a cell is the hop of the arriving descent (arrive_kernels.hip, step 3)
// applied at every node: a function of T alone that gives every finite non-root cell at
// most one parent, so the map is a forest rooted at the goals.  What a cell's route adds up
// to -- hops between axis and diagonal neighbours, the integral, minimum and maximum of up
// to kPathFields fields, the root it ends on -- comes out of pointer doubling:
//
//   k_route_init   per cell its parent (or a terminal entry), the one hop's kind and the
//                  cell's own terms; k_route_roots then marks the roots as k_label_roots does
//   k_route_round  state r+1 of c = state r of c combined with state r of next[c], and
//                  next[c] <- next[next[c]].  Synchronous and double-buffered: a round reads
//                  state r only.  (The label map's in-place jump, goal_kernels.hip, is not
//                  usable here: a lane that read a neighbour's new aggregate with its old
//                  pointer, or the reverse, would count hops twice or skip them.)
//   k_route_final  the terminal entry into sink / NONE, the sink's own sample into the
//                  minimum and maximum, the length, the outputs at the caller's pitch
//
// An aggregate of c covers the nodes from c up to, not including, next[c]; a terminal entry
// (top bit set, as in the label map) holds the root's seed index or NONE, and a terminal
// cell holds the identity (0, 0, 0.0, +inf, -inf).  The state is SoA and an array the
// caller did not ask for is a null pointer that no kernel touches.  The loops over the
// fields are unrolled over kPathFields with uniform tests of the kernel arguments: no array
// is indexed at run time, no scratch.
#include "fim_kernels.h"

namespace dymu {
namespace {

constexpr uint32_t kTag = 0x80000000u;   // next entry: terminal (low 31 bits: the seed index)
constexpr uint32_t kNone = 0xFFFFFFFFu;  // terminal, no route (DYMU_LABEL_NONE)
constexpr double kInfD = __builtin_huge_val();
constexpr double kDiag = 0.7071067811865476;   // a diagonal hop's score per unit of T
constexpr double kSqrt2 = 1.4142135623730951;  // a diagonal hop's length per res

__device__ __forceinline__ unsigned long long dbits(double v) {
  return (unsigned long long)__double_as_longlong(v);
}
// minimum and maximum with -0.0 below +0.0, so that the order of the folds does not show
__device__ __forceinline__ double rmin(double a, double b) {
  return (b < a || (b == a && __builtin_signbit(b))) ? b : a;
}
__device__ __forceinline__ double rmax(double a, double b) {
  return (b > a || (b == a && !__builtin_signbit(b))) ? b : a;
}
__device__ __forceinline__ bool finite(double v) { return v > -kInfD && v < kInfD; }

// arrive_kernels.hip's hop_try: the largest score wins, the first in the order among equals
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

__global__ __launch_bounds__(256) void k_route_init(RouteInitArgs a) {
  const uint32_t n = a.nx * a.ny;  // < 2^31 (checked on the host)
  const uint32_t c = blockIdx.x * 256u + threadIdx.x;
  if (c >= n) return;
  const uint32_t j = c / a.nx, i = c - j * a.nx;
  // rows j-1 .. j+1, columns i-1 .. i+1, clamped for the load; a value from outside the
  // grid is replaced by +inf, which no test accepts
  const int64_t nx = a.nx, ny = a.ny, i1 = i, j1 = j;
  const int64_t i0 = i1 > 0 ? i1 - 1 : 0, i2 = i1 + 1 < nx ? i1 + 1 : nx - 1;
  const int64_t j0 = j1 > 0 ? j1 - 1 : 0, j2 = j1 + 1 < ny ? j1 + 1 : ny - 1;
  const double* q0 = a.T + j0 * a.ld;
  const double* q1 = a.T + j1 * a.ld;
  const double* q2 = a.T + j2 * a.ld;
  const double bmm = q0[i0], b0m = q0[i1], bpm = q0[i2];
  const double bm0 = q1[i0], t00 = q1[i1], bp0 = q1[i2];
  const double bmp = q2[i0], b0p = q2[i1], bpp = q2[i2];
  const bool hw = i1 > 0, he = i1 + 1 < nx, hs = j1 > 0, hn = j1 + 1 < ny;
  const double tmm = hw && hs ? bmm : kInfD, t0m = hs ? b0m : kInfD, tpm = he && hs ? bpm : kInfD;
  const double tm0 = hw ? bm0 : kInfD, tp0 = he ? bp0 : kInfD;
  const double tmp = hw && hn ? bmp : kInfD, t0p = hn ? b0p : kInfD, tpp = he && hn ? bpp : kInfD;
  int bi = 0, bj = 0;
  if (t00 < kInfD) {
    double best = -1.0;
    hop_try(true, t00, t0m, false, 0, -1, best, bi, bj);
    hop_try(true, t00, tm0, false, -1, 0, best, bi, bj);
    hop_try(true, t00, tp0, false, 1, 0, best, bi, bj);
    hop_try(true, t00, t0p, false, 0, 1, best, bi, bj);
    hop_try(tm0 < kInfD && t0m < kInfD, t00, tmm, true, -1, -1, best, bi, bj);
    hop_try(tp0 < kInfD && t0m < kInfD, t00, tpm, true, 1, -1, best, bi, bj);
    hop_try(tm0 < kInfD && t0p < kInfD, t00, tmp, true, -1, 1, best, bi, bj);
    hop_try(tp0 < kInfD && t0p < kInfD, t00, tpp, true, 1, 1, best, bi, bj);
  }
  // a chosen neighbour's value is not the +inf of a node off the grid: it is on the grid.
  // No target: +inf, NaN or a dead end -- terminal, NONE, the identity in both buffers
  const bool term = bi == 0 && bj == 0;
  const bool diag = bi != 0 && bj != 0;
  const uint32_t nxt = term ? kNone : (uint32_t)((int64_t)c + (int64_t)bj * nx + bi);
  // buffer 1 gets the entry too: a round tells a finished cell that is already in both
  // buffers by its own entry in the buffer it writes
  a.s0.next[c] = nxt;
  a.s1.next[c] = nxt;
  if (a.s0.axis) {
    a.s0.axis[c] = term || diag ? 0u : 1u;
    if (term) a.s1.axis[c] = 0u;
  }
  if (a.s0.diag) {
    a.s0.diag[c] = diag ? 1u : 0u;
    if (term) a.s1.diag[c] = 0u;
  }
  const double seg = diag ? a.res * kSqrt2 : a.res;
#pragma unroll
  for (int f = 0; f < kPathFields; ++f) {
    if (!a.field[f]) continue;  // uniform
    const double v = a.field[f][j1 * a.field_ld[f] + i1];
    const bool cnt = !term && finite(v);
    if (a.s0.integ[f]) {
      a.s0.integ[f][c] = cnt ? v * seg : 0.0;
      if (term) a.s1.integ[f][c] = 0.0;
    }
    if (a.s0.vmin[f]) {
      a.s0.vmin[f][c] = cnt ? v : kInfD;
      if (term) a.s1.vmin[f][c] = kInfD;
    }
    if (a.s0.vmax[f]) {
      a.s0.vmax[f][c] = cnt ? v : -kInfD;
      if (term) a.s1.vmax[f][c] = -kInfD;
    }
  }
}

__device__ __forceinline__ void put_identity(const RouteState& s, uint32_t c) {
  if (s.axis) s.axis[c] = 0u;
  if (s.diag) s.diag[c] = 0u;
#pragma unroll
  for (int f = 0; f < kPathFields; ++f) {
    if (s.integ[f]) s.integ[f][c] = 0.0;
    if (s.vmin[f]) s.vmin[f][c] = kInfD;
    if (s.vmax[f]) s.vmax[f][c] = -kInfD;
  }
}

// roots, after k_route_init: k_label_roots' rule (goal_kernels.hip) on both buffers.  step 0
// clears the cell's entry and its aggregates, step 1 min-writes tag | k -- with duplicates
// only the seeds of the smallest t0 can match T, and the lowest k among them wins.
__global__ void k_route_roots(RouteState s0, RouteState s1, const double* T, int64_t ld,
                              uint32_t nx, uint32_t ny, const GoalSeed* seeds, uint32_t n_seeds,
                              int step) {
  for (uint32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < n_seeds;
       s += gridDim.x * blockDim.x) {
    const GoalSeed sd = seeds[s];
    if (sd.i >= nx || sd.j >= ny) continue;
    if (dbits(T[(int64_t)sd.j * ld + sd.i]) != dbits(sd.t0)) continue;  // dominated
    const uint32_t c = sd.j * nx + sd.i;
    if (step == 0) {
      s0.next[c] = kNone;
      s1.next[c] = kNone;
      put_identity(s0, c);
      put_identity(s1, c);
    } else {
      atomicMin(s0.next + c, kTag | s);
      atomicMin(s1.next + c, kTag | s);
    }
  }
}

// One synchronous round, src -> dst.  A cell whose entry is terminal is finished: its
// values are final, and once they stand in both buffers (its own entry in dst is terminal
// too -- only this lane ever writes it) the cell costs one more 4-byte read and nothing
// else.  cnt[round] += the entries still open after this round (one ballot per wave and
// step, one atomic per workgroup); a round that finds the previous round's count at 0 has
// nothing to do.  The grid is capped and strided as k_label_jump's is, for its reason.
constexpr uint32_t kRoundBlocks = 8192;
__global__ __launch_bounds__(256) void k_route_round(RouteState src, RouteState dst, uint32_t n,
                                                     uint32_t* cnt, uint32_t round) {
  if (round > 0 && cnt[round - 1] == 0u) return;  // uniform
  __shared__ uint32_t s_open;
  if (threadIdx.x == 0) s_open = 0u;
  __syncthreads();
  uint32_t wave_open = 0;  // wave-uniform
  // n < 2^31 and the stride is at most 2^21: base never wraps
  for (uint32_t base = blockIdx.x * 256u; base < n; base += gridDim.x * 256u) {
    const uint32_t c = base + threadIdx.x;
    bool open = false;
    if (c < n) {
      const uint32_t v = src.next[c];
      if (v & kTag) {
        if (!(dst.next[c] & kTag)) {  // finished in the round before: the one copy
          if (src.axis) dst.axis[c] = src.axis[c];
          if (src.diag) dst.diag[c] = src.diag[c];
#pragma unroll
          for (int f = 0; f < kPathFields; ++f) {
            if (src.integ[f]) dst.integ[f][c] = src.integ[f][c];
            if (src.vmin[f]) dst.vmin[f][c] = src.vmin[f][c];
            if (src.vmax[f]) dst.vmax[f][c] = src.vmax[f][c];
          }
          dst.next[c] = v;
        }
      } else if (v < n) {  // a cell index written by k_route_init or an earlier round
        const uint32_t w = src.next[v];
        if (src.axis) dst.axis[c] = src.axis[c] + src.axis[v];
        if (src.diag) dst.diag[c] = src.diag[c] + src.diag[v];
#pragma unroll
        for (int f = 0; f < kPathFields; ++f) {
          if (src.integ[f]) dst.integ[f][c] = src.integ[f][c] + src.integ[f][v];
          if (src.vmin[f]) dst.vmin[f][c] = rmin(src.vmin[f][c], src.vmin[f][v]);
          if (src.vmax[f]) dst.vmax[f][c] = rmax(src.vmax[f][c], src.vmax[f][v]);
        }
        dst.next[c] = w;
        open = !(w & kTag);
      } else {
        dst.next[c] = kNone;  // no kernel writes such an entry
      }
    }
    wave_open += (uint32_t)__popcll(__ballot(open));
  }
  if ((threadIdx.x & 63u) == 0u && wave_open) atomicAdd(&s_open, wave_open);
  __syncthreads();
  if (threadIdx.x == 0 && s_open) atomicAdd(&cnt[round], s_open);
}

__global__ __launch_bounds__(256) void k_route_final(RouteFinalArgs a) {
  const uint32_t n = a.nx * a.ny;
  const uint32_t c = blockIdx.x * 256u + threadIdx.x;
  if (c >= n) return;
  const uint32_t j = c / a.nx, i = c - j * a.nx;
  const uint32_t v = a.s.next[c];
  // an entry still open (the round cap was hit) has no route
  uint32_t k = (v & kTag) && v != kNone ? (v & ~kTag) : kNone;
  if (k >= a.n_seeds) k = kNone;
  const bool has = k != kNone;
  const int64_t o = (int64_t)j * a.o_ld + i;
  if (a.o_sink) a.o_sink[o] = k;
  const uint32_t ax = has && a.s.axis ? a.s.axis[c] : 0u;
  const uint32_t dg = has && a.s.diag ? a.s.diag[c] : 0u;
  if (a.o_axis) a.o_axis[o] = ax;
  if (a.o_diag) a.o_diag[o] = dg;
  if (a.o_length)
    a.o_length[o] = has ? a.res * (double)ax + (a.res * kSqrt2) * (double)dg : __builtin_nan("");
  uint32_t si = 0, sj = 0;  // the sink's node
  if (has) {
    const GoalSeed sd = a.seeds[k];
    si = sd.i;
    sj = sd.j;
  }
#pragma unroll
  for (int f = 0; f < kPathFields; ++f) {
    if (a.o_integ[f]) a.o_integ[f][o] = has ? a.s.integ[f][c] : __builtin_nan("");
    if (!a.o_vmin[f] && !a.o_vmax[f]) continue;  // uniform
    double lo = kInfD, hi = -kInfD;
    if (has) {
      const double vt = a.field[f][(int64_t)sj * a.field_ld[f] + si];
      if (finite(vt)) lo = hi = vt;
      if (a.s.vmin[f]) lo = rmin(a.s.vmin[f][c], lo);
      if (a.s.vmax[f]) hi = rmax(a.s.vmax[f][c], hi);
    }
    if (a.o_vmin[f]) a.o_vmin[f][o] = lo;
    if (a.o_vmax[f]) a.o_vmax[f][o] = hi;
  }
}

uint32_t seed_blocks(uint32_t n) { return n < 256u * 1024u ? (n + 255u) / 256u : 1024u; }

}  // namespace

hipError_t launch_route_init(const RouteInitArgs& a, const GoalSeed* seeds, uint32_t n_seeds,
                             hipStream_t st) {
  const uint32_t n = a.nx * a.ny;
  hipLaunchKernelGGL(k_route_init, dim3((n + 255u) / 256u), dim3(256), 0, st, a);
  for (int step = 0; step < 2; ++step)
    hipLaunchKernelGGL(k_route_roots, dim3(seed_blocks(n_seeds)), dim3(256), 0, st, a.s0, a.s1, a.T,
                       a.ld, a.nx, a.ny, seeds, n_seeds, step);
  return hipGetLastError();
}

hipError_t launch_route_round(const RouteState& src, const RouteState& dst, uint32_t n,
                              uint32_t* cnt, uint32_t round, hipStream_t st) {
  const uint32_t blocks = (n + 255u) / 256u;
  hipLaunchKernelGGL(k_route_round, dim3(blocks < kRoundBlocks ? blocks : kRoundBlocks), dim3(256),
                     0, st, src, dst, n, cnt, round);
  return hipGetLastError();
}

hipError_t launch_route_final(const RouteFinalArgs& a, hipStream_t st) {
  const uint32_t n = a.nx * a.ny;
  hipLaunchKernelGGL(k_route_final, dim3((n + 255u) / 256u), dim3(256), 0, st, a);
  return hipGetLastError();
}

}  // namespace dymu
