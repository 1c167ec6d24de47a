// usage_kernels.hip -- how much of the map drains through every cell
// (DyMuPathPlanner::getRouteUsage, dymu_route_usage_device).
//
// route_kernels.hip makes the solved map a forest: every cell with a route has one route
// parent, the roots are the goals.  This file answers the upstream question on the same
// forest -- per cell the weight of all cells whose route passes through it (usage) and the
// largest total cost among them (far) -- by the reverse of that file's pointer doubling:
//
//   launch_route_init  (route_kernels.hip, the entry arrays only) the parents and the roots
//   k_usage_init       A_0[c] = w(c), M_0[c] = T[c] for a cell with T < +inf, else (0, 0)
//   k_usage_copy       A_{r+1} <- A_r, the receiving buffer of round r
//   k_usage_round      an open entry v = next[c] is the 2^r-th ancestor of c: the lane adds
//                      A_r[c] into A_{r+1}[v], folds M[c] into M[v], next'[c] = next[v].
//                      The descendants of v at distance [2^r, 2^(r+1)) are the descendants
//                      at distance < 2^r of the cells whose 2^r-th ancestor is v, so every
//                      descendant is counted once.  A finished cell sends nothing and goes
//                      on receiving.
//   k_usage_gather0    round 0 without atomics: a cell adds the neighbours whose entry
//                      points at it.  Measured faster than k_usage_round's round 0 at
//                      16384^2 and used by default; the atomic form stays
//                      as the reference path (DYMU_USAGE_ROUND0=0)
//   k_usage_final      the mask by route, the outputs at the caller's pitch
//   k_usage_catch      per seed the usage of its root
//
// The sums are 64-bit integers and M holds bit patterns of doubles >= +0.0, which order
// like the values: both atomics are native (global_atomic_add_x2 / umax_x2), neither
// depends on the order of arrival, and two calls give the same bytes.  A round reads A_r
// and adds into A_{r+1}, never into the array it reads; the maximum is idempotent -- a value
// a lane reads early or late is the T of a descendant either way -- and is kept in place.
// Atomics go to the workspace only.
#include "fim_kernels.h"

namespace dymu {
namespace {

constexpr uint32_t kTag = 0x80000000u;   // next entry: terminal (low 31 bits: the seed index)
constexpr uint32_t kNone = 0xFFFFFFFFu;  // terminal, no route (DYMU_LABEL_NONE)
constexpr double kInfD = __builtin_huge_val();
constexpr uint32_t kRoundBlocks = 8192;  // k_route_round's cap, for its reason

typedef unsigned long long u64;

__global__ __launch_bounds__(256) void k_usage_init(const double* T, int64_t ld, uint32_t nx,
                                                    uint32_t ny, const uint32_t* W, int64_t w_ld,
                                                    u64* sum, u64* far) {
  const uint32_t n = nx * ny;  // < 2^31 (checked on the host)
  const uint32_t c = blockIdx.x * 256u + threadIdx.x;
  if (c >= n) return;
  const uint32_t j = c / nx, i = c - j * nx;
  const double t = T[(int64_t)j * ld + i];
  const bool live = t < kInfD;  // not +inf, not NaN
  if (sum) sum[c] = live ? (W ? (u64)W[(int64_t)j * w_ld + i] : 1ull) : 0ull;
  if (far) far[c] = live ? (u64)__double_as_longlong(t) : 0ull;
}

// dst <- src, n 8-byte words (both 256-byte aligned); nothing after the round that closed
// the last entry
__global__ __launch_bounds__(256) void k_usage_copy(const u64* src, u64* dst, uint32_t n,
                                                    const uint32_t* cnt, uint32_t round) {
  if (round > 0 && cnt[round - 1] == 0u) return;  // uniform
  const uint32_t pairs = n >> 1;
  const ulonglong2* s2 = reinterpret_cast<const ulonglong2*>(src);
  ulonglong2* d2 = reinterpret_cast<ulonglong2*>(dst);
  for (uint32_t p = blockIdx.x * 256u + threadIdx.x; p < pairs; p += gridDim.x * 256u)
    d2[p] = s2[p];
  if ((n & 1u) && blockIdx.x == 0 && threadIdx.x == 0) dst[n - 1u] = src[n - 1u];
}

// One round.  nsrc / ndst: the entries of state r and r + 1; asrc: A_r; adst: A_{r+1},
// which holds a copy of A_r when the round starts; far: M, in place.  cnt[round] += the
// entries still open after the round, cnt[kRouteRounds + round] += the entries that sent in
// it (one ballot per wave and step, one atomic per workgroup and counter).
__global__ __launch_bounds__(256) void k_usage_round(const uint32_t* nsrc, uint32_t* ndst,
                                                     const u64* asrc, u64* adst, u64* far,
                                                     uint32_t n, uint32_t* cnt, uint32_t round) {
  if (round > 0 && cnt[round - 1] == 0u) return;  // uniform
  __shared__ uint32_t s_cnt[2];
  if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0u;
  __syncthreads();
  uint32_t wave_open = 0, wave_sent = 0;  // wave-uniform
  // n < 2^31 and the stride is at most 2^21: base never wraps
  for (uint32_t base = blockIdx.x * 256u; base < n; base += gridDim.x * 256u) {
    const uint32_t c = base + threadIdx.x;
    bool open = false, sent = false;
    if (c < n) {
      const uint32_t v = nsrc[c];
      if (v & kTag) {
        if (!(ndst[c] & kTag)) ndst[c] = v;  // finished in the round before
      } else if (v < n) {  // a cell index written by k_route_init or an earlier round
        const uint32_t w = nsrc[v];
        if (asrc) atomicAdd(adst + v, asrc[c]);
        if (far) atomicMax(far + v, __hip_atomic_load(far + c, __ATOMIC_RELAXED,
                                                      __HIP_MEMORY_SCOPE_AGENT));
        ndst[c] = w;
        sent = true;
        open = !(w & kTag);
      } else {
        ndst[c] = kNone;  // no kernel writes such an entry
      }
    }
    wave_open += (uint32_t)__popcll(__ballot(open));
    wave_sent += (uint32_t)__popcll(__ballot(sent));
  }
  if ((threadIdx.x & 63u) == 0u) {
    if (wave_open) atomicAdd(&s_cnt[0], wave_open);
    if (wave_sent) atomicAdd(&s_cnt[1], wave_sent);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    if (s_cnt[0]) atomicAdd(&cnt[round], s_cnt[0]);
    if (s_cnt[1]) atomicAdd(&cnt[kRouteRounds + round], s_cnt[1]);
  }
}

// Round 0 without atomics: in state 0 an open entry is the cell's parent, one of its eight
// neighbours, so cell c receives from exactly the neighbours whose entry is c.  Coalesced
// 4-byte reads of three rows of entries; A_1 and M by plain stores.  M is written in place
// while neighbours read it: a lane that reads a neighbour's new value reads the T of one of
// that neighbour's descendants, which is its own descendant too.
__global__ __launch_bounds__(256) void k_usage_gather0(const uint32_t* nsrc, uint32_t* ndst,
                                                       const u64* asrc, u64* adst, u64* far,
                                                       uint32_t nx, uint32_t ny, uint32_t* cnt) {
  __shared__ uint32_t s_cnt[2];
  if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0u;
  __syncthreads();
  const uint32_t n = nx * ny;
  uint32_t wave_open = 0, wave_sent = 0;
  for (uint32_t base = blockIdx.x * 256u; base < n; base += gridDim.x * 256u) {
    const uint32_t c = base + threadIdx.x;
    bool open = false, sent = false;
    if (c < n) {
      const uint32_t j = c / nx, i = c - j * nx;
      u64 a = asrc ? asrc[c] : 0ull;
      u64 m = far ? far[c] : 0ull;
#pragma unroll
      for (int dj = -1; dj <= 1; ++dj) {
#pragma unroll
        for (int di = -1; di <= 1; ++di) {
          if (di == 0 && dj == 0) continue;
          const int64_t ii = (int64_t)i + di, jj = (int64_t)j + dj;
          if (ii < 0 || ii >= (int64_t)nx || jj < 0 || jj >= (int64_t)ny) continue;
          const uint32_t d = (uint32_t)(jj * (int64_t)nx + ii);
          if (nsrc[d] != c) continue;
          if (asrc) a += asrc[d];
          if (far) {
            const u64 md = __hip_atomic_load(far + d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            m = md > m ? md : m;
          }
        }
      }
      if (adst) adst[c] = a;
      if (far) __hip_atomic_store(far + c, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const uint32_t v = nsrc[c];
      if (v & kTag) {
        // ndst holds the entry already (launch_route_init writes both buffers)
      } else if (v < n) {
        const uint32_t w = nsrc[v];
        ndst[c] = w;
        sent = true;
        open = !(w & kTag);
      } else {
        ndst[c] = kNone;
      }
    }
    wave_open += (uint32_t)__popcll(__ballot(open));
    wave_sent += (uint32_t)__popcll(__ballot(sent));
  }
  if ((threadIdx.x & 63u) == 0u) {
    if (wave_open) atomicAdd(&s_cnt[0], wave_open);
    if (wave_sent) atomicAdd(&s_cnt[1], wave_sent);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    if (s_cnt[0]) atomicAdd(&cnt[0], s_cnt[0]);
    if (s_cnt[1]) atomicAdd(&cnt[kRouteRounds], s_cnt[1]);
  }
}

__global__ __launch_bounds__(256) void k_usage_final(UsageFinalArgs a) {
  const uint32_t n = a.nx * a.ny;
  const uint32_t c = blockIdx.x * 256u + threadIdx.x;
  if (c >= n) return;
  const uint32_t j = c / a.nx, i = c - j * a.nx;
  const uint32_t v = a.next[c];
  // an entry still open (the round cap was hit) has no route
  uint32_t k = (v & kTag) && v != kNone ? (v & ~kTag) : kNone;
  if (k >= a.n_seeds) k = kNone;
  const bool has = k != kNone;
  const int64_t o = (int64_t)j * a.o_ld + i;
  if (a.o_sink) a.o_sink[o] = k;
  if (a.o_usage) a.o_usage[o] = has ? a.sum[c] : 0ull;
  if (a.o_far) a.o_far[o] = has ? __longlong_as_double((long long)a.far[c]) : __builtin_nan("");
}

// catchment[k] = the sum at seed k's cell if k is that cell's root, else 0 (a dominated
// seed, or one that lost its cell to a lower k)
__global__ void k_usage_catch(const uint32_t* next, const u64* sum, uint32_t nx,
                              const GoalSeed* seeds, uint32_t n_seeds, u64* out) {
  for (uint32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < n_seeds;
       s += gridDim.x * blockDim.x) {
    const GoalSeed sd = seeds[s];  // in the grid (checked on the host)
    const uint32_t c = sd.j * nx + sd.i;
    out[s] = next[c] == (kTag | s) ? sum[c] : 0ull;
  }
}

uint32_t strided_blocks(uint32_t n) {
  const uint32_t blocks = (n + 255u) / 256u;
  return blocks < kRoundBlocks ? blocks : kRoundBlocks;
}

}  // namespace

hipError_t launch_usage_init(const double* T, int64_t ld, uint32_t nx, uint32_t ny,
                             const uint32_t* W, int64_t w_ld, unsigned long long* sum,
                             unsigned long long* far, hipStream_t st) {
  const uint32_t n = nx * ny;
  hipLaunchKernelGGL(k_usage_init, dim3((n + 255u) / 256u), dim3(256), 0, st, T, ld, nx, ny, W,
                     w_ld, sum, far);
  return hipGetLastError();
}

hipError_t launch_usage_round(const UsageRoundArgs& a, uint32_t* cnt, uint32_t round,
                              bool gather0, hipStream_t st) {
  const uint32_t n = a.nx * a.ny;
  if (gather0 && round == 0) {
    hipLaunchKernelGGL(k_usage_gather0, dim3(strided_blocks(n)), dim3(256), 0, st, a.nsrc, a.ndst,
                       a.asrc, a.adst, a.far, a.nx, a.ny, cnt);
    return hipGetLastError();
  }
  if (a.asrc)
    hipLaunchKernelGGL(k_usage_copy, dim3(strided_blocks((n + 1u) / 2u)), dim3(256), 0, st, a.asrc,
                       a.adst, n, cnt, round);
  hipLaunchKernelGGL(k_usage_round, dim3(strided_blocks(n)), dim3(256), 0, st, a.nsrc, a.ndst,
                     a.asrc, a.adst, a.far, n, cnt, round);
  return hipGetLastError();
}

hipError_t launch_usage_final(const UsageFinalArgs& a, const GoalSeed* seeds,
                              unsigned long long* catchment, hipStream_t st) {
  const uint32_t n = a.nx * a.ny;
  if (a.o_usage || a.o_far || a.o_sink)
    hipLaunchKernelGGL(k_usage_final, dim3((n + 255u) / 256u), dim3(256), 0, st, a);
  if (catchment) {
    const uint32_t b = a.n_seeds < 256u * 1024u ? (a.n_seeds + 255u) / 256u : 1024u;
    hipLaunchKernelGGL(k_usage_catch, dim3(b), dim3(256), 0, st, a.next, a.sum, a.nx, seeds,
                       a.n_seeds, catchment);
  }
  return hipGetLastError();
}

}  // namespace dymu
