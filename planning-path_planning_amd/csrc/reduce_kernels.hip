// reduce_kernels.hip -- a cell in all planes at once:
//   k_batch_reduce  one left-to-right fp64 fold per cell over a list of planes of a batch
//                   stack (sum / max / min, optional weights and offsets), the combined
//                   map, the arg map and per-workgroup partials of the summary
//   k_reduce_final  the partials folded into the summary record (one workgroup)
//   k_level_mask    the sub-level set of a map as a byte mask, its box and its count
//
// Streaming kernels: 256-thread workgroups walk tiles of 256 work items with a grid-stride
// loop.  A work item is two adjacent cells of one row that share a 16-byte segment of the
// INPUT (one dwordx4 load per plane); a row that starts 8 bytes off a 16-byte boundary (an
// odd pitch, an odd base) has a one-cell head item, and an odd remainder a one-cell tail,
// both read with 8-byte loads.  The plane pitch P * ld is even (P is a multiple of 16), so
// one parity holds for a cell in every plane.  Outputs are stored 16 (8 for the arg map)
// bytes at a time where the pair's address allows, else cell by cell.  Rows narrower than
// 256 items share a tile (a power-of-two number of lanes per row).
#include "fim_kernels.h"

namespace dymu {
namespace {

constexpr double kInfD = __builtin_huge_val();
constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint64_t kNoCell = ~0ull;

// the tile walk both kernels share: tile t, thread tid -> row j and the item's first cell
// i0 (-1: the head item's missing cell), false when the item holds no cell
__device__ __forceinline__ bool tile_item(const TileWalk& w, const double* base, uint64_t ld,
                                          uint32_t nx, uint32_t ny, uint64_t t, uint32_t tid,
                                          uint32_t& j, int64_t& i0) {
  uint64_t jg = t;
  uint32_t c = 0;
  if (w.chunks != 1) {  // then a row has 256 lanes and a tile one row
    jg = t / w.chunks;
    c = (uint32_t)(t - jg * w.chunks);
  }
  const uint64_t row = (jg << (8 - w.lanes_log2)) + (tid >> w.lanes_log2);
  const uint64_t k = (uint64_t)c * 256u + (tid & ((1u << w.lanes_log2) - 1u));
  if (row >= ny) return false;
  j = (uint32_t)row;
  const uint64_t head = ((reinterpret_cast<uintptr_t>(base) >> 3) + row * ld) & 1u;
  i0 = (int64_t)(2 * k) - (int64_t)head;
  return i0 + 1 >= 0 && i0 < (int64_t)nx;  // k = 0 with a head: cell 0 alone
}

__device__ __forceinline__ uint64_t shfl_down64(uint64_t v, int d) {
  const uint32_t lo = (uint32_t)__shfl_down((int)(uint32_t)v, d, 64);
  const uint32_t hi = (uint32_t)__shfl_down((int)(uint32_t)(v >> 32), d, 64);
  return ((uint64_t)hi << 32) | lo;
}

// the summary's order: the smaller value, among equals the lower row-major index
struct Best {
  double v;
  uint64_t cell;
  uint64_t n;
  uint32_t arg;
};
__device__ __forceinline__ void best_take(Best& b, double v, uint64_t cell, uint32_t arg) {
  if (v < b.v || (v == b.v && cell < b.cell)) b.v = v, b.cell = cell, b.arg = arg;
}
__device__ __forceinline__ void best_merge(Best& b, const Best& o) {
  if (o.cell != kNoCell) best_take(b, o.v, o.cell, o.arg);
  b.n += o.n;
}
__device__ __forceinline__ Best best_shfl(const Best& b, int d) {
  Best o;
  o.v = __longlong_as_double((long long)shfl_down64((uint64_t)__double_as_longlong(b.v), d));
  o.cell = shfl_down64(b.cell, d);
  o.n = shfl_down64(b.n, d);
  o.arg = (uint32_t)__shfl_down((int)b.arg, d, 64);
  return o;
}
// wave shuffles, then LDS, then thread 0 holds the workgroup's record
__device__ __forceinline__ void best_block(Best& b, Best* lds) {
  for (int d = 32; d > 0; d >>= 1) {
    const Best o = best_shfl(b, d);
    best_merge(b, o);
  }
  const uint32_t wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63u) == 0) lds[wave] = b;
  __syncthreads();
  if (threadIdx.x == 0)
    for (uint32_t q = 1; q < 4; ++q) best_merge(b, lds[q]);
}

template <int FL>
__device__ __forceinline__ double term_of(double t, const ReduceTerm& e) {
  if (FL & 1) t = e.w * t;
  if (FL & 2) t = t + e.o;
  return t;
}

template <int N>
__device__ __forceinline__ void load_cells(const double* p, double (&v)[N]) {
  if constexpr (N == 2) {
    const double2 d = *reinterpret_cast<const double2*>(p);
    v[0] = d.x, v[1] = d.y;
  } else {
    v[0] = *p;
  }
}

template <int OP, int FL, int N>
__device__ __forceinline__ void fold_step(const ReduceTerm& e, const double (&v)[N],
                                          double (&acc)[N], uint32_t (&arg)[N]) {
#pragma unroll
  for (int q = 0; q < N; ++q) {
    const double t = term_of<FL>(v[q], e);
    if (OP == 0) {
      acc[q] = acc[q] + t;
    } else if (OP == 1 ? t > acc[q] : t < acc[q]) {
      acc[q] = t, arg[q] = e.plane;
    }
  }
}

// N cells at p (their place in plane 0) through the whole list: the loads of four planes
// are issued before the fold consumes them, the fold keeps the list's order
template <int OP, int FL, int N>
__device__ __forceinline__ void fold_cells(const double* p, const ReduceTerm* __restrict__ tm,
                                           uint32_t n, double (&acc)[N], uint32_t (&arg)[N]) {
  double v0[N], v1[N], v2[N], v3[N];
  load_cells<N>(p + tm[0].off, v0);
#pragma unroll
  for (int q = 0; q < N; ++q) acc[q] = term_of<FL>(v0[q], tm[0]), arg[q] = tm[0].plane;
  uint32_t k = 1;
  for (; k + 4 <= n; k += 4) {
    load_cells<N>(p + tm[k].off, v0);
    load_cells<N>(p + tm[k + 1].off, v1);
    load_cells<N>(p + tm[k + 2].off, v2);
    load_cells<N>(p + tm[k + 3].off, v3);
    fold_step<OP, FL, N>(tm[k], v0, acc, arg);
    fold_step<OP, FL, N>(tm[k + 1], v1, acc, arg);
    fold_step<OP, FL, N>(tm[k + 2], v2, acc, arg);
    fold_step<OP, FL, N>(tm[k + 3], v3, acc, arg);
  }
  for (; k < n; ++k) {
    load_cells<N>(p + tm[k].off, v0);
    fold_step<OP, FL, N>(tm[k], v0, acc, arg);
  }
  if (OP == 2) {
#pragma unroll
    for (int q = 0; q < N; ++q)
      if (acc[q] == kInfD) arg[q] = kNone;  // no plane reaches the cell
  }
}

template <int OP, int FL>
__global__ __launch_bounds__(256) void k_batch_reduce(ReduceArgs a,
                                                      const ReduceTerm* __restrict__ terms,
                                                      double* __restrict__ out,
                                                      uint32_t* __restrict__ argmap,
                                                      ReducePartial* __restrict__ part) {
  // the list is read with scalar loads: the pointers are restrict kernel arguments, so no
  // store of the kernel can be taken to clobber it
  __shared__ Best lds[4];
  Best best{kInfD, kNoCell, 0ull, kNone};
  for (uint64_t t = blockIdx.x; t < a.walk.ntiles; t += gridDim.x) {
    uint32_t j;
    int64_t i0;
    if (!tile_item(a.walk, a.T, a.ld, a.nx, a.ny, t, threadIdx.x, j, i0)) continue;
    double acc[2];
    uint32_t arg[2];
    const bool pair = i0 >= 0 && i0 + 1 < (int64_t)a.nx;
    const uint32_t i = i0 < 0 ? 0u : (uint32_t)i0;  // the first (or only) cell
    const double* p = a.T + (uint64_t)j * a.ld + i;
    double* po = out + (uint64_t)j * a.out_ld + i;
    uint32_t* pa = argmap ? argmap + (uint64_t)j * a.arg_ld + i : nullptr;
    if (pair) {
      fold_cells<OP, FL, 2>(p, terms, a.n, acc, arg);
      if ((reinterpret_cast<uintptr_t>(po) & 15u) == 0) {
        *reinterpret_cast<double2*>(po) = make_double2(acc[0], acc[1]);
      } else {
        po[0] = acc[0], po[1] = acc[1];
      }
      if (OP != 0 && pa) {
        if ((reinterpret_cast<uintptr_t>(pa) & 7u) == 0) {
          *reinterpret_cast<uint2*>(pa) = make_uint2(arg[0], arg[1]);
        } else {
          pa[0] = arg[0], pa[1] = arg[1];
        }
      }
    } else {
      double a1[1];
      uint32_t g1[1];
      fold_cells<OP, FL, 1>(p, terms, a.n, a1, g1);
      acc[0] = a1[0], arg[0] = g1[0];
      po[0] = acc[0];
      if (OP != 0 && pa) pa[0] = arg[0];
    }
    if (part) {
      const uint64_t cell = (uint64_t)j * a.nx + i;
      if (acc[0] < kInfD) best_take(best, acc[0], cell, arg[0]), ++best.n;
      if (pair && acc[1] < kInfD) best_take(best, acc[1], cell + 1, arg[1]), ++best.n;
    }
  }
  if (part) {
    best_block(best, lds);
    if (threadIdx.x == 0)
      part[blockIdx.x] = ReducePartial{best.v, best.cell, best.n, best.arg, 0u};
  }
}

__global__ __launch_bounds__(256) void k_reduce_final(const ReducePartial* part, uint32_t n,
                                                      ReducePartial* out) {
  __shared__ Best lds[4];
  Best best{kInfD, kNoCell, 0ull, kNone};
  for (uint32_t k = threadIdx.x; k < n; k += 256u)
    best_merge(best, Best{part[k].v, part[k].cell, part[k].n, part[k].arg});
  best_block(best, lds);
  if (threadIdx.x == 0) *out = ReducePartial{best.v, best.cell, best.n, best.arg, 0u};
}

// box words: min i, min j (start at ~0), max i, max j (start at 0); cnt: the marked cells.
// Integer min / max / add: the result does not depend on the order the atomics arrive in.
__global__ __launch_bounds__(256) void k_level_mask(const double* map, uint64_t ld, uint32_t nx,
                                                    uint32_t ny, double bound, uint8_t* mask,
                                                    uint64_t mask_ld, TileWalk walk,
                                                    uint32_t* box, unsigned long long* cnt) {
  __shared__ uint32_t s_box[4];
  __shared__ unsigned long long s_cnt;
  if (threadIdx.x == 0) s_box[0] = s_box[1] = kNone, s_box[2] = s_box[3] = 0u, s_cnt = 0ull;
  __syncthreads();
  uint32_t li0 = kNone, lj0 = kNone, li1 = 0u, lj1 = 0u, n = 0u;
  for (uint64_t t = blockIdx.x; t < walk.ntiles; t += gridDim.x) {
    uint32_t j;
    int64_t i0;
    if (!tile_item(walk, map, ld, nx, ny, t, threadIdx.x, j, i0)) continue;
    const bool pair = i0 >= 0 && i0 + 1 < (int64_t)nx;
    const uint32_t i = i0 < 0 ? 0u : (uint32_t)i0;
    const double* p = map + (uint64_t)j * ld + i;
    uint8_t* pm = mask + (uint64_t)j * mask_ld + i;
    double v[2] = {kInfD, kInfD};
    if (pair) {
      load_cells<2>(p, v);
    } else {
      v[0] = *p;
    }
    const uint32_t m0 = v[0] <= bound ? 1u : 0u, m1 = pair && v[1] <= bound ? 1u : 0u;
    if (pair && (reinterpret_cast<uintptr_t>(pm) & 1u) == 0) {
      *reinterpret_cast<uint16_t*>(pm) = (uint16_t)(m0 | (m1 << 8));
    } else {
      pm[0] = (uint8_t)m0;
      if (pair) pm[1] = (uint8_t)m1;
    }
    if (m0 | m1) {
      const uint32_t lo = m0 ? i : i + 1, hi = m1 ? i + 1 : i;
      li0 = min(li0, lo), li1 = max(li1, hi), lj0 = min(lj0, j), lj1 = max(lj1, j);
      n += m0 + m1;
    }
  }
  if (box) {
    if (n) {
      atomicMin(&s_box[0], li0), atomicMin(&s_box[1], lj0);
      atomicMax(&s_box[2], li1), atomicMax(&s_box[3], lj1);
      atomicAdd(&s_cnt, (unsigned long long)n);
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_cnt) {
      atomicMin(&box[0], s_box[0]), atomicMin(&box[1], s_box[1]);
      atomicMax(&box[2], s_box[2]), atomicMax(&box[3], s_box[3]);
      atomicAdd(cnt, s_cnt);
    }
  }
}

template <int OP>
hipError_t launch_reduce_op(const ReduceArgs& a, uint32_t blocks, hipStream_t st) {
  switch (a.flags & 3u) {
    case 0: hipLaunchKernelGGL((k_batch_reduce<OP, 0>), dim3(blocks), dim3(256), 0, st, a, a.terms, a.out, a.arg, a.part); break;
    case 1: hipLaunchKernelGGL((k_batch_reduce<OP, 1>), dim3(blocks), dim3(256), 0, st, a, a.terms, a.out, a.arg, a.part); break;
    case 2: hipLaunchKernelGGL((k_batch_reduce<OP, 2>), dim3(blocks), dim3(256), 0, st, a, a.terms, a.out, a.arg, a.part); break;
    default: hipLaunchKernelGGL((k_batch_reduce<OP, 3>), dim3(blocks), dim3(256), 0, st, a, a.terms, a.out, a.arg, a.part); break;
  }
  return hipGetLastError();
}

}  // namespace

TileWalk tile_walk(const void* base, uint64_t ld, uint32_t nx, uint32_t ny) {
  // a row may have a head item when its first cell can sit 8 bytes off a 16-byte boundary
  const uint64_t head = ((reinterpret_cast<uintptr_t>(base) >> 3) | ld) & 1u;
  const uint64_t items = ((uint64_t)nx + head + 1) / 2;  // per row, at most
  TileWalk w{};
  w.lanes_log2 = 8;
  w.chunks = 1;
  if (items >= 256) {
    w.chunks = (uint32_t)((items + 255) / 256);
  } else {
    w.lanes_log2 = 0;
    while ((1u << w.lanes_log2) < items) ++w.lanes_log2;
  }
  const uint64_t rows_per_tile = 256u >> w.lanes_log2;
  w.ntiles = (((uint64_t)ny + rows_per_tile - 1) / rows_per_tile) * w.chunks;
  return w;
}

hipError_t launch_batch_reduce(const ReduceArgs& a, int op, uint32_t blocks, ReducePartial* d_sum,
                               hipStream_t st) {
  hipError_t e = op == 0   ? launch_reduce_op<0>(a, blocks, st)
                 : op == 1 ? launch_reduce_op<1>(a, blocks, st)
                           : launch_reduce_op<2>(a, blocks, st);
  if (e != hipSuccess || !a.part) return e;
  hipLaunchKernelGGL(k_reduce_final, dim3(1), dim3(256), 0, st, a.part, blocks, d_sum);
  return hipGetLastError();
}

hipError_t launch_level_mask(const double* map, uint64_t ld, uint32_t nx, uint32_t ny, double bound,
                             uint8_t* mask, uint64_t mask_ld, const TileWalk& walk, uint32_t blocks,
                             uint32_t* box, unsigned long long* cnt, hipStream_t st) {
  hipLaunchKernelGGL(k_level_mask, dim3(blocks), dim3(256), 0, st, map, ld, nx, ny, bound, mask,
                     mask_ld, walk, box, cnt);
  return hipGetLastError();
}

}  // namespace dymu
