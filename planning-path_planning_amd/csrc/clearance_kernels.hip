// clearance_kernels.hip -- the obstacle clearance field and the risk-inflated speed
// (DESIGN.md s5.11).
//
// The clearance field S is the multi-source solution on a constant speed c with every
// obstacle cell of the speed map F (+inf or NaN) seeded at 0: S = 1 where a cell lies one
// risk distance from the nearest obstacle (c = global_res / risk_distance), and the
// reference's risk is max(1 - S, 0) (src/DyMu_LocalPathRepairing.cpp:493-576, there on
// the local layer only).
//
// k_fill_const writes the constant work map.  k_seed_mask seeds a cold domain from F
// itself, a workgroup on one tile at a time: what k_seed_values and k_seed_tiles (goal_kernels.hip)
// do for a seed list on the host, for the millions of obstacle cells of a device-resident
// map.  Every seed value is 0, so every key is 0 and every queued tile lands in bin 0 of a
// histogram whose origin is 0: one launch, nothing depends on the order of arrival.  The
// pass kernels run unchanged behind it.
// k_inflate_speed folds the risk into the speed: out = F * (risk_ratio * R + 1).
// k_seed_mask_window and k_claimed_box serve the incremental update after obstacles were
// added inside a window: the new cells seeded into the old field, which is an upper bound
// of the new one, and the bounding box of the tiles the passes behind it claimed.
// k_cone_keys and k_cone_queue serve the edit that also frees obstacles (s5.11.2): behind
// the seeded raise (update_kernels.hip) they queue the boundary of what it invalidated.
#include "fim_kernels.h"

#include <algorithm>

namespace dymu {
namespace {

constexpr double kInfD = __builtin_huge_val();

// one lane per cell of a row strip, rows and column strips by grid stride (k_stack_speed)
__global__ __launch_bounds__(256) void k_fill_const(double* __restrict__ W, uint64_t ld,
                                                    uint32_t nx, uint32_t ny, double v) {
  for (uint64_t r = blockIdx.y; r < ny; r += gridDim.y) {
    double* d = W + r * ld;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < nx;
         i += (uint64_t)gridDim.x * 256u)
      d[i] = v;
  }
}

// A workgroup of tw * th lanes takes one tile at a time (tiles by grid stride), one lane per
// cell: S = 0 at the tile's obstacle cells.  A tile that has any enters list 0 with key 0
// and, for the priority kernels, so does the tile across each tile edge an obstacle cell
// lies on (fim_kernels.h SeedTiles: the cell across is updated from a value no visit
// changes).  Each tile is claimed once through tile_epoch, whichever workgroups reach it;
// lanes 0..4 make the up to five claims of a tile side by side.  The claimed tiles are
// collected in LDS and published with one atomic per workgroup and flush, like the pass
// kernels' enqueues: the kShards list counters share a cache line, and one atomic per
// tile on it -- a million at 16384^2 -- took 11.9 ms there.
constexpr uint32_t kMaskQueue = 1024;
__global__ __launch_bounds__(256) void k_seed_mask(const double* __restrict__ F, MaskSeedArgs a,
                                                   uint32_t ntiles) {
  __shared__ uint32_t s_q[kMaskQueue];
  __shared__ uint32_t s_n, s_base;
  __shared__ uint32_t s_edges[2];  // per tile, alternating: bit 0 W, 1 E, 2 N, 3 S -- an
                                   // obstacle on that edge with a tile across it
  const uint32_t shard = blockIdx.x % kShards;
  const uint32_t cj = threadIdx.x / a.tw, ci = threadIdx.x - cj * a.tw;
  unsigned long long cells = 0;  // lane 0: the obstacle cells of this workgroup's tiles
  if (threadIdx.x == 0) s_n = s_edges[0] = s_edges[1] = 0u;
  __syncthreads();
  // list 0 <- the collected tiles (all lanes, after a barrier behind the last claim)
  auto flush = [&]() {
    const uint32_t n = s_n;
    if (threadIdx.x == 0) {
      s_base = atomicAdd(&a.counts[shard], n);
      if (a.hist) atomicAdd(&a.hist[shard * kBins], n);  // key_bin(0, base = 0) = 0
    }
    __syncthreads();
    const uint32_t base = s_base;
    for (uint32_t k = threadIdx.x; k < n; k += blockDim.x)
      a.list[(uint64_t)shard * a.shard_cap + base + k] = s_q[k];
    __syncthreads();
    if (threadIdx.x == 0) s_n = 0u;
    __syncthreads();
  };
  uint32_t it = 0;
  for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x, ++it) {
    uint32_t* edges = &s_edges[it & 1u];
    if (threadIdx.x == 0) s_edges[(it + 1u) & 1u] = 0u;  // the next tile's, last read a barrier ago
    const uint32_t ty = tile / a.ntx, tx = tile - ty * a.ntx;
    const uint32_t i = tx * a.tw + ci, j = ty * a.th + cj;
    bool obst = false;
    if (i < a.nx && j < a.ny) {
      const int64_t k = (int64_t)j * a.ld + i;
      obst = !(F[k] < kInfD);
      if (obst) a.T[k] = 0.0;
    }
    if (obst) {
      uint32_t e = 0u;
      if (ci == 0u && i > 0u) e |= 1u;
      if (ci == a.tw - 1u && i + 1u < a.nx) e |= 2u;
      if (cj == 0u && j > 0u) e |= 4u;
      if (cj == a.th - 1u && j + 1u < a.ny) e |= 8u;
      if (e) atomicOr(edges, e);
      // 16x16 tiles: column 0 -> ec[0..15], column 15 -> ec[16..31] (k_ec_rebuild); the
      // edge columns are +inf after the cold dom_begin and this tile's are written here only
      if (a.ec && (ci == 0u || ci == 15u))
        a.ec[(uint64_t)tile * 32u + (ci ? 16u : 0u) + cj] = 0.0;
    }
    const int n_obst = __syncthreads_count(obst);
    if (n_obst && threadIdx.x < 5u) {
      const uint32_t e = *edges;
      uint32_t t = tile;
      bool want = true;  // lane 0: the tile itself; 1..4: the tiles across its W, E, N, S edge
      if (threadIdx.x == 1u) want = e & 1u, t = tile - 1u;
      if (threadIdx.x == 2u) want = e & 2u, t = tile + 1u;
      if (threadIdx.x == 3u) want = e & 4u, t = tile - a.ntx;
      if (threadIdx.x == 4u) want = e & 8u, t = tile + a.ntx;
      if (threadIdx.x > 0u && !a.keys) want = false;  // the plain FIM: the own tile only
      if (want) {
        if (a.keys) a.keys[t] = 0ull;  // the bits of +0.0: no other value is stored before the passes
        if (atomicMax(&a.tile_epoch[t], a.epoch) < a.epoch) s_q[atomicAdd(&s_n, 1u)] = t;
      }
      if (threadIdx.x == 0u) cells += (unsigned long long)n_obst;
    }
    __syncthreads();
    if (s_n > kMaskQueue - 8u) flush();  // at most five more per tile
  }
  if (s_n > 0u) flush();
  if (threadIdx.x == 0 && cells) atomicAdd(a.n_obst, cells);
}

// k_seed_mask for a warm field and a window of new obstacles (dymu_clearance_update_device):
// the tiles that meet the clipped window, a workgroup on one tile at a time, one lane per
// cell.  A cell of the window is NEW when it is an obstacle in F and S does not hold +0.0
// yet, FREED when F is finite and S holds +0.0.  w.seed = 0 counts both and writes nothing
// else; w.seed = 1 seeds the new cells as k_seed_mask seeds an obstacle cell: S = +0.0, the
// edge-column entry, the tile and (priority kernels) the tiles across its edges claimed once
// through tile_epoch, collected in LDS and published with one atomic per workgroup.
__global__ __launch_bounds__(256) void k_seed_mask_window(const double* __restrict__ F,
                                                          MaskSeedArgs a, MaskWindow w) {
  __shared__ uint32_t s_q[kMaskQueue];
  __shared__ uint32_t s_n, s_base;
  __shared__ uint32_t s_edges[2];  // as in k_seed_mask
  const uint32_t shard = blockIdx.x % kShards;
  const uint32_t cj = threadIdx.x / a.tw, ci = threadIdx.x - cj * a.tw;
  unsigned long long n_new = 0, n_freed = 0;  // lane 0
  if (threadIdx.x == 0) s_n = s_edges[0] = s_edges[1] = 0u;
  __syncthreads();
  auto flush = [&]() {
    const uint32_t n = s_n;
    if (threadIdx.x == 0) {
      s_base = atomicAdd(&a.counts[shard], n);
      if (a.hist) atomicAdd(&a.hist[shard * kBins], n);  // key_bin(0, base = 0) = 0
    }
    __syncthreads();
    const uint32_t base = s_base;
    for (uint32_t k = threadIdx.x; k < n; k += blockDim.x)
      a.list[(uint64_t)shard * a.shard_cap + base + k] = s_q[k];
    __syncthreads();
    if (threadIdx.x == 0) s_n = 0u;
    __syncthreads();
  };
  const uint32_t nwt = w.ntwx * w.ntwy;
  uint32_t it = 0;
  for (uint32_t q = blockIdx.x; q < nwt; q += gridDim.x, ++it) {
    uint32_t* edges = &s_edges[it & 1u];
    if (threadIdx.x == 0) s_edges[(it + 1u) & 1u] = 0u;
    const uint32_t wy = q / w.ntwx, wx = q - wy * w.ntwx;
    const uint32_t tx = w.tx0 + wx, ty = w.ty0 + wy, tile = ty * a.ntx + tx;
    const uint32_t i = tx * a.tw + ci, j = ty * a.th + cj;
    bool fresh = false, freed = false;
    if (i >= w.i0 && i < w.i1 && j >= w.j0 && j < w.j1) {  // i1 <= nx, j1 <= ny
      const int64_t k = (int64_t)j * a.ld + i;
      const bool obst = !(F[k] < kInfD);
      const bool zero = __double_as_longlong(a.T[k]) == 0ll;
      fresh = obst && !zero;
      freed = !obst && zero;
    }
    if (!w.seed) {
      const int nn = __syncthreads_count(fresh), nf = __syncthreads_count(freed);
      if (threadIdx.x == 0u) n_new += (unsigned long long)nn, n_freed += (unsigned long long)nf;
      continue;
    }
    if (fresh) {
      a.T[(int64_t)j * a.ld + i] = 0.0;
      uint32_t e = 0u;
      if (ci == 0u && i > 0u) e |= 1u;
      if (ci == a.tw - 1u && i + 1u < a.nx) e |= 2u;
      if (cj == 0u && j > 0u) e |= 4u;
      if (cj == a.th - 1u && j + 1u < a.ny) e |= 8u;
      if (e) atomicOr(edges, e);
      if (a.ec && (ci == 0u || ci == 15u))
        a.ec[(uint64_t)tile * 32u + (ci ? 16u : 0u) + cj] = 0.0;
    }
    const int n_fresh = __syncthreads_count(fresh);
    if (n_fresh && threadIdx.x < 5u) {
      const uint32_t e = *edges;
      uint32_t t = tile;
      bool want = true;  // lane 0: the tile itself; 1..4: the tiles across its W, E, N, S edge
      if (threadIdx.x == 1u) want = e & 1u, t = tile - 1u;
      if (threadIdx.x == 2u) want = e & 2u, t = tile + 1u;
      if (threadIdx.x == 3u) want = e & 4u, t = tile - a.ntx;
      if (threadIdx.x == 4u) want = e & 8u, t = tile + a.ntx;
      if (threadIdx.x > 0u && !a.keys) want = false;
      if (want) {
        if (a.keys) a.keys[t] = 0ull;
        if (atomicMax(&a.tile_epoch[t], a.epoch) < a.epoch) s_q[atomicAdd(&s_n, 1u)] = t;
      }
    }
    __syncthreads();
    if (s_n > kMaskQueue - 8u) flush();
  }
  if (w.seed) {
    if (s_n > 0u) flush();
  } else if (threadIdx.x == 0) {
    if (n_new) atomicAdd(a.n_obst, n_new);
    if (n_freed) atomicAdd(w.n_freed, n_freed);
  }
}

// box = {x0, y0, x1, y1} in tiles (x1, y1 exclusive; from {~0, ~0, 0, 0}) over the tiles whose
// stamp is at least epoch_lo, the first epoch of the domain that just ran: the tiles some
// list of it held.  A lane's tiles by grid stride, a shuffle reduction per wave, the waves'
// results through LDS, one atomic per word and workgroup.
__global__ __launch_bounds__(256) void k_claimed_box(const uint32_t* __restrict__ tile_epoch,
                                                     uint32_t ntiles, uint32_t ntx,
                                                     uint32_t epoch_lo, uint32_t* box) {
  __shared__ uint32_t s_box[8][4];  // up to 8 waves of 32
  uint32_t x0 = ~0u, y0 = ~0u, x1 = 0u, y1 = 0u;
  for (uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x; t < ntiles;
       t += (uint64_t)gridDim.x * 256u)
    if (tile_epoch[t] >= epoch_lo) {
      const uint32_t ty = (uint32_t)t / ntx, tx = (uint32_t)t - ty * ntx;
      x0 = min(x0, tx), y0 = min(y0, ty), x1 = max(x1, tx + 1u), y1 = max(y1, ty + 1u);
    }
  for (int off = warpSize / 2; off > 0; off >>= 1) {
    x0 = min(x0, (uint32_t)__shfl_xor((int)x0, off));
    y0 = min(y0, (uint32_t)__shfl_xor((int)y0, off));
    x1 = max(x1, (uint32_t)__shfl_xor((int)x1, off));
    y1 = max(y1, (uint32_t)__shfl_xor((int)y1, off));
  }
  const uint32_t wave = threadIdx.x / warpSize, nwaves = blockDim.x / warpSize;
  if (threadIdx.x % warpSize == 0u)
    s_box[wave][0] = x0, s_box[wave][1] = y0, s_box[wave][2] = x1, s_box[wave][3] = y1;
  __syncthreads();
  if (threadIdx.x == 0u) {
    for (uint32_t v = 1; v < nwaves; ++v) {
      x0 = min(x0, s_box[v][0]), y0 = min(y0, s_box[v][1]);
      x1 = max(x1, s_box[v][2]), y1 = max(y1, s_box[v][3]);
    }
    if (x1) {
      atomicMin(&box[0], x0);
      atomicMin(&box[1], y0);
      atomicMax(&box[2], x1);
      atomicMax(&box[3], y1);
    }
  }
}

// The cone's boundary after a seeded raise (dymu_clearance_edit_device), in two launches so
// that the first reads the raise's stamps while nothing overwrites them: the pass domain's
// claims go to the same array, and with 8-cell pass tiles to other indices of it.
//
// k_cone_keys: a workgroup of 256 lanes on one 16x16 raise tile of the box at a time, one
// lane per cell.  A tile the raise did not claim is skipped: its +inf cells beside finite
// ones are where the old solve stopped at the level, not a cone.  A boundary cell lowers the
// key of its pass tile (one of up to four under a raise tile) through LDS, then one atomic
// per pass tile and raise tile on the key, and one on theta.
__global__ __launch_bounds__(256) void k_cone_keys(ConeArgs a) {
  __shared__ unsigned long long s_key[4];
  constexpr unsigned long long kInfBits = 0x7FF0000000000000ull;
  const uint32_t ci = threadIdx.x & 15u, cj = threadIdx.x >> 4;
  const uint32_t per = 16u / a.tw;  // pass tiles per raise tile edge: 1 or 2 (tw = th)
  const uint32_t sub = (cj / a.th) * per + ci / a.tw;
  const uint32_t nb = a.nbx * a.nby;
  for (uint32_t q = blockIdx.x; q < nb; q += gridDim.x) {  // block-uniform
    const uint32_t by = q / a.nbx, tx = a.bx0 + (q - by * a.nbx), ty = a.by0 + by;
    if (a.tile_epoch[ty * a.ntx16 + tx] < a.stamp_lo) continue;
    if (threadIdx.x < 4u) s_key[threadIdx.x] = kInfBits;
    __syncthreads();
    const uint32_t i = tx * 16u + ci, j = ty * 16u + cj;
    if (i < a.nx && j < a.ny) {
      const int64_t k = (int64_t)j * a.ld + i;
      if (a.S[k] == kInfD && a.F[k] < kInfD) {
        double m = kInfD;  // S >= 0 and never NaN: fmin over the in-grid neighbours
        if (j > 0u) m = fmin(m, a.S[k - a.ld]);
        if (i > 0u) m = fmin(m, a.S[k - 1]);
        if (i + 1u < a.nx) m = fmin(m, a.S[k + 1]);
        if (j + 1u < a.ny) m = fmin(m, a.S[k + a.ld]);
        if (m < kInfD) atomicMin(&s_key[sub], (unsigned long long)__double_as_longlong(m));
      }
    }
    __syncthreads();
    if (threadIdx.x < per * per && s_key[threadIdx.x] != kInfBits) {
      const uint32_t px = tx * per + threadIdx.x % per, py = ty * per + threadIdx.x / per;
      atomicMin(&a.keys[py * a.ntx + px], s_key[threadIdx.x]);
      atomicMin(a.theta_bits, s_key[threadIdx.x]);
    }
    __syncthreads();  // s_key is written again for the next tile
  }
}

// k_cone_queue: a lane per pass tile under the raise's box; a tile whose key is finite --
// k_cone_keys lowered it, or the seeding of the added cells stored +0.0 and claimed the tile
// already -- enters list 0 once.  The histogram is binned from the final keys afterwards.
__global__ __launch_bounds__(256) void k_cone_queue(ConeArgs a) {
  const uint32_t per = 16u / a.tw;
  const uint32_t px0 = a.bx0 * per, py0 = a.by0 * per;
  const uint32_t nty = (a.ny + a.th - 1u) / a.th;
  const uint32_t pw = min((a.bx0 + a.nbx) * per, a.ntx) - px0;
  const uint32_t ph = min((a.by0 + a.nby) * per, nty) - py0;
  const uint32_t n = pw * ph, shard = blockIdx.x % kShards;
  for (uint32_t q = blockIdx.x * 256u + threadIdx.x; q < n; q += gridDim.x * 256u) {
    const uint32_t y = q / pw, t = (py0 + y) * a.ntx + px0 + (q - y * pw);
    if (a.keys[t] == 0x7FF0000000000000ull) continue;
    if (atomicMax(&a.tile_epoch[t], a.epoch) < a.epoch)
      a.list[(uint64_t)shard * a.shard_cap + atomicAdd(&a.counts[shard], 1u)] = t;
  }
}

// a wave on 64 consecutive doubles of a row, 2-D grid stride; out may be F (every cell is
// read and written by its own lane)
__global__ __launch_bounds__(256) void k_inflate_speed(const double* F, const double* S,
                                                       double* out, uint64_t ld, uint32_t nx,
                                                       uint32_t ny, double risk_ratio) {
  for (uint64_t r = blockIdx.y; r < ny; r += gridDim.y) {
    const uint64_t row = r * ld;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < nx;
         i += (uint64_t)gridDim.x * 256u) {
      const double R = fmax(1.0 - S[row + i], 0.0);
      out[row + i] = F[row + i] * (risk_ratio * R + 1.0);
    }
  }
}

dim3 row_grid(uint32_t nx, uint32_t ny) {
  const unsigned gx = (unsigned)std::min<uint64_t>(((uint64_t)nx + 255u) / 256u, 64u);
  const unsigned gy = (unsigned)std::min<uint64_t>(ny, 16384u);
  return dim3(gx, gy);
}

}  // namespace

hipError_t launch_fill_const(double* W, uint64_t ld, uint32_t nx, uint32_t ny, double v,
                             hipStream_t st) {
  hipLaunchKernelGGL(k_fill_const, row_grid(nx, ny), dim3(256), 0, st, W, ld, nx, ny, v);
  return hipGetLastError();
}

hipError_t launch_seed_mask(const double* F, const MaskSeedArgs& a, uint32_t ntiles, uint32_t blocks,
                            hipStream_t st) {
  hipLaunchKernelGGL(k_seed_mask, dim3(std::min(ntiles, std::max(blocks, 1u))), dim3(a.tw * a.th),
                     0, st, F, a, ntiles);
  return hipGetLastError();
}

hipError_t launch_seed_mask_window(const double* F, const MaskSeedArgs& a, const MaskWindow& w,
                                   uint32_t blocks, hipStream_t st) {
  const uint32_t nwt = w.ntwx * w.ntwy;
  hipLaunchKernelGGL(k_seed_mask_window, dim3(std::min(nwt, std::max(blocks, 1u))),
                     dim3(a.tw * a.th), 0, st, F, a, w);
  return hipGetLastError();
}

hipError_t launch_claimed_box(const uint32_t* tile_epoch, uint32_t ntiles, uint32_t ntx,
                              uint32_t epoch_lo, uint32_t* box, hipStream_t st) {
  const unsigned blocks = (unsigned)std::min<uint64_t>(((uint64_t)ntiles + 255u) / 256u, 1024u);
  hipLaunchKernelGGL(k_claimed_box, dim3(blocks), dim3(256), 0, st, tile_epoch, ntiles, ntx,
                     epoch_lo, box);
  return hipGetLastError();
}

hipError_t launch_cone_keys(const ConeArgs& a, uint32_t blocks, hipStream_t st) {
  const uint32_t nb = a.nbx * a.nby;
  if (nb == 0u) return hipSuccess;
  hipLaunchKernelGGL(k_cone_keys, dim3(std::min(nb, std::max(blocks, 1u))), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_cone_queue(const ConeArgs& a, hipStream_t st) {
  const uint64_t per = 16u / a.tw, n = (uint64_t)a.nbx * per * a.nby * per;
  if (n == 0u) return hipSuccess;
  const unsigned blocks = (unsigned)std::min<uint64_t>((n + 255u) / 256u, 1024u);
  hipLaunchKernelGGL(k_cone_queue, dim3(blocks), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_inflate_speed(const double* F, const double* S, double* out, uint64_t ld,
                                uint32_t nx, uint32_t ny, double risk_ratio, hipStream_t st) {
  hipLaunchKernelGGL(k_inflate_speed, row_grid(nx, ny), dim3(256), 0, st, F, S, out, ld, nx, ny,
                     risk_ratio);
  return hipGetLastError();
}

}  // namespace dymu
