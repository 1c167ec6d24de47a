// goal_kernels.hip -- goal sets: multi-source seeding of a cold solve and the
// nearest-goal label map.
//
// Seeding: k_seed_values min-writes every seed's t0 into T (and into its tile's key
// and, for kernel 5, its tile's edge columns); k_seed_tiles then claims each distinct
// tile once through tile_epoch (the k_seed idiom), appends it to list 0 and bins it by
// its FINAL key against base = min t0 -- two launches, so that a tile's bin does not
// depend on the order its seeds arrived in.  The pass kernels run unchanged behind it.
//
// Labels: the label of a cell is a function of T alone.  k_label_init writes, per
// cell, either a resolved label (top bit set) or the index of the cell's parent (the
// first smallest strictly lower 4-neighbour); k_label_jump halves every chain in place
// (L[c] <- L[L[c]]) until a device counter of unresolved entries reaches 0;
// k_label_strip removes the tag bit.
#include "fim_kernels.h"

namespace dymu {
namespace {

constexpr uint32_t kTag = 0x80000000u;       // L entry: resolved (low 31 bits: the label)
constexpr uint32_t kNone = 0xFFFFFFFFu;      // resolved, no goal (DYMU_LABEL_NONE)
constexpr double kInfD = __builtin_huge_val();

__device__ __forceinline__ unsigned long long dbits(double v) {
  return (unsigned long long)__double_as_longlong(v);
}
__device__ __forceinline__ double bitsd(unsigned long long b) {
  return __longlong_as_double((long long)b);
}
// fim_kernels.hip's key_bin, operation by operation: the pass that reads list 0
// classifies a tile with that function, and the histogram must agree with it
__device__ __forceinline__ int key_bin(double k, double origin, double inv_delta) {
  const float x = (float)((k - origin) * inv_delta);
  if (!(x > 0.0f)) return 0;
  const float b = 4.0f * __builtin_amdgcn_logf(1.0f + x);
  return b < (float)(kBins - 1) ? (int)b : kBins - 1;
}

// fn(tile) for the tiles a seed queues (fim_kernels.h SeedTiles): its own, then the tile
// across each tile edge its cell lies on
template <class Fn>
__device__ __forceinline__ void for_seed_tiles(const SeedArgs& a, const GoalSeed& sd, Fn fn) {
  const uint32_t tile = (sd.j / a.th) * a.ntx + sd.i / a.tw;
  fn(tile);
  if (!a.keys) return;  // the plain FIM (kernel 3) keeps the seed's own tile only
  const uint32_t ci = sd.i % a.tw, cj = sd.j % a.th;
  if (ci == 0u && sd.i > 0u) fn(tile - 1u);
  if (ci == a.tw - 1u && sd.i + 1u < a.nx) fn(tile + 1u);
  if (cj == 0u && sd.j > 0u) fn(tile - a.ntx);
  if (cj == a.th - 1u && sd.j + 1u < a.ny) fn(tile + a.ntx);
}

// t0 >= +0.0 and finite (checked on the host), so the bit patterns order like the values
__global__ void k_seed_values(SeedArgs a) {
  for (uint32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < a.n; s += gridDim.x * blockDim.x) {
    const GoalSeed sd = a.seeds[s];
    if (sd.i >= a.nx || sd.j >= a.ny) continue;  // rejected on the host; never indexed here
    const unsigned long long b = dbits(sd.t0);
    atomicMin(reinterpret_cast<unsigned long long*>(a.T + (int64_t)sd.j * a.ld + sd.i), b);
    const uint32_t tile = (sd.j / a.th) * a.ntx + sd.i / a.tw;
    if (a.keys) for_seed_tiles(a, sd, [&](uint32_t t) { atomicMin(&a.keys[t], b); });
    if (a.ec) {  // 16x16 tiles: column 0 -> ec[0..15], column 15 -> ec[16..31] (k_ec_rebuild)
      const uint32_t ci = sd.i % 16u, r = sd.j % 16u;
      if (ci == 0u || ci == 15u)
        atomicMin(reinterpret_cast<unsigned long long*>(a.ec + (uint64_t)tile * 32 +
                                                        (ci ? 16u : 0u) + r),
                  b);
    }
  }
}

__global__ void k_seed_tiles(SeedArgs a) {
  const uint32_t shard = blockIdx.x % kShards;
  for (uint32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < a.n; s += gridDim.x * blockDim.x) {
    const GoalSeed sd = a.seeds[s];
    if (sd.i >= a.nx || sd.j >= a.ny) continue;
    for_seed_tiles(a, sd, [&](uint32_t tile) {
      if (atomicMax(&a.tile_epoch[tile], a.epoch) < a.epoch) {
        const uint32_t pos = atomicAdd(&a.counts[shard], 1u);
        a.list[(uint64_t)shard * a.shard_cap + pos] = tile;
        if (a.hist)
          atomicAdd(&a.hist[shard * kBins + key_bin(bitsd(a.keys[tile]), *a.base, 1.0 / *a.delta)],
                    1u);
      }
    });
  }
}

// ---- labels ----

__device__ __forceinline__ uint32_t ld_relaxed(const uint32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_relaxed(uint32_t* p, uint32_t v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the parent of every cell, or NONE: +inf / NaN cells and cells without a strictly
// lower neighbour.  Neighbours in the reference's nb4 order (i,j-1), (i-1,j), (i+1,j),
// (i,j+1); the first one holding the smallest value wins.
__global__ __launch_bounds__(256) void k_label_init(const double* T, int64_t ld, uint32_t nx,
                                                    uint32_t ny, uint32_t* L) {
  const uint32_t n = nx * ny;  // < 2^31 (checked on the host)
  const uint32_t c = blockIdx.x * 256u + threadIdx.x;
  if (c >= n) return;
  const uint32_t j = c / nx, i = c - j * nx;
  const double* p = T + (int64_t)j * ld + i;
  const double t = *p;
  uint32_t v = kNone;
  if (t < kInfD) {
    double best = t;
    if (j > 0) {
      const double u = p[-ld];
      if (u < best) { best = u; v = c - nx; }
    }
    if (i > 0) {
      const double u = p[-1];
      if (u < best) { best = u; v = c - 1u; }
    }
    if (i + 1u < nx) {
      const double u = p[1];
      if (u < best) { best = u; v = c + 1u; }
    }
    if (j + 1u < ny) {
      const double u = p[ld];
      if (u < best) { best = u; v = c + nx; }
    }
  }
  L[c] = v;
}

// roots, after k_label_init: a seed whose cell holds exactly its t0.  step 0 clears the
// cell's entry, step 1 min-writes tag | k -- with duplicates only the seeds of the
// smallest t0 can match T, and the lowest k among them wins.
__global__ void k_label_roots(const double* T, int64_t ld, uint32_t nx, uint32_t ny,
                              const GoalSeed* seeds, uint32_t n_seeds, uint32_t* L, int step) {
  for (uint32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < n_seeds;
       s += gridDim.x * blockDim.x) {
    const GoalSeed sd = seeds[s];
    if (sd.i >= nx || sd.j >= ny) continue;
    if (dbits(T[(int64_t)sd.j * ld + sd.i]) != dbits(sd.t0)) continue;  // dominated
    uint32_t* e = L + ((uint64_t)sd.j * nx + sd.i);
    if (step == 0) *e = kNone;
    else atomicMin(e, kTag | s);
  }
}

// One in-place jump.  An entry read here may be another lane's old or new value: both
// point further along the same chain (or are its resolved label), so the race only
// changes how fast a chain shortens.  cnt[round] += the entries still unresolved after
// this round (one ballot per wave and step, one atomic per workgroup); a round that
// finds the previous round's count at 0 has nothing to do.  The grid is capped
// (kJumpBlocks) and strided: the counter is one address, and a million workgroups'
// atomics on it would serialise into more time than the jumps take.
constexpr uint32_t kJumpBlocks = 8192;
__global__ __launch_bounds__(256) void k_label_jump(uint32_t* L, uint32_t n, uint32_t* cnt,
                                                    uint32_t round) {
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
      const uint32_t v = ld_relaxed(L + c);
      if (!(v & kTag)) {  // a cell index written by k_label_init or an earlier jump
        const uint32_t w = v < n ? ld_relaxed(L + v) : kNone;
        st_relaxed(L + c, w);
        open = !(w & kTag);
      }
    }
    wave_open += (uint32_t)__popcll(__ballot(open));
  }
  if ((threadIdx.x & 63u) == 0u && wave_open) atomicAdd(&s_open, wave_open);
  __syncthreads();
  if (threadIdx.x == 0 && s_open) atomicAdd(&cnt[round], s_open);
}

__global__ __launch_bounds__(256) void k_label_strip(uint32_t* L, uint32_t n) {
  const uint32_t c = blockIdx.x * 256u + threadIdx.x;
  if (c >= n) return;
  const uint32_t v = L[c];
  // an entry still unresolved (the round cap was hit) has no label
  L[c] = (v & kTag) ? (v == kNone ? kNone : (v & ~kTag)) : kNone;
}

uint32_t seed_blocks(uint32_t n) { return n < 256u * 1024u ? (n + 255u) / 256u : 1024u; }

}  // namespace

hipError_t launch_seed_goals(const SeedArgs& a, hipStream_t st) {
  if (a.n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_seed_values, dim3(seed_blocks(a.n)), dim3(256), 0, st, a);
  hipLaunchKernelGGL(k_seed_tiles, dim3(seed_blocks(a.n)), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_label_init(const double* T, int64_t ld, uint32_t nx, uint32_t ny,
                             const GoalSeed* seeds, uint32_t n_seeds, uint32_t* L,
                             hipStream_t st) {
  const uint32_t n = nx * ny;
  hipLaunchKernelGGL(k_label_init, dim3((n + 255u) / 256u), dim3(256), 0, st, T, ld, nx, ny, L);
  for (int step = 0; step < 2; ++step)
    hipLaunchKernelGGL(k_label_roots, dim3(seed_blocks(n_seeds)), dim3(256), 0, st, T, ld, nx, ny,
                       seeds, n_seeds, L, step);
  return hipGetLastError();
}

hipError_t launch_label_jump(uint32_t* L, uint32_t n, uint32_t* cnt, uint32_t round,
                             hipStream_t st) {
  const uint32_t blocks = (n + 255u) / 256u;
  hipLaunchKernelGGL(k_label_jump, dim3(blocks < kJumpBlocks ? blocks : kJumpBlocks), dim3(256), 0,
                     st, L, n, cnt, round);
  return hipGetLastError();
}

hipError_t launch_label_strip(uint32_t* L, uint32_t n, hipStream_t st) {
  hipLaunchKernelGGL(k_label_strip, dim3((n + 255u) / 256u), dim3(256), 0, st, L, n);
  return hipGetLastError();
}

}  // namespace dymu
