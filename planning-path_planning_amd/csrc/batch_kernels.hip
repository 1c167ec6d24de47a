// batch_kernels.hip -- batched solves: B maps stacked into one domain.
//
// The stack: plane b, row j lives at stacked row b * P + j, P = 16 * ceil((ny + 1) / 16)
// (dymu_batch_plane_rows); rows ny .. P-1 of every plane are wall rows of speed +inf.
// The pass kernels ignore a +inf neighbour, so the planes share passes without
// influencing each other.
//
// k_stack_speed writes the stacked F from B planes (or one shared plane, stride 0);
// k_gather_costs evaluates DyMuPathPlanner::getTotalCost (planner.cpp) for M points on
// every plane of a solved stack: the host's tests in the host's order and its bilinear
// expression operation by operation, built with -ffp-contract=off like the host code,
// so the values are bit-identical to the host's on the same T.
// k_probe_targets is the stop test of the early exit on target cells: the
// largest value among the targets of finite speed, per plane and over the whole stack.
#include "descent_step.h"  // kInfD, grid_u32
#include "fim_kernels.h"

namespace dymu {
namespace {

// one lane per cell of a row strip, rows and column strips by grid stride: a wave
// reads / writes 64 consecutive doubles of one row
__global__ __launch_bounds__(256) void k_stack_speed(const double* __restrict__ src,
                                                     uint64_t src_ld, uint64_t src_plane_stride,
                                                     uint32_t nx, uint32_t ny, uint32_t planes,
                                                     uint32_t P, double* __restrict__ dst,
                                                     uint64_t ld) {
  const uint64_t rows = (uint64_t)planes * P;
  for (uint64_t r = blockIdx.y; r < rows; r += gridDim.y) {
    const uint64_t b = r / P, j = r - b * P;
    const bool wall = j >= ny;
    const double* s = src + b * src_plane_stride + (wall ? 0 : j) * src_ld;
    double* d = dst + r * ld;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < nx;
         i += (uint64_t)gridDim.x * 256u)
      d[i] = wall ? kInfD : s[i];
  }
}

__global__ __launch_bounds__(256) void k_gather_costs(const double* __restrict__ T, uint64_t ld,
                                                      uint32_t nx, uint32_t ny, uint32_t planes,
                                                      uint32_t P, double res,
                                                      const double* __restrict__ xy, uint32_t M,
                                                      double* __restrict__ out) {
  const uint64_t n = (uint64_t)planes * M;
  for (uint64_t q = (uint64_t)blockIdx.x * 256u + threadIdx.x; q < n;
       q += (uint64_t)gridDim.x * 256u) {
    const uint64_t b = q / M, m = q - b * M;
    const double* Tp = T + b * P * ld;  // plane b: an ordinary nx x ny map of pitch ld
    const double x = xy[2 * m], y = xy[2 * m + 1];
    // getTotalCost (:860-890; Q6 kept: a = x - i, not x / res - i)
    const uint64_t i = grid_u32(x / res), j = grid_u32(y / res);
    const double a = x - (double)i, bb = y - (double)j;
    // the nearest node: loaded only once both indices are proven inside the plane
    const uint64_t ni = grid_u32(x / res + 0.5), nj = grid_u32(y / res + 0.5);
    const bool near_in = ni < nx && nj < ny;
    double v;
    if (i >= nx || j >= ny || i + 1 >= nx || j + 1 >= ny) {  // a corner is off the grid
      v = near_in ? Tp[nj * ld + ni] : kInfD;
    } else {
      const uint64_t k = j * ld + i;  // i + 1 < nx, j + 1 < ny: the four corners exist
      const double w00 = Tp[k], w10 = Tp[k + 1], w01 = Tp[k + ld], w11 = Tp[k + ld + 1];
      if (!(w00 < kInfD) || !(w10 < kInfD) || !(w01 < kInfD) || !(w11 < kInfD))
        v = near_in ? Tp[nj * ld + ni] : kInfD;
      else
        v = w00 + (w10 - w00) * a + (w01 - w00) * bb + (w11 + w00 - w10 - w01) * a * bb;
    }
    out[q] = v;
  }
}

// ---- early exit on target cells ----
// The stop test's inputs: the largest value among the counting targets (finite speed) of
// every plane and of the whole stack, as bit patterns -- T >= 0, so bit order is value
// order and +inf wins.  A wave takes 64 consecutive targets per step; they are sorted by
// plane, so it mostly holds one plane: the lanes of the first live lane's plane reduce
// with shuffles and that lane makes the plane's one atomic, until no lane is live.  The
// stack-wide maximum stays in registers over the steps and goes through LDS: one atomic
// per workgroup on out[0], and the grid is capped (kProbeBlocks), so that word sees at
// most that many however long the list is.  A value of 0 needs no atomic (out is zeroed).
// T is read only after the target is proven inside its plane; the index is 64-bit (s5.3).
constexpr uint32_t kProbeBlocks = 256;
constexpr uint32_t kNoPlane = 0xFFFFFFFFu;

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long m) {
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long o = __shfl_xor(m, off, 64);
    m = o > m ? o : m;
  }
  return m;
}

__global__ __launch_bounds__(256) void k_probe_targets(
    const double* __restrict__ F, const double* __restrict__ T, uint64_t ld, uint32_t nx,
    uint32_t ny, uint32_t planes, uint32_t P, const ProbeTarget* __restrict__ tg, uint32_t n,
    const unsigned long long* __restrict__ minkey, unsigned long long* __restrict__ out) {
  __shared__ unsigned long long s_max;
  if (threadIdx.x == 0) s_max = 0ull;
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63u;
  unsigned long long all = 0ull;
  // n < 2^31 and the stride is at most 2^16: base never wraps
  for (uint32_t base = blockIdx.x * 256u; base < n; base += gridDim.x * 256u) {
    const uint32_t k = base + threadIdx.x;
    uint32_t plane = kNoPlane;
    unsigned long long v = 0ull;
    if (k < n) {
      const ProbeTarget t = tg[k];
      if (t.plane < planes && t.i < nx && t.j < ny) {  // rejected on the host otherwise
        const uint64_t idx = ((uint64_t)t.plane * P + t.j) * ld + t.i;
        if (F[idx] < kInfD) {  // a counting target
          plane = t.plane;
          v = (unsigned long long)__double_as_longlong(T[idx]);
        }
      }
    }
    all = v > all ? v : all;
    unsigned long long live = __ballot(plane != kNoPlane);  // wave-uniform
    while (live) {
      const int lead = __ffsll((long long)live) - 1;
      const uint32_t pl = __shfl(plane, lead, 64);
      const bool mine = plane == pl;
      const unsigned long long m = wave_max_u64(mine ? v : 0ull);
      if ((int)lane == lead && m) atomicMax(&out[2 + pl], m);
      live &= ~__ballot(mine);
    }
  }
  all = wave_max_u64(all);
  if (lane == 0u && all) atomicMax(&s_max, all);
  __syncthreads();
  if (threadIdx.x == 0) {
    if (s_max) atomicMax(&out[0], s_max);
    if (blockIdx.x == 0) out[1] = minkey ? *minkey : 0x7FF0000000000000ull;
  }
}

}  // namespace

hipError_t launch_probe_targets(const double* F, const double* T, uint64_t ld, uint32_t nx,
                                uint32_t ny, uint32_t planes, uint32_t P, const ProbeTarget* tg,
                                uint32_t n, const unsigned long long* minkey,
                                unsigned long long* out, hipStream_t st) {
  uint32_t b = (n + 255u) / 256u;
  if (b > kProbeBlocks) b = kProbeBlocks;
  if (b == 0) b = 1;  // out[1] is written even without a target
  hipLaunchKernelGGL(k_probe_targets, dim3(b), dim3(256), 0, st, F, T, ld, nx, ny, planes, P, tg, n,
                     minkey, out);
  return hipGetLastError();
}

hipError_t launch_stack_speed(const double* src, uint64_t src_ld, uint64_t src_plane_stride,
                              uint32_t nx, uint32_t ny, uint32_t planes, uint32_t P, double* dst,
                              uint64_t ld, hipStream_t st) {
  const uint64_t rows = (uint64_t)planes * P;
  if (rows == 0 || nx == 0) return hipSuccess;
  uint32_t gx = (nx + 255u) / 256u;
  if (gx > 64) gx = 64;
  uint64_t gy = 8192u / gx;
  if (gy > rows) gy = rows;
  hipLaunchKernelGGL(k_stack_speed, dim3(gx, (unsigned)gy), dim3(256), 0, st, src, src_ld,
                     src_plane_stride, nx, ny, planes, P, dst, ld);
  return hipGetLastError();
}

hipError_t launch_gather_costs(const double* T, uint64_t ld, uint32_t nx, uint32_t ny,
                               uint32_t planes, uint32_t P, double res, const double* xy,
                               uint32_t M, double* out, hipStream_t st) {
  const uint64_t n = (uint64_t)planes * M;
  if (n == 0) return hipSuccess;
  uint64_t b = (n + 255) / 256;
  if (b > 4096) b = 4096;
  hipLaunchKernelGGL(k_gather_costs, dim3((unsigned)b), dim3(256), 0, st, T, ld, nx, ny, planes,
                     P, res, xy, M, out);
  return hipGetLastError();
}

}  // namespace dymu
