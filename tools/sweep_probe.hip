// sweep_probe.hip -- where does a kernel-5 half-sweep's time go?  (development
// probe, not part of the product)  Every wave of one workgroup per CU runs a
// fixed number of red-black sweep pairs over its own 16x16 tile image in LDS,
// with kernel 5's own update (rb_update2<true, true>, fim_kernels.hip), and the
// kernel is timed with events.  Variants:
//   0  kernel 5's half-sweep: 7 LDS reads, the update, 2 LDS writes  (full)
//   1  the same without the LDS writes (reads + VALU)                (no-write)
//   2  LDS reads + writes with a few v_min instead of the update     (LDS only)
//   3  the update (cand_approx2) on register values only             (VALU only)
// Read form: "merged" = plain loads, which the compiler pairs into 3
// ds_read2_b64 + 1 ds_read_b64 per half-sweep (kernel 5 up to v35); "single" =
// 7 ds_read_b64 (lds_read64, kernel 5 from v38).  Write form: "w2" = one
// ds_write2_b64 per half-sweep (kernel 5 up to v35), "w1" = two ds_write_b64
// (img_put2, kernel 5 from v38).
// Waves per CU W = 4 / 8 / 12 / 16 give 1..4 waves per SIMD.  Each table is
// printed REPS times so the run-to-run spread stands next to the differences.
// Usage: sweep_probe [pairs = 20000] [reps = 3]
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -Iplanning-path_planning_amd/csrc \
//          -Iinclude tools/sweep_probe.hip -o tools/sweep_probe
#include "../planning-path_planning_amd/csrc/fim_kernels.hip"

#include <cstdio>
#include <cstdlib>

namespace probe {
using namespace dymu;

// variant 2's half-sweep: the seven reads, three v_min per cell, the two writes
template <bool SINGLE, bool SPLITW>
__device__ __forceinline__ void lds_only(double* p, const double* pn, const double* ps, double& t0,
                                         double& t1) {
  double a0, a1, a2, a3, a4, a5, a6;
  if constexpr (SINGLE) {
    a0 = lds_read64(p - 1), a1 = lds_read64(p + 1), a2 = lds_read64(pn), a3 = lds_read64(ps);
    a4 = lds_read64(p + 3), a5 = lds_read64(pn + 2), a6 = lds_read64(ps + 2);
  } else {
    a0 = p[-1], a1 = p[1], a2 = pn[0], a3 = ps[0], a4 = p[3], a5 = pn[2], a6 = ps[2];
  }
  t0 = vmin64(t0, vmin64(vmin64(a0, a1), vmin64(a2, a3)));
  t1 = vmin64(t1, vmin64(vmin64(a1, a4), vmin64(a5, a6)));
  img_put2<SPLITW>(p, t0, t1);
}

// variant 3's half-sweep: rb_update2<true, true>'s arithmetic, the seven
// neighbour values made from the other colour's registers instead of read
__device__ __forceinline__ void valu_only(double x0, double x1, double f0, double f1, double& t0,
                                          double& t1, bool& ch0, bool& ch1) {
  double w0 = x0 + 1, e0 = x1 + 2, n0 = x0 + 3, so0 = x1 + 4, e1 = x0 + 5, n1 = x1 + 6, so1 = x0 + 7;
  asm volatile("" : "+v"(w0), "+v"(e0), "+v"(n0), "+v"(so0), "+v"(e1), "+v"(n1), "+v"(so1));
  const double w1 = e0;
  const double c20 = 2.0 * (f0 * f0), c21 = 2.0 * (f1 * f1);
  const double tx0 = vmin64(w0, e0), ty0 = vmin64(n0, so0);
  const double tx1 = vmin64(w1, e1), ty1 = vmin64(n1, so1);
  const double m0 = vmin64(tx0, ty0), m1 = vmin64(tx1, ty1);
  const double d0 = tx0 - ty0, d1 = tx1 - ty1;
  double u0, u1;
  cand_approx2(vmin64_abs(d0, f0), c20, m0, vmin64_abs(d1, f1), c21, m1, u0, u1);
  ch0 = u0 < t0;
  ch1 = u1 < t1;
  t0 = vmin64(t0, u0);
  t1 = vmin64(t1, u1);
}

template <int V, bool SINGLE, bool SPLITW>
__global__ __launch_bounds__(1024) void k_probe(double* sink, int pairs) {
  __shared__ double s_img[16][IMG16];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  double* img = s_img[wv];
  for (int k = lane; k < IMG16; k += 64) img[k] = 1000.0 + (double)((k * 37) % 101);
  const int r = lane >> 2, q = lane & 3, odd = r & 1;
  const int rb = img16_row(r);
  const int dn = img16_row(r + 1) - rb, ds = rb - img16_row(r - 1);
  double* pr = img + rb + 4 * q + odd;
  double* pb = img + rb + 4 * q + 1 - odd;
  const double *prn = pr + dn, *prs = pr - ds, *pbn = pb + dn, *pbs = pb - ds;
  double fr[2] = {1.5 + 0.01 * lane, 2.5}, fb[2] = {3.0, 1.25 + 0.02 * lane};
  __builtin_amdgcn_wave_barrier();
  double tr[2] = {pr[0], pr[2]}, tb[2] = {pb[0], pb[2]};
  bool c0 = false, c1 = false, c2 = false, c3 = false;
  __builtin_amdgcn_wave_barrier();
  for (int s = 0; s < pairs; ++s) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      if constexpr (V == 0 || V == 1) {
        __builtin_amdgcn_wave_barrier();
        rb_update2<true, true, SINGLE>(pr, prn, prs, fr[0], fr[1], tr[0], tr[1], c0, c1);
        if constexpr (V == 0) img_put2<SPLITW>(pr, tr[0], tr[1]);
        __builtin_amdgcn_wave_barrier();
        rb_update2<true, true, SINGLE>(pb, pbn, pbs, fb[0], fb[1], tb[0], tb[1], c2, c3);
        if constexpr (V == 0) img_put2<SPLITW>(pb, tb[0], tb[1]);
      } else if constexpr (V == 2) {
        __builtin_amdgcn_wave_barrier();
        lds_only<SINGLE, SPLITW>(pr, prn, prs, tr[0], tr[1]);
        __builtin_amdgcn_wave_barrier();
        lds_only<SINGLE, SPLITW>(pb, pbn, pbs, tb[0], tb[1]);
      } else {
        valu_only(tb[0], tb[1], fr[0], fr[1], tr[0], tr[1], c0, c1);
        valu_only(tr[0], tr[1], fb[0], fb[1], tb[0], tb[1], c2, c3);
      }
    }
  }
  sink[blockIdx.x * blockDim.x + threadIdx.x] = tr[0] + tr[1] + tb[0] + tb[1] + (c0 + c1 + c2 + c3);
}

}  // namespace probe

#define CK(x)                                                             \
  do {                                                                    \
    hipError_t e_ = (x);                                                  \
    if (e_ != hipSuccess) {                                               \
      std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));        \
      std::exit(1);                                                       \
    }                                                                     \
  } while (0)

// ns per sweep pair (2 sweeps = 4 half-sweeps, 8 cell updates per lane) with
// `waves` waves on every CU
template <int V, bool SINGLE, bool SPLITW>
static double run(double* sink, int cus, int waves, int pairs) {
  hipEvent_t a, b;
  CK(hipEventCreate(&a));
  CK(hipEventCreate(&b));
  hipLaunchKernelGGL((probe::k_probe<V, SINGLE, SPLITW>), dim3(cus), dim3(64 * waves), 0, 0, sink,
                     pairs);
  CK(hipDeviceSynchronize());
  CK(hipEventRecord(a));
  hipLaunchKernelGGL((probe::k_probe<V, SINGLE, SPLITW>), dim3(cus), dim3(64 * waves), 0, 0, sink,
                     pairs);
  CK(hipEventRecord(b));
  CK(hipEventSynchronize(b));
  float ms = 0;
  CK(hipEventElapsedTime(&ms, a, b));
  CK(hipEventDestroy(a));
  CK(hipEventDestroy(b));
  return 1e6 * ms / pairs;
}

template <bool SINGLE, bool SPLITW>
static void table(double* sink, int cus, int pairs, int rep) {
  for (int w : {4, 8, 12, 16}) {
    const double full = run<0, SINGLE, SPLITW>(sink, cus, w, pairs);
    const double now = run<1, SINGLE, SPLITW>(sink, cus, w, pairs);
    const double lds = run<2, SINGLE, SPLITW>(sink, cus, w, pairs);
    const double valu = run<3, SINGLE, SPLITW>(sink, cus, w, pairs);
    std::printf("rep %d reads %-6s writes %s waves/CU %2d (%d per SIMD): full %7.1f  no-write %7.1f  "
                "LDS-only %7.1f  VALU-only %7.1f  ns per sweep pair\n",
                rep, SINGLE ? "single" : "merged", SPLITW ? "w1" : "w2", w, w / 4, full, now, lds,
                valu);
  }
}

int main(int argc, char** argv) {
  const int pairs = argc > 1 ? std::atoi(argv[1]) : 20000;
  const int reps = argc > 2 ? std::atoi(argv[2]) : 3;
  int dev = 0, cus = 0;
  CK(hipGetDevice(&dev));
  CK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  double* sink = nullptr;
  CK(hipMalloc(&sink, sizeof(double) * (size_t)cus * 1024));
  for (int rep = 1; rep <= reps; ++rep) {
    table<false, false>(sink, cus, pairs, rep);
    table<true, false>(sink, cus, pairs, rep);
    table<false, true>(sink, cus, pairs, rep);
    table<true, true>(sink, cus, pairs, rep);
  }
  CK(hipFree(sink));
  return 0;
}
