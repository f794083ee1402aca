// Spectrum mode: the K largest eigenpairs of every system (1 <= K <= kMaxModes), mode 0 = lam_max, the values descending.  Every odd N
// in [66, 65,537], FP64, one wavefront per system on a persistent grid, everything in division form on the rows in memory (the
// pieces of the long-grid path, ibs_long.hpp):
//   1. bounds        ||A||, the spectrum's bounds [lmin, hi] and the data checks of long_bounds<true>
//   2. eigenvalues   simultaneous multisection (ibs_modes.hpp: the bookkeeping, plain C++): one bracket per mode, every pass of 64
//                    shifts (count_above_chunked) tightens all of them; closed to 2 eps ||A||; kModesPassCap passes, then status bit 0
//   3. clusters      one more count at lam_{K-1} - tau, tau = 4 N eps ||A||; adjacent modes less than tau apart carry the informational
//                    status bit kModesClusterBit (their vector: some vector of the cluster's invariant subspace)
//   4. eigenvectors  per mode, twisted factorisation and the FD4 / Simpson quotient (long_vector_growth<true>), the entry of largest
//                    magnitude +1.  The modes run one after the other: see docs/EXPERIMENTS.md for the form with all pivot recurrences
//                    in one pass.
// Outputs at sys * n_modes + m (X / dX: rows of N there); info = passes of the system's multisection (bits 0-15, the same in all its
// modes) | the mode's status << 16.  Invalid data (status bit 1 on every mode of the system): lam, gam and the X / dX rows are written
// as NaN (the nearest-sigma kernel leaves X / dX of such a system alone; here no row of a caller's buffer stays unwritten).
// Per-wave workspace: modes_ws_doubles(N) (ibs_launch.hpp) in global memory -- the eigenvector stage's three rows, then the closed
// eigenvalues and status words the per-mode loop reads back.
#include "ibs_long.hpp"
#include "ibs_modes.hpp"
#include "ibs_launch.hpp"

namespace ibs {

// the 64 (shift, count) pairs of a pass, as modes_tighten reads them
struct ModesWave {
  double sig; int cnt;
  __device__ __forceinline__ unsigned long long inside_ge(double lo, double hi, int k) const {
    return __builtin_amdgcn_ballot_w64(sig > lo && sig < hi && cnt >= k);
  }
  __device__ __forceinline__ unsigned long long inside_lt(double lo, double hi, int k) const {
    return __builtin_amdgcn_ballot_w64(sig > lo && sig < hi && cnt < k);
  }
  __device__ __forceinline__ double shift(int lane) const { return readlane_t(sig, lane); }
};

template <bool HAS_GH>
__global__ void __launch_bounds__(64) k_solve_gcf_modes(long n_sys, int N, double h, const double* __restrict__ g,
                                                        const double* __restrict__ c, const double* __restrict__ f,
                                                        const double* __restrict__ gh, long ld, int K, double* lam_out, double* gam_out,
                                                        double* X_out, double* dX_out, int* info_out, double* work) {
  __shared__ double lds[3 * kLongChunk];                    // (the LDS budget of the long path: static_assert at kLongChunk)
  static_assert(sizeof(lds) * 8 <= 160 * 1024, "eight blocks per CU");
  const int lane = threadIdx.x & 63;
  const int n = N - 2;
  const double ih2 = 1.0 / (h * h);
  double* my = work + (size_t)blockIdx.x * modes_ws_doubles(N);
  double* lam_ws = my + nearest_ws_doubles(N);
  int* st_ws = reinterpret_cast<int*>(lam_ws + kMaxModes);
  const bool want_vec = gam_out || X_out || dX_out;
  for (long sys = blockIdx.x; sys < n_sys; sys += gridDim.x) {
    const SrcLong<double, HAS_GH> src{g + sys * ld, c + sys * ld, f + sys * ld, HAS_GH ? gh + sys * ld : nullptr};
    const LongBounds b = long_bounds<true>(src, N, ih2, lane);
    int passes = 0;
    if (!b.bad) {
      const double stop = 2.0 * Eps<double>::v * b.normA, tau = 4.0 * (double)N * Eps<double>::v * b.normA;
      ModesBrackets br;
      modes_init(br, K, b.lmin, b.hi);
      ModesWave w{0.0, 0};
      while (passes < kModesPassCap && modes_lane_shift(br, stop, lane, w.sig)) {
        w.cnt = count_above_chunked(src, n, ih2, w.sig, lds, lane);
        ++passes;
        modes_tighten(br, stop, w);
      }
      int probe = -1;
      if (modes_all_closed(br, stop)) {
        probe = __builtin_amdgcn_readfirstlane(count_above_chunked(src, n, ih2, modes_probe_shift(br, tau), lds, lane));
        ++passes;
      }
      if (lane == 0) modes_finish(br, stop, tau, probe, lam_ws, st_ws);
      long_fence();
    }
    for (int m = 0; m < K; ++m) {
      const long o = sys * K + m;
      const double lam = b.bad ? __builtin_nan("") : uniform(lam_ws[m]);
      const int status = b.bad ? 2 : __builtin_amdgcn_readfirstlane(st_ws[m]);
      double gam = __builtin_nan("");
      if (want_vec && (status & 3) == 0) {
        gam = long_vector_growth<true, double>(src, N, h, lam, o, my, X_out, dX_out, lds, lane);
      } else {
        for (int j = lane; j < N; j += kWave) {
          if (X_out) X_out[o * N + j] = __builtin_nan("");
          if (dX_out) dX_out[o * N + j] = __builtin_nan("");
        }
      }
      if (lane == 0) {
        if (lam_out) lam_out[o] = lam;
        if (gam_out) gam_out[o] = gam;
        if (info_out) info_out[o] = (passes & 0xffff) | (status << 16);
      }
    }
    long_fence();                                           // (the workspace is reused by this wave's next system)
  }
}

hipError_t launch_gcf_modes(const ModesArgs& a, hipStream_t st) {
  if (a.n_sys <= 0) return hipSuccess;
  if (a.n_modes < 1 || a.n_modes > kMaxModes) return hipErrorInvalidValue;
  const long grid = persistent_grid(a.n_sys, a.n_waves, a.work, a.work_doubles, modes_ws_doubles(a.N));
  if (!grid) return hipErrorInvalidValue;
  if (a.gh) {
    hipLaunchKernelGGL(k_solve_gcf_modes<true>, dim3((unsigned)grid), dim3(64), 0, st, a.n_sys, a.N, a.h, a.g, a.c, a.f, a.gh, a.ld, a.n_modes,
                       a.lam, a.gam, a.X, a.dX, a.info, a.work);
    note_launch(grid, 64, "ibs::k_solve_gcf_modes<true>");
  } else {
    hipLaunchKernelGGL(k_solve_gcf_modes<false>, dim3((unsigned)grid), dim3(64), 0, st, a.n_sys, a.N, a.h, a.g, a.c, a.f, a.gh, a.ld, a.n_modes,
                       a.lam, a.gam, a.X, a.dX, a.info, a.work);
    note_launch(grid, 64, "ibs::k_solve_gcf_modes<false>");
  }
  return hipGetLastError();
}

}  // namespace ibs
