// The eigenpair NEAREST a shift s = sigma[sys]: what the reference's eigs(A, 1, sigma=sigma0, ...) returns (utils.py:1597: ARPACK
// shift-invert, which='LM').  The rest of the library returns lam_max's eigenpair; the two agree only while lam_max < sigma0 (the
// reference's shifts: 1.0 in the coarse scan, ball_scan.py:230 / 269; 1.3 |gam| + 0.05 in the refinement, :289 / 310; 0.42 in the
// final solve, :337).  Every odd N in [66, 65,537], FP64, one wavefront per system on a persistent grid, everything in division form
// on the rows in memory (the pieces of the long-grid path, ibs_long.hpp):
//   1. bounds        ||A||, the upper bound hi and the data checks of long_bounds, plus a lower bound of the whole spectrum
//                    min_r (d_r - e_r - e_{r+1}) / f_r; a non-finite s is invalid data as well (status bit 1)
//   2. eigenvalue    k = count_above(s).  k = 0: s >= lam_max, the nearest is lam_max, found exactly as k_solve_gcf_long finds it.
//                    k >= 1: lam_k (the smallest eigenvalue above s) by multisection for the k-th largest in (s, hi]; with
//                    delta = lam_k - s, if count_above(s - delta - tau) == k no eigenvalue below s is within delta + tau and lam_k is the
//                    nearest; else lam_{k+1} (the largest <= s) by multisection for the (k+1)-th largest in [s - delta - tau, s], and the
//                    nearer of the two is taken.  tau = 4 N eps ||A||; brackets are closed to 2 eps ||A||
//   3. ties          distances that differ by less than tau do not decide: the larger eigenvalue is returned with the informational
//                    status bit 5
//   4. eigenvector   twisted factorisation and the FD4 / Simpson quotient of utils.py:1601-1621 (long_vector_growth), the vector
//                    scaled so that its entry of largest magnitude is +1
// Outputs lam, idx (the number of eigenvalues strictly above the returned one: 0 = lam_max), gam, X, dX, info (bits 0-15 = multisection
// passes in total, status bits as in include/ibs.h).  Per-wave workspace: nearest_ws_doubles(N) (ibs_launch.hpp) in global memory.
#include "ibs_nearest.hpp"
#include "ibs_launch.hpp"

namespace ibs {

template <bool HAS_GH>
__global__ void __launch_bounds__(64) k_solve_gcf_nearest(long n_sys, int N, double h, const double* __restrict__ g,
                                                          const double* __restrict__ c, const double* __restrict__ f,
                                                          const double* __restrict__ gh, long ld, const double* __restrict__ sigma,
                                                          double* lam_out, int* idx_out, double* gam_out, double* X_out, double* dX_out,
                                                          int* info_out, double* work) {
  __shared__ double lds[3 * kLongChunk];                    // (the LDS budget of the long path: static_assert at kLongChunk)
  static_assert(sizeof(lds) * 8 <= 160 * 1024, "eight blocks per CU");
  double* my = work + (size_t)blockIdx.x * nearest_ws_doubles(N);
  for (long sys = blockIdx.x; sys < n_sys; sys += gridDim.x) {
    const SrcLong<double, HAS_GH> src{g + sys * ld, c + sys * ld, f + sys * ld, HAS_GH ? gh + sys * ld : nullptr};
    solve_nearest_one<HAS_GH>(src, N, h, sigma[sys], sys, my, lam_out, idx_out, gam_out, X_out, dX_out, info_out, lds);
    long_fence();                                           // (the workspace is reused by this wave's next system)
  }
}

hipError_t launch_gcf_nearest(const NearestArgs& a, hipStream_t st) {
  if (a.n_sys <= 0) return hipSuccess;
  const long grid = persistent_grid(a.n_sys, a.n_waves, a.work, a.work_doubles, nearest_ws_doubles(a.N));
  if (!grid) return hipErrorInvalidValue;
  if (a.gh) {
    hipLaunchKernelGGL(k_solve_gcf_nearest<true>, dim3((unsigned)grid), dim3(64), 0, st, a.n_sys, a.N, a.h, a.g, a.c, a.f, a.gh, a.ld, a.sigma,
                       a.lam, a.idx, a.gam, a.X, a.dX, a.info, a.work);
    note_launch(grid, 64, "ibs::k_solve_gcf_nearest<true>");
  } else {
    hipLaunchKernelGGL(k_solve_gcf_nearest<false>, dim3((unsigned)grid), dim3(64), 0, st, a.n_sys, a.N, a.h, a.g, a.c, a.f, a.gh, a.ld, a.sigma,
                       a.lam, a.idx, a.gam, a.X, a.dX, a.info, a.work);
    note_launch(grid, 64, "ibs::k_solve_gcf_nearest<false>");
  }
  return hipGetLastError();
}

}  // namespace ibs
