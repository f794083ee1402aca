// Exact vector-Jacobian product of the growth rate gam (the FD4 / Simpson quotient of utils.py:1601-1621) and of the eigenvalue lam
// with respect to the (g, c, f) rows of a system: given a simple eigenpair (lam, X) of the pencil of utils.py:1574-1592 and the
// cotangents gam_bar, lam_bar, the rows g_bar, c_bar, f_bar (length N).  Every odd N in [66, 65,537], FP64, one wavefront per system on
// the persistent grid of the long path (long_waves()), the rows read from memory.  Uniform grid, half-grid g = mean of neighbours.
//   A. 64 lanes     dX = D X (the stencils of utils.py:1610-1616), P = S(c X^2 - g dX^2), Q1 = S(f X^2) (S: composite Simpson),
//                   gam = P / Q1, Q = X^T F X, the row k of largest |X|, and the residual max_r |((S - lam F) X)_r| / f_r.  A pair that
//                   is not an eigenpair of these rows (residual above kVjpResTol N eps (||A|| + |lam|) max |X|), invalid data
//                   (non-finite, g <= 0, f <= 0) or a non-finite lam / X / cotangent gives status bit 1 and NaN rows.
//                   Then r = d gam / d X = (2 / Q1) [D^T (-w g dX) + w c X - gam w f X] on the interior (X^T r = 0).
//   B. lanes 0, 1   (S - lam F) z = r, singular with null vector X, by the twisted split at k: z_k = 0, equation k dropped; the
//                   leading block (rows < k) factors with the forward pivots D+ (lane 0), the trailing block (rows > k) with the
//                   backward pivots D- (lane 1) -- the recurrences of long_vector_growth's pivots, the rows passed through LDS in
//                   chunks.  A pivot below pivmin is replaced by -pivmin (as in count_above_chunked) and sets status bit 0.
//                   Skipped where gam_bar = 0 (z = 0).
//   C. 64 lanes     z^ = z - (z^T F X / Q) X; gh_bar_j = gam_bar (z^_{j+1} - z^_j)(X_{j+1} - X_j) / h^2 - lam_bar (X_{j+1} - X_j)^2 /
//                   (h^2 Q), c_bar = gam_bar (w X^2 / Q1 - z^ X) + lam_bar X^2 / Q, f_bar = gam_bar (-gam w X^2 / Q1 + lam z^ X) -
//                   lam_bar lam X^2 / Q, g_bar = -gam_bar w dX^2 / Q1 + (gh_bar_{j-1} + gh_bar_j) / 2.
// No floating-point atomics; every sum has a fixed order (lane-strided partial sums, then the DPP reduction): the rows are bitwise
// repeatable and the same whatever the batch.  Per-wave workspace: vjp_ws_doubles(N) (ibs_launch.hpp) in global memory.
// Stages A-C are vjp_one (ibs_vjp.hpp), shared with the geometry-fed point kernel of ibs_exact_grad.hip.
#include "ibs_vjp.hpp"
#include "ibs_launch.hpp"

namespace ibs {

__global__ void __launch_bounds__(64) k_solve_gcf_vjp(const VjpArgs a) {
  __shared__ double lds[3 * kLongChunk];                  // (the LDS budget of the long path: static_assert at kLongChunk)
  static_assert(sizeof(lds) * 8 <= 160 * 1024, "eight blocks per CU");
  const int lane = threadIdx.x & 63;
  double* my = a.work + (size_t)blockIdx.x * vjp_ws_doubles(a.N);
  for (long sys = blockIdx.x; sys < a.n_sys; sys += gridDim.x) {
    const long o = sys * a.ld;
    const SrcLong<double, false> src{a.g + o, a.c + o, a.f + o, nullptr};
    const double gbar = a.gam_bar ? uniform(a.gam_bar[sys]) : 0.0, lbar = a.lam_bar ? uniform(a.lam_bar[sys]) : 0.0;
    vjp_one(src, a.N, a.h, uniform(a.lam[sys]), a.X + o, gbar, lbar, a.g_bar + o, a.c_bar + o, a.f_bar + o, a.info, sys, my, lds, lane);
    long_fence();                                         // (the workspace is reused by this wave's next system)
  }
}

hipError_t launch_gcf_vjp(const VjpArgs& a, hipStream_t st) {
  if (a.n_sys <= 0) return hipSuccess;
  const long grid = persistent_grid(a.n_sys, a.n_waves, a.work, a.work_doubles, vjp_ws_doubles(a.N));
  if (!grid) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_solve_gcf_vjp, dim3((unsigned)grid), dim3(64), 0, st, a);
  note_launch(grid, 64, "ibs::k_solve_gcf_vjp");
  return hipGetLastError();
}

}  // namespace ibs
