// Geometry-fed points with the EXACT gradient of gam, FP64, every odd N in [66, 65,537]: the batched form of the reference's objective
// (utils.py:1632-1728) with the derivative of the gam it returns in place of the Hellmann-Feynman formulas (utils.py:1676-1680,
// 1721-1725), which put gam in place of lam.  One wavefront per point on the persistent grid of the long path (long_waves()), the
// pieces of ibs_long.hpp / ibs_nearest.hpp / ibs_vjp.hpp.  k_exact_points<NEAREST>, per point p:
//   1. dPdrho      of each of the three lines (alpha - d/2, alpha, alpha + d/2), -1/2 mean((cvdrift - gbdrift) bmag^2) as a wave
//                  reduction (ball_scan.py:262, utils.py:1657, 1691, 1703)
//   2. rows        theta0 folded into the centre line and its (g, c, f) rows written to the wave's workspace (utils.py:1659-1660,
//                  1560-1562); the half-grid g is the mean of neighbouring values          (1-2: as k_nearest_points<true>)
//   3. eigenpair   NEAREST: solve_nearest_one at sigma[p] (utils.py:1597); else lam_max as k_solve_gcf_long takes it (long_bounds,
//                  long_lam_max, long_vector_growth).  X stays in the workspace
//   4. adjoint     vjp_one with gam_bar = 1, lam_bar = 0 on those rows and that pair: g_bar, c_bar, f_bar = d gam / d (g, c, f) in the
//                  workspace (g_bar and c_bar in the adjoint's own first two work rows, dead by then)
//   5. contraction jac_theta0 = S(g_bar g_t + c_bar c_t + f_bar f_t) with the theta0 tangent of the centre line (utils.py:1669-1673),
//                  jac_alpha = S(g_bar (g_r - g_l) + c_bar (c_r - c_l) + f_bar (f_r - f_l)) / del_alpha with each side line's own dPdrho
//                  (utils.py:1683-1718).  The tangents are formed from the geometry as they are summed, never written out
//   6. outputs     val = -gam, jac = (-dgam/dalpha, -dgam/dtheta0) (utils.py:1728); optional gam, lam, idx, info
// No floating-point atomics; every sum has a fixed order (lane-strided partial sums, then the DPP reduction): results are bitwise
// repeatable and the same whatever the batch.  info = the solve's word (bits 0-15 passes, status from bit 16) with the adjoint's two
// flags at status bits 6 (a replaced pivot: informational) and 7 (refused: jac = NaN, val kept).  A failed solve (status bits 0-1)
// gives val = jac = NaN.  Per-wave workspace: exact_points_ws(N) (ibs_launch.hpp), in global memory.
// Stages 1, 2 and the tangents of 5 are the per-line functions of ibs_geo_line.hpp (line_mdP, line_gcf, line_gcf_dtheta0); stages 3, 4
// and 6 are exact_eigenpair, exact_adjoint and exact_store of ibs_exact_stages.hpp, shared with k_exact_tangent_points.
#include "ibs_exact_stages.hpp"
#include "ibs_geo_line.hpp"

namespace ibs {

template <bool NEAREST>
__global__ void __launch_bounds__(64) k_exact_points(const ExactPointsArgs a) {
  __shared__ double lds[3 * kLongChunk];                    // (the LDS budget of the long path: static_assert at kLongChunk)
  static_assert(sizeof(lds) * 8 <= 160 * 1024, "eight blocks per CU");
  const int lane = threadIdx.x & 63;
  const int N = a.N;
  const ExactPointsWs L = exact_points_ws(N);
  double* my = a.work + (size_t)blockIdx.x * L.total;
  double* G = my + L.g; double* C = my + L.c; double* F = my + L.f;
  const double* gb = my + L.gb; const double* cb = my + L.cb; const double* fb = my + L.fb;
  for (long p = blockIdx.x; p < a.n_pts; p += gridDim.x) {
    const double th0 = uniform(a.theta0[p]);
    // ---- 1. dPdrho of the three lines
    GeoLine ln[3];
    double mdP[3];                                          // -dPdrho
#pragma unroll
    for (int l = 0; l < 3; ++l) ln[l] = GeoLine{a.geo + ((size_t)p * 3 + l) * 8 * (size_t)a.ld, a.ld};
    line_mdP<3>(ln, N, lane, mdP);
    // ---- 2. the centre line's rows
    for (int j = lane; j < N; j += kWave) {
      double g, c, f;
      line_gcf(ln[1], j, mdP[1], th0, g, c, f);
      G[j] = g; C[j] = c; F[j] = f;
    }
    long_fence();                                           // (rows written by every lane, read by every lane below)
    const SrcLong<double, false> src{G, C, F, nullptr};
    // ---- 3. the eigenpair, 4. d gam / d (g, c, f)
    ExactPair e = exact_eigenpair<NEAREST>(src, a, p, my, L, lds, lane);
    double ja = __builtin_nan(""), jt = __builtin_nan("");
    if (((e.word >> 16) & 3) == 0 && (exact_adjoint(src, a, e, my, L, lds, lane) & 2) == 0) {
      // ---- 5. contraction with the theta0 and alpha tangents
      double st = 0.0, sa = 0.0;
      for (int j = lane; j < N; j += kWave) {
        const double gbj = gb[j], cbj = cb[j], fbj = fb[j];
        double gt, ct, ft;                                  // theta0 tangent of the centre line
        line_gcf_dtheta0(ln[1], j, mdP[1], th0, gt, ct, ft);
        // alpha tangent (utils.py:1705-1719): each side line with its own dPdrho
        double gl, cl, fl, gr, cr, fr;
        line_gcf(ln[0], j, mdP[0], th0, gl, cl, fl);
        line_gcf(ln[2], j, mdP[2], th0, gr, cr, fr);
        st += gbj * gt + cbj * ct + fbj * ft;
        sa += gbj * (gr - gl) + cbj * (cr - cl) + fbj * (fr - fl);
      }
      jt = wave_sum(st);
      ja = wave_sum(sa) / a.del_alpha;
    }
    // ---- 6. utils.py:1728
    if (lane == 0) exact_store<NEAREST>(a, p, e, ja, jt);
    long_fence();                                           // (the workspace is reused by this wave's next point)
  }
}

hipError_t launch_obj_w_grad_exact(const ExactPointsArgs& a, hipStream_t st) {
  if (a.n_pts <= 0) return hipSuccess;
  const long grid = persistent_grid(a.n_pts, a.n_waves, a.work, a.work_doubles, exact_points_ws(a.N).total);
  if (!grid || !a.geo || !a.theta0 || !a.val || !a.jac) return hipErrorInvalidValue;
  if (a.sigma) {
    hipLaunchKernelGGL(k_exact_points<true>, dim3((unsigned)grid), dim3(64), 0, st, a);
    note_launch(grid, 64, "ibs::k_exact_points<true>");
  } else {
    hipLaunchKernelGGL(k_exact_points<false>, dim3((unsigned)grid), dim3(64), 0, st, a);
    note_launch(grid, 64, "ibs::k_exact_points<false>");
  }
  return hipGetLastError();
}

}  // namespace ibs
