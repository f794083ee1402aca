// Geometry-fed points with the eigenpair NEAREST sigma[p] (utils.py:1597), FP64, every odd N in [66, 65,537]: the batched forms of the
// reference's objective with its Hellmann-Feynman gradient (utils.py:1632-1728, the refinement of ball_scan.py:305-314, shift
// 1.3 |gam| + 0.05) and of its final solve (ball_scan.py:322-339, shift 0.42).  One wavefront per point on the persistent grid of the
// long path (long_waves()), the pieces of ibs_long.hpp / ibs_nearest.hpp.  k_nearest_points<GRAD>, per point p:
//   1. dPdrho      GRAD: of each of the three lines (alpha - d/2, alpha, alpha + d/2), -1/2 mean((cvdrift - gbdrift) bmag^2) as a
//                  wave reduction (ball_scan.py:262, utils.py:1657, 1691, 1703); else dPdrho[p] is given, as in ibs_gamma_points_f64
//   2. rows        theta0 folded into the centre line and its (g, c, f) rows written to the wave's workspace (utils.py:1659-1660,
//                  1560-1562; the expressions of k_assemble_gcf_long); the half-grid g is the mean of neighbouring values
//   3. eigenpair   solve_nearest_one: k = 0 path, tie rule (status bit 5), X scaled so that its largest-magnitude entry is +1
//   4. gradient    GRAD: both Hellmann-Feynman derivatives in one more pass over the rows (utils.py:1666-1680, 1683-1725),
//                  (S(c_p X^2) - S(g_p dX^2) - gam S(f_p X^2)) / S(f X^2) with composite Simpson; the theta0 tangent from the centre
//                  line's cvdrift0 / gds21 / gds22, the alpha tangent (right - left) / del_alpha with each side line's own dPdrho.  The
//                  tangents are formed from the geometry as they are summed, never written out
//   5. outputs     GRAD: val = -gam, jac = (-dgam/dalpha, -dgam/dtheta0) (utils.py:1728); else gam (and X, dX) as the solve gives them
// Per-wave workspace: nearest_points_ws(N, GRAD) (ibs_launch.hpp), in global memory.  dPdrho, the rows and their theta0 tangent are
// the per-line functions of ibs_geo_line.hpp (line_mdP, line_gcf on either layout, line_gcf_dtheta0).
#include "ibs_nearest.hpp"
#include "ibs_geo_line.hpp"
#include "ibs_launch.hpp"

namespace ibs {

template <bool GRAD>
__global__ void __launch_bounds__(64) k_nearest_points(const NearestPointsArgs a) {
  __shared__ double lds[3 * kLongChunk];                    // (the LDS budget of the long path: static_assert at kLongChunk)
  static_assert(sizeof(lds) * 8 <= 160 * 1024, "eight blocks per CU");
  const int lane = threadIdx.x & 63;
  const int N = a.N;
  const NearestPointsWs L = nearest_points_ws(N, GRAD);
  double* my = a.work + (size_t)blockIdx.x * L.total;
  double* G = my + L.g; double* C = my + L.c; double* F = my + L.f;
  for (long p = blockIdx.x; p < a.n_pts; p += gridDim.x) {
    const double th0 = uniform(a.theta0[p]);
    GeoLine ln[3];
    double mdP[3];                                          // -dPdrho
    if constexpr (GRAD) {
      // ---- 1. dPdrho of the three lines
#pragma unroll
      for (int l = 0; l < 3; ++l) ln[l] = GeoLine{a.geo + ((size_t)p * 3 + l) * 8 * (size_t)a.ld, a.ld};
      line_mdP<3>(ln, N, lane, mdP);
    } else {
      mdP[1] = -uniform(a.dPdrho[p]);
    }
    // ---- 2. the centre line's rows
    const GeoLine7 l7 = geo_line7(a.geo7, p * a.ld);        // (the points form without GRAD)
    for (int j = lane; j < N; j += kWave) {
      double g, c, f;
      if constexpr (GRAD) line_gcf(ln[1], j, mdP[1], th0, g, c, f);
      else line_gcf(l7, j, mdP[1], th0, g, c, f);
      G[j] = g; C[j] = c; F[j] = f;
    }
    long_fence();                                           // (rows written by every lane, read by every lane below)
    const SrcLong<double, false> src{G, C, F, nullptr};
    // ---- 3. the eigenpair nearest sigma[p]
    if constexpr (GRAD) {
      double* Xw = my + L.X; double* dXw = my + L.dX;
      const double gam = solve_nearest_one<false>(src, N, a.h, a.sigma[p], 0, my + L.work, a.lam ? a.lam + p : nullptr,
                                                  a.idx ? a.idx + p : nullptr, nullptr, Xw, dXw, a.info ? a.info + p : nullptr, lds);
      long_fence();
      // ---- 4. Hellmann-Feynman derivatives (utils.py:1676-1680, 1721-1725; the sums of k_hf_grad)
      double ja = __builtin_nan(""), jt = __builtin_nan("");
      if (gam == gam) {
        const double inv_del = 1.0 / a.del_alpha;
        double y1 = 0.0, sct = 0.0, sgt = 0.0, sft = 0.0, sca = 0.0, sga = 0.0, sfa = 0.0;
        for (int j = lane; j < N; j += kWave) {
          const double w = (j == 0 || j == N - 1) ? 1.0 : ((j & 1) ? 4.0 : 2.0);
          const double x2 = w * Xw[j] * Xw[j], d2 = w * dXw[j] * dXw[j];
          double gt, ct, ft;                                // theta0 tangent of the centre line
          line_gcf_dtheta0(ln[1], j, mdP[1], th0, gt, ct, ft);
          // alpha tangent (utils.py:1705-1719): each side line with its own dPdrho
          double gl, cl, fl, gr, cr, fr;
          line_gcf(ln[0], j, mdP[0], th0, gl, cl, fl);
          line_gcf(ln[2], j, mdP[2], th0, gr, cr, fr);
          const double ga = (gr - gl) * inv_del, ca = (cr - cl) * inv_del, fa = (fr - fl) * inv_del;
          y1 += F[j] * x2;
          sct += ct * x2; sgt += gt * d2; sft += ft * x2;
          sca += ca * x2; sga += ga * d2; sfa += fa * x2;
        }
        y1 = wave_sum(y1);
        sct = wave_sum(sct); sgt = wave_sum(sgt); sft = wave_sum(sft);
        sca = wave_sum(sca); sga = wave_sum(sga); sfa = wave_sum(sfa);
        jt = sct / y1 - sgt / y1 - gam * sft / y1;
        ja = sca / y1 - sga / y1 - gam * sfa / y1;
      }
      // ---- 5. utils.py:1728
      if (lane == 0) {
        a.val[p] = -gam; a.jac[2 * p] = -ja; a.jac[2 * p + 1] = -jt;
        if (a.gam) a.gam[p] = gam;
      }
    } else {
      solve_nearest_one<false>(src, N, a.h, a.sigma[p], 0, my + L.work, a.lam ? a.lam + p : nullptr, a.idx ? a.idx + p : nullptr,
                               a.gam + p, a.X ? a.X + p * N : nullptr, a.dX ? a.dX + p * N : nullptr, a.info ? a.info + p : nullptr,
                               lds);
    }
    long_fence();                                           // (the workspace is reused by this wave's next point)
  }
}

static hipError_t launch_points(const NearestPointsArgs& a, bool grad, hipStream_t st) {
  if (a.n_pts <= 0) return hipSuccess;
  const long grid = persistent_grid(a.n_pts, a.n_waves, a.work, a.work_doubles, nearest_points_ws(a.N, grad).total);
  if (!grid) return hipErrorInvalidValue;
  if (grad) {
    if (!a.geo || !a.val || !a.jac) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_nearest_points<true>, dim3((unsigned)grid), dim3(64), 0, st, a);
    note_launch(grid, 64, "ibs::k_nearest_points<true>");
  } else {
    if (!a.dPdrho || !a.gam) return hipErrorInvalidValue;
    for (int k = 0; k < 7; ++k) if (!a.geo7[k]) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_nearest_points<false>, dim3((unsigned)grid), dim3(64), 0, st, a);
    note_launch(grid, 64, "ibs::k_nearest_points<false>");
  }
  return hipGetLastError();
}

hipError_t launch_obj_w_grad_nearest(const NearestPointsArgs& a, hipStream_t st) { return launch_points(a, true, st); }
hipError_t launch_points_nearest(const NearestPointsArgs& a, hipStream_t st) { return launch_points(a, false, st); }

}  // namespace ibs
