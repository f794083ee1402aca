// Geometry-fed points with the EXACT gradient of gam in BOTH variables, FP64, every odd N in [66, 65,537]: k_exact_points
// (ibs_exact_grad.hip) with the alpha-derivative of the rows taken from the alpha-tangent of the geometry
// (ibs_fieldline_geometry_dalpha_f64) in place of the reference's difference of two side lines over del_alpha (utils.py:1641-1646 /
// 1683-1718): ONE field line per point.  Stages 1-2 are the per-line functions of ibs_geo_line.hpp, stages 3, 4 and 6 the functions of
// ibs_exact_stages.hpp that k_exact_points calls too; only the lines read and the contraction (5) are this kernel's own.
// k_exact_tangent_points<NEAREST>, per point p (geo and geo_da in the [8][n_pts][ld] layout of the two geometry calls):
//   1. dPdrho      of the line, -1/2 mean((cvdrift - gbdrift) bmag^2) as a wave reduction (ball_scan.py:262); it has no alpha-tangent
//   2. rows        theta0 folded into the line and its (g, c, f) rows written to the wave's workspace
//   3. eigenpair   NEAREST: solve_nearest_one at sigma[p]; else lam_max as k_solve_gcf_long takes it
//   4. adjoint     vjp_one with gam_bar = 1, lam_bar = 0: g_bar, c_bar, f_bar in the workspace            (1-4: as k_exact_points)
//   5. contraction jac_theta0 = S(g_bar g_t + c_bar c_t + f_bar f_t) as k_exact_points; jac_alpha = S(g_bar g_a + c_bar c_a + f_bar f_a)
//                  with the tangent rows of line_gcf_tangent, formed from the two plane sets as they are summed
//   6. outputs     val = -gam, jac = (-dgam/dalpha, -dgam/dtheta0) (utils.py:1728); optional gam, lam, idx, info
// No floating-point atomics; every sum has a fixed order (lane-strided partial sums, then the DPP reduction).  Status word and
// workspace (exact_points_ws) as k_exact_points.  A non-finite entry of geo_da reaches jac[.][0] alone.
#include "ibs_exact_stages.hpp"
#include "ibs_geo_line.hpp"

namespace ibs {

template <bool NEAREST>
__global__ void __launch_bounds__(64) k_exact_tangent_points(const ExactPointsArgs a) {
  __shared__ double lds[3 * kLongChunk];                    // (the LDS budget of the long path: static_assert at kLongChunk)
  static_assert(sizeof(lds) * 8 <= 160 * 1024, "eight blocks per CU");
  const int lane = threadIdx.x & 63;
  const int N = a.N;
  const ExactPointsWs L = exact_points_ws(N);
  double* my = a.work + (size_t)blockIdx.x * L.total;
  double* G = my + L.g; double* C = my + L.c; double* F = my + L.f;
  const double* gb = my + L.gb; const double* cb = my + L.cb; const double* fb = my + L.fb;
  const long plane = (long)a.n_pts * a.ld;
  for (long p = blockIdx.x; p < a.n_pts; p += gridDim.x) {
    const double th0 = uniform(a.theta0[p]);
    const GeoLine ln{a.geo + (size_t)p * a.ld, plane}, lt{a.geo_da + (size_t)p * a.ld, plane};
    // ---- 1. dPdrho of the line
    double mdP;                                             // -dPdrho
    line_mdP<1>(&ln, N, lane, &mdP);
    // ---- 2. the line's rows
    for (int j = lane; j < N; j += kWave) {
      double g, c, f;
      line_gcf(ln, j, mdP, th0, g, c, f);
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
        double gt, ct, ft;                                  // theta0 tangent of the line
        line_gcf_dtheta0(ln, j, mdP, th0, gt, ct, ft);
        double ga, ca, fa;                                  // alpha tangent: the derivative of the rows, dPdrho fixed
        line_gcf_tangent(ln, lt, j, mdP, th0, ga, ca, fa);
        st += gbj * gt + cbj * ct + fbj * ft;
        sa += gbj * ga + cbj * ca + fbj * fa;
      }
      jt = wave_sum(st);
      ja = wave_sum(sa);
    }
    // ---- 6. utils.py:1728
    if (lane == 0) exact_store<NEAREST>(a, p, e, ja, jt);
    long_fence();                                           // (the workspace is reused by this wave's next point)
  }
}

hipError_t launch_obj_w_grad_exact_tangent(const ExactPointsArgs& a, hipStream_t st) {
  if (a.n_pts <= 0) return hipSuccess;
  const long grid = persistent_grid(a.n_pts, a.n_waves, a.work, a.work_doubles, exact_points_ws(a.N).total);
  if (!grid || !a.geo || !a.geo_da || !a.theta0 || !a.val || !a.jac) return hipErrorInvalidValue;
  if (a.sigma) {
    hipLaunchKernelGGL(k_exact_tangent_points<true>, dim3((unsigned)grid), dim3(64), 0, st, a);
    note_launch(grid, 64, "ibs::k_exact_tangent_points<true>");
  } else {
    hipLaunchKernelGGL(k_exact_tangent_points<false>, dim3((unsigned)grid), dim3(64), 0, st, a);
    note_launch(grid, 64, "ibs::k_exact_tangent_points<false>");
  }
  return hipGetLastError();
}

}  // namespace ibs
