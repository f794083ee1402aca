// Marginal stability at geometry-fed points with the gradient of s* in (alpha, theta0): marginal_one (ibs_marginal.hpp, the stages listed
// in ibs_marginal.hip's header) on the three-line layout of k_exact_points (ibs_exact_grad.hip).  FP64, every odd N in [66, 65,537], one
// wavefront per point on the persistent grid of the long path, division form throughout; per-wave workspace marginal_ws(N, true).
// k_marginal_points is the objective of the refinement of the margin in (alpha, theta0).
// Per point p with geo[p][3][8][ld] (lines alpha - d/2, alpha, alpha + d/2) and theta0[p]:
//   1. dPdrho      of the lines, -1/2 mean((cvdrift - gbdrift) bmag^2) as wave reductions (only the centre line without a gradient)
//   2. rows        the centre line's (g, c) at theta0 in the wave's workspace: line_gcf (ibs_geo_line.hpp), as k_marginal_scan
//   3. s*          marginal_one: s*, status, passes and, with a gradient, the marginal mode X
//   4. gradient    Hellmann-Feynman on the discrete pencil, q = sum c_j X_j^2, w_j = (X_j - X_{j-1})^2 + (X_{j+1} - X_j)^2:
//                  d s* / d theta0 = (1/2 h^-2 sum g_t,j w_j - s* sum c_t,j X_j^2) / q with the theta0 tangent of utils.py:1669-1673,
//                  d s* / d alpha = (1/2 h^-2 sum (g_r - g_l)_j w_j - s* sum (c_r - c_l)_j X_j^2) / (q del_alpha), each side line with
//                  its own dPdrho (utils.py:1683-1718); the tangents are formed as they are summed, never written out; f plays no part
//   5. outputs     val = -mu = -1 / s* (finite everywhere: 0 where no scale makes the line unstable), jac = -(d mu / d alpha,
//                  d mu / d theta0) = dscale / s*^2, scale, dscale, dPdrho of the centre line.  Status bits 0-1 of the centre solve:
//                  every output NaN; bit 8: scale = +inf, val = 0, jac = dscale = 0; a gradient that is not finite after a good
//                  centre solve (invalid data in a side line): status bit 1, jac = dscale = NaN, val and scale kept.
// No floating-point atomics; every sum has a fixed order (lane-strided partial sums, then the DPP reduction): results are bitwise
// repeatable and the same whatever the batch.  info = bits 0-15 multisection passes, status from bit 16 (include/ibs.h).
// Shared with k_marginal_tangent_points and k_marginal_scan: line_mdP, line_gcf, line_gcf_dtheta0 (ibs_geo_line.hpp), pencil_weight and
// marginal_store (ibs_marginal.hpp).  The loop of 4 stays written out: it is one pass over the alpha sums as well.
#include "ibs_marginal.hpp"
#include "ibs_geo_line.hpp"
#include "ibs_launch.hpp"

namespace ibs {

__global__ void __launch_bounds__(64) k_marginal_points(const MarginalPointsArgs a) {
  __shared__ double lds[3 * kLongChunk];
  static_assert(sizeof(lds) * 8 <= 160 * 1024, "eight blocks per CU");
  const int lane = threadIdx.x & 63;
  const int N = a.N;
  const MarginalWs L = marginal_ws(N, true);
  double* my = a.work + (size_t)blockIdx.x * L.total;
  double* Xw = my + L.X; double* G = my + L.g; double* C = my + L.c;
  const bool want_grad = a.jac || a.dscale;                 // (kernel-uniform)
  const double ih2 = 1.0 / (a.h * a.h);
  for (long p = blockIdx.x; p < a.n_pts; p += gridDim.x) {
    const double th0 = uniform(a.theta0[p]);
    // ---- 1. dPdrho of the lines (as k_exact_points; the side lines are read only for a gradient)
    GeoLine ln[3];
    double mdP[3] = {0.0, 0.0, 0.0};                        // -dPdrho
#pragma unroll
    for (int l = 0; l < 3; ++l) ln[l] = GeoLine{a.geo + ((size_t)p * 3 + l) * 8 * (size_t)a.ld, a.ld};
    if (want_grad) line_mdP<3>(ln, N, lane, mdP);
    else line_mdP<1>(ln + 1, N, lane, mdP + 1);
    const double mdPc = mdP[1];
    // ---- 2. the centre line's rows at theta0
    for (int j = lane; j < N; j += kWave) line_gcf(ln[1], j, mdPc, th0, G[j], C[j]);
    long_fence();                                           // (rows written by every lane, read by every lane below)
    // ---- 3. s* and the marginal mode
    int status, passes;
    double gam0;
    double s = marginal_one(G, C, N, a.h, my + L.work, Xw, want_grad, lds, status, passes, gam0);
    // ---- 4. the gradient
    const double fill = (status & 256) ? 0.0 : __builtin_nan("");
    double dal = fill, dth = fill;
    if (want_grad && status == 0) {
      double q = 0.0, sg = 0.0, sc = 0.0, ag = 0.0, ac = 0.0;
      for (int j = lane; j < N; j += kWave) {
        const double x0 = Xw[j], x2 = x0 * x0, w = pencil_weight(Xw, j, N);
        double gt, ct;                                      // theta0 tangent of the centre line
        line_gcf_dtheta0(ln[1], j, mdPc, th0, gt, ct);
        q = xfma(C[j], x2, q);
        sg = xfma(gt, w, sg);
        sc = xfma(ct, x2, sc);
        // alpha tangent (utils.py:1705-1719): each side line with its own dPdrho
        double gl, cl, gr, cr;
        line_gcf(ln[0], j, mdP[0], th0, gl, cl);
        line_gcf(ln[2], j, mdP[2], th0, gr, cr);
        ag = xfma(gr - gl, w, ag);
        ac = xfma(cr - cl, x2, ac);
      }
      q = wave_sum(q); sg = wave_sum(sg); sc = wave_sum(sc); ag = wave_sum(ag); ac = wave_sum(ac);
      dth = (0.5 * ih2 * sg - s * sc) / q;
      dal = (0.5 * ih2 * ag - s * ac) / (q * a.del_alpha);
      if (!(finite_of(dth) && finite_of(dal))) {            // (invalid data in a side line: val and scale stand)
        status |= 2;
        dth = dal = __builtin_nan("");
      }
    }
    // ---- 5. outputs
    if (lane == 0) marginal_store(a, p, s, status, passes, dal, dth, mdPc);
    long_fence();                                           // (the workspace is reused by this wave's next point)
  }
}

hipError_t launch_marginal_points(const MarginalPointsArgs& a, hipStream_t st) {
  if (a.n_pts <= 0) return hipSuccess;
  const long grid = persistent_grid(a.n_pts, a.n_waves, a.work, a.work_doubles, marginal_ws(a.N, true).total);
  if (!grid || !a.geo || !a.theta0 || !a.val) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_marginal_points, dim3((unsigned)grid), dim3(64), 0, st, a);
  note_launch(grid, 64, "ibs::k_marginal_points");
  return hipGetLastError();
}

}  // namespace ibs
