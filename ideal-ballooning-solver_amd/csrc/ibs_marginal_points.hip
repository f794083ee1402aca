// Marginal stability at geometry-fed points with the gradient of s* in (alpha, theta0): marginal_one (ibs_marginal.hpp, the stages listed
// in ibs_marginal.hip's header) on the three-line layout of k_exact_points (ibs_exact_grad.hip).  FP64, every odd N in [66, 65,537], one
// wavefront per point on the persistent grid of the long path, division form throughout; per-wave workspace marginal_ws(N, true).
// k_marginal_points is the objective of the refinement of the margin in (alpha, theta0).
// Per point p with geo[p][3][8][ld] (lines alpha - d/2, alpha, alpha + d/2) and theta0[p]:
//   1. dPdrho      of the lines, -1/2 mean((cvdrift - gbdrift) bmag^2) as wave reductions (only the centre line without a gradient)
//   2. rows        the centre line's (g, c) at theta0 in the wave's workspace, the arithmetic of k_marginal_scan
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
    if (want_grad) {
      double s[3] = {0.0, 0.0, 0.0};
      for (int j = lane; j < N; j += kWave) {
#pragma unroll
        for (int l = 0; l < 3; ++l) {
          const double B = ln[l].at(0, j);
          s[l] += (ln[l].at(2, j) - ln[l].at(7, j)) * B * B;
        }
      }
#pragma unroll
      for (int l = 0; l < 3; ++l) mdP[l] = 0.5 * wave_sum(s[l]) / (double)N;
    } else {
      double s = 0.0;
      for (int j = lane; j < N; j += kWave) {
        const double B = ln[1].at(0, j);
        s += (ln[1].at(2, j) - ln[1].at(7, j)) * B * B;
      }
      mdP[1] = 0.5 * wave_sum(s) / (double)N;
    }
    const double mdPc = mdP[1];
    // ---- 2. the centre line's rows at theta0 (the arithmetic of k_marginal_scan)
    for (int j = lane; j < N; j += kWave) {
      const double B = ln[1].at(0, j), gp = xabs(ln[1].at(1, j));
      const double inv = 1.0 / (gp * B);
      const double A1 = gp / B;
      const double C0 = mdPc * ln[1].at(2, j) * inv, C1 = mdPc * ln[1].at(3, j) * inv;
      const double d = ln[1].at(4, j) + (2.0 * th0) * ln[1].at(5, j) + (th0 * th0) * ln[1].at(6, j);
      G[j] = A1 * d; C[j] = C0 + th0 * C1;
    }
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
        const double x0 = Xw[j], x2 = x0 * x0;
        const double dm = j > 0 ? x0 - Xw[j - 1] : 0.0, dp = j < N - 1 ? Xw[j + 1] - x0 : 0.0;
        const double w = xfma(dm, dm, dp * dp);
        // theta0 tangent of the centre line (utils.py:1669-1673)
        const double B = ln[1].at(0, j), gp = xabs(ln[1].at(1, j));
        const double gt = (gp / B) * (2.0 * ln[1].at(5, j) + (2.0 * th0) * ln[1].at(6, j));
        const double ct = mdPc * ln[1].at(3, j) * (1.0 / (gp * B));
        q = xfma(C[j], x2, q);
        sg = xfma(gt, w, sg);
        sc = xfma(ct, x2, sc);
        // alpha tangent (utils.py:1705-1719): each side line with its own dPdrho
        double gl, cl, fl, gr, cr, fr;
        line_gcf(ln[0], j, mdP[0], th0, gl, cl, fl);
        line_gcf(ln[2], j, mdP[2], th0, gr, cr, fr);
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
    if (lane == 0) {
      const bool failed = s != s || (status & 1);           // (the centre solve: iteration cap or invalid data)
      if (failed) s = __builtin_nan("");
      const double rs = 1.0 / s;                            // mu: 0 with s* = +inf
      a.val[p] = (status & 256) ? 0.0 : -rs;
      if (a.jac) { a.jac[2 * p] = dal * rs * rs; a.jac[2 * p + 1] = dth * rs * rs; }
      if (a.scale) a.scale[p] = s;
      if (a.dscale) { a.dscale[2 * p] = dal; a.dscale[2 * p + 1] = dth; }
      if (a.dPdrho) a.dPdrho[p] = failed ? __builtin_nan("") : -mdPc;
      if (a.info) a.info[p] = passes | (status << 16);
    }
    long_fence();                                           // (the workspace is reused by this wave's next point)
  }
}

hipError_t launch_marginal_points(const MarginalPointsArgs& a, hipStream_t st) {
  if (a.n_pts <= 0) return hipSuccess;
  const long grid = a.n_pts < a.n_waves ? a.n_pts : a.n_waves;
  if (grid < 1 || !a.geo || !a.theta0 || !a.val || !a.work || a.work_doubles < (size_t)grid * marginal_ws(a.N, true).total) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_marginal_points, dim3((unsigned)grid), dim3(64), 0, st, a);
  note_launch(grid, 64, "ibs::k_marginal_points");
  return hipGetLastError();
}

}  // namespace ibs
