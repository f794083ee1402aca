// Marginal stability at geometry-fed points with the EXACT gradient of s* in (alpha, theta0) and its cotangent planes: k_marginal_points
// (ibs_marginal_points.hip) with the alpha-derivative of the rows taken from the alpha-tangent of the geometry
// (ibs_fieldline_geometry_dalpha_f64) in place of the del_alpha difference of two side lines (utils.py:1683-1718): ONE field line per
// point, on the data layout of k_exact_tangent_points (ibs_exact_tangent.hip).  Stages 1, 2, the theta0 part of 4 and 6 are the
// functions k_marginal_points calls too: line_mdP, line_gcf, line_gcf_dtheta0 (ibs_geo_line.hpp), pencil_weight, marginal_store
// (ibs_marginal.hpp).  FP64, every odd N in [66, 65,537], one wavefront per point on the persistent grid of the
// long path, division form throughout; per-wave workspace marginal_ws(N, true).
// Per point p (geo and geo_da in the [8][n_pts][ld] layout of the two geometry calls) and theta0[p]:
//   1. dPdrho      of the line, -1/2 mean((cvdrift - gbdrift) bmag^2) as a wave reduction (the centre line's sum of k_marginal_points)
//   2. rows        the line's (g, c) at theta0 in the wave's workspace: line_gcf, as k_marginal_scan
//   3. s*          marginal_one: s*, status, passes and, with a gradient or geo_bar, the marginal mode X
//   4. gradient    Hellmann-Feynman on the discrete pencil, q = sum c_j X_j^2, w_j = (X_j - X_{j-1})^2 + (X_{j+1} - X_j)^2:
//                  d s* / d theta0 as k_marginal_points (the same sums in the same order);
//                  d s* / d alpha = (1/2 h^-2 sum g_a,j w_j - s* sum c_a,j X_j^2) / q with (g_a, c_a) of line_gcf_tangent (dPdrho held
//                  fixed, d|gradpar| = sgn(gradpar) d gradpar); the tangents are formed as they are summed; f plays no part
//   5. geo_bar     d s* / d (every entry of the eight arrays read), the dependence through the line's own dPdrho included, in closed
//                  form per grid point from g_bar_j = 1/2 h^-2 w_j / q and c_bar_j = -s* X_j^2 / q; sum c_bar_j c_j = -s*, so
//                  d s* / d m = -s* / m for m = -dPdrho and no further reduction is needed.  With a = |gradpar|, B = bmag, k = -s* / m:
//                    bmag     -g_bar g / B - c_bar c / B + k B (cvdrift - gbdrift) / N      gradpar  sgn(gradpar) (g_bar g - c_bar c) / a
//                    cvdrift  c_bar m / (a B) + k B^2 / (2 N)                               cvdrift0 theta0 c_bar m / (a B)
//                    gds2     g_bar a / B        gds21  2 theta0 g_bar a / B                gds22    theta0^2 g_bar a / B
//                    gbdrift  -k B^2 / (2 N)
//                  Each lane writes its own points j = lane, lane + 64, ... with vector stores; entries N .. ld-1 are never written.
//   6. outputs     as k_marginal_points: val = -1 / s*, jac = dscale / s*^2, scale, dscale, dPdrho.  Status bits 0-1 of the solve: every
//                  floating-point output NaN, the geo_bar rows included; bit 8: scale = +inf, val = 0, jac = dscale = 0, zero geo_bar
//                  rows; a gradient that is not finite after a good solve (invalid data in geo_da): status bit 1, jac = dscale = NaN,
//                  val, scale and geo_bar kept.  With jac, dscale and geo_bar all null no mode is formed (the point-evaluation form).
// No floating-point atomics; every sum has a fixed order (lane-strided partial sums, then the DPP reduction): results are bitwise
// repeatable and the same whatever the batch.  info = bits 0-15 multisection passes, status from bit 16 (include/ibs.h).
#include "ibs_marginal.hpp"
#include "ibs_geo_line.hpp"
#include "ibs_launch.hpp"

namespace ibs {

__global__ void __launch_bounds__(64) k_marginal_tangent_points(const MarginalTangentArgs a) {
  __shared__ double lds[3 * kLongChunk];
  static_assert(sizeof(lds) * 8 <= 160 * 1024, "eight blocks per CU");
  const int lane = threadIdx.x & 63;
  const int N = a.N;
  const MarginalWs L = marginal_ws(N, true);
  double* my = a.work + (size_t)blockIdx.x * L.total;
  double* Xw = my + L.X; double* G = my + L.g; double* C = my + L.c;
  const bool want_grad = a.jac || a.dscale;                 // (kernel-uniform)
  const bool want_mode = want_grad || a.geo_bar;
  const double ih2 = 1.0 / (a.h * a.h);
  const long plane = (long)a.n_pts * a.ld, plane_bar = (long)a.n_pts * a.ld_bar;
  for (long p = blockIdx.x; p < a.n_pts; p += gridDim.x) {
    const double th0 = uniform(a.theta0[p]);
    const GeoLine ln{a.geo + (size_t)p * a.ld, plane};
    // ---- 1. dPdrho of the line
    double mdP;                                             // -dPdrho
    line_mdP<1>(&ln, N, lane, &mdP);
    // ---- 2. the line's rows at theta0
    for (int j = lane; j < N; j += kWave) line_gcf(ln, j, mdP, th0, G[j], C[j]);
    long_fence();                                           // (rows written by every lane, read by every lane below)
    // ---- 3. s* and the marginal mode
    int status, passes;
    double gam0;
    double s = marginal_one(G, C, N, a.h, my + L.work, Xw, want_mode, lds, status, passes, gam0);
    const bool failed = s != s || (status & 1);             // (the solve: iteration cap or invalid data; wave-uniform)
    // ---- 4. the gradient
    const double fill = (status & 256) ? 0.0 : __builtin_nan("");
    double dal = fill, dth = fill, q = 0.0;
    if (want_mode && status == 0) {
      double sg = 0.0, sc = 0.0, ag = 0.0, ac = 0.0;
      if (want_grad) {
        const GeoLine lt{a.geo_da + (size_t)p * a.ld, plane};
        for (int j = lane; j < N; j += kWave) {
          const double x0 = Xw[j], x2 = x0 * x0, w = pencil_weight(Xw, j, N);
          double gt, ct;                                    // theta0 tangent of the line
          line_gcf_dtheta0(ln, j, mdP, th0, gt, ct);
          q = xfma(C[j], x2, q);
          sg = xfma(gt, w, sg);
          sc = xfma(ct, x2, sc);
          // alpha tangent: the derivative of the rows, dPdrho fixed
          double ga, ca, fa;
          line_gcf_tangent(ln, lt, j, mdP, th0, ga, ca, fa);
          ag = xfma(ga, w, ag);
          ac = xfma(ca, x2, ac);
        }
        q = wave_sum(q); sg = wave_sum(sg); sc = wave_sum(sc); ag = wave_sum(ag); ac = wave_sum(ac);
        dth = (0.5 * ih2 * sg - s * sc) / q;
        dal = (0.5 * ih2 * ag - s * ac) / q;
        if (!(finite_of(dth) && finite_of(dal))) {          // (invalid data in geo_da: val, scale and geo_bar stand)
          status |= 2;
          dth = dal = __builtin_nan("");
        }
      } else {
        for (int j = lane; j < N; j += kWave) {
          const double x0 = Xw[j];
          q = xfma(C[j], x0 * x0, q);
        }
        q = wave_sum(q);
      }
    }
    // ---- 5. the cotangent planes
    if (a.geo_bar) {
      double* gb = a.geo_bar + (size_t)p * a.ld_bar;
      if (failed || (status & 256)) {
        const double v = failed ? __builtin_nan("") : 0.0;
        for (int j = lane; j < N; j += kWave) {
#pragma unroll
          for (int k = 0; k < 8; ++k) gb[(long)k * plane_bar + j] = v;
        }
      } else {
        const double iq = 1.0 / q, kap = -s / mdP, iN = 1.0 / (double)N;
        for (int j = lane; j < N; j += kWave) {
          const double x0 = Xw[j], w = pencil_weight(Xw, j, N);
          const double gbar = 0.5 * ih2 * w * iq, cbar = -s * (x0 * x0) * iq;
          const double B = ln.at(0, j), gpr = ln.at(1, j), gp = xabs(gpr);
          const double iB = 1.0 / B, ia = 1.0 / gp;
          const double g = G[j], c = C[j];
          const double cv = ln.at(2, j), gbd = ln.at(7, j);
          const double gA = gbar * gp * iB;                 // g_bar a / B
          const double cM = cbar * mdP * ia * iB;           // c_bar m / (a B)
          const double kB2 = 0.5 * kap * B * B * iN;        // k B^2 / (2 N)
          const double gg = gbar * g, cc = cbar * c;
          const double dgp = (gg - cc) * ia;
          gb[j] = -(gg + cc) * iB + kap * B * (cv - gbd) * iN;
          gb[1 * plane_bar + j] = gpr < 0.0 ? -dgp : dgp;
          gb[2 * plane_bar + j] = cM + kB2;
          gb[3 * plane_bar + j] = th0 * cM;
          gb[4 * plane_bar + j] = gA;
          gb[5 * plane_bar + j] = (2.0 * th0) * gA;
          gb[6 * plane_bar + j] = (th0 * th0) * gA;
          gb[7 * plane_bar + j] = -kB2;
        }
      }
    }
    // ---- 6. outputs
    if (lane == 0) marginal_store(a, p, s, status, passes, dal, dth, mdP);
    long_fence();                                           // (the workspace is reused by this wave's next point)
  }
}

hipError_t launch_marginal_tangent_points(const MarginalTangentArgs& a, hipStream_t st) {
  if (a.n_pts <= 0) return hipSuccess;
  const long grid = persistent_grid(a.n_pts, a.n_waves, a.work, a.work_doubles, marginal_ws(a.N, true).total);
  if (!grid || !a.geo || !a.theta0 || !a.val) return hipErrorInvalidValue;
  if (((a.jac || a.dscale) && !a.geo_da) || a.ld < a.N || (a.geo_bar && a.ld_bar < a.N)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_marginal_tangent_points, dim3((unsigned)grid), dim3(64), 0, st, a);
  note_launch(grid, 64, "ibs::k_marginal_tangent_points");
  return hipGetLastError();
}

}  // namespace ibs
