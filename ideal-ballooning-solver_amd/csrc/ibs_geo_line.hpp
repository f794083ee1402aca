// One field line of a geometry-fed system and the per-line stages every kernel that forms (g, c, f) rows from the geometry shares:
// dPdrho of a line, its rows at theta0, their theta0 tangent and their alpha tangent.  Each stage is written once, on a line accessor
// with at(k, j) = array k (bmag gradpar cvdrift cvdrift0 gds2 gds21 gds22 [gbdrift]) at grid point j, so that the kernels which must
// agree bitwise (the point kernels of ibs_nearest_grad / ibs_exact_grad / ibs_exact_tangent / ibs_marginal_points /
// ibs_marginal_tangent.hip, k_marginal_scan, k_geo_reclose, k_assemble_gcf_long) run the same expressions in the same order.
#pragma once
#include "ibs_wave.hpp"

namespace ibs {

// one field line of a point layout: array k at p + k * ld (eight arrays)
struct GeoLine {
  const double* p; long ld;
  __device__ __forceinline__ double at(int k, int j) const { return p[(long)k * ld + j]; }
};
// one field line of a scan layout: seven arrays held apart, the line at element off of each (no gbdrift: dPdrho is given)
struct GeoLine7 {
  const double* a[7]; long off;
  __device__ __forceinline__ double at(int k, int j) const { return a[k][off + j]; }
};
__device__ __forceinline__ GeoLine7 geo_line7(const double* const a[7], long off) {
  return GeoLine7{{a[0], a[1], a[2], a[3], a[4], a[5], a[6]}, off};
}
// -dPdrho of NL lines, 0.5 mean((cvdrift - gbdrift) bmag^2) (ball_scan.py:262, utils.py:1657, 1691, 1703): ONE lane-strided pass with
// the NL sums interleaved (all loads of a grid point in flight at once), then the wave reductions
template <int NL, class Line>
__device__ __forceinline__ void line_mdP(const Line* ln, int N, int lane, double* mdP) {
  double s[NL] = {};
  for (int j = lane; j < N; j += kWave) {
#pragma unroll
    for (int l = 0; l < NL; ++l) {
      const double B = ln[l].at(0, j);
      s[l] += (ln[l].at(2, j) - ln[l].at(7, j)) * B * B;
    }
  }
#pragma unroll
  for (int l = 0; l < NL; ++l) mdP[l] = 0.5 * wave_sum(s[l]) / (double)N;
}
// (g, c, f) of a line at theta0 (ball_scan.py:267-268, utils.py:1560-1562; the expressions of the scan kernels' staging, SrcGeo)
template <class Line>
__device__ __forceinline__ void line_gcf(const Line& L, int j, double mdP, double th0, double& g, double& c, double& f) {
  const double B = L.at(0, j), gp = xabs(L.at(1, j));
  const double inv = 1.0 / (gp * B);
  const double A1 = gp / B, A3 = inv / (B * B);
  const double C0 = mdP * L.at(2, j) * inv, C1 = mdP * L.at(3, j) * inv;
  const double d = L.at(4, j) + (2.0 * th0) * L.at(5, j) + (th0 * th0) * L.at(6, j);
  g = A1 * d; c = C0 + th0 * C1; f = A3 * d;
}
// theta0 tangent (gt, ct, ft) of those rows (utils.py:1669-1673)
template <class Line>
__device__ __forceinline__ void line_gcf_dtheta0(const Line& L, int j, double mdP, double th0, double& gt, double& ct, double& ft) {
  const double B = L.at(0, j), gp = xabs(L.at(1, j));
  const double inv = 1.0 / (gp * B);
  const double A1 = gp / B, A3 = inv / (B * B);
  const double dp = 2.0 * L.at(5, j) + (2.0 * th0) * L.at(6, j);
  gt = A1 * dp; ct = mdP * L.at(3, j) * inv; ft = A3 * dp;
}
// the margin kernels have no use for f: its chain is dead code there
template <class Line>
__device__ __forceinline__ void line_gcf(const Line& L, int j, double mdP, double th0, double& g, double& c) {
  double f;
  line_gcf(L, j, mdP, th0, g, c, f);
}
template <class Line>
__device__ __forceinline__ void line_gcf_dtheta0(const Line& L, int j, double mdP, double th0, double& gt, double& ct) {
  double ft;
  line_gcf_dtheta0(L, j, mdP, th0, gt, ct, ft);
}
// alpha-tangent of those rows: L the line, T the alpha-derivative of its eight arrays (ibs_fieldline_geometry_dalpha_f64), dPdrho
// held fixed (a surface constant: (cvdrift - gbdrift) bmag^2 does not depend on alpha); d|gradpar| = sgn(gradpar) d gradpar
__device__ __forceinline__ void line_gcf_tangent(const GeoLine& L, const GeoLine& T, int j, double mdP, double th0, double& ga,
                                                 double& ca, double& fa) {
  const double B = L.at(0, j), gpr = L.at(1, j), gp = xabs(gpr);
  const double dB = T.at(0, j), dgp = gpr > 0.0 ? T.at(1, j) : (gpr < 0.0 ? -T.at(1, j) : 0.0 * T.at(1, j));
  const double iBv = 1.0 / B;
  const double inv = 1.0 / (gp * B), dinv = -inv * inv * (dgp * B + gp * dB);
  const double A1 = gp * iBv, dA1 = (dgp - A1 * dB) * iBv;
  const double A3 = inv * iBv * iBv, dA3 = (dinv - 2.0 * inv * dB * iBv) * iBv * iBv;
  const double dC0 = mdP * (T.at(2, j) * inv + L.at(2, j) * dinv), dC1 = mdP * (T.at(3, j) * inv + L.at(3, j) * dinv);
  const double d = L.at(4, j) + (2.0 * th0) * L.at(5, j) + (th0 * th0) * L.at(6, j);
  const double dd = T.at(4, j) + (2.0 * th0) * T.at(5, j) + (th0 * th0) * T.at(6, j);
  ga = dA1 * d + A1 * dd; ca = dC0 + th0 * dC1; fa = dA3 * d + A3 * dd;
}

}  // namespace ibs
