// One field line of a geometry-fed point and its (g, c, f) rows at theta0: shared by the point kernels of ibs_nearest_grad.hip
// (Hellmann-Feynman gradient) and ibs_exact_grad.hip (exact gradient).
#pragma once
#include "ibs_wave.hpp"

namespace ibs {

// one field line: array k (bmag gradpar cvdrift cvdrift0 gds2 gds21 gds22 gbdrift) at p + k * ld
struct GeoLine {
  const double* p; long ld;
  __device__ __forceinline__ double at(int k, int j) const { return p[(long)k * ld + j]; }
};
// (g, c, f) of a line at theta0 (the arithmetic of k_assemble_gcf_long: ball_scan.py:267-268, utils.py:1560-1562)
__device__ __forceinline__ void line_gcf(const GeoLine& L, int j, double mdP, double th0, double& g, double& c, double& f) {
  const double B = L.at(0, j), gp = xabs(L.at(1, j));
  const double inv = 1.0 / (gp * B);
  const double A1 = gp / B, A3 = inv / (B * B);
  const double C0 = mdP * L.at(2, j) * inv, C1 = mdP * L.at(3, j) * inv;
  const double d = L.at(4, j) + (2.0 * th0) * L.at(5, j) + (th0 * th0) * L.at(6, j);
  g = A1 * d; c = C0 + th0 * C1; f = A3 * d;
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
