// Pullback of ONE grid point of a geometry-fed system through the theta0 fold and the coefficients (the transpose of line_gcf,
// ibs_geo_line.hpp): the cotangents (g_bar, c_bar, f_bar) of the rows
//   cv = cvdrift + theta0 cvdrift0,  d = gds2 + 2 theta0 gds21 + theta0^2 gds22                      (ball_scan.py:267-268)
//   g = |gradpar| d / bmag,  c = -dPdrho cv / (|gradpar| bmag),  f = d / bmag^2 / (|gradpar| bmag)    (utils.py:1560-1562)
// become the cotangents of the seven values v[] = (bmag gradpar cvdrift cvdrift0 gds2 gds21 gds22) and of dPdrho.  The terms in theta0
// and theta0^2 go to cvdrift0, gds21 and gds22; |gradpar| is differentiated as line_gcf_tangent does, d|x| = sgn(x) dx (0 at 0).
// The results are ADDED to bar[] and dP_bar: the caller sums the systems of a line over theta0, ascending.
// Plain C++ on both sides, so that the host can check it (tests/test_scan_vjp_cpu.py); the device caller is k_scan_vjp_reduce.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define IBS_PB_HD __host__ __device__
#else
#define IBS_PB_HD
#endif

namespace ibs {

// mdP = -dPdrho, as line_gcf takes it
IBS_PB_HD inline void scan_pullback_point(double g_bar, double c_bar, double f_bar, const double v[7], double mdP, double th0,
                                          double bar[7], double& dP_bar) {
  const double B = v[0], gpr = v[1], gp = gpr < 0.0 ? -gpr : gpr;
  const double iB = 1.0 / B, inv = 1.0 / (gp * B);
  const double A1 = gp * iB, A3 = inv * iB * iB;
  const double cv = v[2] + th0 * v[3];
  const double d = v[4] + (2.0 * th0) * v[5] + (th0 * th0) * v[6];
  // g = A1 d, f = A3 d
  const double d_bar = g_bar * A1 + f_bar * A3;
  const double A1_bar = g_bar * d, A3_bar = f_bar * d;
  // c = mdP cv inv
  const double cm = c_bar * inv;
  const double cv_bar = cm * mdP;
  // inv enters c and A3 = inv / B^2;  inv = 1 / (gp B):  d inv = -inv^2 (B d gp + gp d B)
  const double inv_bar = c_bar * (mdP * cv) + A3_bar * (iB * iB);
  const double q = -inv_bar * inv * inv;
  // A1 = gp / B
  const double gp_bar = A1_bar * iB + q * B;
  const double B_bar = q * gp - (A1_bar * A1 + 2.0 * (A3_bar * A3)) * iB;
  bar[0] += B_bar;
  bar[1] += gpr > 0.0 ? gp_bar : (gpr < 0.0 ? -gp_bar : 0.0 * gp_bar);
  bar[2] += cv_bar;
  bar[3] += th0 * cv_bar;
  bar[4] += d_bar;
  bar[5] += (2.0 * th0) * d_bar;
  bar[6] += (th0 * th0) * d_bar;
  dP_bar -= cm * cv;                                        // (c is linear in mdP = -dPdrho)
}

}  // namespace ibs
