// Local-equilibrium variations of a field line: the (g, c, f) rows of a line whose surface has its global shear and its pressure
// gradient varied about the equilibrium, formed from the line's eight arrays alone -- no new geometry.  Nothing upstream corresponds
// for a real field line (bishop_ball_s-alpha.py does the analytic shifted-circle model only).
//
// THE RULE.  A line: bmag B, gradpar, cvdrift cv, cvdrift0 cv0, gds2, gds21, gds22, gbdrift gb on the uniform grid theta_j = theta_lo + j h,
// its dPdrho, the centre theta_c of its secular term (= alpha for lines of ibs_fieldline_geometry_f64, whose phi_center is 0), the sign
// sigma = sign(-phiedge) = +-1, and optionally a row ps_j = the change of the integrated local shear per unit of (p - 1), in units of
// the fold variable (absent: 0, frozen local shear).  A variation: (theta0, eps, p), eps = the relative change of the surface's shear,
// p = the factor on the pressure gradient.  Then
//   x_j   = theta0 (1 + eps) + sigma eps (theta_j - theta_c) + (p - 1) ps_j
//   cv'_j = gb_j + p (cv_j - gb_j) + x_j cv0_j
//   gd'_j = gds2_j + 2 x_j gds21_j + x_j^2 gds22_j
//   dP'   = p dPdrho
//   g = |gradpar| gd' / B,   c = -dP' cv' / (|gradpar| B),   f = gd' / B^2 / (|gradpar| B)                    (utils.py:1560-1562)
// and the operator is the one every other entry point solves.  Why: a change of iota' at fixed p' (Greene-Chance) moves only the
// secular term of grad alpha, which points along grad psi -- for the arrays that is the theta0 fold (utils.py:1659-1660) with a fold
// variable that depends on theta; a change of p' scales dPdrho and the pressure part cvdrift - gbdrift of the curvature drift.
//   eps = 0, p = 1, no ps:   the fold of ibs_gamma_scan_f64 at theta0
//   no ps, theta_c = alpha:  the geometry re-evaluated with d_iota_d_s (1 + eps) and d_pressure_d_s p, folded at theta0 (the
//                            ballooning angle of the VARIED equilibrium)
//   ps:                      where a local-equilibrium code puts the self-consistent change of the local shear; the s-alpha model's
//                            row is -alpha0 (sin theta - sin theta0) / shat0
// numpy restatement: ibs_amd.operators.local_eq_fold.
#pragma once
#include <hip/hip_runtime.h>

#include "ibs_launch.hpp"
#include "ibs_wave.hpp"

namespace ibs {

// one variation as the rule consumes it, wave-uniform: formed once per system from the line's (theta_c, sigma) and the triple
struct LocalEqFold {
  double x0;      // theta0 (1 + eps): the fold variable at theta = theta_c
  double xs;      // sigma eps: its slope in theta
  double pm1, p;  // p - 1 (the weight of ps), p
  double mdP;     // -p dPdrho
};
__device__ __forceinline__ LocalEqFold local_eq_fold_of(double dPdrho, double sigma, double theta0, double eps, double p) {
  return LocalEqFold{theta0 * (1.0 + eps), sigma * eps, p - 1.0, p, -(p * dPdrho)};
}
// THE RULE at grid point j of a line with accessor at(k, j), k = bmag gradpar cvdrift cvdrift0 gds2 gds21 gds22 gbdrift (ibs_geo_line.hpp):
// dth = theta_j - theta_c, ps = ps_j (0 without a row)
template <class Line>
__device__ __forceinline__ void local_eq_gcf(const Line& L, int j, const LocalEqFold& v, double dth, double ps, double& g, double& c,
                                             double& f) {
  const double B = L.at(0, j), gp = xabs(L.at(1, j)), gb = L.at(7, j);
  const double x = xfma(v.pm1, ps, xfma(v.xs, dth, v.x0));
  const double cv = xfma(x, L.at(3, j), xfma(v.p, L.at(2, j) - gb, gb));
  const double gd = xfma(x, xfma(x, L.at(6, j), 2.0 * L.at(5, j)), L.at(4, j));
  const double inv = 1.0 / (gp * B);
  g = gp * gd / B; c = v.mdP * cv * inv; f = gd / (B * B) * inv;
}

// k_local_eq_scan (ibs_local_eq.hip): FP64, any odd N in [66, kMaxLongN], one wave per (line, variation) system on the persistent grid of
// min(n_lines * n_var, n_waves) waves.  Per-wave workspace, in this order (LocalEqWs: the kernel carves it, the host sizes it): the
// eigenvector stage's nearest_ws_doubles(N), then the system's g, c and f rows.
struct LocalEqWs {
  size_t work, g, c, f, total;
};
constexpr LocalEqWs local_eq_ws(int N) {
  const size_t n = (size_t)N, w = nearest_ws_doubles(N);
  return LocalEqWs{0, w, w + n, w + 2 * n, w + 3 * n};
}
struct LocalEqArgs {
  int n_lines, n_var, N; double theta_lo, h;
  const double* geo; long ld; size_t plane;                         // array k of line l at geo + k * plane + l * ld
  const double *dPdrho, *centre, *sigma;                            // [n_lines]
  const double* ps; long ps_ld;                                     // [n_lines][ps_ld] or null
  const double* var;                                                // [n_var][3] = (theta0, eps, p)
  double shift;                                                     // of the count
  double *gam, *lam; int* count; int* info;                         // [n_lines][n_var], each optional
  double* work; size_t work_doubles; long n_waves;                  // the launch refuses less than min(n_sys, n_waves) waves' worth
};
hipError_t launch_local_eq_scan(const LocalEqArgs& a, hipStream_t st);

}  // namespace ibs
