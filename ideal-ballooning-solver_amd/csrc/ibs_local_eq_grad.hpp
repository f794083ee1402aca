// Local-equilibrium gradients: lam_max at points (line, theta0, eps, p) of the rule of ibs_local_eq.hpp with its EXACT derivatives in theta0,
// eps, p and the line's dPdrho, and optionally its cotangent planes in the line's eight arrays -- Hellmann-Feynman on the discrete pencil.
//
// lam_max is a simple eigenvalue of the pencil with mode X, X_0 = X_{N-1} = 0, and
//   lam = (sum_j c_j X_j^2 - 1/2 h^-2 sum_j g_j w_j) / q,   q = sum_j f_j X_j^2,   w_j = pencil_weight(X, j, N) (ibs_marginal.hpp)
// so for a parameter s of the rows
//   d lam / d s = (sum c_s X^2 - 1/2 h^-2 sum g_s w - lam sum f_s X^2) / q
// exact for the lam returned to first order in the error of X.  With a = |gradpar|, B = bmag and the x, cv', gd' of the rule
//   g_s = a gd'_s / B,  f_s = gd'_s / (B^3 a),  gd'_s = (2 gds21 + 2 x gds22) x_s,  c_s = -p dPdrho cv0 x_s / (a B) + (the extra term)
//   s        x_s                              extra term of c_s
//   theta0   1 + eps
//   eps      theta0 + sigma (theta_j - theta_c)
//   p        ps_j                             -dPdrho (cv' + p (cv - gb)) / (a B)
//   dPdrho   0                                -p cv' / (a B)
// Per grid point everything that multiplies x_s is ONE number,
//   K_j = (2 gds21 + 2 x gds22) (-1/2 h^-2 (a / B) w - lam X^2 / (B^3 a)) - p dPdrho cv0 X^2 / (a B)
// and the four derivatives are five sums over j: K, K (theta_j - theta_c), K ps, (cv' + p (cv - gb)) X^2 / (a B), cv' X^2 / (a B).
// The cotangent planes, from g_bar = -1/2 h^-2 w / q, c_bar = X^2 / q, f_bar = -lam X^2 / q, gd_bar = g_bar a / B + f_bar / (B^3 a),
// cv_bar = -p dPdrho c_bar / (a B):
//   bmag     -(g_bar g + c_bar c + 3 f_bar f) / B          gradpar  sgn(gradpar) (g_bar g - c_bar c - f_bar f) / a
//   cvdrift  p cv_bar         cvdrift0  x cv_bar           gbdrift  (1 - p) cv_bar
//   gds2     gd_bar           gds21     2 x gd_bar         gds22    x^2 gd_bar
// numpy restatement: ibs_amd.operators.local_eq_fold_tangent, local_eq_lam_grad.
//
// THE KERNEL (k_local_eq_grad, ibs_local_eq_grad.hip): FP64, any odd N in [66, kMaxLongN], one wavefront per point on the persistent grid
// of min(n_pts, n_waves) waves, division form throughout.  A point names its line by index (line_of), so one staged geometry serves any
// number of points.  Per-wave workspace, in this order (LocalEqGradWs: the kernel carves it, the host sizes it): local_eq_ws(N) -- the
// eigenvector stage's rows, then g, c, f -- and the mode X.
#pragma once
#include <hip/hip_runtime.h>

#include "ibs_local_eq.hpp"

namespace ibs {

struct LocalEqGradWs {
  LocalEqWs rows; size_t X, total;
};
constexpr LocalEqGradWs local_eq_grad_ws(int N) {
  const LocalEqWs r = local_eq_ws(N);
  return LocalEqGradWs{r, r.total, r.total + (size_t)N};
}
struct LocalEqGradArgs {
  int n_lines; long n_pts; int N; double theta_lo, h;
  const double* geo; long ld; size_t plane;                         // array k of line l at geo + k * plane + l * ld
  const double *dPdrho, *centre, *sigma;                            // [n_lines]
  const double* ps; long ps_ld;                                     // [n_lines][ps_ld] or null
  const int* line_of;                                               // [n_pts]: the line of a point; outside [0, n_lines): status bit 1
  const double* var;                                                // [n_pts][3] = (theta0, eps, p)
  double *lam, *gam;                                                // [n_pts], each optional
  double* dlam;                                                     // [n_pts][4] = d lam / d (theta0, eps, p, dPdrho) or null
  double* geo_bar; long ld_bar; size_t plane_bar;                   // plane k of point p at geo_bar + k * plane_bar + p * ld_bar, or null
  int* info;                                                        // [n_pts] or null
  double* work; size_t work_doubles; long n_waves;                  // the launch refuses less than min(n_pts, n_waves) waves' worth
};
hipError_t launch_local_eq_grad(const LocalEqGradArgs& a, hipStream_t st);

}  // namespace ibs
