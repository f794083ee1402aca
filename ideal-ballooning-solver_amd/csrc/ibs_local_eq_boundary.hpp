// Local-equilibrium boundaries: the stability boundaries of a field line along straight rays in the (eps, p) plane of the rule of
// ibs_local_eq.hpp -- the CURVE of the s-alpha picture where k_local_eq_scan gives the raster.
//
// A RAY: seven doubles (theta0, eps0, p0, d_eps, d_p, t_lo, t_hi), t_lo < t_hi; the triple at parameter t is (theta0, eps0 + t d_eps,
// p0 + t d_p).  theta0 does not vary along a ray, so the fold variable of the rule is LINEAR in t,
//   x_j(t) = X0_j + t X1_j,   X0_j = theta0 (1 + eps0) + sigma eps0 dth_j + (p0 - 1) ps_j,   X1_j = theta0 d_eps + sigma d_eps dth_j + d_p ps_j
// and the rows of the rule are QUADRATIC polynomials in t.  STAGED FORM (the builder's choice of the two the design allows): the
// per-point polynomial coefficients in t, seven values per grid point j --
//   gt_j(t) = G0 + t (G1 + t G2)   = g_j(t) / (2 h^2): the half-grid e between j and j + 1 is gt_j + gt_{j+1}
//   f_j(t)  = R gt_j(t),           R = 2 h^2 / (gradpar_j bmag_j)^2       (f / g of the rule does not depend on the variation)
//   c_j(t)  = C0 + t (C1 + t C2)   = -p(t) dPdrho (gb + p(t) (cv - gb) + x_j(t) cv0) / (|gradpar| bmag)
// formed ONCE per (system, chunk, pass) by the lanes together (coalesced loads of the eight arrays and the ps row; the t-invariant factors
// |gradpar| / bmag / (2 h^2), 1 / (|gradpar| bmag) and R are formed there, not per lane).  A lane evaluates its own t with four fma and one
// product per point and reads LDS only, at wave-uniform addresses.  The expansion in t rounds differently from local_eq_gcf at the
// triple (a few ulp of the largest term of each polynomial): verdicts agree with k_local_eq_scan wherever lam_max is farther from the
// shift than the count margin, which is all a count at a fixed shift ever promises.
//
// THE KERNEL (k_local_eq_boundary, ibs_local_eq_boundary.hip): FP64, any odd N in [66, kMaxLongN], one wavefront per (line, ray) on the
// persistent grid of min(n_lines * n_ray, n_waves) waves, division form, no atomics, no global workspace.  The 64 lanes are 64 values
// of t of ONE system; each runs its own division-form count at the fixed shift (the pivot guard and fast_rcp recurrence of
// count_above_chunked, ibs_long.hpp); the verdict of a lane is count > 0.
//   pass 0    lanes at the nodes t_lo + k (t_hi - t_lo) / 63 (lane 63: t_hi itself); a crossing = an adjacent node pair with different
//             verdicts; the first max_cross <= kMaxCross in increasing t are kept, more set status bit 2
//   closing   one crossing after the other: the lanes at a + (l + 1) (b - a) / 65 inside the bracket [a, b]; the new bracket = the first
//             adjacent pair (ends included) whose verdicts differ; until b - a <= xtol (t_hi - t_lo), or no lane point lies strictly
//             inside (a, b) (status bit 3 where xtol was not met), or kBoundaryPassCap passes were made (status bit 0)
// Status bit 1 (NaN parameters, n_cross -1, lo_unstable -1, node counts -1): non-finite data in the line, g or f <= 0 at any lane's t of
// any pass, sigma not +-1, a non-finite ray, t_lo >= t_hi -- of that system alone.  A system's outputs depend on its line and its ray
// alone, bit for bit.
#pragma once
#include <hip/hip_runtime.h>

#include "ibs_launch.hpp"

namespace ibs {

constexpr int kMaxCross = 4;             // crossings kept per (line, ray)
constexpr int kBoundaryPassCap = 12;     // closing passes per crossing
constexpr int kBoundaryVals = 7;         // staged values per grid point: G0 G1 G2 R C0 C1 C2
constexpr int kBoundaryChunk = 360;      // grid points per chunk: 7 x 360 doubles = 20,160 bytes per block -- eight blocks per CU as on the long path
static_assert(kBoundaryVals * kBoundaryChunk * sizeof(double) <= 20 * 1024, "at most 20 KB of LDS per block");
static_assert(8 * kBoundaryVals * kBoundaryChunk * sizeof(double) <= 160 * 1024, "eight blocks per CU");

struct LocalEqBoundaryArgs {
  int n_lines, n_ray, N; double theta_lo, h;
  const double* geo; long ld; size_t plane;                         // array k of line l at geo + k * plane + l * ld
  const double *dPdrho, *centre, *sigma;                            // [n_lines]
  const double* ps; long ps_ld;                                     // [n_lines][ps_ld] or null
  const double* rays;                                               // [n_ray][7]
  double shift; int max_cross; double xtol;
  double *t_stable, *t_unstable;                                    // [n_lines][n_ray][max_cross]
  int* n_cross;                                                     // [n_lines][n_ray]
  int *lo_unstable, *node_count, *info;                             // [n_lines][n_ray], [n_lines][n_ray][64], [n_lines][n_ray]; each optional
  long n_waves;                                                     // the persistent grid: min(n_sys, n_waves) waves
};
hipError_t launch_local_eq_boundary(const LocalEqBoundaryArgs& a, hipStream_t st);

}  // namespace ibs
