// Local-equilibrium boundaries minimised over theta0: the first-stability parameter of a ray family between the nodes of a coarse theta0
// grid -- the envelope over theta0 that the boundary of an s-alpha picture is by convention, where ibs_local_eq_boundary_f64 gives the
// crossings of rays with theta0 frozen.
//
// THE RULE (restated in Python: ibs_amd.scan.local_eq_first_up and ibs_amd.scan.polish_first_up)
//   family     seven doubles as a ray of ibs_local_eq_boundary.hpp, (-, eps0, p0, d_eps, d_p, t_lo, t_hi); entry 0 is ignored and replaced
//              by the theta0 under evaluation.
//   T(theta0)  the boundary rule of ibs_local_eq_boundary.hpp on the family's ray at that theta0 with max_cross = 1, COLD: the same 64
//              nodes, the same closing passes, the same xtol and pass cap, so that T is bit for bit what ibs_local_eq_boundary_f64
//              returns for that ray.  Unstable at t_lo (lo_unstable): T = t_lo.  Else a crossing (the first crossing of a ray that
//              starts stable is stable -> unstable): T = (t_stable[0] + t_unstable[0]) / 2.  Else T = +inf.  An evaluation with status
//              bit 0 (pass cap) or 1 (invalid data) is a FAILED evaluation.
//   search     f(theta0) = -T(theta0) is maximised by the rule of ibs_theta0_polish.hpp, unchanged: the peaks of the coarse row
//              f_j = -T(theta0_j) ranked by row_peaks, K <= t0p::kMaxSlots start slots per (line, family), the bracket between the
//              neighbouring nodes (cut at a row end or a NaN neighbour), init / step / result with failed and non-finite values
//              counting as -inf, the incumbent rule (the result is never worse than the node), status bits 10, 11 and 12,
//              max_eval <= t0p::kMaxEval and the absolute tolerance xtol_theta0.
//   addition   a slot whose node already has T = t_lo is returned at once: no evaluation, bit 10 set.  Nothing can beat it.
//   the row    is an INPUT, t_row[line][family][n_theta0] = T at the nodes: +inf where there is no crossing, t_lo where the ray is
//              unstable at t_lo, NaN where the node is not to be used.
//   outputs    per slot: theta0*, T* = t_out, and the t_stable / t_unstable / lo_unstable of the evaluation at theta0* (the first
//              crossing's two ends, whichever way it goes; NaN without a crossing).  Where the node itself is returned (bit 10) t_out is
//              the row's entry and ONE more evaluation at the node supplies the ends; it is not a step of the search and enters neither
//              n_eval nor the pass count of info, its status bits 0-1 and 3 enter the slot's word.  The early return of the addition
//              gives NaN ends and lo_unstable = 1.  A slot with status bit 1 (invalid data in some evaluation, a non-finite family,
//              t_lo >= t_hi, sigma not +-1, a bad theta0 grid) has NaN in every floating-point output and lo_unstable = -1; a row
//              without a usable node has node -1, NaN outputs and a clean word.  Bit 3 (a bracket's ends became FP64 neighbours
//              before xtol was met, in some evaluation) and bits 10-12 are informational.
//
// THE KERNEL (k_local_eq_boundary_polish, ibs_local_eq_boundary_polish.hip): FP64, any odd N in [66, kMaxLongN], one wavefront per (line,
// family, slot) on the persistent grid of min(n_sys, n_waves) waves, no atomics, no global workspace.  The wave holds a t0p::State
// wave-uniform; for each requested theta0 it runs pass 0 and the closing passes of the first crossing by the stages of
// ibs_local_eq_boundary_stages.hpp (the definitions k_local_eq_boundary runs), then feeds -T to t0p::step.  Before the first evaluation
// the LDS that the stages use holds f = -T of the slot's coarse row, which is why n_theta0 <= kBoundaryVals * kBoundaryChunk.
// A slot's outputs depend on its line, its family, its coarse row and its slot alone, bit for bit.
#pragma once
#include <hip/hip_runtime.h>

#include "ibs_local_eq_boundary.hpp"
#include "ibs_theta0_polish.hpp"

namespace ibs {

constexpr int kBoundaryPolishMaxTheta0 = kBoundaryVals * kBoundaryChunk;      // the coarse row of a slot lies in the block's LDS

struct LocalEqBoundaryPolishArgs {
  int n_lines, n_ray, N; double theta_lo, h;
  const double* geo; long ld; size_t plane;                         // array k of line l at geo + k * plane + l * ld
  const double *dPdrho, *centre, *sigma;                            // [n_lines]
  const double* ps; long ps_ld;                                     // [n_lines][ps_ld] or null
  const double* rays;                                               // [n_ray][7], entry 0 ignored
  const double* theta0; int n_theta0;                               // [n_theta0], finite and strictly increasing
  const double* t_row;                                              // [n_lines][n_ray][n_theta0]
  double shift, xtol; int n_starts; double xtol_theta0; int max_eval;
  double *theta0_out, *t_out, *t_stable_out, *t_unstable_out;       // [n_lines][n_ray][n_starts]
  int *node, *n_eval, *lo_unstable, *info;                          // [n_lines][n_ray][n_starts], each optional
  int* n_found;                                                     // [n_lines][n_ray], optional
  long n_waves;                                                     // the persistent grid: min(n_sys, n_waves) waves
};
hipError_t launch_local_eq_boundary_polish(const LocalEqBoundaryPolishArgs& a, hipStream_t st);

}  // namespace ibs
