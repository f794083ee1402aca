// Launch-argument structs and the per-M launcher table shared by ibs_kernels.hip (one object per
// rows-per-lane value M) and ibs_api.hip (the C-ABI layer).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdio>

#include "ibs_plan.hpp"     // kMaxM, kMaxLongN, lds_pitch, scan_max_threads(_g): the launch shapes are planned there

namespace ibs {

template <typename T>
struct GcfArgs {
  long n_sys; int N; T h; const T* g; const T* c; const T* f; long ld;
  T* lam; T* gam; T* X; T* dX; int* info; int wpb;
  const T* gh;      // optional half-grid g [n_sys][ld] (N-1 used); null = mean of neighbouring g
  int flags;        // FP64 solvers: bit 0 = re-close suspect systems in division form, bit 1 = only mark them
  // big-batch forms (rows from global memory, sub-wave): a suspect system is only LISTED by the solver kernel -- its re-close and the
  // repeat of its eigenvector stage run in a second, tiny launch (k_fix_gcf) so that none of that code sits in the hot kernel (it cost
  // 2 % at N_zeta = 512 and 9 % on the two-waves-per-SIMD forms: tools/ab_reclose.py).  fix_count[1] (zeroed by the caller),
  // fix_sys / fix_center [>= n_sys]: system index and the Rayleigh polish to re-close about.  null = re-close inside the kernel.
  int* fix_count; long* fix_sys; double* fix_center;
};
template <typename T>
struct ScanArgs {
  int n_lines, n_theta0, N; T h;
  const T *bmag, *gradpar, *cvdrift, *cvdrift0, *gds2, *gds21, *gds22; long ld;
  const T *dPdrho, *theta0;
  T *gam, *lam, *X, *dX, *dth0; int* info; int wpb;
  const T* lam_guess; T guess_width;     // optional warm start ([n_lines][n_theta0], absolute width); null = cold
  int chain; T chain_w1, chain_w2;       // k_gamma_scan_chain: theta0 values per wave and the widths of its warm starts
  // fused per-surface argmax (k_gamma_scan only): lines_per_surf consecutive lines form a surface; the block that
  // completes a surface reduces its [lines_per_surf * n_theta0] growth rates into pack[surf] = (max, first index).
  // surf_counter[n_surf]: zero between launches (the last arriver resets its word).  null pack = no fusion.
  int lines_per_surf; int* surf_counter; T* pack;
  int pack_mode;                         // 1 = write-through stores + sc1 loads (one block per CU), 2 = release / acquire fences
  int t0_stride;                         // k_gamma_scan only: 0 = theta0[n_theta0] shared by all lines, 1 = theta0[n_lines] (n_theta0 = 1)
  // k_gamma_scan, 3 <= M <= 8: 1 = the resident form (set-up rows carried in registers, 186 VGPRs at M = 8: launches of at most two waves
  // per SIMD), 0 = the lean form k_gamma_scan_lean (126 VGPRs at M = 8).  ih2 = 1 / (h * h), ih = 1 / h: divided once, on the host
  int resident; T ih2, ih;
  // resident form only: the Context's trial table for (N, rows per lane) (k_trial_table, kTrialTableLen values, built on the launch's
  // stream), or null = every wave computes the start of its trial vector itself.  Same bits either way
  const T* trial_tab;
};
// gam maximised over theta0 about the peaks of every line's coarse row (k_theta0_polish; the rule: ibs_theta0_polish.hpp).  One block
// per line, n_starts <= 4 waves.  gam (required), lam (optional warm starts) [n_lines][n_theta0]; node_in (optional) and every output
// but n_found [n_lines] are [n_lines][n_starts]; theta0_star and gam_star are required.  w1, w2: the widths of the warm starts, as
// ScanArgs::chain_w1 / chain_w2
template <typename T>
struct Theta0PolishArgs {
  int n_lines, n_theta0, N; T h;
  const T *bmag, *gradpar, *cvdrift, *cvdrift0, *gds2, *gds21, *gds22; long ld;
  const T *dPdrho, *theta0, *gam, *lam; const int* node_in;
  int n_starts; T xtol; int max_eval; T w1, w2;
  T *theta0_star, *gam_star, *lam_star; int *node, *n_eval, *info, *n_found;
};
template <typename T>
struct SturmArgs {
  long n_sys; int N; T h; const T* g; const T* c; const T* f; long ld; const T* shift; int* count; int wpb;
};

template <typename T>
struct GradArgs {
  int n_pts, N; T h; const T* geo; long ld; const T* theta0; T del_alpha;
  T *val, *jac, *gam, *dalpha, *dth0; int* info; int wpb;
  long arr_stride, line_stride;   // 0 = the [n_pts][3][8][ld] layout (ld, 8 ld); see k_obj_w_grad
};

// grids beyond 64 * kMaxM + 2 points (ibs_long.hip): one wave per system, division form throughout
struct LongGcfArgs {
  long n_sys; int N; double h;
  const void *g, *c, *f, *gh; int f32;      // f32: the arrays (inputs and outputs) are float; the arithmetic is FP64 either way
  long ld; void *lam, *gam, *X, *dX; int* info;
  double* work; int n_waves;                // n_waves * 3 * N doubles of workspace; the grid is min(n_sys, n_waves) waves
};
hipError_t launch_gcf_long(const LongGcfArgs& a, hipStream_t st);
// the persistent grid of the one-wave-per-system kernels below: min(n, n_waves) waves, each with per_wave doubles of workspace at
// work + wave * per_wave; 0 = the workspace is missing or too short for that grid (the launch refuses)
inline long persistent_grid(long n, long n_waves, const double* work, size_t work_doubles, size_t per_wave) {
  const long grid = n < n_waves ? n : n_waves;
  return grid >= 1 && work && work_doubles >= (size_t)grid * per_wave ? grid : 0;
}
// the eigenpair nearest sigma[sys] (ibs_nearest.hip), FP64, any N in [66, kMaxLongN]: one wave per system, persistent grid of
// min(n_sys, n_waves) waves, each with nearest_ws_doubles(N) doubles of workspace at work + wave * nearest_ws_doubles(N)
constexpr size_t nearest_ws_doubles(int N) { return 3 * (size_t)N; }
struct NearestArgs {
  long n_sys; int N; double h;
  const double *g, *c, *f, *gh; long ld; const double* sigma;     // gh: null = mean of neighbouring g
  double* lam; int* idx; double* gam; double* X; double* dX; int* info;
  double* work; size_t work_doubles; long n_waves;                // the launch refuses a workspace below min(n_sys, n_waves) waves
};
hipError_t launch_gcf_nearest(const NearestArgs& a, hipStream_t st);
// the n_modes largest eigenpairs (ibs_modes.hip), FP64, any N in [66, kMaxLongN], 1 <= n_modes <= kMaxModes: one wave per system on the
// same persistent grid.  Per-wave workspace, in this order: the eigenvector stage's nearest_ws_doubles(N), kMaxModes closed
// eigenvalues, kMaxModes status words (ints, in kMaxModes doubles of room).  Outputs [n_sys][n_modes] (X, dX: [n_sys][n_modes][N])
constexpr size_t modes_ws_doubles(int N) { return nearest_ws_doubles(N) + 2 * (size_t)kMaxModes; }
struct ModesArgs {
  long n_sys; int N; double h;
  const double *g, *c, *f, *gh; long ld; int n_modes;            // gh: null = mean of neighbouring g
  double *lam, *gam, *X, *dX; int* info;                          // each optional
  double* work; size_t work_doubles; long n_waves;                // the launch refuses a workspace below min(n_sys, n_waves) waves
};
hipError_t launch_gcf_modes(const ModesArgs& a, hipStream_t st);
// the same with an F-orthonormal Ritz basis of every cluster of modes (ibs_modes_basis.hip; the construction: ibs_modes_basis.hpp).
// X is required: the members' vectors are built in the caller's rows.  cluster_first [n_sys][n_modes], optional.  Per-wave
// workspace, in this order: the five rows of the elimination (the first three serve the unclustered modes' eigenvector stage),
// kMaxModes closed eigenvalues, kMaxModes growth rates of a cluster's members, then status words, cluster_first and the open flag
// (2 kMaxModes + 1 ints, in 2 kMaxModes doubles of room)
constexpr size_t basis_rows_doubles(int N) { return 5 * (size_t)N; }
constexpr size_t basis_ws_doubles(int N) { return basis_rows_doubles(N) + 4 * (size_t)kMaxModes; }
struct ModesBasisArgs {
  long n_sys; int N; double h;
  const double *g, *c, *f, *gh; long ld; int n_modes;            // gh: null = mean of neighbouring g
  double *lam, *gam, *X, *dX; int* cluster_first; int* info;      // X required, the others optional
  double* work; size_t work_doubles; long n_waves;                // the launch refuses a workspace below min(n_sys, n_waves) waves
};
hipError_t launch_gcf_modes_basis(const ModesBasisArgs& a, hipStream_t st);
// exact vector-Jacobian product of gam and lam in the (g, c, f) rows (ibs_vjp.hip), FP64, any N in [66, kMaxLongN]: one wave per
// system, persistent grid of min(n_sys, n_waves) waves, each with vjp_ws_doubles(N) doubles of workspace at work + wave * vjp_ws_doubles(N)
constexpr size_t vjp_ws_doubles(int N) { return 3 * (size_t)N; }
struct VjpArgs {
  long n_sys; int N; double h;
  const double *g, *c, *f; long ld;                              // every row array (inputs, X and the outputs) has rows ld apart
  const double *lam, *X, *gam_bar, *lam_bar;                      // gam_bar / lam_bar: null = 0
  double *g_bar, *c_bar, *f_bar; int* info;                       // info optional
  double* work; size_t work_doubles; long n_waves;                // the launch refuses a workspace below min(n_sys, n_waves) waves
};
hipError_t launch_gcf_vjp(const VjpArgs& a, hipStream_t st);
// geometry-fed points with the eigenpair nearest sigma[p] (ibs_nearest_grad.hip): one wave per point on the persistent grid of
// min(n_pts, n_waves) waves.  Per-wave workspace, in this order (NearestPointsWs: the kernel carves it, the host sizes it):
// the solver's nearest_ws_doubles(N), the centre line's g, c, f rows, and with GRAD the eigenfunction X and dX.
struct NearestPointsWs {
  size_t work, g, c, f, X, dX, total;
};
constexpr NearestPointsWs nearest_points_ws(int N, bool grad) {
  const size_t n = (size_t)N, w = nearest_ws_doubles(N);
  return NearestPointsWs{0, w, w + n, w + 2 * n, grad ? w + 3 * n : 0, grad ? w + 4 * n : 0, w + (grad ? 5 : 3) * n};
}
struct NearestPointsArgs {
  int n_pts, N; double h; long ld;
  // GRAD: geo [n_pts][3][8][ld] (lines alpha - d/2, alpha, alpha + d/2 x bmag gradpar cvdrift cvdrift0 gds2 gds21 gds22 gbdrift);
  // else geo7[k] [n_pts][ld] (the seven arrays of ibs_gamma_points_f64) and dPdrho [n_pts]
  const double* geo; const double* geo7[7]; const double* dPdrho;
  const double* theta0; const double* sigma; double del_alpha;      // theta0, sigma: [n_pts]
  double *val, *jac;                                                  // GRAD: [n_pts], [n_pts][2] (required)
  double* gam; double* lam; int* idx; double* X; double* dX; int* info;     // optional, except gam without GRAD
  double* work; size_t work_doubles; long n_waves;                    // the launch refuses less than min(n_pts, n_waves) waves' worth
};
hipError_t launch_obj_w_grad_nearest(const NearestPointsArgs& a, hipStream_t st);
hipError_t launch_points_nearest(const NearestPointsArgs& a, hipStream_t st);
// geometry-fed points with the EXACT gradient of gam (ibs_exact_grad.hip): one wave per point on the persistent grid of
// min(n_pts, n_waves) waves.  Per-wave workspace, in this order (ExactPointsWs: the kernel carves it, the host sizes it): three work
// rows -- the solver's (D+, D-, z: nearest_ws_doubles(N)) until X is out, then the adjoint's (V, B, Y: vjp_ws_doubles(N)), the first two
// of which receive g_bar and c_bar once V and B are dead (stage C of vjp_one reads Y alone) --, the centre line's g, c, f rows, the
// eigenfunction X, f_bar, and eight doubles of scalars (lam; the status words of the solve and of the adjoint).
struct ExactPointsWs {
  size_t work, gb, cb, g, c, f, X, fb, scal, total;
};
constexpr ExactPointsWs exact_points_ws(int N) {
  const size_t n = (size_t)N, w = nearest_ws_doubles(N) > vjp_ws_doubles(N) ? nearest_ws_doubles(N) : vjp_ws_doubles(N);
  return ExactPointsWs{0, 0, n, w, w + n, w + 2 * n, w + 3 * n, w + 4 * n, w + 5 * n, w + 5 * n + 8};
}
// The same struct feeds k_exact_tangent_points (ibs_exact_tangent.hip): ONE line per point and its alpha-tangent, same stages, grid and workspace.
struct ExactPointsArgs {
  int n_pts, N; double h; long ld;
  const double* geo;                                                  // [n_pts][3][8][ld], as NearestPointsArgs::geo; tangent form: [8][n_pts][ld]
  const double* geo_da;                                               // tangent form only: [8][n_pts][ld], the layout of the two geometry calls
  const double* theta0; const double* sigma; double del_alpha;        // theta0 [n_pts]; sigma [n_pts] or null = lam_max's eigenpair; del_alpha: three-line form only
  double *val, *jac;                                                  // [n_pts], [n_pts][2] (required)
  double* gam; double* lam; int* idx; int* info;                      // optional
  double* work; size_t work_doubles; long n_waves;                    // the launch refuses less than min(n_pts, n_waves) waves' worth
};
hipError_t launch_obj_w_grad_exact(const ExactPointsArgs& a, hipStream_t st);
hipError_t launch_obj_w_grad_exact_tangent(const ExactPointsArgs& a, hipStream_t st);
// vector-Jacobian product of a whole (line, theta0) table of growth rates (ibs_scan_vjp.hip), one chunk of whole lines.  Two launches:
// k_scan_vjp_points, one wave per system on the persistent grid of min(n_lines * n_theta0, n_waves) waves with the per-wave workspace
// of k_exact_points (exact_points_ws), leaves each system's cotangent rows in rows [sys][3][N] and its verdict in flag [sys];
// k_scan_vjp_reduce, one block per line, sums them through the fold over theta0, ascending.
enum : int { kScanVjpSkip = 0, kScanVjpUse = 1, kScanVjpPoison = 2 };   // flag: gam_bar = 0 | rows valid | failed under a non-zero cotangent
struct ScanVjpArgs {
  int n_lines, n_theta0, N; double h;
  const double* geo7[7]; long ld;                                   // the seven arrays of ibs_gamma_scan_f64, [n_lines][ld]
  const double *dPdrho, *theta0;                                    // [n_lines], [n_theta0]
  const double* sigma;                                              // [n_lines][n_theta0] or null = lam_max's eigenpair
  const double* gam_bar;                                            // [n_lines][n_theta0]
  double* geo_bar[7]; long ld_bar;                                  // optional (all seven or none), [n_lines][ld_bar]
  double *dPdrho_bar, *theta0_bar;                                  // optional [n_lines], [n_lines][n_theta0]
  double *gam, *lam; int* info;                                     // optional [n_lines][n_theta0]
  double* rows; int* flag;                                          // chunk workspace: [n_sys][3][N] (null: theta0_bar alone is wanted), [n_sys]
  double* work; size_t work_doubles; long n_waves;                  // the launch refuses less than min(n_sys, n_waves) waves' worth
};
hipError_t launch_scan_vjp(const ScanVjpArgs& a, hipStream_t st);
// marginal stability (ibs_marginal.hip): the critical scale s* of the pressure gradient at fixed rows, FP64, any odd N in
// [66, kMaxLongN]: one wave per system on the persistent grid of min(n_sys, n_waves) waves.  Per-wave workspace, in this order
// (MarginalWs: the kernels carve it, the host sizes it): the eigenvector stage's nearest_ws_doubles(N), the marginal mode X, and in
// the geometry-fed kernel the g and c rows of the wave's (line, theta0).
struct MarginalWs {
  size_t work, X, g, c, total;
};
constexpr MarginalWs marginal_ws(int N, bool scan) {
  const size_t n = (size_t)N, w = nearest_ws_doubles(N);
  return MarginalWs{0, w, scan ? w + n : 0, scan ? w + 2 * n : 0, w + (scan ? 3 : 1) * n};
}
struct MarginalArgs {
  long n_sys; int N; double h;
  const double *g, *c; long ld;                                     // rows ld apart
  double *scale, *mu, *gam0; int* info;                             // [n_sys]; scale required
  double *X, *g_bar, *c_bar;                                        // [n_sys][N], optional
  double* work; size_t work_doubles; long n_waves;                  // the launch refuses a workspace below min(n_sys, n_waves) waves
};
hipError_t launch_marginal_gcf(const MarginalArgs& a, hipStream_t st);
struct MarginalScanArgs {
  int n_lines, n_theta0, N; double h;
  const double* geo7[7]; long ld;                                   // the seven arrays of ibs_gamma_scan_f64, [n_lines][ld]
  const double *dPdrho, *theta0;                                    // [n_lines], [n_theta0]
  double *scale, *mu, *dth0, *ddP; int* info;                       // [n_lines][n_theta0]; scale required
  double* work; size_t work_doubles; long n_waves;
};
hipError_t launch_marginal_scan(const MarginalScanArgs& a, hipStream_t st);
// mu = 1 / s* maximised over theta0 about the peaks of every line's coarse row (ibs_marginal_polish.hip; the rule: ibs_theta0_polish.hpp):
// one wave per (line, slot) on the persistent grid of min(n_lines * n_starts, n_waves) waves, workspace marginal_ws(N, true).  mu
// (required) [n_lines][n_theta0]; node_in (optional) and every output but n_found [n_lines] are [n_lines][n_starts]; theta0_star and
// mu_star are required
struct MarginalPolishArgs {
  int n_lines, n_theta0, N; double h;
  const double* geo7[7]; long ld;                                   // as MarginalScanArgs
  const double *dPdrho, *theta0, *mu; const int* node_in;
  int n_starts; double xtol; int max_eval;
  double *theta0_star, *mu_star, *scale_star; int *node, *n_eval, *info, *n_found;
  double* work; size_t work_doubles; long n_waves;
};
hipError_t launch_marginal_theta0_polish(const MarginalPolishArgs& a, hipStream_t st);
// geometry-fed points with the gradient of s* in (alpha, theta0) (ibs_marginal_points.hip): one wave per point, workspace marginal_ws(N, true)
struct MarginalPointsArgs {
  int n_pts, N; double h; long ld;
  const double* geo;                                                // [n_pts][3][8][ld], as ExactPointsArgs::geo
  const double* theta0; double del_alpha;                           // theta0 [n_pts]
  double *val, *jac, *scale, *dscale, *dPdrho; int* info;           // [n_pts] ([n_pts][2]: jac, dscale); val required
  double* work; size_t work_doubles; long n_waves;                  // the launch refuses less than min(n_pts, n_waves) waves' worth
};
hipError_t launch_marginal_points(const MarginalPointsArgs& a, hipStream_t st);
// the same from ONE line per point and the alpha-tangent of its geometry, with the cotangent planes of s* (ibs_marginal_tangent.hip): the
// persistent grid and the per-wave workspace of k_marginal_points
struct MarginalTangentArgs {
  int n_pts, N; double h; long ld;
  const double *geo, *geo_da;                                       // both [8][n_pts][ld]; geo_da only with jac or dscale
  const double* theta0;                                             // [n_pts]
  double *val, *jac, *scale, *dscale, *dPdrho; int* info;           // as MarginalPointsArgs; val required
  double* geo_bar; long ld_bar;                                     // optional [8][n_pts][ld_bar]: d scale / d geo, entries 0 .. N-1 of a row
  double* work; size_t work_doubles; long n_waves;                  // the launch refuses less than min(n_pts, n_waves) waves' worth
};
hipError_t launch_marginal_tangent_points(const MarginalTangentArgs& a, hipStream_t st);
hipError_t launch_sturm_long(const SturmArgs<double>& a, hipStream_t st);
hipError_t launch_sturm_div(const SturmArgs<double>& a, hipStream_t st);     // lanes as systems, division form, any N
template <typename T> struct ScanArgs;
hipError_t launch_assemble_long(const ScanArgs<double>& a, double* g, double* c, double* f, double* gt, double* ct, double* ft, hipStream_t st);
// lines on a non-uniform theta grid (ibs_regrid.hip): the regrid of utils.py:1565-1576 onto the uniform grid of the window [lo, hi].
// n_lines grids (theta + line * theta_ld; theta_ld = 0: one shared row), each shared by per_line consecutive systems; outputs
// g_u, gh, c_u, f_u [n_lines * per_line][ld_out], gh[N - 1] = 0; info [n_lines * per_line] optional (status bit 1: not a grid, NaN rows).
// launch_regrid_rows: raw rows g, c, f [n_lines * per_line][ld] (c / c_u and f / f_u optional as pairs).  launch_assemble_regrid: the
// seven arrays geo7 [n_lines][ld], dPdrho [n_lines] and theta0 [per_line] -- or, t0_per_line, per_line = 1 and theta0 [n_lines].
struct RegridArgs {
  long n_lines, per_line; int N;
  const double* theta; long theta_ld; double lo, hi;
  const double *g, *c, *f; long ld;
  const double* geo7[7]; const double *dPdrho, *theta0; int t0_per_line;
  double *g_u, *gh, *c_u, *f_u; long ld_out; int* info;
  int n_cu;
};
hipError_t launch_regrid_rows(const RegridArgs& a, hipStream_t st);
hipError_t launch_assemble_regrid(const RegridArgs& a, hipStream_t st);
// NaN into lam, gam [n_sys] and X, dX [n_sys][N] (each optional) of the systems whose flag word (RegridArgs::info) carries status bit 1
hipError_t launch_regrid_poison(long n_sys, int N, const int* flag, double* lam, double* gam, double* X, double* dX, hipStream_t st);

// the n_starts best peaks of every surface's coarse table and the refinement's starts from them (ibs_scan_peaks.hip; the rule:
// ibs_scan_peaks.hpp).  gam [n_surf][n_alpha][n_theta0]; start [n_surf][n_starts][2], peak [n_surf][n_starts]; index, sigma0
// [n_surf][n_starts] and n_found [n_surf] optional; *n_bad is added to.  One block of `threads` (a multiple of 64, at most 256) per surface
struct ScanPeaksArgs {
  int n_surf, n_alpha, n_theta0, n_starts;
  const double *alpha, *theta0, *gam;
  double *start, *peak; int* index; double* sigma0; int* n_found; int* n_bad;
};
hipError_t launch_scan_peaks(const ScanPeaksArgs& a, int threads, hipStream_t st);

// field-line geometry kernel (ibs_geometry.hip)
// dPdrho[line] = -0.5 mean((cvdrift - gbdrift) bmag^2) of lines laid out geo[k * plane + line * ld + j], k = 0 .. 7 (ball_scan.py:262)
hipError_t launch_line_dPdrho(int n_lines, int N, long ld, size_t plane, const double* geo, double* dPdrho, hipStream_t st);
struct GeoForm { int ppl, lpp; };   // grid points per lane, lanes per grid point (one of them is 1)
constexpr int kGeoMaxPairs = 64;    // pair indices about a row's centre the one-lane-per-point table image holds for the root solve
struct GeoArgs {
  int n_surf, mnmax, mnmax_nyq, n_lines, N;
  const double *xm, *xn, *xm_nyq, *xn_nyq;
  const double* tab_mn;    // [n_surf][6][mnmax]      rmnc zmns lmns d_rmnc_d_s d_zmns_d_s d_lmns_d_s
  const double* tab_nyq;   // [n_surf][7][mnmax_nyq]  gmnc bmnc d_bmnc_d_s bsupvmnc bsubsmns bsubumnc bsubvmnc
  const double* scal;      // [n_surf][6]             s iota d_iota_d_s d_pressure_d_s phiedge Aminor_p
  const int* line_surf; const double* line_alpha; const double* theta;
  long ld;
  double* geo;             // [8][n_lines][ld]  bmag gradpar cvdrift cvdrift0 gds2 gds21 gds22 gbdrift
  double* dPdrho;          // [n_lines]
  // optional row structure of the mode lists (VMEC order: modes grouped by m, consecutive n inside a group):
  // rows_*[r] = {first mode index, number of modes}; the angle then advances by -dphi_n per mode and only
  // one sincos per row is needed.  nrows_* = 0 selects the generic one-sincos-per-mode kernel.
  int nrows_mn, nrows_nyq;
  const int* rows_mn;      // [nrows_mn][2]
  const int* rows_nyq;     // [nrows_nyq][2]
  double dn_mn, dn_nyq;    // common n-spacing inside the rows of each set (rows with another spacing are split by the host)
  int lpp;                 // lanes per grid point: 0 = chosen from the batch size, else 1 | 2 | 4 | 8; -2 = two grid points per lane
  int j_begin, j_end;      // (set by launch_geometry) grid points [j_begin, j_end) of every line are this launch's
  // round 3: the row kernels work from per-surface table images prepared once per call (k_geo_prepare), one image set
  // per lanes-per-point value (index geo_lpp_index: 1, 2, 4, 8); img_ready = bit per set already built from these tables
  GeoForm form;            // {0, 0} = picked by launch_geometry from the batch size
  double* img[4];
  unsigned img_ready;
  const int* n_lines_dev;  // optional: the number of lines actually requested, read on the device (<= n_lines, which then
                           // only sizes the grid): the refinement rounds of ibs_refine_f64 shrink without a host round trip
  size_t plane;            // distance between the 8 output planes in elements; 0 = n_lines * ld
  int* surf_used;          // optional [n_surf] scratch: launch_geometry marks the surfaces the lines refer to and k_geo_prepare builds
                           // only their images (a caller that works through a large table set piece by piece: AdjointStep)
};
GeoForm geo_pick_form(long n_lines, int N, int n_cu, int lpp_opt);
GeoForm geo_pick_usable(const GeoArgs& a, long n_lines, int N, int n_cu);      // ... among the forms whose table image fits the LDS
int geo_lpp_index(int lpp);
size_t geo_image_doubles(const GeoArgs& a, int lpp);      // per surface
bool geo_rows_usable(const GeoArgs& a, int lpp);
hipError_t launch_geometry(GeoArgs& a, hipStream_t st, int n_cu);

// vector-Jacobian product of the geometry (ibs_geometry_vjp.hip)
constexpr int kGeoVjpW = 29;   // workspace doubles per grid point
constexpr int kGeoVjpG = 8;    // modes per wave of the table reduction
struct GeoVjpArgs {
  int n_surf, mnmax, mnmax_nyq, n_lines, N;
  const double *xm, *xn, *xm_nyq, *xn_nyq;
  const double *tab_mn, *tab_nyq, *scal;       // as GeoArgs
  const int* line_surf; const double* line_alpha; const double* theta;
  long ld;
  size_t plane;                // distance between the 8 planes of geo_bar in elements; 0 = n_lines * ld
  const double* geo_bar;       // [8][n_lines][ld]
  const double* dPdrho_bar;    // optional [n_lines]
  double* ws;                  // [n_lines][kGeoVjpW][N]
  double *tab_mn_bar, *tab_nyq_bar, *scal_bar, *alpha_bar;   // each optional
};
hipError_t launch_geometry_vjp(GeoVjpArgs& a, hipStream_t st);

// alpha-tangent of the geometry (ibs_geometry_tangent.hip): d/d alpha of the eight arrays of every line, one lane per grid point
struct GeoDalphaArgs {
  int n_surf, mnmax, mnmax_nyq, n_lines, N;
  const double *xm, *xn, *xm_nyq, *xn_nyq;
  const double *tab_mn, *tab_nyq, *scal;       // as GeoArgs
  const int* line_surf; const double* line_alpha; const double* theta;
  long ld;
  size_t plane;                // distance between the 8 planes of geo_da in elements; 0 = n_lines * ld
  double* geo_da;              // [8][n_lines][ld]
};
hipError_t launch_geometry_dalpha(GeoDalphaArgs& a, hipStream_t st);

template <typename T> struct RefineEvalArgs;
struct LaunchTable {
  hipError_t (*gcf_f64[kMaxM + 1])(const GcfArgs<double>&, hipStream_t);
  hipError_t (*gcf_rows_f64[kMaxM + 1])(const GcfArgs<double>&, hipStream_t);   // row-streamed form (k_solve_gcf_rows)
  hipError_t (*gcf_direct_f64[kMaxM + 1])(const GcfArgs<double>&, hipStream_t);  // rows straight from global memory (k_solve_gcf_direct)
  hipError_t (*gcf_direct_f32w[kMaxM + 1])(const GcfArgs<float>&, hipStream_t);  // the same on FP32 arrays (FP64 solver)
  hipError_t (*gcf_direct_f32lam[kMaxM + 1])(const GcfArgs<float>&, hipStream_t); // FP32 eigenvalues only: all-FP32 iteration + FP64 certificate, rows from global memory
  hipError_t (*gcf_fix_f64[kMaxM + 1])(const GcfArgs<double>&, hipStream_t);     // the listed suspects of a big-batch launch: re-close + eigenvector stage (k_fix_gcf), M = ceil((N - 2) / 64)
  hipError_t (*gcf_fix_f32w[kMaxM + 1])(const GcfArgs<float>&, hipStream_t);
  hipError_t (*gcf_f32[kMaxM + 1])(const GcfArgs<float>&, hipStream_t);
  hipError_t (*gcf_f32_wide[kMaxM + 1])(const GcfArgs<float>&, hipStream_t);   // FP32 in HBM, FP64 in the solver (gam / X wanted)
  hipError_t (*gcf_f32w_rows[kMaxM + 1])(const GcfArgs<float>&, hipStream_t);  // the same, row-streamed (long grids)
  hipError_t (*gcf_f32w_g[2][kMaxM + 1])(const GcfArgs<float>&, hipStream_t);  // the same, 32 / 16 lanes per system
  hipError_t (*scan_f64[kMaxM + 1])(const ScanArgs<double>&, hipStream_t);
  hipError_t (*trial_table_f64[kMaxM + 1])(int N, double* tab, hipStream_t);         // scan_resident_built(M) only: fills ScanArgs::trial_tab
  hipError_t (*scan_chain_f64[kMaxM + 1])(const ScanArgs<double>&, hipStream_t);
  hipError_t (*theta0_polish_f64[kMaxM + 1])(const Theta0PolishArgs<double>&, hipStream_t);
  hipError_t (*sturm_f64[kMaxM + 1])(const SturmArgs<double>&, hipStream_t);
  hipError_t (*grad_f64[kMaxM + 1])(const GradArgs<double>&, hipStream_t);
  hipError_t (*refine_f64[kMaxM + 1])(const RefineEvalArgs<double>&, hipStream_t);   // one round of ibs_refine_f64 (ibs_refine.hpp)
  // sub-wave variants (ibs_group.hpp): index 0 -> 32 lanes per system, 1 -> 16 lanes per system
  hipError_t (*gcf_f64_g[2][kMaxM + 1])(const GcfArgs<double>&, hipStream_t);
  hipError_t (*scan_f64_g[2][kMaxM + 1])(const ScanArgs<double>&, hipStream_t);
  hipError_t (*scan_chain_f64_g[2][kMaxM + 1])(const ScanArgs<double>&, hipStream_t);   // chained / warm-started
};
LaunchTable& launch_table();

// Diagnostic record of the solver / geometry kernel most recently launched by this thread (C ABI: ibs_last_launch): the
// name as rocprofv3 prints it ("ibs::k_gamma_scan<double, 8>") and the launch dimensions -- the library picks lanes per
// system, chaining and geometry form from the batch size, and a measurement must be able to say which kernel it timed.
struct LaunchNote { char name[96]; long blocks; int threads; };
LaunchNote& last_launch();      // thread-local (ibs_api.hip)
void note_launch(long blocks, int threads, const char* fmt, ...);
template <typename T> constexpr const char* type_name() { return sizeof(T) == 8 ? "double" : "float"; }

// One launch of the per-M launchers: the dynamic-LDS limit of `kern` raised to `lds` where any is asked for, the launch, `note()` (the
// site's note_launch: only a launch that was issued is noted), the launch's error.
template <class Note, class... KA, class... A>
inline hipError_t launch_kernel(void (*kern)(KA...), dim3 grid, dim3 block, size_t lds, hipStream_t st, Note&& note, const A&... args) {
  if (lds) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(kern, grid, block, lds, st, args...);
  note();
  return hipGetLastError();
}

}  // namespace ibs
