/* libibs_hip.so -- C ABI of the MI355X-native ideal-ballooning hot path.
 *
 * Drop-in boundary for the reference's module-level Python operators (there is no FFI upstream:
 * the operators are reached by `from utils import *`, ball_scan.py:19).  Each entry point names
 * the reference interface it replaces (paths relative to the reference checkout).  Plain pointers
 * and sizes only; no exceptions cross the boundary.
 *
 * Conventions
 *   - return value: 0 = ok; < 0 = argument/runtime error (text via ibs_last_error());
 *     > 0 = number of systems whose info word reports a non-zero status (IBS_MEM_HOST calls only: a device-pointer
 *     call is asynchronous and returns 0 -- request the info words and look at their status bits).
 *   - `mem`: IBS_MEM_DEVICE = all data pointers are device (HBM) pointers, the call is
 *     asynchronous on the context's stream; IBS_MEM_HOST = host pointers, the library stages
 *     through its own device workspace and the call returns after the results are back.
 *   - grids are uniform in theta with N points (N odd, N >= 66) and spacing h -- except in the four *_theta_f64 / ibs_regrid_rows_f64
 *     entry points, which take any increasing grid and regrid it as the reference does (utils.py:1565-1576); every entry point that
 *     takes h alone assumes a uniform grid and does not look at theta.  Arrays of one system/line are contiguous,
 *     consecutive systems are `ld` elements apart.  Up to N = 2050 the register-resident kernels run (one wavefront or a part of
 *     one per system).  The reference takes any length (utils.py:1556-1624; its own rule N = 2 mpol ntor 4 + 1, ball_scan.py:201-208,
 *     passes 2050 from mpol ntor > 256 on): for 2050 < N <= 65537 ibs_solve_gcf_f64 / _f32, ibs_solve_gcfh_f64, ibs_gamma_scan_f64 /
 *     _warm_f64 (the guesses are then unused) / _argmax_f64, ibs_gamma_points_f64, ibs_obj_w_grad_f64 and ibs_sturm_count_f64 run a
 *     generic path that works in division form on the rows in memory (csrc/ibs_long.hip: correct to the same tolerances, slower per
 *     row); the on-device refinement ibs_refine_f64 stays limited to N <= 2050 (IBS_ERR_UNSUPPORTED): beyond, ibs_obj_w_grad_f64
 *     under the caller's optimizer -- upstream's own form (ball_scan.py:307-314); the Python host layer drives the library's
 *     L-BFGS-B state machines (ibs_lbfgsb2_*) with one batched ibs_obj_w_grad_f64 launch per round.
 *   - optional outputs may be NULL.
 *   - info word per system: bits 0..15 = sweeps used, bits 16.. = status
 *     (bit 0 = iteration cap hit, bit 1 = invalid data: non-finite, g <= 0 or f <= 0.  Bits 2-4 are INFORMATIONAL -- the returned
 *     values are good; return values > 0 and the host-side counts look at bits 0 and 1 only:
 *     bit 2, FP32 eigenvalue-only path: the all-FP32 result failed its FP64 certificate and the system was solved in FP64;
 *     bit 3, FP64 raw-system entry points: the closing bracket of the shift iteration disagreed with the twisted factorisation's
 *            Rayleigh polish by more than min(512, 2 N) eps ||A|| and lam_max was closed again by division-form multisection on the
 *            rows (the recurrence of LAPACK dstebz): 0 .. 60 systems per million on iid-random coefficients, none on field-line
 *            data.  With it |lam - lam_max| <= 4 N eps ||A|| holds a priori (tests/test_gpu_configs.py), ||A|| = max_r (|d_r| +
 *            e_r + e_{r+1}) / f_r of utils.py:1584-1592's rows;
 *     bit 4, only with option "sigma0" set and both lam and info requested: lam_max >= sigma0.  The reference's ARPACK call returns
 *            the eigenpair NEAREST sigma0 (utils.py:1597); this library always returns lam_max's.  They are the same eigenpair
 *            whenever lam_max < sigma0 -- and only then: this bit marks the one case in which upstream may have returned another);
 *     bit 5, nearest-sigma entry points (ibs_*_nearest_f64): "nearest not determined" -- the eigenvalues on either side of
 *            sigma lie at distances that differ by less than 4 N eps ||A||; the larger one is returned
 *            (these entry points never set bit 3, whose re-close diagnostic occupies bits 5 and up on the lam_max entry points).
 *     bits 6-7, ibs_obj_w_grad_exact*_f64 and ibs_gamma_scan_vjp_f64 only: the two status bits of the adjoint solve
 *            (ibs_solve_gcf_vjp_f64's bits 0 and 1), moved clear of bits 0-5 -- bit 6: a pivot of the adjoint solve fell below pivmin
 *            and was replaced (informational: jac may be inaccurate); bit 7: the adjoint refused the pair (jac = NaN, val is good;
 *            ibs_gamma_scan_vjp_f64: that line's bars NaN).  Neither is counted by return values > 0.
 *     bit 8, marginal-stability entry points (ibs_marginal_*_f64) only: no row has c_j > 0, so no scale of the pressure gradient makes
 *            the line unstable -- scale = +inf, mu = 0, the derivatives are 0 and X, gam0 are NaN (informational: not counted by
 *            return values > 0).  ibs_marginal_obj_w_grad_f64 writes val = 0 and jac = dscale = 0 with it, and sets bit 1 with val
 *            and scale kept (jac = dscale = NaN) where the centre line solved but a side line of the alpha tangent held invalid data.
 *     bit 9, spectrum-mode entry points (ibs_*_modes_f64) only, per mode: "clustered" -- a neighbouring eigenvalue (the mode before
 *            or after it, or the first one not asked for) lies within tau = 4 N eps ||A||.  lam still holds to tau; the vector is
 *            SOME vector of the cluster's invariant subspace (it satisfies the pencil to the residual bound of ibs_solve_gcf_vjp_f64
 *            and is otherwise unspecified) and gam is that vector's quotient.  Informational: not counted by return values > 0.
 *            The derivative of one member of a cluster does not exist: do not hand such a pair to ibs_solve_gcf_vjp_f64.
 *            ibs_solve_gcf_modes_basis_f64 gives the members of a cluster an F-orthonormal Ritz basis of it instead (bits 13, 14).
 *     bits 10-12, ibs_theta0_polish_f64, ibs_marginal_theta0_polish_f64 and ibs_local_eq_boundary_polish_f64 only, per start slot, all informational (not counted by return values > 0): bit 10 = the
 *            coarse node itself was returned (no evaluated point beat it strictly); bit 11 = the search stopped at max_eval;
 *            bit 12 = one-sided bracket (the row ends at the node, or the neighbour on that side is NaN).
 *     bits 13-14, ibs_solve_gcf_modes_basis_f64 only, per mode, both informational (not counted by return values > 0): bit 13 "basis" =
 *            the mode's vector is a member of its cluster's F-orthonormal Ritz basis; bit 14 "open cluster" = the cluster continues
 *            below the last mode asked for, so the basis spans a part of the cluster's invariant subspace.
 *   - idx (nearest-sigma entry points): the number of eigenvalues strictly above the returned one (0 = lam_max); -1 where the status
 *     reports invalid data.  Those entry points return the eigenpair the reference's eigs(A, 1, sigma=sigma0) returns (utils.py:1597)
 *     for every sigma, lam_max's among them; they never set bit 4.
 */
#ifndef IBS_H
#define IBS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IBS_MEM_DEVICE 0
#define IBS_MEM_HOST 1

#define IBS_ERR_ARG (-1)
#define IBS_ERR_HIP (-2)
#define IBS_ERR_UNSUPPORTED (-3)

typedef struct ibs_ctx ibs_ctx;

int ibs_version(void);
const char* ibs_last_error(void);

/* context = device + stream + staging workspace.  One per process/GPU (ball_scan.py runs one
 * process per MPI rank; here one process per GPU). */
int ibs_create(ibs_ctx** ctx, int device_id);
int ibs_destroy(ibs_ctx* ctx);
/* run on an existing hipStream_t (e.g. torch.cuda.current_stream().cuda_stream); NULL = default stream */
int ibs_set_stream(ibs_ctx* ctx, void* hip_stream);
int ibs_synchronize(ibs_ctx* ctx);
int ibs_device_count(void);
/* Bounded quasi-Newton on the two unknowns (alpha, theta0), reverse communication, HOST side (no GPU involved).
 * Replaces: the optimizer behind ball_scan.py:307-314, scipy.optimize.minimize(obj_w_grad, jac=True,
 * bounds=((0, pi), (0, pi/2)), options={ftol, gtol, maxiter}) = scipy's L-BFGS-B (un-vendored dependency: scipy, pinned
 * to 1.15.3 by the build container; algorithm L-BFGS-B 3.0, m = 10, maxls = 20), restated for n = 2 in
 * csrc/ibs_lbfgsb2.hpp.  The same code runs per surface inside ibs_refine_f64; these entry points let a host drive
 * it and let the CPU tests compare its trajectories with scipy's.
 *   state: caller-owned buffer of ibs_lbfgsb2_state_bytes() bytes.
 *   init:  x0 is clipped into [lo, hi]; the first evaluation is wanted at the clipped point (returned by step's
 *          x_next convention: call ibs_lbfgsb2_result() for it, or clip yourself).
 *   step:  hand over (f, g[2]) evaluated at the point last requested; returns 1 = evaluate at x_next[2],
 *          0 = finished (x_next = result).
 *   result: x[2], f, counters[5] = {iterations, evaluations, task code (10 = projected gradient <= gtol,
 *          11 = f reduction <= ftol, 12 = abnormal line-search termination, 13 = maxiter), memory restarts, skipped updates}. */
int ibs_lbfgsb2_state_bytes(void);
int ibs_lbfgsb2_init(void* state, const double* x0, const double* lo, const double* hi, double ftol, double gtol,
                     int32_t maxiter, int32_t maxls);
int ibs_lbfgsb2_step(void* state, double f, const double* g, double* x_next);
int ibs_lbfgsb2_result(const void* state, double* x, double* f, int32_t* counters);

/* Native collective (optional): ONE all-gather of per-surface rows over RCCL on the context's stream, with no host
 * framework in between.  Replaces: the three comm_lead.Gather([x, MPI.DOUBLE], ..., root=0) of ball_scan.py:345-347
 * (theta0*, alpha*, gam per surface) as one all-gather of [n_surf_local][k] doubles per rank.
 *   ibs_comm_load(path)      bind librccl at run time (NULL: the copy the process already holds, else librccl.so.1);
 *   ibs_comm_unique_id(id)   rank 0: 128 bytes to hand to every rank by any means (MPI, a torch.distributed broadcast, a file);
 *   ibs_comm_init(ctx, id, rank, nranks)   collective over the ranks (ncclCommInitRank on the context's device);
 *   ibs_comm_allgather_f64(ctx, send, recv, count)   recv[nranks][count] <- every rank's send[count], device pointers,
 *                            asynchronous on the context's stream (ordered after the kernels that produced `send`);
 *   ibs_comm_allgather_start_f64(ctx, send, recv, count, slot, then_wait_slot)   the same gather, ordered after everything enqueued so
 *                            far on the context's stream but run on the communicator's OWN stream: the next scan does not
 *                            wait for the ranks to meet (the reference has nothing to overlap: its Gather is blocking).
 *                            slot in [0, 16) names the gather; then_wait_slot >= 0 (another slot) additionally does
 *                            ibs_comm_wait(ctx, then_wait_slot) in the same call, -1 = nothing, -2 - s = wait for slot s
 *                            on the HOST instead (event query; blocks only if that gather is still running) so that the
 *                            context's stream carries no wait at all -- for callers running several slots ahead;
 *   ibs_comm_wait(ctx, slot) orders the context's stream after the gather of `slot` (slot < 0: after every pending one)
 *                            without blocking the host: call it before `send` / `recv` of that slot are reused or read;
 *   ibs_comm_destroy(ctx)    (also done by ibs_destroy).
 * The Python layer (BallooningScan, bench.py) uses torch.distributed by default; Context.comm_init(dist) switches it. */
int ibs_comm_load(const char* librccl_path);
int ibs_comm_unique_id(void* id128);
int ibs_comm_init(ibs_ctx* ctx, const void* id128, int32_t rank, int32_t nranks);
int ibs_comm_allgather_f64(ibs_ctx* ctx, const double* send, double* recv, int64_t count_per_rank);
int ibs_comm_allgather_start_f64(ibs_ctx* ctx, const double* send, double* recv, int64_t count_per_rank, int32_t slot,
                                 int32_t then_wait_slot);
int ibs_comm_wait(ibs_ctx* ctx, int32_t slot);
int ibs_comm_destroy(ibs_ctx* ctx);

/* Diagnostic override of a dispatch heuristic of THIS context (tests, experiments; nothing upstream corresponds).
 * name: "force_p" (lanes per system 64|32|16), "scan_chain" (theta0 values chained through one wave),
 * "chain_w1" / "chain_w2" (relative widths of the chain's warm starts), "geo_lpp" (lanes per grid point of the
 * geometry kernel 1|2|4|8, or -2 = two grid points per lane), "gcf_rows" (0: three-row staging instead of the row-streamed raw
 * kernel on long grids), "gcf_direct" (raw systems, one wave per system: rows read straight from global memory instead of staged in LDS; -1 = by
 * batch size, 0 = never, 1 = wherever a one-wave-per-system form would run: not where the sub-wave forms are picked, with a half-grid g, or
 * below the rows-per-lane the direct kernels are built for), "f32_lam" (FP32 eigenvalue-only requests: 1 = all-FP32 iteration + FP64 certificate, 2 = FP64 solver on
 * the FP32 arrays; 0 = form 2 where the 16-lane sub-wave kernels run, else form 1), "reclose" (FP64 raw systems: 1 = a solve whose closing bracket
 * disagrees with its Rayleigh polish is closed again in division form, the default; 2 = only marked with status bit 3 and the distance
 * in bits 5..10; 0 = off, i.e. the round-5 results), "sigma0" (any finite value: solves that return lam and info flag lam_max >= sigma0
 * with the informational status bit 4 -- the nearest-sigma report of the drop-in, utils.py:1597; NaN = off, the default),
 * "sturm_form" (ibs_sturm_count_f64: 1 = prefix-product sweep, 2 = division form with lanes as systems, 3 = division form with one wave
 * per system; 0 = by grid length and batch size, see ibs_sturm_count_f64), "forget_rows" (an action: drop the remembered verdicts on device-resident mode rows, see ibs_fieldline_geometry_f64),
 * "pack_mode" (1|2: hand-off of the fused argmax), "refine_tangent" (refinement: the alpha-tangent of a point
 * staged in LDS, 1, or read from global memory by the sums, 0: two blocks per CU instead of one at N = 969; -1 = by batch size),
 * "scan_resident" (the one-wave-per-system theta0 scan at 3 to 8 rows per lane, N = 131 .. 514: 1 = k_gamma_scan, which carries the rows
 * of its set-up in registers up to the growth-rate stage, wherever it is built; 0 = k_gamma_scan_lean, which rebuilds them, everywhere;
 * -1 = the default: the former while the launch holds at most two waves per SIMD, the latter above; same results bit for bit),
 * "scan_trial_table" (k_gamma_scan: 1 = the start of every lane's trial vector is loaded from a table the context builds on the device once
 * per grid length, the default; 0 = every wave computes it; same results bit for bit);
 * value 0 = automatic (refine_tangent, gcf_direct, scan_resident: -1); value NaN = back to what ibs_create() read from the environment
 * (IBS_FORCE_P, IBS_SCAN_CHAIN, IBS_CHAIN_W1, IBS_CHAIN_W2, IBS_GEO_LPP are read once, there); name "all" with NaN
 * resets every option.  Results never depend on these switches beyond rounding; only the kernel variant does. */
int ibs_set_option(ibs_ctx* ctx, const char* name, double value);

/* Raw (g, c, f) systems -> largest eigenvalue of the tridiagonal pencil and the reference growth rate.
 * Replaces: utils.py:1574-1624 (the part of gamma_ball_full after the coefficient assembly), batched.
 *   lam[n_sys]  matrix eigenvalue lam_max(T, F)            (optional)
 *   gam[n_sys]  Simpson/FD4 Rayleigh quotient (utils.py:1618-1621)  (optional)
 *   X, dX [n_sys][N]  normalised eigenfunction and its derivative (utils.py:1602-1616) (optional)
 *   info[n_sys] (optional) */
int ibs_solve_gcf_f64(ibs_ctx* ctx, int64_t n_sys, int32_t N, double h, const double* g, const double* c,
                      const double* f, int64_t ld, double* lam, double* gam, double* X, double* dX,
                      int32_t* info, int32_t mem);
/* Same with the half-grid values gh[n_sys][ld] (gh[k] between grid points k and k+1, N-1 used) supplied by the
 * caller instead of the mean of neighbouring g: what utils.py:1567-1576 produces for a NON-uniform theta_PEST
 * (coefficients regridded by np.interp onto the uniform grid, g interpolated at the uniform half points). */
int ibs_solve_gcfh_f64(ibs_ctx* ctx, int64_t n_sys, int32_t N, double h, const double* g, const double* gh,
                       const double* c, const double* f, int64_t ld, double* lam, double* gam, double* X, double* dX,
                       int32_t* info, int32_t mem);
/* FP32 form (BASELINE configs[4], the stress leg).  With lam alone (gam, X, dX all null) the shift iteration runs in FP32 --
 * the throughput form -- and EVERY result is then certified in FP64 on the staged rows: one Sturm-count pair at
 * lam32 +- n eps32 ||A|| (n = N - 2) must read (0 above, >= 1 below); a system that fails (an FP32 count off by one between
 * two close eigenvalues would otherwise return lam_2) is solved in FP64 and carries status bit 2.  Hence
 * |lam - lam64| <= n eps32 ||A|| + the rounding of lam to FP32 for every system.  When gam, X or dX is asked for the arrays
 * are widened to FP64 as they are read and the FP64 solver runs on them (FP32 in HBM only; results rounded to FP32; the same
 * kernel forms as the FP64 entry point): an FP32 eigenvector's noise is multiplied by ~N^2 in the FD4 / Simpson quotient, so
 * an all-FP32 growth rate would be noise above N_zeta = 512.  |gam - gam64| <= 1e-6 at every N_zeta on smooth systems. */
int ibs_solve_gcf_f32(ibs_ctx* ctx, int64_t n_sys, int32_t N, float h, const float* g, const float* c,
                      const float* f, int64_t ld, float* lam, float* gam, float* X, float* dX,
                      int32_t* info, int32_t mem);

/* The eigenpair NEAREST sigma[sys] (utils.py:1597: eigs(A, 1, sigma=sigma0)); gh may be NULL (mean of neighbouring g).
 * Arrays as in ibs_solve_gcf_f64 / ibs_solve_gcfh_f64; sigma[n_sys]; idx[n_sys] (conventions above; optional).  FP64, any odd N in
 * [66, 65537], one wavefront per system in division form (csrc/ibs_nearest.hip): |lam - lam_nearest| <= 4 N eps ||A||.  info: bits 0-15
 * = multisection passes in total (two to three multisections per system), status bits 1 (also: sigma not finite) and 5.
 * X is scaled so that its entry of largest magnitude is +1 (an interior eigenfunction changes sign; lam_max's does not). */
int ibs_solve_gcf_nearest_f64(ibs_ctx* ctx, int64_t n_sys, int32_t N, double h, const double* g, const double* gh,
                              const double* c, const double* f, int64_t ld, const double* sigma, double* lam,
                              int32_t* idx, double* gam, double* X, double* dX, int32_t* info, int32_t mem);
/* Spectrum mode: the n_modes LARGEST eigenpairs of every system, 1 <= n_modes <= 16 (else IBS_ERR_ARG).  Nothing upstream corresponds
 * (utils.py:1597 asks ARPACK for one pair); ibs_sturm_count_f64 says how many modes lie above a shift, this returns them.
 * Arrays as in ibs_solve_gcf_nearest_f64 (gh may be NULL).  lam, gam, info [n_sys][n_modes]: mode 0 is lam_max's, the eigenvalues
 * descend; X, dX [n_sys][n_modes][N], scaled so that the entry of largest magnitude is +1.  Every output is optional, at least one
 * must be given.  FP64, any odd N in [66, 65537], one wavefront per system in division form (csrc/ibs_modes.hip): all n_modes
 * brackets are closed by the SAME passes of 64 shifts (simultaneous multisection, csrc/ibs_modes.hpp: 10 passes for one mode, 15-17
 * for eight, against 9-12 each one by one), |lam_m - lam_m(exact)| <= 4 N eps ||A||.  info: bits 0-15 = the passes of the system's
 * multisection (the same in all its modes); status per mode: bit 0 (32 passes did not close the mode's bracket), bit 1 (invalid
 * data: set on all modes of the system, every floating-point output NaN) and the informational bit 9 (clustered: conventions above). */
int ibs_solve_gcf_modes_f64(ibs_ctx* ctx, int64_t n_sys, int32_t N, double h, const double* g, const double* gh,
                            const double* c, const double* f, int64_t ld, int32_t n_modes, double* lam, double* gam,
                            double* X, double* dX, int32_t* info, int32_t mem);
/* The same with an F-orthonormal basis of every CLUSTER of modes (conventions above: bits 9, 13 and 14).  Arguments as
 * ibs_solve_gcf_modes_f64, except: X is required (else IBS_ERR_ARG: the members' vectors are built in the caller's rows) and
 * cluster_first [n_sys][n_modes] (int32, optional) receives the index of the first mode of every mode's cluster, the mode's own index
 * where it is in none.  A cluster: consecutive modes whose closed eigenvalues lie less than tau = 4 N eps ||A|| apart, the last mode
 * alone included where the first eigenvalue NOT asked for lies within tau of it.  Of the same input, lam of every mode, the pass
 * count, status bits 0, 1 and 9 and every output of every mode outside the clusters are ibs_solve_gcf_modes_f64's, bit for bit.  The
 * m <= 16 returned members of a cluster get m vectors of the cluster's invariant subspace (inverse iteration at each member's lam
 * with Gram-Schmidt against the members before it, csrc/ibs_modes_basis.hpp) that are
 *   - F-orthogonal: |<x^_i, x^_j>_F| <= 64 N eps, <x, y>_F = sum f_r x_r y_r over the interior rows, x^ = x / sqrt(<x, x>_F);
 *   - Ritz vectors: |x^_i^T S x^_j| <= 64 N eps ||A|| for i != j, the Ritz values descending with the mode index (an m x m
 *     Rayleigh-Ritz step: the choice is canonical wherever the splitting inside the cluster is resolvable);
 *   - each an eigenvector of its lam to the residual bound of ibs_solve_gcf_vjp_f64; a cluster at most tau / 8 wide: within
 *     max(1e-8, 64 eps ||A|| / gap_out) of the subspace, gap_out = the distance to the nearest eigenvalue outside the cluster;
 *   - scaled so that the entry of largest magnitude is +1; dX and gam are the FD4 / Simpson derivative and quotient of that vector.
 * Their modes carry status bit 13, those of an open cluster bit 14 too.  A member whose vector could not be completed gets bit 0
 * (counted), its lam kept, gam and its X / dX rows NaN; the members found still meet the above.  Results are bitwise repeatable and
 * independent of n_sys and of the system's place in the batch.  A batch without clusters costs what ibs_solve_gcf_modes_f64 costs. */
int ibs_solve_gcf_modes_basis_f64(ibs_ctx* ctx, int64_t n_sys, int32_t N, double h, const double* g, const double* gh,
                                  const double* c, const double* f, int64_t ld, int32_t n_modes, double* lam, double* gam,
                                  double* X, double* dX, int32_t* cluster_first, int32_t* info, int32_t mem);
/* Exact vector-Jacobian product of gam (the FD4 / Simpson quotient of utils.py:1601-1621) and of lam with respect to the rows
 * (g, c, f) of raw systems on a uniform grid, the half-grid g the mean of neighbouring g (the systems of ibs_solve_gcf_f64).  Nothing
 * upstream corresponds: its only derivatives are the Hellmann-Feynman formulas of obj_w_grad (utils.py:1666-1725), which put gam in
 * place of lam and are not the derivative of the gam they come with.
 *   g, c, f, X [n_sys][ld] (X: the eigenvector of lam, any scale and sign; X[0] and X[N-1] are taken as 0); lam[n_sys];
 *   gam_bar[n_sys], lam_bar[n_sys]: the cotangents (either may be NULL = 0, not both);
 *   g_bar, c_bar, f_bar [n_sys][ld] (out): gam_bar d gam / d row + lam_bar d lam / d row, entries 0 .. N-1 of each row (a host call
 *   returns the padding entries N .. ld-1 as 0); info[n_sys] optional.
 * (lam, X) may be ANY simple eigenpair: lam_max's (ibs_solve_gcf_f64, ibs_gamma_points_f64) or the nearest-sigma one
 * (ibs_solve_gcf_nearest_f64, ibs_gamma_points_nearest_f64).  The singular adjoint system (S - lam F) z = d gam / d X is solved by a
 * twisted split at the row of largest |X| with z orthogonal to F X afterwards (csrc/ibs_vjp.hip).  Status: bit 1 = the pair is not an
 * eigenpair of these rows (residual max_r |((S - lam F) X)_r| / f_r above 1024 N eps (||A|| + |lam|) max |X|), invalid data (as in
 * ibs_solve_gcf_f64) or a non-finite lam, X or cotangent: that system's rows are NaN; bit 0 = a pivot of the adjoint solve fell below
 * pivmin and was replaced (the rows may be inaccurate; never on lam_max's pair, whose pivots are bounded away from 0).  FP64, any odd N
 * in [66, 65537] (even N and N outside: IBS_ERR_UNSUPPORTED, as every entry point); one wavefront per system; no floating-point atomics:
 * the rows are bitwise repeatable and independent of the batch. */
int ibs_solve_gcf_vjp_f64(ibs_ctx* ctx, int64_t n_sys, int32_t N, double h, const double* g, const double* c, const double* f,
                          int64_t ld, const double* lam, const double* X, const double* gam_bar, const double* lam_bar, double* g_bar,
                          double* c_bar, double* f_bar, int32_t* info, int32_t mem);
/* the coarse scan of ball_scan.py:248-273 with upstream's shift: sigma[n_lines][n_theta0] (1.0 there, ball_scan.py:230 / 269).
 * Arrays as in ibs_gamma_scan_f64; outputs [n_lines][n_theta0], all optional.  The (g, c, f) rows of whole lines are assembled in a
 * workspace of about 1 GiB at most and solved by the kernel of ibs_solve_gcf_nearest_f64, chunk after chunk (option
 * "nearest_chunk_systems" sets the chunk instead); a chunk of one line that cannot be allocated fails with the bytes it needs. */
int ibs_gamma_scan_nearest_f64(ibs_ctx* ctx, int32_t n_lines, int32_t n_theta0, int32_t N, double h,
                               const double* bmag, const double* gradpar, const double* cvdrift, const double* cvdrift0,
                               const double* gds2, const double* gds21, const double* gds22, int64_t ld,
                               const double* dPdrho, const double* theta0, const double* sigma, double* gam, double* lam,
                               int32_t* idx, int32_t* info, int32_t mem);
/* The n_modes largest eigenvalues and growth rates of every (line, theta0) of a coarse scan (ibs_solve_gcf_modes_f64 on the rows of
 * ibs_gamma_scan_f64's arrays).  gam, lam, info [n_lines][n_theta0][n_modes], all optional, at least one given; no eigenfunctions.
 * Rows of whole lines are assembled and solved chunk after chunk exactly as in ibs_gamma_scan_nearest_f64 (the same workspace bound
 * of about 1 GiB, the same option "nearest_chunk_systems"); the chunking changes no bit of the results. */
int ibs_gamma_scan_modes_f64(ibs_ctx* ctx, int32_t n_lines, int32_t n_theta0, int32_t N, double h,
                             const double* bmag, const double* gradpar, const double* cvdrift, const double* cvdrift0,
                             const double* gds2, const double* gds21, const double* gds22, int64_t ld,
                             const double* dPdrho, const double* theta0, int32_t n_modes, double* gam, double* lam,
                             int32_t* info, int32_t mem);
/* Exact vector-Jacobian product of the whole table of growth rates of a coarse scan: the cotangent gam_bar[n_lines][n_theta0] of
 * gam(line, theta0) carried back to the seven geometry arrays, dPdrho and theta0 of ibs_gamma_scan_f64.  Nothing upstream corresponds
 * (its only derivatives are the Hellmann-Feynman formulas of obj_w_grad at one point per surface, utils.py:1666-1725).
 *   arrays, ld, dPdrho [n_lines], theta0 [n_theta0] (shared by the lines): as in ibs_gamma_scan_f64;
 *   sigma: NULL = lam_max's eigenpair, else [n_lines][n_theta0]: the eigenpair nearest sigma (as ibs_gamma_scan_nearest_f64);
 *   gam_bar [n_lines][n_theta0]: required;
 *   geo_bar [7][n_lines][ld] (out): geo_bar[k][l][j] = sum over theta0 of gam_bar[l][theta0] d gam(l, theta0) / d (array k of line l
 *   at point j), k in the order bmag gradpar cvdrift cvdrift0 gds2 gds21 gds22, entries 0 .. N-1 of each row (a host call returns the
 *   padding entries N .. ld-1 as 0, a device call leaves them alone); dPdrho_bar [n_lines] (out): the same sum for dPdrho (through c);
 *   theta0_bar [n_lines][n_theta0] (out): gam_bar d gam / d theta0 PER SYSTEM (a caller whose lines share theta0 sums over the lines);
 *   each of the three optional, at least one given; gam, lam, info [n_lines][n_theta0] optional.
 * gam is the FD4 / Simpson quotient this call returns (utils.py:1601-1621), the half-grid g the mean of neighbouring g, and the
 * derivative is exact for it; it passes through |gradpar| as d|x| = sgn(x) dx.  The eigenpair is solved here in division form at every
 * N (as ibs_obj_w_grad_exact_f64), so gam may differ from ibs_gamma_scan_f64's in its last digits.  Status (conventions above): the
 * solve's word with the adjoint's two flags at status bits 6 and 7, as ibs_obj_w_grad_exact_f64.  A system with gam_bar exactly 0
 * contributes exactly 0 whatever its status.  A system with a non-zero cotangent whose solve failed (bits 0-1), whose adjoint was
 * refused (bit 7) or whose gam_bar is not finite (sets bit 1) makes the seven rows and dPdrho_bar of ITS line and its own theta0_bar
 * NaN; no other line changes by a bit.  FP64, any odd N in [66, 65537] (even N and N outside: IBS_ERR_UNSUPPORTED).  One wavefront per
 * system (solve, adjoint, theta0 contraction), then one block per line that sums the systems' cotangent rows through the theta0 fold,
 * theta0 ascending (csrc/ibs_scan_vjp.hip); whole lines chunk after chunk under the workspace bound of ibs_gamma_scan_nearest_f64 (the
 * same option "nearest_chunk_systems").  No floating-point atomics: results are bitwise repeatable and independent of the batch, of
 * the order of the lines and of the chunking. */
int ibs_gamma_scan_vjp_f64(ibs_ctx* ctx, int32_t n_lines, int32_t n_theta0, int32_t N, double h,
                           const double* bmag, const double* gradpar, const double* cvdrift, const double* cvdrift0,
                           const double* gds2, const double* gds21, const double* gds22, int64_t ld,
                           const double* dPdrho, const double* theta0, const double* sigma, const double* gam_bar,
                           double* geo_bar, double* dPdrho_bar, double* theta0_bar, double* gam, double* lam, int32_t* info,
                           int32_t mem);
/* ibs_obj_w_grad_f64 with the eigenpair nearest sigma[n_pts] (utils.py:1632-1728 as the refinement of ball_scan.py:305-314 runs it,
 * sigma = 1.3 |gam| + 0.05 of the surface's coarse maximum): geo, theta0, del_alpha, val and jac as in ibs_obj_w_grad_f64; lam,
 * idx and info [n_pts] optional (conventions above: status bits 1 (also: sigma not finite) and 5, idx).  FP64, any odd N in
 * [66, 65537]: one wavefront per point forms dPdrho of the three lines, the centre line's rows, its nearest eigenpair (as
 * ibs_solve_gcf_nearest_f64) and both Hellmann-Feynman derivatives in one kernel (csrc/ibs_nearest_grad.hip).  A point whose solve
 * fails (status bits 0-1) gets val = jac = NaN. */
int ibs_obj_w_grad_nearest_f64(ibs_ctx* ctx, int32_t n_pts, int32_t N, double h, const double* geo, int64_t ld,
                               const double* theta0, const double* sigma, double del_alpha, double* val, double* jac,
                               double* lam, int32_t* idx, int32_t* info, int32_t mem);
/* ibs_gamma_points_f64 with the eigenpair nearest sigma[n_pts] (the final solve of ball_scan.py:322-339: sigma = 0.42 there, the
 * default of gamma_ball_full): one (line, theta0) per point, arrays as in ibs_gamma_points_f64; gam [n_pts] required; lam, idx, info
 * [n_pts] and X, dX [n_pts][N] optional.  The same kernel as ibs_obj_w_grad_nearest_f64 without its gradient pass. */
int ibs_gamma_points_nearest_f64(ibs_ctx* ctx, int32_t n_pts, int32_t N, double h, const double* bmag, const double* gradpar,
                                 const double* cvdrift, const double* cvdrift0, const double* gds2, const double* gds21,
                                 const double* gds22, int64_t ld, const double* dPdrho, const double* theta0, const double* sigma,
                                 double* gam, double* lam, int32_t* idx, double* X, double* dX, int32_t* info, int32_t mem);

/* The objective of the refinement with the EXACT gradient of the gam it returns: utils.py:1632-1728 with the exact derivative in place
 * of the Hellmann-Feynman formulas of utils.py:1676-1680 / 1721-1725 (which put gam in place of lam and are 0.1-5 % off the gam they
 * come with).  geo [n_pts][3][8][ld], theta0 [n_pts], del_alpha, val [n_pts] and jac [n_pts][2] as in ibs_obj_w_grad_f64: val = -gam,
 * jac = (-dgam/dalpha, -dgam/dtheta0) (utils.py:1728).  sigma [n_pts]: the eigenpair nearest sigma (as ibs_obj_w_grad_nearest_f64), or
 * NULL: lam_max's (as ibs_obj_w_grad_f64).  gam, lam, idx (0 with sigma = NULL) and info [n_pts] optional.  FP64, any odd N in
 * [66, 65537] (even N and N outside: IBS_ERR_UNSUPPORTED): one wavefront per point forms dPdrho of the three lines, the centre line's
 * rows, the eigenpair in division form (lam_max: as the long-grid path of ibs_solve_gcf_f64, at every N), d gam / d (g, c, f) (as
 * ibs_solve_gcf_vjp_f64 with gam_bar = 1) and its contractions with the theta0 tangent (utils.py:1669-1673) and the alpha tangent
 * (right minus left line, each with its own dPdrho, over del_alpha: utils.py:1683-1718) in one kernel (csrc/ibs_exact_grad.hip); the
 * derivative in theta0 is exact, in alpha that of the reference's central difference of the rows.  No floating-point atomics: results
 * are bitwise repeatable and independent of the batch.  Status (conventions above): a point whose solve fails (bits 0-1; also theta0 or
 * sigma not finite) gets val = jac = NaN; bit 7 (the adjoint refused the pair) gives jac = NaN with val kept; bits 5 and 6 are
 * informational. */
int ibs_obj_w_grad_exact_f64(ibs_ctx* ctx, int32_t n_pts, int32_t N, double h, const double* geo, int64_t ld,
                             const double* theta0, const double* sigma, double del_alpha, double* val, double* jac,
                             double* gam, double* lam, int32_t* idx, int32_t* info, int32_t mem);

/* ibs_obj_w_grad_exact_f64 with the derivative in alpha exact as well, from ONE field line per point.
 * Replaces: the central difference of the rows over del_alpha of utils.py:1683-1718 (and the two side lines of utils.py:1641-1646) by
 * the contraction of d gam / d (g, c, f) with the alpha-derivative of the rows, formed from geo_da = the output of
 * ibs_fieldline_geometry_dalpha_f64 for the same lines; d|gradpar| = sgn(gradpar) d gradpar, and dPdrho is held fixed (it does not
 * depend on alpha).  There is no del_alpha.
 *   geo, geo_da [8][n_pts][ld]: the layout both geometry calls write (plane k of point p at (k n_pts + p) ld), no permuted copy;
 *   theta0, sigma, val, jac, gam, lam, idx, info: exactly as in ibs_obj_w_grad_exact_f64, status bits included.  val, gam, lam, idx,
 *   info and jac[.][1] are the bits ibs_obj_w_grad_exact_f64 gives on the same centre line.  A non-finite entry of geo_da gives
 *   jac[p][0] = NaN and nothing else.
 * FP64, any odd N in [66, 65537] (even N and N outside: IBS_ERR_UNSUPPORTED, checked before the context is touched): one wavefront
 * per point, the stages and the workspace of ibs_obj_w_grad_exact_f64 (csrc/ibs_exact_tangent.hip).  No floating-point atomics:
 * results are bitwise repeatable and independent of the batch. */
int ibs_obj_w_grad_exact_tangent_f64(ibs_ctx* ctx, int32_t n_pts, int32_t N, double h, const double* geo, const double* geo_da,
                                     int64_t ld, const double* theta0, const double* sigma, double* val, double* jac,
                                     double* gam, double* lam, int32_t* idx, int32_t* info, int32_t mem);

/* Marginal stability of raw systems: the factor s* by which c (i.e. the pressure gradient: c is linear in dPdrho, utils.py:1560-1562)
 * may be scaled, at fixed g, before the system goes unstable; s* < 1 = unstable now.  Nothing upstream corresponds: the quantity
 * generalises the marginal-stability scan of the reference's s-alpha test (bishop_ball_s-alpha.py:90-115), which only reports a
 * boolean per (shat, alpha).  With D the stiffness matrix of utils.py:1574-1592 on a uniform grid (e_k = (g_k + g_{k+1}) / 2 h^2,
 * D_jj = e_{j-1} + e_j, D_{j,j+-1} = -e) and C = diag(c_j) on the interior points, s* = inf { s > 0 : lam_max(s C - D) >= 0 } =
 * 1 / mu_max of C x = mu D x; f plays no part (f > 0 only scales rows).
 *   g, c [n_sys][ld]; scale [n_sys] (required); mu [n_sys] = 1 / s* (0 with status bit 8); gam0 [n_sys]: the FD4 / Simpson quotient
 *   of utils.py:1601-1621 of the marginal mode on the rows (g, s* c, 1), O(h^2) from 0 (a diagnostic); X [n_sys][N]: the marginal
 *   mode, zero ends, largest entry +1; g_bar, c_bar [n_sys][N]: d s* / d g and d s* / d c, exact for the discrete pencil
 *   (Hellmann-Feynman: no adjoint solve, no floating-point atomics, bitwise repeatable and independent of the batch); info [n_sys]:
 *   bits 0-15 = multisection passes, status bits 0, 1 (invalid data: a non-finite entry or g <= 0; c may have any sign) and 8.
 * Everything but scale is optional.  FP64, any odd N in [66, 65537] (even N and N outside: IBS_ERR_UNSUPPORTED), one wavefront per
 * system in division form (csrc/ibs_marginal.hip): 64-way multisection on "s C - D has a positive eigenvalue" to a width of 8 eps s*. */
int ibs_marginal_gcf_f64(ibs_ctx* ctx, int64_t n_sys, int32_t N, double h, const double* g, const double* c, int64_t ld,
                         double* scale, double* mu, double* X, double* gam0, double* g_bar, double* c_bar, int32_t* info, int32_t mem);
/* The same margin of every (line, theta0) of a geometry-fed scan: arrays as in ibs_gamma_scan_f64, outputs [n_lines][n_theta0];
 * s* scales dPdrho[line] at fixed geometry arrays (dPdrho_crit = s* dPdrho).  Nothing upstream corresponds (utils.py:1560-1562 and
 * bishop_ball_s-alpha.py:90-115 are what the quantity generalises).  scale required; mu, dscale_dtheta0 (the derivative rows of
 * ibs_marginal_gcf_f64 contracted with the theta0 tangent of utils.py:1669-1673), dscale_ddPdrho (= -s* / dPdrho) and info optional.
 * One wavefront per (line, theta0) forms the rows and solves them in one kernel.  A real equilibrium's geometry moves with its
 * pressure: s* = 1 marks the true boundary, s* != 1 is a local, frozen-geometry margin. */
int ibs_marginal_scan_f64(ibs_ctx* ctx, int32_t n_lines, int32_t n_theta0, int32_t N, double h, const double* bmag,
                          const double* gradpar, const double* cvdrift, const double* cvdrift0, const double* gds2,
                          const double* gds21, const double* gds22, int64_t ld, const double* dPdrho, const double* theta0,
                          double* scale, double* mu, double* dscale_dtheta0, double* dscale_ddPdrho, int32_t* info, int32_t mem);
/* The objective of the refinement of the margin in (alpha, theta0), at geometry-fed points: geo, theta0 and del_alpha as in
 * ibs_obj_w_grad_exact_f64 (geo [n_pts][3][8][ld]: the lines alpha - del_alpha / 2, alpha, alpha + del_alpha / 2).  The objective is
 * the marginal eigenvalue mu = 1 / s*, not s*: mu is finite everywhere (0 where no scale makes the line unstable), so a minimiser
 * can cross a stable region.  Nothing upstream corresponds; the tangents are those of utils.py:1669-1673 (theta0) and 1683-1718
 * (alpha: each side line with its own dPdrho, divided by del_alpha).
 *   val [n_pts] = -mu (required); jac [n_pts][2] = -(d mu / d alpha, d mu / d theta0) = dscale / s*^2; scale [n_pts] = s*;
 *   dscale [n_pts][2] = (d s* / d alpha, d s* / d theta0), Hellmann-Feynman on the discrete pencil (fixed-order sums: bitwise
 *   repeatable and independent of the batch); dPdrho [n_pts]: the centre line's, so that dPdrho_crit = s* dPdrho; info [n_pts]:
 *   bits 0-15 = multisection passes, status bits 0, 1 and 8.  Everything but val is optional; with jac and dscale both NULL the side
 *   lines are not read and no mode is formed (the point-evaluation form).
 *   Status bit 8: scale = +inf, val = 0, jac = dscale = 0 (not counted).  Bits 0-1 of the centre solve: every floating-point output of
 *   the point is NaN.  A gradient that is not finite after a good centre solve: bit 1, jac = dscale = NaN, val and scale kept.
 * FP64, any odd N in [66, 65537], one wavefront per point (k_marginal_points, csrc/ibs_marginal_points.hip).  The frozen-geometry caveat of
 * ibs_marginal_scan_f64 applies. */
int ibs_marginal_obj_w_grad_f64(ibs_ctx* ctx, int32_t n_pts, int32_t N, double h, const double* geo, int64_t ld,
                                const double* theta0, double del_alpha, double* val, double* jac, double* scale, double* dscale,
                                double* dPdrho, int32_t* info, int32_t mem);
/* ibs_marginal_obj_w_grad_f64 with the derivative in alpha exact as well, from ONE field line per point, and the cotangent of s* in the
 * geometry arrays.
 * Replaces: the del_alpha difference of the rows of two side lines (utils.py:1683-1718 and the side lines of utils.py:1641-1646) by the
 * contraction of d s* / d (g, c) with the alpha-derivative of the rows, formed from geo_da = the output of
 * ibs_fieldline_geometry_dalpha_f64 for the same lines; d|gradpar| = sgn(gradpar) d gradpar, and dPdrho is held fixed (it does not
 * depend on alpha).  There is no del_alpha.  s* is an eigenvalue of the discrete pencil, so Hellmann-Feynman is exact: dscale is the
 * derivative of the scale returned in BOTH variables, with no adjoint solve.
 *   geo, geo_da [8][n_pts][ld]: the layout both geometry calls write (plane k of point p at (k n_pts + p) ld), no permuted copy;
 *   geo_da may be NULL only when jac and dscale both are (else IBS_ERR_ARG);
 *   theta0, val (required), jac, scale, dscale, dPdrho, info: as in ibs_marginal_obj_w_grad_f64.  val, scale, dPdrho, info, jac[.][1]
 *   and dscale[.][1] are what ibs_marginal_obj_w_grad_f64 gives on the same centre line;
 *   geo_bar [8][n_pts][ld] (optional): the derivative of scale[p] in every entry of the eight arrays of point p that were read, the
 *   dependence through the line's own dPdrho included -- pass it to ibs_fieldline_geometry_vjp_f64 with dPdrho_bar = NULL to get
 *   d s* / d (tab_mn, tab_nyq, scal, alpha).  Closed form per grid point from the marginal mode (csrc/ibs_marginal_tangent.hip); entries
 *   N .. ld-1 of a row are never written, with host pointers either.
 *   With jac, dscale and geo_bar all NULL no mode is formed (the point-evaluation form).
 *   Status bit 8: scale = +inf, val = 0, jac = dscale = 0, zero geo_bar rows (not counted).  Bits 0-1 of the solve: every floating-point
 *   output of the point is NaN, its geo_bar rows (entries 0 .. N-1) included.  A gradient that is not finite after a good solve (a
 *   non-finite entry of geo_da): bit 1, jac = dscale = NaN; val, scale and geo_bar kept.
 * FP64, any odd N in [66, 65537] (even N and N outside: IBS_ERR_UNSUPPORTED; this and the argument checks run before the context is
 * touched), one wavefront per point (k_marginal_tangent_points), the workspace of ibs_marginal_obj_w_grad_f64.  No floating-point
 * atomics: results are bitwise repeatable and independent of the batch.  The frozen-geometry caveat of ibs_marginal_scan_f64 applies. */
int ibs_marginal_obj_w_grad_tangent_f64(ibs_ctx* ctx, int32_t n_pts, int32_t N, double h, const double* geo, const double* geo_da,
                                        int64_t ld, const double* theta0, double* val, double* jac, double* scale, double* dscale,
                                        double* dPdrho, double* geo_bar, int32_t* info, int32_t mem);

/* Local-equilibrium scan: the s-alpha picture of a real field line -- gam, lam_max and the number of eigenvalues above `shift` of every
 * line under variations of its surface's global shear and pressure gradient about the equilibrium, from the line's eight arrays alone
 * (no geometry launch per shear value).  Nothing upstream corresponds for a real line: bishop_ball_s-alpha.py does the analytic
 * shifted-circle model only.  THE RULE (csrc/ibs_local_eq.hpp; numpy: ibs_amd.operators.local_eq_fold), per line and variation v =
 * (theta0, eps, p), eps = the relative change of the shear, p = the factor on the pressure gradient, theta_j = theta_lo + j h:
 *     x_j   = theta0 (1 + eps) + sigma eps (theta_j - centre) + (p - 1) ps_j
 *     cv'_j = gbdrift_j + p (cvdrift_j - gbdrift_j) + x_j cvdrift0_j
 *     gd'_j = gds2_j + 2 x_j gds21_j + x_j^2 gds22_j
 *     dP'   = p dPdrho
 *     g = |gradpar| gd' / bmag,  c = -dP' cv' / (|gradpar| bmag),  f = gd' / bmag^2 / (|gradpar| bmag)          (utils.py:1560-1562)
 * then the operator of every other entry point: half-grid g = mean of neighbours, lam_max of (T, F), gam by the FD4 + Simpson quotient
 * (utils.py:1574-1621).  eps = 0, p = 1, ps = NULL: the fold of ibs_gamma_scan_f64.  ps = NULL, centre = alpha: the geometry
 * re-evaluated with d_iota_d_s (1 + eps) and d_pressure_d_s p (scal columns 2, 3 of ibs_fieldline_geometry_f64) and folded at theta0,
 * the ballooning angle of the varied equilibrium -- a frozen-local-shear variation on the pressure axis (the caveat of
 * ibs_marginal_scan_f64).  ps: the change of the integrated local shear per unit of (p - 1), in units of the fold variable, from a
 * local-equilibrium code; the s-alpha model's row is -alpha0 (sin theta - sin theta0) / shat0.  eps is relative to the surface's own
 * shear: on a surface with shat -> 0 the shear axis degenerates (gds21, gds22, cvdrift0 vanish).
 *   geo [8][n_lines][ld]: bmag gradpar cvdrift cvdrift0 gds2 gds21 gds22 gbdrift, as ibs_fieldline_geometry_f64 writes them;
 *   dPdrho, centre (= alpha for lines of ibs_fieldline_geometry_f64), sigma (= sign(-phiedge), +1 or -1) [n_lines];
 *   ps [n_lines][ps_ld >= N] or NULL (= 0); var [n_var][3] = (theta0, eps, p); shift: a HOST scalar, finite if count is given;
 *   gam, lam, count, info [n_lines][n_var]; gam, lam and count may each be NULL, not all three (IBS_ERR_ARG).  count alone: no
 *   eigenvalue is computed -- the stable / unstable diagram at one pass over the rows per system;
 *   info: bits 0-15 = multisection passes, status bits 0 (iteration cap), 1 (a line with non-finite data or g, f <= 0, sigma not +-1,
 *   a non-finite triple: NaN gam and lam, count -1, of those systems only);
 *   flags: IBS_MEM_DEVICE or IBS_MEM_HOST, the `mem` of the other entry points (anything else: IBS_ERR_ARG).
 * FP64, uniform grids, any odd N in [66, 65537] (even N and N outside: IBS_ERR_UNSUPPORTED); a NULL required argument, ld < N, ps_ld < N,
 * n_var < 1: IBS_ERR_ARG; all of these run before the context is touched.  One wavefront per (line, variation) forms the rows and
 * solves them in division form in one kernel (k_local_eq_scan, csrc/ibs_local_eq.hip).  No atomics: a system's outputs depend on its
 * line and its triple alone, bit for bit -- not on the batch, the order of the lines or the chunks of whole lines the call is worked
 * through in when its workspace would exceed the budget (option "nearest_chunk_systems" sets the chunk). */
int ibs_local_eq_scan_f64(ibs_ctx* ctx, int32_t n_lines, int32_t n_var, int32_t N, double theta_lo, double h, const double* geo,
                          int64_t ld, const double* dPdrho, const double* centre, const double* sigma, const double* ps,
                          int64_t ps_ld, const double* var, double shift, double* gam, double* lam, int32_t* count, int32_t* info,
                          int flags);

/* Local-equilibrium boundaries: the CURVE of the s-alpha picture where ibs_local_eq_scan_f64 gives the raster -- the parameters at which
 * every line crosses the stability boundary along straight rays in the (eps, p) plane of the rule above, closed to rounding on the
 * device.  A ray is seven doubles (theta0, eps0, p0, d_eps, d_p, t_lo, t_hi), t_lo < t_hi; the triple at parameter t is (theta0,
 * eps0 + t d_eps, p0 + t d_p), the rows at t are those of the rule at that triple and the operator is the one every entry point solves.
 * The pressure axis at fixed shear: d_eps = 0, d_p = 1; the shear axis: d_eps = 1, d_p = 0; oblique rays are allowed; theta0 does not vary
 * along a ray (the fold variable stays linear in t; numpy: ibs_amd.operators.local_eq_ray_triples).  The verdict at t is "the pencil has
 * an eigenvalue above `shift`" (count > 0).
 *   inputs up to ps_ld: as ibs_local_eq_scan_f64; rays [n_ray][7]; shift: a HOST scalar, finite; max_cross in [1, 4]; xtol in [0, 1);
 *   t_stable, t_unstable [n_lines][n_ray][max_cross]: the two ends of each closed bracket, by verdict, in increasing t; NaN beyond n_cross;
 *   n_cross [n_lines][n_ray]: crossings returned (all three required);
 *   lo_unstable [n_lines][n_ray] or NULL: the verdict at t_lo;
 *   node_count [n_lines][n_ray][64] or NULL: the counts above shift at the nodes t_lo + k (t_hi - t_lo) / 63 of pass 0 -- the diagram row
 *   at node resolution, for free;
 *   info [n_lines][n_ray] or NULL: bits 0-15 = passes over the rows; status bits 0 (a crossing was not closed in 12 passes), 1 (invalid:
 *   non-finite data in the line, g or f <= 0 at any evaluated t, sigma not +-1, a non-finite ray, t_lo >= t_hi -- NaN parameters, n_cross,
 *   lo_unstable and node counts -1, of that system alone), 2 (more than max_cross crossings: the first max_cross are returned), 3 (the
 *   bracket's ends became FP64 neighbours before xtol was met; always with xtol = 0);
 *   flags: IBS_MEM_DEVICE or IBS_MEM_HOST.
 * Pass 0 puts the 64 lanes of a wavefront at the 64 nodes; a crossing is an adjacent node pair with different verdicts.  Each kept
 * crossing is closed in turn: 64 points strictly inside the bracket, the new bracket = the first adjacent pair (ends included) whose
 * verdicts differ, until its width is <= xtol (t_hi - t_lo): six passes for 1e-12.  LIMITS: a tangency (double root) and two crossings
 * between one pair of nodes are missed -- narrow the range or split the ray; within rounding of the marginal point the verdict may
 * flicker, and the first flip is returned; theta0 is fixed per ray; ps is consumed, not computed; the derivatives of t*
 * are a second call, ibs_local_eq_grad_f64 at the returned crossings (below).
 * FP64, uniform grids, any odd N in [66, 65537] (even N and N outside: IBS_ERR_UNSUPPORTED); a NULL required argument, ld < N, ps_ld < N,
 * n_ray < 1, max_cross outside [1, 4], xtol outside [0, 1), a non-finite shift: IBS_ERR_ARG; all of these run before the context is
 * touched.  One wavefront per (line, ray) (k_local_eq_boundary, csrc/ibs_local_eq_boundary.hip; the staged form:
 * csrc/ibs_local_eq_boundary.hpp), no atomics, no workspace: a system's outputs depend on its line and its ray alone, bit for bit --
 * not on the batch, the order of the lines or the chunks of whole lines (option "nearest_chunk_systems"). */
int ibs_local_eq_boundary_f64(ibs_ctx* ctx, int32_t n_lines, int32_t n_ray, int32_t N, double theta_lo, double h, const double* geo,
                              int64_t ld, const double* dPdrho, const double* centre, const double* sigma, const double* ps,
                              int64_t ps_ld, const double* rays, double shift, int32_t max_cross, double xtol, double* t_stable,
                              double* t_unstable, int32_t* n_cross, int32_t* lo_unstable, int32_t* node_count, int32_t* info,
                              int flags);

/* Local-equilibrium boundaries minimised over theta0: the first-stability parameter of every (line, ray family) BETWEEN the nodes of a
 * coarse theta0 grid -- the envelope over theta0 that the boundary of an s-alpha picture is by convention.  The rule is stated once in
 * csrc/ibs_local_eq_boundary_polish.hpp (Python: ibs_amd.scan.polish_first_up).  A family is a ray of ibs_local_eq_boundary_f64 whose entry
 * 0 is ignored and replaced by the theta0 under evaluation.  T(theta0) is what ibs_local_eq_boundary_f64 gives for that ray with
 * max_cross = 1, bit for bit (every evaluation is cold): t_lo where the ray is unstable at t_lo, else (t_stable[0] + t_unstable[0]) / 2,
 * else +inf; an evaluation with status bit 0 or 1 is a failed one.  f = -T is maximised by the rule of ibs_theta0_polish_f64 unchanged
 * (peaks of the coarse row, n_starts <= 4 slots, the bracket between the neighbouring nodes, Brent's bounded search on the absolute
 * tolerance xtol_theta0, at most max_eval <= 64 evaluations, the incumbent rule), with one addition: a slot whose node already has
 * T = t_lo is returned at once, no evaluation, bit 10.
 *   inputs up to ps_ld: as ibs_local_eq_boundary_f64; rays [n_ray][7]; theta0 [n_theta0], finite and strictly increasing,
 *   n_theta0 in [1, 2520]; t_row [n_lines][n_ray][n_theta0] = T at the nodes (+inf: no crossing; t_lo: unstable at t_lo; NaN: not to be
 *   used), e.g. from one ibs_local_eq_boundary_f64 call; shift, xtol: as ibs_local_eq_boundary_f64;
 *   theta0_out, t_out, t_stable_out, t_unstable_out [n_lines][n_ray][n_starts] (required): theta0*, T(theta0*) -- never above the node's
 *   -- and the two ends of the first crossing of the evaluation at theta0* (NaN without one, and after the early return);
 *   node, n_eval, lo_unstable, info [n_lines][n_ray][n_starts], n_found [n_lines][n_ray], each or NULL: the slot's node (-1: the row has
 *   no usable node; NaN outputs), the evaluations of the search, the verdict at t_lo of the evaluation at theta0*, bits 0-15 = passes
 *   over the rows of the search | status << 16, and the peaks of the row; slots from n_found on repeat slot 0.
 *   Status bits 0 (the pass cap in some evaluation) and 1 (invalid data in some evaluation, a non-finite family, t_lo >= t_hi, sigma not
 *   +-1, theta0 not increasing: NaN outputs, lo_unstable -1, of that slot alone) are failures; bit 3 (some bracket's ends became FP64
 *   neighbours before xtol) and bits 10 (the node itself is returned: t_out is the row's entry, and one more evaluation at the node, not
 *   counted in n_eval, supplies the ends), 11 (max_eval reached) and 12 (one-sided bracket) are informational.
 *   flags: IBS_MEM_DEVICE or IBS_MEM_HOST.  Host pointers: returns the number of slots with status bit 0 or 1.
 * LIMITS: theta0 alone is polished; a peak is a local maximum of the row's NODES; the tangency limit of the ray rule holds in every
 * evaluation; T(theta0) is continuous only while the first crossing stays the same branch; the cost is n_eval boundary closures.
 * FP64, uniform grids, any odd N in [66, 65537] (even N and N outside: IBS_ERR_UNSUPPORTED); a NULL required argument, ld < N, ps_ld < N,
 * n_ray < 1, n_theta0 outside [1, 2520], n_starts outside [1, 4], max_eval outside [1, 64], xtol_theta0 <= 0 or non-finite, xtol outside
 * [0, 1), a non-finite shift: IBS_ERR_ARG; all of these run before the context is touched.  One wavefront per (line, family, slot)
 * (k_local_eq_boundary_polish, csrc/ibs_local_eq_boundary_polish.hip), no atomics, no workspace: a slot's outputs depend on its line, its
 * family, its row and its slot alone, bit for bit -- not on the batch, the order of the lines or the chunks of whole lines. */
int ibs_local_eq_boundary_polish_f64(ibs_ctx* ctx, int32_t n_lines, int32_t n_ray, int32_t N, double theta_lo, double h, const double* geo,
                                     int64_t ld, const double* dPdrho, const double* centre, const double* sigma, const double* ps,
                                     int64_t ps_ld, const double* rays, int32_t n_theta0, const double* theta0, const double* t_row,
                                     double shift, double xtol, int32_t n_starts, double xtol_theta0, int32_t max_eval,
                                     double* theta0_out, double* t_out, double* t_stable_out, double* t_unstable_out, int32_t* node,
                                     int32_t* n_eval, int32_t* lo_unstable, int32_t* info, int32_t* n_found, int flags);

/* Local-equilibrium gradients: lam_max of the rule above at POINTS (line, theta0, eps, p) with its EXACT derivatives -- the derivatives
 * the scan and the boundaries lack.  lam_max is a simple eigenvalue of the discrete pencil with mode X (X_0 = X_{N-1} = 0), and
 *     lam = (sum c_j X_j^2 - 1/2 h^-2 sum g_j w_j) / q,   q = sum f_j X_j^2,   w_j = (X_j - X_{j-1})^2 + (X_{j+1} - X_j)^2
 * so d lam / d s = (sum c_s X^2 - 1/2 h^-2 sum g_s w - lam sum f_s X^2) / q for every parameter s of the rows (Hellmann-Feynman), exact
 * for the lam returned to first order in the error of X.  The row tangents are polynomial (csrc/ibs_local_eq_grad.hpp; numpy:
 * ibs_amd.operators.local_eq_fold_tangent, local_eq_lam_grad).  Along a ray of ibs_local_eq_boundary_f64 every crossing is
 * lam_max(t*) = shift; with lam_t = d_eps lam_eps + d_p lam_p the implicit-function theorem gives d t* / d theta0 = -lam_theta0 / lam_t,
 * d t* / d eps0 = -lam_eps / lam_t, d t* / d p0 = -lam_p / lam_t, d t* / d shift = 1 / lam_t, d t* / d dPdrho = -lam_dP / lam_t and
 * d t* / d (arrays) = -geo_bar / lam_t (the host composition: ibs_amd Context.local_eq_boundary_grad).
 *   inputs up to ps_ld: as ibs_local_eq_scan_f64 -- ONE staged geometry serves any number of points;
 *   line_of int32 [n_pts]: the line of each point; var [n_pts][3] = (theta0, eps, p) of each point;
 *   lam, gam [n_pts]; dlam [n_pts][4] = d lam / d (theta0, eps, p, dPdrho);
 *   geo_bar [8][n_pts][ld_bar >= N] or NULL: d lam / d (every entry of the line's eight arrays), plane k = array k in the order of geo;
 *   entries N .. ld_bar-1 of a row are never written.  lam, gam, dlam and geo_bar may each be NULL, not all four (IBS_ERR_ARG).  With
 *   dlam and geo_bar both NULL no mode is kept and lam, gam are the bits of ibs_local_eq_scan_f64 at that line and triple;
 *   info [n_pts] or NULL: bits 0-15 = multisection passes, status bits 0 (iteration cap), 1 (a line with non-finite data or g, f <= 0,
 *   sigma not +-1, a non-finite triple, line_of outside [0, n_lines)): NaN in every floating-point output of those points alone, entries
 *   0 .. N-1 of their geo_bar rows included; the line of an index out of range is never read;
 *   flags: IBS_MEM_DEVICE or IBS_MEM_HOST.  Host pointers: returns the number of points with status bit 0 or 1.
 * LIMITS: the derivative of lam_max, not of gam; lam_max must be simple -- on a doublet of a symmetric line the derivative of one member
 * does not exist, and nothing detects it; at a tangency of a ray lam_t -> 0 and the d t* are inf or NaN by arithmetic; ps is consumed,
 * not differentiated.
 * FP64, uniform grids, any odd N in [66, 65537] (even N and N outside: IBS_ERR_UNSUPPORTED); a NULL required argument, ld < N, ps_ld < N,
 * ld_bar < N with geo_bar, n_lines < 0, n_pts < 0: IBS_ERR_ARG; n_pts = 0 does nothing; all of these run before the context is touched.
 * One wavefront per point (k_local_eq_grad, csrc/ibs_local_eq_grad.hip): k_local_eq_scan's stages with the mode kept, then five
 * lane-strided sums and the wave reduction in a fixed order.  No atomics: a point's outputs depend on the point and its line alone, bit
 * for bit -- not on the batch, the order of the points or the chunks of points the call is worked through in (option
 * "nearest_chunk_systems" sets the chunk). */
int ibs_local_eq_grad_f64(ibs_ctx* ctx, int32_t n_lines, int32_t n_pts, int32_t N, double theta_lo, double h, const double* geo,
                          int64_t ld, const double* dPdrho, const double* centre, const double* sigma, const double* ps, int64_t ps_ld,
                          const int32_t* line_of, const double* var, double* lam, double* gam, double* dlam, double* geo_bar,
                          int64_t ld_bar, int32_t* info, int flags);

/* Field-line geometry x theta0 grid -> growth rates.
 * Replaces: the inner loops of ball_scan.py:248-275 (theta0 fold :267-268, gamma_ball_full call :269)
 * and utils.py:1556-1624; with dgam_dtheta0 also utils.py:1666-1680 (Hellmann-Feynman d/dtheta0).
 *   dgam_dtheta0 keeps the reference's formula (gam in place of lam, Simpson sums): it is NOT the derivative of the gam returned;
 *   the exact one is the rows' theta0 tangents contracted with ibs_solve_gcf_vjp_f64's rows (ibs_amd.autograd.growth_rate).
 *   geometry arrays [n_lines][ld] (first N of each row used): bmag, gradpar (gradpar_theta_pest),
 *   cvdrift, cvdrift0, gds2, gds21, gds22;  dPdrho[n_lines] (ball_scan.py:262);  theta0[n_theta0].
 *   outputs are [n_lines][n_theta0] (X, dX: [n_lines][n_theta0][N]). */
int ibs_gamma_scan_f64(ibs_ctx* ctx, int32_t n_lines, int32_t n_theta0, int32_t N, double h,
                       const double* bmag, const double* gradpar, const double* cvdrift, const double* cvdrift0,
                       const double* gds2, const double* gds21, const double* gds22, int64_t ld,
                       const double* dPdrho, const double* theta0, double* gam, double* lam, double* X,
                       double* dX, double* dgam_dtheta0, int32_t* info, int32_t mem);

/* Same scan, warm-started: lam_guess[n_lines][n_theta0] holds the eigenvalues of a nearby problem (the
 * previous optimizer iteration, or the base equilibrium when one of the DOF-perturbed equilibria of
 * sims_runner_NCSX.py:151-276 is re-scanned) and guess_width their expected absolute change.  The result
 * is certified exactly as in the cold scan (a wrong guess costs sweeps, never correctness). */
int ibs_gamma_scan_warm_f64(ibs_ctx* ctx, int32_t n_lines, int32_t n_theta0, int32_t N, double h,
                            const double* bmag, const double* gradpar, const double* cvdrift, const double* cvdrift0,
                            const double* gds2, const double* gds21, const double* gds22, int64_t ld,
                            const double* dPdrho, const double* theta0, const double* lam_guess, double guess_width,
                            double* gam, double* lam, double* X, double* dX, double* dgam_dtheta0, int32_t* info,
                            int32_t mem);

/* Scan + per-surface first maximum in ONE call (device pointers only): the lines are ordered surface-major,
 * n_lines / n_surf consecutive lines form a surface, and pack[n_surf][2] = (max gam of the surface's (alpha, theta0)
 * table, its first row-major index as a double) -- the buffer the per-surface all-gather sends.
 * Replaces: ball_scan.py:248-295 (coarse scan loops + argmax with the first-maximum rule :283-288) for all surfaces of a
 * rank at once.  For small batches this is a single kernel launch: the thread block that completes a surface reduces
 * it (agent-scope release / acquire on a per-surface arrival counter); large batches run the chained / sub-wave scan
 * kernels followed by the reduction kernel.  * The arrival counters are per (context, stream): launches of one context on ONE stream are ordered and may be queued
 * back to back; the same context used under two streams gets two counter sets.  A launch that faults leaves its
 * counters undefined: destroy the context. */
int ibs_gamma_scan_argmax_f64(ibs_ctx* ctx, int32_t n_lines, int32_t n_theta0, int32_t N, double h,
                              const double* bmag, const double* gradpar, const double* cvdrift, const double* cvdrift0,
                              const double* gds2, const double* gds21, const double* gds22, int64_t ld,
                              const double* dPdrho, const double* theta0, int32_t n_surf, double* gam, double* lam,
                              double* pack, int32_t* info);

/* One (field line, theta0) PAIR per point: growth rates of n_pts lines, line i at its own theta0[i].
 * Replaces: the final solve of ball_scan.py:322-339 (one more vmec_fieldlines + gamma_ball_full at the refined
 * (alpha*, theta0*) of every surface) for all surfaces of a rank -- or of all equilibria of an optimizer step -- at once.
 * Arrays as in ibs_gamma_scan_f64 with n_lines = n_pts ([n_pts][ld]); theta0[n_pts]; outputs [n_pts] (X, dX: [n_pts][N]). */
int ibs_gamma_points_f64(ibs_ctx* ctx, int32_t n_pts, int32_t N, double h, const double* bmag, const double* gradpar,
                         const double* cvdrift, const double* cvdrift0, const double* gds2, const double* gds21,
                         const double* gds22, int64_t ld, const double* dPdrho, const double* theta0, double* gam,
                         double* lam, double* X, double* dX, double* dgam_dtheta0, int32_t* info, int32_t mem);

/* Lines on a NON-UNIFORM theta grid.
 * Replaces: utils.py:1565-1576 -- gamma_ball_full takes any increasing theta_PEST and regrids before it solves: g, c, f by np.interp
 * onto np.linspace(theta[0], theta[-1], N), g once more at the uniform half points, h = np.diff(th_half)[2] -- batched on the device
 * (csrc/ibs_regrid.hpp states the arithmetic with its rounding, csrc/ibs_regrid.hip runs it).  The four entry points share
 *   theta, theta_ld: the grids; theta_ld = 0: theta[N], one grid shared by all lines, theta_ld >= N: one row per line (per system of
 *     ibs_regrid_rows_f64), theta_ld apart (anything else: IBS_ERR_ARG);
 *   theta_lo, theta_hi: HOST scalars, the window every line shares (finite, theta_hi > theta_lo, else IBS_ERR_ARG): every grid must have
 *     theta[0] == theta_lo and theta[N-1] == theta_hi.  h is a host scalar everywhere in this library, so it is not read from device memory;
 *   h_out: host pointer, optional: the spacing to hand to the raw solvers with the rows.
 * A row is a grid when it is finite, strictly increasing and has its ends on the window.  A line whose row is not gets NaN rows and
 * status bit 1 in its info word (growth rates: NaN and the solver's status bit 1), counted by return values > 0; no other line changes
 * by a bit.  One thread per uniform node finds the node's interval of the line's grid once, by bisection (the row staged in LDS up to
 * 2050 points, read from global memory beyond) and serves every system of the line with it.  No sums and no atomics: the results are
 * bitwise repeatable and independent of the batch, of the order of the lines and of the chunking.  Any odd N in [66, 65537] (even N
 * and N outside: IBS_ERR_UNSUPPORTED); all argument checks run before the context is touched.
 *
 * ibs_regrid_rows_f64: raw rows g, c, f [n_sys][ld] on theta -> g_u, c_u, f_u on the uniform nodes and gh at the half nodes (gh[k]
 * between nodes k and k+1, gh[N-1] = 0), [n_sys][ld_out]: the arguments of ibs_solve_gcfh_f64 / _nearest_f64 / _modes_f64.  c / c_u and
 * f / f_u are optional as pairs; info [n_sys] optional. */
int ibs_regrid_rows_f64(ibs_ctx* ctx, int64_t n_sys, int32_t N, const double* theta, int64_t theta_ld, double theta_lo,
                        double theta_hi, const double* g, const double* c, const double* f, int64_t ld, double* g_u, double* gh,
                        double* c_u, double* f_u, int64_t ld_out, double* h_out, int32_t* info, int32_t mem);
/* The same from the geometry: for every (line, theta0) system g, c, f are formed AT THE SAMPLES (ball_scan.py:267-268,
 * utils.py:1560-1562: the expressions of ibs_gamma_scan_f64) and then interpolated -- upstream's order: the formed rows are
 * interpolated, not the geometry arrays.  Arrays, dPdrho and theta0 as in ibs_gamma_scan_f64; theta0_per_line != 0: n_theta0 = 1 and
 * theta0 [n_lines], one value per line (as ibs_gamma_points_f64).  g_u, gh, c_u, f_u [n_lines * n_theta0][N], all required;
 * info [n_lines * n_theta0] optional. */
int ibs_assemble_gcf_theta_f64(ibs_ctx* ctx, int32_t n_lines, int32_t n_theta0, int32_t N, const double* theta, int64_t theta_ld,
                               double theta_lo, double theta_hi, const double* bmag, const double* gradpar, const double* cvdrift,
                               const double* cvdrift0, const double* gds2, const double* gds21, const double* gds22, int64_t ld,
                               const double* dPdrho, const double* theta0, int32_t theta0_per_line, double* g_u, double* gh,
                               double* c_u, double* f_u, double* h_out, int32_t* info, int32_t mem);
/* ibs_gamma_scan_f64 on a non-uniform grid: the regridded rows of whole lines are written to a workspace of about 1 GiB at most,
 * chunk after chunk (option "nearest_chunk_systems" sets the chunk instead, as in ibs_gamma_scan_nearest_f64; a chunk of one line that
 * cannot be allocated fails with the bytes it needs), and solved by the kernel of ibs_solve_gcfh_f64 -- one wave per system up to 2050
 * points, the long-grid path beyond.  Outputs [n_lines][n_theta0] (X, dX: [n_lines][n_theta0][N]), all optional.  On a uniform grid
 * the result differs from ibs_gamma_scan_f64's by rounding only (gh is the interpolant at the midpoint there, not the mean). */
int ibs_gamma_scan_theta_f64(ibs_ctx* ctx, int32_t n_lines, int32_t n_theta0, int32_t N, const double* theta, int64_t theta_ld,
                             double theta_lo, double theta_hi, const double* bmag, const double* gradpar, const double* cvdrift,
                             const double* cvdrift0, const double* gds2, const double* gds21, const double* gds22, int64_t ld,
                             const double* dPdrho, const double* theta0, double* gam, double* lam, double* X, double* dX,
                             int32_t* info, int32_t mem);
/* ibs_gamma_points_f64 on a non-uniform grid (the final solve of ball_scan.py:322-339): line i at its own theta0[i]; the bits of
 * ibs_gamma_scan_theta_f64 at the same (line, theta0). */
int ibs_gamma_points_theta_f64(ibs_ctx* ctx, int32_t n_pts, int32_t N, const double* theta, int64_t theta_ld, double theta_lo,
                               double theta_hi, const double* bmag, const double* gradpar, const double* cvdrift,
                               const double* cvdrift0, const double* gds2, const double* gds21, const double* gds22, int64_t ld,
                               const double* dPdrho, const double* theta0, double* gam, double* lam, double* X, double* dX,
                               int32_t* info, int32_t mem);

/* Start points of the refinement from the coarse scan's per-surface maxima, on the device (device pointers only).
 * Replaces: ball_scan.py:279-295 -- the first maximum of the surface's (alpha, theta0) table gives x0 = (alpha_scan[i],
 * theta0_scan[j]) and sigma0 = 1.3 |gam| + 0.05 (:283-295); an all-zero table starts from (0, 0) with sigma0 = 0.05 (:279-282).
 *   pack[n_surf][2] = (max, first row-major index as a double): the output of ibs_gamma_scan_argmax_f64 /
 *   ibs_surface_argmax_pack_f64;  alpha[n_alpha], theta0[n_theta0]: the scan grids (ball_scan.py:225-226);
 *   start[n_surf][2] = (alpha, theta0): the `start` input of ibs_refine_f64;  sigma0[n_surf] (optional; the deterministic
 *   solver ignores it);  *n_bad (device int, NOT cleared here) += the number of surfaces whose maximum is not finite (a
 *   flagged or NaN table: ball_scan.py would have crashed in eigs; their start is (0, 0)). */
int ibs_scan_starts_f64(ibs_ctx* ctx, int32_t n_surf, int32_t n_alpha, int32_t n_theta0, const double* alpha,
                        const double* theta0, const double* pack, double* start, double* sigma0, int32_t* n_bad);

/* Objective and Hellmann-Feynman ("adjoint") gradient at n_pts points (alpha, theta0).
 * Replaces: utils.py:1632-1728 obj_w_grad, given the geometry of the three field lines
 * (alpha - del_alpha/2, alpha, alpha + del_alpha/2) that utils.py:1641-1646 obtains from vmec_fieldlines.
 *   geo [n_pts][3][8][ld]: per line bmag, gradpar, cvdrift, cvdrift0, gds2, gds21, gds22, gbdrift
 *   (dPdrho of each line is formed on the device, utils.py:1657/1691/1703);  theta0[n_pts];
 *   val[n_pts] = -gam;  jac[n_pts][2] = (-dgam/dalpha, -dgam/dtheta0)   (utils.py:1728). */
int ibs_obj_w_grad_f64(ibs_ctx* ctx, int32_t n_pts, int32_t N, double h, const double* geo, int64_t ld,
                       const double* theta0, double del_alpha, double* val, double* jac, int32_t* info,
                       int32_t mem);

/* Hellmann-Feynman derivative of gam with respect to any parameter p, given the eigenfunction and the tangent
 * coefficient arrays (d g/dp, d c/dp, d f/dp) on the grid:
 *   jac = [ S(c_p X^2) - S(g_p dX^2) - gam S(f_p X^2) ] / S(f X^2),   S = composite Simpson, unit spacing.
 * Replaces: utils.py:1676-1680 (p = theta0) and utils.py:1721-1725 (p = alpha) for caller-built tangents; the
 * fused entry point above builds both tangents itself.  All arrays [n_sys][ld], gam and jac [n_sys]; N odd. */
int ibs_hf_grad_f64(ibs_ctx* ctx, int64_t n_sys, int32_t N, const double* X, const double* dX, const double* f,
                    const double* g_p, const double* c_p, const double* f_p, int64_t ld, const double* gam,
                    double* jac, int32_t mem);

/* Field-line geometry on the device: the eight arrays of ball_scan.py:251-261 for
 * n_lines field lines (surface index, alpha) on the theta_PEST grid theta[N].
 * Replaces: the per-line arithmetic of vmec_fieldlines, utils.py:359-720 (theta_pest -> theta_vmec secant
 * solve :391-416, Fourier synthesis :420-468, metric algebra :474-720); the radial splines of
 * utils.py:37-158 / :311-357 stay on the host and provide, per surface,
 *   tab_mn  [n_surf][6][mnmax]      rmnc zmns lmns d_rmnc_d_s d_zmns_d_s d_lmns_d_s
 *   tab_nyq [n_surf][7][mnmax_nyq]  gmnc bmnc d_bmnc_d_s bsupvmnc bsubsmns bsubumnc bsubvmnc
 *   scal    [n_surf][6]             s iota d_iota_d_s d_pressure_d_s phiedge Aminor_p
 * and the mode numbers xm, xn [mnmax], xm_nyq, xn_nyq [mnmax_nyq] (xn includes nfp).
 *   geo [8][n_lines][ld]: bmag gradpar_theta_pest cvdrift cvdrift0 gds2 gds21 gds22 gbdrift; entries N..ld-1 of a row are
 *   never written, with host pointers as with device pointers
 *   dPdrho[n_lines] (optional): -0.5 mean((cvdrift - gbdrift) bmag^2), ball_scan.py:262.
 *   rows_mn [nrows_mn][2], rows_nyq [nrows_nyq][2] (optional, nrows = 0 to omit): {first mode, count} of each
 *   run of modes with equal m and n advancing by the common step dn_mn / dn_nyq (= nfp in VMEC's own
 *   ordering); enables the rotation-recurrence kernels (no sincos per mode).  Every row must lie inside its mode list
 *   (else IBS_ERR_ARG).  The row kernels hold at most 64 pair indices about a row's centre -- the mode with n = 0 if the
 *   row has one, else its first mode: rows of up to 129 modes n = -64 dn .. 64 dn, or up to 65 modes otherwise; tables
 *   with a longer row in rows_mn are valid and run on the one-sincos-per-mode kernel (split such rows to stay on the fast
 *   path: ibs_amd.geometry.mode_rows does).  Rows of one list must not overlap (IBS_ERR_ARG).  Device-resident rows are copied back
 *   and checked once per table set, the verdict kept under the rows' ADDRESSES and sizes (four sets): a caller that reuses that device
 *   memory for other rows calls ibs_set_option(ctx, "forget_rows", 1) first.
 * The first seven planes of geo and dPdrho are exactly the inputs of ibs_gamma_scan_f64. */
int ibs_fieldline_geometry_f64(ibs_ctx* ctx, int32_t n_surf, int32_t mnmax, int32_t mnmax_nyq, const double* xm,
                               const double* xn, const double* xm_nyq, const double* xn_nyq, const double* tab_mn,
                               const double* tab_nyq, const double* scal, int32_t n_lines, const int32_t* line_surf,
                               const double* line_alpha, int32_t N, const double* theta, int64_t ld, double* geo,
                               double* dPdrho, int32_t nrows_mn, const int32_t* rows_mn, int32_t nrows_nyq,
                               const int32_t* rows_nyq, double dn_mn, double dn_nyq, int32_t mem);

/* Vector-Jacobian product of ibs_fieldline_geometry_f64: from cotangents of the eight arrays (and of dPdrho) to cotangents
 * of the surface tables, the surface scalars and the line labels.
 * Replaces: nothing.  Nothing upstream corresponds: the reference obtains sensitivities to the equilibrium by re-scanning
 * perturbed equilibria (sims_runner_NCSX.py:151-276) and its alpha-derivative by a central difference of the rows
 * (utils.py:1641-1646).  The arithmetic differentiated is utils.py:359-720 as the forward call restates it; the
 * theta_pest -> theta_vmec root solve (utils.py:391-416) is differentiated by the implicit-function theorem at the
 * converged root theta_vmec + Lambda(theta_vmec, phi) = theta_pest, not through the secant iterations; sgn(Psi') is a
 * constant and d|Psi'| = sgn(Psi') dPsi' (utils.py:474, 654-665).
 *   every forward input as for ibs_fieldline_geometry_f64 (mode rows are not needed: any mode ordering);
 *   geo_bar [8][n_lines][ld]: cotangents of the eight arrays, entries N..ld-1 of a row are never read;
 *   dPdrho_bar [n_lines] (optional): cotangent of dPdrho, folded into planes 0, 2 and 7 (ball_scan.py:262);
 *   tab_mn_bar [n_surf][6][mnmax], tab_nyq_bar [n_surf][7][mnmax_nyq], scal_bar [n_surf][6], alpha_bar [n_lines]: each
 *   optional, at least one required.  A surface no line refers to gets zeros.  theta gets no cotangent (the grid is fixed).
 * A line whose forward evaluation is not finite gives NaN in alpha_bar[line] and in the rows of its surface.
 * No floating-point atomics: every sum runs in a fixed order (lines of a surface by index), so the same call gives the same
 * bits on every run, with host or device pointers, whichever outputs are requested.
 * n_lines and n_surf <= 65535.  IBS_MEM_HOST: synchronous; IBS_MEM_DEVICE: asynchronous on the context's stream, nothing is
 * read back (device-resident line_surf is clamped to [0, n_surf), like the forward call's). */
int ibs_fieldline_geometry_vjp_f64(ibs_ctx* ctx, int32_t n_surf, int32_t mnmax, int32_t mnmax_nyq, const double* xm,
                                   const double* xn, const double* xm_nyq, const double* xn_nyq, const double* tab_mn,
                                   const double* tab_nyq, const double* scal, int32_t n_lines, const int32_t* line_surf,
                                   const double* line_alpha, int32_t N, const double* theta, int64_t ld,
                                   const double* geo_bar, const double* dPdrho_bar, double* tab_mn_bar,
                                   double* tab_nyq_bar, double* scal_bar, double* alpha_bar, int32_t mem);

/* Tangent of ibs_fieldline_geometry_f64 in the line label: d/d alpha of the eight arrays of every line, in forward mode.
 * Replaces: the central difference of the rows in utils.py:1641-1646 / 1683-1718 (three field lines per point, the side lines
 * del_alpha / 2 away, an O(del_alpha^2) error of 1e-5 .. 3e-4 of an array's scale at upstream's 0.004) by their derivative.  The
 * arithmetic differentiated is utils.py:359-720 in the plain form ibs_fieldline_geometry_vjp_f64 recomputes: phi = (theta - alpha) /
 * iota so phi' = -1 / iota; the theta_pest -> theta_vmec root solve (utils.py:391-416) by the implicit-function theorem at the
 * converged root, theta_vmec' = -Lambda_phi phi' / (1 + Lambda_theta), not through the secant iterations; every synthesised sum
 * S' = sum coef trig'(m theta_vmec - n phi) (m theta_vmec' - n phi'), taken as two partial sums in the same pass over the modes as
 * the values; then the metric algebra on (value, tangent) pairs.
 * dPdrho has no alpha-tangent and none is returned: cvdrift - gbdrift is the pressure term -2 mu0 sgn(Psi') p' B_ref Aminor^2 sqrt(s)
 * / (Psi' |B|^2) (utils.py:700-720) and bmag^2 = |B|^2 / B_ref^2, so (cvdrift - gbdrift) bmag^2 holds surface quantities alone and
 * dPdrho = -1/2 mean(...) (ball_scan.py:262) is the same on every line of a surface; a caller that differentiates rows in alpha holds
 * it fixed.
 *   every forward input as for ibs_fieldline_geometry_vjp_f64 up to ld (mode rows are not needed: any mode ordering);
 *   geo_da [8][n_lines][ld]: d/d alpha of bmag gradpar cvdrift cvdrift0 gds2 gds21 gds22 gbdrift; entries N..ld-1 of a row are
 *   never written.  A grid point whose forward evaluation is not finite gets NaN in its eight entries, nothing else is touched.
 * One lane per grid point, no atomics and no cross-lane sums: a line alone gives the bits it has in a batch, with host or device
 * pointers (csrc/ibs_geometry_tangent.hip).  Any N >= 2; n_lines and n_surf <= 65535.  IBS_MEM_HOST: synchronous; IBS_MEM_DEVICE:
 * asynchronous on the context's stream (device-resident line_surf is clamped to [0, n_surf), like the forward call's). */
int ibs_fieldline_geometry_dalpha_f64(ibs_ctx* ctx, int32_t n_surf, int32_t mnmax, int32_t mnmax_nyq, const double* xm,
                                      const double* xn, const double* xm_nyq, const double* xn_nyq, const double* tab_mn,
                                      const double* tab_nyq, const double* scal, int32_t n_lines, const int32_t* line_surf,
                                      const double* line_alpha, int32_t N, const double* theta, int64_t ld, double* geo_da,
                                      int32_t mem);

/* Host part of the geometry producer: the per-surface Fourier coefficient vectors of n_eq equilibria at n_s surfaces.
 * Replaces: vmec_splines (utils.py:58-119: one InterpolatedUnivariateSpline per mode and array) + their evaluation at the
 * surface (utils.py:311-357) for all equilibria of an optimizer step (sims_runner_NCSX.py:151-276) at once.  Cubic
 * interpolating splines are linear in the data and all modes share the radial meshes, so the caller supplies four weight
 * matrices [n_s][ns] -- value / derivative on VMEC's full mesh, value / derivative on the half mesh with a zero first
 * column (half-mesh data live in columns 1..ns-1) -- built once per (ns, surfaces) by splining the identity.
 *   tabs[n_eq][9]: pointers to the (modes, ns) row-major wout arrays rmnc zmns lmns (mnmax rows) gmnc bmnc bsupvmnc
 *   bsubsmns bsubumnc bsubvmnc (mnmax_nyq rows);  tab_mn [n_eq * n_s][6][mnmax], tab_nyq [n_eq * n_s][7][mnmax_nyq]: the
 *   inputs of ibs_fieldline_geometry_f64 (surface index = i_eq * n_s + i_s).  Host pointers only; n_threads <= 0: up to 16.
 * No GPU is involved; results do not depend on the thread count. */
int ibs_surface_tables_f64(int32_t n_eq, int32_t ns, int32_t n_s, int32_t mnmax, int32_t mnmax_nyq,
                           const double* const* tabs, const double* w_full, const double* w_full_d,
                           const double* w_half, const double* w_half_d, double* tab_mn, double* tab_nyq,
                           int32_t n_threads);

/* Refinement of the per-surface maximum: maximise gam over (alpha, theta0) in
 * [0, pi] x [0, pi/2] from n_pts start points at once, entirely on the device.
 * Replaces: ball_scan.py:305-314 (scipy.optimize.minimize(obj_w_grad, x0, jac=True, bounds, ftol, gtol, maxiter), i.e.
 * scipy's L-BFGS-B: restated for the two unknowns in csrc/ibs_lbfgsb2.hpp, one state machine per point) together with
 * the evaluations it drives (utils.py:1632-1728 on the three field lines of utils.py:1641-1646, produced by the
 * geometry kernel).  A round = the geometry kernel (3 lines per point still running) + one fused kernel per point
 * (objective, Hellmann-Feynman gradient, optimizer step; the eigen-solve is warm-started from the point's previous
 * evaluation; the block that finishes last re-packs the batch).  Nothing returns to the host between rounds: the device
 * posts the count of unfinished points per round into pinned memory, and the host enqueues rounds two ahead of the last
 * count it has seen (csrc/ibs_refine.hpp).
 *   surface tables, mode tables, row tables: as for ibs_fieldline_geometry_f64;  pt_surf[n_pts] surface of each point;
 *   start[n_pts][2] = (alpha, theta0);  theta[N] uniform theta_PEST grid;  del_alpha (utils.py:1639: 0.004);
 *   maxiter, ftol, gtol: ball_scan.py:312-313 (30, 5e-11, 2e-8); like scipy's driver the limit is tested after each
 *   completed iteration, so maxiter = 0 performs one.
 *   x_opt[n_pts][2], f_opt[n_pts] = -gam at x_opt (utils.py:1728 sign), n_evals[n_pts] (optional).  x_opt lies in the box up
 *   to the rounding of x + stp d (L-BFGS-B projects directions, not points).
 *   n_pts = 0 (a rank without surfaces) is a no-op: the per-point pointers may be null, 0 rounds are returned.
 * `mem` applies to every pointer.  IBS_MEM_HOST: synchronous.  IBS_MEM_DEVICE: the host returns once every round's count
 * has been read, but the kernel that writes x_opt / f_opt / n_evals may still be running: the outputs are STREAM-ORDERED
 * on the context's stream like those of every other device-pointer call (read them from that stream, or after
 * ibs_synchronize()).  A round that does not report within 120 s fails with IBS_ERR_HIP.
 * Returns the number of rounds (>= 0) or an error (< 0). */
int ibs_refine_f64(ibs_ctx* ctx, int32_t n_surf, int32_t mnmax, int32_t mnmax_nyq, const double* xm, const double* xn,
                   const double* xm_nyq, const double* xn_nyq, const double* tab_mn, const double* tab_nyq,
                   const double* scal, int32_t nrows_mn, const int32_t* rows_mn, int32_t nrows_nyq,
                   const int32_t* rows_nyq, double dn_mn, double dn_nyq, int32_t n_pts, const int32_t* pt_surf,
                   const double* start, int32_t N, const double* theta, double del_alpha, int32_t maxiter,
                   double ftol, double gtol, double* x_opt, double* f_opt, int32_t* n_evals, int32_t mem);

/* Statistics of the last ibs_refine_f64 call of this context (diagnostic; no reference counterpart):
 * out4 = {objective evaluations, forward sweeps of their eigen-solves, rounds needed, rounds enqueued}. */
int ibs_refine_stats(ibs_ctx* ctx, int64_t* out4);

/* Diagnostic (no reference counterpart): the solver / geometry kernel most recently launched by the calling thread -- its
 * name as rocprofv3 prints it ("ibs::k_gamma_scan<double, 8>"; the library picks lanes per system, theta0 chaining and the
 * geometry form from the batch size) and the launch dimensions (blocks, threads per block; waves = blocks * threads / 64).
 * bench.py uses it to look a leg's kernel up in the committed PMC passes by its exact name and batch size. */
int ibs_last_launch(char* name, int32_t len, int64_t* blocks, int32_t* threads);

/* Number of eigenvalues of (T, F) strictly above shift[i] for each system (Sturm sequence).
 * Replaces: tests/shifted-circle-s-alpha/bishop_ball_s-alpha.py:20-115 check_ball (isunstable <=> count(0) > 0).
 * Up to N = 2050 this is ONE prefix-product sweep per system (the bandwidth kernel): exact for a pencil perturbed by ~N eps ||A||
 * on smooth coefficients, but by up to ~N^2 eps ||A|| on iid-random ones -- within that distance of an eigenvalue the count can be
 * off by one.  Option "sturm_form" = 2 selects the DIVISION-form kernel instead (lanes as systems, the rows through an LDS transpose,
 * every system read from its own 128-byte line boundary: exact for a pencil a few ulp away, any N, 4.8-5.5 TB/s in batches of 65,536
 * systems or more against the sweep's 6 TB/s at N_zeta <= 512; Python: sturm_count(..., exact=True)); it is what grids beyond 2050
 * points get (batches under 64 systems: one wave per system) and, where it is also the faster one, what big batches get by default
 * (16 rows per lane = N in 963 .. 1026 from 65,536 systems, 32 rows = 1987 .. 2050 from 32,768: the sweep runs at 4.2 / 2.8 TB/s
 * there).  Even N is accepted here.  Magnitudes: the sweep rescales its recurrence every 8 rows inside a lane, so g, c, f may be given in
 * any units that keep the row magnitudes max(|d - shift f|, e) (d = c - (e_lo + e_hi), e = half-grid g / h^2) between about 1e-30 and
 * 1e30 -- counts are tested exact for inputs of order 1 ... 1e3 with (g, c) scaled by 2^-40 ... 2^40 and f by 2^20, at shifts from
 * below the spectrum to above it; the division forms take anything above about 1e-280. */
int ibs_sturm_count_f64(ibs_ctx* ctx, int64_t n_sys, int32_t N, double h, const double* g, const double* c,
                        const double* f, int64_t ld, const double* shift, int32_t* count, int32_t mem);

/* The same count for every (line, theta0) of a geometry-fed scan: the number of unstable modes per field line and theta0 at shift 0.
 * Replaces: tests/shifted-circle-s-alpha/bishop_ball_s-alpha.py:110-115 (isunstable <=> count(0) > 0) for real field lines: arrays,
 * dPdrho and theta0 as in ibs_gamma_scan_f64, shift and count [n_lines][n_theta0].  The rows are folded and assembled on the device
 * (ball_scan.py:267-268, utils.py:1560-1562, 1574-1592) and counted in division form with lanes as systems (csrc/ibs_certify.hip):
 * exact for a pencil a few ulp away, any N in [66, 65537].  Even N is accepted, as in ibs_sturm_count_f64. */
int ibs_geo_sturm_count_f64(ibs_ctx* ctx, int32_t n_lines, int32_t n_theta0, int32_t N, double h, const double* bmag,
                            const double* gradpar, const double* cvdrift, const double* cvdrift0, const double* gds2,
                            const double* gds21, const double* gds22, int64_t ld, const double* dPdrho, const double* theta0,
                            const double* shift, int32_t* count, int32_t mem);

/* Certificate of the eigenvalues a geometry-fed scan returned.  Nothing upstream corresponds.  The scan, objective and refinement
 * kernels close lam_max with the scaled-row shift iteration and state no a-priori bound; this call states one afterwards, independent
 * of their arithmetic: with tol = tol_factor N eps ||A|| (tol_factor <= 0: 4, the bound of the raw entry points; ||A|| as under status
 * bit 3 above) the division-form Sturm counts of the system's rows must read 0 above lam + tol and >= 1 above lam - tol.
 *   arrays, dPdrho, theta0 as in ibs_gamma_scan_f64; lam [n_lines][n_theta0] (in); cert [n_lines][n_theta0] (out), per system:
 *   bit 0 = an eigenvalue lies above lam + tol: lam is not the largest eigenvalue; bit 1 = no eigenvalue lies above lam - tol: there
 *   is none at lam; bit 2 = not checked: lam is not finite or the data are invalid (non-finite, g <= 0 or f <= 0); 0 = certified:
 *   |lam - lam_max| <= tol.  (Bit 3 is set by the re-close below.)
 * N as for ibs_gamma_scan_f64 (odd, 66 .. 65537; else IBS_ERR_UNSUPPORTED).  Host pointers: returns the number of systems with a
 * non-zero cert word.  One kernel, lanes as systems, two passes over each line (csrc/ibs_certify.hip). */
int ibs_gamma_scan_certify_f64(ibs_ctx* ctx, int32_t n_lines, int32_t n_theta0, int32_t N, double h, const double* bmag,
                               const double* gradpar, const double* cvdrift, const double* cvdrift0, const double* gds2,
                               const double* gds21, const double* gds22, int64_t ld, const double* dPdrho, const double* theta0,
                               const double* lam, double tol_factor, int32_t* cert, int32_t mem);
/* The same certificate for the points of ibs_gamma_points_f64: one (line, theta0) pair per point, theta0, lam and cert [n_pts].
 * Nothing upstream corresponds. */
int ibs_gamma_points_certify_f64(ibs_ctx* ctx, int32_t n_pts, int32_t N, double h, const double* bmag, const double* gradpar,
                                 const double* cvdrift, const double* cvdrift0, const double* gds2, const double* gds21,
                                 const double* gds22, int64_t ld, const double* dPdrho, const double* theta0, const double* lam,
                                 double tol_factor, int32_t* cert, int32_t mem);
/* Re-close of the systems a certificate refused.  Nothing upstream corresponds.  Every system whose cert word has bit 0 or 1 (and not
 * bit 2) is solved again on its rows in division form -- bounds, 64-way multisection to 2 eps ||A||, twisted-factorisation
 * eigenvector and the growth rate of utils.py:1601-1621, the pieces of the long-grid path of ibs_solve_gcf_f64 -- and certified again
 * with tol_factor (as above).  On success lam, gam (and X, dX [n_lines][n_theta0][N] where given) of that system are replaced and its
 * cert word becomes bit 3 alone (re-closed: informational); a system that still fails keeps its bits.  Every other entry of cert, lam,
 * gam, X, dX is left untouched bit for bit.  cert, lam, gam are in-out and required; X, dX optional.
 * Device pointers: list, solve and second certificate are queued on the context's stream; nothing is read back in between (the list of
 * refused systems and its counter live on the device).  Host pointers: returns the number of systems that still carry bit 0 or 1.
 * The composition for a C caller: ibs_gamma_scan_f64 (lam requested) -> ibs_gamma_scan_certify_f64 -> ibs_gamma_scan_reclose_f64. */
int ibs_gamma_scan_reclose_f64(ibs_ctx* ctx, int32_t n_lines, int32_t n_theta0, int32_t N, double h, const double* bmag,
                               const double* gradpar, const double* cvdrift, const double* cvdrift0, const double* gds2,
                               const double* gds21, const double* gds22, int64_t ld, const double* dPdrho, const double* theta0,
                               double tol_factor, int32_t* cert, double* lam, double* gam, double* X, double* dX, int32_t mem);
/* The same re-close for the points of ibs_gamma_points_f64 (theta0, cert, lam, gam [n_pts]; X, dX [n_pts][N]).  Nothing upstream
 * corresponds. */
int ibs_gamma_points_reclose_f64(ibs_ctx* ctx, int32_t n_pts, int32_t N, double h, const double* bmag, const double* gradpar,
                                 const double* cvdrift, const double* cvdrift0, const double* gds2, const double* gds21,
                                 const double* gds22, int64_t ld, const double* dPdrho, const double* theta0, double tol_factor,
                                 int32_t* cert, double* lam, double* gam, double* X, double* dX, int32_t mem);

/* Per-surface reduction of a scan: first (row-major) index of the maximum and its value, the rule of
 * ball_scan.py:279-295.  gam is [n_surf][n_per_surf]. */
int ibs_surface_argmax_f64(ibs_ctx* ctx, int32_t n_surf, int32_t n_per_surf, const double* gam,
                           int32_t* idx, double* val, int32_t mem);

/* Same reduction on device pointers, written as pack[n_surf][2] = (value, index as double): the one buffer the
 * per-surface all-gather sends (replaces the three comm_lead.Gather of ball_scan.py:345-347). */
int ibs_surface_argmax_pack_f64(ibs_ctx* ctx, int32_t n_surf, int32_t n_per_surf, const double* gam, double* pack);

/* The n_starts best local maxima ("peaks") of every surface's coarse table and the starts of a multi-start refinement from them.
 * Replaces, in slot 0: ball_scan.py:279-295 -- the first maximum of the table, x0 = (alpha_scan[i], theta0_scan[j]) and sigma0 =
 * 1.3 |gam| + 0.05; a maximum of exactly 0 starts from (0, 0) with sigma0 = 0.05 (:279-282); the start and sigma0 of
 * ibs_surface_argmax_pack_f64 + ibs_scan_starts_f64, bit for bit.  Slots >= 1 have no upstream counterpart (upstream refines from the
 * first maximum alone).
 *   The rule (csrc/ibs_scan_peaks.hpp; ibs_amd.scan.pick_starts in numpy): a neighbour w of entry v beats it if w > v, or w == v and w
 *   has the smaller row-major index; a NaN never beats anything.  A peak is an entry that is not NaN and that none of its up to
 *   eight neighbours (i +- 1, j +- 1) inside the table beats -- no wrap-around: (alpha, theta0) is a box.  Peaks rank by value
 *   descending, ties by index ascending; slot k holds peak k: its node, its value, its row-major index and its own sigma0 =
 *   1.3 |peak| + 0.05.  n_found = the number of peaks found (<= n_starts); the slots from n_found on repeat slot 0.  A first maximum
 *   of exactly 0, or one that is not finite (counted once in *n_bad; a table of NaN counts too), starts from (0, 0) with n_found = 0
 *   and index -1 in every slot.
 *   gam [n_surf][n_alpha][n_theta0]; alpha [n_alpha], theta0 [n_theta0]: the scan grids;  start [n_surf][n_starts][2] = (alpha,
 *   theta0), peak [n_surf][n_starts];  index (int32), sigma0 [n_surf][n_starts] and n_found [n_surf] are optional (NULL);
 *   *n_bad (NOT cleared here) += the number of surfaces whose maximum is not finite.  1 <= n_starts <= 16.
 * Host or device pointers (mem).  n_starts outside [1, 16], a dimension < 1 or a required pointer NULL: IBS_ERR_ARG before the
 * context is touched; n_surf = 0: nothing happens.  Results are bitwise repeatable and independent of n_surf. */
int ibs_scan_peaks_f64(ibs_ctx* ctx, int32_t n_surf, int32_t n_alpha, int32_t n_theta0, int32_t n_starts, const double* alpha,
                       const double* theta0, const double* gam, double* start, double* peak, int32_t* index, double* sigma0,
                       int32_t* n_found, int32_t* n_bad, int32_t mem);

/* The growth rate of every line maximised over theta0 BETWEEN the nodes of the coarse scan: gam_env = max over theta0 of gam(line,
 * theta0), about the n_starts best peaks of the line's coarse row.  Stands beside ball_scan.py:248-295, where upstream has no such
 * step: it reads every maximum off the nodes and refines only the surface's first maximum, in (alpha, theta0), at three new field
 * lines per evaluation.  The theta0 direction needs no new geometry: the fold (ball_scan.py:267-268) turns the staged line into the
 * system of any theta0.
 *   The rule (csrc/ibs_theta0_polish.hpp; ibs_amd.scan.row_peaks and polish_theta0 in Python).  Row peaks: entry j of gam[line][:] is
 *   a peak if it is not NaN and neither neighbour inside the row beats it (w beats v if w > v, or w == v and w has the smaller index; a
 *   NaN never beats anything); peaks rank by value descending, ties by index ascending; slot k holds peak k, slots from n_found on
 *   repeat slot 0, a row without a finite entry has n_found = 0, node -1 and NaN outputs.  Bracket of node j: [theta0[j-1],
 *   theta0[j+1]], cut to the node on a side where the row ends or the neighbour is NaN; zero length: the node, 0 evaluations; exactly
 *   one side cut: status bit 12.  Search: Brent's bounded maximiser (parabolic step, golden-section fallback; derivative-free: the
 *   Hellmann-Feynman dgam_dtheta0 is not the derivative of the gam that is returned), seeded with the three known node values so that
 *   nothing known is solved again (one-sided: first the golden point next to the node); it stops on |x - m| <= 2 xtol - (b - a) / 2
 *   or after max_eval evaluations (bit 11); an evaluation that fails or is not finite counts as -inf and its status bits 0-1 are
 *   OR-ed into the slot's word.  Incumbent: the result is the polished point only if its gam is STRICTLY greater than the node's,
 *   else the node itself with the table's gam (bit 10): gam_star is never below the coarse row.
 *   The seven arrays [n_lines][ld], dPdrho [n_lines]: as ibs_gamma_scan_f64;  theta0 [n_theta0]: finite and strictly increasing;
 *   gam [n_lines][n_theta0]: the coarse table (required);  lam, same shape, optional: warm starts of the first solve of a slot;
 *   node_in [n_lines][n_starts], optional: polish about THESE nodes (-1, a node outside the row or one whose gam is NaN = skip the
 *   slot: NaN outputs, node -1) instead of the row's own peaks; n_found is then written as 0;
 *   theta0_star, gam_star [n_lines][n_starts] (required);  lam_star (the eigenvalue at theta0_star; NaN where the node is returned and
 *   lam is NULL), node, n_eval, info (int32) [n_lines][n_starts] and n_found [n_lines] optional.
 *   info: bits 0..15 = forward sweeps of all evaluations of the slot, saturated; bits 16.. = the status (conventions above).
 * FP64, odd N in [66, 2050]; beyond, and even N: IBS_ERR_UNSUPPORTED (the staged-line kernel has no long-grid form).  n_starts outside
 * [1, 4], xtol <= 0 or not finite, max_eval outside [1, 64], a dimension < 1 or a required pointer NULL: IBS_ERR_ARG before the context
 * is touched; n_lines = 0: nothing happens.  A theta0 grid that is not finite and strictly increasing: IBS_ERR_ARG on host pointers;
 * on device pointers every slot gets status bit 1 and NaN.  Host or device pointers (mem); host pointers: returns the number of slots
 * with status bit 0 or 1.  One block per line, one wavefront per slot; results are bitwise repeatable and independent of n_lines, of
 * the order of the lines and, for slot 0, of n_starts. */
int ibs_theta0_polish_f64(ibs_ctx* ctx, int32_t n_lines, int32_t n_theta0, int32_t N, double h, const double* bmag,
                          const double* gradpar, const double* cvdrift, const double* cvdrift0, const double* gds2,
                          const double* gds21, const double* gds22, int64_t ld, const double* dPdrho, const double* theta0,
                          const double* gam, const double* lam, const int32_t* node_in, int32_t n_starts, double xtol,
                          int32_t max_eval, double* theta0_star, double* gam_star, double* lam_star, int32_t* node,
                          int32_t* n_eval, int32_t* info, int32_t* n_found, int32_t mem);

/* HOST side of the same rule (no GPU involved; the pattern of ibs_lbfgsb2_*): the search of one node as a reverse-communication
 * state machine, and the row peaks.
 *   state: caller-owned buffer of ibs_theta0_polish_state_bytes() bytes.
 *   init:  theta0 [n_theta0], row [n_theta0] = the coarse gam of the line, node = the entry to polish about; returns 1 = evaluate gam
 *          at *x_next, 0 = finished at once (zero-length bracket).  A bad grid, node, xtol or max_eval: IBS_ERR_ARG.
 *   step:  hand over gam at the point last requested and the status bits 0-1 of that evaluation; returns 1 = evaluate at *x_next,
 *          0 = finished.
 *   result: theta0_star, gam_star, n_eval, status (bits 0-1, 10, 11, 12), each optional.
 *   ibs_row_peaks_f64: gam [n_rows][n_theta0] -> node [n_rows][K] (int32), n_found [n_rows] (optional), 1 <= K <= 4. */
int ibs_theta0_polish_state_bytes(void);
int ibs_theta0_polish_init(void* state, int32_t n_theta0, const double* theta0, const double* row, int32_t node, double xtol,
                           int32_t max_eval, double* x_next);
int ibs_theta0_polish_step(void* state, double gam, int32_t eval_status, double* x_next);
int ibs_theta0_polish_result(const void* state, double* theta0_star, double* gam_star, int32_t* n_eval, int32_t* status);
int ibs_row_peaks_f64(int32_t n_rows, int32_t n_theta0, int32_t K, const double* gam, int32_t* node, int32_t* n_found);

/* The margin of every line maximised over theta0 BETWEEN the nodes of ibs_marginal_scan_f64's table: mu_env = max over theta0 of
 * mu(line, theta0) = 1 / s*, i.e. the smallest critical scale of the line, about the n_starts best peaks of the line's coarse row of
 * mu.  The twin of ibs_theta0_polish_f64 on the margin; nothing upstream corresponds.  The rule is that call's, point for point (row
 * peaks, bracket, Brent's bounded search seeded with the three node values, incumbent, slots from n_found on repeat slot 0, NaN rows,
 * node_in), with mu in place of gam: s* = +inf is the VALUE mu = 0, an evaluation with status bit 0 or 1 counts as -inf and its bits
 * are OR-ed into the slot's word.  The ibs_theta0_polish_init / _step / _result state machine drives the same search on the host.
 *   The seven arrays [n_lines][ld], dPdrho [n_lines], theta0 [n_theta0] (finite and strictly increasing): as ibs_marginal_scan_f64;
 *   mu [n_lines][n_theta0]: the coarse table, that call's mu (required);  node_in [n_lines][n_starts], optional, as in
 *   ibs_theta0_polish_f64;
 *   theta0_star, mu_star [n_lines][n_starts] (required);  scale_star = s* at theta0_star, node, n_eval, info (int32)
 *   [n_lines][n_starts] and n_found [n_lines] optional.
 *   Every evaluation is a cold solve: scale_star is bit for bit ibs_marginal_scan_f64's scale of that line at theta0_star (where the
 *   node itself is returned, one more solve at the node supplies it; it enters neither n_eval nor info), and mu_star = 1 / scale_star.
 *   info: bits 0..15 = multisection passes of all evaluations of the slot, saturated; bits 16.. = the status: bits 0-1, 10, 11, 12 as
 *   in ibs_theta0_polish_f64, bit 8 iff the returned point has s* = +inf (mu_star = 0; informational).
 * FP64, any odd N in [66, 65537] (even N and N outside: IBS_ERR_UNSUPPORTED).  n_starts outside [1, 4], xtol <= 0 or not finite,
 * max_eval outside [1, 64], a dimension < 1, ld < N or a required pointer NULL: IBS_ERR_ARG; all of these run before the context is
 * touched; n_lines = 0: nothing happens.  A theta0 grid that is not finite and strictly increasing: IBS_ERR_ARG on host pointers; on
 * device pointers every slot gets status bit 1 and NaN.  Host or device pointers (mem); host pointers: returns the number of slots with
 * status bit 0 or 1.  One wavefront per (line, slot) on the persistent grid and workspace of ibs_marginal_scan_f64
 * (k_marginal_theta0_polish, csrc/ibs_marginal_polish.hip), at most max_eval <= 64 evaluations per slot whatever the data; no
 * floating-point atomics: results are bitwise repeatable and independent of n_lines, of the order of the lines and, for slot 0, of
 * n_starts.  The frozen-geometry caveat of ibs_marginal_scan_f64 applies. */
int ibs_marginal_theta0_polish_f64(ibs_ctx* ctx, int32_t n_lines, int32_t n_theta0, int32_t N, double h, const double* bmag,
                                   const double* gradpar, const double* cvdrift, const double* cvdrift0, const double* gds2,
                                   const double* gds21, const double* gds22, int64_t ld, const double* dPdrho, const double* theta0,
                                   const double* mu, const int32_t* node_in, int32_t n_starts, double xtol, int32_t max_eval,
                                   double* theta0_star, double* mu_star, double* scale_star, int32_t* node, int32_t* n_eval,
                                   int32_t* info, int32_t* n_found, int32_t mem);

#ifdef __cplusplus
}
#endif
#endif /* IBS_H */
