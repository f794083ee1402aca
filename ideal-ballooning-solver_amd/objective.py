"""Consumer contract of the scan results.

The optimizer drivers combine the per-surface growth rates of the base equilibrium (dof 0) and of the
DOF-perturbed equilibria (dof 1..n) into the objective and its forward-difference gradient
(sims_runner_NCSX.py:249-261, 300-313).  With one process per GPU the DOF-perturbed equilibria are sharded
over ranks; the only exchange is one gather of the per-surface rows (AdjointStep) or one all-reduce (sum) of a
(n_dof+1)-vector (allreduce_dof_vector).
"""
import numpy as np

from ._lib import IbsError


def ballooning_objective(f_other, gam, gamma_thresh=-2.0e-4, prefac=50.0):
    """f0 = f_other + prefac * sum_s max(gam_s - gamma_thresh, 0)   (sims_runner_NCSX.py:254-257, 311-313;
    thresholds/weights: sims_runner_NCSX.py:56-57, sims_runner_D3D.py:57-58, sims_runner_HBERG.py:55-56).
    gam: (..., nsurfs).  fobj returns sqrt(f0) (sims_runner_NCSX.py:318)."""
    gam = np.asarray(gam, dtype=np.float64)
    return np.asarray(f_other, dtype=np.float64) + prefac * np.sum(np.maximum(gam - gamma_thresh, 0.0), axis=-1)


def smooth_max(gam, beta):
    """a smooth stand-in for the maximum of a (..., n_alpha, n_theta0) table of growth rates over its last two axes:
    (logsumexp(beta gam) - log n) / beta, n = n_alpha n_theta0, beta > 0.  max - log(n) / beta <= value <= max, and the value is
    differentiable where the maximum jumps between grid points.  gam: a torch tensor (differentiable) or anything numpy takes;
    the result is of the same kind, shaped gam.shape[:-2]."""
    beta = float(beta)
    if not beta > 0.0:
        raise IbsError("smooth_max: beta must be > 0")
    if type(gam).__module__.startswith("torch"):
        import torch
        flat = gam.reshape(*gam.shape[:-2], -1)
        return (torch.logsumexp(beta * flat, dim=-1) - float(np.log(flat.shape[-1]))) / beta
    gam = np.asarray(gam, dtype=np.float64)
    flat = beta * gam.reshape(*gam.shape[:-2], -1)
    top = flat.max(axis=-1)
    return (top + np.log(np.exp(flat - top[..., None]).sum(axis=-1)) - np.log(flat.shape[-1])) / beta


def dof_fd_gradient(f0_arr, step_arr):
    """forward-difference gradient of sqrt(f0) over the DOFs (sims_runner_NCSX.py:258-261):
    df[i-1] = (f0_arr[i] - f0_arr[0]) / step_arr[i] * 0.5 / sqrt(f0_arr[0]),  i = 1..n_dof."""
    f0_arr = np.asarray(f0_arr, dtype=np.float64)
    step_arr = np.asarray(step_arr, dtype=np.float64)
    return (f0_arr[1:] - f0_arr[0]) / step_arr[1:] * 0.5 * 1 / np.sqrt(f0_arr[0])


WOUT_SENSITIVITY_KEYS = ("rmnc", "zmns", "lmns", "gmnc", "bmnc", "bsupvmnc", "bsubsmns", "bsubumnc", "bsubvmnc", "iotas", "pres",
                         "phi", "Aminor_p")


def linearised_dof_gradient(sens, wouts, f_other, steps, gam0, gamma_thresh=-2.0e-4, prefac=50.0):
    """the forward-difference dfobj of sims_runner_NCSX.py:258-261 with the growth rates of the DOF-perturbed equilibria
    LINEARISED about the base equilibrium instead of scanned:
        gam_s(k) = gam0[s] + sum_keys <sens[s][key], wouts[k][key] - wouts[0][key]>,     k = 1 .. n_dof,
    then f0 = ballooning_objective(f_other, gam) (the max(gam - thresh, 0) switch per surface and equilibrium) and
    dof_fd_gradient(f0, steps).  sens: per surface, the cotangents d gam_s / d wout of the base equilibrium
    (AdjointStep.sensitivity(...)["wout_bar"]: the nine wout arrays, iotas, pres, phi, Aminor_p); wouts: the n_dof + 1 equilibria,
    entry 0 = base; f_other, steps (n_dof + 1,) as in AdjointStep.run; gam0 (n_surf,).
    What it is: a first-order estimate at FIXED (alpha*, theta0*).  At a refined maximum the derivative of the per-surface maximum
    equals the partial derivative at the fixed maximiser (envelope theorem), so to first order nothing is lost by not re-scanning;
    second-order terms in the step, a maximum that jumps to another (alpha, theta0) and the clipping of the maximiser to the scan's
    box are not seen.  72 dot products per surface in place of 72 scans; pure numpy."""
    gam0 = np.asarray(gam0, dtype=np.float64)
    if len(sens) != len(gam0):
        raise ValueError("linearised_dof_gradient: one sensitivity per surface")
    gam = _linearised_rows(sens, wouts, gam0, np.ones(len(gam0), dtype=bool))
    f0 = ballooning_objective(f_other, gam, gamma_thresh, prefac)
    return dof_fd_gradient(f0, steps)


def _linearised_rows(sens, wouts, v0, use):
    """(n_eq, n_surf): v0[s] + sum_keys <sens[s][key], wouts[k][key] - wouts[0][key]> for every equilibrium k (row 0 = v0), on the
    surfaces with use[s]; the others keep v0[s] in every row"""
    n_eq, n_s = len(wouts), len(v0)
    val = np.tile(v0, (n_eq, 1))
    w0 = wouts[0]
    for k in range(1, n_eq):
        for key in WOUT_SENSITIVITY_KEYS:
            d = np.asarray(wouts[k][key], dtype=np.float64) - np.asarray(w0[key], dtype=np.float64)
            if not np.any(d):
                continue
            for si in range(n_s):
                if use[si]:
                    val[k, si] += float(np.sum(np.asarray(sens[si][key]) * d))
    return val


def linearised_margin_gradient(sens, wouts, steps, scale0):
    """the forward differences AdjointStep.marginal(wouts, steps)["dscale"] with the margins of the DOF-perturbed equilibria LINEARISED
    about the base equilibrium instead of scanned and refined:
        s*_s(k) = scale0[s] + sum_keys <sens[s][key], wouts[k][key] - wouts[0][key]>,     k = 1 .. n_dof,
    then (s*(k) - s*(0)) / steps[k] -> (n_dof, n_surf).  sens: per surface, the cotangents d s*_s / d wout of the base equilibrium
    (AdjointStep.marginal_sensitivity(...)["wout_bar"]); wouts: the n_dof + 1 equilibria, entry 0 = base; steps (n_dof + 1,), entry 0
    unused; scale0 (n_surf,) the base equilibrium's margins.  A surface whose scale0 is not finite (no scale makes it unstable: its
    sensitivities are zero) gets a zero column.
    What it is: a first-order estimate at FIXED (alpha*, theta0*).  At a refined minimum that is a stationary point of the s* whose
    derivative is taken (marginal(refine=True, jac="exact_tangent")), the derivative of the per-surface minimum equals the partial
    derivative at the fixed minimiser (envelope theorem), so to first order nothing is lost by not re-scanning; second-order terms in
    the step, a minimum that jumps to another (alpha, theta0) and the clipping of the minimiser to the scan's box are not seen.  s*
    scales dPdrho at FROZEN geometry arrays: away from s* = 1 it is a local margin, and so is its derivative.  Pure numpy."""
    scale0 = np.asarray(scale0, dtype=np.float64)
    if len(sens) != len(scale0):
        raise ValueError("linearised_margin_gradient: one sensitivity per surface")
    ok = np.isfinite(scale0)
    val = _linearised_rows(sens, wouts, np.where(ok, scale0, 0.0), ok)
    return (val[1:] - val[0]) / np.asarray(steps, dtype=np.float64)[1:, None]


def dof_steps(x0, isabs, abs_step=1.0e-3, rel_step=2.0e-3):
    """finite-difference step of every DOF (create_dict.py:67, 70; sims_runner_NCSX.py:190-196):
    abs_step where flagged absolute, else rel_step * x0.  Entry 0 (base equilibrium) is unused."""
    x0 = np.asarray(x0, dtype=np.float64)
    isabs = np.asarray(isabs)
    return np.concatenate([[1.0], np.where(isabs[1:] == 1, abs_step, rel_step * x0)])


def shard_dofs(n_dof_plus_1, rank, world):
    return list(range(rank, n_dof_plus_1, world))


def allreduce_dof_vector(local_values, owned, n_dof_plus_1, world, dist=None, device=None):
    """every rank contributes the entries of the DOF-perturbed equilibria it scanned; one all-reduce(sum)
    yields the full (n_dof+1,) vector everywhere (RCCL on GPUs, gloo in CPU tests)."""
    vec = np.zeros(n_dof_plus_1)
    vec[list(owned)] = np.asarray(local_values, dtype=np.float64)
    if world == 1:
        return vec
    import torch
    t = torch.from_numpy(vec)
    if device is not None:
        t = t.to(device)
    dist.all_reduce(t, op=dist.ReduceOp.SUM)
    return t.cpu().numpy()


def chunk_cuts(n, n_chunks, growth=1.0):
    """boundaries of the coarse runs of AdjointStep: n equilibria in at most n_chunks runs, run k + 1 holding `growth` times the
    equilibria of run k (rounded; empty runs dropped).  Returns the increasing list [0, ..., n]."""
    nch = max(1, min(int(n_chunks), int(n)))
    wts = np.cumsum([0.0] + [float(growth) ** k for k in range(nch)])
    return sorted(set(int(round(n * w / wts[-1])) for w in wts))


class AdjointStep:
    """The ballooning work of ONE optimizer iteration for all equilibria of the step at once: the base equilibrium and one
    per boundary DOF (BASELINE configs[3]: 73 x 5 surfaces x 24 alpha x 15 theta0, N = 969).  Like the scan driver it works on
    lam_max's eigenpair by default; eigenpair="nearest" runs every equilibrium's scan in upstream's mode (the eigenpair nearest
    sigma = 1.0 / 1.3 |gam| + 0.05 / 0.42: BallooningScan's eigenpair="nearest"), with the same chunking, gather and objective.
    jac="exact" refines every surface on the exact gradient of gam (BallooningScan's jac="exact"), jac="exact_tangent" on the
    gradient that is exact in alpha as well, from one line per point (BallooningScan's jac="exact_tangent"); "reference" is the default.
    certify=True (eigenpair="max" only, else ValueError) certifies and re-closes the coarse tables and the final solves of every
    equilibrium (BallooningScan's certify=True; the refinement's own evaluations are not certified): the counts travel with the rows'
    one copy into .last_certificate = dict(checked, reclosed, failed), summed over the ranks; failed > 0 raises IbsError.
    n_starts=K > 1 (an integer in [1, 16], else ValueError) refines every surface of every equilibrium from the K best peaks of its
    coarse table and reports the best candidate (BallooningScan's n_starts); run()'s result keeps its keys.  n_starts=1, the default,
    builds the scan exactly as before.

    Upstream this is ball_submit.py:64-95 (one `srun ball_scan.py iter dof ngroups` per DOF-perturbed equilibrium, each
    running vmec_splines -> coarse scan -> argmax -> L-BFGS-B -> final solve, ball_scan.py:190-347) followed by
    sims_runner_NCSX.py:249-261 (objective of every equilibrium, forward-difference gradient over the DOFs).  Here the
    equilibria of a rank form ONE batch: the radial spline step for all of them (SurfaceTables.from_wouts), one geometry
    launch, one scan + argmax call, one refinement call, one final solve, one copy of the rows (BallooningScan.device_rows).
    With world > 1 the equilibria are dealt round-robin over the ranks (the reference's DP-1 level) and ONE
    all-gather of [n_eq_local][n_surf * 3] doubles assembles the table everywhere.

    SIMSOPT / VMEC stay outside: `wouts` are the wout tables of the (already converged) equilibria, `f_other` the
    non-ballooning part of each equilibrium's objective (Simsopt_runner.py -> f{dof}.npy), `steps` the DOF steps
    (dof_steps / ScanConfig.dof_step)."""

    def __init__(self, ctx, theta, svals, device, nalpha=24, ntheta0=15, del_alpha=0.004, gamma_thresh=-2.0e-4, prefac=50.0,
                 rank=0, world=1, dist=None, n_threads=0, n_chunks=4, gather_device=None, chunk_growth=1.0, eigenpair="max",
                 jac="reference", certify=False, n_starts=1):
        from .scan import check_eigenpair, check_jac, check_n_starts
        self.n_starts = check_n_starts(n_starts)
        self.eigenpair = check_eigenpair(eigenpair)
        self.jac = check_jac(jac)
        self.certify = bool(certify)
        if self.certify and self.eigenpair == "nearest":
            raise ValueError("certify=True applies to eigenpair='max': eigenpair='nearest' runs in division form with its a-priori bound")
        self.last_certificate = None
        self.ctx, self.device = ctx, device
        self.theta = np.asarray(theta, dtype=np.float64)
        self.svals = np.atleast_1d(np.asarray(svals, dtype=np.float64))       # ball_scan.py:197
        self.nalpha, self.ntheta0, self.del_alpha = int(nalpha), int(ntheta0), float(del_alpha)
        self.gamma_thresh, self.prefac = float(gamma_thresh), float(prefac)
        self.rank, self.world, self.dist, self.n_threads = int(rank), int(world), dist, int(n_threads)
        # the coarse part runs in n_chunks runs of equilibria: the host computes (ibs_surface_tables_f64) and uploads the tables
        # of run k + 1 while the GPU scans run k -- of the 2.2 ms the radial step of 73 equilibria takes, the first run's share
        # is all that stays exposed
        self.n_chunks = max(1, int(n_chunks))
        # (chunk_growth > 1: run k + 1 holds that many times the equilibria of run k -- a short first run exposes less host time;
        # the host must still finish run k + 1's tables while the GPU works on run k)
        self.chunk_growth = float(chunk_growth)
        self.gather_device = gather_device        # None: the rows are gathered where they are (RCCL); "cpu": through host copies (gloo)
        self._scan = None
        self._frame = None

    def _scan_for(self, tables, n_eq_local):
        from .scan import BallooningScan
        n = n_eq_local * len(self.svals)
        if self._scan is None or len(self._scan.rho_arr) != n:
            self._scan = BallooningScan(self.ctx, None, self.theta, np.tile(self.svals, n_eq_local), nalpha=self.nalpha,
                                        ntheta0=self.ntheta0, del_alpha=self.del_alpha, tables=tables, device=self.device,
                                        surf_index=np.arange(n), eigenpair=self.eigenpair, jac=self.jac,
                                        **(dict(certify=True) if self.certify else {}),
                                        **(dict(n_starts=self.n_starts) if self.n_starts > 1 else {}))
        self._scan.tables = tables
        return self._scan

    def run(self, wouts, f_other, steps, refine=True, phases=None):
        """wouts: the n_eq = n_dof + 1 equilibria (entry 0 = base); f_other (n_eq,); steps (n_eq,) with entry 0 unused.
        Returns dict(gam, theta0, alpha: (n_eq, n_surf); f0: (n_eq,); fobj = sqrt(f0[0]) (sims_runner_NCSX.py:318);
        dfobj: (n_dof,) (sims_runner_NCSX.py:258-261)), identical on every rank."""
        import time
        import torch
        from .geometry import SurfaceTables
        from .scan import gather_rows_tensor
        n_eq, ns = len(wouts), len(self.svals)
        own = shard_dofs(n_eq, self.rank, self.world)
        ncc = 3 if self.certify else 0     # trailing columns (checked, reclosed, failed): a rank's counts ride on its first row
        err = None
        try:                               # row of an equilibrium: n_surf x (theta0*, alpha*, gam) + the count of what went wrong
            if own:
                mine = [wouts[q] for q in own]
                fr = self._frame
                if fr is None or fr.n_equilibria != len(own) or not np.array_equal(fr._svals, self.svals) or \
                        fr._ns != int(mine[0]["ns"]) or len(fr.xm) != len(mine[0]["xm"]) or len(fr.xm_nyq) != len(mine[0]["xm_nyq"]):
                    pinned = str(self.device).startswith("cuda")
                    fr = self._frame = SurfaceTables.frame(mine[0], self.svals, len(own), pinned=pinned)
                    self._scan = None
                scan = self._scan_for(fr, len(own))
                nch = min(self.n_chunks, len(own))
                cuts = chunk_cuts(len(own), nch, self.chunk_growth); nch = len(cuts) - 1

                def fill(c0, c1):          # (owned-surface range -> equilibria range: chunks are cut at equilibrium boundaries)
                    q0, q1 = c0 // ns, c1 // ns
                    r0, r1 = fr.fill(q0, mine[q0:q1], self.n_threads)
                    if pinned_upload:
                        self.ctx.upload_tables_rows(fr, self.device, r0, r1)
                pinned_upload = str(self.device).startswith("cuda")
                if not pinned_upload:      # (CPU stand-ins in the tests: no device copies to manage)
                    fr.fill(0, mine, self.n_threads)
                r, bad = scan.device_rows(refine, phases, chunks=[(cuts[k] * ns, cuts[k + 1] * ns) for k in range(nch)],
                                          fill=fill if pinned_upload else None)
                rows = torch.cat([r.reshape(len(own), 3 * ns), bad.reshape(1, 1).expand(len(own), 1)], dim=1)
                if ncc:
                    cc = torch.zeros((len(own), 3), dtype=torch.float64, device=rows.device)
                    cc[0] = scan._cert_dev
                    rows = torch.cat([rows, cc], dim=1)
            else:
                rows = torch.zeros((0, 3 * ns + 1 + ncc), dtype=torch.float64, device=self.device)
        except Exception as e:             # (carried through the gather as NaN rows and raised on every rank afterwards)
            err = e
            rows = torch.full((len(own), 3 * ns + 1 + ncc), float("nan"), dtype=torch.float64, device=self.device)
        t0 = time.perf_counter()
        if self.gather_device is not None and self.world > 1:
            rows = rows.to(self.gather_device)
        full = gather_rows_tensor(rows, n_eq, self.rank, self.world, self.dist, self.ctx if getattr(self.ctx, "_comm_world", 0) == self.world else None)
        host = full.cpu().numpy()                                          # the one copy (and synchronisation)
        if err is not None:
            raise err
        if ncc:
            cc, host = np.nansum(host[:, -3:], axis=0), host[:, :-3]
            self.last_certificate = dict(checked=int(cc[0]), reclosed=int(cc[1]), failed=int(cc[2]))
            if self._scan is not None:
                self._scan.last_certificate = dict(self.last_certificate)
        if not np.all(np.isfinite(host)) or np.any(host[:, -1] != 0):
            raise IbsError("the scan of %d equilibria was flagged or produced non-finite growth rates" %
                           int(np.sum(~np.isfinite(host).all(axis=1) | (host[:, -1] != 0))))
        if ncc and self.last_certificate["failed"]:
            raise IbsError("%d of %d eigenvalues could not be certified (cert bits 0-2 after the re-close)"
                           % (self.last_certificate["failed"], self.last_certificate["checked"]))
        tab = host[:, :-1].reshape(n_eq, ns, 3)
        gam = tab[:, :, 2]
        f0 = ballooning_objective(f_other, gam, self.gamma_thresh, self.prefac)        # sims_runner_NCSX.py:254-257
        out = dict(theta0=tab[:, :, 0], alpha=tab[:, :, 1], gam=gam, f0=f0, fobj=float(np.sqrt(f0[0])),
                   dfobj=dof_fd_gradient(f0, steps))                                   # sims_runner_NCSX.py:258-261
        if phases is not None:
            phases["gather_copy_objective_ms"] = (time.perf_counter() - t0) * 1e3
        return out

    def sensitivity(self, wout0, points=None):
        """exact derivatives of every surface's growth rate of the BASE equilibrium wout0, pulled back to its wout data.
        points (n_surf, 2) = (alpha, theta0) per surface; None: the refined maximum of each surface (one BallooningScan of wout0 in
        this object's eigenpair / jac mode).  One geometry launch, one solve, one rows-VJP, one geometry-VJP
        (BallooningScan.sensitivity), then SurfaceTables.pullback per surface.  Returns dict(gam, alpha, theta0, dgam_dalpha,
        dgam_dtheta0: (n_surf,); wout_bar: per surface a dict of d gam_s / d (rmnc, ..., bsubvmnc (modes, ns), iotas, pres, phi (ns,),
        Aminor_p) -- the `sens` of linearised_dof_gradient).  Not sharded over ranks: every caller computes the same.
        run() is untouched by this and stays the way to the objective's gradient; this is the first-order alternative."""
        from .geometry import SurfaceTables
        from .scan import BallooningScan
        tables = SurfaceTables.from_wout(wout0, self.svals)
        ns = len(self.svals)
        scan = BallooningScan(self.ctx, None, self.theta, self.svals, nalpha=self.nalpha, ntheta0=self.ntheta0, del_alpha=self.del_alpha,
                              tables=tables, device=self.device, surf_index=np.arange(ns), eigenpair=self.eigenpair, jac=self.jac)
        if points is None:
            rows = scan.local_rows(True)
            points = np.stack([rows[:, 1], rows[:, 0]], axis=1)
        r = scan.sensitivity(points)
        host = {k: v.detach().cpu().numpy() for k, v in r.items()}
        bars = tables.pullback(host["tab_mn_bar"], host["tab_nyq_bar"], host["scal_bar"], per_surface=True)[0]
        # (surface k of the scan is its own copy of table row k: its cotangents live in row k alone)
        wout_bar = [{key: np.ascontiguousarray(v[k]) for key, v in bars.items()} for k in range(ns)]
        pts = np.asarray(points, dtype=np.float64).reshape(ns, 2)
        return dict(gam=host["gam"], alpha=pts[:, 0].copy(), theta0=pts[:, 1].copy(), dgam_dalpha=host["dgam_dalpha"],
                    dgam_dtheta0=host["dgam_dtheta0"], wout_bar=wout_bar)

    def marginal_sensitivity(self, wout0, points=None, jac="exact_tangent"):
        """exact derivatives of every surface's critical scale s* of the BASE equilibrium wout0, pulled back to its wout data: the
        margin's counterpart of sensitivity().  points (n_surf, 2) = (alpha, theta0) per surface; None: the refined margin of each
        surface (one BallooningScan.marginal(refine=True, jac=jac) of wout0; with jac="exact_tangent" the refined point is a
        stationary point of the s* differentiated here, which the envelope theorem needs).  One geometry launch, one alpha-tangent
        launch, one point launch with the cotangent planes, one geometry-VJP (BallooningScan.marginal_sensitivity), then
        SurfaceTables.pullback per surface.  Returns dict(scale, alpha, theta0, dscale_dalpha, dscale_dtheta0: (n_surf,); wout_bar:
        per surface a dict of d s*_s / d (rmnc, ..., bsubvmnc (modes, ns), iotas, pres, phi (ns,), Aminor_p) -- the `sens` of
        linearised_margin_gradient).  Not sharded over ranks: every caller computes the same.  The frozen-geometry caveat of
        BallooningScan.marginal applies."""
        from .geometry import SurfaceTables
        from .scan import BallooningScan
        tables = SurfaceTables.from_wout(wout0, self.svals)
        ns = len(self.svals)
        scan = BallooningScan(self.ctx, None, self.theta, self.svals, nalpha=self.nalpha, ntheta0=self.ntheta0, del_alpha=self.del_alpha,
                              tables=tables, device=self.device, surf_index=np.arange(ns))
        if points is None:
            m = scan.marginal(refine=True, jac=jac)
            points = np.stack([m["alpha"], m["theta0"]], axis=1)
        r = scan.marginal_sensitivity(points)
        host = {k: v.detach().cpu().numpy() for k, v in r.items()}
        bars = tables.pullback(host["tab_mn_bar"], host["tab_nyq_bar"], host["scal_bar"], per_surface=True)[0]
        # (surface k of the scan is its own copy of table row k: its cotangents live in row k alone)
        wout_bar = [{key: np.ascontiguousarray(v[k]) for key, v in bars.items()} for k in range(ns)]
        pts = np.asarray(points, dtype=np.float64).reshape(ns, 2)
        return dict(scale=host["scale"], alpha=pts[:, 0].copy(), theta0=pts[:, 1].copy(), dscale_dalpha=host["dscale_dalpha"],
                    dscale_dtheta0=host["dscale_dtheta0"], wout_bar=wout_bar)

    def marginal(self, wouts, steps=None, refine=True, jac="reference", n_starts=1, theta0_polish=False):
        """the marginal-stability scale s* of every surface of every equilibrium of the step (BallooningScan.marginal: the smallest
        critical scale of dPdrho over (alpha, theta0), refined from the coarse minimum unless refine=False), on the SurfaceTables
        frame, the sharding of equilibria over ranks and the ONE all-gather of run().  wouts as in run().
        Returns dict(scale, alpha, theta0: (n_eq, n_surf)), identical on every rank; with steps (n_eq,), entry 0 unused, also dscale
        (n_dof, n_surf) = (scale[1:] - scale[0]) / steps[1:, None]: the forward differences of sims_runner_NCSX.py:258-261 applied
        to the margin.  scale = inf (no scale makes the surface unstable) is a result, not a failure.  jac: the gradient the
        refinement runs on, as in BallooningScan.marginal ("reference", the default, or "exact_tangent").  n_starts, theta0_polish:
        passed to BallooningScan.marginal (multi-start refinement from the K best peaks of mu; start at the crest of the best line's
        theta0 envelope); a bad combination raises ValueError before anything runs; the defaults make the calls made before."""
        import torch
        from .geometry import SurfaceTables
        from .scan import check_marginal_jac, check_n_starts, gather_rows_tensor
        check_marginal_jac(jac)
        if theta0_polish and check_n_starts(n_starts) != 1:
            raise ValueError("theta0_polish=True takes n_starts=1")
        more = {}                          # (nothing at all with the defaults: the call is then exactly what it was)
        if check_n_starts(n_starts) != 1:
            more["n_starts"] = int(n_starts)
        if theta0_polish:
            more["theta0_polish"] = True
        n_eq, ns = len(wouts), len(self.svals)
        own = shard_dofs(n_eq, self.rank, self.world)
        err = None
        try:                               # row of an equilibrium: n_surf x (scale, alpha, theta0)
            if own:
                mine = [wouts[q] for q in own]
                fr = self._frame
                pinned = str(self.device).startswith("cuda")
                if fr is None or fr.n_equilibria != len(own) or not np.array_equal(fr._svals, self.svals) or \
                        fr._ns != int(mine[0]["ns"]) or len(fr.xm) != len(mine[0]["xm"]) or len(fr.xm_nyq) != len(mine[0]["xm_nyq"]):
                    fr = self._frame = SurfaceTables.frame(mine[0], self.svals, len(own), pinned=pinned)
                    self._scan = None
                scan = self._scan_for(fr, len(own))
                r0, r1 = fr.fill(0, mine, self.n_threads)
                if pinned:
                    self.ctx.upload_tables_rows(fr, self.device, r0, r1)
                m = scan.marginal(refine=refine, jac=jac, **more)
                local = np.stack([m["scale"], m["alpha"], m["theta0"]], axis=1).reshape(len(own), 3 * ns)
                rows = torch.from_numpy(np.ascontiguousarray(local, dtype=np.float64)).to(self.device)
            else:
                rows = torch.zeros((0, 3 * ns), dtype=torch.float64, device=self.device)
        except Exception as e:             # (carried through the gather as NaN rows and raised on every rank afterwards)
            err = e
            rows = torch.full((len(own), 3 * ns), float("nan"), dtype=torch.float64, device=self.device)
        if self.gather_device is not None and self.world > 1:
            rows = rows.to(self.gather_device)
        full = gather_rows_tensor(rows, n_eq, self.rank, self.world, self.dist, self.ctx if getattr(self.ctx, "_comm_world", 0) == self.world else None)
        host = full.cpu().numpy()
        if err is not None:
            raise err
        if np.any(np.isnan(host)):
            raise IbsError("the marginal-stability scan of %d equilibria failed (see that rank's error)" % int(np.sum(np.isnan(host).any(axis=1))))
        tab = host.reshape(n_eq, ns, 3)
        out = dict(scale=tab[:, :, 0], alpha=tab[:, :, 1], theta0=tab[:, :, 2])
        if steps is not None:
            out["dscale"] = (out["scale"][1:] - out["scale"][0]) / np.asarray(steps, dtype=np.float64)[1:, None]
        return out
