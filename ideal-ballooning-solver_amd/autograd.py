"""Differentiable growth rates: torch.autograd Functions over the HIP solver, whose backward is the exact vector-Jacobian product
of the library (Context.solve_gcf_vjp, ibs_solve_gcf_vjp_f64) -- the derivative of the very gam the forward returns (the FD4 /
Simpson quotient of utils.py:1601-1621), not the Hellmann-Feynman formulas of utils.py:1666-1725.

    from ibs_amd import autograd as iag
    gam = iag.growth_rate(h, bmag, gradpar, cvdrift, cvdrift0, gds2, gds21, gds22, dPdrho, theta0)
    gam.sum().backward()            # gradients in every geometry array, dPdrho and theta0

    geo, dP = iag.fieldline_geometry(tables, line_surf, line_alpha, theta, tab_mn=tm, tab_nyq=tq, scal=sc)
    gam = iag.growth_rate(h, *geo[:7], dP, theta0)
    gam.sum().backward()            # gradients in the surface tables tm, tq, the scalars sc and line_alpha

    gam = iag.gamma_scan(h, *geo[:7], dP, theta0)       # theta0 (n_theta0,): the scan kernel forward, ONE ibs_gamma_scan_vjp_f64 backward
    objective.smooth_max(gam.reshape(n_surf, n_alpha, -1), 20.0).sum().backward()

    lam = iag.local_eq_lam(theta[0], h, geo, dP, alpha, sigma, line_of, var)            # lam_max at (line, theta0, eps, p) points
    t = iag.local_eq_crossing(theta[0], h, geo, dP, alpha, sigma, rays)                # first stable -> unstable crossing of every (line, ray)
    t.nansum().backward()           # the implicit-function rule on lam_max(t*) = shift, through the geometry to the tables

Float64 CUDA tensors throughout; uniform grids, odd N in [66, 65537] (the limits of the kernels).  A backward whose VJP flags a system
(status bits 0-1 of ibs_solve_gcf_vjp_f64) issues a VjpStatusWarning.  `import ibs_amd` does not import
this module, nor torch."""
import warnings

import torch

from .solver import BASIS_BIT, CLUSTER_BIT, OPEN_CLUSTER_BIT, IbsError, VjpStatusWarning, default_context, vjp_status_message

_MODES = ("max", "nearest")


def _check_mode(eigenpair, sigma):
    if eigenpair not in _MODES:
        raise ValueError("eigenpair must be 'max' or 'nearest', not %r" % (eigenpair,))
    if eigenpair == "nearest" and sigma is None:
        raise ValueError("eigenpair='nearest' needs sigma")


class _SolveGcf(torch.autograd.Function):
    @staticmethod
    def forward(fctx, h, g, c, f, eigenpair, sigma, ictx):
        if eigenpair == "max":
            r = ictx.solve_gcf(h, g, c, f, want_X=True)
        else:
            r = ictx.solve_gcf_nearest(h, g, c, f, sigma, want_X=True)
        fctx.save_for_backward(g, c, f, r["lam"], r["X"])
        fctx.h, fctx.ictx = h, ictx
        return r["gam"], r["lam"]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(fctx, gam_bar, lam_bar):
        g, c, f, lam, X = fctx.saved_tensors
        r = fctx.ictx.solve_gcf_vjp(fctx.h, g, c, f, lam, X, gam_bar=gam_bar.contiguous(), lam_bar=lam_bar.contiguous(),
                                    want_info=True)
        st = (r["info"] >> 16) & 3
        n_pivot, n_bad = torch.stack([(st & 1).ne(0).sum(), (st & 2).ne(0).sum()]).tolist()     # (one host synchronisation)
        if n_pivot or n_bad:
            warnings.warn(vjp_status_message(n_pivot, n_bad), VjpStatusWarning, stacklevel=2)
        return None, r["g_bar"], r["c_bar"], r["f_bar"], None, None, None


def solve_gcf(h, g, c, f, eigenpair="max", sigma=None, ctx=None):
    """(gam, lam), each (n_sys,), of the raw systems g, c, f (n_sys, N): lam_max's eigenpair (Context.solve_gcf) or, with
    eigenpair="nearest", the one nearest sigma (a scalar or (n_sys,): Context.solve_gcf_nearest).  Differentiable in g, c and f;
    the eigenpair is locally constant in sigma (no gradient)."""
    _check_mode(eigenpair, sigma)
    return _SolveGcf.apply(float(h), g, c, f, eigenpair, sigma, ctx or default_context(g.device.index or 0))


class _SolveGcfModes(torch.autograd.Function):
    @staticmethod
    def forward(fctx, h, g, c, f, n_modes, ictx, mean):
        r = ictx.solve_gcf_modes(h, g, c, f, n_modes, want_X=True, want_info=True, basis=mean)
        st = r["info"] >> 16
        cluster, lam = (st & CLUSTER_BIT).ne(0), r["lam"]
        pool = []
        if mean:
            # a COMPLETE cluster: every member has its basis vector and none lies below the last mode (cluster_first names the group)
            cf = r["cluster_first"].long()
            over = lambda v: torch.zeros_like(lam).scatter_add_(1, cf, v.to(lam.dtype)).gather(1, cf)      # summed over the group
            size = over(torch.ones_like(lam))
            pooled = cluster & over(cluster & ((st & BASIS_BIT).eq(0) | (st & OPEN_CLUSTER_BIT).ne(0))).eq(0)
            lam = torch.where(pooled, over(r["lam"]) / size, r["lam"])
            pool = [cf, size, pooled]
        fctx.save_for_backward(g, c, f, r["lam"], r["X"], cluster, *pool)
        fctx.h, fctx.ictx = h, ictx
        return r["gam"], lam

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(fctx, gam_bar, lam_bar):
        g, c, f, lam, X, cluster, *pool = fctx.saved_tensors
        if pool:
            # lam of every member of a complete cluster is the cluster's mean: its members' cotangents, pooled and divided by m, go
            # to each member's own lam-only VJP -- the sum is the derivative of the mean, which exists.  gam of a member has none.
            cf, size, pooled = pool
            share = torch.zeros_like(lam_bar).scatter_add_(1, cf, torch.where(pooled, lam_bar, torch.zeros_like(lam_bar))).gather(1, cf) / size
            lam_bar = torch.where(pooled, share, lam_bar)
            cluster = cluster & ~(pooled & gam_bar.eq(0))
        active = gam_bar.ne(0) | lam_bar.ne(0)                    # (n_sys, n_modes): the pairs the cotangent reaches
        rows = [torch.zeros_like(g), torch.zeros_like(c), torch.zeros_like(f)]
        flags = [(active & cluster).any(1).sum()]
        # (the VJP of an active mode runs on all systems, those with a clustered or untouched pair included: their rows and status
        # words are masked out below, which is cheaper than gathering the systems of every mode)
        for m in [m for m, on in enumerate(active.any(0).tolist()) if on]:
            r = fctx.ictx.solve_gcf_vjp(fctx.h, g, c, f, lam[:, m].contiguous(), X[:, m].contiguous(), gam_bar=gam_bar[:, m].contiguous(),
                                        lam_bar=lam_bar[:, m].contiguous(), want_info=True)
            use = (active[:, m] & ~cluster[:, m])[:, None]        # (a clustered pair with a zero cotangent contributes nothing)
            for acc, k in zip(rows, ("g_bar", "c_bar", "f_bar")):
                acc += torch.where(use, r[k], torch.zeros_like(acc))
            st = ((r["info"] >> 16) & 3) * use[:, 0]
            flags += [(st & 1).ne(0).sum(), (st & 2).ne(0).sum()]
        refused = (active & cluster).any(1)[:, None]              # the derivative of one member of a cluster does not exist
        rows = [torch.where(refused, torch.full_like(a, float("nan")), a) for a in rows]
        n = torch.stack(flags).tolist()                           # (one host synchronisation)
        n_cluster, n_pivot, n_bad = n[0], sum(n[1::2]), sum(n[2::2])
        parts = [vjp_status_message(n_pivot, n_bad)] if n_pivot or n_bad else []
        if n_cluster:
            parts.append("solve_gcf_modes: %d system(s) with a cotangent on a clustered mode (status bit 9: one member of a cluster has "
                         "no derivative of its own, NaN rows)" % n_cluster)
        if parts:
            warnings.warn("; ".join(parts), VjpStatusWarning, stacklevel=2)
        return None, rows[0], rows[1], rows[2], None, None, None


def solve_gcf_modes(h, g, c, f, n_modes, ctx=None, cluster="refuse"):
    """(gam, lam), each (n_sys, n_modes), of the n_modes largest eigenpairs of the raw systems g, c, f (n_sys, N), mode 0 = lam_max's
    (Context.solve_gcf_modes).  Differentiable in g, c and f: the backward is one Context.solve_gcf_vjp per mode the cotangent
    reaches, on that mode's (lam, X) and cotangent columns, summed.  A clustered mode (status bit 9: a neighbouring eigenvalue within
    4 N eps ||A||) has no derivative of its own: with a non-zero cotangent the system's rows are NaN and a VjpStatusWarning is issued;
    with a zero cotangent it contributes nothing.
    cluster="mean": the forward builds the Ritz basis of every cluster (Context.solve_gcf_modes(basis=True)) and every member of a
    complete cluster -- all its members found, none below the last mode asked for -- returns the cluster's MEAN lam, whose derivative
    exists: (1 / m) sum_i x_i^T (dS - lam_i dF) x_i / x_i^T F x_i over the basis, i.e. the members' lam-only VJPs with their
    cotangents pooled and divided by m.  A cotangent on gam of a clustered mode, or on any member of an open or incomplete
    cluster, is refused as above."""
    if cluster not in ("refuse", "mean"):
        raise ValueError("cluster must be 'refuse' or 'mean', not %r" % (cluster,))
    return _SolveGcfModes.apply(float(h), g, c, f, int(n_modes), ctx or default_context(g.device.index or 0), cluster == "mean")


class _MarginalScale(torch.autograd.Function):
    @staticmethod
    def forward(fctx, h, g, c, ictx):
        r = ictx.marginal_gcf(h, g, c, want_grad=True)
        fctx.save_for_backward(r["g_bar"], r["c_bar"])
        return r["scale"]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(fctx, s_bar):
        g_bar, c_bar = fctx.saved_tensors
        return None, g_bar * s_bar[:, None], c_bar * s_bar[:, None], None


def marginal_scale(h, g, c, ctx=None):
    """s* (n_sys,) of the raw rows g, c (n_sys, N): the critical scale of c at fixed g (Context.marginal_gcf; s* < 1 = unstable
    now).  Differentiable in g and c: the backward is the cotangent times the derivative rows the forward's kernel returns
    (Hellmann-Feynman on the discrete pencil, exact for it).  Systems with an infinite margin (no c_j > 0) get zero gradients,
    flagged ones (invalid data) NaN."""
    return _MarginalScale.apply(float(h), g, c, ctx or default_context(g.device.index or 0))


class _MarginalPoints(torch.autograd.Function):
    @staticmethod
    def forward(fctx, h, geo, geo_da, theta0, ictx):
        r = ictx.marginal_obj_w_grad_tangent(h, geo, geo_da, theta0, want_grad=True, want_geo_bar=True, want_info=True)
        nbad = int(((r["info"] >> 16) & 3).ne(0).sum().item())                 # (bit 8, an infinite margin, is informational)
        if nbad:
            raise IbsError("%d of %d marginal-stability solves were flagged (status bits 0-1: iteration cap or invalid data)"
                           % (nbad, r["info"].numel()))
        fctx.save_for_backward(r["geo_bar"], r["dscale"])
        fctx.mark_non_differentiable(r["dscale"], r["dPdrho"])
        return r["scale"], r["dscale"], r["dPdrho"]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(fctx, s_bar, _ds_bar, _dP_bar):
        geo_bar, dscale = fctx.saved_tensors
        return None, geo_bar * s_bar[None, :, None], None, dscale[:, 1] * s_bar, None


def marginal_points_full(h, geo, geo_da, theta0, ctx=None):
    """marginal_points with the alpha-tangent planes geo_da (8, n_pts, N) of the lines given: (scale, dscale (n_pts, 2) = (d s* / d alpha,
    d s* / d theta0), dPdrho), the last two without gradient (BallooningScan.marginal_sensitivity)"""
    return _MarginalPoints.apply(float(h), geo, geo_da, theta0, ctx or default_context(geo.device.index or 0))


def marginal_points(h, geo, theta0, ctx=None):
    """s* (n_pts,) of the field lines geo (8, n_pts, N) -- the planes fieldline_geometry returns -- at theta0 (n_pts,), each line with
    its own dPdrho: the critical scale of the pressure gradient at fixed geometry arrays (Context.marginal_obj_w_grad_tangent,
    ibs_marginal_obj_w_grad_tangent_f64).  Differentiable in geo and theta0: the backward is the cotangent times the planes geo_bar and
    the theta0 derivative the forward's kernel returns (Hellmann-Feynman on the discrete pencil, exact for it; the dependence through
    the line's dPdrho is inside geo_bar).  Composes with fieldline_geometry, so that s.sum().backward() reaches tab_mn, tab_nyq, scal
    and line_alpha.  Points with an infinite margin (no c_j > 0) get zero gradients; status bits 0-1 raise IbsError."""
    return marginal_points_full(h, geo, torch.zeros_like(geo), theta0, ctx)[0]


def growth_rate(h, bmag, gradpar, cvdrift, cvdrift0, gds2, gds21, gds22, dPdrho, theta0, eigenpair="max", sigma=None, ctx=None):
    """gam (n_lines, n_theta0) of the lines (geometry arrays (n_lines, N), dPdrho (n_lines,)) at theta0 ((n_theta0,), shared by all
    lines as in Context.gamma_scan, or (n_lines, n_theta0)): the theta0 fold of ball_scan.py:267-268 and the coefficients of
    utils.py:1560-1562 as torch expressions on the device, then solve_gcf.  Differentiable in every tensor argument.
    eigenpair="nearest": the eigenpair nearest sigma (a scalar or (n_lines, n_theta0))."""
    _check_mode(eigenpair, sigma)
    n_lines, N = bmag.shape
    t0 = theta0 if theta0.dim() == 2 else theta0.expand(n_lines, theta0.shape[0])
    n_t0 = t0.shape[1]
    t = t0[:, :, None]
    cv = cvdrift[:, None, :] + t * cvdrift0[:, None, :]                                   # ball_scan.py:267
    gd = gds2[:, None, :] + 2 * t * gds21[:, None, :] + t ** 2 * gds22[:, None, :]      # ball_scan.py:268
    gp = torch.abs(gradpar)[:, None, :]
    B = bmag[:, None, :]
    g = gp * gd / B                                                                     # utils.py:1560
    c = -1 * dPdrho[:, None, None] * cv * 1 / (gp * B)                                  # utils.py:1561
    f = gd / B ** 2 * 1 / (gp * B)                                                      # utils.py:1562
    if eigenpair == "nearest":
        sigma = torch.as_tensor(sigma, dtype=torch.float64, device=bmag.device)
        sigma = sigma.expand(n_lines, n_t0).reshape(-1) if sigma.dim() == 0 else sigma.reshape(-1)
    gam, _ = solve_gcf(h, g.reshape(-1, N), c.reshape(-1, N), f.reshape(-1, N), eigenpair, sigma, ctx)
    return gam.reshape(n_lines, n_t0)


GAM_RESOLVE_TOL = 1e-8     # the library's stated FP64 tolerance on gam: how far the backward's own solve may be from the forward's


class _GammaScan(torch.autograd.Function):
    @staticmethod
    def forward(fctx, h, bmag, gradpar, cvdrift, cvdrift0, gds2, gds21, gds22, dPdrho, theta0, eigenpair, sigma, ictx):
        geo7 = (bmag, gradpar, cvdrift, cvdrift0, gds2, gds21, gds22)
        if eigenpair == "max":
            gam = ictx.gamma_scan(h, *geo7, dPdrho, theta0)["gam"]
        else:
            gam = ictx.gamma_scan_nearest(h, *geo7, dPdrho, theta0, sigma)["gam"]
        fctx.save_for_backward(*geo7, dPdrho, theta0, gam, *([sigma] if eigenpair == "nearest" else []))
        fctx.h, fctx.ictx = h, ictx
        return gam

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(fctx, gam_bar):
        *geo7, dPdrho, theta0, gam = fctx.saved_tensors[:10]
        sigma = fctx.saved_tensors[10] if len(fctx.saved_tensors) > 10 else None
        need = fctx.needs_input_grad
        want = [k for k, on in (("geo", any(need[1:8])), ("dPdrho", need[8]), ("theta0", need[9])) if on]
        if not want:
            return (None,) * 13
        r = fctx.ictx.gamma_scan_vjp(fctx.h, *geo7, dPdrho, theta0, gam_bar.contiguous(), sigma=sigma, want=want, want_info=True)
        # the backward re-solved in division form: a line on which its gam is not the forward's (another eigenpair: clustered modes, a
        # nearest pair that changed hands) has no gradient here
        active = gam_bar.ne(0)
        moved = (active & ~((r["gam"] - gam).abs() <= GAM_RESOLVE_TOL)).any(1)
        st = ((r["info"] >> 16) & 3) | (((r["info"] >> (16 + 6)) & 2))           # solve failed | adjoint refused
        n_moved, n_pivot, n_bad = torch.stack([moved.sum(), (active & ((r["info"] >> (16 + 6)) & 1).ne(0)).sum(),
                                               (active & st.ne(0)).sum()]).tolist()     # (one host synchronisation)
        parts = [vjp_status_message(n_pivot, n_bad)] if n_pivot or n_bad else []
        if n_moved:
            parts.append("gamma_scan: %d line(s) on which the backward's division-form solve gave a gam more than %g from the forward's "
                         "(another eigenpair: NaN gradients)" % (n_moved, GAM_RESOLVE_TOL))
        if parts:
            warnings.warn("; ".join(parts), VjpStatusWarning, stacklevel=2)
        nan = float("nan")
        geo_bar = r["geo_bar"]
        if geo_bar is not None:
            geo_bar = torch.where(moved[None, :, None], torch.full_like(geo_bar, nan), geo_bar)
        dP_bar = r["dPdrho_bar"]
        if dP_bar is not None:
            dP_bar = torch.where(moved, torch.full_like(dP_bar, nan), dP_bar)
        t0_bar = r["theta0_bar"]
        if t0_bar is not None:
            t0_bar = torch.where(moved[:, None], torch.full_like(t0_bar, nan), t0_bar).sum(0)      # theta0 is shared by the lines
        planes = [geo_bar[k] if geo_bar is not None and need[1 + k] else None for k in range(7)]
        return (None, *planes, dP_bar, t0_bar, None, None, None)


def gamma_scan(h, bmag, gradpar, cvdrift, cvdrift0, gds2, gds21, gds22, dPdrho, theta0, eigenpair="max", sigma=None, ctx=None):
    """gam (n_lines, n_theta0) of the lines (geometry arrays (n_lines, N), dPdrho (n_lines,)) at theta0 (n_theta0,), shared by all lines:
    the forward is the scan kernel itself (Context.gamma_scan, or gamma_scan_nearest with eigenpair="nearest" and sigma a scalar or
    (n_lines, n_theta0)), the backward ONE Context.gamma_scan_vjp call (ibs_gamma_scan_vjp_f64): the (g, c, f) rows of the systems
    never become torch tensors.  Differentiable in the seven arrays, dPdrho and theta0 (its gradient is the sum over the lines).
    Composes with fieldline_geometry: gamma_scan(h, *geo[:7], dP, theta0).  The backward solves again, in division form; a line
    on which that gam is more than 1e-8 from the forward's gets NaN gradients and a VjpStatusWarning, as do status bits 0-1 and 7 of
    the VJP.  growth_rate is the same function through torch expressions (and takes per-line theta0)."""
    _check_mode(eigenpair, sigma)
    if theta0.dim() != 1:
        raise ValueError("gamma_scan takes theta0 (n_theta0,), shared by the lines; growth_rate takes (n_lines, n_theta0)")
    if eigenpair == "nearest":
        sigma = torch.as_tensor(sigma, dtype=torch.float64, device=bmag.device)
        sigma = sigma.expand(bmag.shape[0], theta0.shape[0]).contiguous() if sigma.dim() == 0 else sigma
    return _GammaScan.apply(float(h), bmag, gradpar, cvdrift, cvdrift0, gds2, gds21, gds22, dPdrho, theta0, eigenpair, sigma,
                            ctx or default_context(bmag.device.index or 0))


class _FieldlineGeometry(torch.autograd.Function):
    @staticmethod
    def forward(fctx, tables, line_surf, line_alpha, theta, tab_mn, tab_nyq, scal, ictx):
        r = ictx.fieldline_geometry(tables, line_surf, line_alpha, theta, device=line_alpha.device, tabs=(tab_mn, tab_nyq, scal))
        fctx.save_for_backward(line_surf, line_alpha, theta, tab_mn, tab_nyq, scal)
        fctx.tables, fctx.ictx = tables, ictx
        return r["geo"], r["dPdrho"]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(fctx, geo_bar, dP_bar):
        line_surf, line_alpha, theta, tab_mn, tab_nyq, scal = fctx.saved_tensors
        need = fctx.needs_input_grad
        want = [k for k, i in (("alpha", 2), ("tab_mn", 4), ("tab_nyq", 5), ("scal", 6)) if need[i]]
        if not want:
            return (None,) * 8
        r = fctx.ictx.fieldline_geometry_vjp(fctx.tables, line_surf, line_alpha, theta, geo_bar.contiguous(), dP_bar.contiguous(),
                                             device=line_alpha.device, want=want, tabs=(tab_mn, tab_nyq, scal))
        return None, None, r["alpha_bar"], None, r["tab_mn_bar"], r["tab_nyq_bar"], r["scal_bar"], None


def fieldline_geometry(tables, line_surf, line_alpha, theta, tab_mn=None, tab_nyq=None, scal=None, ctx=None):
    """(geo (8, n_lines, N), dPdrho (n_lines,)) of the field lines (surface line_surf[i], label line_alpha[i]) on the grid theta:
    Context.fieldline_geometry on the device.  Differentiable in line_alpha and in tab_mn (n_surf, 6, mnmax), tab_nyq (n_surf, 7,
    mnmax_nyq), scal (n_surf, 6) when these are given as device tensors; each defaults to the values of `tables` (its resident
    device copy), then without gradient.  line_surf then indexes the tensors given; the mode tables are those of `tables`.  The
    backward is the library's exact vector-Jacobian product (Context.fieldline_geometry_vjp, ibs_fieldline_geometry_vjp_f64): the
    root solve of utils.py:391-416 by the implicit-function theorem.  theta gets no gradient.
    line_surf: int tensor (n_lines,); line_alpha, theta: float64 device tensors."""
    ictx = ctx or default_context(line_alpha.device.index or 0)
    if tab_mn is None or tab_nyq is None or scal is None:
        d = ictx._device_tables(tables, line_alpha.device)
        given = [t for t in (tab_mn, tab_nyq, scal) if t is not None]
        if given and any(int(t.shape[0]) != len(tables.s) for t in given):
            raise ValueError("tab_mn, tab_nyq and scal must hold the same surfaces: give all three or the tables' own count")
        tab_mn, tab_nyq, scal = (d[4] if tab_mn is None else tab_mn, d[5] if tab_nyq is None else tab_nyq,
                                 d[6] if scal is None else scal)
    line_surf = torch.as_tensor(line_surf, device=line_alpha.device).to(torch.int32)
    return _FieldlineGeometry.apply(tables, line_surf, line_alpha, theta, tab_mn, tab_nyq, scal, ictx)


def _raise_flagged(info, what):
    nbad = int(((info >> 16) & 3).ne(0).sum().item())
    if nbad:
        raise IbsError("%d of %d %s were flagged (status bits 0-1: iteration cap or invalid data)" % (nbad, info.numel(), what))


class _LocalEqLam(torch.autograd.Function):
    @staticmethod
    def forward(fctx, theta_lo, h, geo, dPdrho, centre, sigma, line_of, var, ps, ictx):
        r = ictx.local_eq_grad(theta_lo, h, geo, dPdrho, centre, sigma, line_of, var, ps=ps, want_geo_bar=True, want_info=True)
        _raise_flagged(r["info"], "local-equilibrium points")
        fctx.save_for_backward(r["geo_bar"], r["dlam"], line_of.to(torch.int64))
        fctx.n_lines = int(geo.shape[1])
        return r["lam"]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(fctx, lam_bar):
        geo_bar, dlam, line_of = fctx.saved_tensors
        N = geo_bar.shape[2]
        gb = torch.zeros((8, fctx.n_lines, N), dtype=geo_bar.dtype, device=geo_bar.device).index_add_(1, line_of, geo_bar * lam_bar[None, :, None])
        dP = torch.zeros(fctx.n_lines, dtype=geo_bar.dtype, device=geo_bar.device).index_add_(0, line_of, dlam[:, 3] * lam_bar)
        return None, None, gb, dP, None, None, None, dlam[:, :3] * lam_bar[:, None], None, None


def local_eq_lam(theta_lo, h, geo, dPdrho, centre, sigma, line_of, var, ps=None, ctx=None):
    """lam_max (n_pts,) at the points (line_of[k], var[k] = (theta0, eps, p)) of the local-equilibrium rule on the lines geo (8, n_lines,
    N), dPdrho (n_lines,) on the grid theta_lo + j h -- the planes fieldline_geometry returns -- with centre, sigma (n_lines,) and the
    optional ps (n_lines, N) of Context.local_eq_scan (Context.local_eq_grad, ibs_local_eq_grad_f64).  Differentiable in geo, dPdrho
    and var: the backward is the cotangent times the planes and the derivatives the forward's kernel returns (Hellmann-Feynman on the
    discrete pencil, exact for the lam returned; lam_max must be simple), summed over the points of a line.  centre, sigma, ps and the
    grid get no gradient.  Composes with fieldline_geometry.  Status bits 0-1 raise IbsError."""
    ictx = ctx or default_context(geo.device.index or 0)
    line_of = torch.as_tensor(line_of, device=geo.device).to(torch.int32)
    var = torch.as_tensor(var, dtype=geo.dtype, device=geo.device)
    return _LocalEqLam.apply(float(theta_lo), float(h), geo, dPdrho, centre, sigma, line_of, var, ps, ictx)


class _LocalEqCrossing(torch.autograd.Function):
    @staticmethod
    def forward(fctx, theta_lo, h, geo, dPdrho, centre, sigma, rays, ps, shift, xtol, ictx):
        b = ictx.local_eq_boundary_grad(theta_lo, h, geo, dPdrho, centre, sigma, rays, ps=ps, shift=shift, xtol=xtol, want_geo_bar=True)
        _raise_flagged(b["info"], "local-equilibrium boundary systems")
        if b["grad_nbad"]:
            raise IbsError("%d local-equilibrium points at the crossings were flagged (status bits 0-1)" % b["grad_nbad"])
        up = b["t_stable"] < b["t_unstable"]                 # (NaN beyond n_cross: False)
        has = up.any(dim=2)
        first = up.to(torch.int8).argmax(dim=2)
        t = torch.where(has, b["t"].gather(2, first[..., None])[..., 0], torch.full_like(b["t"][..., 0], float("nan")))
        l_sel, r_sel = torch.nonzero(has, as_tuple=True)
        c_sel = first[l_sel, r_sel]
        # the rows of dt_geo of the chosen crossings: pts lists every gathered crossing in (line, ray, crossing) order
        where = torch.full(tuple(up.shape), -1, dtype=torch.int64)
        pts = torch.from_numpy(b["pts"])
        where[pts[:, 0], pts[:, 1], pts[:, 2]] = torch.arange(len(pts))
        sel = where.to(geo.device)[l_sel, r_sel, c_sel]
        fctx.save_for_backward(b["dt_geo"][:, sel], b["dt"][l_sel, r_sel, c_sel], t[l_sel, r_sel], l_sel, r_sel)
        fctx.shape = (int(geo.shape[1]), int(rays.shape[0]))
        lt = torch.where(has, b["dlam_dt"].gather(2, first[..., None])[..., 0], torch.full_like(t, float("nan")))
        fctx.mark_non_differentiable(lt)
        return t, lt

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(fctx, t_bar, _lt_bar):
        dt_geo, dt, t, l_sel, r_sel = fctx.saved_tensors
        n_lines, n_ray = fctx.shape
        tb = t_bar[l_sel, r_sel]
        kw = dict(dtype=dt.dtype, device=dt.device)
        gb = torch.zeros((8, n_lines, dt_geo.shape[2]), **kw).index_add_(1, l_sel, dt_geo * tb[None, :, None])
        dP = torch.zeros(n_lines, **kw).index_add_(0, l_sel, dt[:, 4] * tb)
        z = torch.zeros_like(tb)
        # t* depends on d_eps and d_p through the triple at t*: eps = eps0 + t d_eps, p = p0 + t d_p
        cols = torch.stack([dt[:, 0] * tb, dt[:, 1] * tb, dt[:, 2] * tb, t * dt[:, 1] * tb, t * dt[:, 2] * tb, z, z], dim=1)
        rb = torch.zeros((n_ray, 7), **kw).index_add_(0, r_sel, cols)
        return None, None, gb, dP, None, None, rb, None, None, None, None


def local_eq_crossing(theta_lo, h, geo, dPdrho, centre, sigma, rays, ps=None, shift=0.0, xtol=1e-12, ctx=None, want_slope=False):
    """t* (n_lines, n_ray) of the FIRST stable -> unstable crossing of every line along every ray (n_ray, 7) = (theta0, eps0, p0, d_eps,
    d_p, t_lo, t_hi) of Context.local_eq_boundary, NaN where a (line, ray) has none among the returned crossings.  Differentiable in
    geo, dPdrho and the rays' (theta0, eps0, p0, d_eps, d_p): the backward is the implicit-function rule on lam_max(t*) = shift,
    d t* / d (.) = -lam_(.) / lam_t with the derivatives of lam_max from ONE Context.local_eq_grad call at the crossings
    (Context.local_eq_boundary_grad); the cotangent of a ray is summed over the lines, that of a line over the rays.  t_lo, t_hi, shift,
    centre, sigma and ps get no gradient.  At a tangency lam_t -> 0 and the gradients are inf or NaN by arithmetic: want_slope=True
    returns (t*, lam_t) so that the caller can judge.  Composes with fieldline_geometry.  Status bits 0-1 raise IbsError."""
    ictx = ctx or default_context(geo.device.index or 0)
    rays = torch.as_tensor(rays, dtype=geo.dtype, device=geo.device)
    t, lt = _LocalEqCrossing.apply(float(theta_lo), float(h), geo, dPdrho, centre, sigma, rays, ps, float(shift), float(xtol), ictx)
    return (t, lt) if want_slope else t
