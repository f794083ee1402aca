"""Drop-in operators with the reference's names and signatures (utils.py:1550-1552, 1632).

    from ibs_amd import gamma_ball_full          # instead of `from utils import *` (ball_scan.py:19)

`vguess` only steers ARPACK upstream (utils.py:1597) and is accepted and ignored.  `sigma0` is ARPACK's shift: the reference
returns the eigenpair NEAREST sigma0, this library always the LARGEST eigenvalue's.  The two are the same eigenpair whenever
lam_max < sigma0 -- the case the reference is written for (sigma0 = 1.0 / 1.3 |gam| + 0.05 / 0.42 against growth rates of
1e-4 .. 1e-1: ball_scan.py:230, 289, 337) and the only one observed -- and ONLY then: with lam_max >= sigma0 upstream would
have returned another eigenpair (or lam_max itself, if it happens to be the nearest).  The drop-in reports that case instead of
hiding it: the solve carries the informational status bit 4 (include/ibs.h), `gamma_ball_full(..., info=d)` fills
d["above_sigma0"], and a NearestSigmaWarning is issued.  All eigen-work runs on the GPU through libibs_hip.so; the only host
arithmetic is the elementwise coefficient formulas returned to the caller as (g, c, f).

Two modes, chosen by `eigenpair`:
  "max"      (the default) lam_max's eigenpair -- the physical one: the largest growth rate of the line, what the scan driver
             (scan.py) and AdjointStep use throughout;
  "nearest"  the eigenpair nearest sigma0 -- the FAITHFUL one: what utils.py:1597 returns on every input, lam_max >= sigma0
             included (include/ibs.h: ibs_solve_gcf_nearest_f64).  No NearestSigmaWarning: there is nothing to report.
"""
import warnings

import numpy as np

from .solver import VjpStatusWarning, default_context, vjp_status_message
from ._lib import IbsError


def uniform_spacing(theta, rtol=1e-9):
    """h of a uniform grid (the batched geometry-fed entry points need one; gamma_ball_full also accepts
    non-uniform grids and regrids like the reference)."""
    theta = np.asarray(theta, dtype=np.float64)
    N = len(theta)
    h = (theta[-1] - theta[0]) / (N - 1)
    if np.max(np.abs(np.diff(theta) - h)) > rtol * abs(h) * N:
        raise IbsError("theta grid is not uniform: the batched entry points need a uniform grid (use gamma_ball_full)")
    return float(h)


def is_uniform(theta, rtol=1e-9):
    theta = np.asarray(theta, dtype=np.float64)
    h = (theta[-1] - theta[0]) / (len(theta) - 1)
    return bool(np.max(np.abs(np.diff(theta) - h)) <= rtol * abs(h) * len(theta))


class NearestSigmaWarning(UserWarning):
    """lam_max >= sigma0: utils.py:1597 (ARPACK shift-invert about sigma0) would have returned the eigenpair nearest sigma0"""


def _report_sigma(r, sigma0, info):
    """the library's nearest-sigma flag (status bit 4, option "sigma0") of a one-system solve -> info dict / warning"""
    word = int(np.asarray(r["info"]).ravel()[0])
    lam = float(np.asarray(r["lam"]).ravel()[0])
    above = bool((word >> 16) & 16)
    if info is not None:
        info.update(lam=lam, above_sigma0=above, status=(word >> 16) & 3, sweeps=word & 0xffff)
    if above:
        warnings.warn("lam_max = %.6g >= sigma0 = %.6g: the reference (eigs(..., sigma=sigma0), utils.py:1597) returns the eigenpair "
                      "nearest sigma0 here, this library the largest eigenvalue's" % (lam, sigma0), NearestSigmaWarning, stacklevel=3)


def gamma_ball_full(dPdrho, theta_PEST, B, gradpar, cvdrift, gds2, vguess=None, sigma0=0.42, ctx=None, info=None, eigenpair="max"):
    """reference: utils.py:1550-1624.  Returns (gam, X, dX, g, c, f) with the same meaning.
    Uniform grids go through the fused geometry-fed kernel; a non-uniform theta_PEST is regridded exactly
    as upstream (np.interp of g, c, f onto the uniform grid, g interpolated at the uniform half points,
    utils.py:1567-1576 -- elementwise host glue) and solved by the raw (g, gh, c, f) kernel.
    eigenpair="max": the returned eigenpair is lam_max's; upstream's is the one nearest sigma0 -- the same whenever
    lam_max < sigma0.  Otherwise (module docstring) a NearestSigmaWarning is issued; info (optional dict) receives lam (the matrix
    eigenvalue), above_sigma0, status, sweeps.
    eigenpair="nearest": the eigenpair nearest sigma0, as upstream, from the host-side (g, c, f) (regridded as above on a non-uniform
    grid) by ibs_solve_gcf_nearest_f64; info receives lam, idx (eigenvalues above lam: 0 = lam_max), status (bit 5: the two
    eigenvalues about sigma0 are equally near, the larger is returned), sweeps (multisection passes)."""
    if eigenpair == "nearest":
        return _gamma_ball_nearest(ctx or default_context(), dPdrho, theta_PEST, B, gradpar, cvdrift, gds2, sigma0, info)
    if eigenpair != "max":
        raise ValueError("eigenpair must be 'max' or 'nearest', not %r" % (eigenpair,))
    ctx = ctx or default_context()
    ctx.set_option("sigma0", float(sigma0))
    try:
        return _gamma_ball_full(ctx, dPdrho, theta_PEST, B, gradpar, cvdrift, gds2, sigma0, info)
    finally:
        ctx.set_option("sigma0", None)


def _gamma_ball_full(ctx, dPdrho, theta_PEST, B, gradpar, cvdrift, gds2, sigma0, info):
    theta = np.asarray(theta_PEST, dtype=np.float64)
    B = np.asarray(B, dtype=np.float64)
    gradpar = np.asarray(gradpar, dtype=np.float64)
    cvdrift = np.asarray(cvdrift, dtype=np.float64)
    gds2 = np.asarray(gds2, dtype=np.float64)
    N = len(B)
    gp = np.abs(gradpar)
    g = gp * gds2 / B                         # utils.py:1560
    c = -1 * dPdrho * cvdrift * 1 / (gp * B)  # utils.py:1561
    f = gds2 / B ** 2 * 1 / (gp * B)          # utils.py:1562
    if is_uniform(theta):
        h = uniform_spacing(theta)
        z = np.zeros((1, N))
        r = ctx.gamma_scan(h, B[None], gradpar[None], cvdrift[None], z, gds2[None], z, z,
                           np.array([float(dPdrho)]), np.zeros(1), want_X=True, want_info=True)
        _report_sigma(r, sigma0, info)
        return float(r["gam"][0, 0]), r["X"][0, 0], r["dX"][0, 0], g, c, f
    tu = np.linspace(theta[0], theta[-1], N)                       # utils.py:1565
    g_u, c_u, f_u = np.interp(tu, theta, g), np.interp(tu, theta, c), np.interp(tu, theta, f)   # utils.py:1567-1571
    th_half = (tu[:-1] + tu[1:]) / 2                                # utils.py:1574
    h = np.diff(th_half)[2]                                         # utils.py:1575
    gh = np.zeros(N)
    gh[:-1] = np.interp(th_half, theta, g)                          # utils.py:1576
    r = ctx.solve_gcf(h, g_u[None], c_u[None], f_u[None], want_X=True, gh=gh[None], want_info=True)
    _report_sigma(r, sigma0, info)
    return float(r["gam"][0]), r["X"][0], r["dX"][0], g_u, c_u, f_u


def _gamma_ball_nearest(ctx, dPdrho, theta_PEST, B, gradpar, cvdrift, gds2, sigma0, info):
    theta = np.asarray(theta_PEST, dtype=np.float64)
    B = np.asarray(B, dtype=np.float64)
    gradpar = np.asarray(gradpar, dtype=np.float64)
    cvdrift = np.asarray(cvdrift, dtype=np.float64)
    gds2 = np.asarray(gds2, dtype=np.float64)
    N = len(B)
    gp = np.abs(gradpar)
    g = gp * gds2 / B                         # utils.py:1560
    c = -1 * dPdrho * cvdrift * 1 / (gp * B)  # utils.py:1561
    f = gds2 / B ** 2 * 1 / (gp * B)          # utils.py:1562
    if is_uniform(theta):
        h, gh = uniform_spacing(theta), None
    else:
        tu = np.linspace(theta[0], theta[-1], N)                       # utils.py:1565
        g, c, f = np.interp(tu, theta, g), np.interp(tu, theta, c), np.interp(tu, theta, f)      # utils.py:1567-1571
        th_half = (tu[:-1] + tu[1:]) / 2                                # utils.py:1574
        h = np.diff(th_half)[2]                                         # utils.py:1575
        gh = np.zeros((1, N))
        gh[0, :-1] = np.interp(th_half, theta, gp * gds2 / B)           # utils.py:1576
    r = ctx.solve_gcf_nearest(h, g[None], c[None], f[None], float(sigma0), gh=gh, want_X=True, want_info=True)
    if info is not None:
        word = int(r["info"][0])
        info.update(lam=float(r["lam"][0]), idx=int(r["idx"][0]), status=word >> 16, sweeps=word & 0xffff)
    return float(r["gam"][0]), r["X"][0], r["dX"][0], g, c, f


def gamma_ball_full_many(dPdrho, theta_PEST, B, gradpar, cvdrift, gds2, ctx=None, eigenpair="max", sigma0=0.42):
    """gamma_ball_full for n lines in one call, on ANY increasing grids: dPdrho (n,), theta_PEST (N,) shared or (n, N), the four arrays
    (n, N).  Returns (gam (n,), X, dX, g, c, f), each array (n, N), with the meaning of utils.py:1624: every line is regridded as
    upstream does (utils.py:1565-1576) and solved on the device (Context.gamma_points_theta with zero theta0 planes); a uniform grid
    goes the same way and agrees with gamma_ball_full to rounding.  All lines share the window theta_PEST[..., 0], theta_PEST[..., -1].
    eigenpair="max": lam_max's eigenpair; "nearest": the one nearest sigma0, as upstream (utils.py:1597).  A line whose grid is not
    increasing on the window comes back NaN.  numpy arrays or torch CUDA tensors."""
    if eigenpair not in ("max", "nearest"):
        raise ValueError("eigenpair must be 'max' or 'nearest', not %r" % (eigenpair,))
    ctx = ctx or default_context()
    if len(B.shape) != 2:
        raise IbsError("gamma_ball_full_many: B, gradpar, cvdrift and gds2 must be (n, N), not %s" % (tuple(B.shape),))
    if type(B).__module__.startswith("torch"):
        import torch
        z, zn = torch.zeros_like(B), torch.zeros(B.shape[0], dtype=B.dtype, device=B.device)
        dPdrho = torch.as_tensor(dPdrho, dtype=B.dtype, device=B.device)
    else:
        B, gradpar, cvdrift, gds2 = (np.asarray(a, dtype=np.float64) for a in (B, gradpar, cvdrift, gds2))
        theta_PEST = np.asarray(theta_PEST, dtype=np.float64)
        z, zn = np.zeros_like(B), np.zeros(B.shape[0])
        dPdrho = np.asarray(dPdrho, dtype=np.float64)
    geo = (theta_PEST, B, gradpar, cvdrift, z, gds2, z, z, dPdrho, zn)
    rows = ctx.assemble_gcf_theta(*geo, points=True)
    kw = dict(sigma=float(sigma0)) if eigenpair == "nearest" else {}
    r = ctx.gamma_points_theta(*geo, want_X=True, eigenpair=eigenpair, **kw)
    return r["gam"], r["X"], r["dX"], rows["g"], rows["c"], rows["f"]


def marginal_dPdrho(dPdrho, theta_PEST, B, gradpar, cvdrift, gds2, ctx=None):
    """The pressure gradient at which the line of gamma_ball_full's arguments is marginally stable, at FIXED geometry arrays:
    returns (dPdrho_crit, s*, X) with dPdrho_crit = s* dPdrho, s* the critical scale of Context.marginal_gcf (s* < 1: the line is
    unstable at dPdrho; s* = inf: no scale makes it unstable) and X the marginal mode.  Nothing upstream corresponds: c is linear in
    dPdrho (utils.py:1561) and the quantity generalises the scan of bishop_ball_s-alpha.py:90-115.  A real equilibrium's geometry
    moves with its pressure, so s* = 1 marks the true boundary and s* != 1 is a local, frozen-geometry margin.  Uniform grids only
    (the half-grid g is the mean of neighbours): a non-uniform theta_PEST raises ValueError."""
    theta = np.asarray(theta_PEST, dtype=np.float64)
    if not is_uniform(theta):
        raise ValueError("marginal_dPdrho needs a uniform theta_PEST grid")
    B = np.asarray(B, dtype=np.float64)
    gp = np.abs(np.asarray(gradpar, dtype=np.float64))
    g = gp * np.asarray(gds2, dtype=np.float64) / B                                   # utils.py:1560
    c = -1 * dPdrho * np.asarray(cvdrift, dtype=np.float64) * 1 / (gp * B)            # utils.py:1561
    r = (ctx or default_context()).marginal_gcf(uniform_spacing(theta), g[None], c[None], want_X=True)
    if r["nbad"]:
        raise IbsError("marginal_dPdrho: the solve was flagged (invalid data or the multisection did not close)")
    s = float(r["scale"][0])
    return s * float(dPdrho), s, r["X"][0]


def dPdrho_of(cvdrift, gbdrift, bmag):
    """ball_scan.py:262 / utils.py:1657"""
    return -1.0 * 0.5 * np.mean((cvdrift - gbdrift) * bmag ** 2)


def local_eq_fold(theta, line8, dPdrho, centre, sigma, theta0, eps, p, ps=None):
    """The rule of the local-equilibrium scan (csrc/ibs_local_eq.hpp, Context.local_eq_scan) in numpy: the line line8 = (bmag, gradpar,
    cvdrift, cvdrift0, gds2, gds21, gds22, gbdrift) on the grid theta under a relative change eps of its surface's global shear and a
    factor p on its pressure gradient, folded at theta0 (the ballooning angle of the varied equilibrium):
        x     = theta0 (1 + eps) + sigma eps (theta - centre) + (p - 1) ps
        cv'   = gbdrift + p (cvdrift - gbdrift) + x cvdrift0
        gd'   = gds2 + 2 x gds21 + x^2 gds22
        dP'   = p dPdrho
    centre: the centre of the line's secular term (alpha for lines of Context.fieldline_geometry); sigma = sign(-phiedge) = +-1; ps:
    the change of the integrated local shear per unit of (p - 1), in units of the fold variable (None: 0, frozen local shear; the
    s-alpha model's row is -alpha0 (sin theta - sin theta0) / shat0).  eps = 0, p = 1, ps = None is the theta0 fold of
    ball_scan.py:267-268.  Returns (dP', cv', gd'), ready for gamma_ball_full(dP', theta, bmag, gradpar, cv', gd')."""
    theta = np.asarray(theta, dtype=np.float64)
    cv, cv0, gds2, gds21, gds22, gb = (np.asarray(line8[k], dtype=np.float64) for k in (2, 3, 4, 5, 6, 7))
    x = theta0 * (1.0 + eps) + sigma * eps * (theta - centre)
    if ps is not None:
        x = x + (p - 1.0) * np.asarray(ps, dtype=np.float64)
    return p * dPdrho, gb + p * (cv - gb) + x * cv0, gds2 + 2 * x * gds21 + x * x * gds22


def _local_eq_x(theta, centre, sigma, theta0, eps, p, ps):
    """the fold variable x of local_eq_fold and its tangents (4, N) in (theta0, eps, p, dPdrho)"""
    dth = theta - centre
    psr = np.zeros_like(theta) if ps is None else np.asarray(ps, dtype=np.float64)
    x = theta0 * (1.0 + eps) + sigma * eps * dth + (p - 1.0) * psr
    return x, np.stack([np.full_like(theta, 1.0 + eps), theta0 + sigma * dth, psr, np.zeros_like(theta)])


def local_eq_fold_tangent(theta, line8, dPdrho, centre, sigma, theta0, eps, p, ps=None):
    """The tangents of local_eq_fold's three results in s = (theta0, eps, p, dPdrho), in that order: returns (dP'_s (4,), cv'_s (4, N),
    gd'_s (4, N)).  With x_s = (1 + eps, theta0 + sigma (theta - centre), ps, 0):
        dP'_s = (0, 0, dPdrho, p),   cv'_s = cvdrift0 x_s + (0, 0, cvdrift - gbdrift, 0),   gd'_s = (2 gds21 + 2 x gds22) x_s.
    The results are polynomials of degree <= 2 in every s, so central differences of local_eq_fold reproduce these to rounding."""
    theta = np.asarray(theta, dtype=np.float64)
    cv, cv0, gds21, gds22, gb = (np.asarray(line8[k], dtype=np.float64) for k in (2, 3, 5, 6, 7))
    x, xs = _local_eq_x(theta, centre, sigma, theta0, eps, p, ps)
    dcv = cv0[None] * xs
    dcv[2] += cv - gb
    return np.array([0.0, 0.0, dPdrho, p]), dcv, (2 * gds21 + 2 * x * gds22)[None] * xs


def local_eq_lam_grad(theta, line8, dPdrho, centre, sigma, triple, X, lam, ps=None):
    """The derivatives of lam_max at the point triple = (theta0, eps, p) of a line under the local-equilibrium rule, from an eigenpair
    (lam, X) of the point's pencil, X (N,) with zero ends (csrc/ibs_local_eq_grad.hpp, Context.local_eq_grad): with g = |gradpar| gd' /
    bmag, c = -dP' cv' / (|gradpar| bmag), f = gd' / (bmag^3 |gradpar|), w_j = (X_j - X_{j-1})^2 + (X_{j+1} - X_j)^2 and q = sum f X^2,
        d lam / d s = (sum c_s X^2 - 1/2 h^-2 sum g_s w - lam sum f_s X^2) / q
    for s = theta0, eps, p, dPdrho (the tangents of local_eq_fold_tangent) and for every entry of the eight arrays (closed forms per
    grid point).  Exact for this lam to first order in the error of X; lam must be a simple eigenvalue.
    Returns dict(dlam (4,), geo_bar (8, N), q, dlam_scale (4,), geo_bar_scale (8, N)): a scale is the sum of the absolute values of
    the three terms of its component, over q -- what a deviation of the component is measured against."""
    theta = np.asarray(theta, dtype=np.float64)
    X = np.asarray(X, dtype=np.float64)
    theta0, eps, p = (float(v) for v in triple)
    B, gpr = (np.asarray(line8[k], dtype=np.float64) for k in (0, 1))
    a = np.abs(gpr)
    dPv, cvv, gd = local_eq_fold(theta, line8, dPdrho, centre, sigma, theta0, eps, p, ps=ps)
    ddP, dcv, dgd = local_eq_fold_tangent(theta, line8, dPdrho, centre, sigma, theta0, eps, p, ps=ps)
    x, _ = _local_eq_x(theta, centre, sigma, theta0, eps, p, ps)
    g, c, f = a * gd / B, -dPv * cvv / (a * B), gd / (B ** 3 * a)
    d2 = np.diff(X) ** 2
    w = np.concatenate([[0.0], d2]) + np.concatenate([d2, [0.0]])
    X2 = X * X
    k2 = 0.5 / float(theta[1] - theta[0]) ** 2
    q = float(np.sum(f * X2))
    terms = np.stack([np.sum(-(ddP[:, None] * cvv[None] + dPv * dcv) / (a * B) * X2, axis=1),
                      -k2 * np.sum(a * dgd / B * w, axis=1),
                      -lam * np.sum(dgd / (B ** 3 * a) * X2, axis=1)])                       # (3, 4)
    gbar, cbar, fbar = -k2 * w / q, X2 / q, -lam * X2 / q
    z = np.zeros_like(theta)
    sgn = np.where(gpr < 0, -1.0, 1.0)
    cvb = -dPv * cbar / (a * B)
    gdg, gdf = gbar * a / B, fbar / (B ** 3 * a)
    planes = np.array([[-gbar * g / B, -cbar * c / B, -3 * fbar * f / B],
                       [sgn * gbar * g / a, -sgn * cbar * c / a, -sgn * fbar * f / a],
                       [z, p * cvb, z], [z, x * cvb, z],
                       [gdg, z, gdf], [2 * x * gdg, z, 2 * x * gdf], [x * x * gdg, z, x * x * gdf],
                       [z, (1.0 - p) * cvb, z]])                                             # (8, 3, N)
    return dict(dlam=terms.sum(axis=0) / q, geo_bar=planes.sum(axis=1), q=q, dlam_scale=np.abs(terms).sum(axis=0) / abs(q),
                geo_bar_scale=np.abs(planes).sum(axis=1))


def local_eq_ray_triples(rays, t):
    """The rule for a ray of the local-equilibrium boundaries (csrc/ibs_local_eq_boundary.hpp, Context.local_eq_boundary) in numpy:
    rays (..., 7) = (theta0, eps0, p0, d_eps, d_p, t_lo, t_hi) and parameters t, broadcast against the rays' leading shape, give the
    triples (..., 3) = (theta0, eps0 + t d_eps, p0 + t d_p) that local_eq_fold takes.  theta0 does not vary along a ray.  The
    pressure axis at fixed shear is d_eps = 0, d_p = 1, the shear axis d_eps = 1, d_p = 0."""
    rays = np.asarray(rays, dtype=np.float64)
    t = np.asarray(t, dtype=np.float64)
    th0, eps, p = np.broadcast_arrays(rays[..., 0], rays[..., 1] + t * rays[..., 3], rays[..., 2] + t * rays[..., 4])
    return np.stack([th0, eps, p], axis=-1)


def local_eq_ray_nodes(rays):
    """the 64 pass-0 nodes (..., 64) of rays (..., 7): t_lo + k (t_hi - t_lo) / 63, node 63 being t_hi itself (the kernel forms node k
    with one fused multiply-add: the two may differ in the last bit)"""
    rays = np.asarray(rays, dtype=np.float64)
    lo, hi = rays[..., 5:6], rays[..., 6:7]
    t = lo + np.arange(64.0) * ((hi - lo) / 63.0)
    t[..., 63] = hi[..., 0]
    return t


def make_obj_w_grad(fieldlines, ctx=None, del_alpha=0.004, eigenpair="max", jac="reference"):
    """Factory for a drop-in `obj_w_grad(x0, vs, rho_val, theta, vguess00, sigma00=0.42)` (utils.py:1632).

    `fieldlines(vs, rho_val, alphas, theta)` supplies the geometry exactly as the reference gets it from
    `vmec_fieldlines(vs, rho_val, alphas, theta1d=theta)` (utils.py:1641-1646) and must return an array
    (3, 8, N) in scan.GEO_ORDER.  With the reference available:
        fl = lambda vs, s, al, th: np.stack([[getattr(utils.vmec_fieldlines(vs, s, al, theta1d=th), k)[0][i]
                                             for k in GEO_ORDER] for i in range(3)])
    Returns (-gam, array([-dgam/dalpha, -dgam/dtheta0])) like utils.py:1728 (scipy jac=True convention).
    eigenpair="max": lam_max's eigenpair, one fused ibs_obj_w_grad_f64 call (sigma00 unused).  eigenpair="nearest": the eigenpair
    nearest sigma00, as upstream on every input: the centre line is solved by ibs_solve_gcf_nearest_f64, the alpha tangents (right
    minus left line, each with its own dPdrho, over del_alpha: utils.py:1683-1718) and theta0 tangents (utils.py:1669-1673) are built
    on the host and both derivatives taken by ibs_hf_grad_f64 (utils.py:1676-1680, 1721-1725).
    jac="reference" (the default): the Hellmann-Feynman formulas above, as upstream -- they put gam in place of lam and are not the
    derivative of the gam returned (0.1-5 % off on field-line data).  jac="exact": the same val; jac is the exact derivative of that
    gam (ibs_solve_gcf_vjp_f64) along the rows' tangents -- in theta0 the exact one (utils.py:1669-1673), in alpha (right minus left
    line, each with its own dPdrho, over del_alpha: utils.py:1683-1718), which is the only approximation left.  Either eigenpair."""
    if jac == "exact":
        if eigenpair not in ("max", "nearest"):
            raise ValueError("eigenpair must be 'max' or 'nearest', not %r" % (eigenpair,))
        return _make_obj_w_grad_exact(fieldlines, ctx, del_alpha, eigenpair)
    if jac != "reference":
        raise ValueError("jac must be 'reference' or 'exact', not %r" % (jac,))
    if eigenpair == "nearest":
        return _make_obj_w_grad_nearest(fieldlines, ctx, del_alpha)
    if eigenpair != "max":
        raise ValueError("eigenpair must be 'max' or 'nearest', not %r" % (eigenpair,))

    def obj_w_grad(x0, vs, rho_val, theta, vguess00=None, sigma00=0.42):
        c = ctx or default_context()
        alpha_val, theta0_val = float(x0[0]), float(x0[1])
        al = np.array([alpha_val - 0.5 * del_alpha, alpha_val, alpha_val + 0.5 * del_alpha])
        geo = np.asarray(fieldlines(vs, rho_val, al, theta), dtype=np.float64)
        val, jac = c.obj_w_grad(uniform_spacing(theta), geo[None], np.array([theta0_val]), del_alpha)
        return float(val[0]), np.asarray(jac[0], dtype=np.float64)
    return obj_w_grad


def _line_gcf(line, theta0):
    """(dPdrho, g, c, f) of one field line (8, N) at theta0"""
    bmag, gradpar, cvdrift, cvdrift0, gds2, gds21, gds22, gbdrift = line
    dP = dPdrho_of(cvdrift, gbdrift, bmag)                        # utils.py:1657 (each line its own)
    cv = cvdrift + theta0 * cvdrift0                               # utils.py:1659
    gd = gds2 + 2 * theta0 * gds21 + theta0 ** 2 * gds22           # utils.py:1660
    gp = np.abs(gradpar)
    return dP, gp * gd / bmag, -1 * dP * cv * 1 / (gp * bmag), gd / bmag ** 2 * 1 / (gp * bmag)   # utils.py:1560-1562


def _theta0_tangent(line, theta0, dP):
    """d(g, c, f)/dtheta0 of one field line (8, N) at theta0 (utils.py:1669-1673)"""
    bmag, gradpar, _, cvdrift0, _, gds21, gds22, _ = line
    gp = np.abs(gradpar)
    dgd = 2 * gds21 + 2 * theta0 * gds22
    return gp * dgd / bmag, -1 * dP * cvdrift0 * 1 / (gp * bmag), dgd / bmag ** 2 * 1 / (gp * bmag)


def _make_obj_w_grad_exact(fieldlines, ctx, del_alpha, eigenpair):
    def obj_w_grad(x0, vs, rho_val, theta, vguess00=None, sigma00=0.42):
        c = ctx or default_context()
        alpha_val, theta0_val = float(x0[0]), float(x0[1])
        al = np.array([alpha_val - 0.5 * del_alpha, alpha_val, alpha_val + 0.5 * del_alpha])
        geo = np.asarray(fieldlines(vs, rho_val, al, theta), dtype=np.float64)
        h = uniform_spacing(theta)
        dP, g, cc, f = _line_gcf(geo[1], theta0_val)
        if eigenpair == "nearest":
            r = c.solve_gcf_nearest(h, g[None], cc[None], f[None], float(sigma00), want_X=True)
        else:
            r = c.solve_gcf(h, g[None], cc[None], f[None], want_X=True)
        gam = float(r["gam"][0])
        v = c.solve_gcf_vjp(h, g[None], cc[None], f[None], r["lam"], r["X"], gam_bar=1.0, want_info=True)
        if v["nbad"]:
            st = int(v["info"][0]) >> 16
            warnings.warn(vjp_status_message(st & 1, (st >> 1) & 1), VjpStatusWarning, stacklevel=2)
        gb, cb, fb = v["g_bar"][0], v["c_bar"][0], v["f_bar"][0]
        g_t, c_t, f_t = _theta0_tangent(geo[1], theta0_val, dP)
        jac_t = gb @ g_t + cb @ c_t + fb @ f_t
        _, g_r, c_r, f_r = _line_gcf(geo[2], theta0_val)
        _, g_l, c_l, f_l = _line_gcf(geo[0], theta0_val)
        jac_a = (gb @ (g_r - g_l) + cb @ (c_r - c_l) + fb @ (f_r - f_l)) / del_alpha
        return -1 * gam, np.array([-1 * float(jac_a), -1 * float(jac_t)])
    return obj_w_grad


def _make_obj_w_grad_nearest(fieldlines, ctx, del_alpha):
    gcf_of = _line_gcf

    def obj_w_grad(x0, vs, rho_val, theta, vguess00=None, sigma00=0.42):
        c = ctx or default_context()
        alpha_val, theta0_val = float(x0[0]), float(x0[1])
        al = np.array([alpha_val - 0.5 * del_alpha, alpha_val, alpha_val + 0.5 * del_alpha])
        geo = np.asarray(fieldlines(vs, rho_val, al, theta), dtype=np.float64)
        h = uniform_spacing(theta)
        dP, g, cc, f = gcf_of(geo[1], theta0_val)
        r = c.solve_gcf_nearest(h, g[None], cc[None], f[None], float(sigma00), want_X=True)
        gam = float(r["gam"][0])
        g_t, c_t, f_t = _theta0_tangent(geo[1], theta0_val, dP)        # utils.py:1669-1673
        _, g_r, c_r, f_r = gcf_of(geo[2], theta0_val)                  # utils.py:1683-1693, 1707-1709
        _, g_l, c_l, f_l = gcf_of(geo[0], theta0_val)                  # utils.py:1695-1705, 1711-1713
        g_a, c_a, f_a = (g_r - g_l) / del_alpha, (c_r - c_l) / del_alpha, (f_r - f_l) / del_alpha    # utils.py:1716-1718
        two = lambda a: np.ascontiguousarray(np.broadcast_to(a, (2, len(a))))
        jac = c.hf_grad(two(r["X"][0]), two(r["dX"][0]), two(f), np.stack([g_a, g_t]), np.stack([c_a, c_t]),
                        np.stack([f_a, f_t]), np.array([gam, gam]))
        return -1 * gam, np.array([-1 * float(jac[0]), -1 * float(jac[1])])                         # utils.py:1728
    return obj_w_grad


def theta_grid(N, theta_fac=4):
    """the theta_PEST grid of ball_scan.py:201-209: N points on [-theta_fac pi, theta_fac pi]"""
    return np.linspace(-theta_fac * np.pi, theta_fac * np.pi, int(N))
