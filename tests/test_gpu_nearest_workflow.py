"""GPU: the scan workflow in nearest-sigma mode -- the batched objective + gradient (ibs_obj_w_grad_nearest_f64), the batched final
solve (ibs_gamma_points_nearest_f64), BallooningScan(eigenpair="nearest") on the resident and host-callable paths and
AdjointStep(eigenpair="nearest"), against the host-composed drop-in, the raw-system entry point and a CPU restatement built from
the oracle's public pieces (tests/nearest_oracle.py)."""
import os

import numpy as np
import pytest

from oracle import ballooning_oracle as bo
from tests.nearest_oracle import EPS, dense_nearest, gcf_at, obj_w_grad_nearest_lines

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
DEL = 0.004


@pytest.fixture(scope="module")
def ctx():
    import ibs_amd
    c = ibs_amd.Context(0)
    yield c
    c.close()


def vec_tol(r):
    return max(1e-8, 64 * EPS * r["nA"] / r["gap"])


def top_two(th, g, c, f):
    from scipy.linalg import eigh_tridiagonal
    d, e, fd = bo.assemble(th, g, c, f)[:3]
    n = len(d)
    w = eigh_tridiagonal(d / fd, e[1:n] / np.sqrt(fd[:-1] * fd[1:]), eigvals_only=True, select="i", select_range=(n - 2, n - 1))
    return w[1], w[0]


def gap_at(th, g, c, f, idx):
    """(||A||, distance to the nearest other eigenvalue) of the eigenvalue with idx eigenvalues above it"""
    from scipy.linalg import eigh_tridiagonal
    d, e, fd = bo.assemble(th, g, c, f)[:3]
    n = len(d)
    j = n - 1 - idx
    lo, hi = max(0, j - 1), min(n - 1, j + 1)
    w = eigh_tridiagonal(d / fd, e[1:n] / np.sqrt(fd[:-1] * fd[1:]), eigvals_only=True, select="i", select_range=(lo, hi))
    lj = w[j - lo]
    gap = min([abs(x - lj) for i, x in enumerate(w) if i != j - lo] or [np.inf])
    return float(((np.abs(d) + e[:-1] + e[1:]) / fd).max()), gap


def point_batch(N, n_pts, seed):
    """n_pts points of driven synthetic field lines (dPdrho = -K, K in {1, 4, 8}): geo (n_pts, 3, 8, N), theta0, sigma cycling
    through above lam_max / 0.42 / 1.0 / midway between the two largest eigenvalues (undecided: bit 5)"""
    from tests.helpers import synthetic_fieldlines
    th = bo.theta_grid(N)
    base = synthetic_fieldlines(th)
    rng = np.random.default_rng(seed)
    geo = np.empty((n_pts, 3, 8, N))
    t0 = rng.uniform(0.0, 0.5 * np.pi, n_pts)
    sig = np.empty(n_pts)
    for k in range(n_pts):
        s, a, K = rng.uniform(0.3, 0.9), rng.uniform(0.0, np.pi), (1.0, 4.0, 8.0)[k % 3]
        ln = base(s, np.array([a - 0.5 * DEL, a, a + 0.5 * DEL]))
        ln[:, 7] = ln[:, 2] - 2.0 * K / ln[:, 0] ** 2
        geo[k] = ln
        m = k % 4
        if m == 0:
            sig[k] = 1e3
        elif m == 1:
            sig[k] = 0.42
        elif m == 2:
            sig[k] = 1.0
        else:
            g, c, f = gcf_at(bo.dPdrho_of(ln[1, 2], ln[1, 7], ln[1, 0]), *ln[1, :7], t0[k])
            l1, l2 = top_two(th, g, c, f)
            sig[k] = 0.5 * (l1 + l2)
    return th, geo, t0, sig


def close(a, b, tol):
    return np.abs(a - b) <= tol * np.maximum(1.0, np.abs(b))


@pytest.mark.parametrize("N,n_pts", [(513, 96), (969, 640), (2561, 608)])
def test_obj_w_grad_nearest_batched(ctx, N, n_pts):
    """ibs_obj_w_grad_nearest_f64 on a batch of mixed shifts (>= 600 points at 969 and 2561: more than 512, the workspace carve-out
    of the persistent grid) against make_obj_w_grad(eigenpair="nearest") point by point (val 1e-10, jac 1e-9) and a sample against
    the dense restatement (val 1e-8, jac 1e-7); with every shift above lam_max it is ibs_obj_w_grad_f64 (1e-9); host and device
    pointers agree bit for bit; the midway shifts carry bit 5"""
    import torch
    import ibs_amd
    th, geo, t0, sig = point_batch(N, n_pts, 20261 + N)
    h = th[1] - th[0]
    val, jac, inf = ctx.obj_w_grad_nearest(h, geo, t0, sig, DEL, want_info=True)
    st = inf["info"] >> 16
    assert int(((st & 3) != 0).sum()) == 0 and np.isfinite(val).all() and np.isfinite(jac).all()
    assert all(st[k] & 32 for k in range(3, n_pts, 4)), st[3::4]
    assert (inf["idx"][1::4] > 0).any()                          # (shifts inside the spectrum: not lam_max's eigenpair)
    inf_nA, inf_gap = np.empty(n_pts), np.empty(n_pts)
    for k in range(n_pts):
        ln = geo[k, 1]
        inf_nA[k], inf_gap[k] = gap_at(th, *gcf_at(bo.dPdrho_of(ln[2], ln[7], ln[0]), *ln[:7], t0[k]), int(inf["idx"][k]))
    for k in range(n_pts):
        near = ibs_amd.make_obj_w_grad(lambda vs, rho, al, theta, k=k: geo[k], ctx=ctx, eigenpair="nearest", del_alpha=DEL)
        v, j = near(np.array([0.0, t0[k]]), None, 0.5, th, None, sig[k])
        assert close(val[k], v, 1e-10), (k, val[k], v)
        # (the two solves see rows a few ulp apart: the gradient moves with the eigenvector, by up to ~eps ||A|| / gap)
        tj = max(1e-9, 64 * EPS * float(inf_nA[k]) / float(inf_gap[k]))
        assert close(jac[k], j, tj).all(), (k, jac[k], j, tj)
    for k in np.random.default_rng(N).choice(n_pts, 12, replace=False):
        rv, rj, ref = obj_w_grad_nearest_lines(th, t0[k], geo[k], sig[k], DEL)
        tv = max(1e-8, vec_tol(ref))
        assert int(inf["idx"][k]) == ref["idx"], (k, inf["idx"][k], ref["idx"])
        assert close(val[k], rv, tv), (k, val[k], rv, tv)
        assert close(jac[k], rj, max(1e-7, 10 * tv)).all(), (k, jac[k], rj, tv)
    dev = torch.device("cuda:0")
    dv, dj, dinf = ctx.obj_w_grad_nearest(h, torch.from_numpy(geo).to(dev), torch.from_numpy(t0).to(dev),
                                          torch.from_numpy(sig).to(dev), DEL, want_info=True)
    assert np.array_equal(dv.cpu().numpy(), val) and np.array_equal(dj.cpu().numpy(), jac)
    assert np.array_equal(dinf["info"].cpu().numpy(), inf["info"]) and np.array_equal(dinf["idx"].cpu().numpy(), inf["idx"])
    v0, j0 = ctx.obj_w_grad(h, geo, t0, DEL)
    v1, j1 = ctx.obj_w_grad_nearest(h, geo, t0, 1e3, DEL)
    assert close(v1, v0, 1e-9).all() and close(j1, j0, 1e-9).all(), (np.abs(v1 - v0).max(), np.abs(j1 - j0).max())


def salpha_points(N, seed, n_lines=8):
    """seven geometry arrays of s-alpha lines (B = 1, gradpar = 1) with dyadic theta0: the device's assembly and host_rows below
    round alike, so the two solves see the same rows"""
    th = bo.theta_grid(N)
    rng = np.random.default_rng(seed)
    geo, dP, t0 = [], [], []
    for i in range(n_lines):
        shat, alpha = rng.uniform(0.4, 1.6), rng.uniform(0.5, 1.2)
        lam0 = shat * th - alpha * np.sin(th)
        geo.append(np.stack([np.ones(N), np.ones(N), alpha * (np.cos(th) + np.sin(th) * lam0), -alpha * shat * np.sin(th),
                             1 + lam0 ** 2, -shat * lam0, np.full(N, shat ** 2)]))
        dP.append((-1.0, -4.0, -8.0)[i % 3]); t0.append((0.0, 0.25, 0.5, 1.0)[i % 4])
    return th, np.stack(geo), np.array(dP), np.array(t0)


def host_rows(geo7, dP, t0):
    bmag, gradpar, cvdrift, cvdrift0, gds2, gds21, gds22 = geo7
    gp = np.abs(gradpar)
    inv = 1.0 / (gp * bmag)
    d = gds2 + (2.0 * t0) * gds21 + (t0 * t0) * gds22
    return gp / bmag * d, -dP * cvdrift * inv + t0 * (-dP * cvdrift0 * inv), inv / (bmag * bmag) * d


@pytest.mark.parametrize("N", [513, 2561])
def test_gamma_points_nearest_against_raw_systems(ctx, N):
    """ibs_gamma_points_nearest_f64 against ibs_solve_gcf_nearest_f64 on the host-assembled rows of the same lines, four shifts per
    line (below the spectrum, 0.42, 1.0, midway between the top two): gam and lam to 1e-12 relative, idx and status bits equal, X
    within vec_tol"""
    th, geo, dP, t0 = salpha_points(N, 77 + N)
    h = th[1] - th[0]
    rows, pts, sig = [], [], []
    for i in range(len(geo)):
        g, c, f = host_rows(geo[i], dP[i], t0[i])
        l1, l2 = top_two(th, g, c, f)
        for s in (-1e3, 0.42, 1.0, 0.5 * (l1 + l2)):
            rows.append((g, c, f)); pts.append(i); sig.append(s)
    pts, sig = np.array(pts), np.array(sig)
    arrs = [np.ascontiguousarray(geo[pts, k]) for k in range(7)]
    r = ctx.gamma_points_nearest(h, *arrs, dP[pts], t0[pts], sig, want_X=True, want_info=True)
    gg, cc, ff = (np.stack([x[k] for x in rows]) for k in range(3))
    q = ctx.solve_gcf_nearest(h, gg, cc, ff, sig, want_X=True, want_info=True)
    assert r["nbad"] == 0 and q["nbad"] == 0
    assert np.array_equal(r["idx"], q["idx"]) and np.array_equal(r["info"] >> 16, q["info"] >> 16)
    assert close(r["gam"], q["gam"], 1e-12).all() and close(r["lam"], q["lam"], 1e-12).all()
    assert all(r["info"][k] >> 16 & 32 for k in range(3, len(sig), 4))
    for k in range(len(sig)):
        ref = dense_nearest(th, *rows[k], sig[k])
        d = min(np.abs(r["X"][k] - q["X"][k]).max(), np.abs(r["X"][k] + q["X"][k]).max())
        assert d <= vec_tol(ref), (k, d, vec_tol(ref))


def wout_scaled(factor):
    w = dict(np.load(os.path.join(G, "G8_wout_ncsx_op.npz")))
    w["pres"] = np.asarray(w["pres"], dtype=np.float64) * factor
    return w


PRES_SCALE = 50.0
SVALS = np.array([0.6, 0.9])


@pytest.mark.parametrize("N", [969, 2561])
def test_resident_scan_nearest_on_ncsx_tables(ctx, N):
    """BallooningScan(eigenpair="nearest") on the device (G8 NCSX tables): with the pressure scaled up until coarse lines have
    lam_max > 1.0, the resident rows equal the host-callable nearest path on the same device geometry (gam 1e-8), every final gam is
    the dense nearest eigenpair of its final line at 0.42, and some surface differs from "max" mode; unscaled, the shifts lie above
    lam_max and the two modes agree (gam to 1e-8)"""
    import torch
    import ibs_amd
    dev = torch.device("cuda:0")
    th = np.linspace(-4 * np.pi, 4 * np.pi, N)
    h = th[1] - th[0]
    kw = dict(nalpha=8, ntheta0=5)
    # scaled pressure
    tabs = ibs_amd.SurfaceTables.from_wout(wout_scaled(PRES_SCALE), SVALS)
    res = ibs_amd.BallooningScan(ctx, None, th, SVALS, tables=tabs, device=dev, eigenpair="nearest", **kw)
    t_r, a_r, g_r = res.run()
    host = ibs_amd.BallooningScan(ctx, None, th, SVALS, tables=tabs, eigenpair="nearest", **kw)
    lam_max = []
    for s in SVALS:
        geo = host.fieldlines(s, host.alpha_scan)
        dP = -0.5 * np.mean((geo[:, 2] - geo[:, 7]) * geo[:, 0] ** 2, axis=1)
        lam_max.append(ctx.gamma_scan(h, *[np.ascontiguousarray(geo[:, k]) for k in range(7)], dP, host.theta0_scan)["lam"])
    assert (np.array(lam_max) > 1.0).any(), np.max(lam_max)
    t_h, a_h, g_h = host.run()
    assert np.abs(g_r - g_h).max() < 1e-8, (g_r, g_h)
    assert np.abs(a_r - a_h).max() < 1e-4 and np.abs(t_r - t_h).max() < 1e-4, (a_r, a_h, t_r, t_h)
    for k, s in enumerate(SVALS):
        ln = host.fieldlines(s, np.array([a_r[k]]))[0]
        dP = bo.dPdrho_of(ln[2], ln[7], ln[0])
        ref = dense_nearest(th, *gcf_at(dP, *ln[:7], t_r[k]), 0.42)
        assert abs(g_r[k] - ref["gam"]) <= max(1e-8, vec_tol(ref)), (k, g_r[k], ref["gam"])
    mx = ibs_amd.BallooningScan(ctx, None, th, SVALS, tables=tabs, device=dev, **kw).run()
    assert np.abs(mx[2] - g_r).max() > 1e-3, (mx[2], g_r)
    # unscaled
    tabs0 = ibs_amd.SurfaceTables.from_wout(wout_scaled(1.0), SVALS)
    n0 = ibs_amd.BallooningScan(ctx, None, th, SVALS, tables=tabs0, device=dev, eigenpair="nearest", **kw).run()
    m0 = ibs_amd.BallooningScan(ctx, None, th, SVALS, tables=tabs0, device=dev, **kw).run()
    # (gam to 1e-8; the two modes refine by different optimizers -- on-device ibs_refine_f64 against the host-driven state machines
    # -- whose stopping points on the flat maximum agree to the 1e-4 of the other driver tests)
    assert np.abs(n0[2] - m0[2]).max() < 1e-8, (n0, m0)
    assert np.abs(n0[0] - m0[0]).max() < 1e-4 and np.abs(n0[1] - m0[1]).max() < 1e-4, (n0, m0)


def test_adjoint_step_nearest(ctx):
    """AdjointStep(eigenpair="nearest") on three equilibria (base, scaled pressure, a perturbed boundary mode), N = 969: every
    equilibrium's rows equal a separate BallooningScan(eigenpair="nearest") run, f0 / fobj / dfobj follow from those rows;
    AdjointStep() and AdjointStep(eigenpair="max") agree bit for bit"""
    import torch
    import ibs_amd
    import bench
    dev = torch.device("cuda:0")
    wout0 = wout_scaled(1.0)
    wouts = [wout0, wout_scaled(PRES_SCALE), bench.emulated_equilibria(wout0)[0][1]]
    steps = np.array([1.0, 1e-3, 2e-3])
    f_other = np.array([0.8, 0.81, 0.82])
    th = ibs_amd.theta_grid_for(11, 11)
    assert len(th) == 969
    kw = dict(nalpha=8, ntheta0=5, gamma_thresh=-2.0e-4, prefac=50.0)
    out = ibs_amd.AdjointStep(ctx, th, SVALS, dev, eigenpair="nearest", **kw).run(wouts, f_other, steps)
    rows = []
    for w in wouts:
        tabs = ibs_amd.SurfaceTables.from_wout(w, SVALS)
        rows.append(ibs_amd.BallooningScan(ctx, None, th, SVALS, nalpha=8, ntheta0=5, tables=tabs, device=dev,
                                           eigenpair="nearest").run())
    rows = np.array(rows)                                    # (3 equilibria, theta0 / alpha / gam, surfaces)
    assert np.abs(out["gam"] - rows[:, 2]).max() < 1e-8, (out["gam"], rows[:, 2])
    assert np.abs(out["alpha"] - rows[:, 1]).max() < 1e-4 and np.abs(out["theta0"] - rows[:, 0]).max() < 1e-4
    f0 = ibs_amd.ballooning_objective(f_other, out["gam"], -2.0e-4, 50.0)
    assert np.array_equal(out["f0"], f0) and out["fobj"] == float(np.sqrt(f0[0]))
    assert np.array_equal(out["dfobj"], ibs_amd.dof_fd_gradient(f0, steps))
    mx = ibs_amd.AdjointStep(ctx, th, SVALS, dev, eigenpair="max", **kw).run(wouts, f_other, steps)
    df = ibs_amd.AdjointStep(ctx, th, SVALS, dev, **kw).run(wouts, f_other, steps)
    for key in ("gam", "theta0", "alpha", "f0", "dfobj"):
        assert np.array_equal(mx[key], df[key]), key
    assert mx["fobj"] == df["fobj"]
    assert np.abs(mx["gam"][1] - out["gam"][1]).max() > 1e-3          # (the driven equilibrium: the modes differ)


def test_errors_and_ties(ctx):
    """even N, N = 33 and N = 65,539 are refused; a NaN sigma gives status 2 on its point only; a tie at the coarse shift carries
    bit 5 and the driver does not raise on it"""
    import ibs_amd
    from scipy.optimize import brentq
    from tests.helpers import synthetic_fieldlines
    for N in (512, 33, 65539):
        z = np.ones((1, N))
        with pytest.raises(ibs_amd.IbsError):
            ctx.obj_w_grad_nearest(0.05, np.ones((1, 3, 8, N)), np.zeros(1), 0.42)
        with pytest.raises(ibs_amd.IbsError):
            ctx.gamma_points_nearest(0.05, z, z, z, z, z, z, z, np.array([-1.0]), np.zeros(1), 0.42)
    th, geo, t0, sig = point_batch(513, 8, 5)
    h = th[1] - th[0]
    clean = ctx.obj_w_grad_nearest(h, geo, t0, sig, DEL, want_info=True)
    s_bad = sig.copy(); s_bad[5] = np.nan
    r = ctx.obj_w_grad_nearest(h, geo, t0, s_bad, DEL, want_info=True)
    assert (r[2]["info"][5] >> 16) & 3 == 2 and np.isnan(r[0][5]) and np.isnan(r[1][5]).all()
    keep = np.arange(8) != 5
    assert np.array_equal(r[0][keep], clean[0][keep]) and np.array_equal(r[1][keep], clean[1][keep])
    assert np.array_equal(r[2]["info"][keep], clean[2]["info"][keep])
    _, g7, dP, tt = salpha_points(513, 3, n_lines=3)
    p = ctx.gamma_points_nearest(h, *[np.ascontiguousarray(g7[:, k]) for k in range(7)], dP, tt, np.array([0.42, np.nan, 1.0]),
                                 want_info=True)
    assert p["nbad"] == 1 and (p["info"][1] >> 16) & 3 == 2 and p["idx"][1] == -1 and (p["info"][[0, 2]] >> 16 & 3 == 0).all()
    # a line driven so that the two largest eigenvalues sit symmetrically about the coarse shift 1.0
    N = 129
    th = bo.theta_grid(N)
    base = synthetic_fieldlines(th)

    def line(K):
        ln = base(0.5, np.array([0.0]))
        ln[:, 7] = ln[:, 2] - 2.0 * K / ln[:, 0] ** 2
        return ln

    def mid(K):
        ln = line(K)[0]
        return sum(top_two(th, *gcf_at(bo.dPdrho_of(ln[2], ln[7], ln[0]), *ln[:7], 0.0))) - 2.0
    K = brentq(mid, 0.5, 64.0, xtol=1e-14, rtol=4 * EPS)
    fl = lambda s, alphas: np.repeat(line(K), len(np.atleast_1d(alphas)), axis=0)
    geo = line(K)
    dPk = -0.5 * np.mean((geo[:, 2] - geo[:, 7]) * geo[:, 0] ** 2, axis=1)
    r = ctx.gamma_scan_nearest(th[1] - th[0], *[np.ascontiguousarray(geo[:, k]) for k in range(7)], dPk, np.zeros(1), 1.0,
                               want_info=True)
    assert r["nbad"] == 0 and r["info"][0, 0] >> 16 == 32, r["info"]
    t, a, g = ibs_amd.BallooningScan(ctx, fl, th, [0.5], nalpha=1, ntheta0=1, eigenpair="nearest").run()
    assert np.isfinite(g).all()
