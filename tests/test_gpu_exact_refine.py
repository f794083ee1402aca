"""GPU: the batched objective with the exact gradient of gam (ibs_obj_w_grad_exact_f64) and the scan drivers' jac="exact" mode --
against the host-composed make_obj_w_grad(jac="exact"), a CPU restatement built from the oracle's public pieces
(tests/exact_oracle.py), ibs_obj_w_grad_f64's val, a central difference of the kernel's own val, and the drivers' jac="reference"
runs."""
import os

import numpy as np
import pytest

from oracle import ballooning_oracle as bo
from tests import edge_cases as ec
from tests.exact_oracle import obj_w_grad_exact_lines
from tests.nearest_oracle import EPS, dense_nearest, gcf_at

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
    """(a local copy of test_gpu_nearest_workflow.point_batch) n_pts points of driven synthetic field lines (dPdrho = -K, K in
    {1, 4, 8}): geo (n_pts, 3, 8, N), theta0, sigma cycling through above lam_max / 0.42 / 1.0 / midway between the two largest
    eigenvalues (undecided: bit 5)"""
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


def against_host_composed(ctx, th, geo, t0, sig, val, jac, idx, tag):
    """point by point against make_obj_w_grad(jac="exact"): val 1e-10, jac 1e-9 or the gap-aware bound of
    test_gpu_nearest_workflow.py (the two solves see rows a few ulp apart: the gradient moves with the eigenvector, by up to
    ~eps ||A|| / gap).  Returns the worst figures."""
    import ibs_amd
    mode = "max" if sig is None else "nearest"
    wv = wj = 0.0
    for k in range(len(t0)):
        ln = geo[k, 1]
        nA, gap = gap_at(th, *gcf_at(bo.dPdrho_of(ln[2], ln[7], ln[0]), *ln[:7], t0[k]), int(idx[k]))
        host = ibs_amd.make_obj_w_grad(lambda vs, rho, al, theta, k=k: geo[k], ctx=ctx, eigenpair=mode, jac="exact", del_alpha=DEL)
        v, j = host(np.array([0.0, t0[k]]), None, 0.5, th, None, 0.42 if sig is None else sig[k])
        tj = max(1e-9, 64 * EPS * nA / gap)
        wv = max(wv, float(np.abs(val[k] - v) / max(1.0, abs(v))))
        wj = max(wj, float((np.abs(jac[k] - j) / np.maximum(1.0, np.abs(j))).max()))
        assert close(val[k], v, 1e-10), (tag, k, val[k], v)
        assert close(jac[k], j, tj).all(), (tag, k, jac[k], j, tj)
    print("exact-refine figures: %s against host-composed: worst |dval| %.2e, worst |djac| %.2e (relative to max(1, |.|))" % (tag, wv, wj))
    return wv, wj


@pytest.mark.parametrize("N,n_pts", [(513, 96), (969, 640), (2561, 608)])
@pytest.mark.parametrize("mode", ["max", "mixed"])
def test_obj_w_grad_exact_batched(ctx, N, n_pts, mode):
    """ibs_obj_w_grad_exact_f64 on a batch (>= 600 points at 969 and 2561: more than 512, the workspace carve-out of the persistent
    grid), sigma = NULL or mixed shifts: point by point against make_obj_w_grad(jac="exact") (val 1e-10, jac 1e-9 or the gap-aware
    bound); a sample of 12 against tests/exact_oracle.py (val 1e-8, jac 1e-7); sigma = NULL: val equals ibs_obj_w_grad_f64's to 1e-9;
    jac_theta0 against central differences of the kernel's own val in theta0 (step 1e-4, Richardson-combined with the half and the
    quarter step, 1e-6 relative on every point without a tie); host and device pointers agree bit for bit; a point alone gives the bits it has in the batch"""
    import torch
    th, geo, t0, sig = point_batch(N, n_pts, 20261 + N)
    if mode == "max":
        sig = None
    h = th[1] - th[0]
    val, jac, inf = ctx.obj_w_grad_exact(h, geo, t0, DEL, sigma=sig, want_info=True)
    assert ctx.last_launch()[0] == "ibs::k_exact_points<%s>" % ("false" if sig is None else "true"), ctx.last_launch()
    st = inf["info"] >> 16
    assert int(((st & 3) != 0).sum()) == 0 and np.isfinite(val).all() and np.isfinite(jac).all()
    assert not (st & 128).any(), np.nonzero(st & 128)                 # (no pair refused by the adjoint)
    assert np.array_equal(inf["gam"], -val)
    if sig is None:
        assert (inf["idx"] == 0).all() and not (st & 32).any()
        v0, _ = ctx.obj_w_grad(h, geo, t0, DEL)
        assert close(val, v0, 1e-9).all(), np.abs(val - v0).max()
    else:
        assert all(st[k] & 32 for k in range(3, n_pts, 4)), st[3::4]
        assert (inf["idx"][1::4] > 0).any()                           # (shifts inside the spectrum: not lam_max's eigenpair)
    against_host_composed(ctx, th, geo, t0, sig, val, jac, inf["idx"], "N=%d %s" % (N, mode))
    for k in np.random.default_rng(N).choice(n_pts, 12, replace=False):
        rv, rj, _ = obj_w_grad_exact_lines(th, t0[k], geo[k], None if sig is None else sig[k], DEL)
        ln = geo[k, 1]
        ref = dense_nearest(th, *gcf_at(bo.dPdrho_of(ln[2], ln[7], ln[0]), *ln[:7], t0[k]), 1e3 if sig is None else sig[k])
        assert int(inf["idx"][k]) == ref["idx"], (k, inf["idx"][k], ref["idx"])
        tv = max(1e-8, vec_tol(ref))
        assert close(val[k], rv, tv), (k, val[k], rv, tv)
        assert close(jac[k], rj, max(1e-7, 10 * tv)).all(), (k, jac[k], rj, tv)
    # central differences of the kernel's own val in theta0, steps 1e-4, 5e-5 and 2.5e-5.  Mixed shifts: on every point whose shift
    # does not sit midway between two eigenvalues (there the returned pair may switch inside the step); the index of the returned
    # eigenvalue must then be the same at every step, on every such point.
    # An interior pair can lie 6e-3 from its neighbour (the lam_max pairs: 0.1 and more): gam then bends within the step, and the plain
    # difference at 1e-4 is off by up to 3.6e-3 of the derivative -- its truncation error, a pure step-squared term (the oracle's own
    # derivative against the oracle's own differences at 1e-4 / 3e-5 / 1e-5: 3.1e-3 / 2.8e-4 / 3.1e-5 at N = 969, point 158).  The
    # reference is therefore the Richardson combination R1 = (4 fd(t/2) - fd(t)) / 3, which removes that term; where R1 itself has
    # not converged (its step-to-the-fourth term, 16/15 |R1(t) - R1(t/2)|, is above a third of the bound: on the oracle 3.5e-5 at point
    # 194, 8.6e-7 at 158) the next level R2 = (16 R1(t/2) - R1(t)) / 15 (oracle: 5.9e-8, 1.0e-10).  The bound is 1e-6 relative on
    # every point, against the best converged combination.
    def central(step):
        vp, _, ip = ctx.obj_w_grad_exact(h, geo, t0 + step, DEL, sigma=sig, want_info=True)
        vm, _, im = ctx.obj_w_grad_exact(h, geo, t0 - step, DEL, sigma=sig, want_info=True)
        ok = (ip["idx"] == inf["idx"]) & (im["idx"] == inf["idx"]) & (((ip["info"] | im["info"]) >> 16) & 35 == 0)
        return (vp - vm) / (2 * step), ok
    t = 1e-4
    (fd, ok1), (fd2, ok2), (fd4, ok4) = central(t), central(t / 2), central(t / 4)
    no_tie = (st & 32) == 0
    same = ok1 & ok2 & ok4 & no_tie
    assert no_tie.sum() == (n_pts if sig is None else n_pts - len(range(3, n_pts, 4))), no_tie.sum()
    assert np.array_equal(same, no_tie), np.nonzero(no_tie & ~same)[0]          # (the index is stable on every point without a tie)
    r1, r1h = (4.0 * fd2 - fd) / 3.0, (4.0 * fd4 - fd2) / 3.0
    r2 = (16.0 * r1h - r1) / 15.0
    deep = same & (16.0 / 15.0 * np.abs(r1 - r1h) > (1e-6 / 3) * np.abs(r1))
    ref_fd = np.where(deep, r2, r1)
    aj = np.abs(jac[:, 1])
    rel0, rel = np.abs(jac[:, 1] - fd) / aj, np.abs(jac[:, 1] - ref_fd) / aj
    print("exact-refine figures: N=%d %s jac_theta0 over %d points (min |jac| %.2e): worst relative mismatch against the plain "
          "difference at 1e-4 %.2e, against its Richardson combination %.2e (%d points on the second level)"
          % (N, mode, same.sum(), aj[same].min(), rel0[same].max(), rel[same].max(), deep.sum()))
    assert (rel[same] <= 1e-6).all(), (np.nonzero(same & (rel > 1e-6))[0][:8], rel[same].max())
    # host and device pointers, alone and in the batch
    dev = torch.device("cuda:0")
    ds = None if sig is None else torch.from_numpy(sig).to(dev)
    dv, dj, dinf = ctx.obj_w_grad_exact(h, torch.from_numpy(geo).to(dev), torch.from_numpy(t0).to(dev), DEL, sigma=ds, want_info=True)
    assert np.array_equal(dv.cpu().numpy(), val) and np.array_equal(dj.cpu().numpy(), jac)
    for key in ("gam", "lam", "idx", "info"):
        assert np.array_equal(dinf[key].cpu().numpy(), inf[key]), key
    for k in (0, 1, n_pts // 2 + 1, n_pts - 1):
        v1, j1, i1 = ctx.obj_w_grad_exact(h, geo[k:k + 1], t0[k:k + 1], DEL, sigma=None if sig is None else sig[k:k + 1], want_info=True)
        assert v1[0] == val[k] and np.array_equal(j1[0], jac[k]) and i1["info"][0] == inf["info"][k] and i1["lam"][0] == inf["lam"][k], k
    v2, j2 = ctx.obj_w_grad_exact(h, geo, t0, DEL, sigma=sig)
    assert np.array_equal(v2, val) and np.array_equal(j2, jac)        # (bitwise repeatable)


def test_errors_flag_their_own_point(ctx):
    """even N, N = 33 and N = 65,539 are refused; a NaN theta0 or sigma gives status 2 (val = jac = NaN) on its point only"""
    import ibs_amd
    for N in (512, 33, 65539):
        with pytest.raises(ibs_amd.IbsError):
            ctx.obj_w_grad_exact(0.05, np.ones((1, 3, 8, N)), np.zeros(1))
    th, geo, t0, sig = point_batch(513, 8, 5)
    h = th[1] - th[0]
    keep = np.arange(8) != 5
    for s_clean in (None, sig):
        clean = ctx.obj_w_grad_exact(h, geo, t0, DEL, sigma=s_clean, want_info=True)
        cases = [(np.where(keep, t0, np.nan), s_clean)]
        if s_clean is not None:
            cases.append((t0, np.where(keep, sig, np.nan)))
        for tt, ss in cases:
            r = ctx.obj_w_grad_exact(h, geo, tt, DEL, sigma=ss, want_info=True)
            assert (r[2]["info"][5] >> 16) & 3 == 2 and np.isnan(r[0][5]) and np.isnan(r[1][5]).all() and r[2]["idx"][5] == -1
            assert np.array_equal(r[0][keep], clean[0][keep]) and np.array_equal(r[1][keep], clean[1][keep])
            assert np.array_equal(r[2]["info"][keep], clean[2]["info"][keep])


def edge_points(N):
    """the smooth family at three (s, alpha, theta0) points (the last LDS chunk of this length), and the moving well mapped onto
    geometry arrays with its mode on twist targets -- both ends, on a multiple of 384 and two rows past another: the side lines are
    wells of depth 0.3 -+ 0.001, cvdrift0 = 0.1 cvdrift and theta0 = 0.25 make both tangents non-zero"""
    from tests.helpers import synthetic_fieldlines
    th = ec.theta_grid(N)
    fl = synthetic_fieldlines(th)
    pts = [(0.6, 1.0, 0.4), (0.8, 2.2, 0.0), (0.5, 0.3, 1.1)]
    geo = [fl(s_, np.array([a_ - DEL / 2, a_, a_ + DEL / 2])) for s_, a_, _ in pts]
    t0 = [p[2] for p in pts]
    t = ec.twist_targets(N)
    for j in [t[0], t[1], t[3], t[-1]]:
        lines = []
        for depth in (0.299, 0.3, 0.301):
            b, gp, cv, _, gds2, z1, z2 = ec.to_geometry(*ec.well_rows(th, j, depth=depth))
            lines.append(np.stack([b, gp, cv, 0.1 * cv, gds2, z1, z2, cv - 2.0 / b ** 2]))         # (dPdrho = -1)
        geo.append(np.stack(lines)); t0.append(0.25)
    return th, np.stack(geo), np.array(t0)


@pytest.mark.parametrize("N", ec.EDGE_N_LONG)
def test_exact_objective_on_long_edges(ctx, N):
    """the new entry at the long-path lengths of tests/edge_cases.py (the last LDS chunk holding 1, chunk - 1 and exactly chunk
    rows, the twist row on a multiple of 384) against the host-composed path, both eigenpairs (sigma = 1e3: lam_max's pair through
    the nearest-sigma solve)"""
    th, geo, t0 = edge_points(N)
    h = float(th[1] - th[0])
    for sig in (None, np.full(len(t0), 1e3)):
        val, jac, inf = ctx.obj_w_grad_exact(h, geo, t0, DEL, sigma=sig, want_info=True)
        assert not ((inf["info"] >> 16) & (3 | 128)).any(), (N, inf["info"] >> 16)
        assert (inf["idx"] == 0).all()
        against_host_composed(ctx, th, geo, t0, sig, val, jac, inf["idx"], "edge N=%d %s" % (N, "max" if sig is None else "nearest"))
        assert (np.abs(jac[3:]) > 0).all(), jac[3:]


def wout_scaled(factor):
    w = dict(np.load(os.path.join(G, "G8_wout_ncsx_op.npz")))
    w["pres"] = np.asarray(w["pres"], dtype=np.float64) * factor
    return w


PRES_SCALE = 50.0
SVALS = np.array([0.6, 0.9])


@pytest.mark.parametrize("N", [969, 2561])
@pytest.mark.parametrize("eigenpair", ["max", "nearest"])
def test_resident_scan_exact_on_ncsx_tables(ctx, N, eigenpair):
    """BallooningScan(jac="exact") on the device (G8 NCSX tables): the resident rows equal the host-callable path of the same
    object (gam 1e-8, angles 1e-4); every final gam equals gamma_points / the dense nearest pair at 0.42 of its final line;
    gam_exact >= gam_reference - 1e-10 per surface.  (The tables are the equilibrium's own: with the pressure scaled up 50 x, as
    the nearest-sigma scan test has it, the refinement's shift 1.3 |gam| + 0.05 and the final solve's 0.42 select different
    eigenpairs -- index 196 against the final one at N = 2,561, s = 0.9 -- so a better maximum of the refined objective says nothing
    about the final gam, upstream's included: there the reference run ended ABNORMAL after 57 evaluations beside its start with a
    final gam of 0.711, the exact run converged in 11 to the maximum of the refined pair, where the final pair has -0.086 and a
    slope of 13 in theta0.)"""
    import torch
    import ibs_amd
    dev = torch.device("cuda:0")
    th = np.linspace(-4 * np.pi, 4 * np.pi, N)
    h = th[1] - th[0]
    kw = dict(nalpha=8, ntheta0=5, eigenpair=eigenpair)
    tabs = ibs_amd.SurfaceTables.from_wout(wout_scaled(1.0), SVALS)
    res = ibs_amd.BallooningScan(ctx, None, th, SVALS, tables=tabs, device=dev, jac="exact", **kw)
    t_r, a_r, g_r = res.run()
    assert res.last_refine["rounds"] >= 1 and len(res.last_refine["n_evals"]) == len(SVALS)
    host = ibs_amd.BallooningScan(ctx, None, th, SVALS, tables=tabs, jac="exact", **kw)
    t_h, a_h, g_h = host.run()
    assert np.abs(g_r - g_h).max() < 1e-8, (g_r, g_h)
    assert np.abs(a_r - a_h).max() < 1e-4 and np.abs(t_r - t_h).max() < 1e-4, (a_r, a_h, t_r, t_h)
    for k, s in enumerate(SVALS):
        ln = host.fieldlines(s, np.array([a_r[k]]))[0]
        dP = bo.dPdrho_of(ln[2], ln[7], ln[0])
        if eigenpair == "max":
            gp = ctx.gamma_points(h, *[ln[q][None] for q in range(7)], np.array([dP]), np.array([t_r[k]]))["gam"][0]
            assert abs(g_r[k] - gp) < 1e-8, (k, g_r[k], gp)
        else:
            ref = dense_nearest(th, *gcf_at(dP, *ln[:7], t_r[k]), 0.42)
            assert abs(g_r[k] - ref["gam"]) <= max(1e-8, vec_tol(ref)), (k, g_r[k], ref["gam"])
    ref_scan = ibs_amd.BallooningScan(ctx, None, th, SVALS, tables=tabs, device=dev, jac="reference", **kw)
    t_f, a_f, g_f = ref_scan.run()
    diff = g_r - g_f
    msg = "N=%d eigenpair=%s gam_exact - gam_reference per surface: %s; rounds exact %s reference %s; evaluations per surface exact %s" % (
        N, eigenpair, " ".join("%.3e" % x for x in diff), res.last_refine["rounds"], ref_scan.last_refine["rounds"],
        [int(x) for x in res.last_refine["n_evals"]])
    print("exact-refine figures:", msg)
    if os.environ.get("IBS_EXACT_REFINE_PROFILES"):            # (a record for profiles/ is written on request only)
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "exact_refine_scan_N%d_%s.txt" % (N, eigenpair)), "w") as fh:
            fh.write(msg + "\n")
    assert (diff >= -1e-10).all(), msg


@pytest.mark.parametrize("N", [969, 2561])
def test_resident_scan_exact_nearest_through_interior_pairs(ctx, N):
    """BallooningScan(eigenpair="nearest", jac="exact") with the pressure scaled up 50 x: the refinement's shift lies inside the
    spectrum, so the driver runs the exact gradient of an INTERIOR pair (asserted: idx > 0 at the start points).  The resident rows
    equal the host-callable path's (angles 1e-4) and the final gam is the dense nearest pair at 0.42 of its final line.  No
    gam_exact >= gam_reference here (see the test above).  The final pair is not the refined one, so its gam is not stationary at
    the refined point: the two paths' final gam agree to 1e-8 plus twice the final pair's slope (central differences of the final
    solve, step 1e-5) times the distance between the two end points."""
    import torch
    import ibs_amd
    from ibs_amd.scan import SIGMA_FINAL, pick_start
    dev = torch.device("cuda:0")
    th = np.linspace(-4 * np.pi, 4 * np.pi, N)
    h = th[1] - th[0]
    kw = dict(nalpha=8, ntheta0=5, eigenpair="nearest", jac="exact")
    tabs = ibs_amd.SurfaceTables.from_wout(wout_scaled(PRES_SCALE), SVALS)
    t_r, a_r, g_r = ibs_amd.BallooningScan(ctx, None, th, SVALS, tables=tabs, device=dev, **kw).run()
    host = ibs_amd.BallooningScan(ctx, None, th, SVALS, tables=tabs, **kw)
    t_h, a_h, g_h = host.run()
    assert np.abs(a_r - a_h).max() < 1e-4 and np.abs(t_r - t_h).max() < 1e-4, (a_r, a_h, t_r, t_h)

    def final_gam(s, a, t0):
        ln = host.fieldlines(s, np.array([a]))[0]
        dP = bo.dPdrho_of(ln[2], ln[7], ln[0])
        return ctx.gamma_points_nearest(h, *[ln[q][None] for q in range(7)], np.array([dP]), np.array([t0]), SIGMA_FINAL)["gam"][0], ln, dP

    interior = 0
    for k, (s, tab) in enumerate(zip(SVALS, host.coarse())):
        a0, t00, sigma0, _ = pick_start(tab, host.alpha_scan, host.theta0_scan)
        geo = host.fieldlines(s, np.array([a0 - DEL / 2, a0, a0 + DEL / 2]))
        interior += int(ctx.obj_w_grad_exact(h, geo[None], np.array([t00]), DEL, sigma=sigma0, want_info=True)[2]["idx"][0] > 0)
        g0, ln, dP = final_gam(s, a_r[k], t_r[k])
        ref = dense_nearest(th, *gcf_at(dP, *ln[:7], t_r[k]), 0.42)
        assert abs(g_r[k] - ref["gam"]) <= max(1e-8, vec_tol(ref)), (k, g_r[k], ref["gam"])
        e = 1e-5
        a_lo, a_hi = max(a_r[k] - e, 0.0), min(a_r[k] + e, np.pi)
        t_lo, t_hi = max(t_r[k] - e, 0.0), min(t_r[k] + e, 0.5 * np.pi)
        sl_a = abs(final_gam(s, a_hi, t_r[k])[0] - final_gam(s, a_lo, t_r[k])[0]) / (a_hi - a_lo)
        sl_t = abs(final_gam(s, a_r[k], t_hi)[0] - final_gam(s, a_r[k], t_lo)[0]) / (t_hi - t_lo)
        bound = 1e-8 + 2.0 * (sl_a * abs(a_r[k] - a_h[k]) + sl_t * abs(t_r[k] - t_h[k]))
        print("exact-refine figures: N=%d 50 x pressure, nearest, surface %d: |gam_resident - gam_host| %.2e (bound %.2e: slopes %.2e, %.2e; "
              "end points %.1e, %.1e apart)" % (N, k, abs(g_r[k] - g_h[k]), bound, sl_a, sl_t, abs(a_r[k] - a_h[k]), abs(t_r[k] - t_h[k])))
        assert abs(g_r[k] - g_h[k]) <= bound, (k, g_r[k], g_h[k], bound)
    assert interior >= 1, interior


def test_adjoint_step_exact(ctx):
    """AdjointStep(jac="exact") on three equilibria (base, scaled pressure, a perturbed boundary mode), N = 969: every equilibrium's
    rows equal a separate BallooningScan(jac="exact") run, f0 / fobj / dfobj follow from those rows; AdjointStep() and
    AdjointStep(jac="reference") agree bit for bit on every key"""
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
    out = ibs_amd.AdjointStep(ctx, th, SVALS, dev, jac="exact", **kw).run(wouts, f_other, steps)
    rows = []
    for w in wouts:
        tabs = ibs_amd.SurfaceTables.from_wout(w, SVALS)
        rows.append(ibs_amd.BallooningScan(ctx, None, th, SVALS, nalpha=8, ntheta0=5, tables=tabs, device=dev, jac="exact").run())
    rows = np.array(rows)                                    # (3 equilibria, theta0 / alpha / gam, surfaces)
    assert np.abs(out["gam"] - rows[:, 2]).max() < 1e-8, (out["gam"], rows[:, 2])
    assert np.abs(out["alpha"] - rows[:, 1]).max() < 1e-4 and np.abs(out["theta0"] - rows[:, 0]).max() < 1e-4
    f0 = ibs_amd.ballooning_objective(f_other, out["gam"], -2.0e-4, 50.0)
    assert np.array_equal(out["f0"], f0) and out["fobj"] == float(np.sqrt(f0[0]))
    assert np.array_equal(out["dfobj"], ibs_amd.dof_fd_gradient(f0, steps))
    rf = ibs_amd.AdjointStep(ctx, th, SVALS, dev, jac="reference", **kw).run(wouts, f_other, steps)
    df = ibs_amd.AdjointStep(ctx, th, SVALS, dev, **kw).run(wouts, f_other, steps)
    for key in ("gam", "theta0", "alpha", "f0", "dfobj"):
        assert np.array_equal(rf[key], df[key]), key
    assert rf["fobj"] == df["fobj"]
    print("exact-refine figures: AdjointStep gam_exact - gam_reference:", " ".join("%.3e" % x for x in (out["gam"] - rf["gam"]).ravel()))
