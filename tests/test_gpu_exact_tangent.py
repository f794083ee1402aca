"""GPU: the point objective with the gradient exact in alpha as well (ibs_obj_w_grad_exact_tangent_f64) and the drivers'
jac="exact_tangent" mode -- against ibs_obj_w_grad_exact_f64 on the same centre line (bit for bit outside jac_alpha), central
differences in alpha of the kernel's own val, the CPU adjoint of tests/vjp_oracle.py contracted with the oracle's tangent rows, the
del_alpha difference it replaces, and on the NCSX tables the central difference in alpha of the final solve's gam."""
import numpy as np
import pytest

from oracle import ballooning_oracle as bo
from tests import geometry_tangent_oracle as to
from tests.nearest_oracle import dense_nearest, gcf_at
from tests.test_gpu_exact_refine import SVALS, close, top_two, vec_tol, wout_scaled
from tests.vjp_oracle import eigenpair, gcf_vjp

pytestmark = pytest.mark.gpu
DEL = 0.004


@pytest.fixture(scope="module")
def ctx():
    import ibs_amd
    c = ibs_amd.Context(0)
    yield c
    c.close()


def lines_at(th, par, shift=0.0):
    """(8, n, N): the driven synthetic field line of every point (tests.helpers.synthetic_fieldlines with dPdrho = -K, as point_batch of
    tests/test_gpu_exact_refine.py has them) at alpha + shift: analytic in alpha"""
    from tests.helpers import synthetic_fieldlines
    base = synthetic_fieldlines(th)
    out = np.empty((8, len(par), len(th)))
    for k, (s, a, K) in enumerate(par):
        ln = base(s, np.array([a + shift]))[0]
        ln[7] = ln[2] - 2.0 * K / ln[0] ** 2
        out[:, k] = ln
    return out


def tangent_planes(th, par):
    """d/d alpha of lines_at by Richardson-combined central differences at steps 1e-3, 5e-4, 2.5e-4: R1(t) = (4 fd(t/2) - fd(t)) / 3 at
    t = 1e-3 and 5e-4, then R2 = (16 R1(t/2) - R1(t)) / 15; usable where the two R1 levels agree to 1e-9 of the plane maximum, which
    must be everywhere (asserted)"""
    fd = lambda t: (lines_at(th, par, t) - lines_at(th, par, -t)) / (2 * t)
    f1, f2, f4 = fd(1e-3), fd(5e-4), fd(2.5e-4)
    r1, r1h = (4.0 * f2 - f1) / 3.0, (4.0 * f4 - f2) / 3.0
    scale = np.abs(r1h).max(axis=(1, 2), keepdims=True)
    ok = np.abs(r1 - r1h) <= 1e-9 * np.where(scale > 0, scale, 1.0)
    assert ok.all(), (int((~ok).sum()), np.abs(r1 - r1h).max(axis=(1, 2)) / np.where(scale > 0, scale, 1.0)[:, 0, 0])
    return (16.0 * r1h - r1) / 15.0


_BATCH = {}


def batch(N, n_pts):
    """points (s, alpha, K in {1, 4, 8}), theta0, the mixed shifts of point_batch (above lam_max / 0.42 / 1.0 / midway between the two
    largest eigenvalues: a tie, bit 5), the centre lines and their tangent planes: computed once per shape"""
    if (N, n_pts) not in _BATCH:
        th = bo.theta_grid(N)
        rng = np.random.default_rng(40417 + N)
        t0 = rng.uniform(0.0, 0.5 * np.pi, n_pts)
        par = [(rng.uniform(0.3, 0.9), rng.uniform(0.0, np.pi), (1.0, 4.0, 8.0)[k % 3]) for k in range(n_pts)]
        geo = lines_at(th, par)
        sig = np.empty(n_pts)
        for k in range(n_pts):
            m = k % 4
            if m < 3:
                sig[k] = (1e3, 0.42, 1.0)[m]
            else:
                ln = geo[:, k]
                sig[k] = 0.5 * sum(top_two(th, *gcf_at(bo.dPdrho_of(ln[2], ln[7], ln[0]), *ln[:7], t0[k])))
        _BATCH[(N, n_pts)] = dict(th=th, h=float(th[1] - th[0]), par=par, t0=t0, sig=sig, geo=geo, geo_da=tangent_planes(th, par))
    return _BATCH[(N, n_pts)]


def three_lines(th, par, d):
    """(n, 3, 8, N): the lines alpha - d / 2, alpha, alpha + d / 2 in ibs_obj_w_grad_exact_f64's layout"""
    return np.ascontiguousarray(np.stack([lines_at(th, par, sh) for sh in (-0.5 * d, 0.0, 0.5 * d)]).transpose(2, 0, 1, 3))


SHAPES = [(67, 5), (513, 96), (969, 600), (2313, 3)]


@pytest.mark.parametrize("N,n_pts", SHAPES)
@pytest.mark.parametrize("mode", ["max", "mixed"])
def test_obj_w_grad_exact_tangent_batched(ctx, N, n_pts, mode):
    """ibs_obj_w_grad_exact_tangent_f64 on batches of analytic lines (600 points at N = 969: beyond the 512-point carve-out of the
    persistent grid), sigma = NULL or mixed shifts:
    1. val, gam, lam, idx, info and jac[:, 1] are the bits of ibs_obj_w_grad_exact_f64 on the same centre line;
    2. jac[:, 0] against central differences in alpha of the kernel's own val, the lines regenerated at alpha +- t (t = 1e-4, 5e-5,
       2.5e-5, the Richardson scheme and the 1e-6 relative bound of test_obj_w_grad_exact_batched) on every point without a tie,
       where the index of the returned eigenvalue must be the same at every step;
    3. on a sample of 12, jac[:, 0] against the adjoint rows of tests/vjp_oracle.py contracted with the oracle's tangent rows
       (1e-7 or the gap-aware bound of that test);
    4. |jac_alpha - jac_alpha of ibs_obj_w_grad_exact_f64| shrinks by a factor in [3, 5] when del_alpha goes 0.008 -> 0.004, on the
       points where it is above 1e-9;
    5. host and device pointers agree bit for bit, a point alone gives its batch bits, results repeat bit for bit.
    Measured on an MI355X (docs/EXPERIMENTS.md R6.13): 2. worst 4.5e-8 (smallest |jac_alpha| 3.6e-5); 3. worst 2.3e-14; 4. ratios
    3.998 .. 4.002, gaps up to 1.3e-5 / 3.3e-6."""
    import torch
    b = batch(N, n_pts)
    th, h, par, t0, geo, gda = b["th"], b["h"], b["par"], b["t0"], b["geo"], b["geo_da"]
    sig = None if mode == "max" else b["sig"]
    val, jac, inf = ctx.obj_w_grad_exact_tangent(h, geo, gda, t0, sigma=sig, want_info=True)
    assert ctx.last_launch()[0] == "ibs::k_exact_tangent_points<%s>" % ("false" if sig is None else "true"), ctx.last_launch()
    st = inf["info"] >> 16
    assert int(((st & 3) != 0).sum()) == 0 and np.isfinite(val).all() and np.isfinite(jac).all()
    assert not (st & 128).any(), np.nonzero(st & 128)
    # 1. the centre line's results, bit for bit
    g3 = three_lines(th, par, DEL)
    assert np.array_equal(g3[:, 1], geo.transpose(1, 0, 2))
    ev, ej, einf = ctx.obj_w_grad_exact(h, g3, t0, DEL, sigma=sig, want_info=True)
    assert ctx.last_launch()[0] == "ibs::k_exact_points<%s>" % ("false" if sig is None else "true"), ctx.last_launch()
    assert np.array_equal(val, ev) and np.array_equal(jac[:, 1], ej[:, 1])
    for key in ("gam", "lam", "idx", "info"):
        assert np.array_equal(inf[key], einf[key]), key
    # 2. central differences of the kernel's own val in alpha
    def central(step):
        vp, _, ip = ctx.obj_w_grad_exact_tangent(h, lines_at(th, par, step), gda, t0, sigma=sig, want_info=True)
        vm, _, im = ctx.obj_w_grad_exact_tangent(h, lines_at(th, par, -step), gda, t0, sigma=sig, want_info=True)
        ok = (ip["idx"] == inf["idx"]) & (im["idx"] == inf["idx"]) & (((ip["info"] | im["info"]) >> 16) & 35 == 0)
        return (vp - vm) / (2 * step), ok
    t = 1e-4
    (fd, ok1), (fd2, ok2), (fd4, ok4) = central(t), central(t / 2), central(t / 4)
    no_tie = (st & 32) == 0
    same = ok1 & ok2 & ok4 & no_tie
    assert no_tie.sum() == (n_pts if sig is None else n_pts - len(range(3, n_pts, 4))), no_tie.sum()
    assert np.array_equal(same, no_tie), np.nonzero(no_tie & ~same)[0]
    r1, r1h = (4.0 * fd2 - fd) / 3.0, (4.0 * fd4 - fd2) / 3.0
    r2 = (16.0 * r1h - r1) / 15.0
    deep = same & (16.0 / 15.0 * np.abs(r1 - r1h) > (1e-6 / 3) * np.abs(r1))
    ref_fd = np.where(deep, r2, r1)
    aj = np.abs(jac[:, 0])
    rel0, rel = np.abs(jac[:, 0] - fd) / aj, np.abs(jac[:, 0] - ref_fd) / aj
    print("exact-tangent figures: N=%d %s jac_alpha over %d points (min |jac| %.2e, max %.2e): worst relative mismatch against the plain "
          "difference at 1e-4 %.2e, against its Richardson combination %.2e (%d points on the second level)"
          % (N, mode, same.sum(), aj[same].min(), aj[same].max(), rel0[same].max(), rel[same].max(), deep.sum()))
    assert (rel[same] <= 1e-6).all(), (np.nonzero(same & (rel > 1e-6))[0][:8], rel[same].max())
    # 3. the CPU adjoint contracted with the oracle's tangent rows
    g_a, c_a, f_a = to.rows_dalpha(geo, gda, t0)
    worst = 0.0
    for k in np.random.default_rng(N).choice(n_pts, min(12, n_pts), replace=False):
        ln = geo[:, k]
        g, c, f = gcf_at(bo.dPdrho_of(ln[2], ln[7], ln[0]), *ln[:7], t0[k])
        ref = dense_nearest(th, g, c, f, 1e3 if sig is None else sig[k])
        assert int(inf["idx"][k]) == ref["idx"], (k, inf["idx"][k], ref["idx"])
        gam, lam, X = eigenpair(th, g, c, f, None if sig is None else sig[k])
        gb, cb, fb = gcf_vjp(th, g, c, f, lam, X)
        rj = -(gb @ g_a[k] + cb @ c_a[k] + fb @ f_a[k])
        tv = max(1e-8, vec_tol(ref))
        worst = max(worst, abs(jac[k, 0] - rj) / max(1.0, abs(rj)))
        assert close(jac[k, 0], rj, max(1e-7, 10 * tv)), (k, jac[k, 0], rj, tv)
    print("exact-tangent figures: N=%d %s jac_alpha against the CPU adjoint x oracle tangent rows: worst %.2e" % (N, mode, worst))
    # 4. the del_alpha difference converges onto the tangent as del_alpha^2
    j8 = ctx.obj_w_grad_exact(h, three_lines(th, par, 0.008), t0, 0.008, sigma=sig)[1][:, 0]
    gap8, gap4 = np.abs(jac[:, 0] - j8), np.abs(jac[:, 0] - ej[:, 0])
    big = same & (gap4 > 1e-9)
    ratio = gap8[big] / gap4[big]
    print("exact-tangent figures: N=%d %s |jac_alpha(tangent) - jac_alpha(exact)| at del_alpha 0.008 / 0.004: worst %.2e / %.2e, ratio "
          "%.3f .. %.3f over %d points" % (N, mode, gap8[same].max(), gap4[same].max(), ratio.min(), ratio.max(), big.sum()))
    assert big.sum() > 0 and (ratio >= 3.0).all() and (ratio <= 5.0).all(), (ratio.min(), ratio.max())
    # 5. pointers, batch, repeats
    dev = torch.device("cuda:0")
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    dv, dj, dinf = ctx.obj_w_grad_exact_tangent(h, tt(geo), tt(gda), tt(t0), sigma=None if sig is None else tt(sig), want_info=True)
    assert np.array_equal(dv.cpu().numpy(), val) and np.array_equal(dj.cpu().numpy(), jac)
    for key in ("gam", "lam", "idx", "info"):
        assert np.array_equal(dinf[key].cpu().numpy(), inf[key]), key
    for k in (0, 1, n_pts // 2 + 1, n_pts - 1):
        v1, j1, i1 = ctx.obj_w_grad_exact_tangent(h, geo[:, k:k + 1], gda[:, k:k + 1], t0[k:k + 1],
                                                  sigma=None if sig is None else sig[k:k + 1], want_info=True)
        assert v1[0] == val[k] and np.array_equal(j1[0], jac[k]) and i1["info"][0] == inf["info"][k] and i1["lam"][0] == inf["lam"][k], k
    v2, j2 = ctx.obj_w_grad_exact_tangent(h, geo, gda, t0, sigma=sig)
    assert np.array_equal(v2, val) and np.array_equal(j2, jac)


def test_errors_flag_their_own_point(ctx):
    """even N, N = 33 and N = 65,539 are refused; a NaN theta0 gives status 2 (val = jac = NaN) on its point only; a NaN planted in
    geo_da gives jac[k][0] = NaN with val[k], jac[k][1] and every other point kept"""
    import ibs_amd
    for N in (512, 33, 65539):
        with pytest.raises(ibs_amd.IbsError):
            ctx.obj_w_grad_exact_tangent(0.05, np.ones((8, 1, N)), np.zeros((8, 1, N)), np.zeros(1))
    b = batch(513, 96)
    h, geo, gda, t0 = b["h"], b["geo"][:, :8], b["geo_da"][:, :8], b["t0"][:8]
    keep = np.arange(8) != 5
    for sig in (None, b["sig"][:8]):
        clean = ctx.obj_w_grad_exact_tangent(h, geo, gda, t0, sigma=sig, want_info=True)
        r = ctx.obj_w_grad_exact_tangent(h, geo, gda, np.where(keep, t0, np.nan), sigma=sig, want_info=True)
        assert (r[2]["info"][5] >> 16) & 3 == 2 and np.isnan(r[0][5]) and np.isnan(r[1][5]).all() and r[2]["idx"][5] == -1
        assert np.array_equal(r[0][keep], clean[0][keep]) and np.array_equal(r[1][keep], clean[1][keep])
        assert np.array_equal(r[2]["info"][keep], clean[2]["info"][keep])
        bad = gda.copy(); bad[4, 5, 200] = np.nan
        r = ctx.obj_w_grad_exact_tangent(h, geo, bad, t0, sigma=sig, want_info=True)
        assert np.isnan(r[1][5, 0]) and r[1][5, 1] == clean[1][5, 1] and np.array_equal(r[0], clean[0])
        assert np.array_equal(r[1][keep], clean[1][keep]) and np.array_equal(r[2]["info"], clean[2]["info"])


# ---- the workflow on the NCSX tables ------------------------------------------------------------------------------------
N_SCAN = 969
KW = dict(nalpha=8, ntheta0=5)


def _final_gam(scan, surf, al, t0):
    """gam of the final solve (geometry + gamma_points, or the pair nearest 0.42) at points (surface index, alpha, theta0)"""
    import torch
    from ibs_amd.scan import SIGMA_FINAL
    r = scan.ctx.fieldline_geometry(scan.tables, np.asarray(surf, dtype=np.int32), np.ascontiguousarray(al), scan.theta, device=scan.device)
    tt = torch.from_numpy(np.ascontiguousarray(t0)).to(scan.device)
    g7 = [r["geo"][k] for k in range(7)]
    if scan.nearest:
        out = scan.ctx.gamma_points_nearest(scan.h, *g7, r["dPdrho"], tt, SIGMA_FINAL)
    else:
        out = scan.ctx.gamma_points(scan.h, *g7, r["dPdrho"], tt)
    return out["gam"].cpu().numpy()


def _dgam_dalpha(scan, surf, al, t0):
    """Richardson-combined central differences (steps 1e-3, 5e-4, 2.5e-4, the scheme of tangent_planes) in alpha of the final solve's gam"""
    surf, al, t0 = np.asarray(surf), np.asarray(al, dtype=np.float64), np.asarray(t0, dtype=np.float64)
    n = len(al)
    steps = np.array([1e-3, 5e-4, 2.5e-4])
    sh = np.concatenate([steps, -steps])
    g = _final_gam(scan, np.tile(surf, 6), (al[None, :] + sh[:, None]).reshape(-1), np.tile(t0, 6)).reshape(6, n)
    f1, f2, f4 = ((g[k] - g[3 + k]) / (2 * steps[k]) for k in range(3))
    r1, r1h = (4.0 * f2 - f1) / 3.0, (4.0 * f4 - f2) / 3.0
    return (16.0 * r1h - r1) / 15.0


def _alpha_slope_report(scan, t_r, a_r, tag):
    """per surface: (refined point interior to the box, d gam / d alpha of the final solve there by differences, the kernel's own
    jac_alpha there at the final solve's eigenpair, S = the largest |d gam / d alpha| over the coarse alpha nodes at theta0*)"""
    from ibs_amd.scan import SIGMA_FINAL
    n = len(a_r)
    surf = scan._own_surf()
    fd = _dgam_dalpha(scan, surf, a_r, t_r)
    na = len(scan.alpha_scan)
    nodes = _dgam_dalpha(scan, np.repeat(surf, na), np.tile(scan.alpha_scan, n), np.repeat(t_r, na)).reshape(n, na)
    S = np.abs(nodes).max(axis=1)
    _, jac = scan.batched_obj_w_grad(surf, np.stack([a_r, t_r], axis=1), np.full(n, SIGMA_FINAL) if scan.nearest else None)
    e = 1e-6
    interior = (a_r > e) & (a_r < np.pi - e) & (t_r > e) & (t_r < 0.5 * np.pi - e)
    for k in range(n):
        print("exact-tangent figures: %s surface %d at (alpha, theta0) = (%.6f, %.6f)%s: d gam / d alpha by differences %.3e, kernel "
              "%.3e, S %.3e, |difference| / S %.2e" % (tag, k, a_r[k], t_r[k], "" if interior[k] else " (on the box)", fd[k], -jac[k, 0],
                                                    S[k], abs(fd[k] + jac[k, 0]) / S[k]))
    return interior, fd, -jac[:, 0], S


@pytest.mark.parametrize("eigenpair_mode", ["max", "nearest"])
def test_scan_exact_tangent_on_ncsx_tables(ctx, eigenpair_mode):
    """BallooningScan(jac="exact_tangent") on the G8 NCSX tables at N = 969 (the smallest N of
    test_resident_scan_exact_on_ncsx_tables), both eigenpairs: the resident form (run(): device_rows) equals the host-driven form
    composed here (coarse -> pick_start -> refine_batched -> final_solve_device), gam 1e-8, points 1e-4.  At every surface whose
    refined point is interior to the box, the Richardson central difference in alpha of the FINAL solve's gam is within 1e-6 S of the
    kernel's jac_alpha at that point (taken at the final solve's eigenpair), S the largest |d gam / d alpha| over the surface's coarse
    alpha nodes by the same differences.  The same figures are printed for jac="exact" at its own refined points.  Measured on an
    MI355X (docs/EXPERIMENTS.md R6.13): |difference| / S 1.0e-8 and 3.1e-11 (max, nearest) at the interior point; jac="exact" leaves a
    true slope of 8.5e-5 S there."""
    import torch
    import ibs_amd
    from ibs_amd.scan import pick_start
    dev = torch.device("cuda:0")
    th = np.linspace(-4 * np.pi, 4 * np.pi, N_SCAN)
    tabs = ibs_amd.SurfaceTables.from_wout(wout_scaled(1.0), SVALS)
    kw = dict(tables=tabs, device=dev, eigenpair=eigenpair_mode, **KW)
    res = ibs_amd.BallooningScan(ctx, None, th, SVALS, jac="exact_tangent", **kw)
    t_r, a_r, g_r = res.run()
    assert ctx.last_launch()[0].startswith("ibs::")
    assert res.last_refine["rounds"] >= 1 and len(res.last_refine["n_evals"]) == len(SVALS)
    host = ibs_amd.BallooningScan(ctx, None, th, SVALS, jac="exact_tangent", **kw)
    starts = [pick_start(tab, host.alpha_scan, host.theta0_scan) for tab in host.coarse()]
    x_h, _, rounds = host.refine_batched(np.array([[s[0], s[1]] for s in starts]), sigma0=np.array([s[2] for s in starts]))
    assert ctx.last_launch()[0] == "ibs::k_exact_tangent_points<%s>" % ("true" if eigenpair_mode == "nearest" else "false")
    g_h = host.final_solve_device(x_h)
    assert np.abs(g_r - g_h).max() < 1e-8, (g_r, g_h)
    assert np.abs(a_r - x_h[:, 0]).max() < 1e-4 and np.abs(t_r - x_h[:, 1]).max() < 1e-4, (a_r, t_r, x_h)
    interior, fd, kern, S = _alpha_slope_report(res, t_r, a_r, "exact_tangent %s" % eigenpair_mode)
    ex = ibs_amd.BallooningScan(ctx, None, th, SVALS, jac="exact", **kw)
    t_e, a_e, g_e = ex.run()
    _alpha_slope_report(ex, t_e, a_e, "exact %s" % eigenpair_mode)
    print("exact-tangent figures: %s gam_exact_tangent - gam_exact per surface: %s; rounds %d against %d" % (
        eigenpair_mode, " ".join("%.3e" % x for x in g_r - g_e), res.last_refine["rounds"], ex.last_refine["rounds"]))
    assert (np.abs(fd - kern)[interior] <= 1e-6 * S[interior]).all(), (fd, kern, S, interior)


def test_adjoint_step_exact_tangent(ctx):
    """AdjointStep(jac="exact_tangent") on two equilibria (base, scaled pressure), N = 969: every equilibrium's rows equal a separate
    BallooningScan(jac="exact_tangent") run (gam 1e-8, points 1e-4), f0 / fobj / dfobj follow from those rows"""
    import torch
    import ibs_amd
    from tests.test_gpu_exact_refine import PRES_SCALE
    dev = torch.device("cuda:0")
    wouts = [wout_scaled(1.0), wout_scaled(PRES_SCALE)]
    steps = np.array([1.0, 1e-3])
    f_other = np.array([0.8, 0.81])
    th = ibs_amd.theta_grid_for(11, 11)
    assert len(th) == 969
    out = ibs_amd.AdjointStep(ctx, th, SVALS, dev, jac="exact_tangent", gamma_thresh=-2.0e-4, prefac=50.0, **KW).run(wouts, f_other, steps)
    rows = []
    for w in wouts:
        tabs = ibs_amd.SurfaceTables.from_wout(w, SVALS)
        rows.append(ibs_amd.BallooningScan(ctx, None, th, SVALS, tables=tabs, device=dev, jac="exact_tangent", **KW).run())
    rows = np.array(rows)                                    # (2 equilibria, theta0 / alpha / gam, surfaces)
    assert np.abs(out["gam"] - rows[:, 2]).max() < 1e-8, (out["gam"], rows[:, 2])
    assert np.abs(out["alpha"] - rows[:, 1]).max() < 1e-4 and np.abs(out["theta0"] - rows[:, 0]).max() < 1e-4
    f0 = ibs_amd.ballooning_objective(f_other, out["gam"], -2.0e-4, 50.0)
    assert np.array_equal(out["f0"], f0) and out["fobj"] == float(np.sqrt(f0[0]))
    assert np.array_equal(out["dfobj"], ibs_amd.dof_fd_gradient(f0, steps))
