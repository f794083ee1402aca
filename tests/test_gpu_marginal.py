"""GPU: the marginal-stability entry points (ibs_marginal_gcf_f64 / ibs_marginal_scan_f64, csrc/ibs_marginal.hip) against the CPU
restatement tests/marginal_oracle.py.

Accuracy bound: |s* - s*_oracle| <= 4 u, u = N eps normT / kappa from the oracle's vector (normT = max_j (s* |c_j| + 2 D_jj), kappa =
sum c_j X_j^2 / sum X_j^2 = d lam_max / d s at s*): the library's 4 N eps ||A|| rule carried over to s -- the division-form count is
exact for rows a few ulp away, and lam_max(T(s)) moves by kappa per unit of s.  Independent FP64 methods on the CPU spread by 0.003 u.
The measured worst case is printed (and written to the file named by IBS_MARGINAL_REPORT, if set: profiles/marginal_tests.txt)."""
import os

import numpy as np
import pytest

from oracle import ballooning_oracle as bo
from tests import edge_cases as ec
from tests import marginal_oracle as mo

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(__file__), "golden")
SALPHA = [(0.3, 0.3, 0.0), (1.0, 0.8, 0.3), (1.5, 1.1, 0.1)]
_REPORT = []


def report(line):
    print("marginal figures:", line)
    _REPORT.append(line)
    path = os.environ.get("IBS_MARGINAL_REPORT")
    if path:
        with open(path, "w") as fh:
            fh.write("\n".join(_REPORT) + "\n")


@pytest.fixture(scope="module")
def ctx():
    import ibs_amd
    return ibs_amd.Context(0)


def make_cases():
    """(name, h, g (n, N), c (n, N), smooth) of the raw systems of the accuracy tests"""
    out = []
    for N in (67, 69, 129):
        th = bo.theta_grid(N)
        gc = [bo.salpha_gc(th, *p) for p in SALPHA]
        out.append(("s-alpha N=%d" % N, th[1] - th[0], np.stack([a for a, _ in gc]), np.stack([b for _, b in gc]), True))
    # moving wells: N - 2 = 383 / 385 (the last vector chunk one short / one row), 767 / 769 (the last count chunk one short / one row)
    for N in (385, 387, 769, 771, 2305, 2307):
        th = ec.theta_grid(N)
        rows = [ec.well_rows(th, j) for j in ec.twist_targets(N)]
        out.append(("wells N=%d" % N, th[1] - th[0], np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows]), True))
    rng = np.random.default_rng(20240611)
    th = bo.theta_grid(257)
    out.append(("rough N=257", th[1] - th[0], np.exp(rng.uniform(np.log(0.01), np.log(50.0), (16, 257))),
                rng.uniform(-2.5, 3.5, (16, 257)), False))
    th = bo.theta_grid(65535)
    g, c = bo.salpha_gc(th, 1.0, 0.8, 0.3)
    out.append(("s-alpha N=65535", th[1] - th[0], g[None], c[None], False))
    return out


@pytest.fixture(scope="module")
def solved(ctx):
    """every case solved once on the GPU (all outputs) and by the oracle; shared, unchanged, by the tests below"""
    res = []
    for name, h, g, c, smooth in make_cases():
        r = ctx.marginal_gcf(h, g, c, want_X=True, want_grad=True, want_info=True)
        res.append(dict(name=name, h=h, g=g, c=c, smooth=smooth, gpu=r, ref=[mo.solve(h, g[k], c[k]) for k in range(len(g))]))
    return res


def test_accuracy_of_the_scale(solved):
    worst, lines = 0.0, []
    for s in solved:
        r = s["gpu"]
        assert r["nbad"] == 0 and not (r["info"] >> 16).any(), (s["name"], r["info"] >> 16)
        ref_s = np.array([q["scale"] for q in s["ref"]]); u = np.array([q["u"] for q in s["ref"]])
        assert np.isfinite(ref_s).all()
        err = np.abs(r["scale"] - ref_s) / u
        lines.append("%-16s systems %2d  max |s - s_oracle| / u %.2e  (max relative %.1e)  passes %.1f  mu rel %.1e" % (
            s["name"], len(u), err.max(), (np.abs(r["scale"] - ref_s) / ref_s).max(), (r["info"] & 0xffff).mean(),
            np.abs(r["mu"] * ref_s - 1).max()))
        worst = max(worst, err.max())
    for ln in lines:
        report(ln)
    report("worst case over all systems: %.2e u (bound 4 u)" % worst)
    for s in solved:
        ref_s = np.array([q["scale"] for q in s["ref"]]); u = np.array([q["u"] for q in s["ref"]])
        assert (np.abs(s["gpu"]["scale"] - ref_s) <= 4 * u).all(), s["name"]
        assert (np.abs(s["gpu"]["mu"] * ref_s - 1) <= 4 * u / ref_s + 4e-16).all(), s["name"]


def top_gap(q):
    """the distance of lam_max(T(s*)) = 0 from the next eigenvalue of T(s*)"""
    from scipy.linalg import eigh_tridiagonal
    n = len(q["Dd"])
    w = eigh_tridiagonal(q["scale"] * q["cj"] - q["Dd"], q["e"][1:n], eigvals_only=True, select="i", select_range=(n - 2, n - 1))
    return float(w[1] - w[0])


def test_marginal_mode(solved):
    """X against the oracle's vector: 1e-8 on the smooth systems; elsewhere (iid-rough rows, N = 65,535) both vectors carry the
    conditioning of the problem, N eps normT / gap as in tests/test_gpu_parity.py's eigvec_tol, and the bound is the larger of the two.
    gam0, the FD4 / Simpson quotient of the mode, is finite."""
    for s in solved:
        r = s["gpu"]
        errs = []
        for k, q in enumerate(s["ref"]):
            N = len(q["X"])
            tol = 1e-8 if s["smooth"] else max(1e-8, 2 * N * mo.EPS * q["normT"] / top_gap(q))
            e = np.abs(r["X"][k] - q["X"]).max()
            errs.append(e)
            assert e <= tol, (s["name"], k, e, tol)
            assert abs(r["X"][k].max() - 1.0) <= 4e-16 and r["X"][k, 0] == 0.0 and r["X"][k, -1] == 0.0 and r["X"][k].min() >= 0.0
        assert np.isfinite(r["gam0"]).all()
        report("%-16s max |X - X_oracle| %.1e  max |gam0| %.1e" % (s["name"], max(errs), np.abs(r["gam0"]).max()))


def test_derivative_rows(solved):
    """g_bar, c_bar against the oracle's formula: 1e-9 relative to max(1, |.|), the project's bar for Hellmann-Feynman sums"""
    for s in solved:
        r = s["gpu"]
        eg = ecb = 0.0
        for k, q in enumerate(s["ref"]):
            gb, cb = mo.grad_rows(s["h"], q)
            eg = max(eg, (np.abs(r["g_bar"][k] - gb) / np.maximum(1.0, np.abs(gb))).max())
            ecb = max(ecb, (np.abs(r["c_bar"][k] - cb) / np.maximum(1.0, np.abs(cb))).max())
        report("%-16s g_bar err %.1e  c_bar err %.1e" % (s["name"], eg, ecb))
        assert eg <= 1e-9 and ecb <= 1e-9, (s["name"], eg, ecb)


def test_consistency_with_the_division_form_count(ctx, solved):
    """at s = s* (1 +- 1e-6) the library's own exact count of the rows (g, s c, 1) at shift 0 reads >= 1 / 0.  That count is exact for
    rows a few ulp away, i.e. for a scale within a few eps normT / kappa = a few u / N of the one asked for: every system on which
    64 u / N is below a tenth of the step is checked -- all but N = 65,535, where u / N is 2e-6 s*."""
    seen = []
    for s in solved:
        ref_s = np.array([q["scale"] for q in s["ref"]]); u = np.array([q["u"] for q in s["ref"]])
        if not (64 * u / s["g"].shape[1] < 1e-7 * ref_s).all():
            seen.append(s["name"])
            continue
        sc = s["gpu"]["scale"]
        one = np.ones_like(s["g"]); z = np.zeros(len(sc))
        up = ctx.sturm_count(s["h"], s["g"], (sc * (1 + 1e-6))[:, None] * s["c"], one, z, exact=True)
        dn = ctx.sturm_count(s["h"], s["g"], (sc * (1 - 1e-6))[:, None] * s["c"], one, z, exact=True)
        assert (up >= 1).all() and (dn == 0).all(), (s["name"], up, dn)
    assert seen == ["s-alpha N=65535"], seen


def test_G2_stability_table(ctx):
    """(scale < 1) == the reference's verdict (bishop_ball_s-alpha.py), all 240 rows of the 401-point column"""
    tab = np.load(os.path.join(G, "G2_salpha_stability.npz"))["table"]
    th = np.linspace(-20 * np.pi, 20 * np.pi, 401)
    gc = [bo.salpha_gc(th, row[0], row[1], row[2]) for row in tab]
    r = ctx.marginal_gcf(th[1] - th[0], np.stack([a for a, _ in gc]), np.stack([b for _, b in gc]), want_info=True)
    assert r["nbad"] == 0 and not (r["info"] >> 16).any()
    assert ((r["scale"] < 1).astype(int) == tab[:, 4].astype(int)).all()
    report("G2 N=401: 240 verdicts reproduced; s* in [%.3f, %.3f], min |s* - 1| %.1e" % (r["scale"].min(), r["scale"].max(),
                                                                                          np.abs(r["scale"] - 1).min()))


def test_G3_ncsx_scan(ctx):
    """marginal_scan on the reference's NCSX lines (N = 513, 16 lines x 4 theta0) against the oracle: scale to 4 u, the theta0 and
    dPdrho derivatives to 1e-9 relative to max(1, |.|); no status bit"""
    g3 = np.load(os.path.join(G, "G3_ncsx_lines.npz"))
    geo = g3["geo_513"]
    th = bo.theta_grid(513)
    h = th[1] - th[0]
    geo7 = [np.ascontiguousarray(geo[:, k, :]) for k in range(7)]
    t0 = np.array([0.0, 0.5, 1.0, 0.5 * np.pi])
    dP = g3["dPdrho_513"]
    r = ctx.marginal_scan(h, *geo7, dP, t0, want_grad=True, want_info=True)
    ref = mo.scan(h, geo7, dP, t0, want_grad=True)
    assert r["nbad"] == 0 and not (r["info"] >> 16).any()
    err = np.abs(r["scale"] - ref["scale"]) / ref["u"]
    rel = lambda a, b: (np.abs(a - b) / np.maximum(1.0, np.abs(b))).max()
    e_t, e_p = rel(r["dscale_dtheta0"], ref["dscale_dtheta0"]), rel(r["dscale_ddPdrho"], ref["dscale_ddPdrho"])
    report("G3 N=513 scan: s* in [%.3f, %.3f]  max |s - s_oracle| / u %.2e  dscale_dtheta0 err %.1e  dscale_ddPdrho err %.1e  passes %.1f"
           % (r["scale"].min(), r["scale"].max(), err.max(), e_t, e_p, (r["info"] & 0xffff).mean()))
    assert (err <= 4).all()
    assert (np.abs(r["mu"] * ref["scale"] - 1) <= 4 * ref["u"] / ref["scale"] + 4e-16).all()
    assert e_t <= 1e-9 and e_p <= 1e-9


def test_infinite_margin_and_invalid_data(ctx):
    """c <= 0 everywhere: scale = inf, mu = 0, status bit 8, not counted; a NaN in g: status bit 1, scale = NaN, counted"""
    N = 129
    th = bo.theta_grid(N)
    g, c = bo.salpha_gc(th, 1.0, 0.8, 0.3)
    G3 = np.stack([g, g, g]); C3 = np.stack([c, -np.abs(c), c])
    r = ctx.marginal_gcf(th[1] - th[0], G3, C3, want_X=True, want_grad=True, want_info=True)
    assert r["nbad"] == 0
    assert list(r["info"] >> 16) == [0, 256, 0]
    assert np.isinf(r["scale"][1]) and r["scale"][1] > 0 and r["mu"][1] == 0.0
    assert (r["g_bar"][1] == 0).all() and (r["c_bar"][1] == 0).all() and np.isnan(r["X"][1]).all()
    assert r["scale"][0] == r["scale"][2] and np.isfinite(r["scale"][0])
    G3[2, 40] = np.nan
    r = ctx.marginal_gcf(th[1] - th[0], G3, C3, want_X=True, want_grad=True, want_info=True)
    assert r["nbad"] == 1
    assert list(r["info"] >> 16) == [0, 256, 2]
    assert np.isnan(r["scale"][2]) and np.isnan(r["mu"][2]) and np.isnan(r["g_bar"][2]).all()
    geo7 = [np.ones((1, N)), np.ones((1, N)), c[None], np.zeros((1, N)), g[None], np.zeros((1, N)), np.zeros((1, N))]
    r = ctx.marginal_scan(th[1] - th[0], *geo7, np.array([0.0]), np.array([0.0]), want_grad=True, want_info=True)       # dPdrho = 0: c = 0
    assert r["nbad"] == 0 and int(r["info"][0, 0] >> 16) == 256 and np.isinf(r["scale"][0, 0]) and r["mu"][0, 0] == 0.0
    assert r["dscale_dtheta0"][0, 0] == 0.0 and r["dscale_ddPdrho"][0, 0] == 0.0


def test_repeatability(ctx):
    """a batch of 1 and of 300 copies, host pointers and device pointers: bitwise equal"""
    import torch
    N = 387
    th = ec.theta_grid(N)
    g, c, _ = ec.well_rows(th, 200)
    h = th[1] - th[0]
    keys = ("scale", "mu", "X", "gam0", "g_bar", "c_bar", "info")
    one = ctx.marginal_gcf(h, g[None], c[None], want_X=True, want_grad=True, want_info=True)
    many = ctx.marginal_gcf(h, np.tile(g, (300, 1)), np.tile(c, (300, 1)), want_X=True, want_grad=True, want_info=True)
    for k in keys:
        assert (many[k] == one[k][0]).all(), k
    dev = torch.device("cuda:0")
    d = ctx.marginal_gcf(h, torch.from_numpy(np.tile(g, (300, 1))).to(dev), torch.from_numpy(np.tile(c, (300, 1))).to(dev),
                         want_X=True, want_grad=True, want_info=True)
    for k in keys:
        assert (d[k].cpu().numpy() == many[k]).all(), k
    assert ctx.last_launch()[0] == "ibs::k_marginal_gcf"


def test_autograd_marginal_scale(ctx):
    """ibs_amd.autograd.marginal_scale against central differences of its own forward along random directions: one N = 67 system,
    step 1e-6, 1e-5 relative"""
    import torch
    from ibs_amd import autograd as iag
    dev = torch.device("cuda:0")
    N = 67
    th = bo.theta_grid(N)
    h = th[1] - th[0]
    g0, c0 = bo.salpha_gc(th, 1.0, 0.8, 0.3)
    g = torch.from_numpy(g0[None]).to(dev).requires_grad_(True)
    c = torch.from_numpy(c0[None]).to(dev).requires_grad_(True)
    s = iag.marginal_scale(h, g, c, ctx=ctx)
    (3.0 * s.sum()).backward()
    rng = np.random.default_rng(7)
    step = 1e-6
    for _ in range(3):
        dg = torch.from_numpy(rng.standard_normal((1, N))).to(dev); dc = torch.from_numpy(rng.standard_normal((1, N))).to(dev)
        with torch.no_grad():
            sp = iag.marginal_scale(h, g + step * dg, c + step * dc, ctx=ctx)
            sm = iag.marginal_scale(h, g - step * dg, c - step * dc, ctx=ctx)
        fd = 3.0 * float((sp - sm).sum()) / (2 * step)
        an = float((g.grad * dg).sum() + (c.grad * dc).sum())
        assert abs(fd - an) <= 1e-5 * abs(fd), (fd, an)


def test_marginal_dPdrho_drop_in(ctx):
    g3 = np.load(os.path.join(G, "G3_ncsx_lines.npz"))
    import ibs_amd
    th = bo.theta_grid(513)
    bmag, gp, cv, cv0, gd2, gd21, gd22, gb = g3["geo_513"][3]
    dP = float(g3["dPdrho_513"][3])
    crit, s, X = ibs_amd.marginal_dPdrho(dP, th, bmag, gp, cv, gd2, ctx=ctx)
    q = mo.solve(th[1] - th[0], *bo.gcf(dP, bmag, gp, cv, gd2)[:2])
    assert abs(s - q["scale"]) <= 4 * q["u"] and crit == s * dP
    assert np.abs(X - q["X"]).max() <= max(1e-8, 2 * 513 * mo.EPS * q["normT"] / top_gap(q))      # (as test_marginal_mode)


def test_scan_driver_marginal_on_ncsx_tables(ctx):
    """BallooningScan.marginal() on the G8 tables (2 surfaces, 8 x 5 coarse grid, N = 969): the device-resident branch against the
    host branch -- the same location, |delta s*| <= 4 u of the line the minimum sits on"""
    import torch
    import ibs_amd
    N = 969
    th = np.linspace(-4 * np.pi, 4 * np.pi, N)
    svals = np.array([0.6, 0.9])
    tabs = ibs_amd.SurfaceTables.from_wout(dict(np.load(os.path.join(G, "G8_wout_ncsx_op.npz"))), svals)
    kw = dict(nalpha=8, ntheta0=5)
    res = ibs_amd.BallooningScan(ctx, None, th, svals, tables=tabs, device=torch.device("cuda:0"), **kw).marginal()
    host_scan = ibs_amd.BallooningScan(ctx, None, th, svals, tables=tabs, **kw)
    host = host_scan.marginal()
    assert (res["index"] == host["index"]).all(), (res["index"], host["index"])
    assert (res["alpha"] == host["alpha"]).all() and (res["theta0"] == host["theta0"]).all()
    for k, s in enumerate(svals):
        ln = host_scan.fieldlines(s, np.array([host["alpha"][k]]))[0]
        q = mo.solve(host_scan.h, *mo.line_gc(bo.dPdrho_of(ln[2], ln[7], ln[0]), *ln[:7], host["theta0"][k]))
        assert abs(res["scale"][k] - host["scale"][k]) <= 4 * q["u"], (k, res["scale"][k], host["scale"][k], q["u"])
        assert abs(host["scale"][k] - q["scale"]) <= 4 * q["u"]
    report("G8 N=969 marginal(): s* per surface %s at (alpha, theta0) %s" % (host["scale"], list(zip(host["alpha"], host["theta0"]))))
