"""GPU: the geometry-fed Sturm count (ibs_geo_sturm_count_f64), the count-pair certificate of geometry-fed growth rates
(ibs_gamma_scan_certify_f64 / ibs_gamma_points_certify_f64), the re-close (ibs_gamma_*_reclose_f64) and certify=True through
Context.gamma_scan, BallooningScan and AdjointStep -- against the C oracle on host-folded rows (tests/certify_oracle.py)."""
import os

import numpy as np
import pytest

from oracle import ballooning_oracle as bo
from oracle import c_oracle as co
from tests import certify_oracle as cz

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def ctx():
    import ibs_amd
    c = ibs_amd.Context(0)
    yield c
    c.close()


def dev_of(arrs):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in arrs]


_BATCH = {}


def salpha_batch(nl, nt, N):
    """nl s-alpha lines as geometry with their theta0 planes x nt theta0 values, the host-folded rows, the oracle's lam_max, gam
    and the tolerance 4 N eps ||A|| of every system (computed once per shape)"""
    key = (nl, nt, N)
    if key not in _BATCH:
        th = np.linspace(-4 * np.pi, 4 * np.pi, N)
        h = th[1] - th[0]
        geo7, dP = cz.salpha_geometry(th, np.linspace(0.3, 2.0, nl), np.linspace(1.5, 0.4, nl))
        t0 = np.linspace(0.0, 0.5 * np.pi, nt)
        g, c, f = cz.fold_rows(geo7, dP, t0)
        if N % 2:
            gam, lam, _ = co.solve_gcf_batch(h, g, c, f)
        else:
            gam, lam = None, co.lam_batch(h, g, c, f)
        _BATCH[key] = dict(th=th, h=h, geo7=geo7, dP=dP, t0=t0, g=g, c=c, f=f, lam=lam, gam=gam, tol=cz.tolerance(h, g, c, f))
    return _BATCH[key]


@pytest.mark.parametrize("N", [67, 129, 131, 512, 513, 1025, 2049, 2051, 2561])
@pytest.mark.parametrize("nl,nt", [(5, 3), (9, 15)])
def test_count_parity(ctx, nl, nt, N):
    """the geometry-fed count equals the C oracle's division-form count on the host-folded rows, exactly, at shift 0 and at
    lam_oracle +- 4 N eps ||A||: 5 x 3 (a partial wave) and 9 x 15 (lines straddling waves); 512: even N, the count only"""
    b = salpha_batch(nl, nt, N)
    d7, (dP, t0) = dev_of(b["geo7"]), dev_of([b["dP"], b["t0"]])
    for shift in (np.zeros(nl * nt), b["lam"] + b["tol"], b["lam"] - b["tol"]):
        ref = co.count_above_batch(b["h"], b["g"], b["c"], b["f"], shift)
        cnt = ctx.geo_sturm_count(b["h"], *d7, dP, t0, dev_of([shift.reshape(nl, nt)])[0])
        assert "k_geo_certify<0" in ctx.last_launch()[0]
        assert np.array_equal(cnt.cpu().numpy().reshape(-1), ref), (shift[:4], cnt.cpu().numpy().reshape(-1)[:8], ref[:8])
    assert (co.count_above_batch(b["h"], b["g"], b["c"], b["f"], b["lam"] + b["tol"]) == 0).all()
    # host pointers, a scalar shift
    cnt_h = ctx.geo_sturm_count(b["h"], *b["geo7"], b["dP"], b["t0"], 0.0)
    assert np.array_equal(cnt_h.reshape(-1), co.count_above_batch(b["h"], b["g"], b["c"], b["f"], np.zeros(nl * nt)))


@pytest.mark.parametrize("which,N,extent", [(3, 1601, 61), (4, 401, 20)])
def test_count_reproduces_the_reference_stability_table(ctx, which, N, extent):
    """count(0) > 0 equals every stored boolean of G2 (bishop_ball_s-alpha.py:110-115), the s-alpha rows as geometry with
    B = gradpar = 1 and f = g: 240 lines x 1 theta0"""
    tab = np.load(os.path.join(G, "G2_salpha_stability.npz"))["table"]
    th = np.linspace(-extent * np.pi, extent * np.pi, N)
    g = np.empty((len(tab), N)); c = np.empty_like(g)
    for k, row in enumerate(tab):
        g[k], c[k] = bo.salpha_gc(th, row[0], row[1], row[2])
    one, z = np.ones_like(g), np.zeros_like(g)
    cnt = ctx.geo_sturm_count(th[1] - th[0], one, one, c, z, g, z, z, -np.ones(len(tab)), np.zeros(1))
    assert ((cnt[:, 0] > 0).astype(int) == tab[:, which].astype(int)).all()


@pytest.mark.parametrize("N", [131, 513, 1025])
def test_decisions_on_prepared_lam(ctx, N):
    """lam_max -> 0, the oracle's lam_2 -> bit 0, lam_max + 10 tol -> bit 1, NaN -> bit 2, mixed within every wave of the 9 x 15 batch
    (scan form) and of its first 64 + 7 systems as points; equal to the oracle's rule on every system, through device and host
    pointers"""
    b = salpha_batch(9, 15, N)
    n = 9 * 15
    lam = b["lam"].copy()
    want = np.zeros(n, dtype=np.int32)
    for k in range(n):
        m = k % 4
        if m == 1:
            lam[k] = cz.second_eigenvalue(b["h"], b["g"][k], b["c"][k], b["f"][k], b["lam"][k], b["tol"][k]); want[k] = cz.NOT_MAX
        elif m == 2:
            lam[k] = b["lam"][k] + 10 * b["tol"][k]; want[k] = cz.NO_EIG
        elif m == 3:
            lam[k] = np.nan; want[k] = cz.UNCHECKED
    assert np.array_equal(cz.cert_rule(b["h"], b["g"], b["c"], b["f"], lam), want)
    d7, (dP, t0, dl) = dev_of(b["geo7"]), dev_of([b["dP"], b["t0"], lam.reshape(9, 15)])
    cert = ctx.certify_scan(b["h"], *d7, dP, t0, dl)
    assert "k_geo_certify<1" in ctx.last_launch()[0]
    assert np.array_equal(cert.cpu().numpy().reshape(-1), want)
    # the points form: line k // 15 at its own theta0
    npt = 71
    line, it0 = np.arange(npt) // 15, np.arange(npt) % 15
    p7 = [a[line] for a in b["geo7"]]
    cp = ctx.certify_points(b["h"], *dev_of(p7), *dev_of([b["dP"][line], b["t0"][it0], lam[:npt]]))
    assert np.array_equal(cp.cpu().numpy(), want[:npt])
    # host pointers: the same words
    ch = ctx.certify_scan(b["h"], *b["geo7"], b["dP"], b["t0"], lam.reshape(9, 15))
    assert np.array_equal(ch.reshape(-1), want)
    ch2 = ctx.certify_points(b["h"], *p7, b["dP"][line], b["t0"][it0], lam[:npt])
    assert np.array_equal(ch2, want[:npt])
    # a wider tolerance takes the lam_max + 10 tol entries in
    c16 = ctx.certify_scan(b["h"], *d7, dP, t0, dl, tol_factor=64.0).cpu().numpy().reshape(-1)
    assert (c16[2::4] == 0).all() and (c16[0::4] == 0).all()


def test_g10_through_certified_scan(ctx):
    """the near-degenerate pair of G10 mapped onto geometry arrays, through gamma_scan(certify=True): lam within 4 N eps ||A|| of
    lam_max and cert 0 or 8 (lam only: gam is not pinned on rough systems)"""
    d = np.load(os.path.join(G, "G10_rough_pair_1025.npz"))
    N = 1025
    h = 8 * np.pi / (N - 1)
    geo7, dP = cz.gcf_to_geometry(d["g"], d["c"], d["f"])
    g, c, f = cz.fold_rows(geo7, dP, np.zeros(1))
    tol = cz.tolerance(h, g, c, f)[0]
    for arrs in (geo7 + [dP, np.zeros(1)], dev_of(geo7 + [dP, np.zeros(1)])):
        r = ctx.gamma_scan(h, *arrs, certify=True)
        lam = float(r["lam"].reshape(-1)[0]); cert = int(r["cert"].reshape(-1)[0])
        print("G10 through gamma_scan(certify=True): cert = %d, lam - lam_max = %.2e (tol %.2e)" % (cert, lam - float(d["lam_max"]), tol))
        assert abs(lam - float(d["lam_max"])) <= tol, (lam, float(d["lam_max"]), tol)
        assert cert in (0, cz.RECLOSED)


def test_reclose_alone(ctx):
    """9 x 15 at N = 513: lam and gam of systems 0, 63, 64 and the last one are overwritten and marked with bit 0; after the
    re-close those four match the oracle (gam 1e-10, lam 4 N eps ||A||) with cert 8, every other entry of cert, lam, gam, X, dX is
    unchanged bit for bit; the same through host pointers"""
    import torch
    b = salpha_batch(9, 15, 513)
    n = 9 * 15
    hit = np.array([0, 63, 64, n - 1])
    d7, (dP, t0) = dev_of(b["geo7"]), dev_of([b["dP"], b["t0"]])
    r = ctx.gamma_scan(b["h"], *d7, dP, t0, want_X=True)
    keep = {k: r[k].clone() for k in ("lam", "gam", "X", "dX")}
    cert = torch.zeros((9, 15), dtype=torch.int32, device="cuda:0")
    for k in hit:
        i, j = divmod(int(k), 15)
        r["lam"][i, j] -= 1.0; r["gam"][i, j] = 123.0; r["X"][i, j] = 7.0; cert[i, j] = cz.NOT_MAX
    host = {k: r[k].cpu().numpy().copy() for k in ("lam", "gam", "X", "dX")}
    hcert = cert.cpu().numpy().copy()
    assert ctx.reclose_scan(b["h"], *d7, dP, t0, cert, r["lam"], r["gam"], r["X"], r["dX"]) == 0
    assert "k_geo_certify<1" in ctx.last_launch()[0]
    nf = ctx.reclose_scan(b["h"], *b["geo7"], b["dP"], b["t0"], hcert, host["lam"], host["gam"], host["X"], host["dX"])
    assert nf == 0
    for lam, gam, X, dX, cw in ((r["lam"].cpu().numpy(), r["gam"].cpu().numpy(), r["X"].cpu().numpy(), r["dX"].cpu().numpy(),
                                 cert.cpu().numpy()), (host["lam"], host["gam"], host["X"], host["dX"], hcert)):
        lam, gam, cw = lam.reshape(-1), gam.reshape(-1), cw.reshape(-1)
        assert (cw[hit] == cz.RECLOSED).all(), cw[hit]
        assert (np.abs(lam[hit] - b["lam"][hit]) <= b["tol"][hit]).all()
        assert np.abs(gam[hit] - b["gam"][hit]).max() < 1e-10, np.abs(gam[hit] - b["gam"][hit])
        rest = np.setdiff1d(np.arange(n), hit)
        assert (cw[rest] == 0).all()
        assert np.array_equal(lam[rest], keep["lam"].cpu().numpy().reshape(-1)[rest])
        assert np.array_equal(gam[rest], keep["gam"].cpu().numpy().reshape(-1)[rest])
        assert np.array_equal(X.reshape(n, -1)[rest], keep["X"].cpu().numpy().reshape(n, -1)[rest])
        assert np.array_equal(dX.reshape(n, -1)[rest], keep["dX"].cpu().numpy().reshape(n, -1)[rest])
        # the re-closed eigenfunctions: normalised, zero ends, close to the scan's own
        Xh, Xk = X.reshape(n, -1)[hit], keep["X"].cpu().numpy().reshape(n, -1)[hit]
        assert np.abs(Xh - Xk).max() < 1e-6 and (Xh[:, 0] == 0).all() and (Xh[:, -1] == 0).all()
    # an uncheckable entry (bit 2) and a certified one are left alone; a system that cannot be re-closed keeps its bits
    c2 = torch.zeros(n, dtype=torch.int32, device="cuda:0"); c2[5] = cz.UNCHECKED
    l2, g2 = keep["lam"].clone(), keep["gam"].clone()
    ctx.reclose_scan(b["h"], *d7, dP, t0, c2.view(9, 15), l2, g2)
    assert int(c2[5]) == cz.UNCHECKED and torch.equal(l2, keep["lam"]) and torch.equal(g2, keep["gam"])


def test_rough_family_mapped(ctx):
    """the rough family of BASELINE configs[4] (iid per point inside the NCSX_op envelopes) mapped onto geometry arrays with small
    positive theta0 planes: 512 lines x 4 theta0, N = 513.  After gamma_scan(certify=True) every lam lies within 4 N eps ||A|| of the C
    oracle's and no system is left open."""
    import torch
    from bench import c5_family
    N, nl = 513, 512
    h, g, c, f = c5_family(torch.device("cuda:0"), "rough", nl, N, seed=20240 + 512)
    geo7, dP = cz.gcf_to_geometry(g.cpu().numpy(), c.cpu().numpy(), f.cpu().numpy(), th0_planes=1e-3, seed=3)
    t0 = np.linspace(0.0, 0.3, 4)
    gg, cc, ff = cz.fold_rows(geo7, dP, t0)
    lam_o = co.lam_batch(h, gg, cc, ff)
    tol = cz.tolerance(h, gg, cc, ff)
    r = ctx.gamma_scan(h, *dev_of(geo7), *dev_of([dP, t0]), want_info=True, certify=True)
    cert = r["cert"].cpu().numpy().reshape(-1)
    lam = r["lam"].cpu().numpy().reshape(-1)
    print("rough family, 512 x 4 at N = 513: %d of %d re-closed, %d left open; max |lam - oracle| / tol = %.3f"
          % (int((cert == cz.RECLOSED).sum()), cert.size, int(((cert & 7) != 0).sum()), float((np.abs(lam - lam_o) / tol).max())))
    assert int(((cert & 7) != 0).sum()) == 0
    assert (np.abs(lam - lam_o) <= tol).all(), float((np.abs(lam - lam_o) / tol).max())
    assert np.isin(cert, (0, cz.RECLOSED)).all()


def test_physical_near_degenerate_lines(ctx):
    """(shat, alpha) = (2, 6) and (12, 1), theta0 in {0, 1e-3, 0.05}, N = 513: near-degenerate even / odd pairs on smooth lines.
    gam against the oracle to 1e-8, cert 0 or 8."""
    N = 513
    th = bo.theta_grid(N)
    h = th[1] - th[0]
    geo7, dP = cz.salpha_geometry(th, [2.0, 12.0], [6.0, 1.0])
    t0 = np.array([0.0, 1e-3, 0.05])
    g, c, f = cz.fold_rows(geo7, dP, t0)
    gam_o, lam_o, _ = co.solve_gcf_batch(h, g, c, f)
    tol = cz.tolerance(h, g, c, f)
    for arrs in (dev_of(geo7 + [dP, t0]), geo7 + [dP, t0]):
        r = ctx.gamma_scan(h, *arrs, certify=True)
        to_np = lambda a: a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
        gam, lam, cert = (to_np(r[k]).reshape(-1) for k in ("gam", "lam", "cert"))
        print("near-degenerate s-alpha lines: cert =", cert, " |gam - oracle| =", np.abs(gam - gam_o))
        assert np.isin(cert, (0, cz.RECLOSED)).all(), cert
        assert (np.abs(lam - lam_o) <= tol).all()
        assert np.abs(gam - gam_o).max() < 1e-8, np.abs(gam - gam_o)


def wout_scaled(factor):
    w = dict(np.load(os.path.join(G, "G8_wout_ncsx_op.npz")))
    w["pres"] = np.asarray(w["pres"], dtype=np.float64) * factor
    return w


SVALS = np.array([0.6, 0.95])
KW = dict(nalpha=8, ntheta0=5)


def test_workflow_scan(ctx):
    """BallooningScan on the G8 NCSX tables with the pressure x 6, N = 513, 2 surfaces x 8 alpha x 5 theta0: certify=True rows within
    1e-8 of the certify=False rows; 2 * 8 * 5 + 2 eigenvalues checked, none failed; mode_count() of one surface equals the oracle's
    counts on the geometry oracle's lines; BallooningScan() and BallooningScan(certify=False) agree bitwise"""
    import torch
    import ibs_amd
    from oracle import geometry_oracle as go
    dev = torch.device("cuda:0")
    N = 513
    th = np.linspace(-4 * np.pi, 4 * np.pi, N)
    w = wout_scaled(6.0)
    tabs = ibs_amd.SurfaceTables.from_wout(w, SVALS)
    plain = ibs_amd.BallooningScan(ctx, None, th, SVALS, tables=tabs, device=dev, **KW)
    rows0 = plain.run()
    off = ibs_amd.BallooningScan(ctx, None, th, SVALS, tables=tabs, device=dev, certify=False, **KW)
    rows1 = off.run()
    for a, b_ in zip(rows0, rows1):
        assert np.array_equal(a, b_)
    assert plain.last_certificate is None
    cs = ibs_amd.BallooningScan(ctx, None, th, SVALS, tables=tabs, device=dev, certify=True, **KW)
    rows2 = cs.run()
    print("BallooningScan(certify=True), NCSX_op pressure x 6, N = 513:", cs.last_certificate)
    assert np.abs(rows2[2] - rows0[2]).max() < 1e-8, (rows2[2], rows0[2])
    assert np.abs(rows2[0] - rows0[0]).max() < 1e-8 and np.abs(rows2[1] - rows0[1]).max() < 1e-8
    assert cs.last_certificate["checked"] == 2 * 8 * 5 + 2 and cs.last_certificate["failed"] == 0
    # the unstable-mode table of the second surface against the oracle on the geometry oracle's lines
    cnt = cs.mode_count()
    assert cnt.shape == (2, 8, 5) and cnt.dtype == np.int32
    ref = go.fieldline_geometry(go.surface_tables_from_wout(w, SVALS[1:2]), 0, cs.alpha_scan, th)
    dP = np.array([bo.dPdrho_of(ln[2], ln[7], ln[0]) for ln in ref])
    g, c, f = cz.fold_rows([ref[:, k] for k in range(7)], dP, cs.theta0_scan)
    assert np.array_equal(cnt[1].reshape(-1), co.count_above_batch(th[1] - th[0], g, c, f, np.zeros(len(g))))
    assert cnt.max() >= 1                                   # (pressure x 6: unstable lines exist)
    # the host-callable path certifies too
    hs = ibs_amd.BallooningScan(ctx, None, th, SVALS[:1], tables=tabs, certify=True, nalpha=4, ntheta0=3)
    hs.run()
    assert hs.last_certificate["checked"] == 4 * 3 + 1 and hs.last_certificate["failed"] == 0


def test_workflow_adjoint_step(ctx):
    """AdjointStep(certify=True), 3 equilibria x 2 surfaces, N = 513: the result of certify=False to 1e-8, the counts summed"""
    import torch
    import ibs_amd
    import bench
    dev = torch.device("cuda:0")
    w6 = wout_scaled(6.0)
    wouts = [w6, wout_scaled(3.0), bench.emulated_equilibria(w6)[0][1]]
    steps = np.array([1.0, 1e-3, 2e-3])
    f_other = np.array([0.8, 0.81, 0.82])
    th = np.linspace(-4 * np.pi, 4 * np.pi, 513)
    kw = dict(gamma_thresh=-2.0e-4, prefac=50.0, **KW)
    a0 = ibs_amd.AdjointStep(ctx, th, SVALS, dev, **kw)
    o0 = a0.run(wouts, f_other, steps)
    a1 = ibs_amd.AdjointStep(ctx, th, SVALS, dev, certify=True, **kw)
    o1 = a1.run(wouts, f_other, steps)
    print("AdjointStep(certify=True), 3 equilibria x 2 surfaces:", a1.last_certificate)
    assert a0.last_certificate is None
    assert a1.last_certificate["checked"] == 3 * (2 * 8 * 5 + 2) and a1.last_certificate["failed"] == 0
    for key in ("gam", "theta0", "alpha"):
        assert np.abs(o1[key] - o0[key]).max() < 1e-8, (key, o1[key], o0[key])
    # what 1e-8 on each of the two growth rates of an equilibrium can move: f0 by prefac * 2e-8, a gradient entry by twice that over
    # its step and 2 sqrt(f0) (sims_runner_NCSX.py:254-261)
    df0 = 50.0 * 2 * 1e-8
    assert np.abs(o1["f0"] - o0["f0"]).max() <= df0
    assert np.abs(o1["dfobj"] - o0["dfobj"]).max() <= 2 * df0 / np.abs(steps[1:]).min() / (2 * np.sqrt(o0["f0"].min()))
