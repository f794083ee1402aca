"""GPU: the local-equilibrium scan (ibs_local_eq_scan_f64, csrc/ibs_local_eq.hip; Context.local_eq_scan, BallooningScan.local_eq) against
the rule in numpy (ibs_amd.operators.local_eq_fold) + the CPU oracles (tests/local_eq_cases.py).

Tolerances, the project's own: |gam - gam_oracle| <= 1e-8; |lam - lam_oracle| <= 4 N eps ||A||; counts exact, every count compared at a
fixed shift on a system with |lam_max - shift| > 16 N^2 eps ||A|| (asserted on the oracle side).  The counts at lam_oracle +- 8 N eps ||A||
are the count-pair certificate of the eigenvalue: 0 above, at least 1 below -- what the lam tolerance itself implies.

Tests 9-12 run the kernel where a wave serves more than one system (the persistent grid of 8 waves per CU: the batch is sized from the
device's CU count, and Context.last_launch must report fewer blocks than systems), on padded rows through the raw entry point, on the
branches of the rule and under the wave cap of the workspace budget."""
import itertools
import os

import numpy as np
import pytest

from oracle import ballooning_oracle as bo
from tests import local_eq_cases as lc

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(__file__), "golden")
EPS = lc.EPS


@pytest.fixture(scope="module")
def ctx():
    import ibs_amd
    return ibs_amd.Context(0)


@pytest.fixture(scope="module")
def g3():
    return np.load(os.path.join(G, "G3_ncsx_lines.npz"))


@pytest.fixture(scope="module")
def g8():
    return dict(np.load(os.path.join(G, "G8_surface_tables.npz")))


def status(r):
    return np.asarray(r["info"]) >> 16


def check_against_oracle(r, ref, what, count0=None):
    """gam, lam (and the counts at shift 0) of a clean result against oracle_of / counts_of; prints the figures first"""
    e_gam = np.abs(r["gam"] - ref["gam"]).max()
    e_lam = (np.abs(r["lam"] - ref["lam"]) / ref["tol_lam"]).max()
    print("%s: max |gam - oracle| %.2e, max |lam - oracle| / (4 N eps ||A||) %.2e" % (what, e_gam, e_lam))
    assert not status(r).any(), status(r)
    assert e_gam <= 1e-8 and e_lam <= 1.0, (what, e_gam, e_lam)
    if count0 is not None:
        assert (np.abs(ref["lam"]) > ref["margin"]).all(), (what, (np.abs(ref["lam"]) / ref["margin"]).min())
        assert np.array_equal(r["count"], count0), what


def test_identity_plane_is_the_theta0_scan(ctx, g3):
    """1. eps = 0, p = 1, no ps on the 16 golden NCSX lines at N = 513 with the fixture's four theta0: gam within 1e-8 of the tight
    golden growth rates and of Context.gamma_scan"""
    lines = g3["geo_513"]
    th = bo.theta_grid(513)
    h = th[1] - th[0]
    t0 = g3["theta0"]
    var = np.stack([t0, np.zeros(4), np.ones(4)], axis=1)
    r = ctx.local_eq_scan(th[0], h, lc.to_geo(lines), g3["dPdrho_513"], g3["lines_513"][:, 1], np.ones(16), var, want_info=True)
    assert "k_local_eq_scan" in ctx.last_launch()[0], ctx.last_launch()
    sc = ctx.gamma_scan(h, *[np.ascontiguousarray(lines[:, k]) for k in range(7)], g3["dPdrho_513"], t0)
    e_gold, e_scan = np.abs(r["gam"] - g3["gam_tight_513"]).max(), np.abs(r["gam"] - sc["gam"]).max()
    print("identity plane: max |gam - golden| %.2e, max |gam - gamma_scan| %.2e" % (e_gold, e_scan))
    assert r["nbad"] == 0 and not status(r).any()
    assert e_gold <= 1e-8 and e_scan <= 1e-8


def test_ncsx_variations_against_the_oracle(ctx, g3, g8):
    """2. the four golden NCSX lines at N = 969, theta0 in {0, 0.5} x eps in {-0.5, 0.3, 1} x p in {0, 0.5, 1.7}: gam, lam, the count at
    shift 0, and the count pair at the oracle's lam +- 8 N eps ||A|| of every system"""
    N = 969
    lines, dP, alpha = g3["geo_969"], g3["dPdrho_969"], g3["lines_969"][:, 1]
    sigma = np.full(4, float(np.sign(-g8["phiedge"])))
    th = bo.theta_grid(N)
    h = th[1] - th[0]
    var = np.array(list(itertools.product((0.0, 0.5), (-0.5, 0.3, 1.0), (0.0, 0.5, 1.7))))
    g, c, f = lc.rows_of(th, lines, dP, alpha, sigma, var)
    ref = lc.oracle_of(th, g, c, f)
    geo = lc.to_geo(lines)
    r = ctx.local_eq_scan(th[0], h, geo, dP, alpha, sigma, var, shift=0.0, want_info=True)
    check_against_oracle(r, ref, "NCSX N=969, 72 systems", lc.counts_of(th, g, c, f, 0.0))
    d = 8 * N * EPS * ref["normA"]
    for i in range(4):
        one = np.ascontiguousarray(geo[:, i:i + 1])
        for k in range(len(var)):
            args = (th[0], h, one, dP[i:i + 1], alpha[i:i + 1], sigma[i:i + 1], var[k:k + 1])
            above = ctx.local_eq_scan(*args, shift=ref["lam"][i, k] + d[i, k], count_only=True)["count"][0, 0]
            below = ctx.local_eq_scan(*args, shift=ref["lam"][i, k] - d[i, k], count_only=True)["count"][0, 0]
            assert above == 0 and below >= 1, (i, k, above, below)


def test_end_to_end_against_the_geometry_of_the_varied_tables(ctx, g8):
    """3. on the device: Context.fieldline_geometry of two G8 surfaces as they are, varied by local_eq_scan, against gamma_scan on the
    geometry of the tables with scal[:, 2] x (1 + eps) and scal[:, 3] x p, N = 513: gam within 1e-8"""
    import torch
    import ibs_amd
    dev = torch.device("cuda:0")
    N = 513
    th = bo.theta_grid(N)
    h = th[1] - th[0]
    surf = np.array([1, 1, 2, 2], dtype=np.int32)
    alpha = np.array([0.0, 1.0, 0.0, 1.0])
    t0 = np.array([0.0, 0.4])
    tabs = ibs_amd.SurfaceTables.from_arrays(g8)
    sigma = np.sign(-tabs.scal[surf, 4])
    base = ctx.fieldline_geometry(tabs, surf, alpha, th, device=dev)
    worst = 0.0
    for eps, p in ((0.3, 1.7), (-0.5, 0.5)):
        var = np.stack([t0, np.full(2, eps), np.full(2, p)], axis=1)
        r = ctx.local_eq_scan(th[0], h, base["geo"], base["dPdrho"], alpha, sigma, var, want_info=True)
        varied = ibs_amd.SurfaceTables.from_arrays(dict(g8, d_iota_d_s=g8["d_iota_d_s"] * (1 + eps), d_pressure_d_s=g8["d_pressure_d_s"] * p))
        q = ctx.fieldline_geometry(varied, surf, alpha, th, device=dev)
        sc = ctx.gamma_scan(h, *[q["geo"][k] for k in range(7)], q["dPdrho"], torch.from_numpy(t0).to(dev), want_info=True)
        assert not (r["info"] >> 16).any().item() and not (sc["info"] >> 16).any().item()
        worst = max(worst, (r["gam"] - sc["gam"]).abs().max().item())
    print("end to end: max |gam(local_eq_scan) - gam(gamma_scan on the varied tables)| %.2e" % worst)
    assert worst <= 1e-8


def test_salpha_diagram_reproduces_the_reference_table(ctx):
    """4. the 240 rows of G2 at N = 401 on +-20 pi as 3 lines x 80 triples with the Pfirsch-Schlueter row, count_only: the booleans of
    check_ball (column 4); gam of the 80 theta0 = 0 rows against the oracle on the analytic rows salpha_gc"""
    tab = np.load(os.path.join(G, "G2_salpha_stability.npz"))["table"]
    N = 401
    th = np.linspace(-20 * np.pi, 20 * np.pi, N)
    h = th[1] - th[0]
    t0s = np.unique(tab[:, 2])
    pairs = sorted({(row[0], row[1]) for row in tab})
    assert len(t0s) == 3 and len(pairs) == 80
    base = [lc.salpha_base_line(th, t0) for t0 in t0s]
    lines = np.stack([b[0] for b in base]); ps = np.stack([b[2] for b in base])
    dP, one = np.full(3, -1.0), np.ones(3)
    var = np.array([(0.0, sh / 1.0 - 1.0, al / 0.5) for sh, al in pairs])
    geo = lc.to_geo(lines)
    r = ctx.local_eq_scan(th[0], h, geo, dP, t0s, one, var, ps=ps, shift=0.0, count_only=True, want_info=True)
    assert set(r) == {"count", "info", "nbad"} and r["nbad"] == 0 and not status(r).any()
    assert (r["info"] & 0xffff == 0).all()                  # no eigenvalue was computed
    index = {pr: k for k, pr in enumerate(pairs)}
    got = np.array([r["count"][list(t0s).index(row[2]), index[(row[0], row[1])]] > 0 for row in tab])
    assert (got != tab[:, 4].astype(bool)).sum() == 0
    rg = ctx.local_eq_scan(th[0], h, geo[:, :1].copy(), dP[:1], t0s[:1], one[:1], var, ps=ps[:1], want_info=True)
    gc = [bo.salpha_gc(th, sh, al, t0s[0]) for sh, al in pairs]
    g = np.stack([a for a, _ in gc])[None]; c = np.stack([b for _, b in gc])[None]
    check_against_oracle(rg, lc.oracle_of(th, g, c, g), "s-alpha N=401, theta0 = 0 rows")


EDGE_VAR = np.array([(0.0, 0.0, 1.6), (0.2, 0.5, 1.6), (0.0, -0.5, 1.2), (0.1, 0.9, 2.2), (0.0, -0.9, 3.0)])


@pytest.mark.parametrize("N", [67, 769, 771, 2049, 2051, 4097, 65537])
def test_grid_length_edges(ctx, N):
    """5. one s-alpha line x 5 triples on the lane, chunk (768 rows: ibs_long.hpp) and path edges; N = 65,537 with 2 triples.  At
    N = 65,537 the count margin 16 N^2 eps ||A|| (~ 400) exceeds every |lam_max|, so by the rule above no count is compared there."""
    th = bo.theta_grid(N)
    line, dP, ps = lc.salpha_base_line(th, 0.1)
    var = EDGE_VAR[:2] if N == 65537 else EDGE_VAR
    args = ([line], np.array([dP]), np.array([0.1]), np.ones(1), var)
    g, c, f = lc.rows_of(th, *args, ps=ps[None])
    r = ctx.local_eq_scan(th[0], th[1] - th[0], lc.to_geo(args[0]), *args[1:], ps=ps[None], shift=0.0, want_info=True)
    check_against_oracle(r, lc.oracle_of(th, g, c, f), "s-alpha edge N=%d" % N, None if N == 65537 else lc.counts_of(th, g, c, f, 0.0))


def ncsx_batch(g3, n_lines=6):
    """six golden NCSX lines at N = 513 with a smooth ps row each and six triples (p = 0 and eps = -1 among them)"""
    th = bo.theta_grid(513)
    lines = np.array(g3["geo_513"][:n_lines])
    k = np.arange(n_lines)[:, None]
    ps = 0.3 * np.sin(th[None] + 0.4 * k) / (1.0 + 0.1 * k)
    var = np.array([(0.0, 0.0, 1.0), (0.3, -1.0, 1.0), (0.0, 0.3, 0.0), (0.5, 0.3, 1.7), (0.2, -0.5, 0.5), (1.0, 1.0, 1.3)])
    return th, lines, g3["dPdrho_513"][:n_lines].copy(), g3["lines_513"][:n_lines, 1].copy(), np.array([1.0, -1.0, 1.0, 1.0, -1.0, 1.0]), ps, var


KEYS = ("gam", "lam", "count", "info")


def test_outputs_do_not_depend_on_the_batch(ctx, g3):
    """6. bitwise: line order reversed, n_var split into two calls, three chunks of whole lines (option nearest_chunk_systems), host
    pointers against device pointers"""
    import torch
    dev = torch.device("cuda:0")
    th, lines, dP, alpha, sigma, ps, var = ncsx_batch(g3)
    lo, h, geo = th[0], th[1] - th[0], lc.to_geo(lines)
    kw = dict(shift=0.0, want_info=True)
    r = ctx.local_eq_scan(lo, h, geo, dP, alpha, sigma, var, ps=ps, **kw)
    assert r["nbad"] == 0 and np.isfinite(r["gam"]).all()
    rev = ctx.local_eq_scan(lo, h, np.ascontiguousarray(geo[:, ::-1]), dP[::-1], alpha[::-1], sigma[::-1], var, ps=ps[::-1], **kw)
    a = ctx.local_eq_scan(lo, h, geo, dP, alpha, sigma, var[:2], ps=ps, **kw)
    b = ctx.local_eq_scan(lo, h, geo, dP, alpha, sigma, var[2:], ps=ps, **kw)
    ctx.set_option("nearest_chunk_systems", 2 * len(var))   # (chunks of two lines: three launches)
    try:
        ch = ctx.local_eq_scan(lo, h, geo, dP, alpha, sigma, var, ps=ps, **kw)
    finally:
        ctx.set_option("nearest_chunk_systems", None)
    d = ctx.local_eq_scan(lo, h, torch.from_numpy(geo).to(dev), torch.from_numpy(dP).to(dev), alpha, sigma, var,
                          ps=torch.from_numpy(ps).to(dev), **kw)
    for k in KEYS:
        assert np.array_equal(rev[k][::-1], r[k]), k
        assert np.array_equal(np.concatenate([a[k], b[k]], axis=1), r[k]), k
        assert np.array_equal(ch[k], r[k]), k
        assert np.array_equal(d[k].cpu().numpy(), r[k]), k


def test_data_faults_are_data(ctx, g3):
    """7. one NaN in gds21 of one line, sigma = 0.5 on another, a NaN eps in one triple: status 2, NaN gam and lam, count -1 on exactly
    those systems, every other system bitwise the clean run's; p = 0 (c = 0) and eps = -1 (no secular term) are valid and match the oracle"""
    th, lines, dP, alpha, sigma, ps, var = ncsx_batch(g3)
    lo, h = th[0], th[1] - th[0]
    kw = dict(shift=0.0, want_info=True)
    clean = ctx.local_eq_scan(lo, h, lc.to_geo(lines), dP, alpha, sigma, var, ps=ps, **kw)
    g, c, f = lc.rows_of(th, lines, dP, alpha, sigma, var, ps=ps)
    assert (c[:, 2] == 0).all()                              # the p = 0 triple
    check_against_oracle(clean, lc.oracle_of(th, g, c, f), "NCSX N=513 with ps, 36 systems", lc.counts_of(th, g, c, f, 0.0))
    bad_lines, bad_sigma, bad_var = lines.copy(), sigma.copy(), var.copy()
    bad_lines[1, 5, 100] = np.nan
    bad_sigma[3] = 0.5
    bad_var[4, 1] = np.nan
    r = ctx.local_eq_scan(lo, h, lc.to_geo(bad_lines), dP, alpha, bad_sigma, bad_var, ps=ps, **kw)
    hit = np.zeros((6, 6), dtype=bool)
    hit[1] = hit[3] = hit[:, 4] = True
    assert r["nbad"] == hit.sum()
    assert (status(r)[hit] == 2).all() and np.isnan(r["gam"][hit]).all() and np.isnan(r["lam"][hit]).all() and (r["count"][hit] == -1).all()
    for k in KEYS:
        assert np.array_equal(r[k][~hit], clean[k][~hit]), k


def test_scan_driver_local_eq_on_ncsx_tables(ctx):
    """8. BallooningScan.local_eq on the G8 wout tables: 2 surfaces, 4 alpha x 3 theta0 x 3 eps x 2 p, N = 513 -- the documented
    shapes, the (eps = 0, p = 1) plane against coarse() within 1e-8, the envelope against the numpy reduction of the table"""
    import torch
    import ibs_amd
    N = 513
    th = np.linspace(-4 * np.pi, 4 * np.pi, N)
    svals = np.array([0.6, 0.9])
    tabs = ibs_amd.SurfaceTables.from_wout(dict(np.load(os.path.join(G, "G8_wout_ncsx_op.npz"))), svals)
    scan = ibs_amd.BallooningScan(ctx, None, th, svals, nalpha=4, ntheta0=3, tables=tabs, device=torch.device("cuda:0"))
    eps, p = np.array([-0.5, 0.0, 0.3]), np.array([1.0, 1.7])
    r = scan.local_eq(eps, p)
    shape = (2, 4, 3, 3, 2)
    assert r["gam"].shape == shape and r["lam"].shape == shape and r["count"].shape == shape and r["count"].dtype == np.int32
    assert r["gam_max"].shape == (2, 3, 2) and r["unstable"].shape == (2, 3, 2) and r["unstable"].dtype == bool
    assert np.array_equal(r["theta0"], scan.theta0_scan) and np.array_equal(r["eps"], eps) and np.array_equal(r["p"], p)
    e = np.abs(r["gam"][:, :, :, 1, 0] - scan.coarse()).max()
    print("BallooningScan.local_eq: max |gam(eps = 0, p = 1) - coarse()| %.2e" % e)
    assert e <= 1e-8
    assert np.array_equal(r["gam_max"], r["gam"].max(axis=(1, 2))) and np.array_equal(r["unstable"], (r["count"] > 0).any(axis=(1, 2)))
    rc = scan.local_eq(eps, p, count_only=True)
    assert "gam" not in rc and np.array_equal(rc["count"], r["count"]) and np.array_equal(rc["unstable"], r["unstable"])
    with pytest.raises(ValueError):
        ibs_amd.BallooningScan(ctx, None, th, svals, nalpha=4, ntheta0=3, tables=tabs).local_eq(eps, p)


# ---- the persistent grid: more systems than waves, faults on a reused wave, padded rows, the rule's branches, the wave cap
@pytest.fixture(scope="module")
def reuse(ctx):
    """9. the batch of tests/local_eq_cases.wave_reuse_batch (2,700 systems at N = 67 on a grid of 8 waves per CU) and its clean run,
    shared by the three tests below"""
    b = lc.wave_reuse_batch(lc.persistent_waves())
    args = (b["th"][0], b["th"][1] - b["th"][0], lc.to_geo(b["lines"]), b["dP"], b["centre"], b["sigma"], b["var"])
    r = ctx.local_eq_scan(*args, ps=b["ps"], shift=0.0, want_info=True)
    lc.assert_wave_reuse(ctx, "k_local_eq_scan", r["gam"].size)
    assert r["gam"].size >= 1.3 * lc.persistent_waves()
    return b, args, r


def test_more_systems_than_waves_against_the_oracle(ctx, reuse):
    """9a. every system of the batch against the oracle: gam, lam, the count at shift 0.  Measured on the CPU side: every oracle value
    finite, min |lam| / margin 2.6e5, 42 % of the systems unstable"""
    b, args, r = reuse
    g, c, f = lc.rows_of(b["th"], b["lines"], b["dP"], b["centre"], b["sigma"], b["var"], ps=b["ps"])
    ref = lc.oracle_of(b["th"], g, c, f)
    assert np.isfinite(ref["gam"]).all() and np.isfinite(ref["lam"]).all()
    count0 = lc.counts_of(b["th"], g, c, f, 0.0)
    print("wave reuse N=67: %d systems, %.0f %% unstable" % (count0.size, 100.0 * (count0 > 0).mean()))
    assert 0.2 < (count0 > 0).mean() < 0.8                   # (both branches of the growth-rate stage are well populated)
    check_against_oracle(r, ref, "wave reuse N=67, %d systems" % count0.size, count0)


def test_faults_between_clean_systems_on_one_wave(ctx, reuse):
    """9b. eps = NaN in every 7th triple, sigma = 0.5 on line 1, one NaN in gds21 of line 2: status 2, NaN gam and lam, count -1 on exactly
    those systems, every other system bitwise the clean run's.  With the lines in this order a wave's second system is one of line 2, so
    a fault follows a clean system on every reused wave; the same batch with the lines reversed puts the clean line last, where clean
    systems follow the faults.  count_only on the clean batch: the clean run's counts, no pass counted"""
    b, args, clean = reuse
    lo, h, geo, dP, centre, sigma, var = args
    n_var = len(var)
    bad_lines, bad_sigma, bad_var = b["lines"].copy(), sigma.copy(), var.copy()
    bad_var[::7, 1] = np.nan
    bad_sigma[1] = 0.5
    bad_lines[2, 5, 40] = np.nan
    hit = np.zeros((3, n_var), dtype=bool)
    hit[1] = hit[2] = hit[:, ::7] = True
    for order in ([0, 1, 2], [2, 1, 0]):
        r = ctx.local_eq_scan(lo, h, lc.to_geo(bad_lines[order]), dP[order], centre[order], bad_sigma[order], bad_var, ps=b["ps"][order],
                              shift=0.0, want_info=True)
        lc.assert_wave_reuse(ctx, "k_local_eq_scan", hit.size)
        r = {k: (v[np.argsort(order)] if k != "nbad" else v) for k, v in r.items()}
        assert r["nbad"] == hit.sum(), (order, r["nbad"], hit.sum())
        assert (status(r)[hit] == 2).all() and (status(r)[~hit] == 0).all()
        assert np.isnan(r["gam"][hit]).all() and np.isnan(r["lam"][hit]).all() and (r["count"][hit] == -1).all()
        for k in KEYS:
            assert np.array_equal(r[k][~hit], clean[k][~hit]), (order, k)
    rc = ctx.local_eq_scan(*args, ps=b["ps"], shift=0.0, count_only=True, want_info=True)
    lc.assert_wave_reuse(ctx, "k_local_eq_scan", hit.size)
    assert set(rc) == {"count", "info", "nbad"} and rc["nbad"] == 0
    assert np.array_equal(rc["count"], clean["count"]) and not rc["info"].any()


def raw_local_eq(ctx, n_lines, n_var, N, lo, h, geo, ld, dP, centre, sigma, ps, ps_ld, var, shift, device, want_gam=True):
    """ibs_local_eq_scan_f64 itself on the caller's leading dimensions, host pointers or device pointers -> (return value, outputs)"""
    import ctypes
    import torch
    shape = (n_lines, n_var)
    ins = [np.ascontiguousarray(a, dtype=np.float64) for a in (geo, dP, centre, sigma, ps, var)]
    out = dict(gam=np.zeros(shape), lam=np.zeros(shape), count=np.zeros(shape, np.int32), info=np.zeros(shape, np.int32))
    if device:
        ctx._stream_from_torch(torch.device("cuda:0"))
        ins = [torch.from_numpy(a).to("cuda:0") for a in ins]
        out = {k: torch.from_numpy(v).to("cuda:0") for k, v in out.items()}
        p = lambda a: ctypes.c_void_p(a.data_ptr())
    else:
        p = lambda a: ctypes.c_void_p(a.ctypes.data)
    rc = ctx._lib.ibs_local_eq_scan_f64(ctx._h, n_lines, n_var, N, float(lo), float(h), p(ins[0]), ld, p(ins[1]), p(ins[2]), p(ins[3]),
                                        p(ins[4]), ps_ld, p(ins[5]), float(shift), p(out["gam"]) if want_gam else None, p(out["lam"]),
                                        p(out["count"]), p(out["info"]), 0 if device else 1)
    if device:
        torch.cuda.synchronize()
        out = {k: v.cpu().numpy() for k, v in out.items()}
    return rc, out


def test_padded_rows_through_the_raw_entry(ctx, g3):
    """10. ld = N + 5 and ps_ld = N + 3 with NaN in every padding element, 3 NCSX lines x 6 triples at N = 513: the four outputs are
    Context.local_eq_scan's bits on the packed arrays, from host pointers and from device pointers; gam = NULL changes neither lam nor info"""
    th, lines, dP, alpha, sigma, ps, var = ncsx_batch(g3, 3)
    N, lo, h, geo = 513, th[0], th[1] - th[0], lc.to_geo(lines)
    packed = ctx.local_eq_scan(lo, h, geo, dP, alpha, sigma, var, ps=ps, shift=0.0, want_info=True)
    assert packed["nbad"] == 0 and np.isfinite(packed["gam"]).all()
    geo_p, ps_p = np.full((8, 3, N + 5), np.nan), np.full((3, N + 3), np.nan)
    geo_p[:, :, :N], ps_p[:, :N] = geo, ps
    for device in (False, True):
        rc, r = raw_local_eq(ctx, 3, len(var), N, lo, h, geo_p, N + 5, dP, alpha, sigma, ps_p, N + 3, var, 0.0, device)
        assert "k_local_eq_scan" in ctx.last_launch()[0]
        assert rc == 0 and not (r["info"] >> 16).any(), (device, rc)
        for k in KEYS:
            assert np.array_equal(r[k], packed[k]), (device, k)
        rc, r = raw_local_eq(ctx, 3, len(var), N, lo, h, geo_p, N + 5, dP, alpha, sigma, ps_p, N + 3, var, 0.0, device, want_gam=False)
        assert rc == 0 and not r["gam"].any()                # (not written)
        for k in ("lam", "count", "info"):
            assert np.array_equal(r[k], packed[k]), (device, k)


def test_the_rule_takes_the_magnitude_of_gradpar(ctx, g3):
    """11a. the lines of test 10 with gradpar negated on lines 0 and 2: the same bits"""
    th, lines, dP, alpha, sigma, ps, var = ncsx_batch(g3, 3)
    lo, h = th[0], th[1] - th[0]
    r = ctx.local_eq_scan(lo, h, lc.to_geo(lines), dP, alpha, sigma, var, ps=ps, shift=0.0, want_info=True)
    flipped = lines.copy()
    flipped[[0, 2], 1] *= -1.0
    assert (flipped[0, 1] < 0).all() and (flipped[1, 1] > 0).all()
    rf = ctx.local_eq_scan(lo, h, lc.to_geo(flipped), dP, alpha, sigma, var, ps=ps, shift=0.0, want_info=True)
    assert r["nbad"] == rf["nbad"] == 0
    for k in KEYS:
        assert np.array_equal(rf[k], r[k]), k


def test_off_centre_theta_window(ctx):
    """11b. theta_lo = -3 pi + 0.37, N = 771, h = 6 pi / 770: one s-alpha line built on that grid with centre 0.25 x the five triples of
    EDGE_VAR against the oracle on theta_lo + j h, counts at shift 0"""
    N, lo, h = 771, -3 * np.pi + 0.37, 6 * np.pi / 770
    th = lo + h * np.arange(N)
    assert abs(th[0] + th[-1]) > 0.7                         # (not symmetric about 0)
    line, dP, ps = lc.salpha_base_line(th, 0.25)
    args = ([line], np.array([dP]), np.array([0.25]), np.ones(1), EDGE_VAR)
    g, c, f = lc.rows_of(th, *args, ps=ps[None])
    r = ctx.local_eq_scan(lo, h, lc.to_geo(args[0]), *args[1:], ps=ps[None], shift=0.0, want_info=True)
    check_against_oracle(r, lc.oracle_of(th, g, c, f), "s-alpha off-centre window N=771", lc.counts_of(th, g, c, f, 0.0))


def test_wave_cap_on_the_longest_grid(ctx):
    """12. N = 65,537, one s-alpha line x 400 triples (theta0 = 0.1, eps x p on 20 x 20), count_only: the workspace budget of a chunk
    caps the grid at 2^30 / (6 N 8 bytes) = 341 waves, below the 400 systems; the counts are those of two calls with 200 triples each,
    bit for bit.  (No count is compared with the oracle at this length: test 5.)"""
    import time
    N = 65537
    th = bo.theta_grid(N)
    line, dP, ps = lc.salpha_base_line(th, 0.1)
    var = np.array([(0.1, e, p) for e in np.linspace(-0.9, 1.0, 20) for p in np.linspace(0.0, 3.0, 20)])
    args = (th[0], th[1] - th[0], lc.to_geo([line]), np.array([dP]), np.array([0.1]), np.ones(1))
    kw = dict(ps=ps[None], shift=0.0, count_only=True, want_info=True)
    ctx.synchronize()
    t = time.perf_counter()
    r = ctx.local_eq_scan(*args, var, **kw)
    dt = time.perf_counter() - t
    blocks = lc.assert_wave_reuse(ctx, "k_local_eq_scan", 400, at_most=2 ** 30 // (6 * N * 8))
    print("wave cap N=65537: 400 systems on %d blocks, %.3f s (host pointers, the call)" % (blocks, dt))
    assert r["nbad"] == 0 and not r["info"].any() and (r["count"] >= 0).all()
    halves = [ctx.local_eq_scan(*args, var[k:k + 200], **kw) for k in (0, 200)]
    assert np.array_equal(np.concatenate([q["count"] for q in halves], axis=1), r["count"])
