"""GPU: k_theta0_polish (ibs_theta0_polish_f64) on the shifted lines of tests/theta0_polish_cases.py -- nodes and slot order against
ibs_amd.row_peaks on the device's own coarse table, gam* against the CPU oracle at the device's own theta0*, theta0* against the
oracle-driven host state machine, the incumbent rule on the edge cases, bitwise invariances of one call; and the drivers
(BallooningScan.envelope, theta0_polish=True) on the NCSX tables of tests/golden/G8_*."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import theta0_polish_cases as tc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
XTOL = 1e-5
TOL_GAM = 1e-10          # the suite's small-shape bound on a growth rate against the oracle
BIT_NODE, BIT_MAXEVAL, BIT_ONE_SIDED = 1 << 10, 1 << 11, 1 << 12
# rows per lane M = 2 (the LDS-round-trip growth-rate stage), 3, 9, 16 and 32 (the longest grid: the first two interior cases only)
SHAPES = [(N, nt) for N in (67, 131, 515, 969, 2049) for nt in tc.GRIDS]


def cases_of(N):
    return tc.CASES[:2] if N == 2049 else tc.CASES


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.fixture(scope="module")
def ctx():
    import ibs_amd
    c = ibs_amd.Context(0)
    yield c
    c.close()


def up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def down(r):
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in r.items()}


_COARSE = {}


def coarse(ctx, N, nt):
    """(h, geo7, dPdrho, theta0, gam, lam) of the shape on the host: the table is the device's own (ctx.gamma_scan), computed once"""
    if (N, nt) not in _COARSE:
        h, geo7, dP = tc.case_lines(N, cases_of(N))
        t0 = tc.theta0_grid(nt)
        sc = down(ctx.gamma_scan(h, *[up(a) for a in geo7], up(dP), up(t0)))
        _COARSE[(N, nt)] = (h, geo7, dP, t0, sc["gam"], sc["lam"])
    return _COARSE[(N, nt)]


def polish(ctx, N, nt, device=True, K=1, order=None, gam=None, node=None, **kw):
    h, geo7, dP, t0, g, lam = coarse(ctx, N, nt)
    g = g if gam is None else gam
    o = slice(None) if order is None else order
    args = [a[o] for a in geo7] + [dP[o], t0, g[o]]
    kw = dict(n_starts=K, xtol=XTOL, lam=lam[o], want_lam=True, want_info=True, **kw)
    if node is not None:
        kw["node"] = up(node) if device else node
    if device:
        args, kw["lam"] = [up(a) for a in args], up(kw["lam"])
    return down(ctx.theta0_polish(h, *args, **kw))


_REF = {}


def reference(N, nt, case, row):
    """the host state machine driven by the CPU oracle from the device's own row: (theta0*, gam*, n_eval, status)"""
    from tests.test_theta0_polish_cpu import drive_c
    key = (N, nt, case)
    if key not in _REF:
        import ibs_amd
        node = int(ibs_amd.row_peaks(row, 1)[0][0, 0])
        _REF[key] = drive_c(lambda t: tc.oracle_gam(N, case, t), tc.theta0_grid(nt), row, node, XTOL, 32)
    return _REF[key]


@pytest.mark.parametrize("N,nt", SHAPES)
def test_polish_against_the_oracle(ctx, N, nt):
    import ibs_amd
    h, geo7, dP, t0, gam, lam = coarse(ctx, N, nt)
    r = polish(ctx, N, nt)
    node, n_found = ibs_amd.row_peaks(gam, 1)
    assert np.array_equal(r["node"], node) and np.array_equal(r["n_found"], n_found)
    status = r["info"] >> 16
    assert not (status & 3).any() and (r["n_eval"] <= 32).all()
    for i, case in enumerate(cases_of(N)):
        j = int(node[i, 0])
        ts, gs = float(r["theta0"][i, 0]), float(r["gam"][i, 0])
        ref = reference(N, nt, case, gam[i])
        lo, hi = tc.bracket(t0, gam[i], j)
        dense = tc.dense_max(N, case, lo, hi)
        og = tc.oracle_gam(N, case, ts)
        print("N=%d nt=%d case=%s: n_eval %d (host %d) status %#x  gam*-oracle(theta0*) %.2e  theta0*-ref %.2e  gam*-dense %.2e  gain %.2e"
              % (N, nt, case, r["n_eval"][i, 0], ref["n_eval"], status[i, 0], gs - og, ts - ref["theta0"], gs - dense, gs - gam[i, j]))
        assert lo <= ts <= hi
        assert gs >= gam[i, j]
        assert abs(gs - og) <= TOL_GAM
        if case in tc.EDGE:
            # the maximum sits on the edge of the box: the node and the table's value, bit for bit
            assert bits(ts) == bits(t0[j]) and bits(gs) == bits(gam[i, j]) and bits(r["lam"][i, 0]) == bits(lam[i, j])
            assert status[i, 0] & BIT_NODE and status[i, 0] & BIT_ONE_SIDED
        else:
            assert not status[i, 0] & (BIT_NODE | BIT_MAXEVAL) and r["n_eval"][i, 0] <= 10
            assert bool(status[i, 0] & BIT_ONE_SIDED) == (j in (0, nt - 1))
        assert abs(ts - ref["theta0"]) <= 8 * XTOL
        assert gs >= dense - 1e-8


def test_invariances_of_one_call(ctx):
    N, nt = 131, 15
    h, geo7, dP, t0, gam, lam = coarse(ctx, N, nt)
    n = len(dP)
    keys = ("theta0", "gam", "lam")
    ints = ("node", "n_eval", "info", "n_found")
    base = polish(ctx, N, nt)

    def same(a, b, rows_a=slice(None), rows_b=slice(None)):
        return all(np.array_equal(bits(a[k][rows_a]), bits(b[k][rows_b])) for k in keys) and all(
            np.array_equal(a[k][rows_a], b[k][rows_b]) for k in ints)

    host = polish(ctx, N, nt, device=False)
    assert host.pop("nbad") == 0
    assert same(base, host), "host-pointer and device-pointer calls differ"
    assert same(base, polish(ctx, N, nt)), "a second call differs"
    rev = np.arange(n)[::-1].copy()
    assert same(base, polish(ctx, N, nt, order=rev), rows_b=rev), "the order of the lines matters"
    one = polish(ctx, N, nt, order=np.array([2]))
    assert same(base, one, rows_a=slice(2, 3)), "n_lines matters"
    for K in (2, 4):
        rk = polish(ctx, N, nt, K=K)
        assert rk["theta0"].shape == (n, K)
        for k in keys + ("node", "n_eval", "info"):
            assert np.array_equal(bits(rk[k][:, 0]) if k in keys else rk[k][:, 0], bits(base[k][:, 0]) if k in keys else base[k][:, 0]), (K, k)
        import ibs_amd
        node, n_found = ibs_amd.row_peaks(gam, K)
        assert np.array_equal(rk["node"], node) and np.array_equal(rk["n_found"], n_found)
        pad = np.arange(K)[None, :] >= n_found[:, None]
        for k in keys:
            assert np.array_equal(bits(rk[k])[pad], np.broadcast_to(bits(rk[k])[:, :1], (n, K))[pad]), "slots from n_found on repeat slot 0"


def test_nan_lines_and_named_nodes(ctx):
    import ibs_amd
    N, nt = 131, 15
    h, geo7, dP, t0, gam, lam = coarse(ctx, N, nt)
    base = polish(ctx, N, nt)
    g2 = gam.copy()
    g2[1] = np.nan                                   # a line without a finite entry
    j3 = int(ibs_amd.row_peaks(gam[3], 1)[0][0, 0])  # an interior peak: one NaN node beside it makes the bracket one-sided
    assert 0 < j3 < nt - 1
    g2[3, j3 + 1] = np.nan
    r = polish(ctx, N, nt, gam=g2)
    assert r["node"][1, 0] == -1 and r["n_found"][1] == 0 and r["n_eval"][1, 0] == 0
    assert np.isnan(r["theta0"][1, 0]) and np.isnan(r["gam"][1, 0]) and np.isnan(r["lam"][1, 0])
    assert r["node"][3, 0] == j3 and (r["info"][3, 0] >> 16) & BIT_ONE_SIDED
    assert t0[j3 - 1] <= r["theta0"][3, 0] <= t0[j3] and r["gam"][3, 0] >= gam[3, j3]
    others = [0, 2, 4, 5]
    for k in ("theta0", "gam", "lam"):
        assert np.array_equal(bits(r[k][others]), bits(base[k][others])), k
    assert np.array_equal(r["info"][others], base["info"][others])
    # the caller's nodes: -1 slots stay empty, the others are polished about the node named
    own = ibs_amd.row_peaks(gam, 1)[0]
    node = np.stack([own[:, 0], np.full(len(dP), -1, dtype=np.int32)], axis=1).astype(np.int32)
    node[0, 0] = -1
    rn = polish(ctx, N, nt, K=2, node=node)
    assert np.array_equal(rn["node"], node)
    empty = node < 0
    assert np.isnan(rn["theta0"][empty]).all() and np.isnan(rn["gam"][empty]).all() and (rn["n_eval"][empty] == 0).all()
    for k in ("theta0", "gam", "lam"):
        assert np.array_equal(bits(rn[k][1:, 0]), bits(base[k][1:, 0])), k


def test_unsupported_and_bad_grids(ctx):
    import ibs_amd
    N = 2051
    z = np.ones((1, N))
    with pytest.raises(ibs_amd.IbsError) as e:
        ctx.theta0_polish(0.01, z, z, z, z, z, z, z, np.ones(1), np.array([0.0, 1.0]), np.zeros((1, 2)))
    assert "(-3)" in str(e.value)
    # a grid that does not increase: refused on host pointers; on device pointers every slot gets status bit 1 and NaN
    h, geo7, dP, t0, gam, lam = coarse(ctx, 131, 5)
    bad = t0.copy(); bad[2] = bad[1]
    with pytest.raises(ibs_amd.IbsError) as e:
        ctx.theta0_polish(h, *geo7, dP, bad, gam)
    assert "(-1)" in str(e.value)
    r = down(ctx.theta0_polish(h, *[up(a) for a in geo7], up(dP), up(bad), up(gam), want_info=True))
    assert np.isnan(r["theta0"]).all() and np.isnan(r["gam"]).all() and ((r["info"] >> 16) == 2).all()


# ---- the drivers on the NCSX tables (the shapes of tests/test_gpu_scan_peaks.py's driver)
N_DRV = 513
SVALS3 = np.array([0.5, 0.7, 0.9])
GRID = dict(nalpha=8, ntheta0=5)


# On the three surfaces above every row of the 8 x 5 table peaks on an edge node, so the envelope equals the coarse table there.  These
# three, on a 12 x 9 grid, have their surface maximum on a crest BETWEEN two theta0 nodes: there the polish has something to find
SVALS_IN = np.array([0.80, 0.83, 0.86])
GRID_IN = dict(nalpha=12, ntheta0=9)


def driver(ctx, svals=SVALS3, grid=GRID, **kw):
    import torch
    import ibs_amd
    th = np.linspace(-4 * np.pi, 4 * np.pi, N_DRV)
    tabs = ibs_amd.SurfaceTables.from_wout(dict(np.load(os.path.join(G, "G8_wout_ncsx_op.npz"))), svals)
    return ibs_amd.BallooningScan(ctx, None, th, svals, tables=tabs, device=torch.device("cuda:0"), **grid, **kw)


def test_drivers_on_surfaces_with_an_interior_crest(ctx):
    """where the crest lies between nodes the envelope is STRICTLY above the coarse table (a polished point is returned only if it
    beats its node strictly), theta0_polish=True moves the start off the node, and the refinement does not fall below it"""
    inner = dict(svals=SVALS_IN, grid=GRID_IN)
    plain = driver(ctx, **inner)
    tab = plain.coarse()
    env = plain.envelope()
    cmax = tab.max(axis=(1, 2))
    print("interior crests: envelope - coarse maximum %s at theta0* %s, largest n_eval per surface %s"
          % (env["surface"][:, 2] - cmax, env["surface"][:, 0], env["n_eval"].max(axis=(1, 2))))
    assert (env["surface"][:, 2] > cmax).all()
    assert not np.isin(env["surface"][:, 0], plain.theta0_scan).any()
    assert (env["gam"][:, :, 0] >= tab.max(axis=2)).all()
    geo = ctx.fieldline_geometry(plain.tables, np.repeat(plain._own_surf(), 12), np.tile(plain.alpha_scan, 3), plain.theta, device=plain.device)
    pts = ctx.gamma_points(plain.h, *[geo["geo"][q] for q in range(7)], geo["dPdrho"], up(env["theta0"].reshape(-1)))
    assert np.abs(pts["gam"].cpu().numpy() - env["gam"].reshape(-1)).max() <= TOL_GAM
    node_rows = plain.device_rows(refine=False)[0].cpu().numpy()
    assert np.array_equal(node_rows[:, 2], cmax)
    on = driver(ctx, theta0_polish=True, **inner)
    r0, bad = on.device_rows(refine=False)
    r0 = r0.cpu().numpy()
    assert float(bad.item()) == 0.0
    assert np.array_equal(bits(r0), bits(env["surface"]))
    assert (r0[:, 2] > node_rows[:, 2]).all() and (r0[:, 0] != node_rows[:, 0]).all()
    rows, bad = on.device_rows()
    rows = rows.cpu().numpy()
    assert float(bad.item()) == 0.0
    today = plain.device_rows()[0].cpu().numpy()
    print("refined from the crest %s, from the node %s, the crest itself %s" % (rows[:, 2], today[:, 2], r0[:, 2]))
    assert (rows[:, 2] >= r0[:, 2] - 1e-8).all()


def test_envelope_on_three_surfaces(ctx):
    scan = driver(ctx)
    tab = scan.coarse()
    env = scan.envelope(n_starts=2)
    assert env["gam"].shape == (3, 8, 2) and env["n_found"].shape == (3, 8) and env["surface"].shape == (3, 3)
    print("envelope maximum - coarse maximum per surface:", env["surface"][:, 2] - tab.max(axis=(1, 2)), "mean n_eval %.2f" % env["n_eval"].mean())
    assert (env["surface"][:, 2] >= tab.max(axis=(1, 2))).all()
    assert (env["gam"][:, :, 0] >= tab.max(axis=2)).all()
    flat = env["gam"].reshape(3, -1)
    assert np.array_equal(env["surface"][:, 2], flat.max(axis=1))
    best = flat.argmax(axis=1)
    assert np.array_equal(env["surface"][:, 0], env["theta0"].reshape(3, -1)[np.arange(3), best])
    assert np.array_equal(env["surface"][:, 1], scan.alpha_scan[best // 2])
    # every gam is the growth rate of its line at theta0*: ctx.gamma_points on the same lines
    geo = ctx.fieldline_geometry(scan.tables, np.repeat(scan._own_surf(), 8), np.tile(scan.alpha_scan, 3), scan.theta, device=scan.device)
    for k in range(2):
        pts = ctx.gamma_points(scan.h, *[geo["geo"][q] for q in range(7)], geo["dPdrho"], up(env["theta0"][:, :, k].reshape(-1)))
        assert np.abs(pts["gam"].cpu().numpy() - env["gam"][:, :, k].reshape(-1)).max() <= TOL_GAM
    import ibs_amd
    with pytest.raises(ValueError):
        driver(ctx, eigenpair="nearest").envelope()


def test_driver_with_theta0_polish(ctx):
    plain = driver(ctx)
    today = plain.device_rows()[0].cpu().numpy()
    off = driver(ctx, theta0_polish=False)
    assert np.array_equal(bits(today), bits(off.device_rows()[0].cpu().numpy())) and off.last_envelope is None
    on = driver(ctx, theta0_polish=True)
    r0, bad = on.device_rows(refine=False)
    r0 = r0.cpu().numpy()
    assert float(bad.item()) == 0.0
    env = on.envelope()
    last = {k: v.cpu().numpy() for k, v in on.last_envelope.items()}
    assert np.array_equal(bits(r0), bits(env["surface"])), (r0, env["surface"])
    assert np.array_equal(bits(last["gam"].reshape(3, 8, 1)), bits(env["gam"]))
    coarse_rows = plain.device_rows(refine=False)[0].cpu().numpy()
    assert (r0[:, 2] >= coarse_rows[:, 2]).all()
    rows, bad = on.device_rows()
    rows = rows.cpu().numpy()
    assert float(bad.item()) == 0.0
    print("refined from the polished start - polished start:", rows[:, 2] - r0[:, 2], " refined today:", today[:, 2])
    assert (rows[:, 2] >= r0[:, 2] - 1e-8).all()
    for kw in (dict(eigenpair="nearest"), dict(n_starts=2)):
        with pytest.raises(ValueError):
            driver(ctx, theta0_polish=True, **kw)
    import ibs_amd
    with pytest.raises(ValueError):
        ibs_amd.BallooningScan(ctx, lambda s, a: None, np.linspace(-1, 1, 67), SVALS3, theta0_polish=True)
