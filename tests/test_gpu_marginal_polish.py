"""GPU: k_marginal_theta0_polish (ibs_marginal_theta0_polish_f64) on the shifted lines of tests/theta0_polish_cases.py -- nodes and slot
order against ibs_amd.row_peaks on the device's own table of mu, s* against the CPU oracle at the device's own theta0* (4 u, u from
marginal_oracle.solve: tests/test_gpu_marginal.py's bound), theta0* against the oracle-driven host state machine (8 xtol), scale_star
bitwise against ibs_marginal_scan_f64 at theta0*, the incumbent rule on the edge cases, the bitwise invariances of one call, the status
words, a batch of more slots than the persistent grid has waves; and the drivers (BallooningScan.marginal_envelope, marginal(n_starts=K | theta0_polish=True), AdjointStep.marginal) on the NCSX
tables of tests/golden/G8_*."""
import os

import numpy as np
import pytest

from tests import marginal_oracle as mo
from tests import marginal_polish_oracle as mpol
from tests import theta0_polish_cases as tc

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
XTOL = 1e-5
BIT_INF, BIT_NODE, BIT_MAXEVAL, BIT_ONE_SIDED = 1 << 8, 1 << 10, 1 << 11, 1 << 12
# the lane edge; the issue's CPU length; n = N - 2 = 767 and 769, either side of the 768-row LDS chunk of the count; the drivers' length;
# the first length beyond the register-resident growth-rate kernels
SHAPES = [(N, nt) for N in (67, 131, 769, 771, 969, 2051) for nt in tc.GRIDS]
KEYS, INTS = ("theta0", "mu", "scale"), ("node", "n_eval", "info", "n_found")


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
    """(h, geo7, dPdrho, theta0, mu, scale) of the shape on the host: the tables are the device's own (ctx.marginal_scan), computed once"""
    if (N, nt) not in _COARSE:
        h, geo7, dP = tc.case_lines(N)
        t0 = tc.theta0_grid(nt)
        sc = down(ctx.marginal_scan(h, *[up(a) for a in geo7], up(dP), up(t0), want_info=True))
        assert not ((sc["info"] >> 16) & 3).any()
        _COARSE[(N, nt)] = (h, geo7, dP, t0, sc["mu"], sc["scale"])
    return _COARSE[(N, nt)]


def polish(ctx, N, nt, device=True, K=1, order=None, mu=None, node=None, dP=None, t0=None):
    h, geo7, dP0, t00, m, _ = coarse(ctx, N, nt)
    m, dP, t0 = (m if mu is None else mu), (dP0 if dP is None else dP), (t00 if t0 is None else t0)
    o = slice(None) if order is None else order
    args = [a[o] for a in geo7] + [dP[o], t0, m[o]]
    kw = dict(n_starts=K, xtol=XTOL, want_info=True)
    if node is not None:
        kw["node"] = up(node) if device else node
    if device:
        args = [up(a) for a in args]
    return down(ctx.marginal_theta0_polish(h, *args, **kw))


def same(a, b, rows_a=slice(None), rows_b=slice(None)):
    return all(np.array_equal(bits(a[k][rows_a]), bits(b[k][rows_b])) for k in KEYS) and all(
        np.array_equal(a[k][rows_a], b[k][rows_b]) for k in INTS)


@pytest.mark.parametrize("N,nt", SHAPES)
def test_polish_against_the_oracle(ctx, N, nt):
    import ibs_amd
    from tests.test_theta0_polish_cpu import drive_c
    h, geo7, dP, t0, mu, scale = coarse(ctx, N, nt)
    r = polish(ctx, N, nt)
    node, n_found = ibs_amd.row_peaks(mu, 1)
    assert np.array_equal(r["node"], node) and np.array_equal(r["n_found"], n_found)
    status = r["info"] >> 16
    assert not (status & 3).any() and (r["n_eval"] <= 32).all()
    # scale_star is ibs_marginal_scan_f64's scale of the line at theta0_star, bit for bit: one scan of every line at every theta0*
    at = down(ctx.marginal_scan(h, *[up(a) for a in geo7], up(dP), up(r["theta0"][:, 0])))
    assert np.array_equal(bits(np.diagonal(at["scale"])), bits(r["scale"][:, 0]))
    assert np.array_equal(bits(np.diagonal(at["mu"])), bits(r["mu"][:, 0]))
    for i, case in enumerate(tc.CASES):
        j = int(node[i, 0])
        ln7 = [a[i] for a in geo7]
        ts, ss, ms = float(r["theta0"][i, 0]), float(r["scale"][i, 0]), float(r["mu"][i, 0])
        q = mo.solve(h, *mo.line_gc(dP[i], *ln7, ts))
        ref = drive_c(lambda t: 1.0 / mpol.line_scale(h, ln7, dP[i], t), t0, mu[i], j, XTOL, 32)
        lo, hi = tc.bracket(t0, mu[i], j)
        dense, ud = mpol.dense_min(h, ln7, dP[i], lo, hi)
        print("N=%d nt=%d case=%s: n_eval %d (host %d) status %#x  (s*-oracle(theta0*))/u %.2e  theta0*-ref %.2e  (s*-dense)/u %.2e  "
              "mu gain %.2e  passes %d" % (N, nt, case, r["n_eval"][i, 0], ref["n_eval"], status[i, 0], (ss - q["scale"]) / q["u"],
                                           ts - ref["theta0"], (ss - dense) / max(ud, q["u"]), ms - mu[i, j], r["info"][i, 0] & 0xffff))
        assert lo <= ts <= hi and ms >= mu[i, j] and bits(ms) == bits(1.0 / ss)
        assert abs(ss - q["scale"]) <= 4 * q["u"]
        assert abs(ts - ref["theta0"]) <= 8 * XTOL
        assert ss <= dense + 4 * max(ud, q["u"])
        if case in tc.EDGE:
            # the maximum sits on the edge of the box: the node and the table's values, bit for bit
            assert bits(ts) == bits(t0[j]) and bits(ms) == bits(mu[i, j]) and bits(ss) == bits(scale[i, j])
            assert status[i, 0] & BIT_NODE and status[i, 0] & BIT_ONE_SIDED and not status[i, 0] & (BIT_MAXEVAL | BIT_INF)
        else:
            assert not status[i, 0] & (BIT_NODE | BIT_MAXEVAL | BIT_INF)
            assert bool(status[i, 0] & BIT_ONE_SIDED) == (j in (0, nt - 1))
            if N == 131:                                 # (the length at which the crests were measured: 6.5e-4 and more above the row)
                assert ms > mu[i, j] and r["n_eval"][i, 0] <= 10


def test_invariances_of_one_call(ctx):
    import ibs_amd
    N, nt = 131, 15
    h, geo7, dP, t0, mu, scale = coarse(ctx, N, nt)
    n = len(dP)
    base = polish(ctx, N, nt)
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
        for k in KEYS + ("node", "n_eval", "info"):
            assert np.array_equal(bits(rk[k][:, 0]) if k in KEYS else rk[k][:, 0], bits(base[k][:, 0]) if k in KEYS else base[k][:, 0]), (K, k)
        node, n_found = ibs_amd.row_peaks(mu, K)
        assert np.array_equal(rk["node"], node) and np.array_equal(rk["n_found"], n_found)
        pad = np.arange(K)[None, :] >= n_found[:, None]
        for k in KEYS:
            assert np.array_equal(bits(rk[k])[pad], np.broadcast_to(bits(rk[k])[:, :1], (n, K))[pad]), "slots from n_found on repeat slot 0"
        for k in ("n_eval", "info"):
            assert np.array_equal(rk[k][pad], np.broadcast_to(rk[k][:, :1], (n, K))[pad]), k
        assert (rk["mu"] >= np.take_along_axis(mu, node, axis=1)).all() and (rk["n_eval"] <= 32).all()


def test_status_words(ctx):
    import ibs_amd
    N, nt = 131, 15
    h, geo7, dP, t0, mu, scale = coarse(ctx, N, nt)
    base = polish(ctx, N, nt)
    # a line without a drive: dPdrho = 0, no c_j > 0, the whole row has mu = 0 -- a VALUE: the plateau's first node comes back with
    # scale = inf, bits 8, 10 and 12, and it is not counted
    dP0 = dP.copy(); dP0[1] = 0.0
    args = [up(a) for a in geo7] + [up(dP0), up(t0)]
    sc0 = down(ctx.marginal_scan(h, *args, want_info=True))
    assert (sc0["mu"][1] == 0).all() and np.isinf(sc0["scale"][1]).all() and ((sc0["info"][1] >> 16) == BIT_INF).all()
    for device in (True, False):
        r = polish(ctx, N, nt, device=device, mu=sc0["mu"], dP=dP0)
        assert r.get("nbad", 0) == 0
        assert r["node"][1, 0] == 0 and r["theta0"][1, 0] == t0[0] and r["mu"][1, 0] == 0.0 and np.isposinf(r["scale"][1, 0])
        assert (r["info"][1, 0] >> 16) == BIT_INF | BIT_NODE | BIT_ONE_SIDED and 1 <= r["n_eval"][1, 0] <= 32
        others = [0, 2, 3, 4, 5]
        assert same({k: base[k] for k in KEYS + INTS}, r, rows_a=others, rows_b=others)
    # a line without a finite entry, and one NaN node beside an interior peak
    m2 = mu.copy()
    m2[1] = np.nan
    j3 = int(ibs_amd.row_peaks(mu[3], 1)[0][0, 0])
    assert 0 < j3 < nt - 1
    m2[3, j3 + 1] = np.nan
    r = polish(ctx, N, nt, mu=m2)
    assert r["node"][1, 0] == -1 and r["n_found"][1] == 0 and r["n_eval"][1, 0] == 0 and r["info"][1, 0] == 0
    assert np.isnan(r["theta0"][1, 0]) and np.isnan(r["mu"][1, 0]) and np.isnan(r["scale"][1, 0])
    assert r["node"][3, 0] == j3 and (r["info"][3, 0] >> 16) & BIT_ONE_SIDED
    assert t0[j3 - 1] <= r["theta0"][3, 0] <= t0[j3] and r["mu"][3, 0] >= mu[3, j3]
    others = [0, 2, 4, 5]
    assert same({k: base[k] for k in KEYS + INTS}, r, rows_a=others, rows_b=others)
    # the caller's nodes: -1 and a node outside the row leave the slot empty, the others are polished about the node named
    own = ibs_amd.row_peaks(mu, 1)[0]
    node = np.stack([own[:, 0], np.full(len(dP), -1, dtype=np.int32)], axis=1).astype(np.int32)
    node[0, 0] = -1
    node[2, 1] = nt + 3
    rn = polish(ctx, N, nt, K=2, node=node)
    want = node.copy(); want[2, 1] = -1
    assert np.array_equal(rn["node"], want) and not rn["n_found"].any()
    empty = want < 0
    assert np.isnan(rn["theta0"][empty]).all() and np.isnan(rn["mu"][empty]).all() and np.isnan(rn["scale"][empty]).all()
    assert (rn["n_eval"][empty] == 0).all() and (rn["info"][empty] == 0).all()
    for k in KEYS:
        assert np.array_equal(bits(rn[k][1:, 0]), bits(base[k][1:, 0])), k
    # a grid that does not increase: refused on host pointers; on device pointers every slot gets status bit 1 and NaN
    bad = t0.copy(); bad[2] = bad[1]
    with pytest.raises(ibs_amd.IbsError) as e:
        polish(ctx, N, nt, device=False, t0=bad)
    assert "(-1)" in str(e.value)
    rb = polish(ctx, N, nt, t0=bad)
    assert np.isnan(rb["theta0"]).all() and np.isnan(rb["mu"]).all() and np.isnan(rb["scale"]).all() and ((rb["info"] >> 16) == 2).all()


def test_more_slots_than_waves(ctx):
    """N = 67, the six case lines with their coarse rows on 15 nodes, K = 3, tiled until the slots number 1.3 times the persistent grid (8
    waves per CU): every wave rebuilds G and C in its workspace for every evaluation of every slot it serves.  Every 5th line has a NaN in
    gds21 and keeps its case's finite row -- each evaluation fails (status bit 1), the node comes back with the row's entry (the
    incumbent rule of csrc/ibs_theta0_polish.hpp); every 11th line has a row without a finite entry -- node -1, nothing is evaluated, as
    test_status_words pins it.  Every line's outputs: the bits of the same line in the batch of the 18 (case, kind) pairs"""
    import time
    from tests.local_eq_cases import assert_wave_reuse, persistent_waves
    N, nt, K = 67, 15, 3
    h, geo7, dP, t0, mu, _ = coarse(ctx, N, nt)
    n_case = len(tc.CASES)

    def run(case, kind):
        geo = [a[case].copy() for a in geo7]
        geo[5][kind == 1, 30] = np.nan
        m = mu[case].copy()
        m[kind == 2] = np.nan
        t = time.perf_counter()
        r = down(ctx.marginal_theta0_polish(h, *[up(a) for a in geo], up(dP[case]), up(t0), up(m), n_starts=K, xtol=XTOL, want_info=True))
        return r, time.perf_counter() - t

    case18, kind18 = np.tile(np.arange(n_case), 3), np.repeat(np.arange(3), n_case)
    ref, _ = run(case18, kind18)
    assert same(polish(ctx, N, nt, K=K), ref, rows_b=slice(0, n_case)), "the clean lines of the reference batch differ from the call alone"
    st = ref["info"] >> 16
    nan_line, no_row = kind18 == 1, kind18 == 2
    slot_node = np.clip(ref["node"], 0, None)
    assert (ref["node"][nan_line] >= 0).all() and (st[nan_line] & 2).all() and (st[nan_line] & BIT_NODE).all() and (ref["n_eval"][nan_line] > 0).all()
    assert np.array_equal(bits(ref["theta0"][nan_line]), bits(t0[slot_node[nan_line]]))
    assert np.array_equal(bits(ref["mu"][nan_line]), bits(np.take_along_axis(mu[case18], slot_node, axis=1)[nan_line]))
    assert (ref["node"][no_row] == -1).all() and not ref["n_found"][no_row].any() and not ref["n_eval"][no_row].any() and not ref["info"][no_row].any()
    assert all(np.isnan(ref[k][no_row]).all() for k in KEYS)
    assert not (st[kind18 == 0] & 3).any()
    n_lines = -(-int(np.ceil(1.3 * persistent_waves())) // K)
    i = np.arange(n_lines)
    case, kind = i % n_case, np.where(i % 11 == 0, 2, np.where(i % 5 == 0, 1, 0))
    r, dt = run(case, kind)
    blocks = assert_wave_reuse(ctx, "k_marginal_theta0_polish", n_lines * K)
    print("polish wave reuse N=67: %d lines x %d slots on %d blocks, %.3f s (uploads, the call, downloads); mean n_eval %.2f, max %d"
          % (n_lines, K, blocks, dt, r["n_eval"].mean(), r["n_eval"].max()))
    assert same(r, ref, rows_b=kind * n_case + case), "a line's outputs depend on the systems its waves served before"


# ---- the drivers on the NCSX tables (the shapes of tests/test_gpu_marginal_refine.py's driver test)
SVALS = np.array([0.6, 0.9])
N_DRV = 969
GRID = dict(nalpha=8, ntheta0=5)


def g8_wout():
    return dict(np.load(os.path.join(G, "G8_wout_ncsx_op.npz")))


@pytest.fixture(scope="module")
def drv(ctx):
    import torch
    import ibs_amd
    th = np.linspace(-4 * np.pi, 4 * np.pi, N_DRV)
    tabs = ibs_amd.SurfaceTables.from_wout(g8_wout(), SVALS)
    scan = ibs_amd.BallooningScan(ctx, None, th, SVALS, tables=tabs, device=torch.device("cuda:0"), **GRID)
    coarse_ = scan.marginal()
    plain = scan.marginal(refine=True)
    # the unit of every surface at the plain run's point, from the oracle on the host geometry of that line
    u = []
    for k, s in enumerate(SVALS):
        ln = scan.fieldlines(s, np.array([plain["alpha"][k]]))[0]
        u.append(mo.solve(scan.h, *mo.line_gc(-0.5 * np.mean((ln[2] - ln[7]) * ln[0] ** 2), *ln[:7], plain["theta0"][k]))["u"])
    return scan, coarse_, plain, np.array(u)


def test_envelope_on_two_surfaces(ctx, drv):
    scan, coarse_, plain, u = drv
    env = scan.marginal_envelope()
    assert ctx.last_launch()[0] == "ibs::k_marginal_theta0_polish"
    assert env["mu"].shape == env["scale"].shape == env["theta0"].shape == (2, 8, 1) and env["n_found"].shape == (2, 8)
    print("margin envelope: surface s* %s, coarse minimum %s, theta0* %s, mean n_eval %.2f"
          % (env["surface"][:, 2], coarse_["scale"], env["surface"][:, 0], env["n_eval"].mean()))
    assert (env["surface"][:, 2] <= coarse_["scale"]).all()
    assert (env["scale"][:, :, 0] <= coarse_["table"].min(axis=2)).all() and (env["n_eval"] <= 32).all()
    flat = env["scale"].reshape(2, -1)
    assert np.array_equal(env["surface"][:, 2], flat.min(axis=1))
    env2 = scan.marginal_envelope(n_starts=2)
    assert env2["mu"].shape == (2, 8, 2) and np.array_equal(bits(env2["mu"][:, :, 0]), bits(env["mu"][:, :, 0]))
    assert np.array_equal(bits(env2["surface"]), bits(env["surface"]))


def test_refinement_with_the_two_options(ctx, drv):
    scan, coarse_, plain, u = drv
    pol = scan.marginal(refine=True, theta0_polish=True)
    two = scan.marginal(refine=True, n_starts=2)
    print("refined margin: plain %s  from the crest %s  two starts %s  (u %s; candidates %s, n_found %s, evals %s)"
          % (plain["scale"], pol["scale"], two["scale"], u, two["candidates"][:, :, 0], two["n_found"], two["evals"]))
    assert (pol["scale"] <= plain["scale"] + 4 * u).all() and (two["scale"] <= plain["scale"] + 4 * u).all()
    assert set(pol) == set(plain) and np.array_equal(pol["coarse_scale"], coarse_["scale"])
    assert np.array_equal(bits(np.stack([pol["start"][:, 1], pol["start"][:, 0]], axis=1)), bits(scan.last_marginal_envelope["surface"][:, :2]))
    assert two["candidates"].shape == (2, 2, 3) and two["evals"].shape == two["task"].shape == (2, 2)
    assert np.array_equal(bits(two["candidates"][:, 0]), bits(np.stack([plain["scale"], plain["alpha"], plain["theta0"]], axis=1)))
    assert np.array_equal(two["evals"][:, 0], plain["evals"])
    assert np.array_equal(two["scale"], two["candidates"][:, :, 0].min(axis=1))
    again = scan.marginal(refine=True, n_starts=1)
    assert set(again) == set(plain) and all(np.array_equal(again[k], plain[k]) for k in plain)
    with pytest.raises(ValueError):
        scan.marginal(refine=True, n_starts=2, theta0_polish=True)


def test_adjoint_step_passes_the_options_through(ctx):
    """AdjointStep.marginal(n_starts=2) on two equilibria (base, scaled pressure): every equilibrium's rows equal a separate
    BallooningScan.marginal(refine=True, n_starts=2) on that equilibrium's rows of the step's table set, bitwise"""
    import torch
    import ibs_amd
    dev = torch.device("cuda:0")
    wout0 = g8_wout()
    scaled = dict(wout0)
    scaled["pres"] = np.asarray(wout0["pres"], dtype=np.float64) * 50.0
    wouts = [wout0, scaled]
    th = ibs_amd.theta_grid_for(11, 11)
    assert len(th) == N_DRV
    step = ibs_amd.AdjointStep(ctx, th, SVALS, dev, **GRID)
    out = step.marginal(wouts, n_starts=2)
    step_tabs = ibs_amd.SurfaceTables.from_wouts(wouts, SVALS)
    for q in range(2):
        m = ibs_amd.BallooningScan(ctx, None, th, SVALS, tables=step_tabs, surf_index=[2 * q, 2 * q + 1], device=dev,
                                   **GRID).marginal(refine=True, n_starts=2)
        for key in ("scale", "alpha", "theta0"):
            assert np.array_equal(out[key][q], m[key]), (q, key, out[key][q], m[key])
    with pytest.raises(ValueError):
        step.marginal(wouts, n_starts=2, theta0_polish=True)
