"""GPU: the resident form of the one-wave theta0 scan (k_gamma_scan<double, M>, 3 <= M <= 8: the rows of the set-up carried in
registers up to the growth-rate stage) against the lean form (k_gamma_scan_lean<double, M>: rebuilt and replayed), bit for bit.

Shapes: the smallest that reach every edge of the row ownership (WaveSolver::has_last) of the resident form -- N = 131 (M = 3, one
lane with a full chunk), 193 (M = 3, 63 lanes), 451 (M = 8, one lane), 513 (M = 8, 63 lanes) -- on 4 lines x 5 theta0 (the second
block of a line holds one valid and three invalid waves) in 2 surfaces.  The geometry is the first four golden NCSX lines
(tests/golden/G3_ncsx_lines.npz), interpolated linearly onto the shorter grids: bmag > 0, |gradpar| > 0 and the positive gds form
survive a convex combination of neighbouring points.

Tolerances: none is new.  Resident against lean: equal bits (each carried value is the value the lean form recomputes).  Against the
C oracle: what tests/test_gpu_edge_lengths.py holds this kernel to (check_scan: gam 1e-10, lam 4 N eps ||A||)."""
import functools
import os

import numpy as np
import pytest

from oracle import ballooning_oracle as bo
from oracle import c_oracle as co
from tests.test_gpu_edge_lengths import check_scan, scan_norm_a

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
SIZES = [131, 193, 451, 513]
N_LINES, N_SURF = 4, 2
THETA0 = np.array([0.0, 0.4, 0.8, 1.2, 1.5])


def rows_per_lane(N):
    return (N - 2 + 63) // 64


@pytest.fixture(scope="module")
def ctx():
    import ibs_amd
    c = ibs_amd.Context(0)
    yield c
    c.reset_options()
    c.close()


@functools.lru_cache(maxsize=None)
def inputs(N):
    """(h, the seven geometry arrays (N_LINES, N), dPdrho) of the golden lines on the N-point grid"""
    g3 = np.load(os.path.join(G, "G3_ncsx_lines.npz"))
    geo, th513, th = g3["geo_513"][:N_LINES], bo.theta_grid(513), bo.theta_grid(N)
    if N != 513:
        geo = np.stack([np.stack([np.interp(th, th513, ln[k]) for k in range(8)]) for ln in geo])
    a = tuple(np.ascontiguousarray(geo[:, k, :]) for k in range(7))
    assert (a[0] > 0).all() and (np.abs(a[1]) > 0).all()
    return float(th[1] - th[0]), a, np.ascontiguousarray(g3["dPdrho_513"][:N_LINES])


@functools.lru_cache(maxsize=None)
def reference(N):
    """the C oracle on the same systems, once per length: ref tuple of check_scan (no X, no theta0 derivative)"""
    h, a, dP = inputs(N)
    gam_c, lam_c, _ = co.gamma_scan(h, *a, dP, THETA0)
    nA = scan_norm_a(h, np.stack(a, axis=1), dP, THETA0)             # (lines as (n_lines, 7, N), the layout scan_norm_a folds)
    return gam_c, lam_c, None, None, None, nA


def on_device(N, a=None, dP=None, t0=None):
    import torch
    dev = torch.device("cuda:0")
    h, a0, dP0 = inputs(N)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    return h, [up(x) for x in (a0 if a is None else a)], up(dP0 if dP is None else dP), up(THETA0 if t0 is None else t0)


def both_forms(ctx, N, call):
    """call() under scan_resident = 1 and = 0: (resident result, lean result), the kernel names checked"""
    M = rows_per_lane(N)
    out = []
    try:
        for res, name in ((1, "ibs::k_gamma_scan<double, %d>" % M), (0, "ibs::k_gamma_scan_lean<double, %d>" % M)):
            ctx.set_option("scan_resident", res)
            out.append(call())
            assert ctx.last_launch()[0] == name, (N, res, ctx.last_launch())
    finally:
        ctx.set_option("scan_resident", None)
    return out


def same_bits(N, tag, r, l, keys):
    import torch
    for k in keys:
        assert r[k].shape == l[k].shape and torch.equal(r[k], l[k]), (N, tag, k, float((r[k] - l[k]).abs().max()))


@pytest.mark.parametrize("N", SIZES)
def test_resident_equals_lean_in_every_variant(ctx, N):
    """plain, with d gam / d theta0, with X and dX, warm-started, and the fused ScanPlan.scan_argmax: gam, lam, info and every
    requested output carry the same bits in both forms"""
    import torch
    import ibs_amd
    h, geo, dP, t0 = on_device(N)
    scan = lambda **kw: ctx.gamma_scan(h, *geo, dP, t0, want_info=True, **kw)
    r, l = both_forms(ctx, N, lambda: scan())
    assert int((r["info"] >> 16).abs().max()) == 0, (N, r["info"] >> 16)
    same_bits(N, "plain", r, l, ("gam", "lam", "info"))
    plain = r
    r, l = both_forms(ctx, N, lambda: scan(want_dtheta0=True))
    same_bits(N, "dtheta0", r, l, ("gam", "lam", "info", "dgam_dtheta0"))
    assert torch.equal(r["gam"], plain["gam"]) and bool(torch.isfinite(r["dgam_dtheta0"]).all())
    r, l = both_forms(ctx, N, lambda: scan(want_X=True))
    same_bits(N, "X, dX", r, l, ("gam", "lam", "info", "X", "dX"))
    # (X = x / max |x| formed as x * (1 / max |x|): 1 to an ulp, as check_pair of tests/test_gpu_edge_lengths.py holds it)
    assert torch.equal(r["gam"], plain["gam"]) and float((r["X"].abs().amax(dim=2) - 1.0).abs().max()) < 1e-15
    r, l = both_forms(ctx, N, lambda: scan(want_X=True, want_dtheta0=True))
    same_bits(N, "X, dX, dtheta0", r, l, ("gam", "lam", "info", "X", "dX", "dgam_dtheta0"))
    r, l = both_forms(ctx, N, lambda: scan(lam_guess=plain["lam"], guess_width=1e-3))
    same_bits(N, "warm", r, l, ("gam", "lam", "info"))

    def fused():
        plan = ibs_amd.ScanPlan(ctx, h, geo, dP, t0, N_SURF)
        plan.scan_argmax()
        torch.cuda.synchronize()
        return dict(gam=plan.gam.clone(), lam=plan.lam.clone(), info=plan.info.clone(), pack=plan.pack.clone())
    r, l = both_forms(ctx, N, fused)
    same_bits(N, "fused argmax", r, l, ("gam", "lam", "info", "pack"))
    assert torch.equal(r["gam"], plain["gam"])
    per = (N_LINES // N_SURF) * len(THETA0)
    for s in range(N_SURF):
        blk = plain["gam"].reshape(N_SURF, per)[s]
        k = int(torch.argmax(blk))
        assert float(r["pack"][s, 0]) == float(blk[k]) and int(r["pack"][s, 1]) == k, (N, s)


@pytest.mark.parametrize("N", SIZES)
def test_a_line_with_nonpositive_g(ctx, N):
    """one line whose g is negative at one grid point (status bit 1): both forms return the same status words and the same, possibly
    NaN, values; the other lines are untouched"""
    h, a, dP = inputs(N)
    a = [x.copy() for x in a]
    j = N // 3
    a[4][1, j], a[5][1, j], a[6][1, j] = -1.0, 0.0, 0.0               # gds2 + 2 theta0 gds21 + theta0^2 gds22 = -1 for every theta0
    h, geo, dP_d, t0 = on_device(N, a=a)
    call = lambda: ctx.gamma_scan(h, *geo, dP_d, t0, want_X=True, want_dtheta0=True, want_info=True)
    r, l = both_forms(ctx, N, call)
    st = (r["info"] >> 16).cpu().numpy()
    assert (st[1] & 2).all() and not (np.delete(st, 1, axis=0) & 3).any(), (N, st)
    for k in ("gam", "lam", "info", "X", "dX", "dgam_dtheta0"):
        assert np.array_equal(r[k].cpu().numpy(), l[k].cpu().numpy(), equal_nan=k != "info"), (N, k)
    h, geo0, dP0, _ = on_device(N)
    good = ctx.gamma_scan(h, *geo0, dP0, t0)
    keep = [0, 2, 3]
    assert np.array_equal(r["gam"].cpu().numpy()[keep], good["gam"].cpu().numpy()[keep]), N


@pytest.mark.parametrize("N", SIZES)
def test_resident_form_against_the_c_oracle(ctx, N):
    h, a, dP = inputs(N)
    try:
        ctx.set_option("scan_resident", 1)
        r = ctx.gamma_scan(h, *a, dP, THETA0, want_info=True)
        assert ctx.last_launch()[0] == "ibs::k_gamma_scan<double, %d>" % rows_per_lane(N), ctx.last_launch()
    finally:
        ctx.set_option("scan_resident", None)
    assert r["nbad"] == 0 and not ((r["info"] >> 16) & 3).any(), (N, r["info"] >> 16)
    check_scan(N, "resident", r, reference(N))


@pytest.mark.parametrize("N", SIZES)
def test_dispatch_names_the_form_it_runs(ctx, N):
    """automatic mode: these sizes hold 20 waves, far below two per SIMD: the resident form, under its own name"""
    h, geo, dP, t0 = on_device(N)
    ctx.gamma_scan(h, *geo, dP, t0)
    assert ctx.last_launch()[0] == "ibs::k_gamma_scan<double, %d>" % rows_per_lane(N), (N, ctx.last_launch())


def test_above_two_waves_per_simd_runs_the_lean_form(ctx):
    """N = 131, the four lines x (2 n_cu + 128) theta0 = 8 n_cu + 512 one-wave solves (force_p = 64, scan_chain = 1: the dispatch
    would take the sub-wave or the chained kernel at this size): more than two waves per SIMD, so automatic mode reports the lean
    name; its results equal the resident form's, on the whole batch and on the (line, theta0) pairs the small scan shares with it"""
    import torch
    N = 131
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    t_big = np.concatenate([THETA0, np.linspace(0.0, 1.5, 2 * n_cu + 128 - len(THETA0))])
    h, geo, dP, t0 = on_device(N, t0=t_big)
    try:
        ctx.set_option("force_p", 64); ctx.set_option("scan_chain", 1)
        auto = ctx.gamma_scan(h, *geo, dP, t0, want_info=True)
        name, waves = ctx.last_launch()
        assert name == "ibs::k_gamma_scan_lean<double, 3>" and waves > 8 * n_cu, (name, waves, n_cu)
        ctx.set_option("scan_resident", 1)
        res = ctx.gamma_scan(h, *geo, dP, t0, want_info=True)
        assert ctx.last_launch()[0] == "ibs::k_gamma_scan<double, 3>", ctx.last_launch()
        ctx.set_option("scan_resident", None)
        small = ctx.gamma_scan(h, *geo, dP, t0[:len(THETA0)], want_info=True)
        assert ctx.last_launch()[0] == "ibs::k_gamma_scan<double, 3>", ctx.last_launch()
    finally:
        ctx.set_option("scan_resident", None); ctx.set_option("force_p", None); ctx.set_option("scan_chain", None)
    assert int((auto["info"] >> 16).abs().max()) == 0
    same_bits(N, "big batch", res, auto, ("gam", "lam", "info"))
    for k in ("gam", "lam", "info"):
        assert torch.equal(auto[k][:, :len(THETA0)], small[k]), k
