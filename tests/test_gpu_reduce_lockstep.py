"""GPU: the wave-wide reductions of the resident one-wave scan (wave_reduce_lockstep, max_plain and wave_argmax_first_l63 in
csrc/ibs_wave.hpp: several ladders advanced level by level, a max step of one fetch and one v_max, row_bcast fetches that set up
nothing) against the lean form, which keeps the ladders wave_sum / wave_max one after the other -- option scan_resident 1 / 0, bit
for bit, as tests/test_gpu_scan_resident.py compares the forms.

What a ladder can get wrong is WHERE a value travels: a partial that lane 63 never receives, or a fill value that it does.  So the
extremes are put into every lane at which the ladder changes its step: lanes 0, 15, 16, 31, 32, 47, 48 and 63 are the two ends of
each row of 16 lanes, i.e. every row_shr edge and every source (15, 31) and target row (16 .., 32 .., 48 ..) of the two row_bcast
steps.  Lines: the moving well of tests/edge_cases.py, one line per lane, centred on the grid point of that lane's first row, 0.7
grid rows wide and 30 deep as in tests/test_gpu_twist_pick.py: the mode sits on one grid point, so the largest |X| (the
normalisation's max), the twist key (largest f |u w|; f is constant) and the Gershgorin maxima of set-up (largest c / f, d / f and
(|d| + e + e) / f: all at the centre of the well) lie in the aimed lane.  N = 131 (M = 3) and N = 513 (M = 8): the smallest and
the largest rows-per-lane of the resident form.  Each case asserts from X that |X| peaks on its target.

Groups run: set-up's eight (every call), the growth-rate stage's two sums (no theta0 derivative) and five (with it; on the
golden NCSX lines as well, whose theta0 tangents are not zero), the single ladders of the twist key, sum f x^2 and max |x| (every
call), the hand-off's first maximum (fused scan_argmax).  One line with a non-positive g takes the `bad` path.

Tolerances: none; gam, lam, info, X, dX and d gam / d theta0 carry equal bits in both forms."""
import functools

import numpy as np
import pytest

from tests import edge_cases as ec
from tests.test_gpu_scan_resident import both_forms, on_device, same_bits

pytestmark = pytest.mark.gpu

SIZES = [131, 513]
LANES = [0, 15, 16, 31, 32, 47, 48, 63]
THETA0 = np.array([0.0, 0.5])
WELL = dict(wr=0.7, depth=30.0)
KEYS = ("gam", "lam", "info", "X", "dX", "dgam_dtheta0")


@pytest.fixture(scope="module")
def ctx():
    import ibs_amd
    c = ibs_amd.Context(0)
    c.set_option("force_p", 64)
    yield c
    c.reset_options()
    c.close()


def lane_of(N, j):
    """the lane that holds grid point j (row j - 1)"""
    n = N - 2
    return max(L for L in range(64) if ec.lane_rows_start(L, n) <= j - 1)


def targets(N):
    """the grid point of the first row of each lane of LANES"""
    return [ec.lane_rows_start(L, N - 2) + 1 for L in LANES]


@functools.lru_cache(maxsize=None)
def lines(N):
    """(h, seven geometry arrays (8, N), dPdrho (8,), targets): one moving-well line per lane of LANES (read only)"""
    th = ec.theta_grid(N)
    tg = targets(N)
    geo = [ec.to_geometry(*ec.well_rows(th, j, **WELL)) for j in tg]
    arrays = tuple(np.ascontiguousarray(np.stack([g[k] for g in geo])) for k in range(7))
    return float(th[1] - th[0]), arrays, np.full(len(tg), -1.0), tg


def upload(arrays, dP):
    import torch
    dev = torch.device("cuda:0")
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    return [up(a) for a in arrays], up(dP), up(THETA0)


def equal_bits(N, tag, r, l, keys):
    import torch
    same_bits(N, tag, r, l, keys)
    for k in keys:
        if k != "info":                                   # (torch.equal holds -0.0 equal to 0.0: the integer view does not)
            assert torch.equal(r[k].view(torch.int64), l[k].view(torch.int64)), (N, tag, k)


def test_targets_lie_in_the_aimed_lanes():
    assert {N: ec.rows_per_lane(N) for N in SIZES} == {131: 3, 513: 8}
    for N in SIZES:
        tg = targets(N)
        assert [lane_of(N, j) for j in tg] == LANES, (N, tg)
        assert tg[0] == 1 and len(set(tg)) == len(LANES) and max(tg) <= N - 2, (N, tg)


@pytest.mark.parametrize("dth0", [False, True], ids=["two_sums", "five_sums"])
@pytest.mark.parametrize("N", SIZES)
def test_extremes_in_every_ladder_edge_lane(ctx, N, dth0):
    import torch
    h, arrays, dP, tg = lines(N)
    geo, dP_d, t0 = upload(arrays, dP)
    call = lambda: ctx.gamma_scan(h, *geo, dP_d, t0, want_X=True, want_dtheta0=dth0, want_info=True)
    r, l = both_forms(ctx, N, call)
    peak = r["X"].abs().argmax(dim=2).cpu().numpy()
    want = np.array(tg)
    print(N, "lanes", LANES, "targets", tg, "peaks", peak[:, 0].tolist())
    assert np.array_equal(peak[:, 0], want) and np.array_equal(peak[:, 1], want), (N, peak.T, want)
    assert int((r["info"] >> 16).abs().max()) == 0, (N, r["info"] >> 16)
    assert bool(torch.isfinite(r["gam"]).all()) and bool(torch.isfinite(r["X"]).all())
    equal_bits(N, "well", r, l, KEYS if dth0 else KEYS[:5])


@pytest.mark.parametrize("N", SIZES)
def test_five_sums_with_nonzero_theta0_tangents(ctx, N):
    """the golden NCSX lines of tests/test_gpu_scan_resident.py: every one of the five sums of the growth-rate stage is non-trivial"""
    import torch
    h, geo, dP, t0 = on_device(N)
    call = lambda: ctx.gamma_scan(h, *geo, dP, t0, want_X=True, want_dtheta0=True, want_info=True)
    r, l = both_forms(ctx, N, call)
    assert bool(torch.isfinite(r["dgam_dtheta0"]).all()) and float(r["dgam_dtheta0"].abs().max()) > 0.0
    equal_bits(N, "ncsx", r, l, KEYS)


@pytest.mark.parametrize("N", SIZES)
def test_a_line_with_nonpositive_g_takes_the_bad_path(ctx, N):
    """the line aimed at lane 31 gets g = -1 at one grid point (status bit 1): equal status words and equal, possibly NaN, values in
    both forms; the other lines are untouched"""
    h, arrays, dP, tg = lines(N)
    a = [x.copy() for x in arrays]
    a[4][3, N // 3] = -1.0                                 # gds2 (the theta0 terms are zero): g = gradpar * gds2 < 0 for every theta0
    geo, dP_d, t0 = upload(a, dP)
    call = lambda: ctx.gamma_scan(h, *geo, dP_d, t0, want_X=True, want_dtheta0=True, want_info=True)
    r, l = both_forms(ctx, N, call)
    st = (r["info"] >> 16).cpu().numpy()
    assert (st[3] & 2).all() and not (np.delete(st, 3, axis=0) & 3).any(), (N, st)
    for k in KEYS:
        rk, lk = r[k].cpu().numpy(), l[k].cpu().numpy()
        assert np.array_equal(rk, lk, equal_nan=k != "info"), (N, k)
        if k != "info":
            keep = np.delete(np.arange(len(LANES)), 3)
            assert np.array_equal(rk[keep].view(np.int64), lk[keep].view(np.int64)), (N, k)
    geo0, dP0, _ = upload(arrays, dP)
    good = ctx.gamma_scan(h, *geo0, dP0, t0)
    keep = np.delete(np.arange(len(LANES)), 3)
    assert np.array_equal(r["gam"].cpu().numpy()[keep], good["gam"].cpu().numpy()[keep]), N


@pytest.mark.parametrize("N", SIZES)
def test_hand_off_first_maximum(ctx, N):
    """the fused scan_argmax on the well lines as one surface: both theta0 give the same line (the theta0 terms are zero), so every
    growth rate occurs twice and the FIRST of the equal maxima must win"""
    import torch
    import ibs_amd
    h, arrays, dP, _ = lines(N)
    geo, dP_d, t0 = upload(arrays, dP)

    def fused():
        plan = ibs_amd.ScanPlan(ctx, h, geo, dP_d, t0, 1)
        plan.scan_argmax()
        torch.cuda.synchronize()
        return dict(gam=plan.gam.clone(), pack=plan.pack.clone())
    r, l = both_forms(ctx, N, fused)
    same_bits(N, "fused argmax", r, l, ("gam", "pack"))
    assert torch.equal(r["pack"].view(torch.int64), l["pack"].view(torch.int64)), N
    flat = r["gam"].reshape(-1)
    k = int(torch.argmax(flat))
    first = int((flat == flat[k]).nonzero()[0])
    assert float(r["pack"][0, 0]) == float(flat[k]) and int(r["pack"][0, 1]) == first, (N, r["pack"], k, first)
