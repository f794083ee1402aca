"""GPU: the twist-row pick of the resident one-wave scan (WaveSolver<T, M, true>::twisted in csrc/ibs_wave.hpp: the entries around
the twist row are read from the winning lane's registers by a wave-uniform switch on the row's slot) against the lean form, which
keeps the per-row select chain -- option scan_resident 1 / 0, bit for bit, as tests/test_gpu_scan_resident.py compares the forms.

Lines: the moving well of tests/edge_cases.py (well_rows through to_geometry), one line per target, the well centred on the grid
point of slot i = 0 .. (rows of the lane) - 1 of lanes 0, 1, 62 and 63 -- row r of the matrix is grid point r + 1, lane L holds the
rows from lane_rows_start(L).  N = 131: M = 3, lane 0 holds three rows and the others two (9 targets); N = 513: M = 8, lanes 0, 1
and 62 hold eight rows and lane 63 seven (31 targets).  The well is taken 0.7 grid rows wide and 30 deep instead of 6 and 0.3: the
mode then sits on ONE grid point (its neighbours carry about 4 % of it), also next to the ends, where the wide well's mode peaks 4
to 6 points inside; the twist row is the largest f |u w|, which is the largest |X| (f is constant on these lines).  Each case
asserts from X that |X| peaks on its target: the pick has then been taken from every slot of those four lanes.

Tolerances: none; gam, lam, info, X, dX and d gam / d theta0 carry equal bits in both forms."""
import functools

import numpy as np
import pytest

from tests import edge_cases as ec
from tests.test_gpu_scan_resident import both_forms, same_bits

pytestmark = pytest.mark.gpu

SIZES = [131, 513]
LANES = [0, 1, 62, 63]
THETA0 = np.array([0.0, 0.5])
WELL = dict(wr=0.7, depth=30.0)


@pytest.fixture(scope="module")
def ctx():
    import ibs_amd
    c = ibs_amd.Context(0)
    c.set_option("force_p", 64)
    yield c
    c.reset_options()
    c.close()


def slot_targets(N):
    """[(lane, slot, grid point)] of every row lanes 0, 1, 62 and 63 hold"""
    n = N - 2
    out = []
    for L in LANES:
        a, b = ec.lane_rows_start(L, n), ec.lane_rows_start(L + 1, n)
        out += [(L, i, a + i + 1) for i in range(b - a)]
    return out


@functools.lru_cache(maxsize=None)
def lines(N):
    """(h, seven geometry arrays (n_targets, N), dPdrho (n_targets,), targets): one moving-well line per target"""
    th = ec.theta_grid(N)
    tg = slot_targets(N)
    geo = [ec.to_geometry(*ec.well_rows(th, j, **WELL)) for _, _, j in tg]
    arrays = tuple(np.ascontiguousarray(np.stack([g[k] for g in geo])) for k in range(7))
    return float(th[1] - th[0]), arrays, np.full(len(tg), -1.0), tg


def test_targets_are_every_slot_of_the_four_lanes():
    M = {N: ec.rows_per_lane(N) for N in SIZES}
    assert M == {131: 3, 513: 8}
    for N in SIZES:
        tg = slot_targets(N)
        per = {L: [i for l, i, _ in tg if l == L] for L in LANES}
        full = [L for L in LANES if per[L] == list(range(M[N]))]
        assert all(per[L] in (list(range(M[N])), list(range(M[N] - 1))) for L in LANES), (N, per)
        assert full == ([0] if N == 131 else [0, 1, 62]), (N, per)          # (lane 63 never holds the last slot: N - 2 < 64 M)
        assert [j for _, _, j in tg][:M[N]] == list(range(1, M[N] + 1)) and tg[-1][2] == N - 2, (N, tg)


@pytest.mark.parametrize("N", SIZES)
def test_resident_pick_equals_the_select_chain_on_every_slot(ctx, N):
    import torch
    dev = torch.device("cuda:0")
    h, arrays, dP, tg = lines(N)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    geo, dP_d, t0 = [up(a) for a in arrays], up(dP), up(THETA0)
    call = lambda: ctx.gamma_scan(h, *geo, dP_d, t0, want_X=True, want_dtheta0=True, want_info=True)
    r, l = both_forms(ctx, N, call)
    peak = r["X"].abs().argmax(dim=2).cpu().numpy()
    want = np.array([j for _, _, j in tg])
    print(N, "targets", want.tolist(), "peaks", peak[:, 0].tolist())
    assert np.array_equal(peak[:, 0], want) and np.array_equal(peak[:, 1], want), (N, peak.T, want)
    assert bool(torch.isfinite(r["gam"]).all()) and bool(torch.isfinite(r["X"]).all())
    same_bits(N, "twist pick", r, l, ("gam", "lam", "info", "X", "dX", "dgam_dtheta0"))
    for k in ("gam", "lam", "X", "dX", "dgam_dtheta0"):                   # (torch.equal holds -0.0 equal to 0.0: the integer view does not)
        assert torch.equal(r[k].view(torch.int64), l[k].view(torch.int64)), (N, k)
