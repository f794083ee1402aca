"""GPU: the resident scan kernel's forward sweep counts from one word of sign bits and answers min(count, 2) from two ballots
(WaveSolver::sweep_fwd_min2, csrc/ibs_sweep_count.hpp), and its scan fetches the row_bcast factors without a fill; the lean form
(k_gamma_scan_lean) still runs the row-by-row count and the filled fetches.  Every decision and every floating-point operation is
meant to be the same, so the two forms must agree in every bit of gam, lam and info (info holds the number of sweeps of each solve).

1. The row-ownership edges of M = 4 .. 7 -- the lengths at which exactly 1 and exactly 63 lanes own a last row (the per-lane mask
   has three values: full chunk, short chunk, lane 63) -- which tests/test_gpu_scan_resident.py reaches for M = 3 and 8 only.
2. Counts of 2 and more, and of 0, on purpose (N = 131 and 513): warm starts far below lam_max (half way to the lower Gershgorin
   end, -||A||: the first shifts have several eigenvalues above them) and above it (half way to the upper Gershgorin end,
   max c / f: the first shift, the shift below the guess and the bisection steps that follow all count 0).  info & 0xffff must
   differ from the cold scan's, so that the cases cannot pass by never leaving the usual path.
3. The resident form against the C oracle at the new lengths.

Geometry, helpers and tolerances are those of tests/test_gpu_scan_resident.py: 4 golden NCSX lines x 5 theta0, interpolated onto
the shorter grids; resident against lean: equal bits; against the oracle: check_scan of tests/test_gpu_edge_lengths.py (gam 1e-10,
lam 4 N eps ||A||)."""
import numpy as np
import pytest

from oracle import ballooning_oracle as bo
from tests.test_gpu_edge_lengths import check_scan
from tests.test_gpu_scan_resident import THETA0, both_forms, ctx, inputs, on_device, reference, rows_per_lane, same_bits  # noqa: F401

pytestmark = pytest.mark.gpu

# (N, M, lanes that own a last row)
EDGES = [(195, 4, 1), (257, 4, 63), (259, 5, 1), (321, 5, 63), (323, 6, 1), (385, 6, 63), (387, 7, 1), (449, 7, 63)]
KEYS = ("gam", "lam", "info")


@pytest.mark.parametrize("N,M,full", EDGES)
def test_row_ownership_edges_resident_equals_lean(ctx, N, M, full):
    assert rows_per_lane(N) == M and (N - 2) - 64 * (M - 1) == full
    h, geo, dP, t0 = on_device(N)
    r, l = both_forms(ctx, N, lambda: ctx.gamma_scan(h, *geo, dP, t0, want_info=True))
    assert int((r["info"] >> 16).abs().max()) == 0, (N, r["info"] >> 16)
    same_bits(N, "plain", r, l, KEYS)
    plain = r
    r, l = both_forms(ctx, N, lambda: ctx.gamma_scan(h, *geo, dP, t0, want_info=True, lam_guess=plain["lam"], guess_width=1e-3))
    same_bits(N, "warm", r, l, KEYS)


@pytest.mark.parametrize("N,M,full", EDGES)
def test_row_ownership_edges_against_the_c_oracle(ctx, N, M, full):
    h, a, dP = inputs(N)
    try:
        ctx.set_option("scan_resident", 1)
        r = ctx.gamma_scan(h, *a, dP, THETA0, want_info=True)
        assert ctx.last_launch()[0] == "ibs::k_gamma_scan<double, %d>" % M, ctx.last_launch()
    finally:
        ctx.set_option("scan_resident", None)
    assert r["nbad"] == 0 and not ((r["info"] >> 16) & 3).any(), (N, r["info"] >> 16)
    check_scan(N, "resident", r, reference(N))


def upper_gershgorin(N):
    """max c / f over the interior grid points of every (line, theta0) system: WaveSolver::setup's upper end of the bracket"""
    h, a, dP = inputs(N)
    out = np.zeros((len(dP), len(THETA0)))
    for i in range(len(dP)):
        for j, t in enumerate(THETA0):
            cv, gd = bo.fold_theta0(t, *[a[k][i] for k in range(2, 7)])
            g, c, f = bo.gcf(dP[i], a[0][i], a[1][i], cv, gd)
            out[i, j] = (c[1:-1] / f[1:-1]).max()
    return out


@pytest.mark.parametrize("N", [131, 513])
def test_counts_of_two_and_more_and_of_zero(ctx, N):
    import torch
    h, geo, dP, t0 = on_device(N)
    scan = lambda **kw: ctx.gamma_scan(h, *geo, dP, t0, want_info=True, **kw)
    cold, cold_l = both_forms(ctx, N, lambda: scan())
    same_bits(N, "cold", cold, cold_l, KEYS)
    lam = cold["lam"]
    nA = torch.from_numpy(reference(N)[5]).to(lam.device)
    top = torch.from_numpy(upper_gershgorin(N)).to(lam.device)
    assert bool((top - lam > 4e-3).all())                 # (guess - width > lam_max, and guess + width inside the solver's bracket)
    sweeps = lambda r: (r["info"] & 0xffff)
    for tag, guess in (("far below", lam - 0.5 * (lam + nA)), ("above", lam + 0.5 * (top - lam))):
        r, l = both_forms(ctx, N, lambda: scan(lam_guess=guess.contiguous(), guess_width=1e-3))
        print("sweep-count figures: N=%d %s  sweeps %s  cold %s" % (N, tag, sweeps(r).flatten().tolist(), sweeps(cold).flatten().tolist()))
        assert int((r["info"] >> 16).abs().max()) == 0, (N, tag, r["info"] >> 16)
        same_bits(N, tag, r, l, KEYS)
        assert not torch.equal(sweeps(r), sweeps(cold)) and int(sweeps(r).sum()) != int(sweeps(cold).sum()), (N, tag)
        # the same eigenvalue all the same: both are certified to 4 x 64 eps ||A|| (solve(): tol = 64 eps ||A||)
        assert bool(((r["lam"] - lam).abs() <= 512 * 2.220446049250313e-16 * nA).all()), (N, tag)
