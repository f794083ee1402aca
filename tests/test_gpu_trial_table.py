"""GPU: the per-grid trial table of the resident theta0 scan (k_trial_table<double, M> -> k_gamma_scan<double, M>, 3 <= M <= 8).

The start of every lane's trial vector -- x_a, x_{a+1} and 2 cos(pi / (N - 1)) -- depends on the grid length, the rows per lane and
the lane alone.  The Context builds it once per grid length on the device, with the expressions set-up uses, and the resident kernel
loads it; option scan_trial_table = 0 hands the kernel a null table, and every wave computes the values as before.  Both ways must
give the same bits, whatever the cache has seen before.

Shapes: N = 131 (M = 3: lane 0 owns a last row, the other 63 do not), 195 (M = 4: one lane with a last row), 513 (M = 8: 63 lanes
with one) on 1, 8 and 9 lines x 3 theta0 (9 lines: a second chunk of the block map with one live column).  The geometry is the golden
NCSX lines (tests/golden/G3_ncsx_lines.npz), interpolated linearly onto the shorter grids as tests/test_gpu_scan_resident.py does.

Tolerances: none.  Every comparison is of bits, through the integer view."""
import functools
import os

import numpy as np
import pytest

from oracle import ballooning_oracle as bo

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
SIZES = [131, 195, 513]
LINES = [1, 8, 9]
THETA0 = np.array([0.0, 0.7, 1.4])


def rows_per_lane(N):
    return (N - 2 + 63) // 64


@functools.lru_cache(maxsize=None)
def inputs(N):
    """(h, the seven geometry arrays (9, N), dPdrho (9,)) of the first nine golden lines on the N-point grid"""
    g3 = np.load(os.path.join(G, "G3_ncsx_lines.npz"))
    geo, th513, th = g3["geo_513"][:9], bo.theta_grid(513), bo.theta_grid(N)
    if N != 513:
        geo = np.stack([np.stack([np.interp(th, th513, ln[k]) for k in range(8)]) for ln in geo])
    a = tuple(np.ascontiguousarray(geo[:, k, :]) for k in range(7))
    assert (a[0] > 0).all() and (np.abs(a[1]) > 0).all()
    return float(th[1] - th[0]), a, np.ascontiguousarray(g3["dPdrho_513"][:9])


def on_device(N, n_lines, a=None):
    import torch
    dev = torch.device("cuda:0")
    h, a0, dP = inputs(N)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x[:n_lines])).to(dev)
    return h, [up(x) for x in (a0 if a is None else a)], up(dP), torch.from_numpy(THETA0).to(dev)


def new_ctx():
    import ibs_amd
    c = ibs_amd.Context(0)
    c.set_option("scan_resident", 1)
    return c


@pytest.fixture(scope="module")
def ctx():
    c = new_ctx()
    yield c
    c.reset_options()
    c.close()


def bits(t):
    import torch
    t = t.detach().cpu().contiguous()
    return (t.view(torch.int64) if t.dtype == torch.float64 else t).numpy()


def same_bits(tag, r, l, keys=("gam", "lam", "info")):
    for k in keys:
        assert r[k].shape == l[k].shape and np.array_equal(bits(r[k]), bits(l[k])), (tag, k)


def scan(c, N, n_lines, table=True, a=None, **kw):
    """the resident scan of n_lines x 3 theta0, with the table or -- table = False -- with a null table pointer"""
    h, geo, dP, t0 = on_device(N, n_lines, a=a)
    try:
        c.set_option("scan_trial_table", 1 if table else 0)
        r = c.gamma_scan(h, *geo, dP, t0, want_info=True, **kw)
        assert c.last_launch()[0] == "ibs::k_gamma_scan<double, %d>" % rows_per_lane(N), (N, c.last_launch())
    finally:
        c.set_option("scan_trial_table", None)
    return r


@pytest.mark.parametrize("n_lines", LINES)
@pytest.mark.parametrize("N", SIZES)
def test_table_equals_the_in_kernel_values(ctx, N, n_lines):
    """cold and warm-started: gam, lam and info carry the same bits with the table and with a null table pointer"""
    t, k = scan(ctx, N, n_lines), scan(ctx, N, n_lines, table=False)
    assert not ((bits(t["info"]) >> 16) & 3).any(), (N, n_lines)
    assert np.isfinite(t["gam"].cpu().numpy()).all()
    same_bits((N, n_lines, "cold"), t, k)
    warm = dict(lam_guess=k["lam"], guess_width=1e-3)
    tw, kw = scan(ctx, N, n_lines, **warm), scan(ctx, N, n_lines, table=False, **warm)
    same_bits((N, n_lines, "warm"), tw, kw)
    # the table is used again on the second call (cache hit): still the same bits
    same_bits((N, n_lines, "again"), scan(ctx, N, n_lines), t)


def test_cache_keeps_one_table_per_grid_length():
    """N = 131, then 195, then 131 again on one Context: each call equals the call of a fresh Context bit for bit (a stale or
    mixed-up entry would give lane starts of another grid), and equals the in-kernel values"""
    one = new_ctx()
    try:
        for step, N in enumerate((131, 195, 131, 513, 195)):
            r = scan(one, N, 8)
            fresh = new_ctx()
            try:
                same_bits((step, N, "fresh context"), r, scan(fresh, N, 8))
                same_bits((step, N, "in-kernel"), r, scan(fresh, N, 8, table=False))
            finally:
                fresh.close()
    finally:
        one.close()


def test_more_grid_lengths_than_cache_entries():
    """twenty grid lengths through one Context, then the first ones again: an entry that was replaced is rebuilt, never handed out
    for another length"""
    one = new_ctx()
    try:
        sizes = list(range(131, 171, 2))
        ref = {N: scan(one, N, 1, table=False) for N in sizes}
        for N in sizes + sizes[:3]:
            same_bits((N, "replaced entries"), scan(one, N, 1), ref[N])
    finally:
        one.close()


def test_two_contexts_on_two_streams():
    """each Context builds its own table on its own stream, in front of its first launch there; one Context moved to a second
    stream builds a table for that stream as well"""
    import torch
    N = 195
    a, b = new_ctx(), new_ctx()
    try:
        ref = scan(a, N, 9, table=False)
        torch.cuda.synchronize()
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        with torch.cuda.stream(s1):
            ra = scan(a, N, 9)
        with torch.cuda.stream(s2):
            rb = scan(b, N, 9)
            ra2 = scan(a, N, 9)
        torch.cuda.synchronize()
        same_bits("stream 1", ra, ref); same_bits("stream 2", rb, ref); same_bits("moved", ra2, ref)
    finally:
        a.close(); b.close()


@pytest.mark.parametrize("N", SIZES)
def test_a_line_with_nonpositive_g(N):
    """one line whose g is negative at one grid point: status 2 on that line, as with the in-kernel values, on a Context whose
    FIRST launch it is (the table is requested but its values are never consumed by a good solve) -- and the other lines untouched"""
    h, a, dP = inputs(N)
    a = [x.copy() for x in a]
    j = N // 3
    a[4][1, j], a[5][1, j], a[6][1, j] = -1.0, 0.0, 0.0               # gds2 + 2 theta0 gds21 + theta0^2 gds22 = -1 for every theta0
    c = new_ctx()
    try:
        t = scan(c, N, 8, a=a)
        k = scan(c, N, 8, table=False, a=a)
        st = bits(t["info"]) >> 16
        assert (st[1] & 2).all() and not (np.delete(st, 1, axis=0) & 3).any(), (N, st)
        assert np.array_equal(bits(t["info"]), bits(k["info"])), N
        for key in ("gam", "lam"):
            assert np.array_equal(bits(t[key]), bits(k[key])), (N, key)
        good = scan(c, N, 8)
        keep = [0] + list(range(2, 8))
        assert np.array_equal(bits(t["gam"])[keep], bits(good["gam"])[keep]), N
    finally:
        c.close()


@pytest.mark.parametrize("N", SIZES)
def test_fused_surface_maxima(ctx, N):
    """the fused per-surface maximum at 9 lines in 3 surfaces with the table in use: table, pack and status equal the null-pointer
    run, and pack is the first maximum of every surface's block"""
    import torch
    import ibs_amd
    h, geo, dP, t0 = on_device(N, 9)

    def fused(table):
        try:
            ctx.set_option("scan_trial_table", 1 if table else 0)
            plan = ibs_amd.ScanPlan(ctx, h, geo, dP, t0, 3)
            plan.scan_argmax()
            torch.cuda.synchronize()
            assert ctx.last_launch()[0] == "ibs::k_gamma_scan<double, %d>" % rows_per_lane(N), ctx.last_launch()
            return dict(gam=plan.gam.clone(), lam=plan.lam.clone(), info=plan.info.clone(), pack=plan.pack.clone())
        finally:
            ctx.set_option("scan_trial_table", None)
    t, k = fused(True), fused(False)
    same_bits((N, "fused"), t, k, keys=("gam", "lam", "info", "pack"))
    same_bits((N, "fused against plain"), t, scan(ctx, N, 9, table=False), keys=("gam", "lam"))
    per = 3 * len(THETA0)
    for s in range(3):
        blk = t["gam"].reshape(3, per)[s]
        i = int(torch.argmax(blk))
        assert float(t["pack"][s, 0]) == float(blk[i]) and int(t["pack"][s, 1]) == i, (N, s)
