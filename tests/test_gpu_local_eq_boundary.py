"""GPU: the local-equilibrium boundaries (ibs_local_eq_boundary_f64, csrc/ibs_local_eq_boundary.hip; Context.local_eq_boundary,
BallooningScan.local_eq_boundary) against the C oracle on rows formed by ibs_amd.local_eq_fold at ibs_amd.local_eq_ray_triples(rays, t)
(tests/local_eq_boundary_cases.py, tests/local_eq_cases.py).

Every verdict compared with the oracle is compared where the oracle's lam_max is farther from the shift than the project's count
margin 16 N^2 eps ||A||, asserted on the oracle side.  The margin grows as N^4 on a fixed theta window: on the default grid it passes
|lam_max| at t* -+ 1e-5 (t_hi - t_lo) between N = 361 and N = 721, so the root property is tested at N = 67 and at N = 361 = the kernel's
chunk of 360 grid points + 1, and the three-chunk length N = 771 is compared node by node where the margin allows."""
import os

import numpy as np
import pytest

from ibs_amd import local_eq_ray_nodes, local_eq_ray_triples
from oracle import ballooning_oracle as bo
from tests import local_eq_boundary_cases as bc
from tests import local_eq_cases as lc

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(__file__), "golden")
DELTA = 1e-5
XTOL = 1e-12
KEYS = ("t_stable", "t_unstable", "n_cross", "lo_unstable", "node_count", "info")


@pytest.fixture(scope="module")
def ctx():
    import ibs_amd
    return ibs_amd.Context(0)


def run(ctx, b, rays, **kw):
    kw = dict(dict(ps=b["ps"], shift=0.0, xtol=XTOL, want_nodes=True, want_info=True), **kw)
    return ctx.local_eq_boundary(*bc.call_args(b), rays, **kw)


def same_bits(a, b, what):
    for k in KEYS:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=np.asarray(a[k]).dtype.kind == "f"), (what, k)


@pytest.fixture(scope="module", params=[67, 361])
def rooted(ctx, request):
    """the three s-alpha base lines x the six rays of bc.RAYS at N = 67 and 361: the device result and the oracle at the 64 nodes,
    computed once for tests 1 and 3"""
    N = request.param
    b = bc.salpha_lines(bo.theta_grid(N))
    r = run(ctx, b, bc.RAYS)
    assert "k_local_eq_boundary" in ctx.last_launch()[0], ctx.last_launch()
    return N, b, r, bc.oracle_nodes(b, bc.RAYS)


def test_root_property_and_completeness(rooted):
    """1. every returned crossing has the oracle's lam_max below 0 at the stable side's t -+ D and above it at the other, D = 1e-5 of
    the range, both outside the count margin; the bracket is within xtol of the range or bit 3 is set; bits 0-2 are clear; n_cross,
    lo_unstable and the flip positions are those of the oracle's verdicts at the 64 nodes, none of which lies within the margin.
    Oracle side, measured on the CPU: N = 67: 9 crossings per line (2, 2, 1, 1 on the p-rays, 2 on the eps-ray, 1 on the oblique ray),
    min |lam| at t -+ D 2.9e-7 = 640 margins, nodes at least 5.7e4 margins away; N = 361: 7 per line (the shat = 0.1 ray is stable
    throughout on this window), 2.3e-6 = 6.2 margins, nodes at least 16.8 margins away."""
    N, b, r, nd = rooted
    rays = bc.RAYS
    st = bc.status(r)
    print("N=%d: passes per system %s, status %s" % (N, (r["info"] & 0xffff).tolist(), np.unique(st).tolist()))
    assert r["nbad"] == 0 and not (st & 7).any(), st
    node_ratio = (np.abs(nd["lam"]) / nd["margin"]).min()
    print("N=%d: min |lam| / margin over the nodes %.2e" % (N, node_ratio))
    assert node_ratio > 1.0
    bc.check_sides(b, rays, r, delta=DELTA, what="s-alpha N=%d" % N)
    width = np.abs(r["t_unstable"] - r["t_stable"])
    rng = (rays[:, 6] - rays[:, 5])[None, :, None]
    have = np.isfinite(width)
    print("N=%d: max bracket width / range %.2e" % (N, (width / rng)[have].max()))
    assert ((width <= XTOL * rng) | ((st & 8) != 0)[:, :, None])[have].all()
    unst = nd["count"] > 0
    assert np.array_equal(r["lo_unstable"], unst[:, :, 0].astype(np.int32))
    for i in range(unst.shape[0]):
        for k in range(unst.shape[1]):
            fl = bc.flips(unst[i, k])
            assert r["n_cross"][i, k] == len(fl) <= 4, (i, k, fl)
            tm = 0.5 * (r["t_stable"][i, k] + r["t_unstable"][i, k])[:len(fl)]
            assert ((nd["t"][i, k, fl] < tm) & (tm < nd["t"][i, k, fl + 1])).all(), (i, k, fl, tm)
            up = r["t_stable"][i, k, :len(fl)] < r["t_unstable"][i, k, :len(fl)]
            assert np.array_equal(up, ~unst[i, k, fl]), (i, k)
    assert (r["n_cross"] > 0).sum() >= 15                     # (15 of 18 systems cross at either length)


def test_consistent_with_the_scan_on_the_device(ctx, rooted):
    """3. node_count is Context.local_eq_scan(count_only=True)'s count at the node triples, and the scan's verdicts at t -+ D of every
    crossing are the reported sides (integers; the margins of test 1 cover them)"""
    N, b, r, nd = rooted
    rays = bc.RAYS
    var = local_eq_ray_triples(rays[:, None, :], local_eq_ray_nodes(rays)).reshape(-1, 3)
    sc = ctx.local_eq_scan(*bc.call_args(b), var, ps=b["ps"], shift=0.0, count_only=True)["count"]
    assert np.array_equal(r["node_count"], sc.reshape(3, len(rays), 64))      # (the rays, like the triples, are shared by the lines)
    assert np.array_equal(r["node_count"], nd["count"])
    side = bc.check_sides(b, rays, r, delta=DELTA, what="s-alpha N=%d (sides for the scan)" % N)      # (3, n_ray, 4, 2)
    have = np.isfinite(side[..., 0])
    q = np.where(np.isfinite(side), side, 0.5 * (rays[:, 5] + rays[:, 6])[None, :, None, None])
    for i in range(3):
        var = local_eq_ray_triples(rays[:, None, :], q[i].reshape(len(rays), -1)).reshape(-1, 3)
        one = {k: b[k][i:i + 1] for k in ("lines", "dP", "centre", "sigma", "ps")}
        cnt = ctx.local_eq_scan(*bc.call_args(dict(one, th=b["th"])), var, ps=one["ps"], shift=0.0, count_only=True)["count"]
        cnt = cnt.reshape(len(rays), 4, 2)
        assert (cnt[..., 0][have[i]] == 0).all() and (cnt[..., 1][have[i]] > 0).all(), i


def test_three_chunks_node_by_node(ctx):
    """1b. N = 771 = two chunks of 360 grid points + 51: the counts at the nodes against the oracle's at every node whose lam_max lies
    outside the count margin (the margin passes |lam| at t* -+ D here, so no root property); measured on the CPU: at least 0.63 margins
    at every node of these rays, so only a few nodes drop out -- at least 90 % must remain.  Bits 0-2 clear; every crossing lies between
    two nodes with different device verdicts"""
    b = bc.salpha_lines(bo.theta_grid(771))
    r = run(ctx, b, bc.RAYS)
    nd = bc.oracle_nodes(b, bc.RAYS)
    ok = np.abs(nd["lam"]) > nd["margin"]
    print("N=771: %.1f %% of the nodes outside the margin, passes %s" % (100.0 * ok.mean(), np.unique(r["info"] & 0xffff).tolist()))
    assert ok.mean() >= 0.9 and r["nbad"] == 0 and not (bc.status(r) & 7).any()
    assert np.array_equal(r["node_count"][ok], nd["count"][ok])
    unst = r["node_count"] > 0
    for i in range(3):
        for k in range(len(bc.RAYS)):
            fl = bc.flips(unst[i, k])
            tm = 0.5 * (r["t_stable"][i, k] + r["t_unstable"][i, k])[:len(fl)]
            assert r["n_cross"][i, k] == len(fl) and ((nd["t"][i, k, fl] < tm) & (tm < nd["t"][i, k, fl + 1])).all(), (i, k)


def test_reference_stability_table(ctx):
    """2. N = 401 on theta in [-20 pi, 20 pi] (check_ball_long, column 4 of G2_salpha_stability.npz): three base lines at theta0 = 0, 0.1,
    0.2, p-rays over alpha in [0.1, 1.5] (t = alpha / 0.5) at the table's ten shat.  Every crossing lies strictly between two adjacent
    alpha nodes of the table whose verdicts differ, every such pair holds exactly one crossing, lo_unstable is the table's verdict at
    alpha = 0.1.  (numpy oracle at theta0 = 0: alpha* = 0.2816 and 0.7180 at shat = 0.1, 0.3371 and 1.2635 at 0.3, 0.5689 at 0.9, 1.1352
    at 1.9.)"""
    tab = np.load(os.path.join(G, "G2_salpha_stability.npz"))["table"]
    th = np.linspace(-20 * np.pi, 20 * np.pi, 401)
    t0s, shats, alphas = np.unique(tab[:, 2]), np.unique(tab[:, 0]), np.unique(tab[:, 1])
    assert len(t0s) == 3 and len(shats) == 10 and len(alphas) == 8 and alphas[0] == 0.1 and alphas[-1] == 1.5
    b = bc.salpha_lines(th, tuple(t0s))
    rays = np.array([(0.0, sh - 1.0, 0.0, 0.0, 1.0, alphas[0] / 0.5, alphas[-1] / 0.5) for sh in shats])
    r = run(ctx, b, rays)
    assert r["nbad"] == 0 and not (bc.status(r) & 7).any()
    alpha_star = 0.5 * r["t"]
    for i, t0 in enumerate(t0s):
        for k, sh in enumerate(shats):
            rows = tab[(tab[:, 2] == t0) & (tab[:, 0] == sh)]
            rows = rows[np.argsort(rows[:, 1])]
            assert np.array_equal(rows[:, 1], alphas)
            verdict = rows[:, 4].astype(bool)
            fl = bc.flips(verdict)
            assert r["lo_unstable"][i, k] == int(verdict[0]), (t0, sh)
            got = alpha_star[i, k, :r["n_cross"][i, k]]
            assert len(got) == len(fl), (t0, sh, got, fl)
            assert ((alphas[fl] < got) & (got < alphas[fl + 1])).all(), (t0, sh, got, alphas[fl])
    print("alpha* at theta0 = 0: " + "; ".join("shat %.1f: %s" % (sh, np.round(alpha_star[0, k, :r["n_cross"][0, k]], 4).tolist())
                                              for k, sh in enumerate(shats)))
    for k, want in ((0, (0.2816, 0.7180)), (1, (0.3371, 1.2635)), (4, (0.5689,)), (9, (1.1352,))):
        assert np.isclose(shats[k], (0.1, 0.3, 0.9, 1.9)).any()
        assert np.abs(alpha_star[0, k, :len(want)] - np.array(want)).max() <= 1e-4, (k, alpha_star[0, k])


def reuse_rays(waves):
    """the product grid of lc.wave_reuse_batch turned into p-rays: the triple (theta0, eps, p) becomes the ray folded at theta0 along the
    pressure axis at eps over t in [0.2 + 0.1 p, 3 + 0.2 p]"""
    b = lc.wave_reuse_batch(waves)
    v = b["var"]
    zero, one = np.zeros(len(v)), np.ones(len(v))
    return b, np.stack([v[:, 0], v[:, 1], zero, zero, one, 0.2 + 0.1 * v[:, 2], 3.0 + 0.2 * v[:, 2]], axis=1)


def test_wave_reuse_and_independence_of_the_batch(ctx):
    """4. more (line, ray) systems than the persistent grid has waves (N = 67, three lines x at least 900 p-rays): the kernel ran on
    fewer blocks than systems, and the outputs of a subset of systems run alone, with the lines in reversed order, are bitwise their
    values in the big batch; so are those of the batch worked through in chunks of whole lines"""
    b, rays = reuse_rays(lc.persistent_waves())
    big = run(ctx, b, rays)
    n_sys = big["n_cross"].size
    lc.assert_wave_reuse(ctx, "k_local_eq_boundary", n_sys)
    assert n_sys >= 1.3 * lc.persistent_waves() and big["nbad"] == 0 and not (bc.status(big) & 3).any()
    print("wave reuse: %d systems, crossings per system %s" % (n_sys, np.bincount(big["n_cross"].ravel()).tolist()))
    assert (big["n_cross"] == 1).mean() > 0.5 and (big["n_cross"] == 2).mean() > 0.1      # (the oracle at the nodes, on the CPU: 78 % and 22 % at 2,700 systems)
    pick = np.array([3, 17, 400, len(rays) - 1, 250])
    order = [2, 0]
    sub = {k: b[k][order] for k in ("lines", "dP", "centre", "sigma", "ps")}
    small = run(ctx, dict(sub, th=b["th"]), rays[pick])
    same_bits(small, {k: big[k][order][:, pick] for k in KEYS}, "subset")
    ctx.set_option("nearest_chunk_systems", len(rays))     # (chunks of one line: three launches)
    try:
        chunked = run(ctx, b, rays)
    finally:
        ctx.set_option("nearest_chunk_systems", None)
    same_bits(chunked, big, "chunks of whole lines")


def raw_boundary(ctx, n_lines, n_ray, N, lo, h, geo, ld, dP, centre, sigma, ps, ps_ld, rays, shift, max_cross, xtol, device):
    """ibs_local_eq_boundary_f64 itself on the caller's leading dimensions, host or device pointers -> (return value, outputs)"""
    import ctypes
    import torch
    shape = (n_lines, n_ray)
    ins = [np.ascontiguousarray(a, dtype=np.float64) for a in (geo, dP, centre, sigma, ps, rays)]
    out = dict(t_stable=np.zeros(shape + (max_cross,)), t_unstable=np.zeros(shape + (max_cross,)), n_cross=np.zeros(shape, np.int32),
               lo_unstable=np.zeros(shape, np.int32), node_count=np.zeros(shape + (64,), np.int32), info=np.zeros(shape, np.int32))
    if device:
        ctx._stream_from_torch(torch.device("cuda:0"))
        ins = [torch.from_numpy(a).to("cuda:0") for a in ins]
        out = {k: torch.from_numpy(v).to("cuda:0") for k, v in out.items()}
        p = lambda a: ctypes.c_void_p(a.data_ptr())
    else:
        p = lambda a: ctypes.c_void_p(a.ctypes.data)
    rc = ctx._lib.ibs_local_eq_boundary_f64(ctx._h, n_lines, n_ray, N, float(lo), float(h), p(ins[0]), ld, p(ins[1]), p(ins[2]), p(ins[3]),
                                            p(ins[4]), ps_ld, p(ins[5]), float(shift), max_cross, float(xtol), p(out["t_stable"]),
                                            p(out["t_unstable"]), p(out["n_cross"]), p(out["lo_unstable"]), p(out["node_count"]),
                                            p(out["info"]), 0 if device else 1)
    if device:
        torch.cuda.synchronize()
        out = {k: v.cpu().numpy() for k, v in out.items()}
    return rc, out


def test_padded_rows_and_invalid_data(ctx):
    """5. N = 67, four lines (theta0 = 0, 0.1, -0.3, 0.2) x the six rays + one ray with t_lo = t_hi and one with t_lo > t_hi.  ld = N + 5
    and ps_ld = N + 3 with NaN in every padding element through the raw entry, host and device pointers: the packed call's bits.  A NaN
    in the middle of line 1, sigma = 0 on line 2 and the two bad rays: status bit 1, NaN parameters, n_cross -1 on exactly those systems
    (and on the bad rays in the clean run), every other system bitwise the clean run's"""
    N = 67
    b = bc.salpha_lines(bo.theta_grid(N), bc.T0S + (0.2,))
    rays = np.concatenate([bc.RAYS, [(0.0, 0.0, 0.0, 0.0, 1.0, 1.5, 1.5), (0.0, 0.0, 0.0, 0.0, 1.0, 2.0, 1.0)]])
    clean = run(ctx, b, rays)
    hit = np.zeros((4, len(rays)), dtype=bool)
    hit[:, 6:] = True

    def check_hit(r, hit, what):
        st = bc.status(r)
        assert (st[hit] == 2).all() and not (st[~hit] & 3).any(), (what, st)
        assert np.isnan(r["t_stable"][hit]).all() and np.isnan(r["t_unstable"][hit]).all() and np.isnan(r["t"][hit]).all(), what
        assert (r["n_cross"][hit] == -1).all() and (r["n_cross"][~hit] >= 0).all(), what
        assert r["nbad"] == hit.sum(), (what, r["nbad"])

    check_hit(clean, hit, "clean lines, two bad rays")
    assert (clean["n_cross"][~hit] > 0).all()
    lo, h, geo = bc.call_args(b)[:3]
    geo_p, ps_p = np.full((8, 4, N + 5), np.nan), np.full((4, N + 3), np.nan)
    geo_p[:, :, :N], ps_p[:, :N] = geo, b["ps"]
    for device in (False, True):
        rc, r = raw_boundary(ctx, 4, len(rays), N, lo, h, geo_p, N + 5, b["dP"], b["centre"], b["sigma"], ps_p, N + 3, rays, 0.0, 4, XTOL, device)
        assert "k_local_eq_boundary" in ctx.last_launch()[0]
        assert rc == (0 if device else hit.sum()), (device, rc)      # (host pointers: the count of flagged systems)
        same_bits(r, clean, "padded rows, device pointers %s" % device)
    bad = dict(b, lines=b["lines"].copy(), sigma=b["sigma"].copy())
    bad["lines"][1, 5, 33] = np.nan
    bad["sigma"][2] = 0.0
    hit[1] = hit[2] = True
    r = run(ctx, bad, rays)
    check_hit(r, hit, "NaN line, sigma = 0, two bad rays")
    same_bits({k: r[k][~hit] for k in KEYS}, {k: clean[k][~hit] for k in KEYS}, "neighbours of the invalid systems")
    assert (r["lo_unstable"][hit] == -1).all() and (r["node_count"][hit] == -1).all()


def test_max_cross_truncation(ctx):
    """6. the shat = 0.3 p-ray (two crossings) with max_cross = 1: the first crossing, bitwise that of the max_cross = 4 run, bit 2 set;
    the one-crossing shat = 0.9 ray beside it has bit 2 clear"""
    b = bc.salpha_lines(bo.theta_grid(67))
    rays = bc.RAYS[1:3]
    four, one = run(ctx, b, rays), run(ctx, b, rays, max_cross=1)
    assert (four["n_cross"] == [2, 1]).all() and (one["n_cross"] == 1).all()
    assert one["t_stable"].shape == (3, 2, 1)
    for k in ("t_stable", "t_unstable", "t"):
        assert np.array_equal(one[k][:, :, 0], four[k][:, :, 0]), k
    assert np.array_equal(one["lo_unstable"], four["lo_unstable"]) and np.array_equal(one["node_count"], four["node_count"])
    assert np.array_equal(bc.status(one) & 4, [[4, 0]] * 3) and not (bc.status(four) & 4).any() and one["nbad"] == 0


def test_xtol_zero_closes_to_fp64_neighbours(ctx):
    """6b. xtol = 0 on the shat = 0.3 and shat = 0.9 p-rays at N = 67: the closing stops when no point lies strictly inside the bracket
    -- the two ends are neighbours in FP64 --, sets bit 3 and no other, within the pass cap (0.044 / 65^8 is below an ulp); the brackets
    lie inside those of the xtol = 1e-12 run"""
    b = bc.salpha_lines(bo.theta_grid(67))
    rays = bc.RAYS[1:3]
    loose, tight = run(ctx, b, rays), run(ctx, b, rays, xtol=0.0)
    have = np.isfinite(loose["t"])
    assert np.array_equal(tight["n_cross"], loose["n_cross"]) and np.array_equal(np.isfinite(tight["t"]), have) and tight["nbad"] == 0
    assert (bc.status(tight) == 8).all() and not bc.status(loose).any()
    ts, tu = tight["t_stable"][have], tight["t_unstable"][have]
    assert np.array_equal(np.nextafter(ts, tu), tu)
    lo, hi = np.minimum(loose["t_stable"], loose["t_unstable"])[have], np.maximum(loose["t_stable"], loose["t_unstable"])[have]
    assert ((lo <= np.minimum(ts, tu)) & (np.maximum(ts, tu) <= hi)).all()
    print("xtol = 0: passes %s against %s at xtol = 1e-12" % ((tight["info"] & 0xffff).tolist(), (loose["info"] & 0xffff).tolist()))


def test_host_pointers(ctx):
    """7. IBS_MEM_HOST numpy inputs give bitwise the device-tensor results (N = 361, the six rays)"""
    import torch
    dev = torch.device("cuda:0")
    b = bc.salpha_lines(bo.theta_grid(361))
    host = run(ctx, b, bc.RAYS)
    lo, h, geo, dP, centre, sigma = bc.call_args(b)
    d = ctx.local_eq_boundary(lo, h, torch.from_numpy(geo).to(dev), torch.from_numpy(dP).to(dev), centre, sigma, bc.RAYS,
                              ps=torch.from_numpy(b["ps"]).to(dev), shift=0.0, xtol=XTOL, want_nodes=True, want_info=True)
    assert isinstance(host["t"], np.ndarray) and d["t"].is_cuda
    same_bits({k: d[k].cpu().numpy() for k in KEYS}, host, "device tensors")
    assert np.array_equal(d["t"].cpu().numpy(), host["t"], equal_nan=True)


# the pressure range of the driver test, from BallooningScan.local_eq(eps = (-0.5, 0), p = linspace(0, 8, 33), count_only=True) on this
# fixture, run once on an MI355X: see the test's docstring
P_RANGE = (0.0, 3.0)


def test_scan_driver_boundary_on_ncsx_tables(ctx):
    """8. BallooningScan.local_eq_boundary on the G8 wout tables: 2 surfaces x 3 alpha x 2 theta0 x 2 eps at N = 513 (the N of the
    local_eq driver test), p-rays over P_RANGE.  The raw arrays are a direct Context.local_eq_boundary call's on the same geometry,
    first_unstable is the numpy reduction (ibs_amd.first_unstable, pinned on the CPU), and the scan's verdicts at first_unstable -+ D on
    the line that attains it are stable and unstable.  At least one line must cross.  P_RANGE = (0, 3): the count_only raster of
    BallooningScan.local_eq on this fixture over p = linspace(0, 8, 33) has every one of the 24 (line, theta0, eps) rows stable up to
    p = 0.75 at least and unstable from p = 1.5 on at the latest, with one flip each -- all rows cross inside (0, 3)."""
    import torch
    import ibs_amd
    dev = torch.device("cuda:0")
    N = 513
    th = np.linspace(-4 * np.pi, 4 * np.pi, N)
    svals = np.array([0.6, 0.9])
    tabs = ibs_amd.SurfaceTables.from_wout(dict(np.load(os.path.join(G, "G8_wout_ncsx_op.npz"))), svals)
    scan = ibs_amd.BallooningScan(ctx, None, th, svals, nalpha=3, ntheta0=2, tables=tabs, device=dev)
    eps = np.array([-0.5, 0.0])
    r = scan.local_eq_boundary(eps, P_RANGE)
    shape = (2, 3, 2, 2)
    for k in ("t_stable", "t_unstable", "t"):
        assert r[k].shape == shape + (4,), k
    for k in ("n_cross", "lo_unstable", "info"):
        assert r[k].shape == shape and r[k].dtype == np.int32, k
    assert r["first_unstable"].shape == (2, 2) and r["axis"] == "p" and np.array_equal(r["fixed"], eps)
    print("driver: n_cross %s, first_unstable %s" % (r["n_cross"].ravel().tolist(), r["first_unstable"].tolist()))
    assert (r["n_cross"] > 0).any()
    # the same geometry, directly (with the driver's own h: (theta[-1] - theta[0]) / (N - 1) is not theta[1] - theta[0] bit for bit)
    surf, alpha = np.repeat(np.arange(2), 3), np.tile(scan.alpha_scan, 2)
    geo = ctx.fieldline_geometry(tabs, surf, alpha, th, device=dev)
    sigma = np.sign(-np.asarray(tabs.scal)[surf, 4])
    t0 = scan.theta0_scan
    tt, ee = (a.ravel() for a in np.meshgrid(t0, eps, indexing="ij"))
    zero, one = np.zeros(4), np.ones(4)
    rays = np.stack([tt, ee, zero, zero, one, np.full(4, P_RANGE[0]), np.full(4, P_RANGE[1])], axis=1)
    d = ctx.local_eq_boundary(th[0], scan.h, geo["geo"], geo["dPdrho"], alpha, sigma, rays, want_info=True)
    for k in ("t_stable", "t_unstable", "t"):
        assert np.array_equal(d[k].cpu().numpy().reshape(shape + (4,)), r[k], equal_nan=True), k
    for k in ("n_cross", "lo_unstable", "info"):
        assert np.array_equal(d[k].cpu().numpy().reshape(shape), r[k]), k
    # the envelope
    fu = ibs_amd.first_unstable(r["t_stable"], r["t_unstable"], r["lo_unstable"], P_RANGE[0])
    assert np.array_equal(r["first_unstable"], fu)
    up = r["t_stable"] < r["t_unstable"]
    D = DELTA * (P_RANGE[1] - P_RANGE[0])
    checked = 0
    for s in range(2):
        for k in range(2):
            f = r["first_unstable"][s, k]
            if r["lo_unstable"][s, :, :, k].any():
                assert f == P_RANGE[0]
                continue
            cand = np.where(up[s, :, :, k], r["t"][s, :, :, k], np.inf)
            assert f == cand.min()
            if not np.isfinite(f):
                continue
            ia, it, _ = np.unravel_index(np.argmin(cand), cand.shape)
            line = s * 3 + ia
            var = np.array([(t0[it], eps[k], f - D), (t0[it], eps[k], f + D)])
            cnt = ctx.local_eq_scan(th[0], scan.h, geo["geo"][:, line:line + 1].contiguous(), geo["dPdrho"][line:line + 1],
                                    alpha[line:line + 1], sigma[line:line + 1], var, count_only=True)["count"].cpu().numpy()
            assert cnt[0, 0] == 0 and cnt[0, 1] > 0, (s, k, f, cnt)
            checked += 1
    assert checked >= 1
