"""GPU: the local-equilibrium boundaries minimised over theta0 (ibs_local_eq_boundary_polish_f64, csrc/ibs_local_eq_boundary_polish.hip;
Context.local_eq_boundary_polish, BallooningScan.local_eq_boundary_envelope and local_eq_boundary_sensitivity(theta0_polish=True)).
The rule is csrc/ibs_local_eq_boundary_polish.hpp's; its host-driven form is ibs_amd.scan.polish_first_up on one-ray
Context.local_eq_boundary(max_cross=1) calls (tests/local_eq_boundary_polish_cases.py), and the kernel must ask for the same points and
return the same bits.  Lines, ray families and the oracle side: tests/local_eq_boundary_cases.py."""
import os

import numpy as np
import pytest

import ibs_amd
from ibs_amd import scan as sc
from oracle import ballooning_oracle as bo
from tests import local_eq_boundary_cases as bc
from tests import local_eq_boundary_polish_cases as pc
from tests import local_eq_cases as lc

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(__file__), "golden")
XTOL = 1e-12
BIT10, BIT11, BIT12 = 1 << 10, 1 << 11, 1 << 12
KEYS = ("theta0", "t", "t_stable", "t_unstable", "node", "n_eval", "lo_unstable", "info", "n_found")


@pytest.fixture(scope="module")
def ctx():
    return ibs_amd.Context(0)


def same_bits(a, b, what, keys=KEYS):
    for k in keys:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=np.asarray(a[k]).dtype.kind == "f"), (what, k)


@pytest.fixture(scope="module", params=[67, 361, 771])
def polished(ctx, request):
    """the three s-alpha base lines x the six families on the four theta0 nodes at N = 67 (one chunk), 361 (chunk + 1) and 771 (three
    chunks): the coarse rows and the kernel's results with one and with two slots, computed once for tests 1 to 3"""
    N = request.param
    b = bc.salpha_lines(bo.theta_grid(N))
    rows = pc.coarse_rows(ctx, b, pc.FAMILIES, pc.THETA0)
    one = pc.run_polish(ctx, b, pc.FAMILIES, pc.THETA0, rows, n_starts=1)
    assert "k_local_eq_boundary_polish" in ctx.last_launch()[0], ctx.last_launch()
    two = pc.run_polish(ctx, b, pc.FAMILIES, pc.THETA0, rows, n_starts=2)
    return N, b, rows, one, two


def test_same_points_same_bits(ctx, polished):
    """1. every slot against the host-driven rule: theta0*, t, t_stable, t_unstable, lo_unstable, n_eval and the status bits 10-12 (and
    0-3) are EQUAL, bit for bit, to ibs_amd.scan.polish_first_up fed by one-ray Context.local_eq_boundary(max_cross=1) calls; the nodes
    and n_found are row_peaks' of -row; slot 0 with one slot is slot 0 with two.  No tolerance."""
    N, b, rows, one, two = polished
    assert one["nbad"] == 0 and two["nbad"] == 0
    n_eval = []
    for i in range(3):
        nodes, n_found = sc.row_peaks(-rows[i], 2)
        assert np.array_equal(two["node"][i], nodes) and np.array_equal(two["n_found"][i], n_found), i
        assert np.array_equal(one["node"][i, :, 0], nodes[:, 0]) and np.array_equal(one["n_found"][i], np.minimum(n_found, 1)), i
        for k, fam in enumerate(pc.FAMILIES):
            for s in range(2):
                if s and n_found[k] < 2:                    # (a slot beyond n_found repeats slot 0)
                    for key in KEYS[:-1]:
                        assert np.array_equal(two[key][i, k, 1], two[key][i, k, 0], equal_nan=True), (i, k, key)
                    continue
                h = pc.host_polish(ctx, b, i, fam, pc.THETA0, rows[i, k], nodes[k, s])
                n_eval.append(h["n_eval"])
                for r in ((one, two) if s == 0 else (two,)):
                    got = dict(theta0=r["theta0"][i, k, s], t=r["t"][i, k, s], t_stable=r["t_stable"][i, k, s],
                               t_unstable=r["t_unstable"][i, k, s], lo_unstable=r["lo_unstable"][i, k, s], n_eval=r["n_eval"][i, k, s],
                               status=pc.status(r)[i, k, s])
                    for key, v in got.items():
                        assert np.array_equal(v, h[key], equal_nan=True), (N, i, k, s, key, v, h[key])
    print("N=%d: %d slots against the host-driven rule, n_eval %s" % (N, len(n_eval), np.bincount(n_eval).tolist()))


def test_root_property_at_the_polished_theta0(polished):
    """2. bc.check_sides on (t_stable, t_unstable) of every slot with the rays rebuilt at theta0 = theta0*: the oracle's lam_max lies on
    the reported sides at t* -+ 1e-5 of the range, farther than the count margin.  N = 67 and 361; at N = 771 the margin passes |lam|
    there, as the boundary tests document, and nothing is asserted."""
    N, b, rows, one, two = polished
    if N == 771:
        return
    for i in range(3):
        th = two["theta0"][i].reshape(-1)                                       # (family, slot)
        rays = pc.rays_at(np.repeat(pc.FAMILIES, 2, axis=0), th)
        ts, tu = two["t_stable"][i].reshape(1, -1, 1), two["t_unstable"][i].reshape(1, -1, 1)
        r = dict(t_stable=ts, t_unstable=tu, n_cross=np.isfinite(ts[:, :, 0]).astype(np.int32))
        assert r["n_cross"].sum() >= 8, (i, r["n_cross"])
        bc.check_sides(pc.one_line(b, i), rays, r, delta=1e-5, what="polished N=%d line %d" % (N, i))


def test_never_above_the_row_and_strictly_below_where_interior(polished):
    """3. t <= T(node) on every slot; on the nine p-ray rows at shat = 0.3, 0.9, 1.9 the best node is interior and t < T(best node) by
    more than 100 xtol (t_hi - t_lo) = 2.8e-10 (the oracle-driven search on the CPU saw at least 9.9e-5)"""
    N, b, rows, one, two = polished
    node_T = np.take_along_axis(rows, two["node"], axis=2)
    assert (two["t"] <= node_T).all() and not (pc.status(two) & 3).any()
    gain = np.empty((3, 3))
    for i in range(3):
        for q, k in enumerate(pc.P_ROWS):
            j = int(np.argmin(rows[i, k]))
            assert j in (1, 2) and one["node"][i, k, 0] == j, (i, k, rows[i, k])
            gain[i, q] = rows[i, k, j] - one["t"][i, k, 0]
            assert pc.THETA0[j - 1] < one["theta0"][i, k, 0] < pc.THETA0[j + 1] and not pc.status(one)[i, k, 0] & (BIT10 | BIT11 | BIT12)
    print("N=%d: gains over the best node %s" % (N, gain.tolist()))
    assert (gain > 100 * XTOL * 2.8).all()


def test_stationarity_by_the_gradient_kernel(ctx):
    """4. N = 67, xtol_theta0 = 1e-4: on every interior result (a two-sided bracket, a point other than the node) d t* / d theta0 from
    Context.local_eq_boundary_grad -- a kernel this search does not run -- is <= 0 at theta0* - 2e-4 and >= 0 at theta0* + 2e-4 (clipped
    to the bracket): Brent stops with both ends of its bracket within 2 xtol_theta0 of theta0* and values there not below the
    minimum's, so a stationary point lies between.  No bit 11, n_eval <= max_eval.  The nine p-ray rows must all be interior."""
    xt = 1e-4
    b = bc.salpha_lines(bo.theta_grid(67))
    rows = pc.coarse_rows(ctx, b, pc.FAMILIES, pc.THETA0)
    r = pc.run_polish(ctx, b, pc.FAMILIES, pc.THETA0, rows, n_starts=1, xtol_theta0=xt, max_eval=32)
    st = pc.status(r)[:, :, 0]
    assert not (st & (3 | BIT11)).any() and (r["n_eval"] <= 32).all()
    interior = ((st & (BIT10 | BIT12)) == 0) & np.isfinite(r["t_stable"][:, :, 0])
    assert interior[:, list(pc.P_ROWS)].all(), interior
    node = r["node"][:, :, 0]
    n_checked = 0
    for i in range(3):
        ks = np.nonzero(interior[i])[0]
        x = r["theta0"][i, ks, 0]
        lo, hi = pc.THETA0[node[i, ks] - 1], pc.THETA0[node[i, ks] + 1]
        rays = np.concatenate([pc.rays_at(pc.FAMILIES[ks], np.maximum(x - 2 * xt, lo)), pc.rays_at(pc.FAMILIES[ks], np.minimum(x + 2 * xt, hi))])
        one = pc.one_line(b, i)
        g = ctx.local_eq_boundary_grad(*bc.call_args(one), rays, ps=one["ps"], shift=0.0, max_cross=1, xtol=XTOL)
        d = g["dt"][0, :, 0, 0].reshape(2, len(ks))
        print("line %d: d t* / d theta0 left %s right %s" % (i, d[0].tolist(), d[1].tolist()))
        assert np.isfinite(d).all() and (d[0] <= 0).all() and (d[1] >= 0).all(), (i, d)
        n_checked += len(ks)
    assert n_checked >= 9


def raw_polish(ctx, b, fam, theta0, t_row, K, device, pad=0, xtol_theta0=1e-5, max_eval=32):
    """ibs_local_eq_boundary_polish_f64 itself, host or device pointers, with the rows of geo and ps padded by `pad` NaN entries"""
    import ctypes
    import torch
    lo, h, geo = bc.call_args(b)[:3]
    n, N = geo.shape[1], geo.shape[2]
    geo_p, ps_p = np.full((8, n, N + pad), np.nan), np.full((n, N + pad + 1), np.nan)
    geo_p[:, :, :N], ps_p[:, :N] = geo, b["ps"]
    shape = (n, len(fam), K)
    ins = [np.ascontiguousarray(a, dtype=np.float64) for a in (geo_p, b["dP"], b["centre"], b["sigma"], ps_p, fam, theta0, t_row)]
    out = dict(theta0=np.zeros(shape), t=np.zeros(shape), t_stable=np.zeros(shape), t_unstable=np.zeros(shape), node=np.zeros(shape, np.int32),
               n_eval=np.zeros(shape, np.int32), lo_unstable=np.zeros(shape, np.int32), info=np.zeros(shape, np.int32),
               n_found=np.zeros(shape[:2], np.int32))
    if device:
        ctx._stream_from_torch(torch.device("cuda:0"))
        ins = [torch.from_numpy(a).to("cuda:0") for a in ins]
        out = {k: torch.from_numpy(v).to("cuda:0") for k, v in out.items()}
        p = lambda a: ctypes.c_void_p(a.data_ptr())
    else:
        p = lambda a: ctypes.c_void_p(a.ctypes.data)
    rc = ctx._lib.ibs_local_eq_boundary_polish_f64(ctx._h, n, len(fam), N, float(lo), float(h), p(ins[0]), N + pad, p(ins[1]), p(ins[2]),
                                                   p(ins[3]), p(ins[4]), N + pad + 1, p(ins[5]), len(theta0), p(ins[6]), p(ins[7]), 0.0, XTOL,
                                                   K, xtol_theta0, max_eval, *[p(out[k]) for k in KEYS], 0 if device else 1)
    if device:
        torch.cuda.synchronize()
        out = {k: v.cpu().numpy() for k, v in out.items()}
    return rc, out


def test_wave_reuse_and_independence_of_the_batch(ctx):
    """5. three lines at N = 67 x enough eps families (p-rays over [0.2, 3], eps across [-0.9, 1]) x one slot to exceed the persistent
    grid 1.3 times, max_eval = 6: the kernel ran on fewer blocks than slots, and every output is bitwise the big batch's with the lines
    in reversed order, in chunks of one line, for eight systems run alone, with padded rows (ld > N, NaN padding) and with host against
    device pointers"""
    waves = lc.persistent_waves()
    nf = -(-int(np.ceil(1.3 * waves)) // 3)
    b = bc.salpha_lines(bo.theta_grid(67))
    eps = np.linspace(-0.9, 1.0, nf)
    fam = np.stack([np.zeros(nf), eps, np.zeros(nf), np.zeros(nf), np.ones(nf), np.full(nf, 0.2), np.full(nf, 3.0)], axis=1)
    rows = pc.coarse_rows(ctx, b, fam, pc.THETA0)
    kw = dict(n_starts=1, max_eval=6)
    big = pc.run_polish(ctx, b, fam, pc.THETA0, rows, **kw)
    n_sys = big["t"].size
    lc.assert_wave_reuse(ctx, "k_local_eq_boundary_polish", n_sys)
    assert n_sys >= 1.3 * waves and big["nbad"] == 0 and (big["n_eval"] <= 6).all()
    print("wave reuse: %d slots, n_eval %s, bit 10 on %d, bit 11 on %d" % (n_sys, np.bincount(big["n_eval"].ravel()).tolist(),
          ((pc.status(big) & BIT10) != 0).sum(), ((pc.status(big) & BIT11) != 0).sum()))
    assert (big["n_eval"] > 0).mean() > 0.5
    order = [2, 1, 0]
    rev = {k: b[k][order] for k in ("lines", "dP", "centre", "sigma", "ps")}
    same_bits(pc.run_polish(ctx, dict(rev, th=b["th"]), fam, pc.THETA0, rows[order], **kw), {k: big[k][order] for k in KEYS}, "reversed lines")
    ctx.set_option("nearest_chunk_systems", nf)            # (chunks of one line: three launches)
    try:
        chunked = pc.run_polish(ctx, b, fam, pc.THETA0, rows, **kw)
    finally:
        ctx.set_option("nearest_chunk_systems", None)
    same_bits(chunked, big, "chunks of whole lines")
    pick = np.array([0, 3, 17, 250, 400, nf // 2, nf - 2, nf - 1])
    for i in (0, 2):
        alone = pc.run_polish(ctx, pc.one_line(b, i), fam[pick], pc.THETA0, rows[i:i + 1, pick], **kw)
        same_bits(alone, {k: big[k][i:i + 1, pick] for k in KEYS}, "eight systems alone, line %d" % i)
    for device in (False, True):
        rc, r = raw_polish(ctx, b, fam, pc.THETA0, rows, 1, device, pad=5, max_eval=6)
        assert rc == 0 and "k_local_eq_boundary_polish" in ctx.last_launch()[0]
        same_bits(r, big, "padded rows, device pointers %s" % device)


def test_the_envelope_does_not_depend_on_the_centre(polished):
    """6. the s-alpha rule's own identity: the varied integrated shear is shat (theta - theta_c + theta0) - alpha (sin theta - sin theta_c),
    so a change of the base line's centre theta_c is a relabelling of theta0 at each p, and the minimum over theta0 of the marginal p is
    the same for the three base lines.  |dt| <= curvature (2 xtol_theta0)^2 + 2 xtol range, the curvature from the coarse row's second
    difference about the best node (the largest of the three lines): with d = |theta0* - minimiser| <= 2 xtol_theta0."""
    N, b, rows, one, two = polished
    xt = 1e-5
    for k in pc.P_ROWS:
        curv = 0.0
        for i in range(3):
            j = int(np.argmin(rows[i, k]))
            curv = max(curv, (rows[i, k, j - 1] - 2 * rows[i, k, j] + rows[i, k, j + 1]) / 0.09)
        t = one["t"][:, k, 0]
        bound = curv * (2 * xt) ** 2 + 2 * XTOL * 2.8
        print("N=%d shat %.1f: t of the three base lines %s, spread %.3e, bound %.3e (curvature %.2f)"
              % (N, pc.FAMILIES[k, 1] + 1, t.tolist(), t.max() - t.min(), bound, curv))
        assert t.max() - t.min() <= bound, (N, k, t)


def test_faults_stay_local(ctx):
    """7. N = 67, four lines x the six families + one with a NaN entry + one with t_lo >= t_hi: a NaN in the middle of line 1, sigma = 0
    on line 2 and the two bad families give status bit 1, NaN outputs, lo_unstable -1 on exactly those slots, the rest are bitwise the
    clean run's.  A NaN in t_row at the only node that is a peak: another node is searched; a row of NaN: n_found 0, node -1, NaN
    outputs, a clean word.  A row with T = t_lo at its best node: zero evaluations and bit 10.  max_eval = 1: bit 11 and a value not
    above the node's."""
    N = 67
    b = bc.salpha_lines(bo.theta_grid(N), bc.T0S + (0.2,))
    fam = np.concatenate([pc.FAMILIES, [(0.0, np.nan, 0.0, 0.0, 1.0, 0.2, 3.0), (0.0, 0.0, 0.0, 0.0, 1.0, 2.0, 1.0)]])
    rows = pc.coarse_rows(ctx, b, pc.FAMILIES, pc.THETA0)
    rows = np.concatenate([rows, np.tile(rows[:, 2:3], (1, 2, 1))], axis=1)       # (the bad families get a usable row)
    clean = pc.run_polish(ctx, b, fam, pc.THETA0, rows, n_starts=2)
    hit = np.zeros((4, len(fam), 2), dtype=bool)
    hit[:, 6:] = True

    def check_hit(r, hit, what):
        st = pc.status(r)
        assert ((st[hit] & 2) != 0).all() and not (st[~hit] & 3).any(), (what, st)
        for k in ("theta0", "t", "t_stable", "t_unstable"):
            assert np.isnan(r[k][hit]).all() and np.isfinite(r[k][~hit] if k in ("theta0", "t") else 0.0).all(), (what, k)
        assert (r["lo_unstable"][hit] == -1).all() and (r["lo_unstable"][~hit] >= 0).all() and r["nbad"] == hit.sum(), what

    check_hit(clean, hit, "clean lines, two bad families")
    bad = dict(b, lines=b["lines"].copy(), sigma=b["sigma"].copy())
    bad["lines"][1, 5, 33] = np.nan
    bad["sigma"][2] = 0.0
    r = pc.run_polish(ctx, bad, fam, pc.THETA0, rows, n_starts=2)
    hit2 = hit.copy()
    hit2[1] = hit2[2] = True
    check_hit(r, hit2, "NaN line, sigma = 0, two bad families")
    same_bits({k: r[k][~hit2] for k in KEYS[:-1]}, {k: clean[k][~hit2] for k in KEYS[:-1]}, "neighbours of the invalid slots", KEYS[:-1])
    assert np.array_equal(r["n_found"], clean["n_found"])
    # NaN in t_row
    one = pc.one_line(b, 0)
    row = rows[:1, 2:3].copy()
    j = int(np.argmin(row[0, 0]))
    row[0, 0, j] = np.nan
    r = pc.run_polish(ctx, one, pc.FAMILIES[2:3], pc.THETA0, row, n_starts=1)
    nodes, n_found = sc.row_peaks(-row[0], 1)
    assert r["node"][0, 0, 0] == nodes[0, 0] != j and r["n_found"][0, 0] == n_found[0] and not pc.status(r)[0, 0, 0] & 3
    assert r["t"][0, 0, 0] <= row[0, 0, nodes[0, 0]]
    r = pc.run_polish(ctx, one, pc.FAMILIES[2:3], pc.THETA0, np.full((1, 1, 4), np.nan), n_starts=2)
    assert r["nbad"] == 0 and (r["n_found"] == 0).all() and (r["node"] == -1).all() and (pc.status(r) == 0).all() and (r["n_eval"] == 0).all()
    assert all(np.isnan(r[k]).all() for k in ("theta0", "t", "t_stable", "t_unstable"))
    # T = t_lo at the best node
    row = rows[:1, 2:3].copy()
    row[0, 0, 1] = 0.2
    r = pc.run_polish(ctx, one, pc.FAMILIES[2:3], pc.THETA0, row, n_starts=1)
    assert r["n_eval"][0, 0, 0] == 0 and pc.status(r)[0, 0, 0] == BIT10 and r["t"][0, 0, 0] == 0.2 and r["theta0"][0, 0, 0] == pc.THETA0[1]
    assert (r["info"][0, 0, 0] & 0xffff) == 0 and r["lo_unstable"][0, 0, 0] == 1 and np.isnan(r["t_stable"][0, 0, 0])
    # max_eval = 1
    r = pc.run_polish(ctx, b, pc.FAMILIES, pc.THETA0, rows[:, :6], n_starts=1, max_eval=1)
    st = pc.status(r)
    searched = r["n_eval"] == 1
    assert searched.sum() >= 12 and ((st[searched] & BIT11) != 0).all() and not (st & 3).any()
    assert (r["t"] <= np.take_along_axis(rows[:, :6], r["node"], axis=2)).all()


# the pressure range and the grids of the driver tests: tests/test_gpu_local_eq_boundary.py::test_scan_driver_boundary_on_ncsx_tables
P_RANGE = (0.0, 3.0)


@pytest.fixture(scope="module")
def driver(ctx):
    import torch
    dev = torch.device("cuda:0")
    N = 513
    th = np.linspace(-4 * np.pi, 4 * np.pi, N)
    svals = np.array([0.6, 0.9])
    tabs = ibs_amd.SurfaceTables.from_wout(dict(np.load(os.path.join(G, "G8_wout_ncsx_op.npz"))), svals)
    scan = ibs_amd.BallooningScan(ctx, None, th, svals, nalpha=3, ntheta0=4, tables=tabs, device=dev)
    eps = np.array([-0.5, 0.0])
    return scan, tabs, th, eps, scan.local_eq_boundary_envelope(eps, P_RANGE, n_starts=2)


def check_at(ctx, scan, tabs, th, eps, r):
    """`at` reproduces first_unstable_env, bit for bit, through a fresh one-ray boundary call on the same geometry taken directly, as the
    boundary driver test takes it"""
    import torch
    dev = torch.device("cuda:0")
    n, na = len(scan.own), len(scan.alpha_scan)
    surf, alpha = np.repeat(np.arange(n), na), np.tile(scan.alpha_scan, n)
    geo = ctx.fieldline_geometry(tabs, surf, alpha, th, device=dev)
    sigma = np.sign(-np.asarray(tabs.scal)[surf, 4])
    for s in range(n):
        for k in range(len(eps)):
            al, x = r["at"][s, k]
            line = s * na + int(np.nonzero(scan.alpha_scan == al)[0][0])
            ray = np.array([(x, eps[k], 0.0, 0.0, 1.0) + P_RANGE])
            d = ctx.local_eq_boundary(th[0], scan.h, geo["geo"][:, line:line + 1].contiguous(), geo["dPdrho"][line:line + 1],
                                      alpha[line:line + 1], sigma[line:line + 1], ray, max_cross=1)
            T1 = ibs_amd.local_eq_first_up(d["t_stable"].cpu().numpy(), d["t_unstable"].cpu().numpy(), d["lo_unstable"].cpu().numpy(), P_RANGE[0])
            assert T1[0, 0] == r["first_unstable_env"][s, k], (s, k, T1, r["first_unstable_env"][s, k])


def test_scan_driver_envelope_on_ncsx_tables(ctx, driver):
    """8. BallooningScan.local_eq_boundary_envelope on the G8 wout tables: 2 surfaces x 3 alpha x 4 theta0 x 2 eps at N = 513, p-rays over
    (0, 3), two slots.  Everything local_eq_boundary returns is there, bitwise; first_unstable_env <= first_unstable on every (surface,
    eps), with equality, bit for bit, where no slot of the surface beat its node; wherever a slot did not beat its node t_env is the
    coarse call's T at that node; `at` reproduces first_unstable_env through a fresh one-ray boundary call on a fresh geometry."""
    import torch
    scan, tabs, th, eps, r = driver
    coarse = scan.local_eq_boundary(eps, P_RANGE)
    for k in ("t_stable", "t_unstable", "t", "n_cross", "lo_unstable", "info", "first_unstable"):
        assert np.array_equal(r[k], coarse[k], equal_nan=True), k
    shape = (2, 3, 2, 2)
    for k in ("theta0_env", "t_env", "node", "n_eval", "lo_unstable_env"):
        assert r[k].shape == shape, k
    assert r["n_found"].shape == (2, 3, 2) and r["first_unstable_env"].shape == (2, 2) and r["at"].shape == (2, 2, 2)
    T = ibs_amd.local_eq_first_up(r["t_stable"], r["t_unstable"], r["lo_unstable"], P_RANGE[0])       # (2, 3, 4, 2)
    Tn = np.take_along_axis(np.moveaxis(T, 2, 3), r["node"], axis=3)
    beat = r["t_env"] < Tn
    print("driver: first_unstable %s, first_unstable_env %s, gains %s, n_eval %s" % (r["first_unstable"].tolist(),
          r["first_unstable_env"].tolist(), (Tn - r["t_env"]).max(axis=(1, 3)).tolist(), r["n_eval"].ravel().tolist()))
    assert (r["t_env"] <= Tn).all() and np.array_equal(r["t_env"][~beat], Tn[~beat])
    assert (r["first_unstable_env"] <= r["first_unstable"]).all()
    none_beat = ~beat.any(axis=(1, 3))
    assert np.array_equal(r["first_unstable_env"][none_beat], r["first_unstable"][none_beat])
    assert np.array_equal(r["first_unstable_env"], r["t_env"].min(axis=(1, 3)))
    check_at(ctx, scan, tabs, th, eps, r)


def test_scan_driver_strict_gain_between_the_nodes(ctx):
    """8a. a (surfaces, grid) of the G8 tables on which the envelope lies strictly below the nodes: s = 0.5 and 0.7 on the same 3 alpha x 4
    theta0 grid, N = 513, p-rays over (0, 3).  Of the candidates tried on an MI355X (s = (0.6, 0.9), (0.80, 0.83, 0.86), (0.5, 0.7) on 3 x 4,
    5 x 4, 8 x 5 and 12 x 9 grids) this is the smallest with a strict gain: first_unstable 1.061981 -> first_unstable_env 1.060977 on
    (s = 0.5, eps = -0.5), attained at alpha = pi, theta0* = 0.81803 strictly between two nodes.  Asserted: the gain exceeds 100 xtol
    range = 3e-10 (the closing noise of T, as in test 3), theta0* lies strictly inside the bracket of its node, first_unstable_env <=
    first_unstable everywhere, and `at` reproduces the value through a fresh one-ray call at that interior theta0*."""
    import torch
    th = np.linspace(-4 * np.pi, 4 * np.pi, 513)
    svals = np.array([0.5, 0.7])
    tabs = ibs_amd.SurfaceTables.from_wout(dict(np.load(os.path.join(G, "G8_wout_ncsx_op.npz"))), svals)
    scan = ibs_amd.BallooningScan(ctx, None, th, svals, nalpha=3, ntheta0=4, tables=tabs, device=torch.device("cuda:0"))
    eps = np.array([-0.5, 0.0])
    r = scan.local_eq_boundary_envelope(eps, P_RANGE, n_starts=2)
    gain = r["first_unstable"] - r["first_unstable_env"]
    print("driver, s = 0.5 and 0.7: first_unstable %s, first_unstable_env %s, gain %s, at %s" % (r["first_unstable"].tolist(),
          r["first_unstable_env"].tolist(), gain.tolist(), r["at"].tolist()))
    assert (gain >= 0).all() and gain[0, 0] > 100 * XTOL * 3.0
    x, t0 = r["at"][0, 0, 1], r["theta0"]
    assert t0[0] < x < t0[-1] and not np.isin(x, t0)
    check_at(ctx, scan, tabs, th, eps, r)


def test_scan_driver_sensitivity_at_the_polished_point(ctx, driver):
    """8b. local_eq_boundary_sensitivity(theta0_polish=True) on the same grids: the limit is first_unstable_env, taken at `at`, and
    dfirst_dfixed and dfirst_dshift agree with central differences of first_unstable_env (steps 1e-4 and 5e-5) wherever all four displaced
    runs keep the attaining alpha.  Tolerance as in the sensitivity test of the boundary driver: 4/3 of the truncation measured by halving
    the step, the closing errors of the two differenced values over the step -- 3e-12 range each from the ray's bracket, and from the
    search curvature x (2 xtol_theta0)^2 each, the curvature being the largest second difference of the coarse rows T(theta0) -- and
    1e-6 of |derivative| for the formula."""
    scan, tabs, th, eps, env = driver
    s = scan.local_eq_boundary_sensitivity(eps, P_RANGE, theta0_polish=True)
    assert np.array_equal(s["first_unstable_env"], env["first_unstable_env"]) and np.array_equal(s["at"], env["at"])
    m = s["mask"]
    assert m.any() and np.array_equal(s["alpha"][m], env["at"][:, :, 0][m]) and np.array_equal(s["theta0_at"][m], env["at"][:, :, 1][m])
    assert (np.abs(s["lam_at"][m]) <= 1e-6).all() and (s["dlam_dt"][m] > 0).all()
    T = ibs_amd.local_eq_first_up(env["t_stable"], env["t_unstable"], env["lo_unstable"], P_RANGE[0])       # (2, 3, 4, 2)
    d2T = np.abs(T[:, :, :-2] - 2 * T[:, :, 1:-1] + T[:, :, 2:]) / np.diff(env["theta0"])[0] ** 2
    curv = d2T[np.isfinite(d2T)].max()
    step = 1e-4
    closing = 2 * (3e-12 * 3.0 + curv * (2e-5) ** 2) / step
    checked = 0
    for name, run in (("dfirst_dfixed", lambda v: scan.local_eq_boundary_envelope(eps + v, P_RANGE)),
                      ("dfirst_dshift", lambda v: scan.local_eq_boundary_envelope(eps, P_RANGE, shift=v))):
        q = {v: run(v) for v in (step, -step, 0.5 * step, -0.5 * step)}
        keep = np.all([v["at"][:, :, 0] == env["at"][:, :, 0] for v in q.values()], axis=0) & m
        d1 = (q[step]["first_unstable_env"] - q[-step]["first_unstable_env"]) / (2 * step)
        d2 = (q[0.5 * step]["first_unstable_env"] - q[-0.5 * step]["first_unstable_env"]) / step
        tol = 4.0 / 3.0 * np.abs(d1 - d2) + closing + 1e-6 * np.abs(s[name])
        err = np.abs(s[name] - d2)
        print("driver %s at the polished point: %s, differences %s, |err| %s, tol %s (curvature %.2f), kept %s"
              % (name, s[name].tolist(), d2.tolist(), err.tolist(), tol.tolist(), curv, keep.tolist()))
        assert keep.any() and (err[keep] <= tol[keep]).all(), name
        checked += keep.sum()
    assert checked >= 2


def test_sensitivity_default_is_unchanged(ctx, driver):
    """8c. with theta0_polish=False (the default) local_eq_boundary_sensitivity takes its point from the nodes as before: the keys of
    local_eq_boundary plus the derivatives, the limit is first_unstable at (alpha, theta0_at) = a node of the grids, and no key of the
    envelope appears"""
    scan, tabs, th, eps, env = driver
    s = scan.local_eq_boundary_sensitivity(eps, P_RANGE)
    assert "first_unstable_env" not in s and "at" not in s and np.array_equal(s["first_unstable"], env["first_unstable"])
    assert np.isin(s["theta0_at"][s["mask"]], scan.theta0_scan).all() and np.isin(s["alpha"][s["mask"]], scan.alpha_scan).all()
