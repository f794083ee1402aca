"""GPU: the host-pointer protocol of the C ABI.  Every entry point that takes `mem` is called twice on the same seeded inputs, with
host (numpy) and with device (torch) pointers: outputs and status words must agree bit for bit, and a host call returns the count of
status words with bit 0 or 1 set (a device call returns 0).  Covers invalid systems, optional outputs requested and omitted, the
long-grid paths (N = 2561), a host call whose staged bytes exceed the pinned mirror (4 MB) and padded rows (ld > N)."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import ballooning_oracle as bo

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(__file__), "golden")
HOST, DEVICE = 1, 0
LONG_N = 2561                 # beyond 64 * kMaxM + 2 = 2050: the long-grid paths


@pytest.fixture(scope="module")
def ctx():
    import ibs_amd
    return ibs_amd.Context(0)


class Out:
    """an output; eig: rows of eigenfunctions, left unwritten for invalid systems by the long-grid and nearest-sigma solvers"""
    def __init__(self, shape, dtype=np.float64, eig=False):
        self.shape, self.dtype, self.eig = tuple(np.atleast_1d(shape)), np.dtype(dtype), eig


def _call(ctx, name, args, mem):
    """args: numpy arrays (inputs), Out (outputs, pre-filled with one byte pattern in both modes), None, scalars"""
    import torch
    keep, conv, outs = [], [], []
    for a in args:
        if isinstance(a, np.ndarray):
            x = np.ascontiguousarray(a)
            if mem == DEVICE:
                x = torch.from_numpy(x).to("cuda:0")
            keep.append(x)
            conv.append(C.c_void_p(x.ctypes.data if mem == HOST else x.data_ptr()))
        elif isinstance(a, Out):
            nb = int(np.prod(a.shape)) * a.dtype.itemsize
            x = np.full(nb, 0xA5, np.uint8) if mem == HOST else torch.full((nb,), 0xA5, dtype=torch.uint8, device="cuda:0")
            outs.append((x, a))
            conv.append(C.c_void_p(x.ctypes.data if mem == HOST else x.data_ptr()))
        elif a is None:
            conv.append(C.c_void_p(None))
        else:
            conv.append(a)
    torch.cuda.synchronize()
    rc = getattr(ctx._lib, name)(ctx._h, *conv, mem)
    assert rc >= 0, (name, mem, rc, ctx._lib.ibs_last_error().decode())
    ctx.synchronize()
    res = []
    for x, a in outs:
        x = x if mem == HOST else x.cpu().numpy()
        res.append(x.view(a.dtype).reshape(a.shape))
    return rc, res


def _both(ctx, name, args, info=None, status=True, bad=()):
    """host and device runs of one call: bitwise-equal outputs (but the eigenfunction rows of the invalid systems `bad`); returns
    (host return value, host outputs)"""
    rc_h, out_h = _call(ctx, name, args, HOST)
    rc_d, out_d = _call(ctx, name, args, DEVICE)
    specs = [a for a in args if isinstance(a, Out)]
    for k, (a, b, o) in enumerate(zip(out_h, out_d, specs)):
        keep = np.setdiff1d(np.arange(len(a)), bad) if o.eig else slice(None)
        assert a[keep].tobytes() == b[keep].tobytes(), (name, "output %d" % k)
    if status:
        assert rc_d == 0, (name, rc_d)
    if info is not None:
        w = out_h[info]
        assert rc_h == int((((w >> 16) & 3) != 0).sum()), (name, rc_h)
    return rc_h, out_h


def _salpha(n, N, ld=None, seed=0, bad=(), dtype=np.float64):
    """(h, g, c, f) of n s-alpha systems, rows ld apart (padding: finite junk), systems in `bad` invalid (g <= 0)"""
    rng = np.random.default_rng(seed)
    th = bo.theta_grid(N)
    ld = ld or N
    g, c = np.full((n, ld), 3.0), np.full((n, ld), -2.0)
    for k in range(n):
        g[k, :N], c[k, :N] = bo.salpha_gc(th, rng.uniform(0.3, 1.8), rng.uniform(0.3, 1.5), rng.uniform(-0.3, 0.3))
    f = g * (1.0 + 0.05 * rng.random((n, ld)))
    for k in bad:
        g[k, : N // 2] = -1.0
    return th[1] - th[0], g.astype(dtype), c.astype(dtype), f.astype(dtype)


def _lines(n_lines, N, ld=None, bad=(), seed=1):
    """(h, seven geometry arrays [n_lines][ld], dPdrho [n_lines]) of synthetic field lines; lines in `bad` carry a NaN"""
    from tests.helpers import synthetic_fieldlines
    th = bo.theta_grid(N)
    ld = ld or N
    rng = np.random.default_rng(seed)
    geo = synthetic_fieldlines(th)(0.6, rng.uniform(0.0, np.pi, n_lines))
    seven = []
    for k in range(7):
        a = np.full((n_lines, ld), 0.5)
        a[:, :N] = geo[:, k]
        seven.append(a)
    for b in bad:
        seven[0][b, 3] = np.nan
    return th[1] - th[0], seven, -1.0 + 0.5 * rng.random(n_lines)


def _points_geo(n_pts, N, del_alpha=0.004, bad=(), seed=2):
    """(h, geo [n_pts][3][8][N], theta0 [n_pts]): the three lines alpha -+ del_alpha / 2 of each point"""
    from tests.helpers import synthetic_fieldlines
    th = bo.theta_grid(N)
    rng = np.random.default_rng(seed)
    al = rng.uniform(0.0, np.pi, n_pts)
    geo = synthetic_fieldlines(th)(0.6, (al[:, None] + np.array([-0.5, 0.0, 0.5]) * del_alpha).ravel()).reshape(n_pts, 3, 8, N)
    for b in bad:
        geo[b, 1, 0, 5] = np.nan
    return th[1] - th[0], geo, rng.uniform(-0.3, 0.3, n_pts)


# ---------------------------------------------------------------- solver entry points
@pytest.mark.parametrize("N", [257, 1025, LONG_N])
def test_solve_gcf_f64_and_gcfh(ctx, N):
    n = 12
    h, g, c, f = _salpha(n, N, bad=(3, 7))
    gh = 0.5 * (g[:, :-1] + g[:, 1:])
    gh = np.concatenate([gh, gh[:, -1:]], axis=1)
    for want in [(1, 1, 1, 1, 1), (1, 0, 0, 0, 1), (0, 1, 0, 0, 0), (0, 0, 0, 0, 1), (1, 1, 0, 1, 0)]:
        outs = [Out(n), Out(n), Out((n, N), eig=True), Out((n, N), eig=True), Out(n, np.int32)]
        outs = [o if w else None for o, w in zip(outs, want)]
        info = sum(want[:4]) if want[4] else None
        rc, _ = _both(ctx, "ibs_solve_gcf_f64", [n, N, h, g, c, f, N] + outs, info=info, bad=(3, 7))
        if want[4]:
            assert rc == 2
        _both(ctx, "ibs_solve_gcfh_f64", [n, N, h, g, gh, c, f, N] + outs, info=info, bad=(3, 7))


@pytest.mark.parametrize("N", [257, 641, LONG_N])
def test_solve_gcf_f32_lam_only_and_with_gam(ctx, N):
    n = 10
    h, g, c, f = _salpha(n, N, bad=(2,), dtype=np.float32)
    for want in [(1, 0, 0, 0, 1), (1, 0, 0, 0, 0), (1, 1, 0, 0, 1), (0, 1, 0, 0, 1), (1, 1, 1, 1, 1)]:
        outs = [Out(n, np.float32), Out(n, np.float32), Out((n, N), np.float32, True), Out((n, N), np.float32, True), Out(n, np.int32)]
        outs = [o if w else None for o, w in zip(outs, want)]
        _both(ctx, "ibs_solve_gcf_f32", [n, N, C.c_float(h), g, c, f, N] + outs, info=sum(want[:4]) if want[4] else None, bad=(2,))


def test_solve_gcf_padded_rows_and_a_staging_beyond_the_pinned_mirror(ctx):
    n, N, ld = 6, 513, 520
    h, g, c, f = _salpha(n, N, ld=ld, bad=(1,))
    rc, _ = _both(ctx, "ibs_solve_gcf_f64", [n, N, h, g, c, f, ld, Out(n), Out(n), Out((n, N)), Out((n, N)), Out(n, np.int32)], info=4)
    assert rc == 1
    n, N = 200, 1025                                          # 3 x 1.6 MB in, 3.3 MB of eigenfunctions out
    h, g, c, f = _salpha(n, N, bad=(0, 199))
    assert 3 * g.nbytes + 2 * n * N * 8 > 4 << 20
    rc, _ = _both(ctx, "ibs_solve_gcf_f64", [n, N, h, g, c, f, N, Out(n), Out(n), Out((n, N)), Out((n, N)), Out(n, np.int32)], info=4)
    assert rc == 2


@pytest.mark.parametrize("N", [257, LONG_N])
def test_solve_gcf_nearest(ctx, N):
    n = 8
    h, g, c, f = _salpha(n, N, bad=(5,))
    sigma = np.random.default_rng(3).uniform(0.2, 1.5, n)
    for want in [(1, 1, 1, 1, 1, 1), (1, 0, 0, 0, 0, 1), (0, 0, 1, 0, 0, 0), (0, 1, 1, 1, 0, 1)]:
        outs = [Out(n), Out(n, np.int32), Out(n), Out((n, N), eig=True), Out((n, N), eig=True), Out(n, np.int32)]
        outs = [o if w else None for o, w in zip(outs, want)]
        rc, _ = _both(ctx, "ibs_solve_gcf_nearest_f64", [n, N, h, g, None, c, f, N, sigma] + outs,
                      info=sum(want[:5]) if want[5] else None, bad=(5,))
        if want[5]:
            assert rc == 1


@pytest.mark.parametrize("N,ld", [(257, 257), (257, 264), (LONG_N, LONG_N)])
def test_solve_gcf_vjp(ctx, N, ld):
    import torch
    n = 6
    h, g, c, f = _salpha(n, N, ld=ld)
    r = ctx.solve_gcf(h, torch.from_numpy(np.ascontiguousarray(g[:, :N])).cuda(), torch.from_numpy(np.ascontiguousarray(c[:, :N])).cuda(),
                      torch.from_numpy(np.ascontiguousarray(f[:, :N])).cuda(), want_X=True)
    lam = r["lam"].cpu().numpy()
    X = np.zeros((n, ld))
    X[:, :N] = r["X"].cpu().numpy()
    rng = np.random.default_rng(4)
    for gb, lb in [(rng.random(n), rng.random(n)), (rng.random(n), None), (None, rng.random(n))]:
        args = [n, N, h, g, c, f, ld, lam, X, gb, lb, Out((n, ld)), Out((n, ld)), Out((n, ld))]
        for info in (Out(n, np.int32), None):
            rc_h, out_h = _call(ctx, "ibs_solve_gcf_vjp_f64", args + [info], HOST)
            rc_d, out_d = _call(ctx, "ibs_solve_gcf_vjp_f64", args + [info], DEVICE)
            assert rc_d == 0
            for a, b in zip(out_h[:3], out_d[:3]):
                assert a[:, :N].tobytes() == b[:, :N].tobytes()
                assert (a[:, N:] == 0).all()                    # (include/ibs.h: host padding columns come back as 0)
            if info is not None:
                assert out_h[3].tobytes() == out_d[3].tobytes()
                assert rc_h == int((((out_h[3] >> 16) & 3) != 0).sum())


# ---------------------------------------------------------------- geometry-fed scans and points
@pytest.mark.parametrize("N", [257, 1025, LONG_N])
def test_gamma_scan_scan_warm_and_points(ctx, N):
    n_lines, t0 = 6, np.array([-0.2, 0.0, 0.1, 0.3])
    n_t0 = len(t0)
    h, seven, dP = _lines(n_lines, N, ld=N + 6, bad=(2,))
    ld = N + 6
    for want in [(1, 1, 1, 1, 1, 1), (1, 1, 0, 0, 0, 1), (0, 0, 0, 0, 0, 0), (1, 0, 0, 0, 1, 1)]:
        outs = [Out((n_lines, n_t0)), Out((n_lines, n_t0)), Out((n_lines * n_t0, N), eig=True), Out((n_lines * n_t0, N), eig=True),
                Out((n_lines, n_t0)), Out((n_lines, n_t0), np.int32)]
        outs = [o if w else None for o, w in zip(outs, want)]
        info = sum(want[:5]) if want[5] else None
        bad = np.arange(2 * n_t0, 3 * n_t0)                     # (the systems of line 2)
        rc, out = _both(ctx, "ibs_gamma_scan_f64", [n_lines, n_t0, N, h] + seven + [ld, dP, t0] + outs, info=info, bad=bad)
        if want[5]:
            assert rc > 0
        guess = np.full((n_lines, n_t0), 0.3)
        _both(ctx, "ibs_gamma_scan_warm_f64", [n_lines, n_t0, N, h] + seven + [ld, dP, t0, guess, C.c_double(0.2)] + outs, info=info,
              bad=bad)
        pt_t0 = np.linspace(-0.3, 0.3, n_lines)
        outs = [Out(n_lines), Out(n_lines), Out((n_lines, N), eig=True), Out((n_lines, N), eig=True), Out(n_lines), Out(n_lines, np.int32)]
        outs = [o if w else None for o, w in zip(outs, want)]
        _both(ctx, "ibs_gamma_points_f64", [n_lines, N, h] + seven + [ld, dP, pt_t0] + outs, info=info, bad=(2,))


@pytest.mark.parametrize("N", [257, LONG_N])
def test_gamma_scan_nearest_and_points_nearest(ctx, N):
    n_lines, t0 = 5, np.array([0.0, 0.2])
    h, seven, dP = _lines(n_lines, N, bad=(1,))
    sigma = np.random.default_rng(5).uniform(0.2, 1.2, n_lines * len(t0))
    for want in [(1, 1, 1, 1), (1, 0, 0, 0), (0, 1, 0, 1)]:
        outs = [Out(n_lines * 2), Out(n_lines * 2), Out(n_lines * 2, np.int32), Out(n_lines * 2, np.int32)]
        outs = [o if w else None for o, w in zip(outs, want)]
        rc, _ = _both(ctx, "ibs_gamma_scan_nearest_f64", [n_lines, 2, N, h] + seven + [N, dP, t0, sigma] + outs,
                      info=sum(want[:3]) if want[3] else None)
        if want[3]:
            assert rc > 0
    for want in [(1, 1, 1, 1, 1), (0, 0, 0, 0, 1), (1, 0, 1, 0, 0)]:
        outs = [Out(n_lines), Out(n_lines, np.int32), Out((n_lines, N), eig=True), Out((n_lines, N), eig=True), Out(n_lines, np.int32)]
        outs = [o if w else None for o, w in zip(outs, want)]
        _both(ctx, "ibs_gamma_points_nearest_f64", [n_lines, N, h] + seven + [N, dP, t0[:1].repeat(n_lines), sigma[:n_lines], Out(n_lines)] +
              outs, info=1 + sum(want[:4]) if want[4] else None, bad=(1,))


@pytest.mark.parametrize("N", [257, 1025, LONG_N])
def test_obj_w_grad_and_obj_w_grad_nearest(ctx, N):
    n = 7
    h, geo, t0 = _points_geo(n, N, bad=(4,))
    for info in (Out(n, np.int32), None):
        rc, _ = _both(ctx, "ibs_obj_w_grad_f64", [n, N, h, geo, N, t0, C.c_double(0.004), Out(n), Out((n, 2)), info],
                      info=2 if info is not None else None)
        if info is not None:
            assert rc > 0
    sigma = np.random.default_rng(6).uniform(0.2, 1.2, n)
    for want in [(1, 1, 1), (0, 0, 1), (1, 0, 0), (0, 0, 0)]:
        outs = [Out(n), Out(n, np.int32), Out(n, np.int32)]
        outs = [o if w else None for o, w in zip(outs, want)]
        _both(ctx, "ibs_obj_w_grad_nearest_f64", [n, N, h, geo, N, t0, sigma, C.c_double(0.004), Out(n), Out((n, 2))] + outs,
              info=2 + sum(want[:2]) if want[2] else None)


def test_obj_w_grad_long_grid_beyond_512_points_fresh_context():
    """the long-grid objective with more than 512 points on a fresh context (its long-grid workspace sized by this call), against
    the same points in batches of 128"""
    import ibs_amd
    fresh = ibs_amd.Context(0)
    n, N = 520, LONG_N
    h, geo, t0 = _points_geo(n, N, bad=(17,))
    rc, (val, jac, info) = _both(fresh, "ibs_obj_w_grad_f64", [n, N, h, geo, N, t0, C.c_double(0.004), Out(n), Out((n, 2)),
                                                              Out(n, np.int32)], info=2)
    assert rc > 0
    for p0 in range(0, n, 128):
        p1 = min(n, p0 + 128)
        _, (v, j, i) = _call(fresh, "ibs_obj_w_grad_f64", [p1 - p0, N, h, geo[p0:p1], N, t0[p0:p1], C.c_double(0.004), Out(p1 - p0),
                                                           Out((p1 - p0, 2)), Out(p1 - p0, np.int32)], DEVICE)
        assert v.tobytes() == val[p0:p1].tobytes() and j.tobytes() == jac[p0:p1].tobytes() and i.tobytes() == info[p0:p1].tobytes()


# ---------------------------------------------------------------- the remaining entry points (return 0, or the refinement's rounds)
@pytest.mark.parametrize("N,ld", [(257, 257), (1025, 1030), (LONG_N, LONG_N)])
def test_hf_grad_and_sturm_count(ctx, N, ld):
    rng = np.random.default_rng(7)
    n = 9
    six = [rng.random((n, ld)) for _ in range(6)]
    rc, _ = _both(ctx, "ibs_hf_grad_f64", [n, N] + six + [ld, rng.random(n), Out(n)])
    assert rc == 0
    h, g, c, f = _salpha(n, N, ld=ld)
    for form in (0, 2, 3):
        ctx.set_option("sturm_form", form)
        try:
            rc, _ = _both(ctx, "ibs_sturm_count_f64", [n, N, h, g, c, f, ld, rng.uniform(-0.5, 1.0, n), Out(n, np.int32)])
        finally:
            ctx.set_option("sturm_form", None)
        assert rc == 0


def test_surface_argmax(ctx):
    rng = np.random.default_rng(8)
    for n_surf, n_per in [(3, 40), (5, 700)]:
        gam = np.round(rng.random((n_surf, n_per)), 1)           # (ties: the first index wins)
        rc, _ = _both(ctx, "ibs_surface_argmax_f64", [n_surf, n_per, gam, Out(n_surf, np.int32), Out(n_surf)])
        assert rc == 0


def _tables(svals):
    import ibs_amd
    return ibs_amd.SurfaceTables.from_wout(dict(np.load(os.path.join(G, "G8_wout_ncsx_op.npz"))), svals)


def _table_args(t, rows):
    head = [len(t.s), len(t.xm), len(t.xm_nyq)] + [np.ascontiguousarray(a) for a in (t.xm, t.xn, t.xm_nyq, t.xn_nyq, t.tab_mn, t.tab_nyq, t.scal)]
    if rows:
        r = [len(t.rows_mn), np.ascontiguousarray(t.rows_mn, np.int32), len(t.rows_nyq), np.ascontiguousarray(t.rows_nyq, np.int32)]
    else:
        r = [0, None, 0, None]
    return head, r + [C.c_double(t.dn_mn), C.c_double(t.dn_nyq)]


@pytest.mark.parametrize("rows", [True, False])
def test_fieldline_geometry(ctx, rows):
    t = _tables([0.5, 0.7])
    N, n_lines = 257, 5
    head, tail = _table_args(t, rows)
    ls = np.array([0, 1, 1, 0, 1], np.int32)
    la = np.linspace(0.1, 2.0, n_lines)
    th = bo.theta_grid(N)
    for dP in (Out(n_lines), None):
        ctx.set_option("forget_rows", 1)
        rc, _ = _both(ctx, "ibs_fieldline_geometry_f64", head + [n_lines, ls, la, N, th, N, Out((8, n_lines, N)), dP] + tail)
        assert rc == 0


@pytest.mark.parametrize("want_evals", [True, False])
def test_refine(ctx, want_evals):
    t = _tables([0.5, 0.7])
    N = 257
    head, tail = _table_args(t, True)
    n = 4
    ps = np.array([0, 1, 0, 1], np.int32)
    st = np.array([[0.3, 0.1], [1.0, 0.2], [2.0, 0.0], [0.5, 0.4]])
    ne = Out(n, np.int32) if want_evals else None
    ctx.set_option("forget_rows", 1)
    rc_h, out_h = _call(ctx, "ibs_refine_f64", head + tail + [n, ps, st, N, bo.theta_grid(N), C.c_double(0.004), 5, C.c_double(5e-11),
                                                             C.c_double(2e-8), Out((n, 2)), Out(n), ne], HOST)
    ctx.set_option("forget_rows", 1)
    rc_d, out_d = _call(ctx, "ibs_refine_f64", head + tail + [n, ps, st, N, bo.theta_grid(N), C.c_double(0.004), 5, C.c_double(5e-11),
                                                             C.c_double(2e-8), Out((n, 2)), Out(n), ne], DEVICE)
    assert rc_h == rc_d > 0
    for a, b in zip(out_h, out_d):
        assert a.tobytes() == b.tobytes()
