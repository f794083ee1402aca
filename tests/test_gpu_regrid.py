"""GPU: lines on non-uniform theta grids -- the batched regrid (csrc/ibs_regrid.hip), the theta scans and points built on it, and the
drop-in gamma_ball_full_many -- against numpy's np.interp and the oracle's restatement of utils.py:1565-1624
(oracle/ballooning_oracle.py: regrid_uniform, assemble, gamma_ball_full on any increasing grid).

Shapes are the smallest that hit the edges: N = 67 (64 lanes + 3), 131, 257, 2051 (the first long-grid length: the row is searched
in global memory, the long-grid solver runs), 16,385 once; 5 lines x 3 theta0.  The grids are those of tests/regrid_cases.py.
Tolerances: the interpolation to 4 eps (|fp_k| + |fp_{k+1}|) (derived: tests/test_regrid_cpu.py); growth rates to 1e-10, X, dX and
rows to 1e-7 (test_gamma_ball_full_nonuniform_grid_regrids_like_reference); eigenvalues to the library's a-priori 4 N eps ||A||.
Every test prints its worst figure before it asserts it."""
import ctypes as C
import os

import numpy as np
import pytest

import ibs_amd
from oracle import ballooning_oracle as bo
from tests import regrid_cases as rc

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EPS = np.finfo(np.float64).eps
THETA0 = np.array([0.0, 0.7, 1.5])
SALPHA = [(0.8, 1.2), (0.5, 0.9), (1.1, 1.6)]          # (shat, alpha) of the three s-alpha lines
LINE_KINDS = ["random", "clustered", "hits", "sinh", "random"]      # the grid of each of the five lines (two NCSX lines last)
GAM_TOL, ARR_TOL = 1e-10, 1e-7


@pytest.fixture(scope="module")
def ctx():
    return ibs_amd.Context(0)


@pytest.fixture(autouse=True)
def _default_dispatch(ctx):
    ctx.reset_options()
    yield
    ctx.reset_options()


@pytest.fixture(scope="module")
def tables():
    return ibs_amd.SurfaceTables.from_arrays(dict(np.load(os.path.join(G, "G8_surface_tables.npz"))))


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda:0"))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def norm_a(d, e, fd):
    """||A|| = max_r (|d_r| + e_r + e_{r+1}) / f_r (include/ibs.h)"""
    return float(np.max((np.abs(d) + e[:-1] + e[1:]) / fd))


_LINES = {}


def lines(ctx, tables, N):
    """five lines on their own grids at N: theta (5, N), geo7 (7, 5, N), dPdrho (5,) -- three s-alpha lines and two NCSX lines made by
    the geometry kernel on a non-uniform theta (the arrays copied back, so that the oracle sees what the solver sees).  Computed once
    per N and never modified."""
    if N not in _LINES:
        th = np.stack([rc.grid(k, N) for k in LINE_KINDS])
        geo7, dP = np.empty((7, 5, N)), np.empty(5)
        for i, (sh, al) in enumerate(SALPHA):
            geo7[:, i], dP[i] = rc.salpha_line(th[i], sh, al)
        for i, (surf, alpha) in zip((3, 4), ((0, 0.3), (1, 1.1))):
            r = ctx.fieldline_geometry(tables, [surf], [alpha], th[i])
            geo7[:, i], dP[i] = r["geo"][:7, 0], r["dPdrho"][0]
        for a in (th, geo7, dP):
            a.setflags(write=False)
        _LINES[N] = (th, geo7, dP)
    return _LINES[N]


_ORACLE = {}


def oracle(ctx, tables, N):
    """the oracle on the lines of lines(): gam, lam, tol_lam (5, 3); X, dX, g, c, f, gh (5, 3, N)"""
    if N not in _ORACLE:
        th, geo7, dP = lines(ctx, tables, N)
        o = {k: np.empty((5, 3)) for k in ("gam", "lam", "tol_lam")}
        o.update({k: np.zeros((5, 3, N)) for k in ("X", "dX", "g", "c", "f", "gh")})
        for i in range(5):
            bmag, gradpar, cvdrift, cvdrift0, gds2, gds21, gds22 = geo7[:, i]
            for k, t0 in enumerate(THETA0):
                cv, gd = bo.fold_theta0(t0, cvdrift, cvdrift0, gds2, gds21, gds22)
                o["gam"][i, k], o["X"][i, k], o["dX"][i, k], o["g"][i, k], o["c"][i, k], o["f"][i, k] = \
                    bo.gamma_ball_full(dP[i], th[i], bmag, gradpar, cv, gd)
                g, c, f = bo.gcf(dP[i], bmag, gradpar, cv, gd)
                d, e, fd, h = bo.assemble(th[i], g, c, f)[:4]
                o["lam"][i, k] = bo.top_eigenpair(d, e, fd)[0]
                o["tol_lam"][i, k] = 4 * N * EPS * norm_a(d, e, fd)
                o["gh"][i, k, :-1] = e * h ** 2
        for a in o.values():
            a.setflags(write=False)
        _ORACLE[N] = o
    return _ORACLE[N]


# ---- 1. regrid_rows against np.interp ------------------------------------------------------------------------------------
def check_rows(label, th_rows, rows, out):
    """the four outputs of a regrid against numpy within the derived bound, h bit for bit"""
    worst = 0.0
    for s in range(rows[0].shape[0]):
        th = th_rows if th_rows.ndim == 1 else th_rows[s]
        g, c, f = (r[s] for r in rows)
        h, tu, half, gu, gh, cu, fu = rc.regrid_numpy(th, g, c, f)
        assert out["h"] == h, (label, out["h"], h)
        assert out["gh"][s, -1] == 0.0
        for got, ref, fp, x in ((out["g"][s], gu, g, tu), (out["gh"][s, :-1], gh[:-1], g, half), (out["c"][s], cu, c, tu),
                                (out["f"][s], fu, f, tu)):
            bound = rc.interp_bound(th, fp, x)
            err = np.abs(got - ref)
            worst = max(worst, float((err / bound).max()))
            assert np.all(err <= bound), (label, s, float((err / bound).max()))
    print("%s: largest error / bound %.3f" % (label, worst))


@pytest.mark.parametrize("N", [67, 131, 257, 2051])
def test_regrid_rows_against_np_interp(ctx, N):
    """5 systems, a different grid kind per system and then one shared grid (theta_ld = 0); numpy and device tensors bit for bit"""
    th = np.stack([rc.grid(k, N) for k in rc.KINDS])
    rows = [np.stack(x) for x in zip(*[rc.salpha_rows(th[s], 0.8, 1.2, t0) for s, t0 in enumerate((0.0, 0.7, 1.5, 0.0, 0.7))])]
    for label, grid in (("per-system grids", th), ("shared grid", th[1])):
        if grid.ndim == 1:
            rows = [np.stack(x) for x in zip(*[rc.salpha_rows(grid, 0.8, 1.2, t0) for t0 in (0.0, 0.7, 1.5, 0.3, 1.0)])]
        out = ctx.regrid_rows(grid, *rows, want_info=True)
        assert out["nbad"] == 0 and not out["info"].any()
        check_rows("N=%d %s" % (N, label), grid, rows, out)
        od = ctx.regrid_rows(dev(grid), *[dev(r) for r in rows], want_info=True)
        assert od["h"] == out["h"]
        for k in ("g", "gh", "c", "f", "info"):
            assert same_bits(od[k].cpu().numpy(), out[k]), (label, k)
        only_g = ctx.regrid_rows(grid, rows[0])
        assert only_g["c"] is None and only_g["f"] is None and same_bits(only_g["g"], out["g"]) and same_bits(only_g["gh"], out["gh"])


@pytest.mark.parametrize("N", [67, 2051])
def test_regrid_rows_with_padded_rows(ctx, N):
    """the C entry point with ld = N + 5 and ld_out = N + 3, host pointers: the bits of the packed call, padding never written"""
    th = np.stack([rc.grid(k, N) for k in rc.KINDS])
    rows = [np.stack(x) for x in zip(*[rc.salpha_rows(th[s], 0.8, 1.2, 0.7) for s in range(5)])]
    ref = ctx.regrid_rows(th, *rows)
    ld, ld_out, ld_t = N + 5, N + 3, N + 2
    pad = lambda a, n: np.ascontiguousarray(np.concatenate([a, np.full((5, n - N), np.nan)], axis=1))
    tin, gin, cin, fin = pad(th, ld_t), pad(rows[0], ld), pad(rows[1], ld), pad(rows[2], ld)
    outs = [np.full((5, ld_out), -7.0) for _ in range(4)]
    info, h = np.full(5, -1, np.int32), C.c_double(0.0)
    p = lambda a: C.c_void_p(a.ctypes.data)
    rc_ = ctx._lib.ibs_regrid_rows_f64(ctx._h, 5, N, p(tin), ld_t, float(th[0, 0]), float(th[0, -1]), p(gin), p(cin), p(fin), ld,
                                       *[p(o) for o in outs], ld_out, C.byref(h), p(info), ibs_amd._lib.MEM_HOST)
    assert rc_ == 0 and h.value == ref["h"] and not info.any()
    for o, k in zip(outs, ("g", "gh", "c", "f")):
        assert same_bits(o[:, :N], ref[k]), k
        assert np.all(o[:, N:] == -7.0), k


def test_regrid_rows_one_long_line_searched_in_global_memory(ctx):
    N = 16385
    th = rc.grid("clustered", N)
    rows = [r[None] for r in rc.salpha_rows(th, 0.8, 1.2, 0.7)]
    out = ctx.regrid_rows(th, *rows)
    assert out["nbad"] == 0
    check_rows("N=%d clustered" % N, th, rows, out)


# ---- 2. gamma_scan_theta against the oracle ------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [67, 257, 2051])
def test_gamma_scan_theta_against_the_oracle(ctx, tables, N):
    """5 lines x 3 theta0 on per-line grids of different kinds: |gam - oracle| < 1e-10, X, dX and the rows < 1e-7,
    |lam - lambda_matrix| <= 4 N eps ||A||"""
    th, geo7, dP = lines(ctx, tables, N)
    o = oracle(ctx, tables, N)
    r = ctx.gamma_scan_theta(th, *geo7, dP, THETA0, want_X=True, want_info=True)
    rows = ctx.assemble_gcf_theta(th, *geo7, dP, THETA0)
    e_gam, e_lam = np.abs(r["gam"] - o["gam"]), np.abs(r["lam"] - o["lam"]) / o["tol_lam"]
    e_arr = {k: float(np.abs(r[k] - o[k]).max()) for k in ("X", "dX")}
    e_arr.update({k: float(np.abs(rows[k] - o[k]).max()) for k in ("g", "c", "f", "gh")})
    print("N=%d: |gam - oracle| %.2e (gam %.3e .. %.3e), |lam - oracle| / (4 N eps ||A||) %.3f, arrays %s"
          % (N, e_gam.max(), o["gam"].min(), o["gam"].max(), e_lam.max(), {k: "%.1e" % v for k, v in e_arr.items()}))
    assert r["nbad"] == 0 and rows["nbad"] == 0 and not (r["info"] >> 16 & 3).any()
    assert e_gam.max() < GAM_TOL
    assert e_lam.max() <= 1.0
    assert all(v < ARR_TOL for v in e_arr.values()), e_arr
    assert rows["h"] == np.diff((np.linspace(th[0, 0], th[0, -1], N)[:-1] + np.linspace(th[0, 0], th[0, -1], N)[1:]) / 2)[2]


def test_the_regrid_matters(ctx, tables):
    """N = 67, the random grid: gamma_scan fed the same arrays as if the grid were uniform is a different answer"""
    th, geo7, dP = lines(ctx, tables, 67)
    good = ctx.gamma_scan_theta(th[0], *geo7[:, :1], dP[:1], THETA0)["gam"]
    as_uniform = ctx.gamma_scan(ibs_amd.uniform_spacing(bo.theta_grid(67)), *geo7[:, :1], dP[:1], THETA0)["gam"]
    print("gam with the regrid %s, as if uniform %s" % (good, as_uniform))
    assert np.abs(good - as_uniform).max() > 1e-6


# ---- 3. a uniform grid through the theta path ------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [67, 257, 2051])
def test_uniform_grid_agrees_with_gamma_scan(ctx, N):
    th = bo.theta_grid(N)
    geo7 = np.stack([rc.salpha_line(th, sh, al)[0] for sh, al in SALPHA], axis=1)
    dP = -np.ones(3)
    a = ctx.gamma_scan_theta(th, *geo7, dP, THETA0)
    b = ctx.gamma_scan(ibs_amd.uniform_spacing(th), *geo7, dP, THETA0)
    d = np.abs(a["gam"] - b["gam"]).max()
    print("N=%d uniform grid: |gam_theta - gam_scan| %.2e" % (N, d))
    assert a["nbad"] == 0 and d < GAM_TOL


# ---- 4. independence of batch, order and chunking --------------------------------------------------------------------------
@pytest.mark.parametrize("N", [67, 2051])
def test_results_do_not_depend_on_batch_order_or_chunks(ctx, tables, N):
    th, geo7, dP = lines(ctx, tables, N)
    full = ctx.gamma_scan_theta(th, *geo7, dP, THETA0, want_X=True, want_info=True)
    keys = ("gam", "lam", "X", "dX", "info")
    for k, t0 in enumerate(THETA0):                                    # points: entry [i, k] of the scan
        pts = ctx.gamma_points_theta(th, *geo7, dP, np.full(5, t0), want_X=True, want_info=True)
        for key in keys:
            assert same_bits(pts[key], full[key][:, k]), ("points", k, key)
    perm = np.array([3, 0, 4, 2, 1])
    r = ctx.gamma_scan_theta(th[perm], *geo7[:, perm], dP[perm], THETA0, want_X=True, want_info=True)
    for key in keys:
        assert same_bits(r[key], full[key][perm]), ("permuted", key)
    sub = np.array([1, 3])
    r = ctx.gamma_scan_theta(th[sub], *geo7[:, sub], dP[sub], THETA0, want_X=True, want_info=True)
    for key in keys:
        assert same_bits(r[key], full[key][sub]), ("subset", key)
    for chunk in (3, 7):                                               # one line and two lines per chunk: 5 and 3 chunks
        ctx.set_option("nearest_chunk_systems", chunk)
        r = ctx.gamma_scan_theta(th, *geo7, dP, THETA0, want_X=True, want_info=True)
        ctx.set_option("nearest_chunk_systems", None)
        for key in keys:
            assert same_bits(r[key], full[key]), ("chunk", chunk, key)
    # the points form in chunks of 2, 2 and 1 points: a chunk starts at its own theta0 (neighbouring points differ in theta0)
    pick = np.arange(5) % len(THETA0)
    pts = ctx.gamma_points_theta(th, *geo7, dP, THETA0[pick], want_X=True, want_info=True)
    ctx.set_option("nearest_chunk_systems", 2)
    r = ctx.gamma_points_theta(th, *geo7, dP, THETA0[pick], want_X=True, want_info=True)
    ctx.set_option("nearest_chunk_systems", None)
    for key in keys:
        assert same_bits(r[key], pts[key]), ("points in chunks", key)
        assert same_bits(pts[key], full[key][np.arange(5), pick]), ("mixed points", key)


# ---- 5. invalid grids ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [67, 2051])
def test_invalid_grids_are_flagged_and_touch_no_other_line(ctx, tables, N):
    """of 5 lines one has a NaN sample, one a decreasing pair, one an end point off the window: NaN outputs, status bit 1, counted
    by the host call; the two good lines are bit for bit what they are alone.  (The bisection of csrc/ibs_regrid.hpp stays inside
    [0, N - 2] on any row -- tests/test_regrid_cpu.py -- so such rows index nothing out of bounds.)"""
    th, geo7, dP = lines(ctx, tables, N)
    bad_th = th.copy()
    bad_th[1, N // 3] = np.nan
    bad_th[2, N // 2:N // 2 + 2] = bad_th[2, N // 2:N // 2 + 2][::-1].copy()
    bad_th[4, -1] += 1e-9
    bad, good = [1, 2, 4], [0, 3]
    window = (th[0, 0], th[0, -1])
    rows = ctx.assemble_gcf_theta(bad_th, *geo7, dP, THETA0, window=window, want_info=True)
    scan = ctx.gamma_scan_theta(bad_th, *geo7, dP, THETA0, window=window, want_X=True, want_info=True)
    print("N=%d: nbad rows %d scan %d" % (N, rows["nbad"], scan["nbad"]))
    assert rows["nbad"] == 9 and scan["nbad"] == 9
    for k in ("g", "gh", "c", "f"):
        assert np.isnan(rows[k][bad]).all(), k
    assert np.all((rows["info"][bad] >> 16) == 2) and not rows["info"][good].any()
    assert np.isnan(scan["gam"][bad]).all() and np.isnan(scan["lam"][bad]).all()
    assert np.isnan(scan["X"][bad]).all() and np.isnan(scan["dX"][bad]).all()
    assert np.all((scan["info"][bad] >> 16) & 2) and not ((scan["info"][good] >> 16) & 3).any()
    rows_g = ctx.assemble_gcf_theta(th[good], *geo7[:, good], dP[good], THETA0, want_info=True)
    scan_g = ctx.gamma_scan_theta(th[good], *geo7[:, good], dP[good], THETA0, want_X=True, want_info=True)
    for k in ("g", "gh", "c", "f", "info"):
        assert same_bits(rows[k][good], rows_g[k]), k
    for k in ("gam", "lam", "X", "dX", "info"):
        assert same_bits(scan[k][good], scan_g[k]), k
    raw = ctx.regrid_rows(bad_th, rows_g["g"][[0, 0, 0, 1, 1], 0], window=window, want_info=True)     # (any finite rows)
    assert raw["nbad"] == 3 and np.isnan(raw["g"][bad]).all() and np.isnan(raw["gh"][bad]).all() and np.isfinite(raw["g"][good]).all()


# ---- 6. the device-resident chain ----------------------------------------------------------------------------------------
def test_device_resident_chain_equals_the_host_path(ctx, tables):
    """geometry kernel on a non-uniform theta -> gamma_scan_theta on its tensors, against the host-array path on the copied-back arrays"""
    import torch
    N = 131
    th = rc.grid("clustered", N)
    d = torch.device("cuda:0")
    geo = ctx.fieldline_geometry(tables, dev(np.array([0, 1, 1], np.int32)), dev(np.array([0.3, 1.1, 2.0])), dev(th), device=d)
    on_dev = ctx.gamma_scan_theta(dev(th), *geo["geo"][:7], geo["dPdrho"], dev(THETA0), want_X=True, want_info=True,
                                  window=(th[0], th[-1]))
    by_ends = ctx.gamma_scan_theta(dev(th), *geo["geo"][:7], geo["dPdrho"], dev(THETA0), want_X=True, want_info=True)
    host = ctx.gamma_scan_theta(th, *geo["geo"][:7].cpu().numpy(), geo["dPdrho"].cpu().numpy(), THETA0, want_X=True, want_info=True)
    assert host["nbad"] == 0 and np.isfinite(host["gam"]).all()
    for k in ("gam", "lam", "X", "dX", "info"):
        assert same_bits(on_dev[k].cpu().numpy(), host[k]) and same_bits(by_ends[k].cpu().numpy(), host[k]), k


# ---- 7. compositions -----------------------------------------------------------------------------------------------------
def test_nearest_and_modes_compositions(ctx):
    """N = 131, 3 lines x 2 theta0 on the clustered grid: eigenpair="nearest" with sigma above lam_max is lam_max's pair (idx 0);
    n_modes = 3 against scipy's eigenvalues of the pencil bo.assemble returns; all within 4 N eps ||A||"""
    from scipy.linalg import eigh_tridiagonal
    N, t0s = 131, THETA0[:2]
    th = rc.grid("clustered", N)
    geo7 = np.stack([rc.salpha_line(th, sh, al)[0] for sh, al in SALPHA], axis=1)
    dP = -np.ones(3)
    top = ctx.gamma_scan_theta(th, *geo7, dP, t0s)
    near = ctx.gamma_scan_theta(th, *geo7, dP, t0s, eigenpair="nearest", sigma=float(top["lam"].max()) + 1.0, want_info=True)
    modes = ctx.gamma_scan_theta(th, *geo7, dP, t0s, n_modes=3, want_info=True)
    assert near["lam"].shape == (3, 2) and modes["lam"].shape == (3, 2, 3) and near["nbad"] == 0 and modes["nbad"] == 0
    worst = 0.0
    for i in range(3):
        bmag, gradpar, cvdrift, cvdrift0, gds2, gds21, gds22 = geo7[:, i]
        for k, t0 in enumerate(t0s):
            cv, gd = bo.fold_theta0(t0, cvdrift, cvdrift0, gds2, gds21, gds22)
            d, e, fd = bo.assemble(th, *bo.gcf(dP[i], bmag, gradpar, cv, gd))[:3]
            n = len(d)
            w = eigh_tridiagonal(d / fd, e[1:n] / np.sqrt(fd[:-1] * fd[1:]), eigvals_only=True, select="i", select_range=(n - 3, n - 1))[::-1]
            tol = 4 * N * EPS * norm_a(d, e, fd)
            errs = [abs(near["lam"][i, k] - top["lam"][i, k]), abs(modes["lam"][i, k, 0] - top["lam"][i, k]), *np.abs(modes["lam"][i, k] - w)]
            worst = max(worst, max(errs) / tol)
            assert near["idx"][i, k] == 0 and max(errs) <= tol, (i, k, errs, tol)
    print("compositions: largest |lam - reference| / (4 N eps ||A||) %.3f" % worst)


# ---- 8. the batched drop-in ----------------------------------------------------------------------------------------------
@pytest.mark.filterwarnings("ignore::ibs_amd.NearestSigmaWarning")      # (gamma_ball_full's report of lam_max >= sigma0: not the subject)
def test_gamma_ball_full_many_against_gamma_ball_full(ctx):
    """4 systems, one of them on a uniform grid, against four gamma_ball_full calls: gam to 1e-10, the arrays to 1e-7"""
    N = 257
    kinds = ["random", "uniform", "sinh", "clustered"]
    th = np.stack([rc.grid(k, N) for k in kinds])
    par = [(0.8, 1.2), (0.5, 0.9), (1.1, 1.6), (0.8, 1.2)]
    geo = [rc.salpha_line(th[i], sh, al)[0] for i, (sh, al) in enumerate(par)]
    B, gradpar, cvdrift, gds2 = (np.stack([g[k] for g in geo]) for k in (0, 1, 2, 4))
    dP = np.array([-1.0, -0.7, -1.3, -1.0])
    many = ibs_amd.gamma_ball_full_many(dP, th, B, gradpar, cvdrift, gds2, ctx=ctx)
    worst = [0.0, 0.0]
    for i in range(4):
        one = ibs_amd.gamma_ball_full(dP[i], th[i], B[i], gradpar[i], cvdrift[i], gds2[i], ctx=ctx)
        worst[0] = max(worst[0], abs(many[0][i] - one[0]))
        worst[1] = max([worst[1]] + [float(np.abs(a[i] - b).max()) for a, b in zip(many[1:], one[1:])])
    print("gamma_ball_full_many: |gam| %.2e arrays %.2e" % tuple(worst))
    assert worst[0] < GAM_TOL and worst[1] < ARR_TOL
    shared = ibs_amd.gamma_ball_full_many(dP[:1], th[0], B[:1], gradpar[:1], cvdrift[:1], gds2[:1], ctx=ctx)
    assert all(same_bits(a, b[:1]) for a, b in zip(shared, many))
