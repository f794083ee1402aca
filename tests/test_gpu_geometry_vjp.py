"""GPU: ibs_fieldline_geometry_vjp_f64 and the layers on it (Context.fieldline_geometry_vjp, autograd.fieldline_geometry,
BallooningScan.sensitivity, AdjointStep.sensitivity) against the torch oracle of tests/geometry_vjp_oracle.py and against central
differences of the forward pipeline (from_wout -> fieldline_geometry -> gamma_points)."""
import copy
import ctypes as C
import os

import numpy as np
import pytest

import ibs_amd
from ibs_amd import _lib
from tests import geometry_vjp_oracle as vo

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SVALS = np.array([0.3, 0.5, 0.7, 0.9])
# 7 lines over 3 of the 4 surfaces in shuffled order: surface 2 holds four lines, surface 1 none
LINE_SURF = np.array([2, 0, 2, 3, 2, 0, 2], dtype=np.int32)
LINE_ALPHA = np.array([0.3, 2.9, 1.1, 0.0, 2.2, 0.7, np.pi])
BAR = 3.1e-12          # test_vjp_against_the_oracle
NAMES = ("tab_mn_bar", "tab_nyq_bar", "scal_bar", "alpha_bar")


@pytest.fixture(scope="module")
def ctx():
    return ibs_amd.Context(0)


@pytest.fixture(scope="module")
def wout():
    return dict(np.load(os.path.join(G, "G8_wout_ncsx_op.npz")))


def _subset_wout(wout, keep_mn, keep_nyq):
    """the same equilibrium with a subset of its Fourier modes (shape coverage: both sides evaluate the same formulas on it)"""
    w = dict(wout)
    for k in ("rmnc", "zmns", "lmns"):
        w[k] = wout[k][keep_mn]
    for k in ("gmnc", "bmnc", "bsupvmnc", "bsubsmns", "bsubumnc", "bsubvmnc"):
        w[k] = wout[k][keep_nyq]
    w["xm"], w["xn"] = wout["xm"][keep_mn], wout["xn"][keep_mn]
    w["xm_nyq"], w["xn_nyq"] = wout["xm_nyq"][keep_nyq], wout["xn_nyq"][keep_nyq]
    return w


_CASES = {}


def _case(wout, modes, N, lines):
    """tables, lines, a fixed random (geo_bar, dPdrho_bar) scaled by each plane's maximum, and the oracle's VJPs: computed once"""
    key = (modes, N, lines)
    if key in _CASES:
        return _CASES[key]
    w = wout
    if modes == "subset":                      # 37 + 53 modes, the leading (n = 0 .. ) ones kept so that the surfaces stay nested
        rng = np.random.default_rng(3)
        kmn = np.sort(np.concatenate([np.arange(8), 8 + rng.choice(len(wout["xm"]) - 8, 29, replace=False)]))
        knq = np.sort(np.concatenate([np.arange(8), 8 + rng.choice(len(wout["xm_nyq"]) - 8, 45, replace=False)]))
        w = _subset_wout(wout, kmn, knq)
    tabs = ibs_amd.SurfaceTables.from_wout(w, SVALS)
    ls, la = (LINE_SURF, LINE_ALPHA) if lines == 7 else (np.array([3], dtype=np.int32), np.array([1.3]))
    th = ibs_amd.theta_grid(N)
    modes_d = dict(xm=tabs.xm, xn=tabs.xn, xm_nyq=tabs.xm_nyq, xn_nyq=tabs.xn_nyq)
    geo, dP = vo.numpy_forward(modes_d, tabs.tab_mn, tabs.tab_nyq, tabs.scal, ls, la, th)
    rng = np.random.default_rng(17)
    gb = rng.standard_normal(geo.shape) / np.abs(geo).max(axis=(1, 2), keepdims=True)
    db = rng.standard_normal(len(ls)) / np.abs(dP).max()
    args = (tabs.xm, tabs.xn, tabs.xm_nyq, tabs.xn_nyq, tabs.tab_mn, tabs.tab_nyq, tabs.scal, ls, la, th)
    c = dict(tabs=tabs, ls=ls, la=la, th=th, geo=geo, gb=gb, db=db, ref=vo.vjp(*args, gb, None), ref_dp=vo.vjp(*args, gb, db),
             rev_dp=vo.vjp(*args, gb, db, reverse_modes=True))
    _CASES[key] = c
    return c


def _col_ratios(got, ref):
    """max|delta| / max|oracle| per output column: 6 + 7 table columns, 6 scalars, alpha"""
    out = []
    for name, axes in (("tab_mn_bar", (0, 2)), ("tab_nyq_bar", (0, 2)), ("scal_bar", (0,)), ("alpha_bar", None)):
        d, r = np.abs(got[name] - ref[name]).max(axis=axes), np.abs(ref[name]).max(axis=axes)
        out += list(np.atleast_1d(d / r))
    return np.array(out)


def _raw_host_call(ctx, tabs, ls, la, th, gb, db, ld):
    """the C entry point with host pointers and a row pitch ld >= N"""
    n_lines, N = len(ls), len(th)
    out = [np.empty(tabs.tab_mn.shape), np.empty(tabs.tab_nyq.shape), np.empty(tabs.scal.shape), np.empty(n_lines)]
    p = lambda a: C.c_void_p(None if a is None else a.ctypes.data)
    host = [tabs.xm, tabs.xn, tabs.xm_nyq, tabs.xn_nyq, tabs.tab_mn, tabs.tab_nyq, tabs.scal]
    la = np.ascontiguousarray(la, dtype=np.float64); th = np.ascontiguousarray(th)
    _lib.check(_lib.lib().ibs_fieldline_geometry_vjp_f64(ctx._h, len(tabs.s), len(tabs.xm), len(tabs.xm_nyq), *[p(a) for a in host],
                                                         n_lines, p(ls), p(la), N, p(th), ld, p(gb), p(db), *[p(a) for a in out],
                                                         _lib.MEM_HOST), "ibs_fieldline_geometry_vjp_f64")
    return dict(zip(NAMES, out))


@pytest.mark.parametrize("modes,N,lines", [("full", 67, 7), ("full", 131, 7), ("subset", 67, 7), ("subset", 131, 7), ("full", 131, 1),
                                           ("subset", 67, 1)])
def test_vjp_against_the_oracle(ctx, wout, modes, N, lines):
    """max|delta| / max|oracle| per output column (13 table columns, 6 scalars, alpha) <= BAR, with and without dPdrho_bar; the
    surface without lines comes back exactly 0; ld = N + 5 with NaN in the padding once.
    BAR = 10 x the larger of (a) the same ratio of the existing forward kernel against oracle/geometry_oracle on the same lines (both
    use_rows forms) and (b) the oracle VJP's own order-of-summation spread (mode order reversed), each taken as the largest over
    the six cases.  Measured on an MI355X (docs/EXPERIMENTS.md): (a) 4.5e-15 .. 3.10e-13 (full tables, N = 131, 7 lines), (b)
    2.0e-15 .. 1.55e-14, so BAR = 3.1e-12 (the cap of 1e-8 is far away); the kernel's own ratio was 2.8e-14 .. 5.0e-14.  The three
    figures of a run are printed."""
    c = _case(wout, modes, N, lines)
    tabs, ls, la, th = c["tabs"], c["ls"], c["la"], c["th"]
    fwd = 0.0
    for use_rows in (True, False):
        g = ctx.fieldline_geometry(tabs, ls, la, th, use_rows=use_rows)["geo"]
        fwd = max(fwd, float((np.abs(g - c["geo"]).max(axis=(1, 2)) / np.abs(c["geo"]).max(axis=(1, 2))).max()))
    spread = float(_col_ratios(c["rev_dp"], c["ref_dp"]).max())
    bar = BAR
    got = ctx.fieldline_geometry_vjp(tabs, ls, la, th, c["gb"])
    got_dp = ctx.fieldline_geometry_vjp(tabs, ls, la, th, c["gb"], c["db"])
    r0, r1 = _col_ratios(got, c["ref"]), _col_ratios(got_dp, c["ref_dp"])
    print("case %s N=%d lines=%d: forward %.2e  oracle spread %.2e  bar %.2e  vjp %.2e  vjp with dPdrho_bar %.2e"
          % (modes, N, lines, fwd, spread, bar, r0.max(), r1.max()))
    assert r0.max() <= bar and r1.max() <= bar, (r0, r1, bar)
    unused = sorted(set(range(len(SVALS))) - set(int(k) for k in ls))
    assert unused
    for name in NAMES[:3]:
        assert np.all(got_dp[name][unused] == 0.0)
    if modes == "full" and N == 67 and lines == 7:
        ld = N + 5
        gbp = np.full((8, len(ls), ld), np.nan); gbp[:, :, :N] = c["gb"]
        pad = _raw_host_call(ctx, tabs, ls, la, th, gbp, c["db"], ld)
        for name in NAMES:
            assert np.array_equal(pad[name], got_dp[name]), name


def test_host_and_device_pointers_and_repeats_give_the_same_bits(ctx, wout):
    import torch
    c = _case(wout, "full", 67, 7)
    dev = torch.device("cuda:0")
    tabs, ls, la, th = c["tabs"], c["ls"], c["la"], c["th"]
    h1 = ctx.fieldline_geometry_vjp(tabs, ls, la, th, c["gb"], c["db"])
    h2 = ctx.fieldline_geometry_vjp(tabs, ls, la, th, c["gb"], c["db"])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d1 = ctx.fieldline_geometry_vjp(tabs, t(ls), t(la), t(th), t(c["gb"]), t(c["db"]), device=dev)
    d2 = ctx.fieldline_geometry_vjp(tabs, ls, la, th, t(c["gb"]), t(c["db"]), device=dev)
    for name in NAMES:
        assert torch.is_tensor(d1[name]) and d1[name].is_cuda
        for other in (h2[name], d1[name].cpu().numpy(), d2[name].cpu().numpy()):
            assert np.array_equal(h1[name], other), name


def test_each_output_alone_equals_the_same_output_with_the_others(ctx, wout):
    c = _case(wout, "subset", 67, 7)
    tabs, ls, la, th = c["tabs"], c["ls"], c["la"], c["th"]
    full = ctx.fieldline_geometry_vjp(tabs, ls, la, th, c["gb"], c["db"])
    for k in ("tab_mn", "tab_nyq", "scal", "alpha"):
        one = ctx.fieldline_geometry_vjp(tabs, ls, la, th, c["gb"], c["db"], want=(k,))
        assert np.array_equal(one[k + "_bar"], full[k + "_bar"]), k
        assert all(one[n] is None for n in NAMES if n != k + "_bar")


def test_nan_tables_of_one_surface_stay_on_that_surface(ctx, wout):
    c = _case(wout, "subset", 67, 7)
    tabs, ls, la, th = c["tabs"], c["ls"], c["la"], c["th"]
    clean = ctx.fieldline_geometry_vjp(tabs, ls, la, th, c["gb"], c["db"])
    bad = copy.copy(tabs)
    bad.__dict__.pop("_device_copies", None)
    bad.scal = tabs.scal.copy(); bad.scal[0, 1] = np.nan           # iota of surface 0: lines 1 and 5
    got = ctx.fieldline_geometry_vjp(bad, ls, la, th, c["gb"], c["db"])
    on0 = ls == 0
    assert np.all(np.isnan(got["alpha_bar"][on0])) and np.array_equal(got["alpha_bar"][~on0], clean["alpha_bar"][~on0])
    for name in NAMES[:3]:
        assert np.all(np.isnan(got[name][0])), name
        assert np.array_equal(got[name][1:], clean[name][1:]), name


def test_autograd_composition_matches_the_oracle(ctx, wout):
    """autograd.fieldline_geometry: the gradients of a fixed linear functional of (geo, dPdrho) in tab_mn, tab_nyq, scal and alpha are
    the kernel's VJP, and the defaults carry no gradient"""
    import torch
    from ibs_amd import autograd as iag
    c = _case(wout, "subset", 67, 7)
    dev = torch.device("cuda:0")
    tabs = c["tabs"]
    t = lambda a, g=False: torch.from_numpy(np.ascontiguousarray(a)).to(dev).requires_grad_(g)
    tm, tq, sc, al = t(tabs.tab_mn, True), t(tabs.tab_nyq, True), t(tabs.scal, True), t(c["la"], True)
    geo, dP = iag.fieldline_geometry(tabs, t(c["ls"]), al, t(c["th"]), tab_mn=tm, tab_nyq=tq, scal=sc, ctx=ctx)
    ((geo * t(c["gb"])).sum() + (dP * t(c["db"])).sum()).backward()
    want = ctx.fieldline_geometry_vjp(tabs, c["ls"], c["la"], c["th"], c["gb"], c["db"])
    for name, x in zip(NAMES, (tm, tq, sc, al)):
        assert np.array_equal(x.grad.cpu().numpy(), want[name]), name
    al2 = t(c["la"], True)
    geo2, _ = iag.fieldline_geometry(tabs, t(c["ls"]), al2, t(c["th"]), ctx=ctx)
    assert torch.equal(geo2, geo.detach())
    geo2.sum().backward()
    assert al2.grad is not None and np.all(np.isfinite(al2.grad.cpu().numpy()))


# ---- end to end at fixed points ---------------------------------------------------------------------------------------
E2E_N = 131
E2E_S = np.array([0.6, 0.9])
E2E_POINTS = np.array([[0.3, 0.2], [1.1, 0.0]])                  # (alpha, theta0)
WOUT_ARRAYS = ("rmnc", "zmns", "lmns", "gmnc", "bmnc", "bsupvmnc", "bsubsmns", "bsubumnc", "bsubvmnc")


def _fd_rule(f, value, eps, what):
    fd1 = (f(eps) - f(-eps)) / (2 * eps)
    fd2 = (f(eps / 2) - f(-eps / 2)) / eps
    sd = np.abs(fd1 - fd2)
    print("%s: exact %s  fd %s  fd self-difference (relative) %s" % (what, value, fd2, sd / np.abs(fd2)))
    assert np.all(sd <= 1e-5 * np.abs(fd2)), "the finite difference itself is useless here"
    assert np.all(np.abs(value - fd2) <= 4 * sd + 1e-11 * np.abs(fd2))


@pytest.fixture(scope="module")
def e2e(ctx, wout):
    import torch
    dev = torch.device("cuda:0")
    th = ibs_amd.theta_grid(E2E_N)
    step = ibs_amd.AdjointStep(ctx, th, E2E_S, dev)
    sens = step.sensitivity(wout, points=E2E_POINTS)
    h = float(th[1] - th[0])

    def gam_of(w, alpha=E2E_POINTS[:, 0]):
        """the forward pipeline as it was before the sensitivity existed: from_wout -> fieldline_geometry -> gamma_points"""
        tabs = ibs_amd.SurfaceTables.from_wout(w, E2E_S)
        r = ctx.fieldline_geometry(tabs, [0, 1], alpha, th)
        return ctx.gamma_points(h, *[r["geo"][k] for k in range(7)], r["dPdrho"], np.ascontiguousarray(E2E_POINTS[:, 1]))["gam"]
    return dict(step=step, sens=sens, gam_of=gam_of, th=th, h=h, dev=dev)


def test_sensitivity_against_central_differences_in_the_wout(e2e, wout):
    """d gam / d eps along a smooth random direction of the nine wout arrays (per-mode amplitude max|row| x a smooth radial profile)
    at (s, alpha, theta0) = (0.6, 0.3, 0.2) and (0.9, 1.1, 0.0), N = 131: AdjointStep.sensitivity contracted with the direction
    against central differences of the forward pipeline at eps = 1e-5 and eps / 2 (rule and cap of the CPU finite-difference test).
    The CPU oracle pipeline gave -4.1888e-3 and 9.6863e-2 for its direction, self-differences 1.3e-8 and 3.9e-8; this direction on an
    MI355X: exact 1.329086e-2 and 6.8893497e-1, differences 1.329086e-2 and 6.8893429e-1, self-differences 2.6e-9 and 3.0e-6."""
    rng = np.random.default_rng(23)
    ns = int(wout["ns"])
    s = np.linspace(0, 1, ns)
    delta = {}
    for k in WOUT_ARRAYS:
        a = np.asarray(wout[k], dtype=np.float64)
        prof = rng.standard_normal((a.shape[0], 1)) * (0.5 + s * (1 - s))[None, :] + rng.standard_normal((a.shape[0], 1)) * 0.3 * s[None, :]
        delta[k] = np.abs(a).max(axis=1, keepdims=True) * prof
    sens = e2e["sens"]
    exact = np.array([sum(float(np.sum(sens["wout_bar"][i][k] * delta[k])) for k in WOUT_ARRAYS) for i in range(2)])
    assert np.array_equal(sens["gam"], e2e["gam_of"](wout)) or np.allclose(sens["gam"], e2e["gam_of"](wout), rtol=1e-10, atol=0)

    def f(e):
        w = dict(wout)
        for k in WOUT_ARRAYS:
            w[k] = np.asarray(wout[k], dtype=np.float64) + e * delta[k]
        return e2e["gam_of"](w)
    _fd_rule(f, exact, 1e-5, "d gam / d eps (wout direction)")


def test_sensitivity_in_alpha_and_theta0(ctx, e2e, wout):
    """dgam_dalpha against central differences of the forward in alpha (steps 1e-4 and 5e-5, same rule); dgam_dtheta0 equals
    autograd.growth_rate's to rounding"""
    import torch
    from ibs_amd import autograd as iag
    sens = e2e["sens"]
    _fd_rule(lambda e: e2e["gam_of"](wout, E2E_POINTS[:, 0] + e), sens["dgam_dalpha"], 1e-4, "d gam / d alpha")
    dev = e2e["dev"]
    tabs = ibs_amd.SurfaceTables.from_wout(wout, E2E_S)
    r = ctx.fieldline_geometry(tabs, [0, 1], E2E_POINTS[:, 0], e2e["th"], device=dev)
    t0 = torch.from_numpy(np.ascontiguousarray(E2E_POINTS[:, 1])).to(dev).requires_grad_(True)
    gam = iag.growth_rate(e2e["h"], *r["geo"][:7], r["dPdrho"], t0[:, None], ctx=ctx)
    gam.sum().backward()
    want = t0.grad.cpu().numpy()
    print("dgam_dtheta0", sens["dgam_dtheta0"], want)
    assert np.abs(sens["dgam_dtheta0"] - want).max() <= 1e-12 * np.abs(want).max()


def test_scan_sensitivity_defaults_to_the_last_rows(ctx, wout):
    """BallooningScan.sensitivity() without points works at the rows of the last device_rows(), and returns the gam of those rows"""
    import torch
    dev = torch.device("cuda:0")
    th = ibs_amd.theta_grid(E2E_N)
    tabs = ibs_amd.SurfaceTables.from_wout(wout, E2E_S)
    scan = ibs_amd.BallooningScan(ctx, None, th, E2E_S, nalpha=6, ntheta0=5, tables=tabs, device=dev, surf_index=np.arange(2))
    with pytest.raises(ibs_amd.IbsError):
        scan.sensitivity()
    rows = scan.local_rows(refine=False)
    r = scan.sensitivity()
    assert np.abs(r["gam"].cpu().numpy() - rows[:, 2]).max() <= 1e-10 * np.abs(rows[:, 2]).max()
    r2 = scan.sensitivity(points=np.stack([rows[:, 1], rows[:, 0]], axis=1))
    for k in r:
        assert torch.equal(r[k], r2[k]), k
    assert tuple(r["tab_mn_bar"].shape) == (2, 6, len(tabs.xm)) and tuple(r["scal_bar"].shape) == (2, 6)
