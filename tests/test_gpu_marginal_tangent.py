"""GPU: the margin from ONE line per point with its exact gradient and cotangent planes (ibs_marginal_obj_w_grad_tangent_f64,
csrc/ibs_marginal_tangent.hip) against the CPU restatement tests/marginal_tangent_oracle.py, against ibs_marginal_obj_w_grad_f64 on the
same centre line (bit for bit outside the alpha component), against central differences in alpha of the kernel's own scale, and the
drivers' jac="exact_tangent" mode of the margin's refinement (BallooningScan.marginal, AdjointStep.marginal).

Bounds, all the project's existing ones (tests/test_gpu_marginal_refine.py): |s* - s*_oracle| <= 4 u with u = N eps normT / kappa from
the oracle's vector; |val s*_oracle + 1| <= 4 u / s*_oracle + 4e-16; dscale and jac 1e-9 relative to max(1, |.|); dPdrho 1e-13
relative; geo_bar 1e-9 of each oracle row's maximum (the rows are the derivative rows of the Hellmann-Feynman sums times the line's
own smooth factors).  The measured worst cases are printed; on an MI355X (docs/EXPERIMENTS.md R6.14): s* within 3.2e-3 u, dscale and
jac 3e-14 (N = 67) .. 2.6e-10 (N = 2,307), geo_bar 1.4e-13 .. 4.2e-10, the theta0 components equal to the three-line kernel's bit for
bit, the alpha gap to it 1.1e-6 -> 2.8e-7 from del_alpha 0.008 to 0.004 (ratio 4.000 .. 4.001)."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import ballooning_oracle as bo
from tests import marginal_oracle as mo
from tests import marginal_tangent_oracle as mt
from tests.test_gpu_geometry_vjp import _fd_rule
from tests.test_gpu_marginal_refine import LENGTHS, POINTS, SVALS, g8_tables, rel

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(__file__), "golden")
KEYS = ("val", "jac", "scale", "dscale", "dPdrho", "geo_bar", "info")
KW = dict(want_grad=True, want_geo_bar=True, want_info=True)


def report(line):
    print("marginal-tangent figures:", line)


@pytest.fixture(scope="module")
def ctx():
    import ibs_amd
    c = ibs_amd.Context(0)
    yield c
    c.close()


_LINES = {}


def lines(N):
    """(th, h, geo (8, 6, N), geo_da, theta0 (6,)) of the six synthetic points: computed once per length"""
    if N not in _LINES:
        th = bo.theta_grid(N)
        _LINES[N] = (th, float(th[1] - th[0]), mt.lines_at(th, POINTS), mt.tangent_planes(th, POINTS), np.array([p[2] for p in POINTS]))
    return _LINES[N]


def three_lines(th, pts, d):
    """(n, 3, 8, N): the lines alpha - d / 2, alpha, alpha + d / 2 in ibs_marginal_obj_w_grad_f64's layout"""
    return np.ascontiguousarray(np.stack([mt.lines_at(th, pts, sh) for sh in (-0.5 * d, 0.0, 0.5 * d)]).transpose(2, 0, 1, 3))


def geo_bar_err(got, ref):
    """largest |got - ref| over the row maximum of ref, per (plane, point) row; rows that are zero in the oracle must be zero"""
    top = np.abs(ref).max(axis=2)
    err = np.abs(got - ref).max(axis=2)
    assert (err[top == 0] == 0).all(), "a row that is identically zero in the oracle is not in the kernel"
    return float((err[top > 0] / top[top > 0]).max())


def check_against_oracle(name, r, ref):
    """the module docstring's bars"""
    assert r["nbad"] == 0 and not (r["info"] >> 16).any(), (name, r["info"] >> 16)
    assert np.isfinite(ref["scale"]).all() and (ref["u"] > 0).all(), name
    err = np.abs(r["scale"] - ref["scale"]) / ref["u"]
    ev = np.abs(r["val"] * ref["scale"] + 1)
    e_ds, e_j = rel(r["dscale"], ref["dscale"]), rel(r["jac"], ref["jac"])
    e_dP = float((np.abs(r["dPdrho"] - ref["dPdrho"]) / np.abs(ref["dPdrho"])).max())
    e_gb = geo_bar_err(r["geo_bar"], ref["geo_bar"])
    report("%-18s points %d  max |s - s_oracle| / u %.2e  |val s + 1| %.1e  dscale err %.1e  jac err %.1e  dPdrho rel %.1e  geo_bar err "
           "%.1e  passes %.1f" % (name, len(err), err.max(), ev.max(), e_ds, e_j, e_dP, e_gb, (r["info"] & 0xffff).mean()))
    assert (err <= 4).all(), (name, err)
    assert (ev <= 4 * ref["u"] / ref["scale"] + 4e-16).all(), (name, ev)
    assert e_ds <= 1e-9 and e_j <= 1e-9, (name, e_ds, e_j)
    assert e_dP <= 1e-13, (name, e_dP)
    assert e_gb <= 1e-9, (name, e_gb)


@pytest.fixture(scope="module")
def solved(ctx):
    """every synthetic length solved once on the GPU; shared, unchanged, by the tests below"""
    res = {}
    for N in LENGTHS:
        th, h, geo, gda, t0 = lines(N)
        res[N] = ctx.marginal_obj_w_grad_tangent(h, geo, gda, t0, **KW)
        assert ctx.last_launch()[0] == "ibs::k_marginal_tangent_points", ctx.last_launch()
    return res


@pytest.mark.parametrize("N", LENGTHS)
def test_entry_point_against_the_oracle(solved, N):
    """the lane edge, the vector-chunk edges, the count-chunk edges and three count chunks, the six points of
    tests/test_gpu_marginal_refine.py"""
    th, h, geo, gda, t0 = lines(N)
    check_against_oracle("synthetic N=%d" % N, solved[N], mt.points(h, geo, gda, t0))


@pytest.mark.parametrize("N", LENGTHS)
def test_consistency_with_the_three_line_kernel(ctx, solved, N):
    """the same line as the centre line of ibs_marginal_obj_w_grad_f64, side lines at +- 0.002: val, scale, dPdrho and info bitwise;
    the theta0 components of jac and dscale within 1e-13 relative to max(1, |.|) (the same sums in the same order: bitwise equality
    is expected; the bar is that of test_consistency_with_marginal_scan, the measured difference is printed); at N <= 387, on the
    points where the gap at del_alpha = 0.008 exceeds 1e-9, |dscale_dalpha - the three-line kernel's| shrinks by a factor in [3, 5]
    from del_alpha 0.008 to 0.004"""
    th, h, geo, gda, t0 = lines(N)
    r = solved[N]
    g3 = three_lines(th, POINTS, 0.004)
    assert np.array_equal(g3[:, 1], geo.transpose(1, 0, 2))
    r4 = ctx.marginal_obj_w_grad(h, g3, t0, 0.004, want_info=True)
    for key in ("val", "scale", "dPdrho", "info"):
        assert np.array_equal(r[key], r4[key]), (key, r[key], r4[key])
    e_j, e_d = rel(r["jac"][:, 1], r4["jac"][:, 1]), rel(r["dscale"][:, 1], r4["dscale"][:, 1])
    gap4 = np.abs(r["dscale"][:, 0] - r4["dscale"][:, 0])
    line = "N=%d against ibs_marginal_obj_w_grad_f64: theta0 components jac %.1e dscale %.1e; alpha gap at 0.004 %.2e" % (N, e_j, e_d, gap4.max())
    assert e_j <= 1e-13 and e_d <= 1e-13, (e_j, e_d)
    if N <= 387:
        r8 = ctx.marginal_obj_w_grad(h, three_lines(th, POINTS, 0.008), t0, 0.008)
        gap8 = np.abs(r["dscale"][:, 0] - r8["dscale"][:, 0])
        big = gap8 > 1e-9
        ratio = gap8[big] / gap4[big]
        line += ", at 0.008 %.2e, ratio %.3f .. %.3f over %d points" % (gap8.max(), ratio.min(), ratio.max(), big.sum())
        assert big.sum() > 0 and (ratio >= 3.0).all() and (ratio <= 5.0).all(), ratio
    report(line)


@pytest.mark.parametrize("N", [67, 129])
def test_dscale_dalpha_against_central_differences_of_the_kernels_own_scale(ctx, solved, N):
    """steps 1e-4 and 5e-5, the lines regenerated at alpha +- t, the point-evaluation form; rule, cap and bar of _fd_rule
    (tests/test_gpu_geometry_vjp.py)"""
    th, h, geo, gda, t0 = lines(N)
    s_at = lambda e: ctx.marginal_obj_w_grad_tangent(h, mt.lines_at(th, POINTS, e), None, t0, want_grad=False)["scale"]
    _fd_rule(s_at, solved[N]["dscale"][:, 0], 1e-4, "N=%d d s* / d alpha" % N)


# ---- batch forms --------------------------------------------------------------------------------------------------------------------
N_B, N_PTS = 129, 600


@pytest.fixture(scope="module")
def big():
    """600 points at N = 129 (beyond the 512-point carve-out of the persistent grid): the six points and random variations"""
    rng = np.random.default_rng(129600)
    pts = list(POINTS) + [(rng.uniform(0.3, 0.9), rng.uniform(0.0, np.pi), rng.uniform(0.0, 0.5 * np.pi)) for _ in range(N_PTS - len(POINTS))]
    th = bo.theta_grid(N_B)
    return dict(th=th, h=float(th[1] - th[0]), pts=pts, geo=mt.lines_at(th, pts), gda=mt.tangent_planes(th, pts), t0=np.array([p[2] for p in pts]))


def test_batch_beyond_the_persistent_grid(ctx, big):
    """12 sampled points against the oracle; every point against the three-line kernel as above; a point alone gives its batch bits;
    host and device pointers agree bitwise; a second run repeats bitwise"""
    import torch
    b = big
    h, geo, gda, t0 = b["h"], b["geo"], b["gda"], b["t0"]
    r = ctx.marginal_obj_w_grad_tangent(h, geo, gda, t0, **KW)
    assert ctx.last_launch()[0] == "ibs::k_marginal_tangent_points", ctx.last_launch()
    assert r["nbad"] == 0 and not (r["info"] >> 16).any()
    pick = np.sort(np.random.default_rng(7).choice(N_PTS, 12, replace=False))
    sub = {k: (v[:, pick] if k == "geo_bar" else v[pick]) for k, v in r.items() if k != "nbad"}
    sub["nbad"] = 0
    check_against_oracle("batch N=129, 12 of 600", sub, mt.points(h, geo[:, pick], gda[:, pick], t0[pick]))
    r4 = ctx.marginal_obj_w_grad(h, three_lines(b["th"], b["pts"], 0.004), t0, 0.004, want_info=True)
    for key in ("val", "scale", "dPdrho", "info"):
        assert np.array_equal(r[key], r4[key]), key
    assert rel(r["jac"][:, 1], r4["jac"][:, 1]) <= 1e-13 and rel(r["dscale"][:, 1], r4["dscale"][:, 1]) <= 1e-13
    r8 = ctx.marginal_obj_w_grad(h, three_lines(b["th"], b["pts"], 0.008), t0, 0.008)
    gap8, gap4 = np.abs(r["dscale"][:, 0] - r8["dscale"][:, 0]), np.abs(r["dscale"][:, 0] - r4["dscale"][:, 0])
    bigp = gap8 > 1e-9
    ratio = gap8[bigp] / gap4[bigp]
    report("batch N=129: alpha gap to the three-line kernel at 0.008 / 0.004 %.2e / %.2e, ratio %.3f .. %.3f over %d of %d points"
           % (gap8.max(), gap4.max(), ratio.min(), ratio.max(), bigp.sum(), N_PTS))
    assert bigp.sum() > 0 and (ratio >= 3.0).all() and (ratio <= 5.0).all(), (ratio.min(), ratio.max())
    for k in (0, 1, N_PTS // 2 + 1, 511, 512, N_PTS - 1):
        one = ctx.marginal_obj_w_grad_tangent(h, geo[:, k:k + 1], gda[:, k:k + 1], t0[k:k + 1], **KW)
        for key in KEYS:
            assert np.array_equal(one[key][:, 0] if key == "geo_bar" else one[key][0], r[key][:, k] if key == "geo_bar" else r[key][k]), (k, key)
    dev = torch.device("cuda:0")
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d = ctx.marginal_obj_w_grad_tangent(h, tt(geo), tt(gda), tt(t0), **KW)
    assert ctx.last_launch()[0] == "ibs::k_marginal_tangent_points"
    again = ctx.marginal_obj_w_grad_tangent(h, geo, gda, t0, **KW)
    for key in KEYS:
        assert np.array_equal(d[key].cpu().numpy(), r[key]), key
        assert np.array_equal(again[key], r[key]), key


def test_row_pitch_and_untouched_padding(ctx, big):
    """ld = N + 5 through the C ABI, host and device pointers: the results are the packed call's bits and the padding of geo_bar,
    prefilled with a sentinel, is never written"""
    import torch
    from ibs_amd import _lib
    lib = _lib.lib()
    n, N, ld = 7, N_B, N_B + 5
    h, t0 = big["h"], np.ascontiguousarray(big["t0"][:n])
    geo, gda = big["geo"][:, :n], big["gda"][:, :n]
    ref = ctx.marginal_obj_w_grad_tangent(h, geo, gda, t0, **KW)
    pad = lambda a: np.ascontiguousarray(np.concatenate([a, np.full((8, n, 5), np.nan)], axis=2))
    SENT = -12345.0
    p = lambda a: C.c_void_p(a.ctypes.data)
    gp, dp = pad(geo), pad(gda)
    out = dict(val=np.empty(n), jac=np.empty((n, 2)), scale=np.empty(n), dscale=np.empty((n, 2)), dPdrho=np.empty(n),
               geo_bar=np.full((8, n, ld), SENT), info=np.empty(n, dtype=np.int32))
    rc = lib.ibs_marginal_obj_w_grad_tangent_f64(ctx._h, n, N, h, p(gp), p(dp), ld, p(t0), *[p(out[k]) for k in KEYS], 1)
    assert rc == 0, (rc, lib.ibs_last_error())
    assert (out["geo_bar"][:, :, N:] == SENT).all()
    for key in KEYS:
        assert np.array_equal(out[key][:, :, :N] if key == "geo_bar" else out[key], ref[key]), key
    dev = torch.device("cuda:0")
    tt = lambda a: torch.from_numpy(a).to(dev)
    dgeo, dgda, dt0 = tt(gp), tt(dp), tt(t0)
    dout = {k: tt(np.full(v.shape, SENT if v.dtype == np.float64 else 0, dtype=v.dtype)) for k, v in out.items()}
    ctx._stream_from_torch(dgeo)
    q = lambda t: C.c_void_p(t.data_ptr())
    rc = lib.ibs_marginal_obj_w_grad_tangent_f64(ctx._h, n, N, h, q(dgeo), q(dgda), ld, q(dt0), *[q(dout[k]) for k in KEYS], 0)
    assert rc == 0, (rc, lib.ibs_last_error())
    torch.cuda.synchronize()
    gb = dout["geo_bar"].cpu().numpy()
    assert (gb[:, :, N:] == SENT).all()
    for key in KEYS:
        got = dout[key].cpu().numpy()
        assert np.array_equal(got[:, :, :N] if key == "geo_bar" else got, ref[key]), key


def test_point_evaluation_form(ctx, solved):
    """all three gradient outputs off and geo_da = None: the same val, scale, dPdrho and info bits, and no other key"""
    for N in (67, 387, 2307):
        th, h, geo, gda, t0 = lines(N)
        r = ctx.marginal_obj_w_grad_tangent(h, geo, None, t0, want_grad=False, want_info=True)
        assert set(r) == {"val", "scale", "dPdrho", "info", "nbad"}
        for key in ("val", "scale", "dPdrho", "info"):
            assert np.array_equal(r[key], solved[N][key]), (N, key)
    import ibs_amd
    with pytest.raises(ibs_amd.IbsError):
        ctx.marginal_obj_w_grad_tangent(h, geo, None, t0)


def test_status(ctx):
    """dPdrho = 0: bit 8, scale = inf, val = 0, zero jac, dscale and geo_bar, not counted; a NaN in the line: bit 1, everything NaN,
    counted; a NaN in geo_da only: bit 1, jac = dscale = NaN, val, scale and geo_bar finite and the clean run's bits.  Each on its own
    point of a batch of three, whose other points keep their bits.  (Data values handled by the kernel's checks.)"""
    th, h, geo, gda, t0 = lines(129)
    geo, gda, t0 = geo[:, 1:4], gda[:, 1:4], t0[1:4]
    clean = ctx.marginal_obj_w_grad_tangent(h, geo, gda, t0, **KW)
    assert clean["nbad"] == 0 and not (clean["info"] >> 16).any() and np.isfinite(clean["geo_bar"]).all()
    others = np.array([0, 2])

    def kept(r):
        for key in KEYS:
            a, b = (r[key][:, others], clean[key][:, others]) if key == "geo_bar" else (r[key][others], clean[key][others])
            assert np.array_equal(a, b), key
    flat = geo.copy()
    flat[7, 1] = flat[2, 1]                                   # gbdrift = cvdrift: dPdrho = 0, c = 0
    r = ctx.marginal_obj_w_grad_tangent(h, flat, gda, t0, **KW)
    assert r["nbad"] == 0 and int(r["info"][1] >> 16) == 256
    assert np.isinf(r["scale"][1]) and r["scale"][1] > 0 and r["val"][1] == 0.0 and r["dPdrho"][1] == 0.0
    assert (r["jac"][1] == 0).all() and (r["dscale"][1] == 0).all() and (r["geo_bar"][:, 1] == 0).all()
    kept(r)
    bad = geo.copy()
    bad[0, 1, 40] = np.nan                                    # the line's bmag
    r = ctx.marginal_obj_w_grad_tangent(h, bad, gda, t0, **KW)
    assert r["nbad"] == 1 and int(r["info"][1] >> 16) == 2
    assert all(np.isnan(r[k][1]).all() for k in ("val", "jac", "scale", "dscale", "dPdrho")) and np.isnan(r["geo_bar"][:, 1]).all()
    kept(r)
    tang = gda.copy()
    tang[4, 1, 40] = np.nan                                   # the tangent of gds2
    r = ctx.marginal_obj_w_grad_tangent(h, geo, tang, t0, **KW)
    assert r["nbad"] == 1 and int(r["info"][1] >> 16) == 2
    assert np.isnan(r["jac"][1]).all() and np.isnan(r["dscale"][1]).all()
    for key in ("val", "scale", "dPdrho"):
        assert r[key][1] == clean[key][1], key
    assert np.array_equal(r["geo_bar"][:, 1], clean["geo_bar"][:, 1])
    kept(r)


# ---- the drivers on the G8 tables ---------------------------------------------------------------------------------------------------
N_SCAN = 969
GRID = dict(nalpha=8, ntheta0=5)


def fresh_points(ctx, scan, surf, al, t0):
    """ibs_marginal_obj_w_grad_tangent_f64 at (alpha, theta0) of table surfaces surf, the geometry in the form the rounds pin"""
    import torch
    from ibs_amd.scan import MARGINAL_GEO_LPP
    surf, al = np.asarray(surf, dtype=np.int32), np.ascontiguousarray(al)
    with ctx.option_default("geo_lpp", MARGINAL_GEO_LPP):
        r = ctx.fieldline_geometry(scan.tables, surf, al, scan.theta, device=scan.device)
    ra = ctx.fieldline_geometry_dalpha(scan.tables, surf, al, scan.theta, device=scan.device)
    out = ctx.marginal_obj_w_grad_tangent(scan.h, r["geo"], ra["geo_da"], torch.from_numpy(np.ascontiguousarray(t0)).to(scan.device),
                                          want_info=True)
    return {k: v.cpu().numpy() for k, v in out.items() if k != "nbad"}


def test_scan_driver_exact_tangent_margin_on_ncsx_tables(ctx):
    """BallooningScan.marginal on the G8 tables (2 surfaces, 8 x 5 coarse grid, N = 969, the setup of
    test_scan_driver_refined_margin_on_ncsx_tables).  The default path is unchanged: marginal(refine=True) and
    marginal(refine=True, jac="reference") are bitwise equal.  jac="exact_tangent": scale <= coarse_scale; scale within 1e-8 relative
    and the location within 1e-4 of the reference mode's (the bars that file uses between its two branches: the optimum moves only
    at second order in the gradient gap); the returned scale and dscale are the bits of a fresh point launch at the returned point; a
    surface refined alone gives its bits from the two-surface run"""
    import torch
    import ibs_amd
    dev = torch.device("cuda:0")
    th = np.linspace(-4 * np.pi, 4 * np.pi, N_SCAN)
    tabs = g8_tables()
    kw = dict(tables=tabs, device=dev, **GRID)
    a = ibs_amd.BallooningScan(ctx, None, th, SVALS, **kw).marginal(refine=True)
    assert ctx.last_launch()[0] == "ibs::k_marginal_points"
    b = ibs_amd.BallooningScan(ctx, None, th, SVALS, **kw).marginal(refine=True, jac="reference")
    assert set(a) == set(b)
    for key in a:
        assert np.array_equal(a[key], b[key]), key
    scan = ibs_amd.BallooningScan(ctx, None, th, SVALS, **kw)
    t = scan.marginal(refine=True, jac="exact_tangent")
    assert ctx.last_launch()[0] == "ibs::k_marginal_tangent_points"
    assert set(t) == set(a)
    for key in ("index", "table", "coarse_scale", "start"):
        assert np.array_equal(t[key], a[key]), key
    report("G8 N=969 marginal(refine=True): exact_tangent s* %s at alpha %s theta0 %s dscale %s, evals %s tasks %s rounds %d; reference s* "
           "%s at alpha %s theta0 %s dscale %s, evals %s rounds %d" % (t["scale"], t["alpha"], t["theta0"], t["dscale"].ravel(), t["evals"],
                                                                        t["task"], t["rounds"], a["scale"], a["alpha"], a["theta0"],
                                                                        a["dscale"].ravel(), a["evals"], a["rounds"]))
    assert (t["scale"] <= t["coarse_scale"]).all(), (t["scale"], t["coarse_scale"])
    assert (np.abs(t["scale"] - a["scale"]) <= 1e-8 * np.abs(a["scale"])).all(), (t["scale"], a["scale"])
    assert np.abs(t["alpha"] - a["alpha"]).max() < 1e-4 and np.abs(t["theta0"] - a["theta0"]).max() < 1e-4
    f = fresh_points(ctx, scan, scan.surf_index, t["alpha"], t["theta0"])
    assert not (f["info"] >> 16).any()
    for key in ("scale", "dscale", "dPdrho"):
        assert np.array_equal(t[key], f[key]), (key, t[key], f[key])
    alone = ibs_amd.BallooningScan(ctx, None, th, SVALS[1:], surf_index=[1], **kw).marginal(refine=True, jac="exact_tangent")
    for key in ("scale", "alpha", "theta0", "dscale", "dPdrho", "evals", "task"):
        assert np.array_equal(alone[key][0], t[key][1]), (key, alone[key], t[key])


def test_adjoint_step_marginal_exact_tangent(ctx):
    """AdjointStep.marginal(..., jac="exact_tangent") on two equilibria (base, scaled pressure), N = 969: every equilibrium's rows
    equal a separate BallooningScan.marginal(refine=True, jac="exact_tangent") on that equilibrium's rows of the step's table set
    BITWISE (as test_adjoint_step_marginal), and dscale follows from those rows"""
    import torch
    import ibs_amd
    dev = torch.device("cuda:0")
    wout0 = dict(np.load(os.path.join(G, "G8_wout_ncsx_op.npz")))
    scaled = dict(wout0)
    scaled["pres"] = np.asarray(wout0["pres"], dtype=np.float64) * 50.0
    wouts = [wout0, scaled]
    steps = np.array([1.0, 1e-3])
    th = ibs_amd.theta_grid_for(11, 11)
    assert len(th) == N_SCAN
    step = ibs_amd.AdjointStep(ctx, th, SVALS, dev, **GRID)
    out = step.marginal(wouts, steps, jac="exact_tangent")
    assert ctx.last_launch()[0] == "ibs::k_marginal_tangent_points"
    assert set(out) == {"scale", "alpha", "theta0", "dscale"}
    step_tabs = ibs_amd.SurfaceTables.from_wouts(wouts, SVALS)
    for q in range(2):
        m = ibs_amd.BallooningScan(ctx, None, th, SVALS, tables=step_tabs, surf_index=[2 * q, 2 * q + 1], device=dev,
                                   **GRID).marginal(refine=True, jac="exact_tangent")
        for key in ("scale", "alpha", "theta0"):
            assert np.array_equal(out[key][q], m[key]), (q, key, out[key][q], m[key])
    report("AdjointStep.marginal(jac='exact_tangent'), 2 equilibria x 2 surfaces: scale %s" % (out["scale"].ravel(),))
    assert np.array_equal(out["dscale"], (out["scale"][1:] - out["scale"][0]) / steps[1:, None])
    with pytest.raises(ibs_amd.IbsError):
        step.marginal(wouts, steps, jac="exact")
