"""GPU: the gradient of the critical scale s* through the geometry kernel (BallooningScan.marginal_sensitivity,
AdjointStep.marginal_sensitivity, autograd.marginal_points) against central differences of the forward pipeline
(from_wout -> fieldline_geometry -> ibs_marginal_obj_w_grad_tangent_f64), against the forward-mode alpha derivative, and against the
torch oracle of the geometry's VJP fed the cotangent planes of tests/marginal_tangent_oracle.py.

Setup of tests/test_gpu_geometry_vjp.py's end-to-end tests: N = 131, surfaces 0.6 / 0.9, points (alpha, theta0) = (0.3, 0.2) and
(1.1, 0.0).  Checked with the CPU oracle pipeline when the feature was specified: scale 2.0774 / 1.1444, derivative along the wout
direction of seed 23 -12.593 / -96.246 with finite-difference self-differences 2.3e-9 / 1.9e-7 at eps = 1e-5 (1.9e-5 on the second
surface at 1e-4: too coarse); d s* / d alpha -2.21257 / 2.78202 with self-differences 1.4e-7 / 7.4e-7 at 1e-4.  On an MI355X
(docs/EXPERIMENTS.md R6.14): the same values, self-differences 3.3e-9 / 1.9e-7 and 1.5e-7 / 7.4e-7; reverse against forward mode in alpha
2.4e-15; the table cotangents within 2.5e-13 of a row's maximum of the torch oracle's."""
import os

import numpy as np
import pytest

import ibs_amd
from tests import geometry_vjp_oracle as vo
from tests import marginal_tangent_oracle as mt
from ibs_amd.scan import MARGINAL_GEO_LPP
from tests.test_gpu_geometry_vjp import E2E_N, E2E_POINTS, E2E_S, WOUT_ARRAYS, _fd_rule

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def ctx():
    c = ibs_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def wout():
    return dict(np.load(os.path.join(G, "G8_wout_ncsx_op.npz")))


@pytest.fixture(scope="module")
def e2e(ctx, wout):
    """the sensitivity at the two fixed points, computed once, and the forward pipeline it is the derivative of"""
    import torch
    dev = torch.device("cuda:0")
    th = ibs_amd.theta_grid(E2E_N)
    h = float(th[1] - th[0])
    step = ibs_amd.AdjointStep(ctx, th, E2E_S, dev, nalpha=6, ntheta0=5)
    sens = step.marginal_sensitivity(wout, points=E2E_POINTS)
    t0 = np.ascontiguousarray(E2E_POINTS[:, 1])

    def scale_of(w, alpha=E2E_POINTS[:, 0]):
        tabs = ibs_amd.SurfaceTables.from_wout(w, E2E_S)
        r = ctx.fieldline_geometry(tabs, [0, 1], alpha, th)
        return ctx.marginal_obj_w_grad_tangent(h, r["geo"], None, t0, want_grad=False)["scale"]
    return dict(step=step, sens=sens, scale_of=scale_of, th=th, h=h, dev=dev, t0=t0)


def test_sensitivity_against_central_differences_in_the_wout(e2e, wout):
    """d s* / d eps along the smooth random direction of the nine wout arrays of
    test_sensitivity_against_central_differences_in_the_wout (seed 23): AdjointStep.marginal_sensitivity contracted with the direction
    against central differences of the forward pipeline at eps = 1e-5 and eps / 2 (_fd_rule)"""
    rng = np.random.default_rng(23)
    ns = int(wout["ns"])
    s = np.linspace(0, 1, ns)
    delta = {}
    for k in WOUT_ARRAYS:
        a = np.asarray(wout[k], dtype=np.float64)
        prof = rng.standard_normal((a.shape[0], 1)) * (0.5 + s * (1 - s))[None, :] + rng.standard_normal((a.shape[0], 1)) * 0.3 * s[None, :]
        delta[k] = np.abs(a).max(axis=1, keepdims=True) * prof
    sens = e2e["sens"]
    assert set(sens) == {"scale", "alpha", "theta0", "dscale_dalpha", "dscale_dtheta0", "wout_bar"}
    assert np.array_equal(sens["alpha"], E2E_POINTS[:, 0]) and np.array_equal(sens["theta0"], E2E_POINTS[:, 1])
    exact = np.array([sum(float(np.sum(sens["wout_bar"][i][k] * delta[k])) for k in WOUT_ARRAYS) for i in range(2)])
    print("marginal-sensitivity figures: scale", sens["scale"], "forward pipeline", e2e["scale_of"](wout))
    assert np.allclose(sens["scale"], e2e["scale_of"](wout), rtol=1e-10, atol=0)

    def f(e):
        w = dict(wout)
        for k in WOUT_ARRAYS:
            w[k] = np.asarray(wout[k], dtype=np.float64) + e * delta[k]
        return e2e["scale_of"](w)
    _fd_rule(f, exact, 1e-5, "marginal-sensitivity figures: d s* / d eps (wout direction)")


def test_sensitivity_in_alpha_and_theta0(ctx, e2e, wout):
    """dscale_dalpha against central differences of the forward in alpha (steps 1e-4 and 5e-5, _fd_rule); dscale_dtheta0 equals
    marginal_scan's dscale_dtheta0 on the same line within 1e-12 relative"""
    sens = e2e["sens"]
    _fd_rule(lambda e: e2e["scale_of"](wout, E2E_POINTS[:, 0] + e), sens["dscale_dalpha"], 1e-4, "marginal-sensitivity figures: d s* / d alpha")
    tabs = ibs_amd.SurfaceTables.from_wout(wout, E2E_S)
    with ctx.option_default("geo_lpp", MARGINAL_GEO_LPP):
        r = ctx.fieldline_geometry(tabs, [0, 1], E2E_POINTS[:, 0], e2e["th"], device=e2e["dev"])
    geo, dP = r["geo"].cpu().numpy(), r["dPdrho"].cpu().numpy()
    sc = ctx.marginal_scan(e2e["h"], *[np.ascontiguousarray(geo[k]) for k in range(7)], dP, e2e["t0"], want_grad=True)
    want = sc["dscale_dtheta0"][np.arange(2), np.arange(2)]
    print("marginal-sensitivity figures: dscale_dtheta0", sens["dscale_dtheta0"], want)
    assert np.abs(sens["dscale_dtheta0"] - want).max() <= 1e-12 * np.abs(want).max()


@pytest.fixture(scope="module")
def scan_case(ctx, wout, e2e):
    """BallooningScan.marginal_sensitivity at the two points and, on the CPU, the oracle's planes and their VJP"""
    tabs = ibs_amd.SurfaceTables.from_wout(wout, E2E_S)
    scan = ibs_amd.BallooningScan(ctx, None, e2e["th"], E2E_S, nalpha=6, ntheta0=5, tables=tabs, device=e2e["dev"], surf_index=np.arange(2))
    r = scan.marginal_sensitivity(E2E_POINTS)
    ls, la = np.array([0, 1], dtype=np.int32), np.ascontiguousarray(E2E_POINTS[:, 0])
    modes = dict(xm=tabs.xm, xn=tabs.xn, xm_nyq=tabs.xm_nyq, xn_nyq=tabs.xn_nyq)
    geo, _ = vo.numpy_forward(modes, tabs.tab_mn, tabs.tab_nyq, tabs.scal, ls, la, e2e["th"])
    ref = mt.points(e2e["h"], geo, None, e2e["t0"], want_grad=False, want_geo_bar=True)
    bars = vo.vjp(tabs.xm, tabs.xn, tabs.xm_nyq, tabs.xn_nyq, tabs.tab_mn, tabs.tab_nyq, tabs.scal, ls, la, e2e["th"], ref["geo_bar"], None)
    return dict(tabs=tabs, scan=scan, r=r, ls=ls, la=la, ref=ref, bars=bars)


def test_table_cotangents_against_the_oracle(e2e, scan_case):
    """tab_mn_bar, tab_nyq_bar and scal_bar against geometry_vjp_oracle.vjp fed the oracle's geo_bar, within 1e-9 of each row's maximum
    (a row: one array of one surface); scale against the oracle within 4 u"""
    c = scan_case
    r = {k: v.cpu().numpy() for k, v in c["r"].items()}
    assert set(r) == {"scale", "dscale_dalpha", "dscale_dtheta0", "dPdrho", "tab_mn_bar", "tab_nyq_bar", "scal_bar"}
    assert (np.abs(r["scale"] - c["ref"]["scale"]) <= 4 * c["ref"]["u"]).all(), (r["scale"], c["ref"]["scale"])
    for key in ("scale", "dscale_dalpha", "dscale_dtheta0"):
        assert np.array_equal(r[key], e2e["sens"][key]), key
    for name in ("tab_mn_bar", "tab_nyq_bar"):
        got, want = r[name], c["bars"][name]
        assert got.shape == want.shape
        top = np.abs(want).max(axis=2)
        err = np.abs(got - want).max(axis=2)
        assert (err[top == 0] == 0).all(), name
        worst = float((err[top > 0] / top[top > 0]).max())
        print("marginal-sensitivity figures: %s worst |got - oracle| / row maximum %.2e" % (name, worst))
        assert worst <= 1e-9, (name, worst)
    got, want = r["scal_bar"], c["bars"]["scal_bar"]
    worst = float((np.abs(got - want).max(axis=1) / np.abs(want).max(axis=1)).max())
    print("marginal-sensitivity figures: scal_bar worst |got - oracle| / row maximum %.2e\n%s" % (worst, got))
    assert worst <= 1e-9, worst


def test_forward_and_reverse_mode_agree_in_alpha(ctx, e2e, scan_case):
    """alpha_bar of the geometry VJP fed the kernel's geo_bar equals the kernel's dscale_dalpha (formed from the geometry's alpha-tangent)
    within 1e-9 relative (the CPU oracle gives 4e-16)"""
    import torch
    c = scan_case
    dev = e2e["dev"]
    with ctx.option_default("geo_lpp", MARGINAL_GEO_LPP):
        g = ctx.fieldline_geometry(c["tabs"], c["ls"], c["la"], e2e["th"], device=dev)
    ga = ctx.fieldline_geometry_dalpha(c["tabs"], c["ls"], c["la"], e2e["th"], device=dev)
    out = ctx.marginal_obj_w_grad_tangent(c["scan"].h, g["geo"], ga["geo_da"], torch.from_numpy(e2e["t0"]).to(dev), want_geo_bar=True, want_info=True)
    assert not (out["info"] >> 16).any().item()
    tt = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    v = ctx.fieldline_geometry_vjp(c["tabs"], tt(c["ls"], np.int32), tt(c["la"], np.float64), tt(e2e["th"], np.float64), out["geo_bar"], None,
                                   device=dev, want=("alpha",))
    rev, fwd = v["alpha_bar"].cpu().numpy(), out["dscale"][:, 0].cpu().numpy()
    print("marginal-sensitivity figures: alpha_bar (reverse) %s  dscale_dalpha (forward) %s  rel %s" % (rev, fwd, np.abs(rev - fwd) / np.abs(fwd)))
    assert np.array_equal(fwd, c["r"]["dscale_dalpha"].cpu().numpy())
    assert (np.abs(rev - fwd) <= 1e-9 * np.abs(fwd)).all()


def test_scan_sensitivity_defaults_to_the_last_margin(ctx, wout, e2e):
    """BallooningScan.marginal_sensitivity() without points and without an earlier marginal() raises; after marginal(refine=True) it
    works at the refined points and equals the call with those points"""
    import torch
    tabs = ibs_amd.SurfaceTables.from_wout(wout, E2E_S)
    scan = ibs_amd.BallooningScan(ctx, None, e2e["th"], E2E_S, nalpha=6, ntheta0=5, tables=tabs, device=e2e["dev"], surf_index=np.arange(2))
    with pytest.raises(ibs_amd.IbsError):
        scan.marginal_sensitivity()
    m = scan.marginal(refine=True, jac="exact_tangent")
    r = scan.marginal_sensitivity()
    assert np.array_equal(r["scale"].cpu().numpy(), m["scale"]) and np.array_equal(r["dPdrho"].cpu().numpy(), m["dPdrho"])
    assert np.array_equal(torch.stack([r["dscale_dalpha"], r["dscale_dtheta0"]], dim=1).cpu().numpy(), m["dscale"])
    r2 = scan.marginal_sensitivity(points=np.stack([m["alpha"], m["theta0"]], axis=1))
    for k in r:
        assert torch.equal(r[k], r2[k]), k
    assert tuple(r["tab_mn_bar"].shape) == (2, 6, len(tabs.xm)) and tuple(r["tab_nyq_bar"].shape) == (2, 7, len(tabs.xm_nyq))
    assert tuple(r["scal_bar"].shape) == (2, 6)
    print("marginal-sensitivity figures: refined margin %s at alpha %s theta0 %s, dscale there %s" % (m["scale"], m["alpha"], m["theta0"],
                                                                                                  m["dscale"].ravel()))


def test_autograd_composition_gives_the_sensitivitys_bits(ctx, e2e, scan_case):
    """autograd.marginal_points composed with autograd.fieldline_geometry (the geometry in the form marginal_sensitivity pins): the
    same scale and tab_mn.grad, tab_nyq.grad, scal.grad bits as BallooningScan.marginal_sensitivity; alpha.grad is d s* / d alpha
    (1e-9 relative, reverse against forward mode) and theta0.grad the kernel's theta0 derivative"""
    import torch
    from ibs_amd import autograd as iag
    c, dev = scan_case, e2e["dev"]
    t = lambda a, g=False: torch.from_numpy(np.ascontiguousarray(a)).to(dev).requires_grad_(g)
    tabs = c["tabs"]
    tm, tq, sc = t(tabs.tab_mn, True), t(tabs.tab_nyq, True), t(tabs.scal, True)
    al, t0 = t(c["la"], True), t(e2e["t0"], True)
    with ctx.option_default("geo_lpp", MARGINAL_GEO_LPP):
        geo, _ = iag.fieldline_geometry(tabs, t(c["ls"]), al, t(e2e["th"]), tab_mn=tm, tab_nyq=tq, scal=sc, ctx=ctx)
    s = iag.marginal_points(c["scan"].h, geo, t0, ctx=ctx)               # (the scan's own h: (theta[-1] - theta[0]) / (N - 1))
    assert ctx.last_launch()[0] == "ibs::k_marginal_tangent_points"
    s.sum().backward()
    r = c["r"]
    assert torch.equal(s.detach(), r["scale"])
    for name, x in (("tab_mn_bar", tm), ("tab_nyq_bar", tq), ("scal_bar", sc)):
        assert torch.equal(x.grad, r[name]), name
    assert torch.equal(t0.grad, r["dscale_dtheta0"])
    fwd = r["dscale_dalpha"]
    assert ((al.grad - fwd).abs() <= 1e-9 * fwd.abs()).all().item(), (al.grad, fwd)


def test_adjoint_step_sensitivity_at_the_refined_margin(ctx, e2e, wout):
    """AdjointStep.marginal_sensitivity without points works at the refined margin of every surface in mode jac="exact_tangent": the
    scale is that of BallooningScan.marginal(refine=True, jac="exact_tangent") on the equilibrium's tables, and the result feeds
    linearised_margin_gradient"""
    step = e2e["step"]
    sens = step.marginal_sensitivity(wout)
    tabs = ibs_amd.SurfaceTables.from_wout(wout, E2E_S)
    m = ibs_amd.BallooningScan(ctx, None, e2e["th"], E2E_S, nalpha=6, ntheta0=5, tables=tabs, device=e2e["dev"],
                               surf_index=np.arange(2)).marginal(refine=True, jac="exact_tangent")
    for key in ("scale", "alpha", "theta0"):
        assert np.array_equal(sens[key], m[key]), key
    assert np.array_equal(np.stack([sens["dscale_dalpha"], sens["dscale_dtheta0"]], axis=1), m["dscale"])
    scaled = dict(wout)
    scaled["pres"] = np.asarray(wout["pres"], dtype=np.float64) * (1.0 + 1e-3)
    grad = ibs_amd.linearised_margin_gradient(sens["wout_bar"], [wout, scaled], np.array([1.0, 1e-3]), sens["scale"])
    print("marginal-sensitivity figures: refined margin %s at alpha %s theta0 %s; linearised d s* / d (pressure scale) %s"
          % (sens["scale"], sens["alpha"], sens["theta0"], grad))
    assert grad.shape == (1, 2) and np.isfinite(grad).all()
