"""CPU: the margin from one line per point with its exact gradient and cotangent planes (ibs_marginal_obj_w_grad_tangent_f64) -- its
oracle (tests/marginal_tangent_oracle.py) against central differences of tests/marginal_oracle.solve in the geometry arrays and in
alpha, the forward / reverse identity sum geo_bar geo_da = d s* / d alpha on the G8 tables, objective.linearised_margin_gradient, and
the plumbing (export, argument checks, kernel resources, the jac option of the marginal drivers).

No finite-difference check goes beyond N = 129: the conditioning unit u of s* is 1e-8 at N = 387 and 1e-7 at N = 771, and a difference
quotient of s* is noise there (2.8e-4 at N = 771)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import ibs_amd
from ibs_amd import _lib
from oracle import ballooning_oracle as bo
from tests import geometry_tangent_oracle as to
from tests import geometry_vjp_oracle as vo
from tests import marginal_tangent_oracle as mt
from tests.helpers import synthetic_fieldlines

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ideal-ballooning-solver_amd", "csrc")
LIB = os.path.join(ROOT, "ideal-ballooning-solver_amd", "lib", "libibs_hip.so")
G = os.path.join(ROOT, "tests", "golden")
NAME = "ibs_marginal_obj_w_grad_tangent_f64"
IBS_ERR_ARG, IBS_ERR_UNSUPPORTED = -1, -3
POINTS = ((0.3, 1.1, 0.4), (0.9, 0.0, 0.5 * np.pi), (0.9, np.pi, 0.4), (0.3, 0.0, 0.0))
_CASE = {}


def case(N):
    """the four synthetic points at length N: lines, tangent planes and the oracle's outputs, computed once"""
    if N not in _CASE:
        th = bo.theta_grid(N)
        h = float(th[1] - th[0])
        t0 = np.array([p[2] for p in POINTS])
        geo, gda = mt.lines_at(th, POINTS), mt.tangent_planes(th, POINTS)
        _CASE[N] = dict(th=th, h=h, t0=t0, geo=geo, gda=gda, ref=mt.points(h, geo, gda, t0))
    return _CASE[N]


@pytest.mark.parametrize("N", [67, 129])
def test_geo_bar_against_central_differences_of_the_solve(N):
    """sum geo_bar D against Richardson-combined central differences (steps 1e-5, 5e-6) of mo.solve's scale along three random
    directions D, every plane of D scaled by that plane's maximum, at the four synthetic points.  Bar 1e-6 relative (measured when
    the closed form was derived: <= 3.5e-8)"""
    c = case(N)
    assert np.isfinite(c["ref"]["scale"]).all() and not c["ref"]["info"].any()
    rng = np.random.default_rng(1000 + N)
    worst = 0.0
    for k in range(len(POINTS)):
        line, t0 = c["geo"][:, k], float(c["t0"][k])
        for _ in range(3):
            D = rng.standard_normal(line.shape) * np.abs(line).max(axis=1, keepdims=True)
            fd = lambda t: (mt.scale_of_line(c["h"], line + t * D, t0) - mt.scale_of_line(c["h"], line - t * D, t0)) / (2 * t)
            ref = (4.0 * fd(5e-6) - fd(1e-5)) / 3.0
            got = float(np.sum(c["ref"]["geo_bar"][:, k] * D))
            err = abs(got - ref) / abs(ref)
            worst = max(worst, err)
            print("N=%d point %d: sum geo_bar D %.12e  Richardson difference %.12e  rel %.2e" % (N, k, got, ref, err))
            assert err <= 1e-6, (N, k, got, ref)
    print("N=%d worst relative mismatch %.2e" % (N, worst))


@pytest.mark.parametrize("N", [67, 129])
def test_dscale_dalpha_against_central_differences_in_alpha(N):
    """dscale[:, 0] against Richardson-combined central differences (steps 1e-4, 5e-5) in alpha of the oracle's own scale, the lines
    regenerated at alpha +- t (they are analytic in alpha).  Bar 1e-6 relative (measured <= 1.7e-7)"""
    c = case(N)
    s_at = lambda sh: mt.points(c["h"], mt.lines_at(c["th"], POINTS, sh), None, c["t0"], False, False)["scale"]
    fd = lambda t: (s_at(t) - s_at(-t)) / (2 * t)
    ref = (4.0 * fd(5e-5) - fd(1e-4)) / 3.0
    got = c["ref"]["dscale"][:, 0]
    err = np.abs(got - ref) / np.abs(ref)
    print("N=%d dscale_dalpha %s  Richardson difference %s  rel %s" % (N, got, ref, err))
    assert (err <= 1e-6).all(), (got, ref)
    # jac = dscale / s*^2, val = -1 / s*
    assert np.array_equal(c["ref"]["jac"], c["ref"]["dscale"] / c["ref"]["scale"][:, None] ** 2)
    assert np.array_equal(c["ref"]["val"], -1.0 / c["ref"]["scale"])


def test_forward_reverse_identity_on_the_g8_tables():
    """sum geo_bar geo_da = dscale[:, 0] (dPdrho has no alpha-tangent, so the cotangent through the line's own dPdrho contracts to
    zero up to rounding): N = 131, surfaces 0.6 / 0.9, alpha 0.3 / 1.1, theta0 0.2 / 0, geo and geo_da of to.dalpha.  Bar 1e-12
    relative (measured 4e-16)"""
    d = dict(np.load(os.path.join(G, "G8_surface_tables.npz")))
    tab_mn, tab_nyq, scal = vo.packed(d)
    theta = ibs_amd.theta_grid(131)
    geo, gda, dP, dP_da = to.dalpha(d["xm"], d["xn"], d["xm_nyq"], d["xn_nyq"], tab_mn, tab_nyq, scal, np.array([0, 1]),
                                    np.array([0.3, 1.1]), theta)
    r = mt.points(float(theta[1] - theta[0]), geo, gda, np.array([0.2, 0.0]))
    assert np.isfinite(r["scale"]).all()
    lhs = np.sum(r["geo_bar"] * gda, axis=(0, 2))
    err = np.abs(lhs - r["dscale"][:, 0]) / np.abs(r["dscale"][:, 0])
    print("scale %s  sum geo_bar geo_da %s  dscale_dalpha %s  rel %s" % (r["scale"], lhs, r["dscale"][:, 0], err))
    assert (err <= 1e-12).all()


def test_oracle_status_8():
    """gbdrift = cvdrift: dPdrho = 0, no c_j > 0 -- scale = inf, val = 0 and zero derivatives, as the kernel writes them"""
    c = case(67)
    flat = c["geo"].copy()
    flat[7] = flat[2]
    r = mt.points(c["h"], flat, c["gda"], c["t0"])
    assert np.isinf(r["scale"]).all() and (r["val"] == 0).all() and (r["info"] >> 16 == 256).all()
    assert not r["jac"].any() and not r["dscale"].any() and not r["geo_bar"].any()


# ---- objective.linearised_margin_gradient -------------------------------------------------------------------------------------------
SHAPES = lambda ns: dict(rmnc=(6, ns), zmns=(6, ns), lmns=(6, ns), gmnc=(8, ns), bmnc=(8, ns), bsupvmnc=(8, ns), bsubsmns=(8, ns),
                         bsubumnc=(8, ns), bsubvmnc=(8, ns), iotas=(ns,), pres=(ns,), phi=(ns,), Aminor_p=())


def test_linearised_margin_gradient_on_hand_built_inputs():
    """two keys move, by amounts whose dot products are exact in binary: the expected numbers are written out; a surface with an
    infinite scale0 gets a zero column"""
    from ibs_amd.objective import linearised_margin_gradient
    shapes = SHAPES(4)
    w0 = {k: np.zeros(s) for k, s in shapes.items()}
    w1 = {k: v.copy() for k, v in w0.items()}; w1["pres"] = np.array([0.0, 0.5, 0.0, 0.25])
    w2 = {k: v.copy() for k, v in w0.items()}; w2["rmnc"] = w2["rmnc"].copy(); w2["rmnc"][2, 1] = 0.125; w2["Aminor_p"] = np.array(2.0)
    sens = [{k: np.zeros(s) for k, s in shapes.items()} for _ in range(3)]
    sens[0]["pres"] = np.array([9.0, 2.0, 9.0, -4.0]); sens[0]["rmnc"][2, 1] = 8.0; sens[0]["Aminor_p"] = np.array(0.5)
    sens[1]["pres"] = np.array([0.0, 1.0, 0.0, 1.0]); sens[1]["rmnc"][2, 1] = 3.0       # (ignored: scale0[1] = inf)
    sens[2]["pres"] = np.array([0.0, -6.0, 0.0, 0.0]); sens[2]["rmnc"][0, 0] = 5.0
    steps = np.array([1.0, 0.5, 0.25])
    got = linearised_margin_gradient(sens, [w0, w1, w2], steps, np.array([2.0, np.inf, 1.5]))
    #        surface 0: (2 * 0.5 - 4 * 0.25) / 0.5 = 0, (8 * 0.125 + 0.5 * 2) / 0.25 = 8;  surface 2: -6 * 0.5 / 0.5 = -6, 0
    want = np.array([[0.0, 0.0, -6.0], [8.0, 0.0, 0.0]])
    assert got.shape == (2, 3) and np.array_equal(got, want), got
    with pytest.raises(ValueError):
        linearised_margin_gradient(sens[:2], [w0, w1, w2], steps, np.array([2.0, np.inf, 1.5]))


def test_linearised_margin_gradient_equals_the_difference_of_a_linear_table():
    from ibs_amd.objective import linearised_margin_gradient
    rng = np.random.default_rng(5)
    shapes = SHAPES(5)
    w0 = {k: rng.standard_normal(s) for k, s in shapes.items()}
    sens = [{k: rng.standard_normal(s) for k, s in shapes.items()} for _ in range(3)]
    wouts = [w0] + [{k: w0[k] + 1e-2 * rng.standard_normal(s) for k, s in shapes.items()} for _ in range(4)]
    s0 = np.array([2.0, 0.7, 1.1])
    tab = np.array([[s0[s] + sum(np.sum(sens[s][k] * (w[k] - w0[k])) for k in shapes) for s in range(3)] for w in wouts])
    steps = np.concatenate([[1.0], rng.uniform(1e-3, 2e-3, 4)])
    want = (tab[1:] - tab[0]) / steps[1:, None]
    got = linearised_margin_gradient(sens, wouts, steps, s0)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


def test_linearised_dof_gradient_is_unchanged():
    """on the inputs of its own test (tests/test_geometry_vjp_cpu.py) the result equals, bit for bit, the loop it ran before it
    shared that loop with linearised_margin_gradient"""
    from ibs_amd.objective import WOUT_SENSITIVITY_KEYS, ballooning_objective, dof_fd_gradient, linearised_dof_gradient
    rng = np.random.default_rng(7)
    n_dof, n_s, ns = 4, 3, 5
    shapes = SHAPES(ns)
    w0 = {k: rng.standard_normal(s) for k, s in shapes.items()}
    sens = [{k: rng.standard_normal(s) for k, s in shapes.items()} for _ in range(n_s)]
    wouts = [w0] + [{k: w0[k] + 1e-2 * rng.standard_normal(s) for k, s in shapes.items()} for _ in range(n_dof)]
    gam0, thresh = np.array([0.05, -0.01, 0.002]), 1e-3
    f_other = rng.uniform(1.0, 2.0, n_dof + 1)
    steps = np.concatenate([[1.0], rng.uniform(1e-3, 2e-3, n_dof)])
    gam = np.tile(gam0, (n_dof + 1, 1))
    for k in range(1, n_dof + 1):
        for key in WOUT_SENSITIVITY_KEYS:
            d = np.asarray(wouts[k][key], dtype=np.float64) - np.asarray(w0[key], dtype=np.float64)
            if not np.any(d):
                continue
            for si in range(n_s):
                gam[k, si] += float(np.sum(np.asarray(sens[si][key]) * d))
    want = dof_fd_gradient(ballooning_objective(f_other, gam, thresh, 50.0), steps)
    assert np.array_equal(linearised_dof_gradient(sens, wouts, f_other, steps, gam0, gamma_thresh=thresh, prefac=50.0), want)


# ---- plumbing -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("nm") is None, reason="needs nm")
def test_library_exports_the_entry_point():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert NAME in names and NAME in _lib.SYMBOLS
    with open(os.path.join(ROOT, "include", "ibs.h")) as fh:
        assert "int %s(" % NAME in fh.read()
    assert callable(getattr(ibs_amd.Context, "marginal_obj_w_grad_tangent"))
    assert callable(ibs_amd.linearised_margin_gradient)
    for cls, name in ((ibs_amd.BallooningScan, "marginal_sensitivity"), (ibs_amd.AdjointStep, "marginal_sensitivity")):
        assert callable(getattr(cls, name))


def test_arguments_are_checked_before_any_device_work():
    """null context, null val, geo_da missing with jac or with dscale: IBS_ERR_ARG with "null" in the message; geo_da missing without
    either is accepted (the call gets as far as the grid check); even N and N outside [66, 65,537]: IBS_ERR_UNSUPPORTED.  The checks
    come before the context is touched, so a zeroed buffer stands for it (and for the arrays) where no GPU is present."""
    lib = _lib.lib()
    buf = C.create_string_buffer(1 << 16)
    p = C.cast(buf, C.c_void_p)
    fn = lambda ctx, n, val, gda=p, jac=None, dscale=None, geo_bar=None: lib.ibs_marginal_obj_w_grad_tangent_f64(
        ctx, 1, n, 0.05, p, gda, n, p, val, jac, None, dscale, None, geo_bar, None, 0)
    for args in ((None, 513, p), (p, 513, None), (p, 513, p, None, p), (p, 513, p, None, None, p), (p, 512, p, None, p)):
        assert fn(*args) == IBS_ERR_ARG, args
        assert b"null" in lib.ibs_last_error()
    for n in (512, 65, 65538, 65539):
        assert fn(p, n, p, p, p, p, p) == IBS_ERR_UNSUPPORTED, n
        assert fn(p, n, p, None) == IBS_ERR_UNSUPPORTED, n
        assert fn(p, n, p, None, None, None, p) == IBS_ERR_UNSUPPORTED, n


def test_context_method_checks_its_shapes():
    ctx = ibs_amd.Context.__new__(ibs_amd.Context)
    with pytest.raises(ibs_amd.IbsError):
        ctx.marginal_obj_w_grad_tangent(0.05, np.ones((7, 1, 67)), np.zeros((7, 1, 67)), np.zeros(1))
    with pytest.raises(ibs_amd.IbsError):
        ctx.marginal_obj_w_grad_tangent(0.05, np.ones((8, 1, 67)), np.zeros((8, 2, 67)), np.zeros(1))
    with pytest.raises(ibs_amd.IbsError):
        ctx.marginal_obj_w_grad_tangent(0.05, np.ones((8, 1, 67)), None, np.zeros(1))


def test_marginal_jac_option_of_the_drivers():
    """marginal(jac="exact_tangent") needs tables= and device=; unknown values (the gam drivers' "exact" among them) are refused before
    any work; AdjointStep.marginal passes the check on"""
    th = bo.theta_grid(129)
    scan = ibs_amd.BallooningScan(None, synthetic_fieldlines(th), th, [0.5])
    for jac in ("exact_tangent", "bogus", "exact", None):
        with pytest.raises(ibs_amd.IbsError):
            scan.marginal(jac=jac)
        with pytest.raises(ibs_amd.IbsError):
            scan.marginal(refine=True, jac=jac)
    with pytest.raises(ibs_amd.IbsError):
        scan.marginal_sensitivity()
    for jac in ("bogus", "exact"):
        with pytest.raises(ibs_amd.IbsError):
            ibs_amd.AdjointStep(None, th, [0.5], "cpu").marginal([], jac=jac)


def test_reference_mode_remembers_its_points_without_a_gpu():
    """marginal() through the CPU oracle context: jac="reference" is the default path, and the refined points are left on the object"""
    from tests import marginal_points_oracle as mpo
    th = bo.theta_grid(129)
    kw = dict(nalpha=3, ntheta0=2)
    a = ibs_amd.BallooningScan(mpo.MarginalPointsOracleContext(), synthetic_fieldlines(th), th, [0.5], **kw).marginal(refine=True, maxiter=3)
    scan = ibs_amd.BallooningScan(mpo.MarginalPointsOracleContext(), synthetic_fieldlines(th), th, [0.5], **kw)
    b = scan.marginal(refine=True, maxiter=3, jac="reference")
    assert set(a) == set(b)
    for key in a:
        assert np.array_equal(a[key], b[key]), key
    assert np.array_equal(scan._last_marginal_points, np.stack([b["alpha"], b["theta0"]], axis=1))


def test_new_translation_unit_has_no_scratch():
    """ibs_marginal_tangent.hip compiles for gfx950 with ScratchSize 0; the VGPR count is printed (target: two waves per SIMD, <= 256)"""
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-c", "--cuda-device-only", "-o", os.devnull,
                        "-Rpass-analysis=kernel-resource-usage", os.path.join(CSRC, "ibs_marginal_tangent.hip")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    name, scratch, vgprs = None, {}, {}
    for line in r.stderr.split("\n"):
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"remark:\s+ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name:
            scratch[name] = int(m.group(1))
        m = re.search(r"remark:\s+VGPRs: (\d+)", line)
        if m and name:
            vgprs[name] = int(m.group(1))
    print("ibs_marginal_tangent.hip VGPRs:", vgprs)
    assert any("k_marginal_tangent_points" in s for s in scratch), scratch
    assert all(v == 0 for v in scratch.values()), scratch
    assert all(v <= 256 for v in vgprs.values()), vgprs
