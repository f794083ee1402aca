"""CPU: the alpha-tangent of the field-line geometry -- its torch oracle (tests/geometry_tangent_oracle.py) against central
differences of the numpy oracle, against the oracle VJP's alpha_bar, and the plumbing of ibs_fieldline_geometry_dalpha_f64 and
ibs_obj_w_grad_exact_tangent_f64 (export, argument checks, kernel resources, the jac="exact_tangent" option)."""
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
from tests.helpers import synthetic_fieldlines

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ideal-ballooning-solver_amd", "csrc")
LIB = os.path.join(ROOT, "ideal-ballooning-solver_amd", "lib", "libibs_hip.so")
G = os.path.join(ROOT, "tests", "golden")
NAMES = ("ibs_fieldline_geometry_dalpha_f64", "ibs_obj_w_grad_exact_tangent_f64")


@pytest.fixture(scope="module")
def case():
    """G8 tables, N = 67, 3 lines on 2 surfaces, the oracle's forward and alpha-tangent, a fixed random functional"""
    d = dict(np.load(os.path.join(G, "G8_surface_tables.npz")))
    tab_mn, tab_nyq, scal = vo.packed(d)
    theta = ibs_amd.theta_grid(67)
    ls, la = np.array([1, 0, 1]), np.array([0.3, 1.1, 2.0])
    args = (d["xm"], d["xn"], d["xm_nyq"], d["xn_nyq"], tab_mn, tab_nyq, scal, ls)
    geo, geo_da, dP, dP_da = to.dalpha(*args, la, theta)
    rng = np.random.default_rng(11)
    gb = rng.standard_normal(geo.shape) / np.abs(geo).max(axis=(1, 2), keepdims=True)
    db = rng.standard_normal(3) / np.abs(dP).max()
    fwd = lambda al: vo.numpy_forward(d, tab_mn, tab_nyq, scal, ls, al, theta)[0]
    return dict(d=d, args=args, theta=theta, ls=ls, la=la, geo=geo, geo_da=geo_da, dP=dP, dP_da=dP_da, gb=gb, db=db, fwd=fwd)


def _fd_check(f, value, eps):
    """the rule of _fd_check in tests/test_geometry_vjp_cpu.py: central differences at eps and eps / 2; the error of the one at eps / 2
    is a third of its distance to the one at eps, 4 x covers the higher-order terms"""
    fd1 = (f(eps) - f(-eps)) / (2 * eps)
    fd2 = (f(eps / 2) - f(-eps / 2)) / eps
    self_diff = abs(fd1 - fd2)
    print("tangent %.12e  fd %.12e  self-difference %.2e (rel %.2e)" % (value, fd2, self_diff, self_diff / abs(fd2)))
    assert self_diff <= 1e-5 * abs(fd2), "the finite difference itself is useless here"
    assert abs(value - fd2) <= 4 * self_diff + 1e-11 * abs(fd2)


@pytest.mark.parametrize("plane", range(8))
def test_oracle_tangent_against_central_differences(case, plane):
    """per plane and line: a fixed random functional of the plane's row, its tangent against central differences of
    vo.numpy_forward in that line's alpha.  Steps 1e-4 and 5e-5, as the alpha check of tests/test_gpu_geometry_vjp.py: the numpy
    oracle's root solve leaves ~1e-13 of noise in a row, 1e-8 of the derivative at a step of 1e-5 and below the rule's own
    self-difference (truncation, ~1e-7) at 1e-4"""
    c = case
    for line in range(3):
        w = c["gb"][plane, line]
        e_l = np.zeros(3); e_l[line] = 1.0
        _fd_check(lambda e: float(np.sum(c["fwd"](c["la"] + e * e_l)[plane, line] * w)), float(np.sum(c["geo_da"][plane, line] * w)), 1e-4)


def test_central_difference_gap_quarters_per_halving(case):
    """the gap between the tangent and the central difference of the eight arrays at half-steps 0.004 / 0.002 / 0.001 is a pure
    step-squared term: it shrinks by a factor in [3.5, 4.5] per halving (measured: 4.00), and at upstream's 0.002 it is 3e-5 .. 3e-4
    of a plane's maximum"""
    c = case
    gaps = []
    for hs in (0.004, 0.002, 0.001):
        cd = (c["fwd"](c["la"] + hs) - c["fwd"](c["la"] - hs)) / (2 * hs)
        gaps.append(np.abs(cd - c["geo_da"]).max(axis=(1, 2)) / np.abs(c["geo_da"]).max(axis=(1, 2)))
    gaps = np.array(gaps)
    print("gap / plane maximum at half-steps 0.004, 0.002, 0.001:\n", gaps, "\nratios:\n", gaps[:-1] / gaps[1:])
    assert np.all(gaps[:-1] / gaps[1:] >= 3.5) and np.all(gaps[:-1] / gaps[1:] <= 4.5)


def test_adjoint_identity_with_the_oracle_vjp(case):
    """sum geo_bar d geo / d alpha + dPdrho_bar d dPdrho / d alpha = alpha_bar of vo.vjp, per line, to 1e-12 relative
    (measured: 5e-16)"""
    c = case
    bar = vo.vjp(*c["args"], c["la"], c["theta"], c["gb"], c["db"])["alpha_bar"]
    lhs = np.sum(c["gb"] * c["geo_da"], axis=(0, 2)) + c["db"] * c["dP_da"]
    print("adjoint identity:", lhs, bar, np.abs(lhs - bar) / np.abs(bar))
    assert np.all(np.abs(lhs - bar) <= 1e-12 * np.abs(bar))


def test_dPdrho_has_no_alpha_tangent(case):
    """|d dPdrho / d alpha| <= 1e-13 |dPdrho| (measured: 2e-16): (cvdrift - gbdrift) bmag^2 is a surface constant"""
    c = case
    print("d dPdrho / d alpha / dPdrho:", c["dP_da"] / c["dP"])
    assert np.all(np.abs(c["dP_da"]) <= 1e-13 * np.abs(c["dP"]))


def test_oracle_row_tangents_against_central_differences(case):
    """rows_dalpha (the formulas of line_gcf_tangent) against central differences of rows() at fixed dPdrho"""
    c = case
    t0 = np.array([0.2, 0.0, 0.7])
    dP = c["dP"]
    rng = np.random.default_rng(5)
    for k, got in enumerate(to.rows_dalpha(c["geo"], c["geo_da"], t0)):
        w = rng.standard_normal(got.shape) / np.abs(got).max()
        _fd_check(lambda e: float(np.sum(to.rows(c["fwd"](c["la"] + e), t0, dP)[k] * w)), float(np.sum(got * w)), 1e-4)


# ---- plumbing ---------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("nm") is None, reason="needs nm")
def test_library_exports_the_entry_points():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    with open(os.path.join(ROOT, "include", "ibs.h")) as fh:
        header = fh.read()
    for name in NAMES:
        assert name in names and name in _lib.SYMBOLS and "int %s(" % name in header, name
    assert hasattr(ibs_amd.Context, "fieldline_geometry_dalpha") and hasattr(ibs_amd.Context, "obj_w_grad_exact_tangent")


def test_geometry_entry_argument_errors_need_no_gpu():
    """every argument check comes before the context is touched: a placeholder block of memory stands in for it"""
    lib = _lib.lib()
    fn = getattr(lib, NAMES[0])
    ERR_ARG = -1
    N, nl, ns_, mn, mq = 67, 2, 2, 3, 4
    z = lambda *s: np.zeros(s)
    a = dict(xm=z(mn), xn=z(mn), xmq=z(mq), xnq=z(mq), tmn=z(ns_, 6, mn), tnq=z(ns_, 7, mq), sc=z(ns_, 6), ls=np.zeros(nl, np.int32),
             la=z(nl), th=z(N), out=z(8, nl, N))
    fake = C.create_string_buffer(1 << 16)

    def call(ctx=fake, n_lines=nl, ld=N, null=(), **over):
        b = dict(a); b.update(over)
        p = lambda k: None if k in null else C.c_void_p(b[k].ctypes.data)
        return fn(ctx, ns_, mn, mq, p("xm"), p("xn"), p("xmq"), p("xnq"), p("tmn"), p("tnq"), p("sc"), n_lines, p("ls"), p("la"),
                  N, p("th"), ld, p("out"), _lib.MEM_HOST)
    assert call(ctx=None) == ERR_ARG and b"null context" in lib.ibs_last_error()
    for k in ("xm", "xn", "xmq", "xnq", "tmn", "tnq", "sc", "ls", "la", "th", "out"):
        assert call(null=(k,)) == ERR_ARG, k
    assert call(n_lines=-1) == ERR_ARG
    assert call(ld=N - 1) == ERR_ARG and b"ld" in lib.ibs_last_error()
    assert call(ls=np.array([0, 2], np.int32)) == ERR_ARG and b"out of range" in lib.ibs_last_error()


def test_point_entry_argument_errors_need_no_gpu():
    lib = _lib.lib()
    fn = getattr(lib, NAMES[1])
    ERR_ARG, ERR_UNSUPPORTED = -1, -3
    n = 2
    fake = C.create_string_buffer(1 << 16)

    def call(N=67, ctx=fake, ld=None, null=()):
        a = dict(geo=np.ones((8, n, N)), da=np.zeros((8, n, N)), t0=np.zeros(n), val=np.zeros(n), jac=np.zeros((n, 2)))
        p = lambda k: None if k in null else C.c_void_p(a[k].ctypes.data)
        return fn(ctx, n, N, 0.1, p("geo"), p("da"), N if ld is None else ld, p("t0"), None, p("val"), p("jac"), None, None, None, None,
                  _lib.MEM_HOST)
    assert call(ctx=None) == ERR_ARG and b"null context" in lib.ibs_last_error()
    for k in ("geo", "da", "t0", "val", "jac"):
        assert call(null=(k,)) == ERR_ARG, k
    assert call(ld=66) == ERR_ARG
    for N in (512, 65, 65539):
        assert call(N=N) == ERR_UNSUPPORTED, N


def test_error_codes_are_the_headers():
    with open(os.path.join(ROOT, "include", "ibs.h")) as fh:
        header = fh.read()
    assert re.search(r"#define IBS_ERR_ARG \(-1\)", header) and re.search(r"#define IBS_ERR_UNSUPPORTED \(-3\)", header)


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")
@pytest.mark.parametrize("unit,kernels", [("ibs_geometry_tangent.hip", ("k_geo_dalpha_points",)),
                                          ("ibs_exact_tangent.hip", ("k_exact_tangent_pointsILb0", "k_exact_tangent_pointsILb1"))])
def test_new_translation_units_have_no_scratch(unit, kernels):
    """both new translation units compile for gfx950 with ScratchSize 0 for every kernel; the VGPR counts are printed"""
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-c", "--cuda-device-only", "-o", os.devnull,
                        "-Rpass-analysis=kernel-resource-usage", os.path.join(CSRC, unit)], capture_output=True, text=True)
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
    print(unit, "VGPRs:", vgprs)
    for k in kernels:
        assert any(k in s for s in scratch), (k, scratch)
    assert all(v == 0 for v in scratch.values()), scratch


def test_exact_tangent_needs_tables_and_unknown_jac_is_refused():
    th = bo.theta_grid(129)
    with pytest.raises(ibs_amd.IbsError):
        ibs_amd.BallooningScan(None, synthetic_fieldlines(th), th, [0.5], jac="exact_tangent")
    with pytest.raises(ibs_amd.IbsError):
        ibs_amd.BallooningScan(None, synthetic_fieldlines(th), th, [0.5], jac="bogus")
    with pytest.raises(ibs_amd.IbsError):
        ibs_amd.AdjointStep(None, th, [0.5], "cpu", jac="bogus")
    assert ibs_amd.AdjointStep(None, th, [0.5], "cpu", jac="exact_tangent").jac == "exact_tangent"
