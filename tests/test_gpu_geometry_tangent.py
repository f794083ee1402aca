"""GPU: ibs_fieldline_geometry_dalpha_f64 (Context.fieldline_geometry_dalpha) against the jvp oracle of
tests/geometry_tangent_oracle.py, against the alpha_bar of ibs_fieldline_geometry_vjp_f64 (the adjoint identity), and its
batch / pointer / padding / NaN behaviour."""
import copy
import ctypes as C
import os

import numpy as np
import pytest

import ibs_amd
from ibs_amd import _lib
from tests import geometry_tangent_oracle as to
from tests import geometry_vjp_oracle as vo
from tests.test_gpu_geometry_vjp import BAR, LINE_ALPHA, LINE_SURF, SVALS, _subset_wout

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def ctx():
    return ibs_amd.Context(0)


@pytest.fixture(scope="module")
def wout():
    return dict(np.load(os.path.join(G, "G8_wout_ncsx_op.npz")))


_TABS = {}


def _tables(wout, modes):
    """the mode tables of test_vjp_against_the_oracle's cases: full, or the 37 + 53 mode subset"""
    if modes not in _TABS:
        w = wout
        if modes == "subset":
            rng = np.random.default_rng(3)
            kmn = np.sort(np.concatenate([np.arange(8), 8 + rng.choice(len(wout["xm"]) - 8, 29, replace=False)]))
            knq = np.sort(np.concatenate([np.arange(8), 8 + rng.choice(len(wout["xm_nyq"]) - 8, 45, replace=False)]))
            w = _subset_wout(wout, kmn, knq)
        _TABS[modes] = ibs_amd.SurfaceTables.from_wout(w, SVALS)
    return _TABS[modes]


def _oracle(tabs, ls, la, th, reverse_modes=False):
    return to.dalpha(tabs.xm, tabs.xn, tabs.xm_nyq, tabs.xn_nyq, tabs.tab_mn, tabs.tab_nyq, tabs.scal, ls, la, th, reverse_modes)


def _plane_ratios(got, ref):
    return np.abs(got - ref).max(axis=(1, 2)) / np.abs(ref).max(axis=(1, 2))


_CASES = {}


def _case(wout, modes, N, lines):
    key = (modes, N, lines)
    if key not in _CASES:
        tabs = _tables(wout, modes)
        ls, la = (LINE_SURF, LINE_ALPHA) if lines == 7 else (np.array([3], dtype=np.int32), np.array([1.3]))
        th = ibs_amd.theta_grid(N)
        geo, geo_da, dP, _ = _oracle(tabs, ls, la, th)
        rev = _oracle(tabs, ls, la, th, reverse_modes=True)[1]
        modes_d = dict(xm=tabs.xm, xn=tabs.xn, xm_nyq=tabs.xm_nyq, xn_nyq=tabs.xn_nyq)
        _CASES[key] = dict(tabs=tabs, ls=ls, la=la, th=th, geo=geo, geo_da=geo_da, dP=dP, rev=rev,
                           np_geo=vo.numpy_forward(modes_d, tabs.tab_mn, tabs.tab_nyq, tabs.scal, ls, la, th)[0])
    return _CASES[key]


@pytest.mark.parametrize("modes,N,lines", [("full", 67, 7), ("full", 131, 7), ("subset", 67, 7), ("subset", 131, 7), ("full", 131, 1),
                                           ("subset", 67, 1)])
def test_tangent_against_the_oracle(ctx, wout, modes, N, lines):
    """the six cases of test_vjp_against_the_oracle: for every plane max|delta| / max|oracle| <= that test's BAR = 3.1e-12 (10 x the
    larger of the forward kernel's ratio against oracle/geometry_oracle and the oracle's order-of-summation spread, by that test's
    rule).  The forward ratio, the tangent oracle's own spread (mode order reversed) and the kernel's ratio are printed.  Measured on
    an MI355X (docs/EXPERIMENTS.md R6.13): forward 4.5e-15 .. 3.1e-13, spread 2.0e-15 .. 1.7e-14, the kernel 6.6e-15 .. 1.5e-14."""
    c = _case(wout, modes, N, lines)
    tabs, ls, la, th = c["tabs"], c["ls"], c["la"], c["th"]
    fwd = 0.0
    for use_rows in (True, False):
        g = ctx.fieldline_geometry(tabs, ls, la, th, use_rows=use_rows)["geo"]
        fwd = max(fwd, float(_plane_ratios(g, c["np_geo"]).max()))
    spread = float(_plane_ratios(c["rev"], c["geo_da"]).max())
    got = ctx.fieldline_geometry_dalpha(tabs, ls, la, th)["geo_da"]
    assert ctx.last_launch()[0] == "ibs::k_geo_dalpha_points", ctx.last_launch()
    r = _plane_ratios(got, c["geo_da"])
    print("case %s N=%d lines=%d: forward %.2e  tangent-oracle spread %.2e  bar %.2e  tangent %.2e" % (modes, N, lines, fwd, spread, BAR, r.max()))
    assert r.max() <= BAR, (r, BAR)


def test_adjoint_identity_with_the_vjp_kernel(ctx, wout):
    """sum geo_bar geo_da (+ dPdrho_bar x 0: dPdrho has no alpha-tangent) = alpha_bar of ibs_fieldline_geometry_vjp_f64 on the same
    geo_bar / dPdrho_bar, per line, to 1e-11 relative (the floor of _fd_check: both sides are the same plain-form arithmetic;
    measured 2.7e-15 .. 1.4e-14)"""
    for key in (("full", 67, 7), ("subset", 131, 7)):
        c = _case(wout, *key)
        tabs, ls, la, th = c["tabs"], c["ls"], c["la"], c["th"]
        rng = np.random.default_rng(17)
        gb = rng.standard_normal(c["geo"].shape) / np.abs(c["geo"]).max(axis=(1, 2), keepdims=True)
        db = rng.standard_normal(len(ls)) / np.abs(c["dP"]).max()
        got = ctx.fieldline_geometry_dalpha(tabs, ls, la, th)["geo_da"]
        lhs = np.sum(gb * got, axis=(0, 2))
        for dbar in (None, db):
            bar = ctx.fieldline_geometry_vjp(tabs, ls, la, th, gb, dbar, want=("alpha",))["alpha_bar"]
            rel = np.abs(lhs - bar) / np.abs(bar)
            print("adjoint identity %s dPdrho_bar %s: worst relative %.2e" % (key, dbar is not None, rel.max()))
            assert (rel <= 1e-11).all(), (lhs, bar)


@pytest.mark.parametrize("N", [2, 3, 63, 64, 65, 129])
def test_tangent_on_block_edges(ctx, wout, N):
    """N = 2, 3, one short of / exactly / one past a 64-thread block, two blocks + 1, and lines with alpha = -0.7 and 4.0 (outside
    the scan's [0, pi]): against the oracle with the same bar"""
    tabs = _tables(wout, "subset")
    ls = np.array([1, 3, 0], dtype=np.int32); la = np.array([-0.7, 4.0, 1.9])
    th = np.linspace(-np.pi, np.pi, N)
    ref = _oracle(tabs, ls, la, th)[1]
    got = ctx.fieldline_geometry_dalpha(tabs, ls, la, th)["geo_da"]
    r = _plane_ratios(got, ref)
    print("N=%d: tangent %.2e" % (N, r.max()))
    assert r.max() <= BAR, (N, r)


def _raw_host_call(ctx, tabs, ls, la, th, out, ld):
    """the C entry point with host pointers and a row pitch ld >= N"""
    p = lambda a: C.c_void_p(a.ctypes.data)
    host = [tabs.xm, tabs.xn, tabs.xm_nyq, tabs.xn_nyq, tabs.tab_mn, tabs.tab_nyq, tabs.scal]
    ls = np.ascontiguousarray(ls, dtype=np.int32); la = np.ascontiguousarray(la, dtype=np.float64); th = np.ascontiguousarray(th)
    _lib.check(_lib.lib().ibs_fieldline_geometry_dalpha_f64(ctx._h, len(tabs.s), len(tabs.xm), len(tabs.xm_nyq), *[p(a) for a in host],
                                                            len(ls), p(ls), p(la), len(th), p(th), ld, p(out), _lib.MEM_HOST),
               "ibs_fieldline_geometry_dalpha_f64")
    return out


def test_batch_order_pointers_and_padding(ctx, wout):
    """lines in reversed order give the same bits per line; a line alone gives its batch bits; host and device pointers (numpy or
    device index arrays) agree bit for bit; with ld = N + 5 (host and device) and the output pre-filled with NaN the padding is still NaN"""
    import torch
    c = _case(wout, "full", 67, 7)
    tabs, ls, la, th = c["tabs"], c["ls"], c["la"], c["th"]
    N, n = len(th), len(ls)
    got = ctx.fieldline_geometry_dalpha(tabs, ls, la, th)["geo_da"]
    assert np.isfinite(got).all()
    assert np.array_equal(ctx.fieldline_geometry_dalpha(tabs, ls, la, th)["geo_da"], got)
    rev = ctx.fieldline_geometry_dalpha(tabs, ls[::-1], la[::-1], th)["geo_da"]
    assert np.array_equal(rev[:, ::-1], got)
    for k in (0, 3, n - 1):
        one = ctx.fieldline_geometry_dalpha(tabs, ls[k:k + 1], la[k:k + 1], th)["geo_da"]
        assert np.array_equal(one[:, 0], got[:, k]), k
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d1 = ctx.fieldline_geometry_dalpha(tabs, t(ls), t(la), t(th), device=dev)["geo_da"]
    d2 = ctx.fieldline_geometry_dalpha(tabs, ls, la, th, device=dev)["geo_da"]
    assert d1.is_cuda and np.array_equal(d1.cpu().numpy(), got) and np.array_equal(d2.cpu().numpy(), got)
    ld = N + 5
    pad = _raw_host_call(ctx, tabs, ls, la, th, np.full((8, n, ld), np.nan), ld)
    assert np.array_equal(pad[:, :, :N], got) and np.isnan(pad[:, :, N:]).all()
    dpad = torch.full((8, n, ld), float("nan"), dtype=torch.float64, device=dev)
    keep = [t(a) for a in (tabs.xm, tabs.xn, tabs.xm_nyq, tabs.xn_nyq, tabs.tab_mn, tabs.tab_nyq, tabs.scal)] + [t(ls), t(la), t(th)]
    p = lambda x: C.c_void_p(x.data_ptr())
    ctx._stream_from_torch(dpad)
    _lib.check(_lib.lib().ibs_fieldline_geometry_dalpha_f64(ctx._h, len(tabs.s), len(tabs.xm), len(tabs.xm_nyq), *[p(x) for x in keep[:7]],
                                                            n, p(keep[7]), p(keep[8]), N, p(keep[9]), ld, p(dpad), _lib.MEM_DEVICE),
               "ibs_fieldline_geometry_dalpha_f64")
    dpad = dpad.cpu().numpy()
    assert np.array_equal(dpad[:, :, :N], got) and np.isnan(dpad[:, :, N:]).all()


def test_nan_alpha_stays_on_its_line(ctx, wout):
    """a NaN alpha gives NaN in that line's rows only; NaN iota of one surface in the rows of that surface's lines only"""
    c = _case(wout, "subset", 67, 7)
    tabs, ls, la, th = c["tabs"], c["ls"], c["la"], c["th"]
    clean = ctx.fieldline_geometry_dalpha(tabs, ls, la, th)["geo_da"]
    bad_a = la.copy(); bad_a[4] = np.nan
    got = ctx.fieldline_geometry_dalpha(tabs, ls, bad_a, th)["geo_da"]
    keep = np.arange(len(ls)) != 4
    assert np.isnan(got[:, 4]).all() and np.array_equal(got[:, keep], clean[:, keep])
    bad = copy.copy(tabs)
    bad.__dict__.pop("_device_copies", None)
    bad.scal = tabs.scal.copy(); bad.scal[0, 1] = np.nan
    got = ctx.fieldline_geometry_dalpha(bad, ls, la, th)["geo_da"]
    on0 = ls == 0
    assert np.isnan(got[:, on0]).all() and np.array_equal(got[:, ~on0], clean[:, ~on0])
