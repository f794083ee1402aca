"""GPU: the launch plan (csrc/ibs_plan.hpp) against what is really launched.  tests/golden/P1_parent_launches.json holds, for the
calls below, the (kernel name, blocks, threads) that ibs_last_launch reported at the commit before the planner was cut out of the
C-ABI layer, and the CU count of the device they were recorded on; this library must report the same triples for the same calls.

The calls are small: golden NCSX lines (tests/golden/G3_ncsx_lines.npz) interpolated onto the grid and tiled, s-alpha rows for the raw
solves.  Only the launch record is compared with the fixture; every call is made twice and its outputs must carry the same bits both
times (a fault or a race would show there).  The plan depends on the CU count, so a device with another count than the recorded one
fails the test with a message that says so: the fixture then has to be recorded again on that device, from the parent commit."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

from oracle import ballooning_oracle as bo

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
FIXTURE = os.path.join(G, "P1_parent_launches.json")


@functools.lru_cache(maxsize=None)
def lines(N, n):
    """(h, geo (n, 8, N), dPdrho (n,)): the 16 golden lines on the N-point grid, repeated to n lines"""
    g3 = np.load(os.path.join(G, "G3_ncsx_lines.npz"))
    src, th513, th = g3["geo_513"], bo.theta_grid(513), bo.theta_grid(N)
    if N != 513:
        src = np.stack([np.stack([np.interp(th, th513, ln[k]) for k in range(8)]) for ln in src])
    k = np.arange(n) % len(src)
    return float(th[1] - th[0]), np.ascontiguousarray(src[k]), np.ascontiguousarray(g3["dPdrho_513"][k])


@functools.lru_cache(maxsize=None)
def rows(N, n, dtype):
    """(h, g, c) of n s-alpha systems (16 distinct ones, repeated), f = g"""
    th = bo.theta_grid(N)
    base = [bo.salpha_gc(th, 0.4 + 0.1 * i, 0.5 + 0.07 * i, 0.05 * i) for i in range(16)]
    k = np.arange(n) % 16
    g = np.stack([b[0] for b in base])[k].astype(dtype)
    c = np.stack([b[1] for b in base])[k].astype(dtype)
    return float(th[1] - th[0]), g, c


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(torch.device("cuda:0"))


def scan_call(N, n_lines, n_t0, opts=(), warm=False, **kw):
    def run(ctx):
        h, geo, dP = lines(N, n_lines)
        a = [dev(geo[:, k, :]) for k in range(7)]
        d_dP, t0 = dev(dP), dev(np.linspace(0.0, 1.5, n_t0))
        if warm:
            cold = ctx.gamma_scan(h, *a, d_dP, t0)
            kw.update(lam_guess=cold["lam"], guess_width=1e-3)
        return lambda: ctx.gamma_scan(h, *a, d_dP, t0, want_info=True, **kw)
    return dict(opts), run


def points_call(N, n):
    def run(ctx):
        h, geo, dP = lines(N, n)
        a = [dev(geo[:, k, :]) for k in range(7)]
        d_dP, t0 = dev(dP), dev(np.linspace(0.0, 1.0, n))
        return lambda: ctx.gamma_points(h, *a, d_dP, t0, want_info=True)
    return {}, run


def argmax_call(N, n_lines, n_t0, n_surf):
    def run(ctx):
        h, geo, dP = lines(N, n_lines)
        a = [dev(geo[:, k, :]) for k in range(7)]
        d_dP, t0 = dev(dP), dev(np.linspace(0.0, 1.5, n_t0))
        return lambda: ctx.gamma_scan_argmax(h, a, d_dP, t0, n_surf)
    return {}, run


def gcf_call(N, n_sys, opts=(), dtype=np.float64, **kw):
    def run(ctx):
        h, g, c = rows(N, n_sys, dtype)
        dg, dc = dev(g), dev(c)
        return lambda: ctx.solve_gcf(h, dg, dc, dg, want_info=True, dtype=dtype, **kw)
    return dict(opts), run


def grad_call(N, n):
    def run(ctx):
        h, geo, _ = lines(N, 3 * n)
        d_geo, t0 = dev(geo.reshape(n, 3, 8, N)), dev(np.linspace(0.0, 1.0, n))
        return lambda: dict(zip(("val", "jac", "info"), ctx.obj_w_grad(h, d_geo, t0, want_info=True)))
    return {}, run


def sturm_call(N, n_sys, form):
    def run(ctx):
        h, g, c = rows(N, n_sys, np.float64)
        dg, dc, sh = dev(g), dev(c), dev(np.linspace(-1.0, 1.0, n_sys))
        return lambda: dict(count=ctx.sturm_count(h, dg, dc, dg, sh))
    return {"sturm_form": form}, run


CALLS = {
    "scan_131_8x5": scan_call(131, 8, 5),
    "scan_131_1024x8_p64_chain1": scan_call(131, 1024, 8, {"force_p": 64, "scan_chain": 1}),
    "scan_131_1024x8": scan_call(131, 1024, 8),
    "scan_131_64x4_p32": scan_call(131, 64, 4, {"force_p": 32}),
    "scan_131_64x3_p32": scan_call(131, 64, 3, {"force_p": 32}),
    "scan_131_64x4_p16": scan_call(131, 64, 4, {"force_p": 16}),
    "scan_131_64x3_p16": scan_call(131, 64, 3, {"force_p": 16}),
    "scan_131_8x5_warm": scan_call(131, 8, 5, warm=True),
    "scan_131_8x5_warm_X": scan_call(131, 8, 5, warm=True, want_X=True),
    "scan_131_64x4_p32_warm": scan_call(131, 64, 4, {"force_p": 32}, warm=True),
    "scan_513_8x8": scan_call(513, 8, 8),
    "scan_513_9x8": scan_call(513, 9, 8),
    "scan_1025_16x3": scan_call(1025, 16, 3),
    "scan_2051_2x2": scan_call(2051, 2, 2),
    "points_131_5": points_call(131, 5),
    "argmax_131_8x5_2surf": argmax_call(131, 8, 5, 2),
    "gcf_131_3": gcf_call(131, 3),
    "gcf_131_4096": gcf_call(131, 4096),
    "gcf_131_4096_p32": gcf_call(131, 4096, {"force_p": 32}),
    "gcf_131_4096_p16": gcf_call(131, 4096, {"force_p": 16}),
    "gcf_1537_8_rows0": gcf_call(1537, 8, {"gcf_rows": 0}),
    "gcf_1537_8_rows1": gcf_call(1537, 8, {"gcf_rows": 1}),
    "gcf_1795_8_direct1": gcf_call(1795, 8, {"gcf_direct": 1}),
    "gcf_1795_8_direct1_X": gcf_call(1795, 8, {"gcf_direct": 1}, want_X=True),
    "gcf32_131_64_lam_f32lam1": gcf_call(131, 64, {"f32_lam": 1}, np.float32, want_gam=False),
    "gcf32_131_64_lam_f32lam2": gcf_call(131, 64, {"f32_lam": 2}, np.float32, want_gam=False),
    "gcf32_131_64_gam_f32lam1": gcf_call(131, 64, {"f32_lam": 1}, np.float32),
    "gcf32_131_64_gam_f32lam2": gcf_call(131, 64, {"f32_lam": 2}, np.float32),
    "gcf_2051_3": gcf_call(2051, 3),
    "grad_131_3": grad_call(131, 3),
    "grad_131_600": grad_call(131, 600),
    "sturm_1025_64_form0": sturm_call(1025, 64, 0),
    "sturm_1025_64_form1": sturm_call(1025, 64, 1),
    "sturm_1025_64_form2": sturm_call(1025, 64, 2),
    "sturm_1025_64_form3": sturm_call(1025, 64, 3),
}


def last_launch(ctx):
    buf, nb, nt = C.create_string_buffer(96), C.c_int64(0), C.c_int32(0)
    ctx._lib.ibs_last_launch(buf, 96, C.byref(nb), C.byref(nt))
    return [buf.value.decode(), int(nb.value), int(nt.value)]


def launch_of(ctx, key):
    """the call `key` made twice under its options: its launch record; the outputs of the two invocations must carry the same bits"""
    import torch
    opts, prepare = CALLS[key]
    try:
        for k, v in opts.items():
            ctx.set_option(k, v)
        call = prepare(ctx)
        first = call()
        rec = last_launch(ctx)
        second = call()
        torch.cuda.synchronize()
        assert last_launch(ctx) == rec, (key, rec, last_launch(ctx))
    finally:
        ctx.reset_options()
    for k, v in first.items():
        if hasattr(v, "cpu") and v is not None:
            assert np.array_equal(v.cpu().numpy(), second[k].cpu().numpy(), equal_nan=v.is_floating_point()), (key, k)
    return rec


@pytest.fixture(scope="module")
def ctx():
    import ibs_amd
    c = ibs_amd.Context(0)
    yield c
    c.reset_options()
    c.close()


@pytest.fixture(scope="module")
def recorded():
    import torch
    with open(FIXTURE) as fh:
        fx = json.load(fh)
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    assert n_cu == fx["n_cu"], ("this device has %d CUs, tests/golden/P1_parent_launches.json was recorded with %d: launch shapes "
                                "depend on the CU count, so the fixture must be recorded again on this device, from the commit before "
                                "csrc/ibs_plan.hpp" % (n_cu, fx["n_cu"]))
    assert set(fx["launches"]) == set(CALLS), sorted(set(fx["launches"]) ^ set(CALLS))
    return fx["launches"]


@pytest.mark.parametrize("key", sorted(CALLS))
def test_launch_equals_the_recorded_one(ctx, recorded, key):
    assert launch_of(ctx, key) == recorded[key], key
