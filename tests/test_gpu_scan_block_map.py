"""GPU: the block -> (line, part) map of the one-wave theta0 scans (csrc/ibs_scan_map.hpp: a 3-D grid, x = line within its chunk of
8, y = part, z = chunk; a column of the last chunk without a line returns at once) on launches with one chunk, a full chunk, and a
last chunk of one line, with one to eight blocks per line.

Per-system arithmetic does not depend on the map, so a batched call must return, bit for bit, the concatenation of one-line calls
of the same library (one-line launches have one chunk and no idle block).  Every output is pre-filled with a NaN sentinel (info:
the bits of a quiet NaN), the calls go through the C ABI on those buffers, and no sentinel may survive: a (line, part) no block
took shows as a sentinel, one taken by the wrong block as wrong bits.

Shapes: n_lines in {1, 7, 8, 9, 17} x n_theta0 in {1, 3, 5, 8} at N = 131 (M = 3; these launches run one wave per block, so a line
has n_theta0 parts), one case at N = 513 (M = 8); the plain, the warm-started and the per-line theta0 entry points; one chained
launch (scan_chain = 2).  force_p = 64 keeps the sub-wave kernels, which N = 131 admits, out of the dispatch.  Geometry: the
perturbed golden NCSX lines of tests/test_gpu_scan_handoff.py (host_case).

Tolerances: none; equal bits throughout.  The fused maxima are numpy's first maximum of the plain scan's gam."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import ballooning_oracle as bo
from tests.test_gpu_scan_handoff import host_case

pytestmark = pytest.mark.gpu

LINES = [1, 7, 8, 9, 17]
THETA0S = [1, 3, 5, 8]
INFO_SENTINEL = 0x7FC00000          # the bits of a quiet NaN (float32): no status word looks like it


def rows_per_lane(N):
    return (N - 2 + 63) // 64


@pytest.fixture(scope="module")
def ctx():
    import ibs_amd
    c = ibs_amd.Context(0)
    c.set_option("force_p", 64)
    yield c
    c.reset_options()
    c.close()


@functools.lru_cache(maxsize=None)
def device_case(n_lines, N):
    """(h, seven geometry tensors (n_lines, N), dPdrho (n_lines,)) on the device: built once per shape, read only"""
    import torch
    dev = torch.device("cuda:0")
    geo, dP = host_case(n_lines, N, 4242 + 17 * n_lines + N)
    th = bo.theta_grid(N)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return float(th[1] - th[0]), [up(geo[:, k]) for k in range(7)], up(dP)


def theta0_grid(n):
    import torch
    return torch.from_numpy(np.linspace(0.0, 1.4, n) if n > 1 else np.array([0.3])).to(torch.device("cuda:0"))


def call(ctx, h, geo, dP, t0, lam_guess=None, width=1e-3, points=False):
    """one call of the C ABI on sentinel-filled device buffers: dict(gam, lam, info) as host arrays, and the launch"""
    import torch
    from ibs_amd import _lib
    MEM_DEVICE, check = _lib.MEM_DEVICE, _lib.check
    n_lines, N = geo[0].shape
    n_t0 = 1 if points else int(t0.shape[0])
    shape = (n_lines,) if points else (n_lines, n_t0)
    gam = torch.full(shape, float("nan"), dtype=torch.float64, device=dP.device)
    lam = torch.full(shape, float("nan"), dtype=torch.float64, device=dP.device)
    info = torch.full(shape, INFO_SENTINEL, dtype=torch.int32, device=dP.device)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(None)
    geo = [g.contiguous() for g in geo]
    ctx._stream_from_torch(geo[0])
    lib, none = ctx._lib, C.c_void_p(None)
    if points:
        check(lib.ibs_gamma_points_f64(ctx._h, n_lines, N, h, *[p(g) for g in geo], N, p(dP), p(t0), p(gam), p(lam), none, none, none,
                                       p(info), MEM_DEVICE), "ibs_gamma_points_f64")
    elif lam_guess is not None:
        check(lib.ibs_gamma_scan_warm_f64(ctx._h, n_lines, n_t0, N, h, *[p(g) for g in geo], N, p(dP), p(t0), p(lam_guess), width,
                                          p(gam), p(lam), none, none, none, p(info), MEM_DEVICE), "ibs_gamma_scan_warm_f64")
    else:
        check(lib.ibs_gamma_scan_f64(ctx._h, n_lines, n_t0, N, h, *[p(g) for g in geo], N, p(dP), p(t0), p(gam), p(lam), none, none,
                                     none, p(info), MEM_DEVICE), "ibs_gamma_scan_f64")
    torch.cuda.synchronize()
    return dict(gam=gam.cpu().numpy(), lam=lam.cpu().numpy(), info=info.cpu().numpy()), ctx.last_launch()


def bits(a):
    return a.view(np.int64) if a.dtype == np.float64 else a


def batched_equals_lines(ctx, n_lines, N, t0, tag, name, lam_guess=None, points=False, blocks=None):
    """the batched call against the concatenation of its one-line calls: no sentinel left, equal bits, the kernel and grid named"""
    h, geo, dP = device_case(n_lines, N)
    row = lambda t, l: None if t is None else t[l:l + 1]
    big, launch = call(ctx, h, geo, dP, t0, lam_guess=lam_guess, points=points)
    assert launch[0] == name, (tag, launch)
    if blocks is not None:
        assert launch[1] == blocks, (tag, launch, blocks)
    one = [call(ctx, h, [g[l:l + 1] for g in geo], dP[l:l + 1], t0[l:l + 1] if points else t0, lam_guess=row(lam_guess, l),
                points=points)[0] for l in range(n_lines)]
    for k in ("gam", "lam", "info"):
        want = np.concatenate([o[k] for o in one], axis=0)
        if k == "info":
            assert not (big[k] == INFO_SENTINEL).any() and not (want == INFO_SENTINEL).any(), (tag, k, big[k])
        else:
            assert not np.isnan(big[k]).any() and not np.isnan(want).any(), (tag, k, big[k])
        assert big[k].shape == want.shape and np.array_equal(bits(big[k]), bits(want)), (tag, k, big[k], want)
    return big


def grid_blocks(n_lines, nparts):
    """blocks of the 3-D launch: min(8, n_lines) columns, nparts rows, ceil(n_lines / 8) chunks (idle columns of the last chunk included)"""
    return min(8, n_lines) * nparts * ((n_lines + 7) // 8)


@pytest.mark.parametrize("n_theta0", THETA0S)
@pytest.mark.parametrize("n_lines", LINES)
def test_plain_and_warm_scan_equal_their_one_line_calls(ctx, n_lines, n_theta0):
    import torch
    N, t0 = 131, theta0_grid(n_theta0)
    name = "ibs::k_gamma_scan<double, %d>" % rows_per_lane(N)
    # (fewer waves than the device has CUs: one wave per block, so a line has n_theta0 parts and last_launch's waves are blocks)
    plain = batched_equals_lines(ctx, n_lines, N, t0, ("plain", n_lines, n_theta0), name, blocks=grid_blocks(n_lines, n_theta0))
    guess = torch.from_numpy(plain["lam"]).to(t0.device)
    batched_equals_lines(ctx, n_lines, N, t0, ("warm", n_lines, n_theta0), name, lam_guess=guess, blocks=grid_blocks(n_lines, n_theta0))


@pytest.mark.parametrize("n_lines", LINES)
def test_per_line_theta0_equals_its_one_line_calls(ctx, n_lines):
    import torch
    N = 131
    t0 = torch.from_numpy(np.linspace(0.0, 1.4, n_lines) if n_lines > 1 else np.array([0.3])).to(torch.device("cuda:0"))
    batched_equals_lines(ctx, n_lines, N, t0, ("points", n_lines), "ibs::k_gamma_scan<double, %d>" % rows_per_lane(N), points=True,
                         blocks=grid_blocks(n_lines, 1))


def test_eight_rows_per_lane(ctx):
    """N = 513 (M = 8, the bench kernel): two chunks, the second with one line, five parts"""
    batched_equals_lines(ctx, 9, 513, theta0_grid(5), ("N = 513",), "ibs::k_gamma_scan<double, 8>", blocks=grid_blocks(9, 5))


def test_chained_scan_equals_its_one_line_calls(ctx):
    """scan_chain = 2: k_gamma_scan_chain on the same map (two chunks, the second with one line); a line's chain is the same in the
    batched and in the one-line call, so the bits are"""
    try:
        ctx.set_option("scan_chain", 2)
        batched_equals_lines(ctx, 9, 131, theta0_grid(8), ("chain",), "ibs::k_gamma_scan_chain<double, 3>")
    finally:
        ctx.set_option("scan_chain", None)


@pytest.mark.parametrize("n_lines,n_surf", [(9, 3), (16, 2)])
def test_fused_maxima_are_the_first_maxima_of_the_plain_scan(ctx, n_lines, n_surf):
    """ScanPlan.scan_argmax (the arrival counters count a surface's live blocks only): gam equals the plain scan's, and the pair of
    every surface is numpy's first maximum of it"""
    import torch
    import ibs_amd
    N, t0 = 131, theta0_grid(5)
    h, geo, dP = device_case(n_lines, N)
    plain, _ = call(ctx, h, geo, dP, t0)
    plan = ibs_amd.ScanPlan(ctx, h, geo, dP, t0, n_surf)
    for rep in range(2):                                                  # (twice: the counters are reset for the next launch)
        plan.gam.fill_(float("nan")); plan.lam.fill_(float("nan")); plan.pack.fill_(float("nan")); plan.info.fill_(INFO_SENTINEL)
        plan.scan_argmax()
        torch.cuda.synchronize()
        assert ctx.last_launch() == ("ibs::k_gamma_scan<double, 3>", grid_blocks(n_lines, 5)), ctx.last_launch()
        gam, pack = plan.gam.cpu().numpy(), plan.pack.cpu().numpy()
        assert np.array_equal(bits(gam), bits(plain["gam"])) and np.array_equal(bits(plan.lam.cpu().numpy()), bits(plain["lam"])), rep
        assert np.array_equal(plan.info.cpu().numpy(), plain["info"]), rep
        tab = plain["gam"].reshape(n_surf, -1)
        assert not np.isnan(pack).any(), (rep, pack)
        assert np.array_equal(pack[:, 1], tab.argmax(axis=1).astype(np.float64)), (rep, pack, tab.argmax(axis=1))
        assert np.array_equal(bits(np.ascontiguousarray(pack[:, 0])), bits(np.ascontiguousarray(tab.max(axis=1)))), (rep, pack)
