"""CPU: the rule for a ray of the local-equilibrium boundaries (ibs_amd.operators.local_eq_ray_triples), the declaration and the argument
rules of ibs_local_eq_boundary_f64 without a GPU, the resources of k_local_eq_boundary and the driver's precondition."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import ibs_amd
from ibs_amd import _lib, local_eq_ray_nodes, local_eq_ray_triples

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(os.path.dirname(__file__), "golden")
IBS_ERR_ARG, IBS_ERR_UNSUPPORTED = -1, -3
NAME = "ibs_local_eq_boundary_f64"


def test_ray_triples_against_hand_written_triples():
    """a p-ray, an eps-ray and an oblique ray at hand-written parameters; the end points; broadcasting of (n_ray, 7) against (n_ray, K)"""
    rays = np.array([(0.25, -0.5, 0.0, 0.0, 1.0, 0.2, 3.0),         # pressure axis at eps = -0.5: p = t
                     (0.0, 0.0, 1.6, 1.0, 0.0, -0.9, 1.0),          # shear axis at p = 1.6: eps = t
                     (0.1, -0.5, 0.25, 0.5, 2.0, 0.0, 2.0)])        # oblique
    assert local_eq_ray_triples(rays[0], 1.5).tolist() == [0.25, -0.5, 1.5]
    assert local_eq_ray_triples(rays[1], -0.25).tolist() == [0.0, -0.25, 1.6]
    assert local_eq_ray_triples(rays[2], 1.5).tolist() == [0.1, 0.25, 3.25]
    ends = local_eq_ray_triples(rays[:, None, :], rays[:, 5:7])
    assert ends.shape == (3, 2, 3)
    assert ends.tolist() == [[[0.25, -0.5, 0.2], [0.25, -0.5, 3.0]], [[0.0, -0.9, 1.6], [0.0, 1.0, 1.6]], [[0.1, -0.5, 0.25], [0.1, 0.5, 4.25]]]
    t = np.array([[0.5, 1.0], [0.0, 0.5], [1.0, 2.0]])
    tri = local_eq_ray_triples(rays[:, None, :], t)
    assert tri.shape == (3, 2, 3) and (tri[:, :, 0] == rays[:, :1]).all()      # theta0 does not vary along a ray
    assert tri[2].tolist() == [[0.1, 0.0, 2.25], [0.1, 0.5, 4.25]]


def test_ray_nodes():
    """64 nodes per ray, the first t_lo, the last t_hi itself, equidistant within rounding, increasing"""
    rays = np.array([(0.0, 0.0, 0.0, 0.0, 1.0, 0.2, 3.0), (0.0, 0.0, 1.6, 1.0, 0.0, -0.9, 1.0)])
    t = local_eq_ray_nodes(rays)
    assert t.shape == (2, 64) and (t[:, 0] == rays[:, 5]).all() and (t[:, 63] == rays[:, 6]).all() and (np.diff(t, axis=1) > 0).all()
    assert np.abs(t - (rays[:, 5:6] + np.arange(64) * (rays[:, 6:7] - rays[:, 5:6]) / 63)).max() <= 4 * np.finfo(float).eps * 3.0


def test_first_unstable_reduction():
    """the envelope of BallooningScan.local_eq_boundary on a hand-written table: one surface, 2 alpha x 1 theta0 x 3 fixed x 2 crossings"""
    nan = np.nan
    ts = np.array([[[[[1.0, 2.5], [nan, nan], [2.0, nan]]], [[[0.5, nan], [nan, nan], [1.5, nan]]]]])
    tu = np.array([[[[[1.5, 2.0], [nan, nan], [1.0, nan]]], [[[1.0, nan], [nan, nan], [1.0, nan]]]]])
    lo = np.array([[[[0, 0, 1]], [[0, 0, 1]]]])
    assert ts.shape == (1, 2, 1, 3, 2)
    # fixed 0: crossings up at 1.25 and at 0.75 (and one down at 2.25): 0.75; fixed 1: none; fixed 2: unstable at t_lo = 0.2
    assert ibs_amd.first_unstable(ts, tu, lo, 0.2).tolist() == [[0.75, np.inf, 0.2]]


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")
def test_kernel_has_no_scratch():
    """k_local_eq_boundary (csrc/ibs_local_eq_boundary.hip) compiles for gfx950 with ScratchSize 0 and at most 20 KB of LDS: seven
    coefficients x 360 grid points x 8 bytes"""
    src = os.path.join(ROOT, "ideal-ballooning-solver_amd", "csrc", "ibs_local_eq_boundary.hip")
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-c", "--cuda-device-only", "-o", os.devnull,
                        "-Rpass-analysis=kernel-resource-usage", src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert len(re.findall(r"Function Name: \S*k_local_eq_boundary", r.stderr)) == 1
    assert re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr) == ["0"]
    lds = [int(v) for v in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stderr)]
    assert lds == [7 * 360 * 8] and lds[0] <= 20 * 1024


def test_arguments_are_checked_before_any_device_work():
    """the name is declared in include/ibs.h and exported; a NULL required argument, ld < N, ps_ld < N, n_ray < 1, max_cross outside
    [1, 4], xtol outside [0, 1) or NaN, a non-finite shift: IBS_ERR_ARG; N = 512, 65, 65,539: IBS_ERR_UNSUPPORTED.  The checks come before
    the context is touched, so a zeroed buffer stands for it and for the arrays."""
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ibs.h")).read(), flags=re.S)
    assert "int %s(" % NAME in hdr and NAME in _lib.SYMBOLS
    lib = _lib.lib()
    fn = getattr(lib, NAME)
    buf = C.create_string_buffer(1 << 16)
    P = C.cast(buf, C.c_void_p)
    N = 513

    def call(ctx=P, n=N, ld=None, geo=P, dP=P, centre=P, sigma=P, ps=None, ps_ld=None, rays=P, shift=0.0, max_cross=4, xtol=1e-12, ts=P,
             tu=P, nc=P, n_ray=1, flags=0):
        return fn(ctx, 1, n_ray, n, -1.0, 0.05, geo, n if ld is None else ld, dP, centre, sigma, ps, n if ps_ld is None else ps_ld, rays,
                  shift, max_cross, xtol, ts, tu, nc, None, None, None, flags)

    for kw in (dict(ctx=None), dict(geo=None), dict(dP=None), dict(centre=None), dict(sigma=None), dict(rays=None), dict(ts=None),
               dict(tu=None), dict(nc=None)):
        assert call(**kw) == IBS_ERR_ARG, kw
        assert b"null" in lib.ibs_last_error()
    assert call(ld=N - 1) == IBS_ERR_ARG
    assert call(ps=P, ps_ld=N - 1) == IBS_ERR_ARG
    assert call(n_ray=0) == IBS_ERR_ARG
    for mc in (0, 5, -1):
        assert call(max_cross=mc) == IBS_ERR_ARG, mc
    for xtol in (-1e-3, 1.0, 2.0, float("nan"), float("inf")):
        assert call(xtol=xtol) == IBS_ERR_ARG, xtol
    for shift in (float("nan"), float("inf"), -float("inf")):
        assert call(shift=shift) == IBS_ERR_ARG, shift
    assert call(flags=2) == IBS_ERR_ARG
    for n in (512, 65, 65539):
        assert call(n=n) == IBS_ERR_UNSUPPORTED, n


def test_driver_needs_the_resident_path():
    """BallooningScan.local_eq_boundary without tables= and device=: ValueError, before any device work (the context is never used);
    an unknown axis is a ValueError as well"""
    th = np.linspace(-4 * np.pi, 4 * np.pi, 513)
    svals = np.array([0.6, 0.9])
    scan = ibs_amd.BallooningScan(None, None, th, svals, nalpha=3, ntheta0=2)
    with pytest.raises(ValueError):
        scan.local_eq_boundary([0.0], (0.2, 3.0))
    tabs = ibs_amd.SurfaceTables.from_wout(dict(np.load(os.path.join(G, "G8_wout_ncsx_op.npz"))), svals)
    with pytest.raises(ValueError):
        ibs_amd.BallooningScan(None, None, th, svals, nalpha=3, ntheta0=2, tables=tabs).local_eq_boundary([0.0], (0.2, 3.0))
    with pytest.raises(ValueError):
        ibs_amd.BallooningScan(None, None, th, svals, nalpha=3, ntheta0=2, tables=tabs, device="cuda:0").local_eq_boundary(
            [0.0], (0.2, 3.0), axis="q")
