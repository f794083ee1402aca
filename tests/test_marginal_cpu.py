"""CPU: the marginal-stability entry points check their arguments without a GPU, their oracle (tests/marginal_oracle.py) reproduces
the reference's stability table and its own derivative rows, the scan driver's marginal() plumbing, and the kernels compile for gfx950
without scratch."""
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
from tests import marginal_oracle as mo
from tests.helpers import synthetic_fieldlines

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ideal-ballooning-solver_amd", "csrc")
G = os.path.join(os.path.dirname(__file__), "golden")
IBS_ERR_ARG, IBS_ERR_UNSUPPORTED = -1, -3


def test_arguments_are_checked_before_any_device_work():
    """null context and null scale: IBS_ERR_ARG with "null" in the message; even N and N = 65: IBS_ERR_UNSUPPORTED.  The checks come
    before the context is touched, so a zeroed buffer stands for it (and for the arrays) where no GPU is present."""
    lib = _lib.lib()
    N = 513
    buf = C.create_string_buffer(1 << 16)
    p = C.cast(buf, C.c_void_p)
    gcf = lambda ctx, n, scale: lib.ibs_marginal_gcf_f64(ctx, 1, n, 0.05, p, p, n, scale, None, None, None, None, None, None, 0)
    scan = lambda ctx, n, scale: lib.ibs_marginal_scan_f64(ctx, 1, 1, n, 0.05, *([p] * 7), n, p, p, scale, None, None, None, None, 0)
    for fn in (gcf, scan):
        assert fn(None, N, p) == IBS_ERR_ARG
        assert b"null" in lib.ibs_last_error()
        assert fn(p, N, None) == IBS_ERR_ARG
        assert b"null" in lib.ibs_last_error()
        for n in (512, 65, 65538, 65539):
            assert fn(p, n, p) == IBS_ERR_UNSUPPORTED, n


def salpha_table_rows(N, extent, every=1):
    tab = np.load(os.path.join(G, "G2_salpha_stability.npz"))["table"][::every]
    th = np.linspace(-extent * np.pi, extent * np.pi, N)
    g = np.empty((len(tab), N)); c = np.empty_like(g)
    for k, row in enumerate(tab):
        g[k], c[k] = bo.salpha_gc(th, row[0], row[1], row[2])
    return th[1] - th[0], g, c, tab


@pytest.mark.parametrize("which,N,extent,every", [(4, 401, 20, 1), (3, 1601, 61, 4)])
def test_oracle_reproduces_the_reference_stability_table(which, N, extent, every):
    """G2 (bishop_ball_s-alpha.py's verdicts): (s* < 1) == unstable, all 240 rows of the 401-point column, every 4th of the 1601-point one"""
    h, g, c, tab = salpha_table_rows(N, extent, every)
    s = np.array([mo.scale_of(h, g[k], c[k]) for k in range(len(tab))])
    assert np.isfinite(s).all() and s.min() > 0.4 and s.max() < 13.0
    assert ((s < 1).astype(int) == tab[:, which].astype(int)).all()


def test_oracle_derivative_rows_against_central_differences():
    """d s* / d g_j and d s* / d c_j by the Hellmann-Feynman formula against central differences of the oracle, every entry of an s-alpha
    line at N = 129: step 1e-4, 1e-6 relative to the largest entry of the row (the step-squared truncation)"""
    N, step = 129, 1e-4
    th = bo.theta_grid(N)
    h = th[1] - th[0]
    g, c = bo.salpha_gc(th, 1.0, 0.8, 0.3)
    gb, cb = mo.grad_rows(h, mo.solve(h, g, c))
    fg, fc = np.zeros(N), np.zeros(N)
    for j in range(N):
        d = np.zeros(N); d[j] = step
        fg[j] = (mo.scale_of(h, g + d, c) - mo.scale_of(h, g - d, c)) / (2 * step)
        fc[j] = (mo.scale_of(h, g, c + d) - mo.scale_of(h, g, c - d)) / (2 * step)
    assert np.abs(fg - gb).max() <= 1e-6 * np.abs(gb).max(), (np.abs(fg - gb).max(), np.abs(gb).max())
    assert np.abs(fc - cb).max() <= 1e-6 * np.abs(cb).max(), (np.abs(fc - cb).max(), np.abs(cb).max())
    assert gb[0] > 0 and cb[0] == 0 and cb[-1] == 0          # the end rows: one half cell of g, no c


def test_oracle_theta0_derivative_against_central_difference():
    """the contraction with the theta0 tangent (utils.py:1669-1673) and d s* / d dPdrho = -s* / dPdrho"""
    N = 129
    th = bo.theta_grid(N)
    h = th[1] - th[0]
    geo = synthetic_fieldlines(th)(0.6, [0.7])
    geo7 = [geo[:, k] for k in range(7)]
    dP, t0, step = np.array([-1.0]), 0.3, 1e-5
    r = mo.scan(h, geo7, dP, np.array([t0 - step, t0, t0 + step]), want_grad=True)
    fd = (r["scale"][0, 2] - r["scale"][0, 0]) / (2 * step)
    assert abs(fd - r["dscale_dtheta0"][0, 1]) < 1e-7 * max(1.0, abs(fd))
    rp = mo.scan(h, geo7, dP * (1 + 1e-6), np.array([t0]))["scale"][0, 0]
    rm = mo.scan(h, geo7, dP * (1 - 1e-6), np.array([t0]))["scale"][0, 0]
    assert abs((rp - rm) / (2e-6 * dP[0]) - r["dscale_ddPdrho"][0, 1]) < 1e-7 * abs(r["dscale_ddPdrho"][0, 1])


def test_scan_driver_marginal_against_a_direct_loop():
    """BallooningScan.marginal() through the stand-in context: N = 129, 2 surfaces, a 6 x 4 coarse grid"""
    N = 129
    th = bo.theta_grid(N)
    fl = synthetic_fieldlines(th)
    rho = [0.5, 0.8]
    scan = ibs_amd.BallooningScan(mo.MarginalOracleContext(), fl, th, rho, nalpha=6, ntheta0=4)
    m = scan.marginal()
    assert m["table"].shape == (2, 6, 4) and m["scale"].shape == (2,) and m["index"].shape == (2, 2)
    for k, s in enumerate(rho):
        geo = fl(s, scan.alpha_scan)
        best = (np.inf, -1, -1)
        for ia in range(6):
            dP = bo.dPdrho_of(geo[ia, 2], geo[ia, 7], geo[ia, 0])
            for it, t0 in enumerate(scan.theta0_scan):
                g, c = mo.line_gc(dP, *geo[ia, :7], t0)
                r = mo.solve(scan.h, g, c)
                v = r["scale"]
                assert abs(v - m["table"][k, ia, it]) <= 0.1 * r["u"]      # (LAPACK's own noise in lam_max is ~ u / N)
                if v < best[0]:
                    best = (v, ia, it)
        assert m["scale"][k] == m["table"][k, best[1], best[2]]
        assert tuple(m["index"][k]) == best[1:]
        assert m["alpha"][k] == scan.alpha_scan[best[1]] and m["theta0"][k] == scan.theta0_scan[best[2]]


def test_marginal_dPdrho_refuses_a_non_uniform_grid():
    th = bo.theta_grid(129).copy()
    th[5] += 1e-3
    one = np.ones(129)
    with pytest.raises(ValueError):
        ibs_amd.marginal_dPdrho(-1.0, th, one, one, one, one, ctx=mo.MarginalOracleContext())


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")
def test_marginal_kernels_have_no_scratch():
    """k_marginal_gcf and k_marginal_scan (csrc/ibs_marginal.hip) compile for gfx950 with ScratchSize 0"""
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-c", "--cuda-device-only", "-o", os.devnull,
                        "-Rpass-analysis=kernel-resource-usage", os.path.join(CSRC, "ibs_marginal.hip")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    name, scratch = None, {}
    for line in r.stderr.split("\n"):
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"remark:\s+ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name:
            scratch[name] = int(m.group(1))
    kern = {k: v for k, v in scratch.items() if "k_marginal" in k}
    assert len(kern) == 2 and all(v == 0 for v in kern.values()), scratch
