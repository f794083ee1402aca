"""CPU: the scan driver's eigenpair="nearest" workflow and its two batched entry points (ibs_obj_w_grad_nearest_f64,
ibs_gamma_points_nearest_f64) -- argument checks, exported names, the kernel's resources, and the driver's plumbing against a
literal restatement of ball_scan.py:248-339 with upstream's dense ARPACK solve."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import ibs_amd
from ibs_amd import _lib
from oracle import ballooning_oracle as bo
from tests.helpers import synthetic_fieldlines
from tests.nearest_oracle import NearestOracleContext

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ideal-ballooning-solver_amd", "csrc")
LIB = os.path.join(ROOT, "ideal-ballooning-solver_amd", "lib", "libibs_hip.so")
NEW = ("ibs_obj_w_grad_nearest_f64", "ibs_gamma_points_nearest_f64")


def _refused(lib, h):
    N = 513
    assert lib.ibs_obj_w_grad_nearest_f64(h, 1, N, 0.05, None, N, None, None, 0.004, None, None, None, None, None, 0) < 0
    assert lib.ibs_gamma_points_nearest_f64(h, 1, N, 0.05, *([None] * 7), N, None, None, None, None, None, None, None, None,
                                            None, 0) < 0


def test_null_context_and_arguments_are_refused():
    lib = _lib.lib()
    _refused(lib, None)
    assert b"null" in lib.ibs_last_error()
    if lib.ibs_device_count() > 0:          # (a context needs a GPU; the argument checks come before any device work)
        import ctypes as C
        h = C.c_void_p(None)
        assert lib.ibs_create(C.byref(h), 0) == 0
        try:
            _refused(lib, h)
            assert b"bad arguments" in lib.ibs_last_error()
        finally:
            lib.ibs_destroy(h)


@pytest.mark.skipif(shutil.which("nm") is None, reason="needs nm")
def test_library_exports_both_entry_points():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for n in NEW:
        assert n in names and n in _lib.SYMBOLS


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")
def test_point_kernels_have_no_scratch():
    """k_nearest_points<GRAD> (csrc/ibs_nearest_grad.hip): both instantiations compile for gfx950 with ScratchSize 0"""
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-c", "--cuda-device-only", "-o", os.devnull,
                        "-Rpass-analysis=kernel-resource-usage", os.path.join(CSRC, "ibs_nearest_grad.hip")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    name, scratch = None, {}
    for line in r.stderr.split("\n"):
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"remark:\s+ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name:
            scratch[name] = int(m.group(1))
    kern = {k: v for k, v in scratch.items() if "k_nearest_points" in k}
    assert len(kern) == 2 and all(v == 0 for v in kern.values()), scratch


K_DRIVE = 8.0          # dPdrho = -8 on every line: lam_max above the coarse shift 1.0 on some lines


def driven_fieldlines(th):
    base = synthetic_fieldlines(th)

    def fieldlines(s, alphas):
        out = base(s, alphas).copy()
        out[:, 7] = out[:, 2] - 2.0 * K_DRIVE / out[:, 0] ** 2
        return out
    return fieldlines


def upstream_rows(fl, th, svals, nalpha, ntheta0, del_alpha=0.004):
    """ball_scan.py:248-339 written out literally, every solve upstream's dense matrix + ARPACK shift-invert
    (bo.gamma_ball_full_dense_arpack): coarse table at sigma = 1.0, first maximum, L-BFGS-B at 1.3 |gam| + 0.05, final at 0.42"""
    from scipy.optimize import minimize
    alpha_scan = np.linspace(0, np.pi, nalpha)
    theta0_scan = np.linspace(0.0, 0.5 * np.pi, ntheta0)

    def solve(line, t0, sigma0):
        bmag, gradpar, cvdrift, cvdrift0, gds2, gds21, gds22, gbdrift = line
        dP = bo.dPdrho_of(cvdrift, gbdrift, bmag)
        cv, gd = bo.fold_theta0(t0, cvdrift, cvdrift0, gds2, gds21, gds22)
        return dP, bo.gamma_ball_full_dense_arpack(dP, th, bmag, gradpar, cv, gd, sigma0=sigma0)

    rows = []
    for s in svals:
        lines = fl(s, alpha_scan)
        tab = np.array([[solve(lines[i], t0, 1.0)[1][0] for t0 in theta0_scan] for i in range(nalpha)])
        m = tab.max()
        if m == 0.0:
            a0, t00, sigma0 = 0.0, 0.0, 0.05
        else:
            i, j = (int(k[0]) for k in np.where(tab == m))
            a0, t00, sigma0 = alpha_scan[i], theta0_scan[j], 1.3 * abs(tab[i, j]) + 0.05

        def obj(x):
            a, t0 = float(x[0]), float(x[1])
            ll, lc, lr = fl(s, np.array([a - 0.5 * del_alpha, a, a + 0.5 * del_alpha]))
            dP, (gam, X, dX, g, c, f) = solve(lc, t0, sigma0)
            bmag, gradpar, _, cvdrift0, _, gds21, gds22, _ = lc
            gp = np.abs(gradpar)
            dgd = 2 * gds21 + 2 * t0 * gds22
            jt = bo.hf_derivative(gam, X, dX, f, gp * dgd / bmag, -1 * dP * cvdrift0 * 1 / (gp * bmag), dgd / bmag ** 2 * 1 / (gp * bmag))
            side = []
            for ln in (lr, ll):
                dPs = bo.dPdrho_of(ln[2], ln[7], ln[0])
                cv, gd = bo.fold_theta0(t0, ln[2], ln[3], ln[4], ln[5], ln[6])
                side.append(bo.gcf(dPs, ln[0], ln[1], cv, gd))
            (g_r, c_r, f_r), (g_l, c_l, f_l) = side
            ja = bo.hf_derivative(gam, X, dX, f, (g_r - g_l) / del_alpha, (c_r - c_l) / del_alpha, (f_r - f_l) / del_alpha)
            return -1 * gam, np.array([-1 * ja, -1 * jt])

        res = minimize(obj, x0=(a0, t00), jac=True, bounds=((0.0, np.pi), (0.0, 0.5 * np.pi)),
                       options={"ftol": 5.0e-11, "gtol": 2.0e-08, "maxiter": 30})
        a, t = float(res.x[0]), float(res.x[1])
        gam = solve(fl(s, np.array([a]))[0], t, 0.42)[1][0]
        rows.append((t, a, gam))
    return np.array(rows)


def test_scan_driver_nearest_matches_upstream_loop():
    """BallooningScan(eigenpair="nearest").run() on strongly driven synthetic lines (N = 129, 4 alpha x 3 theta0, two surfaces)
    equals ball_scan.py:248-339 restated with dense ARPACK: gam to 1e-8, (alpha, theta0) to 1e-4; "max" mode differs"""
    N = 129
    th = bo.theta_grid(N)
    fl = driven_fieldlines(th)
    svals = [0.5, 0.9]
    ctx = NearestOracleContext()
    scan = ibs_amd.BallooningScan(ctx, fl, th, svals, nalpha=4, ntheta0=3, eigenpair="nearest")
    assert scan.coarse().shape == (2, 4, 3)
    assert (ctx.lam_max > 1.0).any()                 # (the coarse shift lies inside the spectrum on some lines)
    t0, al, gam = scan.run(refine=True)
    ref = upstream_rows(fl, th, svals, 4, 3)
    assert np.abs(gam - ref[:, 2]).max() < 1e-8, (gam, ref[:, 2])
    assert np.abs(al - ref[:, 1]).max() < 1e-4 and np.abs(t0 - ref[:, 0]).max() < 1e-4, (al, t0, ref)
    mx = ibs_amd.BallooningScan(ctx, fl, th, svals, nalpha=4, ntheta0=3).run(refine=True)
    assert np.abs(mx[2] - gam).max() > 1e-3, (mx[2], gam)


def test_unknown_eigenpair_is_refused():
    th = bo.theta_grid(129)
    with pytest.raises(ValueError):
        ibs_amd.BallooningScan(NearestOracleContext(), synthetic_fieldlines(th), th, [0.5], eigenpair="bogus")
    with pytest.raises(ValueError):
        ibs_amd.AdjointStep(None, th, [0.5], "cpu", eigenpair="lam_max")
