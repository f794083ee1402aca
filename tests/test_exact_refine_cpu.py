"""CPU: the scan drivers' jac="exact" mode and its batched entry point ibs_obj_w_grad_exact_f64 -- exported name, argument checks,
the kernel's resources, the driver's plumbing against a literal loop on the same oracle objective, and what the exact gradient buys
over the reference's Hellmann-Feynman one (a refined point that is a maximum of gam)."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import ibs_amd
from ibs_amd import _lib
from oracle import ballooning_oracle as bo
from tests.exact_oracle import ExactOracleContext, obj_w_grad_exact_lines
from tests.helpers import synthetic_fieldlines

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ideal-ballooning-solver_amd", "csrc")
LIB = os.path.join(ROOT, "ideal-ballooning-solver_amd", "lib", "libibs_hip.so")
NEW = "ibs_obj_w_grad_exact_f64"
SVALS = [0.3, 0.5, 0.7, 0.9]
NALPHA, NTHETA0, N = 6, 4, 129


def _refused(lib, h, N=513):
    return lib.ibs_obj_w_grad_exact_f64(h, 1, N, 0.05, None, N, None, None, 0.004, None, None, None, None, None, None, 0)


def test_null_context_and_arguments_are_refused():
    lib = _lib.lib()
    assert _refused(lib, None) < 0
    assert b"null" in lib.ibs_last_error()
    if lib.ibs_device_count() > 0:          # (a context needs a GPU; the argument checks come before any device work)
        import ctypes as C
        h = C.c_void_p(None)
        assert lib.ibs_create(C.byref(h), 0) == 0
        try:
            assert _refused(lib, h) < 0
            assert b"bad arguments" in lib.ibs_last_error()
            buf = np.zeros(3 * 8 * 70000)
            p = lambda a: C.c_void_p(a.ctypes.data)
            val, jac, t0 = np.zeros(1), np.zeros(2), np.zeros(1)
            for bad_N in (512, 65, 65539):       # even, below 66, above 65,537
                rc = lib.ibs_obj_w_grad_exact_f64(h, 1, bad_N, 0.05, p(buf), bad_N, p(t0), None, 0.004, p(val), p(jac), None, None,
                                                  None, None, 1)
                assert rc == -3, (bad_N, rc)     # IBS_ERR_UNSUPPORTED
        finally:
            lib.ibs_destroy(h)


@pytest.mark.skipif(shutil.which("nm") is None, reason="needs nm")
def test_library_exports_the_entry_point():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert NEW in names and NEW in _lib.SYMBOLS


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")
def test_exact_point_kernels_have_no_scratch():
    """k_exact_points<NEAREST> (csrc/ibs_exact_grad.hip): both instantiations compile for gfx950 with ScratchSize 0"""
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-c", "--cuda-device-only", "-o", os.devnull,
                        "-Rpass-analysis=kernel-resource-usage", os.path.join(CSRC, "ibs_exact_grad.hip")],
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
    kern = {k: v for k, v in scratch.items() if "k_exact_points" in k}
    assert len(kern) == 2 and all(v == 0 for v in kern.values()), scratch


def gam_at(fl, th, s, a, t0):
    """the final solve of ball_scan.py:322-339 at one point, on the oracle"""
    ln = fl(s, np.array([a]))[0]
    dP = bo.dPdrho_of(ln[2], ln[7], ln[0])
    cv, gd = bo.fold_theta0(t0, ln[2], ln[3], ln[4], ln[5], ln[6])
    return bo.gamma_ball_full(dP, th, ln[0], ln[1], cv, gd)[0]


def literal_exact_rows(fl, th, svals, nalpha, ntheta0, del_alpha=0.004):
    """coarse table -> first maximum -> scipy L-BFGS-B (upstream's bounds, tolerances and cap) on the oracle objective with the exact
    gradient -> final solve, written out"""
    from scipy.optimize import minimize
    alpha_scan = np.linspace(0, np.pi, nalpha)
    theta0_scan = np.linspace(0.0, 0.5 * np.pi, ntheta0)
    rows = []
    for s in svals:
        tab = np.array([[gam_at(fl, th, s, a, t0) for t0 in theta0_scan] for a in alpha_scan])
        m = tab.max()
        if m == 0.0:
            a0, t00 = 0.0, 0.0
        else:
            i, j = (int(k[0]) for k in np.where(tab == m))
            a0, t00 = alpha_scan[i], theta0_scan[j]

        def obj(x):
            a, t0 = float(x[0]), float(x[1])
            val, jac, _ = obj_w_grad_exact_lines(th, t0, fl(s, np.array([a - 0.5 * del_alpha, a, a + 0.5 * del_alpha])), None, del_alpha)
            return val, jac

        res = minimize(obj, x0=(a0, t00), jac=True, bounds=((0.0, np.pi), (0.0, 0.5 * np.pi)),
                       options={"ftol": 5.0e-11, "gtol": 2.0e-08, "maxiter": 30})
        a, t = float(res.x[0]), float(res.x[1])
        rows.append((t, a, gam_at(fl, th, s, a, t)))
    return np.array(rows)


@pytest.fixture(scope="module")
def runs():
    th = bo.theta_grid(N)
    fl = synthetic_fieldlines(th)
    ctx = ExactOracleContext()
    exact = ibs_amd.BallooningScan(ctx, fl, th, SVALS, nalpha=NALPHA, ntheta0=NTHETA0, jac="exact").run()
    assert ctx.n_exact_evals > 0                     # (the refinement went through obj_w_grad_exact)
    n = ctx.n_exact_evals
    ref = ibs_amd.BallooningScan(ctx, fl, th, SVALS, nalpha=NALPHA, ntheta0=NTHETA0, jac="reference").run()
    assert ctx.n_exact_evals == n                    # (... and the reference mode does not)
    return th, fl, exact, ref


def test_scan_driver_exact_matches_literal_loop(runs):
    """BallooningScan(jac="exact").run() at N = 129 (6 alpha x 4 theta0, four surfaces) equals the loop written out above: gam to
    1e-8, (alpha, theta0) to 1e-4"""
    th, fl, (t0, al, gam), _ = runs
    lit = literal_exact_rows(fl, th, SVALS, NALPHA, NTHETA0)
    assert np.abs(gam - lit[:, 2]).max() < 1e-8, (gam, lit[:, 2])
    assert np.abs(al - lit[:, 1]).max() < 1e-4 and np.abs(t0 - lit[:, 0]).max() < 1e-4, (al, t0, lit)


def test_exact_refinement_ends_on_a_maximum_of_gam(runs):
    """against jac="reference" of the same driver: gam_exact >= gam_reference - 1e-12 on every surface, and the central-difference
    |dgam/dalpha| of the final solve (step 1e-5) at the exact-refined point is at most a tenth of that at the reference-refined one"""
    th, fl, (t0e, ale, game), (t0r, alr, gamr) = runs
    print("gam_exact - gam_reference:", game - gamr)
    assert np.all(game >= gamr - 1e-12), game - gamr
    st = 1e-5
    for k, s in enumerate(SVALS):
        de = abs(gam_at(fl, th, s, ale[k] + st, t0e[k]) - gam_at(fl, th, s, ale[k] - st, t0e[k])) / (2 * st)
        dr = abs(gam_at(fl, th, s, alr[k] + st, t0r[k]) - gam_at(fl, th, s, alr[k] - st, t0r[k])) / (2 * st)
        print("s = %.1f: |dgam/dalpha| exact %.3e reference %.3e ratio 1/%.0f" % (s, de, dr, dr / max(de, 1e-300)))
        assert de <= 0.1 * dr, (s, de, dr)


def test_unknown_jac_is_refused():
    th = bo.theta_grid(129)
    with pytest.raises(ValueError):
        ibs_amd.BallooningScan(ExactOracleContext(), synthetic_fieldlines(th), th, [0.5], jac="bogus")
    with pytest.raises(ValueError):
        ibs_amd.AdjointStep(None, th, [0.5], "cpu", jac="hf")
    step = ibs_amd.AdjointStep(None, th, [0.5], "cpu", jac="exact")
    assert step.jac == "exact" and ibs_amd.AdjointStep(None, th, [0.5], "cpu").jac == "reference"
