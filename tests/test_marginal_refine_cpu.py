"""CPU: the refinement of the marginal-stability scale in (alpha, theta0) -- ibs_marginal_obj_w_grad_f64's exported name, argument
checks and kernel resources; BallooningScan.marginal(refine=True) on the oracle context (tests/marginal_points_oracle.py) against a
literal loop with scipy's L-BFGS-B on the same objective; what the refinement buys over the coarse minimum; the oracle's own
gradient against central differences of its val."""
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
from tests import marginal_points_oracle as mpo
from tests.helpers import synthetic_fieldlines

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ideal-ballooning-solver_amd", "csrc")
LIB = os.path.join(ROOT, "ideal-ballooning-solver_amd", "lib", "libibs_hip.so")
NEW = "ibs_marginal_obj_w_grad_f64"
SVALS = [0.3, 0.5, 0.7, 0.9]
NALPHA, NTHETA0, N = 6, 4, 129
DEL = 0.004


@pytest.mark.skipif(shutil.which("nm") is None, reason="needs nm")
def test_library_exports_the_entry_point():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert NEW in names and NEW in _lib.SYMBOLS


def test_null_context_and_arguments_are_refused():
    lib = _lib.lib()
    fn = getattr(lib, NEW)
    assert fn(None, 1, 513, 0.05, None, 513, None, 0.004, None, None, None, None, None, None, 0) < 0
    assert b"null" in lib.ibs_last_error()
    if lib.ibs_device_count() > 0:          # (a context needs a GPU; the argument checks come before any device work)
        h = C.c_void_p(None)
        assert lib.ibs_create(C.byref(h), 0) == 0
        try:
            buf = np.zeros(3 * 8 * 70000)
            p = lambda a: C.c_void_p(a.ctypes.data)
            val, t0 = np.zeros(1), np.zeros(1)
            for bad_N in (512, 65, 65539):       # even, below 66, above 65,537
                rc = fn(h, 1, bad_N, 0.05, p(buf), bad_N, p(t0), 0.004, p(val), None, None, None, None, None, 1)
                assert rc == -3, (bad_N, rc)     # IBS_ERR_UNSUPPORTED
            assert fn(h, 1, 513, 0.05, p(buf), 513, p(t0), 0.004, None, None, None, None, None, None, 1) == -1      # IBS_ERR_ARG
            assert b"null" in lib.ibs_last_error()
            assert fn(h, 0, 513, 0.05, p(buf), 513, p(t0), 0.004, p(val), None, None, None, None, None, 1) == 0
        finally:
            lib.ibs_destroy(h)


def _scratch_of(source):
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-c", "--cuda-device-only", "-o", os.devnull,
                        "-Rpass-analysis=kernel-resource-usage", os.path.join(CSRC, source)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    name, scratch = None, {}
    for line in r.stderr.split("\n"):
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"remark:\s+ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name:
            scratch[name] = int(m.group(1))
    return scratch


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")
def test_marginal_point_kernel_has_no_scratch():
    """k_marginal_points (csrc/ibs_marginal_points.hip) compiles for gfx950 with ScratchSize 0, and k_marginal_gcf / k_marginal_scan
    (csrc/ibs_marginal.hip) keep theirs at 0"""
    new = {k: v for k, v in _scratch_of("ibs_marginal_points.hip").items() if "k_marginal_points" in k}
    assert len(new) == 1 and all(v == 0 for v in new.values()), new
    old = {k: v for k, v in _scratch_of("ibs_marginal.hip").items() if "k_marginal_gcf" in k or "k_marginal_scan" in k}
    assert len(old) == 2 and all(v == 0 for v in old.values()), old


def scale_at(fl, h, s, a, t0):
    """the oracle's s* and its unit u on the line (s, a) at t0"""
    ln = fl(s, np.array([a]))[0]
    q = mo.solve(h, *mo.line_gc(bo.dPdrho_of(ln[2], ln[7], ln[0]), *ln[:7], t0))
    return q["scale"], q.get("u", 0.0)


def literal_rows(fl, h, svals, nalpha, ntheta0):
    """coarse table of s* -> first minimum -> scipy L-BFGS-B (upstream's bounds, tolerances and cap: ball_scan.py:307-314) on the
    oracle objective -mu -> mo.solve at the result, written out.  Rows (scale, alpha, theta0, coarse minimum, nfev, message)."""
    from scipy.optimize import minimize
    alpha_scan = np.linspace(0, np.pi, nalpha)
    theta0_scan = np.linspace(0.0, 0.5 * np.pi, ntheta0)
    rows = []
    for s in svals:
        tab = np.array([[scale_at(fl, h, s, a, t0)[0] for t0 in theta0_scan] for a in alpha_scan])
        k = int(np.argmin(tab.reshape(-1)))
        a0, t00 = alpha_scan[k // ntheta0], theta0_scan[k % ntheta0]

        def obj(x):
            a, t0 = float(x[0]), float(x[1])
            r = mpo.point(h, fl(s, np.array([a - 0.5 * DEL, a, a + 0.5 * DEL])), t0, DEL)
            return r["val"], r["jac"]

        res = minimize(obj, x0=(a0, t00), jac=True, bounds=((0.0, np.pi), (0.0, 0.5 * np.pi)),
                       options={"ftol": 5.0e-11, "gtol": 2.0e-08, "maxiter": 30})
        a, t = float(res.x[0]), float(res.x[1])
        rows.append((scale_at(fl, h, s, a, t)[0], a, t, tab.min(), res.nfev, str(res.message)))
    return rows


@pytest.fixture(scope="module")
def run():
    th = bo.theta_grid(N)
    fl = synthetic_fieldlines(th)
    ctx = mpo.MarginalPointsOracleContext()
    scan = ibs_amd.BallooningScan(ctx, fl, th, SVALS, nalpha=NALPHA, ntheta0=NTHETA0, del_alpha=DEL)
    coarse = scan.marginal()
    assert ctx.n_point_evals == 0                    # (the coarse call does not touch the point objective)
    res = scan.marginal(refine=True)
    assert ctx.n_point_evals == int(res["evals"].sum()) + len(SVALS)      # (the rounds + the one final launch)
    return th, fl, scan, coarse, res


def test_refine_false_is_the_coarse_result(run):
    """marginal() and marginal(refine=False): the same keys and bitwise the same arrays"""
    th, fl, scan, coarse, _ = run
    again = scan.marginal(refine=False)
    assert set(coarse) == set(again) == {"scale", "alpha", "theta0", "index", "table"}
    for key in coarse:
        assert np.array_equal(coarse[key], again[key]), key


def test_driver_matches_literal_loop(run):
    """BallooningScan.marginal(refine=True) at N = 129 (6 alpha x 4 theta0, four surfaces) equals the loop written out above: scale
    to 1e-8 relative, (alpha, theta0) to 1e-4 -- the bars of test_scan_driver_exact_matches_literal_loop.  Both optimisers converge
    on every surface (projected gradient or f reduction)."""
    th, fl, scan, coarse, res = run
    lit = literal_rows(fl, scan.h, SVALS, NALPHA, NTHETA0)
    for k, (sc, a, t, cmin, nfev, msg) in enumerate(lit):
        print("marginal-refine figures: s = %.1f literal scale %.12f at (%.6f, %.6f) coarse %.12f nfev %d %s | driver scale %.12f at "
              "(%.6f, %.6f) evals %d task %d" % (SVALS[k], sc, a, t, cmin, nfev, msg, res["scale"][k], res["alpha"][k],
                                                 res["theta0"][k], res["evals"][k], res["task"][k]))
        assert "PROJECTED GRADIENT" in msg or "REDUCTION OF F" in msg, msg
        assert res["task"][k] in (10, 11), res["task"]
        assert res["coarse_scale"][k] == cmin == coarse["scale"][k]
        assert abs(res["scale"][k] - sc) <= 1e-8 * sc, (k, res["scale"][k], sc)
        assert abs(res["alpha"][k] - a) < 1e-4 and abs(res["theta0"][k] - t) < 1e-4, (k, res["alpha"][k], a, res["theta0"][k], t)
    assert np.array_equal(res["index"], coarse["index"]) and np.array_equal(res["table"], coarse["table"])
    assert np.array_equal(res["start"], np.stack([coarse["alpha"], coarse["theta0"]], axis=1))
    assert res["rounds"] == res["evals"].max() and res["dscale"].shape == (len(SVALS), 2) and np.allclose(res["dPdrho"], -1.0, rtol=1e-14, atol=0)


def test_what_refinement_buys(run):
    """on every surface the refined s* lies at least 100 u below the coarse minimum (u from mo.solve at the refined point), and the
    central-difference |d s* / d alpha| of the oracle (step 1e-5) at the refined point is at most a tenth of that at the coarse start"""
    th, fl, scan, coarse, res = run
    st = 1e-5
    for k, s in enumerate(SVALS):
        sc, u = scale_at(fl, scan.h, s, res["alpha"][k], res["theta0"][k])
        slope = lambda a, t: abs(scale_at(fl, scan.h, s, a + st, t)[0] - scale_at(fl, scan.h, s, a - st, t)[0]) / (2 * st)
        d_ref, d_start = slope(res["alpha"][k], res["theta0"][k]), slope(*res["start"][k])
        print("marginal-refine figures: s = %.1f coarse - refined %.3e = %.0f u, alpha moved %.3f, |ds*/dalpha| refined %.3e start %.3e"
              % (s, res["coarse_scale"][k] - res["scale"][k], (res["coarse_scale"][k] - res["scale"][k]) / u,
                 res["alpha"][k] - res["start"][k, 0], d_ref, d_start))
        assert res["scale"][k] <= res["coarse_scale"][k] - 100 * u, (k, res["scale"][k], res["coarse_scale"][k], u)
        assert d_ref <= 0.1 * d_start, (k, d_ref, d_start)


def test_oracle_gradient_against_central_differences():
    """the restatement's jac against central differences of its own val (step 1e-5) at one interior point per surface: the theta0
    component to 1e-5 relative; the alpha component to 1e-4 relative -- it is the derivative of the del_alpha central difference of
    the rows by definition, O(del_alpha^2) from the derivative of val"""
    th = bo.theta_grid(N)
    h = th[1] - th[0]
    fl = synthetic_fieldlines(th)
    st = 1e-5
    for s, a, t0 in zip(SVALS, (0.7, 1.3, 1.9, 2.5), (0.3, 0.6, 0.9, 1.2)):
        tri = lambda al: fl(s, np.array([al - 0.5 * DEL, al, al + 0.5 * DEL]))
        r = mpo.point(h, tri(a), t0, DEL)
        fa = (mpo.point(h, tri(a + st), t0, DEL, False)["val"] - mpo.point(h, tri(a - st), t0, DEL, False)["val"]) / (2 * st)
        ft = (mpo.point(h, tri(a), t0 + st, DEL, False)["val"] - mpo.point(h, tri(a), t0 - st, DEL, False)["val"]) / (2 * st)
        print("marginal-refine figures: s = %.1f jac %s central differences (%.9e, %.9e) relative (%.1e, %.1e)"
              % (s, r["jac"], fa, ft, abs(r["jac"][0] - fa) / abs(fa), abs(r["jac"][1] - ft) / abs(ft)))
        assert abs(r["jac"][0] - fa) <= 1e-4 * abs(fa), (s, r["jac"][0], fa)
        assert abs(r["jac"][1] - ft) <= 1e-5 * abs(ft), (s, r["jac"][1], ft)
        assert np.allclose(r["jac"], r["dscale"] / r["scale"] ** 2, rtol=1e-15, atol=0) and r["val"] == -1.0 / r["scale"]
