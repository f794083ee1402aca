"""CPU: the rule of the local-equilibrium boundaries minimised over theta0 (csrc/ibs_local_eq_boundary_polish.hpp; ibs_amd.local_eq_first_up
and ibs_amd.polish_first_up) on the C oracle's verdicts, the declaration and the argument rules of ibs_local_eq_boundary_polish_f64
without a GPU, the resources of k_local_eq_boundary_polish and the driver's precondition."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import ibs_amd
from ibs_amd import _lib
from ibs_amd import scan as sc
from oracle import ballooning_oracle as bo
from tests import local_eq_boundary_cases as bc
from tests import local_eq_boundary_polish_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(os.path.dirname(__file__), "golden")
IBS_ERR_ARG, IBS_ERR_UNSUPPORTED = -1, -3
NAME = "ibs_local_eq_boundary_polish_f64"
BIT10, BIT11, BIT12 = 1 << 10, 1 << 11, 1 << 12


def test_first_up_on_a_hand_written_table():
    """T per ray, no reduction: a crossing up; a crossing down first on a ray that is unstable at t_lo; a crossing down first and one up
    behind it on a ray reported stable at t_lo (the smallest crossing up); none; unstable at t_lo without a crossing; an invalid ray"""
    nan = np.nan
    ts = np.array([[1.0, 2.5], [2.5, nan], [2.5, 2.75], [nan, nan], [nan, nan], [nan, nan]])
    tu = np.array([[1.5, 2.0], [2.0, nan], [2.0, 3.25], [nan, nan], [nan, nan], [nan, nan]])
    lo = np.array([0, 1, 0, 0, 1, -1])
    T = ibs_amd.local_eq_first_up(ts, tu, lo, 0.2)
    assert T.shape == (6,) and T[:5].tolist() == [1.25, 0.2, 3.0, np.inf, 0.2] and np.isnan(T[5])
    # the reduction of first_unstable over (alpha, theta0, crossing) is the minimum of T over (alpha, theta0)
    ts5, tu5, lo4 = ts[:5].reshape(1, 5, 1, 1, 2), tu[:5].reshape(1, 5, 1, 1, 2), np.zeros((1, 5, 1, 1), dtype=int)
    assert ibs_amd.first_unstable(ts5, tu5, lo4, 0.2)[0, 0] == ibs_amd.local_eq_first_up(ts5, tu5, lo4, 0.2).min()
    # a per-ray t_lo broadcasts
    assert ibs_amd.local_eq_first_up(ts[:2], tu[:2], lo[:2], np.array([0.2, 0.3])).tolist() == [1.25, 0.3]


def test_rule_on_the_oracle_finds_the_interior_minimum():
    """the rule on the CPU: polish_theta0 driven by f = -T with T from the C oracle's count (64 nodes, then bisection to 1e-10 of the
    range) on the three s-alpha base lines x the p-ray families at shat = 0.3, 0.9, 1.9, N = 129, theta0 nodes (-0.5, -0.2, 0.1, 0.4).
    The inputs' own property is asserted first: the best node of every row is an interior node with two finite neighbours, so the
    bracket is two-sided.  Then every result lies strictly inside its bracket and strictly below the best node, without bit 11, by more
    than 100 x the bisection's tolerance (2.8e-8; the smallest gain seen is 9.9e-5); and the three base lines agree at each shat (the envelope does not depend on the centre) within the bisection's
    tolerance and the search's: curvature x (2 xtol_theta0)^2 + 2 x 1e-10 x range, the curvature of each shat from its rows' second
    differences (the largest of the three lines)."""
    N, xt = 129, 1e-5
    b = bc.salpha_lines(bo.theta_grid(N))
    env, curvs = np.empty((3, 3)), np.empty((3, 3))
    for i in range(3):
        for q, k in enumerate(pc.P_ROWS):
            fam = pc.FAMILIES[k]
            row = np.array([pc.oracle_first_up(b, i, fam, u) for u in pc.THETA0])
            j = int(np.argmin(row))
            assert np.isfinite(row).all() and j in (1, 2) and (row > fam[5]).all(), (i, k, row)
            nodes, n_found = sc.row_peaks(-row[None, :], 1)
            assert nodes[0, 0] == j and n_found[0] == 1
            r = sc.polish_theta0(lambda u: -pc.oracle_first_up(b, i, fam, u), pc.THETA0, -row, j, xtol=xt, max_eval=32)
            t = -r["gam"]
            curv = (row[j - 1] - 2 * row[j] + row[j + 1]) / 0.09
            print("line %d shat %.1f: row %s -> theta0* %.6f T* %.6f (gain %.2e, %d evaluations, status %#x, curvature %.2f)"
                  % (i, fam[1] + 1, np.round(row, 4).tolist(), r["theta0"], t, row[j] - t, r["n_eval"], r["status"], curv))
            assert pc.THETA0[j - 1] < r["theta0"] < pc.THETA0[j + 1] and r["theta0"] != pc.THETA0[j], (i, k, r)
            assert t < row[j] - 100 * 1e-10 * 2.8 and not r["status"] & (BIT10 | BIT11 | BIT12 | 3), (i, k, r)
            assert curv > 0.0, (i, k, curv)
            env[i, q], curvs[i, q] = t, curv
    spread = env.max(axis=0) - env.min(axis=0)
    print("envelope of the three base lines per shat: %s, spread %s" % (env[0].tolist(), spread.tolist()))
    assert (spread <= curvs.max(axis=0) * (2 * xt) ** 2 + 2 * 1e-10 * 2.8).all(), (spread, curvs)


def test_early_return_and_a_row_of_inf():
    """a node with T = t_lo: returned at once, nothing is evaluated, bit 10; a row of +inf: row_peaks of the row of -inf finds ONE peak
    (node 0), the one-sided search runs its max_eval evaluations on -inf values and the node is returned with T = +inf after one more
    evaluation at the node -- nothing beyond the rule; a failed evaluation (status bit 1) counts as -inf and gives NaN outputs"""
    calls = []

    def never(u):
        calls.append(u)
        raise AssertionError("evaluated")

    r = sc.polish_first_up(never, pc.THETA0, [1.2, 0.2, 1.1, 1.3], 1, 0.2)
    assert not calls and r["theta0"] == -0.2 and r["t"] == 0.2 and r["n_eval"] == 0 and r["status"] == BIT10 and r["lo_unstable"] == 1
    assert np.isnan(r["t_stable"]) and np.isnan(r["t_unstable"])

    def stable(u):
        calls.append(u)
        return np.nan, np.nan, 0, 0

    row = np.full(4, np.inf)
    nodes, n_found = sc.row_peaks(-row[None, :], 2)
    assert n_found.tolist() == [1] and nodes.tolist() == [[0, 0]]
    r = sc.polish_first_up(stable, pc.THETA0, row, 0, 0.2, max_eval=5)
    assert r["n_eval"] == 5 and len(calls) == 6 and calls[-1] == -0.5 and r["points"] == calls[:5]
    assert r["t"] == np.inf and r["theta0"] == -0.5 and r["status"] == BIT10 | BIT11 | BIT12 and r["lo_unstable"] == 0
    r = sc.polish_first_up(lambda u: (np.nan, np.nan, -1, 2), pc.THETA0, [1.2, 1.0, 1.1, 1.3], 1, 0.2, max_eval=4)
    assert r["status"] & 2 and r["status"] & BIT10 and r["lo_unstable"] == -1
    assert all(np.isnan(r[k]) for k in ("theta0", "t", "t_stable", "t_unstable"))


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")
def test_kernel_has_no_scratch():
    """k_local_eq_boundary_polish (csrc/ibs_local_eq_boundary_polish.hip) compiles for gfx950 with ScratchSize 0 and at most 20 KB of
    LDS (seven coefficients x 360 grid points x 8 bytes), at the two waves per SIMD of k_local_eq_boundary"""
    src = os.path.join(ROOT, "ideal-ballooning-solver_amd", "csrc", "ibs_local_eq_boundary_polish.hip")
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-c", "--cuda-device-only", "-o", os.devnull,
                        "-Rpass-analysis=kernel-resource-usage", src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert len(re.findall(r"Function Name: \S*k_local_eq_boundary_polish", r.stderr)) == 1
    assert re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr) == ["0"]
    lds = [int(v) for v in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stderr)]
    assert lds == [7 * 360 * 8] and lds[0] <= 20 * 1024
    assert [int(v) for v in re.findall(r"Occupancy \[waves/SIMD\]: (\d+)", r.stderr)] == [2]


def test_arguments_are_checked_before_any_device_work():
    """the name is declared in include/ibs.h and exported; a NULL required argument: IBS_ERR_ARG with "null" in the message; ld < N,
    ps_ld < N, n_ray < 1, n_theta0 < 1, n_starts outside [1, 4], max_eval outside [1, 64], xtol_theta0 <= 0 or non-finite, xtol outside
    [0, 1), a non-finite shift, unknown flags: IBS_ERR_ARG; N = 512, 65, 65,539: IBS_ERR_UNSUPPORTED.  The checks come before the context
    is touched, so a zeroed buffer stands for it and for the arrays."""
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ibs.h")).read(), flags=re.S)
    assert "int %s(" % NAME in hdr and NAME in _lib.SYMBOLS
    lib = _lib.lib()
    fn = getattr(lib, NAME)
    buf = C.create_string_buffer(1 << 16)
    P = C.cast(buf, C.c_void_p)
    N = 513

    def call(ctx=P, n=N, ld=None, geo=P, dP=P, centre=P, sigma=P, ps=None, ps_ld=None, rays=P, n_theta0=1, theta0=P, t_row=P, shift=0.0,
             xtol=1e-12, n_starts=1, xt0=1e-5, max_eval=32, x=P, t=P, ts=P, tu=P, n_ray=1, flags=0):
        return fn(ctx, 1, n_ray, n, -1.0, 0.05, geo, n if ld is None else ld, dP, centre, sigma, ps, n if ps_ld is None else ps_ld, rays,
                  n_theta0, theta0, t_row, shift, xtol, n_starts, xt0, max_eval, x, t, ts, tu, None, None, None, None, None, flags)

    for kw in (dict(ctx=None), dict(geo=None), dict(dP=None), dict(centre=None), dict(sigma=None), dict(rays=None), dict(theta0=None),
               dict(t_row=None), dict(x=None), dict(t=None), dict(ts=None), dict(tu=None)):
        assert call(**kw) == IBS_ERR_ARG, kw
        assert b"null" in lib.ibs_last_error()
    assert call(ld=N - 1) == IBS_ERR_ARG
    assert call(ps=P, ps_ld=N - 1) == IBS_ERR_ARG
    assert call(n_ray=0) == IBS_ERR_ARG
    for nt in (0, -1, 2521):
        assert call(n_theta0=nt) == IBS_ERR_ARG, nt
    for k in (0, 5, -1):
        assert call(n_starts=k) == IBS_ERR_ARG, k
    for me in (0, 65, -1):
        assert call(max_eval=me) == IBS_ERR_ARG, me
    for xt0 in (0.0, -1e-5, float("nan"), float("inf")):
        assert call(xt0=xt0) == IBS_ERR_ARG, xt0
    for xtol in (-1e-3, 1.0, 2.0, float("nan"), float("inf")):
        assert call(xtol=xtol) == IBS_ERR_ARG, xtol
    for shift in (float("nan"), float("inf"), -float("inf")):
        assert call(shift=shift) == IBS_ERR_ARG, shift
    assert call(flags=2) == IBS_ERR_ARG
    assert call(n_theta0=2, flags=1) == IBS_ERR_ARG                 # (host pointers: a zeroed theta0 is not strictly increasing)
    for n in (512, 65, 65539):
        assert call(n=n) == IBS_ERR_UNSUPPORTED, n


def test_driver_needs_the_resident_path():
    """BallooningScan.local_eq_boundary_envelope and local_eq_boundary_sensitivity(theta0_polish=True) without tables= and device=:
    ValueError, before any device work (the context is never used); an unknown axis and n_starts outside [1, 4] are ValueErrors"""
    th = np.linspace(-4 * np.pi, 4 * np.pi, 513)
    svals = np.array([0.6, 0.9])
    scan = ibs_amd.BallooningScan(None, None, th, svals, nalpha=3, ntheta0=2)
    with pytest.raises(ValueError):
        scan.local_eq_boundary_envelope([0.0], (0.2, 3.0))
    with pytest.raises(ValueError):
        scan.local_eq_boundary_sensitivity([0.0], (0.2, 3.0), theta0_polish=True)
    tabs = ibs_amd.SurfaceTables.from_wout(dict(np.load(os.path.join(G, "G8_wout_ncsx_op.npz"))), svals)
    with pytest.raises(ValueError):
        ibs_amd.BallooningScan(None, None, th, svals, nalpha=3, ntheta0=2, tables=tabs).local_eq_boundary_envelope([0.0], (0.2, 3.0))
    on_dev = ibs_amd.BallooningScan(None, None, th, svals, nalpha=3, ntheta0=2, tables=tabs, device="cuda:0")
    with pytest.raises(ValueError):
        on_dev.local_eq_boundary_envelope([0.0], (0.2, 3.0), axis="q")
    for k in (0, 5, True, 1.0):
        with pytest.raises(ValueError):
            on_dev.local_eq_boundary_envelope([0.0], (0.2, 3.0), n_starts=k)
