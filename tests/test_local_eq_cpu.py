"""CPU: the rule of the local-equilibrium scan (ibs_amd.operators.local_eq_fold, csrc/ibs_local_eq.hpp) against the geometry oracle
re-evaluated with a varied shear and pressure gradient, against the reference's s-alpha stability table (G2), and the argument rules of
ibs_local_eq_scan_f64 without a GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from ibs_amd import _lib, local_eq_fold
from oracle import ballooning_oracle as bo
from oracle import geometry_oracle as go
from tests.local_eq_cases import salpha_base_line

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(os.path.dirname(__file__), "golden")
IBS_ERR_ARG, IBS_ERR_UNSUPPORTED = -1, -3
NAME = "ibs_local_eq_scan_f64"


@pytest.fixture(scope="module")
def g8():
    return dict(np.load(os.path.join(G, "G8_surface_tables.npz")))


@pytest.fixture(scope="module")
def base_lines(g8):
    """the unvaried lines of test 1, computed once: {(js, alpha): (8, N)} on theta_grid(131)"""
    th = bo.theta_grid(131)
    return th, {(js, al): go.fieldline_geometry(g8, js, [al], th)[0] for js in (1, 2) for al in (0.0, 1.0)}


@pytest.mark.parametrize("js", [1, 2])
@pytest.mark.parametrize("alpha", [0.0, 1.0])
def test_fold_equals_the_geometry_of_the_varied_equilibrium(g8, base_lines, js, alpha):
    """d_iota_d_s (1 + eps) and d_pressure_d_s p in the tables, the oracle's geometry of that equilibrium folded at theta0, against
    local_eq_fold on the base line: cvdrift, gds2 and dPdrho within 1e-12 of each array's largest magnitude (the two sides are
    algebraically identical; the bound leaves room for N-term rounding and nothing else)"""
    th, lines = base_lines
    base = lines[(js, alpha)]
    dP = bo.dPdrho_of(base[2], base[7], base[0])
    sigma = float(np.sign(-g8["phiedge"]))
    worst = 0.0
    for eps in (-0.5, 0.3, 1.0):
        for p in (0.5, 1.7):
            tab = dict(g8)
            tab["d_iota_d_s"] = g8["d_iota_d_s"] * (1.0 + eps)
            tab["d_pressure_d_s"] = g8["d_pressure_d_s"] * p
            var = go.fieldline_geometry(tab, js, [alpha], th)[0]
            assert np.array_equal(var[0], base[0]) and np.array_equal(var[1], base[1])        # bmag, gradpar: untouched
            dP_var = bo.dPdrho_of(var[2], var[7], var[0])
            for t0 in (0.0, 0.4):
                cv_ref, gd_ref = bo.fold_theta0(t0, var[2], var[3], var[4], var[5], var[6])
                dP_new, cv, gd = local_eq_fold(th, base, dP, alpha, sigma, t0, eps, p)
                e = (np.abs(cv - cv_ref).max() / np.abs(cv_ref).max(), np.abs(gd - gd_ref).max() / np.abs(gd_ref).max(),
                     abs(dP_new - dP_var) / abs(dP_var))
                worst = max(worst, *e)
                assert max(e) <= 1e-12, (eps, p, t0, e)
    print("worst relative difference: %.2e" % worst)


@pytest.mark.parametrize("col,N,extent", [(4, 401, 20), (3, 1601, 61)])
def test_rule_reproduces_the_reference_stability_table(col, N, extent):
    """all 240 rows of G2 (check_ball and check_ball_long) from three base lines at shat0 = 1, alpha0 = 0.5 by the rule with the
    Pfirsch-Schlueter row: the Sturm count above 0 of the varied rows is positive exactly where the reference says unstable"""
    tab = np.load(os.path.join(G, "G2_salpha_stability.npz"))["table"]
    th = np.linspace(-extent * np.pi, extent * np.pi, N)
    got = np.empty(len(tab), dtype=int)
    for t0 in np.unique(tab[:, 2]):
        line, dP, ps = salpha_base_line(th, t0)
        for k in np.nonzero(tab[:, 2] == t0)[0]:
            shat, alpha = tab[k, 0], tab[k, 1]
            dPv, cv, gd = local_eq_fold(th, line, dP, t0, 1.0, 0.0, shat / 1.0 - 1.0, alpha / 0.5, ps=ps)
            g, c, f = bo.gcf(dPv, line[0], line[1], cv, gd)
            gref, cref = bo.salpha_gc(th, shat, alpha, t0)
            assert np.abs(g - gref).max() <= 1e-12 * np.abs(gref).max() and np.abs(c - cref).max() <= 1e-12 * np.abs(cref).max()
            d, e, fd, *_ = bo.assemble(th, g, c, f)
            got[k] = int(bo.sturm_count_above(d, e, fd, 0.0) > 0)
    assert (got != tab[:, col].astype(int)).sum() == 0


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")
def test_kernel_has_no_scratch():
    """k_local_eq_scan (csrc/ibs_local_eq.hip) compiles for gfx950 with ScratchSize 0 and the 18 KB of LDS of the long path"""
    src = os.path.join(ROOT, "ideal-ballooning-solver_amd", "csrc", "ibs_local_eq.hip")
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-c", "--cuda-device-only", "-o", os.devnull,
                        "-Rpass-analysis=kernel-resource-usage", src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert len(re.findall(r"Function Name: \S*k_local_eq_scan", r.stderr)) == 1
    assert re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr) == ["0"]
    assert re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stderr) == ["18432"]


def test_arguments_are_checked_before_any_device_work():
    """the name is declared in include/ibs.h and exported; NULL required argument, ld < N, all outputs NULL: IBS_ERR_ARG; N = 512, 65,
    65,539: IBS_ERR_UNSUPPORTED.  The checks come before the context is touched, so a zeroed buffer stands for it and for the arrays."""
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ibs.h")).read(), flags=re.S)
    assert "int %s(" % NAME in hdr and NAME in _lib.SYMBOLS
    lib = _lib.lib()
    fn = getattr(lib, NAME)
    buf = C.create_string_buffer(1 << 16)
    P = C.cast(buf, C.c_void_p)
    N = 513

    def call(ctx=P, n=N, ld=None, geo=P, dP=P, centre=P, sigma=P, ps=None, var=P, gam=P, lam=None, count=None, n_var=1, flags=0):
        return fn(ctx, 1, n_var, n, -1.0, 0.05, geo, n if ld is None else ld, dP, centre, sigma, ps, n, var, 0.0, gam, lam, count, None, flags)

    for kw in (dict(ctx=None), dict(geo=None), dict(dP=None), dict(centre=None), dict(sigma=None), dict(var=None)):
        assert call(**kw) == IBS_ERR_ARG, kw
        assert b"null" in lib.ibs_last_error()
    assert call(gam=None) == IBS_ERR_ARG                     # all three outputs NULL
    assert call(ld=N - 1) == IBS_ERR_ARG
    assert call(n_var=0) == IBS_ERR_ARG
    assert call(flags=2) == IBS_ERR_ARG
    for n in (512, 65, 65539):
        assert call(n=n) == IBS_ERR_UNSUPPORTED, n
        assert call(n=n, gam=None, count=P) == IBS_ERR_UNSUPPORTED, n
