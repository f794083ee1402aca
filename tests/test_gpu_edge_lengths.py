"""GPU: every entry point at grid lengths on lane, chunk and path edges (tests/edge_cases.py: the lengths, each with its reason, and
the moving-well family whose mode sits on a chosen grid point; both pinned on the CPU in tests/test_edge_cases_cpu.py).

The rest of the suite runs at N = 2^k + 1 and a few reference grids; there the last chunk of the long path (csrc/ibs_long.hpp) always
holds 255, 127 or 511 rows, the two-grid start is always on, the twist row of the eigenvector stage and of the adjoint solve sits
mid-grid, and the geometry-fed register kernels run at 5 of their 31 rows-per-lane instantiations.

Tolerances: none is new.  Short grids (N <= 2050): gam 1e-10, X 1e-7, dX 1e-7 max|dX| + 1e-7 (test_gpu_parity.py:
test_every_rows_per_lane_instantiation), d gam / d theta0 1e-8 and objective 1e-9 (test_driver_on_gpu_matches_oracle_backed_driver,
test_G4_obj_w_grad_kernel).  Long grids: gam 1e-8, X 1e-6, dX 1e-5 max(1, max|dX|) (test_gpu_round6.py:
test_large_grid_salpha_against_the_oracle), d gam / d theta0 1e-7 max(1, |ref|) (test_large_grid_geometry_fed_scan_with_theta0_
derivative), objective 1e-8 and 1e-6 max(1, |jac|) (test_large_grid_obj_w_grad_against_the_oracle).  lam: 4 N eps ||A||
(test_gpu_configs.py: test_config5_fp64_one_million_systems).  Counts: exact.  VJP rows: 1e-9 of each row's norm (test_gpu_vjp.py:
test_vjp_matches_restatement).  Variants of one scan against the plain scan: as test_large_grid_scan_variants_agree_with_the_plain_scan
(bit for bit) and test_chained_scan_matches_unchained / test_subwave_chained_and_warm_scan (other kernels: gam 1e-11, X 1e-6, lam
1e-10 up to the ||A|| of those tests and the solver's own certificate beyond: tol_lam_between_kernels; d gam / d theta0: same_scan)."""
import os

import numpy as np
import pytest

from oracle import ballooning_oracle as bo
from oracle import c_oracle as co
from tests import edge_cases as ec
from tests import vjp_oracle as vo
from tests.helpers import synthetic_fieldlines
from tests.nearest_oracle import dense_nearest, window_nearest
from tests.test_edge_cases_cpu import shallow_partner

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
EPS = ec.EPS
SHORT, LONG, COUNT = ec.EDGE_N_SHORT, ec.EDGE_N_LONG, ec.EDGE_N_COUNT


@pytest.fixture(scope="module")
def ctx():
    import ibs_amd
    c = ibs_amd.Context(0)
    yield c
    c.close()


def note(entry, N, ctx=None, name=None):
    """one line per (entry point, N[, kernel]) for the run's log (pytest -s / -rP)"""
    print("edge-case: %s N=%d kernel=%s" % (entry, N, name if name is not None else (ctx.last_launch()[0] if ctx else "-")))


def is_short(N):
    return N <= 2050


def tol_gam(N):
    return 1e-10 if is_short(N) else 1e-8


def tol_X(N):
    return 1e-7 if is_short(N) else 1e-6


def tol_dX(N, dX_ref):
    m = float(np.abs(dX_ref).max())
    return 1e-7 * m + 1e-7 if is_short(N) else 1e-5 * max(1.0, m)


def tol_dth0(N, ref):
    return 1e-8 if is_short(N) else 1e-7 * max(1.0, abs(ref))


def clean(info, N=None, no_reclose=False):
    """status words: nothing flagged; on the moving well at long N nothing re-closed either (division form has nothing to re-close)"""
    st = np.asarray(info.cpu() if hasattr(info, "cpu") else info) >> 16
    assert ((st & 3) == 0).all(), (N, st)
    if no_reclose:
        assert ((st & 8) == 0).all(), (N, st)


def up_to_sign(X, Xref):
    """X with the sign of Xref at its largest entry (utils.py:1605 normalises by max |x| and fixes no sign)"""
    k = int(np.argmax(np.abs(Xref)))
    return 1.0 if X[k] * Xref[k] >= 0 else -1.0


def check_pair(N, tag, lam, gam, X, dX, ref, nA):
    """(lam, gam, X, dX) of one system against ref = (gam, lam, X, dX) of the oracle; every figure goes to the log before it is held
    to its bound"""
    gam_o, lam_o, X_o, dX_o = ref
    s = up_to_sign(X, X_o)
    e = (abs(lam - lam_o) / (N * EPS * nA), abs(gam - gam_o), float(np.abs(s * X - X_o).max()), float(np.abs(s * dX - dX_o).max()))
    print("edge-case figures: N=%d %s  |dlam| = %.2f N eps ||A||  |dgam| = %.1e  |dX| = %.1e  |ddX| = %.1e (bound %.1e)"
          % (N, tag, e[0], e[1], e[2], e[3], tol_dX(N, dX_o)))
    assert e[0] <= 4.0, (N, tag, "lam", e[0])
    assert e[1] < tol_gam(N), (N, tag, "gam", e[1])
    assert e[2] < tol_X(N), (N, tag, "X", e[2])
    assert e[3] < tol_dX(N, dX_o), (N, tag, "dX", e[3])
    assert abs(np.abs(X).max() - 1.0) < 1e-15 and X[0] == 0.0 and X[-1] == 0.0, (N, tag)


def salpha_rows(N, n=3, seed=0):
    """n smooth s-alpha systems with f != g (the family of test_subwave_variants_match_full_wave)"""
    th = ec.theta_grid(N)
    params = [(1.0, 0.8, 0.0), (0.5, 0.6, 0.3), (1.7, 1.1, 0.1)]
    if n > 3:
        rng = np.random.default_rng(seed + N)
        params += [(rng.uniform(0.2, 2), rng.uniform(0.1, 1.2), rng.uniform(0, 1.5)) for _ in range(n - 3)]
    g = np.empty((n, N)); c = np.empty_like(g)
    for k, (sh, al, t0) in enumerate(params[:n]):
        g[k], c[k] = bo.salpha_gc(th, sh, al, t0)
    return th, g, c, g * (1 + 0.3 * np.cos(th))[None]


def well_batch(N, targets):
    th = ec.theta_grid(N)
    rows = [ec.well_rows(th, j) for j in targets]
    return th, [np.stack([r[i] for r in rows]) for i in range(3)]


def raw_kernel(N, dtype="double", gh=False):
    """the kernel a handful of systems takes in ibs_solve_gcf_f64 / _f32 (with gam) / ibs_solve_gcfh_f64 (csrc/ibs_plan.hpp: plan_gcf)"""
    M = ec.rows_per_lane(N)
    if not is_short(N):
        return "ibs::k_solve_gcf_long<%s>" % dtype
    if dtype == "float":
        return "ibs::k_solve_gcf_rows<double, %d, float>" % M if M >= 24 else "ibs::k_solve_gcf_wide<%d>" % M
    if M >= 24 and not gh:
        return "ibs::k_solve_gcf_rows<double, %d, double>" % M
    return "ibs::k_solve_gcf<double, %d>" % M


def gcfh_reference(th, g, gh, c, f):
    """the oracle's solve on a caller-supplied half-grid g (rows of utils.py:1574-1592 with gh in place of the interpolated g)"""
    h = th[1] - th[0]
    e = gh[:-1] / h ** 2
    d = -(gh[1:-1] + gh[:-2]) / h ** 2 + c[1:-1]
    lam, x = bo.top_eigenpair(d, e, f[1:-1].copy())
    if x[np.argmax(np.abs(x))] < 0:
        x = -x
    gam, X, dX = bo.rayleigh_growth(x, h, g, c, f)
    return gam, lam, X, dX


# ------------------------------------------------------------------------------------------------ 1. raw solve, smooth systems
@pytest.mark.parametrize("N", SHORT + LONG)
def test_raw_solve_on_smooth_systems(ctx, N):
    """ibs_solve_gcf_f64 with X / dX, ibs_solve_gcf_f32 (FP32 arrays, FP64 solver) and ibs_solve_gcfh_f64 (caller's half-grid g) on
    s-alpha rows with f != g; on short grids also through the 32- and 16-lane forms where pick_lanes admits them"""
    th, g, c, f = salpha_rows(N)
    h = float(th[1] - th[0])
    nA = ec.norm_a(h, g, c, f)
    refs = [co.solve_gcf(h, g[k], c[k], f[k]) if not is_short(N) else bo.solve_gcf(th, g[k], c[k], f[k]) for k in range(len(g))]
    r = ctx.solve_gcf(h, g, c, f, want_X=True, want_info=True)
    assert ctx.last_launch()[0] == raw_kernel(N), (N, ctx.last_launch())
    note("solve_gcf_f64", N, ctx)
    assert r["nbad"] == 0
    clean(r["info"], N)
    for k in range(len(g)):
        check_pair(N, "salpha %d" % k, r["lam"][k], r["gam"][k], r["X"][k], r["dX"][k], refs[k], nA[k])
    # FP32 arrays: the widened form (test_fp32_variant_stated_tolerance; long grids: test_large_grid_salpha_against_the_oracle)
    g32, c32, f32 = (a.astype(np.float32) for a in (g, c, f))
    rw = ctx.solve_gcf(h, g32, c32, f32, want_X=True, want_info=True, dtype=np.float32)
    assert ctx.last_launch()[0] == raw_kernel(N, "float"), (N, ctx.last_launch())
    note("solve_gcf_f32", N, ctx)
    assert rw["gam"].dtype == np.float32 and rw["X"].dtype == np.float32
    clean(rw["info"], N)
    e_gam = float(np.abs(rw["gam"].astype(np.float64) - r["gam"]).max())
    print("edge-case figures: N=%d FP32 arrays |dgam| = %.1e" % (N, e_gam))
    if is_short(N):
        assert (np.abs(rw["lam"].astype(np.float64) - r["lam"]) < 2 * 1.2e-7 * nA).all()
        assert e_gam < 1e-6
        assert np.abs(rw["X"].astype(np.float64) - r["X"]).max() < 1e-5
        assert np.abs(rw["dX"].astype(np.float64) - r["dX"]).max() < 1e-4 * np.abs(r["dX"]).max()
    else:
        assert e_gam < 1e-4
    # the caller's own half-grid g: the analytic g at the half points, not the mean of neighbours
    gh = np.zeros_like(g)
    for k, (sh, al, t0) in enumerate([(1.0, 0.8, 0.0), (0.5, 0.6, 0.3), (1.7, 1.1, 0.1)]):
        gh[k] = bo.salpha_gc(th + 0.5 * h, sh, al, t0)[0]
    rh = ctx.solve_gcf(h, g, c, f, want_X=True, want_info=True, gh=gh)
    assert ctx.last_launch()[0] == raw_kernel(N, gh=True), (N, ctx.last_launch())
    note("solve_gcfh_f64", N, ctx)
    clean(rh["info"], N)
    for k in range(len(g)):
        check_pair(N, "gcfh %d" % k, rh["lam"][k], rh["gam"][k], rh["X"][k], rh["dX"][k], gcfh_reference(th, g[k], gh[k], c[k], f[k]), nA[k])
    # sub-wave forms
    for P in ec.lanes_allowed(N):
        ctx.set_option("force_p", P)
        try:
            rp = ctx.solve_gcf(h, g, c, f, want_X=True, want_info=True)
            name = ctx.last_launch()[0]
        finally:
            ctx.set_option("force_p", None)
        assert name == "ibs::k_solve_gcf_g<double, %d, %d, double>" % ((N - 2 + P - 1) // P, P), (N, P, name)
        note("solve_gcf_f64 force_p=%d" % P, N, name=name)
        assert rp["nbad"] == 0
        clean(rp["info"], N)
        for k in range(len(g)):
            check_pair(N, "P=%d salpha %d" % (P, k), rp["lam"][k], rp["gam"][k], rp["X"][k], rp["dX"][k], refs[k], nA[k])


# ------------------------------------------------------------------------------------------------ 2. raw solve, moving well
@pytest.mark.parametrize("N", [67, 131, 1985, 2049] + LONG)
def test_raw_solve_with_the_mode_on_chunk_edges(ctx, N):
    """the moving well at every twist target of the length: the twist row of the eigenvector stage on and next to multiples of 384,
    and a few rows from either end; on long grids the count around the returned eigenvalue as well"""
    targets = ec.twist_targets(N)
    th, (g, c, f) = well_batch(N, targets)
    h = float(th[1] - th[0])
    nA = ec.norm_a(h, g, c, f)
    r = ctx.solve_gcf(h, g, c, f, want_X=True, want_info=True)
    assert ctx.last_launch()[0] == raw_kernel(N), (N, ctx.last_launch())
    note("solve_gcf_f64 moving well (%d targets)" % len(targets), N, ctx)
    assert r["nbad"] == 0
    clean(r["info"], N, no_reclose=not is_short(N))
    for k, j in enumerate(targets):
        check_pair(N, "well at %d" % j, r["lam"][k], r["gam"][k], r["X"][k], r["dX"][k], bo.solve_gcf(th, g[k], c[k], f[k]), nA[k])
        kk = int(np.argmax(np.abs(r["X"][k])))
        assert (min(kk, N - 1 - kk) <= 6) if ec.is_end_target(N, j) else (kk == j), (N, j, kk)
    if not is_short(N):
        tol = 4 * N * EPS * nA
        assert np.array_equal(ctx.sturm_count(h, g, c, f, r["lam"] + tol), np.zeros(len(targets), dtype=np.int32))
        assert "k_sturm_count_long" in ctx.last_launch()[0]
        assert (ctx.sturm_count(h, g, c, f, r["lam"] - tol) >= 1).all()


# ------------------------------------------------------------------------------------------------ 3. / 4. geometry-fed scan
def scan_reference(N, th, lines, dP, t0):
    """(gam, lam (n_lines, n_t0) of the C oracle; X, dX (n_lines, n_t0, N), d gam / d theta0, ||A|| of the Python oracle)"""
    h = float(th[1] - th[0])
    nl, nt = len(lines), len(t0)
    gam_c, lam_c, _ = co.gamma_scan(h, *[lines[:, k, :] for k in range(7)], dP, t0)
    X = np.zeros((nl, nt, N)); dX = np.zeros_like(X); jac = np.zeros((nl, nt)); nA = np.zeros((nl, nt))
    for i in range(nl):
        for j in range(nt):
            cv, gd = bo.fold_theta0(t0[j], *lines[i, 2:7])
            gam, X[i, j], dX[i, j], gg, cc, ff = bo.gamma_ball_full(dP[i], th, lines[i, 0], lines[i, 1], cv, gd)
            assert abs(gam - gam_c[i, j]) < 0.1 * tol_gam(N)                          # (the two oracles: a tenth of the bound)
            gp = np.abs(lines[i, 1]); B = lines[i, 0]
            gdp = 2 * lines[i, 5] + 2 * t0[j] * lines[i, 6]
            jac[i, j] = bo.hf_derivative(gam, X[i, j], dX[i, j], ff, gp * gdp / B, -dP[i] * lines[i, 3] / (gp * B), gdp / B ** 3 / gp)  # utils.py:1669-1680
            nA[i, j] = ec.norm_a(h, gg, cc, ff)[0]
    return gam_c, lam_c, X, dX, jac, nA


def check_scan(N, tag, r, ref, with_X=True):
    gam_c, lam_c, X, dX, jac, nA = ref
    gam, lam = np.asarray(r["gam"]), np.asarray(r["lam"])
    e_gam = float(np.abs(gam - gam_c).max()); e_lam = float((np.abs(lam - lam_c) / (N * EPS * nA)).max())
    print("edge-case figures: N=%d %s  |dgam| = %.1e  |dlam| = %.2f N eps ||A||" % (N, tag, e_gam, e_lam))
    assert e_gam < tol_gam(N), (N, tag, e_gam)
    assert e_lam <= 4.0, (N, tag, e_lam)
    if "dgam_dtheta0" in r:
        d = np.asarray(r["dgam_dtheta0"])
        for i in range(jac.shape[0]):
            for j in range(jac.shape[1]):
                assert abs(d[i, j] - jac[i, j]) < tol_dth0(N, jac[i, j]), (N, tag, i, j, d[i, j], jac[i, j])
    if with_X and "X" in r:
        for i in range(X.shape[0]):
            for j in range(X.shape[1]):
                Xg, dXg = np.asarray(r["X"][i, j]), np.asarray(r["dX"][i, j])
                s = up_to_sign(Xg, X[i, j])
                assert np.abs(s * Xg - X[i, j]).max() < tol_X(N), (N, tag, i, j)
                assert np.abs(s * dXg - dX[i, j]).max() < tol_dX(N, dX[i, j]), (N, tag, i, j)


def scan_inputs(N, n_lines, t0):
    th = ec.theta_grid(N)
    lines = synthetic_fieldlines(th)(0.6, np.array([0.3, 1.7, 2.6])[:n_lines])
    dP = np.array([bo.dPdrho_of(ln[2], ln[7], ln[0]) for ln in lines])
    return th, lines, dP, np.asarray(t0, dtype=np.float64)


def scan_norm_a(h, lines, dP, t0):
    """||A|| of every (line, theta0) system of a scan (n_lines, n_t0)"""
    out = np.zeros((len(lines), len(t0)))
    for i, ln in enumerate(lines):
        for j, t in enumerate(t0):
            cv, gd = bo.fold_theta0(t, *ln[2:7])
            out[i, j] = ec.norm_a(h, *bo.gcf(dP[i], ln[0], ln[1], cv, gd))[0]
    return out


def tol_lam_between_kernels(nA):
    """two register kernels on one system: 1e-10 where the suite states it (test_chained_scan_matches_unchained,
    test_subwave_chained_and_warm_scan: N <= 1025, ||A|| <= 7e3, "lam is certified to 256 ulp(||A||)"); beyond, that certificate
    itself -- the shift iteration closes on a bracket of 4 x 64 eps ||A|| (csrc/ibs_wave.hpp: solve(), tol = 64 eps ||A||), so two
    certified results lie within 512 eps ||A|| of each other"""
    return np.maximum(1e-10, 512 * EPS * np.asarray(nA))


def same_scan(N, tag, r, base, nA, X=True):
    """another kernel on the same systems (test_chained_scan_matches_unchained, test_subwave_chained_and_warm_scan).  The theta0
    derivative is first order in the eigenvector, whose error grows with ||A|| / gap: the suite's 1e-9 between kernels was set at
    N <= 1025; here the bound is the one the quantity has against the oracle on short grids, 1e-8 (tol_dth0)."""
    assert r["nbad"] == 0, (N, tag)
    e_gam, e_lam = float(np.abs(r["gam"] - base["gam"]).max()), float((np.abs(r["lam"] - base["lam"]) / tol_lam_between_kernels(nA)).max())
    print("edge-case figures: N=%d %s against the plain scan  |dgam| = %.1e  |dlam| = %.2f of its bound" % (N, tag, e_gam, e_lam))
    assert e_gam < 1e-11 and e_lam < 1.0, (N, tag, e_gam, e_lam)
    if "dgam_dtheta0" in r:
        assert np.abs(r["dgam_dtheta0"] - base["dgam_dtheta0"]).max() < tol_dth0(N, 0.0), (N, tag, np.abs(r["dgam_dtheta0"] - base["dgam_dtheta0"]).max())
    if X and "X" in r:
        assert np.abs(r["X"] - base["X"]).max() < 1e-6 and np.abs(r["dX"] - base["dX"]).max() < 1e-5, (N, tag)


def device_variants_equal_the_plain_scan(ctx, N, h, lines, dP, t0, n_surf, nA):
    """fused argmax, one (line, theta0) per point and the warm scan on device tensors against the plain scan, as
    test_large_grid_scan_variants_agree_with_the_plain_scan asserts it"""
    import torch
    dev = torch.device("cuda:0")
    geo = [torch.from_numpy(np.ascontiguousarray(lines[:, k, :])).to(dev) for k in range(7)]
    dP_d, t0_d = torch.from_numpy(dP).to(dev), torch.from_numpy(t0).to(dev)
    base = ctx.gamma_scan(h, *geo, dP_d, t0_d, want_info=True)
    clean(base["info"], N)
    am = ctx.gamma_scan_argmax(h, geo, dP_d, t0_d, n_surf)
    note("gamma_scan_argmax", N, ctx)
    assert torch.equal(am["gam"], base["gam"]) and torch.equal(am["lam"], base["lam"]), N
    per = len(lines) // n_surf
    for s in range(n_surf):
        blk = base["gam"][per * s:per * s + per].reshape(-1)
        k = int(torch.argmax(blk))
        assert float(am["pack"][s, 0]) == float(blk[k]) and int(am["pack"][s, 1]) == k, (N, s)
    col = len(t0) - 1
    pts = ctx.gamma_points(h, *geo, dP_d, torch.from_numpy(np.full(len(lines), t0[col])).to(dev))
    note("gamma_points", N, ctx)
    assert torch.equal(pts["gam"], base["gam"][:, col]) and torch.equal(pts["lam"], base["lam"][:, col]), N
    warm = ctx.gamma_scan(h, *geo, dP_d, t0_d, lam_guess=base["lam"], guess_width=1e-3)
    note("gamma_scan_warm", N, ctx)
    if is_short(N):        # (register kernels: a guess changes the shift iteration, not the certified result)
        same_scan(N, "warm", dict(gam=warm["gam"].cpu().numpy(), lam=warm["lam"].cpu().numpy(), nbad=0),
                  dict(gam=base["gam"].cpu().numpy(), lam=base["lam"].cpu().numpy()), nA)
    else:
        assert torch.equal(warm["gam"], base["gam"]), N
    return base


@pytest.mark.parametrize("N", SHORT)
def test_geometry_fed_scan_at_every_rows_per_lane(ctx, N):
    """ibs_gamma_scan_f64 (X, dX, d gam / d theta0), the fused argmax, gamma_points and the warm scan on three smooth lines x four
    theta0 against the oracle; then the chained kernel (2 and 4 theta0 per wave) and the 32- / 16-lane forms, plain and chained"""
    M = ec.rows_per_lane(N)
    th, lines, dP, t0 = scan_inputs(N, 3, [0.0, 0.4, 0.8, 1.2])
    h = float(th[1] - th[0])
    a = [np.ascontiguousarray(lines[:, k, :]) for k in range(7)]
    ref = scan_reference(N, th, lines, dP, t0)
    base = ctx.gamma_scan(h, *a, dP, t0, want_X=True, want_dtheta0=True, want_info=True)
    assert ctx.last_launch()[0] == "ibs::k_gamma_scan<double, %d>" % M, (N, ctx.last_launch())
    note("gamma_scan_f64", N, ctx)
    assert base["nbad"] == 0
    clean(base["info"], N)
    check_scan(N, "plain", base, ref)
    dbase = device_variants_equal_the_plain_scan(ctx, N, h, lines, dP, t0, 1, ref[5])
    assert np.array_equal(dbase["gam"].cpu().numpy(), ctx.gamma_scan(h, *a, dP, t0)["gam"])              # host and device arrays
    try:
        for chain in (2, 4):
            ctx.set_option("scan_chain", chain)
            r = ctx.gamma_scan(h, *a, dP, t0, want_X=True, want_dtheta0=True, want_info=True)
            assert ctx.last_launch()[0] == "ibs::k_gamma_scan_chain<double, %d>" % M, (N, chain, ctx.last_launch())
            note("gamma_scan_f64 scan_chain=%d" % chain, N, ctx)
            clean(r["info"], N)
            same_scan(N, "chain %d" % chain, r, base, ref[5])
            check_scan(N, "chain %d" % chain, r, ref)
            rn = ctx.gamma_scan(h, *a, dP, t0)                                  # (no X: no per-wave LDS row from M = 3 on)
            assert ctx.last_launch()[0] == "ibs::k_gamma_scan_chain<double, %d>" % M
            same_scan(N, "chain %d, no X" % chain, rn, base, ref[5])
        ctx.set_option("scan_chain", None)
        # sub-wave forms: eight theta0, so that a group of the 16-lane form still has two slots to chain
        if ec.lanes_allowed(N):
            t8 = np.linspace(0.0, 1.4, 8)
            ctx.set_option("force_p", 64); ctx.set_option("scan_chain", 1)
            plain8 = ctx.gamma_scan(h, *a, dP, t8, want_X=True, want_dtheta0=True, want_info=True)
            assert ctx.last_launch()[0] == "ibs::k_gamma_scan<double, %d>" % M
            ref8 = co.gamma_scan(h, *a, dP, t8)[0]
            nA8 = scan_norm_a(h, lines, dP, t8)
            assert np.abs(plain8["gam"] - ref8).max() < tol_gam(N)
        for P in ec.lanes_allowed(N):
            Mg = (N - 2 + P - 1) // P
            ctx.set_option("force_p", P)
            for chain in (1, 2) + ((4,) if P == 32 else ()):
                ctx.set_option("scan_chain", chain)
                r = ctx.gamma_scan(h, *a, dP, t8, want_X=True, want_dtheta0=True, want_info=True)
                want = "ibs::k_gamma_scan_g%s<double, %d, %d>" % ("_chain" if chain > 1 else "", Mg, P)
                assert ctx.last_launch()[0] == want, (N, P, chain, ctx.last_launch())
                note("gamma_scan_f64 force_p=%d scan_chain=%d" % (P, chain), N, ctx)
                clean(r["info"], N)
                same_scan(N, "P=%d chain %d" % (P, chain), r, plain8, nA8)
                assert np.abs(r["gam"] - ref8).max() < tol_gam(N)
            ctx.set_option("scan_chain", 1)
            warm = ctx.gamma_scan(h, *a, dP, t8, lam_guess=plain8["lam"], guess_width=1e-3)
            assert ctx.last_launch()[0] == "ibs::k_gamma_scan_g_chain<double, %d, %d>" % (Mg, P), (N, P, ctx.last_launch())
            note("gamma_scan_warm force_p=%d" % P, N, ctx)
            same_scan(N, "P=%d warm" % P, warm, plain8, nA8)
    finally:
        ctx.set_option("force_p", None); ctx.set_option("scan_chain", None)


@pytest.mark.parametrize("N", LONG)
def test_geometry_fed_scan_on_long_edges(ctx, N):
    """the same entry points on the long path (rows assembled on the device, division-form solver), and the moving well mapped onto
    geometry arrays at four twist targets"""
    big = N > 60000
    th, lines, dP, t0 = scan_inputs(N, 1 if big else 2, [0.0, 1.1] if big else [0.0, 0.4, 1.1])
    h = float(th[1] - th[0])
    a = [np.ascontiguousarray(lines[:, k, :]) for k in range(7)]
    ref = scan_reference(N, th, lines, dP, t0)
    r = ctx.gamma_scan(h, *a, dP, t0, want_X=True, want_dtheta0=True, want_info=True)
    assert ctx.last_launch()[0] == "ibs::k_solve_gcf_long<double>", (N, ctx.last_launch())
    note("gamma_scan_f64", N, ctx)
    assert r["nbad"] == 0
    clean(r["info"], N)
    check_scan(N, "plain", r, ref)
    device_variants_equal_the_plain_scan(ctx, N, h, lines, dP, t0, 1, ref[5])
    # the mapped moving well: both ends, on a multiple of 384 and two rows past another
    t = ec.twist_targets(N)
    targets = [t[0], t[1], t[3], t[-1]]
    thw, (g, c, f) = well_batch(N, targets)
    geo = [np.stack(x) for x in zip(*[ec.to_geometry(g[k], c[k], f[k]) for k in range(len(targets))])]
    nA = ec.norm_a(h, g, c, f)
    rw = ctx.gamma_scan(h, *geo, np.full(len(targets), -1.0), np.array([0.0]), want_X=True, want_info=True)
    note("gamma_scan_f64 mapped moving well", N, ctx)
    assert rw["nbad"] == 0
    clean(rw["info"], N, no_reclose=True)
    for k, j in enumerate(targets):
        check_pair(N, "mapped well at %d" % j, rw["lam"][k, 0], rw["gam"][k, 0], rw["X"][k, 0], rw["dX"][k, 0],
                   bo.solve_gcf(th, g[k], c[k], f[k]), nA[k])
        kk = int(np.argmax(np.abs(rw["X"][k, 0])))
        assert (min(kk, N - 1 - kk) <= 6) if ec.is_end_target(N, j) else (kk == j), (N, j, kk)


# ------------------------------------------------------------------------------------------------ 5. objective with gradient
def objective_points(N, pts, d=0.004):
    th = ec.theta_grid(N)
    fl = synthetic_fieldlines(th)
    geo = np.stack([fl(s_, np.array([a_ - d / 2, a_, a_ + d / 2])) for s_, a_, _ in pts])          # (n_pts, 3, 8, N)
    return th, geo, np.array([p[2] for p in pts])


def check_objective(N, k, val, jac, ref):
    vo_, jo = ref
    print("edge-case figures: N=%d objective point %d  |dval| = %.1e  |djac| = %.1e" % (N, k, abs(val - vo_), np.abs(jac - jo).max()))
    if is_short(N):
        assert abs(val - vo_) < 1e-9 and np.abs(jac - jo).max() < 1e-8, (N, k, val, vo_, jac, jo)
    else:
        assert abs(val - vo_) < 1e-8 and np.abs(jac - jo).max() < 1e-6 * max(1.0, np.abs(jo).max()), (N, k, val, vo_, jac, jo)


@pytest.mark.parametrize("N", SHORT + LONG)
def test_objective_with_gradient_at_every_rows_per_lane(ctx, N):
    """ibs_obj_w_grad_f64 on three (s, alpha, theta0) points of the smooth family against utils.py:1632-1728 restated; host and device
    arrays give the same bits"""
    import torch
    dev = torch.device("cuda:0")
    d = 0.004
    th, geo, t0 = objective_points(N, [(0.6, 1.0, 0.4), (0.8, 2.2, 0.0), (0.5, 0.3, 1.1)], d)
    h = float(th[1] - th[0])
    val, jac, info = ctx.obj_w_grad(h, geo, t0, d, want_info=True)
    want = "ibs::k_obj_w_grad<double, %d>" % ec.rows_per_lane(N) if is_short(N) else "ibs::k_solve_gcf_long<double>"
    assert ctx.last_launch()[0] == want, (N, ctx.last_launch())
    note("obj_w_grad_f64", N, ctx)
    clean(info, N)
    for k in range(len(t0)):
        check_objective(N, k, val[k], jac[k], bo.obj_w_grad_lines(th, t0[k], geo[k, 0], geo[k, 1], geo[k, 2], d))
    v2, j2 = ctx.obj_w_grad(h, torch.from_numpy(geo).to(dev), torch.from_numpy(t0).to(dev), d)
    assert np.array_equal(v2.cpu().numpy(), val) and np.array_equal(j2.cpu().numpy(), jac), N


def test_objective_beyond_512_points_at_2307_fresh_context():
    """more than 512 points in one call on a context that has done nothing else: its long-grid workspace is sized and carved by this
    call, at a length whose last chunk holds one row.  Against the same points in batches of 128, and the oracle on three of them."""
    import ibs_amd
    N, n, d = 2307, 520, 0.004
    rng = np.random.default_rng(2307)
    pts = [(rng.uniform(0.3, 0.9), rng.uniform(0.0, 2.8), rng.uniform(0.0, 1.3)) for _ in range(n)]
    th, geo, t0 = objective_points(N, pts, d)
    h = float(th[1] - th[0])
    fresh = ibs_amd.Context(0)
    try:
        val, jac, info = fresh.obj_w_grad(h, geo, t0, d, want_info=True)
        assert fresh.last_launch()[0] == "ibs::k_solve_gcf_long<double>"
        note("obj_w_grad_f64 520 points", N, fresh)
        clean(info, N)
        for p0 in range(0, n, 128):
            v, j, i = fresh.obj_w_grad(h, geo[p0:p0 + 128], t0[p0:p0 + 128], d, want_info=True)
            assert np.array_equal(v, val[p0:p0 + 128]) and np.array_equal(j, jac[p0:p0 + 128]) and np.array_equal(i, info[p0:p0 + 128]), p0
    finally:
        fresh.close()
    for k in (0, 259, 519):
        check_objective(N, k, val[k], jac[k], bo.obj_w_grad_lines(th, t0[k], geo[k, 0], geo[k, 1], geo[k, 2], d))


# ------------------------------------------------------------------------------------------------ 6. refinement
@pytest.mark.parametrize("N", SHORT)       # (67, 131, 643, 1473, 2049 and one length for every other M: a call costs half a second)
def test_refinement_on_the_device_equals_the_host_driven_steps(ctx, N):
    """ibs_refine_f64 (k_refine_eval<M>) through BallooningScan's device pipeline against the steps it replaces, driven from the
    host; same kernels on the same inputs, bit for bit (the pattern of test_device_rows_equal_the_host_driven_steps)"""
    import torch
    import ibs_amd
    dev = torch.device("cuda:0")
    wout = dict(np.load(os.path.join(G, "G8_wout_ncsx_op.npz")))
    sv = np.linspace(0.5, 0.95, 5)
    th = ibs_amd.theta_grid(N)
    scan = ibs_amd.BallooningScan(ctx, None, th, sv, tables=ibs_amd.SurfaceTables.from_wout(wout, sv), device=dev)
    ph = {}
    rows, bad = scan.device_rows(True, ph)
    rows = rows.cpu().numpy()
    assert float(bad) == 0 and set(ph) == {"geometry_ms", "scan_argmax_ms", "refine_ms", "final_solve_ms"}
    tabs = scan.coarse()
    starts = np.array([ibs_amd.pick_start(t, scan.alpha_scan, scan.theta0_scan)[:2] for t in tabs])
    xo, fo, ne = scan.refine_device(starts)
    evals, sweeps, rounds, _ = ctx.refine_stats()
    assert evals >= len(sv) and (ne >= 1).all() and sweeps > 0 and rounds >= 1, (N, evals, ne, sweeps, rounds)
    gam = scan.final_solve_device(xo)
    # (the evaluation kernel is picked by N alone, launch_table().refine_f64[M]: named here for the log, not read back)
    note("refine_f64 (%d evaluations)" % evals, N, name="ibs::k_refine_eval<double, %d>" % ec.rows_per_lane(N))
    assert np.array_equal(rows[:, 0], xo[:, 1]) and np.array_equal(rows[:, 1], xo[:, 0]) and np.array_equal(rows[:, 2], gam), N
    assert np.array_equal(scan.last_refine["n_evals"].cpu().numpy(), ne)
    t0a, ala, gama = scan.run()
    assert np.array_equal(gama, gam)
    c0, ca, cg = scan.run(refine=False)
    assert np.array_equal(cg, tabs.reshape(5, -1).max(axis=1)) and np.array_equal(np.stack([ca, c0], axis=1), starts)


# ------------------------------------------------------------------------------------------------ 7. nearest sigma
@pytest.mark.parametrize("N", [67, 131, 2049] + LONG)
def test_nearest_sigma_on_edge_lengths(ctx, N):
    """ibs_solve_gcf_nearest_f64 and ibs_gamma_scan_nearest_f64: the s-alpha line of test_gpu_vjp.rows_nearest at sigma = 0.42, and
    two_wells with the shallow well on twist targets and sigma a third of the way from the second eigenvalue to the first, so that
    the returned mode (index 1) sits on the chosen target while lam_max sits elsewhere"""
    th = ec.theta_grid(N)
    h = float(th[1] - th[0])
    t = ec.twist_targets(N)
    targets = t[:2] + ([] if N > 60000 else t[2:6]) + ([t[-1]] if len(t) > 2 else [])
    g1, c1 = bo.salpha_gc(th, 1.0, 0.8, 0.0)
    rows, sig = [(g1, 4.0 * c1, g1.copy())], [0.42]
    for js in targets:
        rw = ec.two_wells(th, shallow_partner(N, js), js)
        w = ec.top_pairs(th, *rw)[0]
        rows.append(rw); sig.append(w[0] + (w[1] - w[0]) / 3.0)
    g, c, f = (np.stack([rw[i] for rw in rows]) for i in range(3))
    sig = np.array(sig)
    # (the full spectrum takes minutes per system at 65,535 points: there the eigenvalues above sigma - 0.25 alone; the two references
    #  are held against each other in tests/test_edge_cases_cpu.py)
    nearest = dense_nearest if N <= 4096 else (lambda *a: window_nearest(*a, radius=0.25))
    import time
    t_ref = time.time()
    refs = [nearest(th, g[k], c[k], f[k], sig[k]) for k in range(len(rows))]
    t_ref, t_gpu = time.time() - t_ref, time.time()
    assert refs[0]["idx"] >= 1 and all(rf["idx"] == 1 and not rf["tie"] for rf in refs[1:])
    r = ctx.solve_gcf_nearest(h, g, c, f, sig, want_X=True, want_info=True)
    assert "ibs::k_solve_gcf_nearest<" in ctx.last_launch()[0], ctx.last_launch()
    note("solve_gcf_nearest_f64 (%d systems)" % len(rows), N, ctx)
    assert r["nbad"] == 0
    assert ((r["info"] >> 16) == 0).all(), (N, r["info"] >> 16)
    geo = [np.stack(x) for x in zip(*[ec.to_geometry(g[k], c[k], f[k]) for k in range(len(rows))])]
    rs = ctx.gamma_scan_nearest(h, *geo, np.full(len(rows), -1.0), np.array([0.0]), sig[:, None], want_info=True)
    note("gamma_scan_nearest_f64", N, ctx)
    print("edge-case figures: N=%d nearest sigma: reference %.1f s, the two GPU calls %.1f s" % (N, t_ref, time.time() - t_gpu))
    assert rs["nbad"] == 0 and ((rs["info"] >> 16) == 0).all(), (N, rs["info"] >> 16)
    for k, rf in enumerate(refs):
        assert r["idx"][k] == rf["idx"] and rs["idx"][k, 0] == rf["idx"], (N, k, r["idx"][k], rs["idx"][k, 0], rf["idx"])
        check_pair(N, "nearest %d" % k, r["lam"][k], r["gam"][k], r["X"][k], r["dX"][k], (rf["gam"], rf["lam"], rf["X"], rf["dX"]), rf["nA"])
        assert abs(rs["lam"][k, 0] - rf["lam"]) <= 4 * N * EPS * rf["nA"] and abs(rs["gam"][k, 0] - rf["gam"]) < tol_gam(N), (N, k)
        if k >= 1:
            js, kk = targets[k - 1], int(np.argmax(np.abs(r["X"][k])))
            assert (min(kk, N - 1 - kk) <= 6) if ec.is_end_target(N, js) else (kk == js), (N, js, kk)
            assert abs(rf["lam_max"] - rf["lam"]) > 0.05


# ------------------------------------------------------------------------------------------------ 8. VJP
@pytest.mark.parametrize("N", [67, 2049, 2051, 2305, 2307, 2313, 3075])
def test_vjp_with_the_twist_row_on_chunk_edges(ctx, N):
    """ibs_solve_gcf_vjp_f64 on the moving well at every twist target, gam_bar and lam_bar, against the bordered-system restatement.
    The kernel twists at the row of largest |X| of the X it is given: that row is checked on the host, on the GPU's own X."""
    targets = ec.twist_targets(N)
    th, (g, c, f) = well_batch(N, targets)
    h = float(th[1] - th[0])
    r = ctx.solve_gcf(h, g, c, f, want_X=True, want_info=True)
    clean(r["info"], N, no_reclose=not is_short(N))
    for k, j in enumerate(targets):
        kk = int(np.argmax(np.abs(r["X"][k])))
        assert (min(kk, N - 1 - kk) <= 6) if ec.is_end_target(N, j) else (kk == j), (N, j, kk)
    worst = 0.0
    for gb, lb in ((1.0, None), (None, 1.0)):
        v = ctx.solve_gcf_vjp(h, g, c, f, r["lam"], r["X"], gam_bar=gb, lam_bar=lb, want_info=True)
        assert ctx.last_launch()[0] == "ibs::k_solve_gcf_vjp", ctx.last_launch()
        assert v["nbad"] == 0 and not (v["info"] >> 16).any(), (N, v["info"] >> 16)
        for k, j in enumerate(targets):
            ref = vo.gcf_vjp(th, g[k], c[k], f[k], r["lam"][k], r["X"][k], gam_bar=gb or 0.0, lam_bar=lb or 0.0)
            err = max(np.linalg.norm(got - rf) / np.linalg.norm(rf) for got, rf in zip((v["g_bar"][k], v["c_bar"][k], v["f_bar"][k]), ref))
            worst = max(worst, err)
            assert err <= 1e-9, (N, j, gb, lb, err)
    note("solve_gcf_vjp_f64 (%d targets, worst row error %.1e)" % (len(targets), worst), N, ctx)


# ------------------------------------------------------------------------------------------------ 9. Sturm count
@pytest.mark.parametrize("N", COUNT + SHORT + LONG)
def test_sturm_count_in_every_form(ctx, N):
    """ibs_sturm_count_f64 in each form that is legal at the length (1: prefix-product sweep, N <= 2050; 2: division form, lanes as
    systems; 3: division form, one wave per system; 0: by size), batches of 3 and of 70 (both sides of the n_sys >= 64 switch of long
    grids), shifts at 0 and at lam +- 4 N eps ||A||: exact against the oracle's division-form count"""
    M = ec.rows_per_lane(N)
    kernels = {1: "ibs::k_sturm_count<double, %d>" % M, 2: "ibs::k_sturm_count_div", 3: "ibs::k_sturm_count_long"}
    try:
        for n in (3, 70):
            th, g, c, f = salpha_rows(N, n - 1, seed=9)
            gw, cw, fw = ec.well_rows(th, ec.twist_targets(N)[-1])
            g, c, f = np.vstack([g, gw[None]]), np.vstack([c, cw[None]]), np.vstack([f, fw[None]])
            h = float(th[1] - th[0])
            lam = co.lam_batch(h, g, c, f)
            tol = 4 * N * EPS * ec.norm_a(h, g, c, f)
            for shift, what in ((np.zeros(n), "0"), (lam + tol, "lam + tol"), (lam - tol, "lam - tol")):
                want = co.count_above_batch(h, g, c, f, shift)
                if what == "lam + tol":
                    assert (want == 0).all()
                elif what == "lam - tol":
                    assert (want >= 1).all()
                for form in ([0, 1] if is_short(N) else [0]) + [2, 3]:
                    ctx.set_option("sturm_form", form if form else None)
                    got = ctx.sturm_count(h, g, c, f, shift)
                    name = ctx.last_launch()[0]
                    assert name == kernels[form or (1 if is_short(N) else (2 if n >= 64 else 3))], (N, n, form, name)
                    assert np.array_equal(got, want), (N, n, form, what, np.nonzero(got != want)[0][:8], got[got != want][:8], want[got != want][:8])
                    if what == "0":
                        note("sturm_count_f64 form %d, %d systems" % (form, n), N, name=name)
    finally:
        ctx.set_option("sturm_form", None)
