"""GPU: spectrum mode (ibs_solve_gcf_modes_f64 / ibs_gamma_scan_modes_f64, Context.solve_gcf_modes / gamma_scan_modes, the autograd
function and BallooningScan.modes): the K largest eigenpairs of every system against the CPU reference of tests/modes_oracle.py.
Tolerances: eigenvalues to tau = 4 N eps ||A||; growth rates and vectors (up to sign) of unclustered modes to max(1e-8, 64 eps ||A|| /
gap), gap = the distance to the nearer neighbouring eigenvalue, and dX to the same bar as X (the one tolerance the vectors have; dX is
a difference formula of X whose coefficients sum to 4 / h in magnitude at most, so the bar asks the errors of neighbouring entries of X
to cancel as they do for a smooth error; the ratio actually seen is printed); the cluster bit required where the reference gap is
below tau / 2, forbidden above 2 tau; clustered modes held to lam and the residual bound of ibs_solve_gcf_vjp_f64."""
import os
import warnings

import numpy as np
import pytest

from oracle import ballooning_oracle as bo
from tests import modes_oracle as mo
from tests.test_gpu_nearest_sigma import host_gcf, salpha_geometry, x_diff

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = mo.EPS
CL = mo.CLUSTER_BIT
DPS = (-1.0, -4.0, -8.0)
_REF = {}
WORST_DX = [0.0]      # the largest |dX - dX_ref| / vec_tol seen (printed; the bound is 1)


@pytest.fixture(scope="module")
def ctx():
    import ibs_amd
    c = ibs_amd.Context(0)
    yield c
    c.close()


def salpha_ref(N, dP, K=16):
    """the line and its reference modes, computed once per (N, dPdrho) for the largest K and shared"""
    key = (N, dP)
    if key not in _REF:
        line = mo.salpha_line(N, dP)
        _REF[key] = (line, mo.dense_modes(*line, K))
    return _REF[key]


def stack(rows):
    return tuple(np.stack([r[k] for r in rows]) for k in range(3))


def check_system(tag, r, i, ref, K, line):
    """system i of the result r against the first K modes of ref"""
    th, g, c, f = line
    info = r["info"][i]
    status = info >> 16
    assert (status & 3 == 0).all() and len(set(info & 0xffff)) == 1 and 0 < (info[0] & 0xffff) <= 33, (tag, info)
    assert np.abs(r["lam"][i] - ref["lam"][:K]).max() <= ref["tau"], (tag, r["lam"][i], ref["lam"][:K], ref["tau"])
    need, never = (x[:K] for x in mo.cluster_rule(ref))
    bit = (status & CL) != 0
    assert bit[need].all() and not bit[never].any(), (tag, bit, ref["gap"][:K] / ref["tau"])
    for m in range(K):
        if bit[m] or need[m]:
            ok, res, bound = mo.residual_ok(th, g, c, f, r["lam"][i, m], r["X"][i, m])
            assert ok, (tag, m, res, bound)
            continue
        tol = max(1e-8, 64 * EPS * ref["nA"] / ref["gap"][m])
        assert abs(r["gam"][i, m] - ref["gam"][m]) <= tol, (tag, m, r["gam"][i, m], ref["gam"][m], tol)
        X, dX = r["X"][i, m], r["dX"][i, m]
        assert abs(X.max() - 1.0) <= 4 * EPS and np.abs(X).max() <= 1.0 + 4 * EPS and X[0] == 0 and X[-1] == 0, (tag, m)
        s = 1.0 if np.abs(X - ref["X"][m]).max() <= np.abs(X + ref["X"][m]).max() else -1.0
        assert np.abs(X - s * ref["X"][m]).max() <= tol, (tag, m, x_diff(X, ref["X"][m]), tol)
        assert np.abs(dX - s * ref["dX"][m]).max() <= tol, (tag, m, np.abs(dX - s * ref["dX"][m]).max(), tol)
        WORST_DX[0] = max(WORST_DX[0], np.abs(dX - s * ref["dX"][m]).max() / tol)


@pytest.mark.parametrize("N", [67, 769, 771, 2051, 2561, 4097])
def test_salpha_lines(ctx, N):
    """shat = 1, alpha = 0.8, dPdrho in {-1, -4, -8}, f = g, K in {1, 2, 8, 16} (N = 4,097: one system, dPdrho = -4): lam, gam, X, dX and
    info against the reference; the gaps among the top nine are >= 4e3 tau (checked), so none of the top eight may carry the cluster
    bit; mode 0 is Context.solve_gcf's pair (lam to tau, gam to 1e-8)"""
    dps, Ks = (DPS if N != 4097 else (-4.0,)), (1, 2, 8, 16)    # (dPdrho = -8 at N = 4,097: modes 3 and 4 are 1.2e3 tau apart)
    refs = [salpha_ref(N, dP, max(Ks)) for dP in dps]
    g, c, f = stack([line[1:] for line, _ in refs])
    h = refs[0][0][0][1] - refs[0][0][0][0]
    base = ctx.solve_gcf(h, g, c, f)
    for (line, ref), dP in zip(refs, dps):
        w = ref["w"]
        assert (w[:8] - w[1:9]).min() >= 4e3 * ref["tau"], (N, dP)
        assert int((w > 0).sum()) == {-1.0: 1, -4.0: 4, -8.0: 5}[dP], (N, dP, w[:8])
    for K in Ks:
        r = ctx.solve_gcf_modes(h, g, c, f, K, want_X=True, want_info=True)
        assert r["nbad"] == 0 and r["lam"].shape == (len(dps), K) and r["X"].shape == (len(dps), K, N)
        assert not ((r["info"][:, :8] >> 16) & CL).any(), (N, K, r["info"] >> 16)
        for i, (line, ref) in enumerate(refs):
            check_system((N, dps[i], K), r, i, ref, K, line)
            assert abs(r["lam"][i, 0] - base["lam"][i]) <= ref["tau"] and abs(r["gam"][i, 0] - base["gam"][i]) <= 1e-8
    print("N=%d passes per system, K=%s: %s; worst |dX - dX_ref| / vec_tol so far %.3g (bound 1)"
          % (N, Ks[-1], (r["info"][:, 0] & 0xffff).tolist(), WORST_DX[0]))


@pytest.mark.parametrize("N", [131, 513])
def test_double_well(ctx, N):
    """g = f = 1, c = 8 (exp(-(theta - 8)^2) + exp(-(theta + 8)^2)) - 0.5: modes (0, 1) are an even / odd doublet far inside tau / 2,
    modes (2, 3) far outside 2 tau (both checked on the reference): the bit is required on 0 and 1, forbidden on 2 and 3; the
    clustered modes hold lam and the residual bound.  Mixed with s-alpha systems inside one launch."""
    K = 4
    well = mo.double_well(N)
    ref = mo.dense_modes(*well, K)
    need, never = mo.cluster_rule(ref)
    assert need.tolist() == [True, True, False, False] and never.tolist() == [False, False, True, True], ref["gap"] / ref["tau"]
    others = [(line, mo.dense_modes(*line, K)) for line in (mo.salpha_line(N, dP) for dP in (-4.0, -8.0))]
    systems = [others[0], (well, ref), others[1], (well, ref)]
    g, c, f = stack([line[1:] for line, _ in systems])
    r = ctx.solve_gcf_modes(well[0][1] - well[0][0], g, c, f, K, want_X=True, want_info=True)
    assert r["nbad"] == 0
    for i, (line, rf) in enumerate(systems):
        check_system((N, i), r, i, rf, K, line)
    st = r["info"] >> 16
    assert ((st[1] & CL) != 0).tolist() == [True, True, False, False] and not (st[0] & CL).any() and not (st[2] & CL).any()
    for k in ("lam", "gam", "X", "dX", "info"):
        assert np.array_equal(r[k][1], r[k][3]), k


def test_persistent_loop_and_batch_independence(ctx):
    """3,000 copies of eight N = 67 systems in a fixed pseudo-random order -- more systems than the grid has waves --: every result
    bitwise equal to that of the eight solved alone"""
    N, K = 67, 4
    rows = [mo.salpha_line(N, dP, shat=sh, alpha=al)[1:] for dP in (-1.0, -8.0) for sh, al in ((1.0, 0.8), (0.5, 0.6), (1.5, 1.0), (0.8, 0.3))]
    g, c, f = stack(rows)
    h = bo.theta_grid(N)[1] - bo.theta_grid(N)[0]
    alone = ctx.solve_gcf_modes(h, g, c, f, K, want_X=True, want_info=True)
    pick = np.random.default_rng(67).integers(0, 8, 3000)
    big = ctx.solve_gcf_modes(h, g[pick], c[pick], f[pick], K, want_X=True, want_info=True)
    assert big["nbad"] == 0 and ctx.last_launch()[1] < 3000
    for k in ("lam", "gam", "X", "dX", "info"):
        assert np.array_equal(big[k], alone[k][pick]), k


def test_half_grid_g_and_invalid_data(ctx):
    """gh supplied (HAS_GH) on a system regridded from a non-uniform grid as gamma_ball_full regrids it (utils.py:1567-1576), against
    the reference on the non-uniform grid; a system with a NaN and one with f <= 0 among good ones: status bit 1 and NaN on all
    their modes, the neighbours bitwise untouched"""
    N, K = 131, 3
    tu = bo.theta_grid(N)
    th = tu + 0.35 * np.sin(tu / 4) * (tu[1] - tu[0])                   # non-uniform, same end points
    gq, c0 = bo.salpha_gc(th, 1.0, 0.8, 0.0)
    cq, fq = 8.0 * c0, gq.copy()
    ref = mo.dense_modes(th, gq, cq, fq, K)
    _, gu, cu, fu = bo.regrid_uniform(th, gq, cq, fq)
    th_half = (tu[:-1] + tu[1:]) / 2
    h = np.diff(th_half)[2]
    gh = np.zeros(N)
    gh[:-1] = np.interp(th_half, th, gq)
    r = ctx.solve_gcf_modes(h, gu[None], cu[None], fu[None], K, gh=gh[None], want_X=True, want_info=True)
    assert r["nbad"] == 0 and not (r["info"] >> 16).any()
    assert np.abs(r["lam"][0] - ref["lam"]).max() <= ref["tau"]
    for m in range(K):
        tol = max(1e-8, 64 * EPS * ref["nA"] / ref["gap"][m])
        assert abs(r["gam"][0, m] - ref["gam"][m]) <= tol and x_diff(r["X"][0, m], ref["X"][m]) <= tol, (m, tol)
    plain = ctx.solve_gcf_modes(h, gu[None], cu[None], fu[None], K)
    assert np.abs(plain["lam"] - r["lam"]).max() > 100 * ref["tau"]         # (the half-grid g is really read)
    rows = [mo.salpha_line(N, dP)[1:] for dP in (-1.0, -4.0, -8.0, -2.0, -6.0)]
    g, c, f = stack(rows)
    h = tu[1] - tu[0]
    clean = ctx.solve_gcf_modes(h, g, c, f, K, want_X=True, want_info=True)
    assert clean["nbad"] == 0
    c_bad, f_bad = c.copy(), f.copy()
    c_bad[1, 40] = np.nan
    f_bad[3, 100] = 0.0
    r = ctx.solve_gcf_modes(h, g, c_bad, f_bad, K, want_X=True, want_info=True)
    assert r["nbad"] == 2 * K
    for i in range(5):
        if i in (1, 3):
            assert ((r["info"][i] >> 16) & 3 == 2).all() and np.isnan(r["lam"][i]).all() and np.isnan(r["gam"][i]).all()
            assert np.isnan(r["X"][i]).all() and np.isnan(r["dX"][i]).all()
        else:
            for k in ("lam", "gam", "X", "dX", "info"):
                assert np.array_equal(r[k][i], clean[k][i]), (i, k)


def test_argument_errors(ctx):
    import ibs_amd
    z = np.ones((1, 67))
    for K in (0, 17, -1, 2.5):
        with pytest.raises(ibs_amd.IbsError):
            ctx.solve_gcf_modes(0.05, z, z, z, K)
    for N in (512, 33, 65539):
        z = np.ones((1, N))
        with pytest.raises(ibs_amd.IbsError):
            ctx.solve_gcf_modes(0.05, z, z, z, 2)
        with pytest.raises(ibs_amd.IbsError):
            ctx.gamma_scan_modes(0.05, z, z, z, z, z, z, z, np.array([-1.0]), np.zeros(1), 2)
    lib, p = ctx._lib, z.ctypes.data
    assert lib.ibs_solve_gcf_modes_f64(ctx._h, 1, 67, 0.05, p, None, p, p, 67, 0, p, None, None, None, None, 1) == -1     # IBS_ERR_ARG
    assert lib.ibs_solve_gcf_modes_f64(ctx._h, 1, 67, 0.05, p, None, p, p, 67, 17, p, None, None, None, None, 1) == -1
    assert lib.ibs_solve_gcf_modes_f64(ctx._h, 1, 67, 0.05, p, None, p, p, 67, 2, None, None, None, None, None, 1) == -1  # no output


def test_scan_entry(ctx):
    """the s-alpha family as geometry arrays, 5 lines x 3 theta0, N = 131, K = 4: against the reference on the host-assembled rows, and
    bitwise against itself with "nearest_chunk_systems" = 6 (chunks of 2, 2 and 1 lines)"""
    N, K = 131, 4
    th, geo = salpha_geometry(N, 5)
    dP = np.array([-4.0, -8.0, -6.0, -1.0, -5.0])
    theta0 = np.array([0.0, 0.4, 1.1])
    h = th[1] - th[0]
    args = [np.ascontiguousarray(geo[:, k]) for k in range(7)]
    r = ctx.gamma_scan_modes(h, *args, dP, theta0, K, want_info=True)
    assert r["nbad"] == 0 and r["lam"].shape == (5, 3, K) and r["info"].dtype == np.int32
    for i in range(5):
        for j, t0 in enumerate(theta0):
            g, c, f = host_gcf(geo[i], dP[i], t0)
            ref = mo.dense_modes(th, g, c, f, K)
            assert np.abs(r["lam"][i, j] - ref["lam"]).max() <= ref["tau"], (i, j)
            need, never = mo.cluster_rule(ref)
            bit = ((r["info"][i, j] >> 16) & CL) != 0
            assert bit[need].all() and not bit[never].any() and not ((r["info"][i, j] >> 16) & 3).any()
            for m in range(K):
                if not bit[m]:
                    tol = max(1e-8, 64 * EPS * ref["nA"] / ref["gap"][m])
                    assert abs(r["gam"][i, j, m] - ref["gam"][m]) <= tol, (i, j, m, r["gam"][i, j, m], ref["gam"][m], tol)
    ctx.set_option("nearest_chunk_systems", 6)
    try:
        r2 = ctx.gamma_scan_modes(h, *args, dP, theta0, K, want_info=True)
    finally:
        ctx.set_option("nearest_chunk_systems", None)
    for k in ("gam", "lam", "info"):
        assert np.array_equal(r[k], r2[k]), k


def test_autograd(ctx):
    """N = 131, 3 systems, K = 3: gam[:, 2].sum() + lam[:, 1].sum() backpropagated, its directional derivative against central
    differences of the CPU reference (tests/test_gpu_vjp.py's steps and bars: gam step 1e-6 to 1e-6, lam by Richardson of 4e-4 and
    2e-4 to 1e-5); on the double well a cotangent on a clustered mode gives NaN rows and a VjpStatusWarning, a zero one nothing"""
    import torch
    import ibs_amd
    from ibs_amd import autograd as iag
    from tests import vjp_oracle as vo
    dev = torch.device("cuda:0")
    N, K = 131, 3
    lines = [mo.salpha_line(N, dP) for dP in (-4.0, -8.0, -6.0)]
    th = lines[0][0]
    h = th[1] - th[0]
    G_, C_, F_ = stack([ln[1:] for ln in lines])
    rng = np.random.default_rng(131)
    dG = np.stack([vo.smooth_direction(rng, th, 0.1 * G_[k]) for k in range(3)])
    dC = np.stack([vo.smooth_direction(rng, th, 0.1 * np.abs(C_[k]).max()) for k in range(3)])
    dF = np.stack([vo.smooth_direction(rng, th, 0.1 * F_[k]) for k in range(3)])
    g, c, f = (torch.from_numpy(a).to(dev).requires_grad_(True) for a in (G_, C_, F_))
    gam, lam = iag.solve_gcf_modes(h, g, c, f, K, ctx=ctx)
    assert gam.shape == (3, K) and lam.shape == (3, K)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        (gam[:, 2].sum() + lam[:, 1].sum()).backward()
    an = ((g.grad.cpu().numpy() * dG).sum(1) + (c.grad.cpu().numpy() * dC).sum(1) + (f.grad.cpu().numpy() * dF).sum(1))

    def ref_at(k, t):
        return mo.dense_modes(th, G_[k] + t * dG[k], C_[k] + t * dC[k], F_[k] + t * dF[k], K)

    for k in range(3):
        central = lambda key, m, t: (ref_at(k, t)[key][m] - ref_at(k, -t)[key][m]) / (2 * t)
        fd_gam = central("gam", 2, 1e-6)
        fd_lam = (4 * central("lam", 1, 2e-4) - central("lam", 1, 4e-4)) / 3
        tol = 1e-6 * abs(fd_gam) + 1e-5 * abs(fd_lam)
        print("system %d: analytic %.12g, central differences %.12g + %.12g, tolerance %.3g" % (k, an[k], fd_gam, fd_lam, tol))
        assert abs(an[k] - (fd_gam + fd_lam)) <= tol, (k, an[k], fd_gam, fd_lam, tol)
    # the double well between two s-alpha systems: modes 0 and 1 are clustered
    well = mo.double_well(N)
    G2, C2, F2 = stack([lines[0][1:], well[1:], lines[1][1:]])
    for col, refused in ((2, False), (1, True)):
        g, c, f = (torch.from_numpy(a).to(dev).requires_grad_(True) for a in (G2, C2, F2))
        gam, lam = iag.solve_gcf_modes(h, g, c, f, K, ctx=ctx)
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            gam[:, col].sum().backward()
        rows = [x.grad.cpu().numpy() for x in (g, c, f)]
        assert bool([x for x in w if issubclass(x.category, ibs_amd.VjpStatusWarning)]) == refused, [str(x.message) for x in w]
        for a in rows:
            assert np.isnan(a[1]).all() == refused and np.isfinite(a[0]).all() and np.isfinite(a[2]).all()
            assert refused or np.isfinite(a[1]).all()
            assert np.abs(a[0]).max() > 0


def test_scan_driver_modes(ctx):
    """BallooningScan.modes(3) on the NCSX tables of the mode_count test (pressure x 6, N = 513, 2 surfaces x 8 alpha x 5 theta0): the
    number of modes with lam > 0 among the three equals min(3, mode_count()); the eigenvalues descend"""
    import torch
    import ibs_amd
    from tests.test_gpu_certify import KW, SVALS, wout_scaled
    dev = torch.device("cuda:0")
    N = 513
    th = np.linspace(-4 * np.pi, 4 * np.pi, N)
    tabs = ibs_amd.SurfaceTables.from_wout(wout_scaled(6.0), SVALS)
    sc = ibs_amd.BallooningScan(ctx, None, th, SVALS, tables=tabs, device=dev, **KW)
    md = sc.modes(3)
    cnt = sc.mode_count()
    assert md["lam"].shape == (2, 8, 5, 3) and md["gam"].shape == (2, 8, 5, 3) and md["cluster"].dtype == bool
    assert np.array_equal((md["lam"] > 0).sum(-1), np.minimum(3, cnt)), ((md["lam"] > 0).sum(-1), cnt)
    assert cnt.max() >= 1 and (np.diff(md["lam"], axis=-1) <= 0).all()
    with pytest.raises(ibs_amd.IbsError):
        sc.modes(17)
