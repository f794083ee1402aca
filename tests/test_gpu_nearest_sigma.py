"""GPU: the eigenpair NEAREST sigma (ibs_solve_gcf_nearest_f64 / ibs_gamma_scan_nearest_f64 and the drop-in's eigenpair="nearest"):
what the reference's eigs(A, 1, sigma=sigma0) returns (utils.py:1597), against a CPU restatement built here from the oracle's public
pieces -- the pencil rows of bo.assemble, its full spectrum in the symmetric form bo.top_eigenpair uses (scipy eigh_tridiagonal), the
nearest eigenvalue, its vector (select="i"), the sign that makes the largest |x| positive, bo.rayleigh_growth."""
import os
import warnings

import numpy as np
import pytest

from oracle import ballooning_oracle as bo

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
EPS = 2.220446049250313e-16


@pytest.fixture(scope="module")
def ctx():
    import ibs_amd
    c = ibs_amd.Context(0)
    yield c
    c.close()


def spectrum(th, g, c, f):
    """(ascending eigenvalues, (a, b) of the symmetric form, fd, h, gu, cu, fu, ||A||) of the pencil of utils.py:1574-1592"""
    from scipy.linalg import eigh_tridiagonal
    d, e, fd, h, gu, cu, fu = bo.assemble(th, g, c, f)
    n = len(d)
    a = d / fd
    b = e[1:n] / np.sqrt(fd[:-1] * fd[1:])
    w = eigh_tridiagonal(a, b, eigvals_only=True)
    nA = float(((np.abs(d) + e[:-1] + e[1:]) / fd).max())
    return w, (a, b), fd, h, gu, cu, fu, nA


def ref_nearest(th, g, c, f, sigma):
    """the eigenpair nearest sigma; distances within 4 N eps ||A|| of each other: the larger eigenvalue, tie=True"""
    from scipy.linalg import eigh_tridiagonal
    w, (a, b), fd, h, gu, cu, fu, nA = spectrum(th, g, c, f)
    n, N = len(w), len(g)
    tau = 4 * N * EPS * nA
    dist = np.abs(w - min(max(sigma, w[0] - 1.0), w[-1] + 1.0))     # (the same order; |w - 1e300| would be 1e300 for every w)
    order = np.argsort(dist, kind="stable")
    j, tie = int(order[0]), False
    if n > 1 and dist[order[1]] - dist[j] < tau:
        j, tie = max(j, int(order[1])), True
    gap = min(w[j] - w[j - 1] if j > 0 else np.inf, w[j + 1] - w[j] if j < n - 1 else np.inf)
    _, v = eigh_tridiagonal(a, b, select="i", select_range=(j, j))
    x = v[:, 0] / np.sqrt(fd)
    if x[np.argmax(np.abs(x))] < 0:
        x = -x
    gam, X, dX = bo.rayleigh_growth(x, h, gu, cu, fu)
    return dict(lam=float(w[j]), idx=n - 1 - j, gam=gam, X=X, dX=dX, gap=gap, nA=nA, tie=tie, w=w)


def x_diff(X, Xref):
    """max |X - Xref| up to the sign: an eigenvector's sign is arbitrary (ARPACK's upstream), and where the largest |x| is taken at
    two points at once -- the odd modes of a symmetric line -- "largest entry positive" does not fix it either"""
    X, Xref = np.asarray(X), np.asarray(Xref)
    return float(min(np.abs(X - Xref).max(), np.abs(X + Xref).max()))


def vec_tol(r):
    return max(1e-8, 64 * EPS * r["nA"] / r["gap"])


def salpha_line(N, dPdrho, shat=1.0, alpha=0.8, theta0=0.0):
    th = bo.theta_grid(N)
    g, c0 = bo.salpha_gc(th, shat, alpha, theta0)
    return th, g, -dPdrho * c0, g.copy()


def test_worked_case_matches_upstream(ctx):
    """ISSUE table: s-alpha, shat = 1, alpha = 0.8, N = 257 -- the line of test_nearest_sigma_divergence_is_reported.  With
    eigenpair="nearest" the drop-in returns what upstream's formulation (dense matrix + ARPACK shift-invert) returns, with the
    index of the eigenvalue, and warns about nothing."""
    import ibs_amd
    N = 257
    th = bo.theta_grid(N)
    g, c0 = bo.salpha_gc(th, 1.0, 0.8, 0.0)
    one = np.ones(N)
    for dP, want_idx in ((-4.0, 1), (-8.0, 2)):
        for sigma0 in (0.42, 1.0):
            info = {}
            with warnings.catch_warnings(record=True) as w:
                warnings.simplefilter("always")
                out = ibs_amd.gamma_ball_full(dP, th, one, one, c0, g, sigma0=sigma0, ctx=ctx, info=info, eigenpair="nearest")
            assert not w, [str(x.message) for x in w]
            ref = bo.gamma_ball_full_dense_arpack(dP, th, one, one, c0, g, sigma0=sigma0)
            assert abs(out[0] - ref[0]) < 1e-8, (dP, sigma0, out[0], ref[0])
            assert info["idx"] == want_idx and (info["status"] & 3) == 0, (dP, sigma0, info)
            assert info["lam"] < 0.5 and info["sweeps"] > 0
            # the other outputs of utils.py:1624: the eigenfunction up to its sign, and the coefficients
            assert x_diff(out[1], ref[1]) < 1e-5
            assert np.abs(out[3] - ref[3]).max() == 0 and np.abs(out[4] - ref[4]).max() < 1e-15 * np.abs(ref[4]).max()


@pytest.mark.parametrize("N", [257, 513, 1025, 2049, 4097])
def test_raw_systems_across_the_spectrum(ctx, N):
    """s-alpha lines, dPdrho in {-1, -4, -8}: shifts below lam_min, on either side of a close pair, midway between two eigenvalues
    (undecided: bit 5, the larger returned), at 0.42 and 1.0 and above the Gershgorin bound -- idx, lam, gam and X against the CPU
    reference (eigenvalues to 4 N eps ||A||, vectors and growth rates to max(1e-8, 64 eps ||A|| / gap))."""
    rows, shifts, refs = [], [], []
    for dP in (-1.0, -4.0, -8.0):
        th, g, c, f = salpha_line(N, dP)
        w = spectrum(th, g, c, f)[0]
        top = w[::-1][:8]
        k = int(np.argmin(top[:-1] - top[1:]))                  # the closest adjacent pair among the top eigenvalues
        hi_, lo_ = top[k], top[k + 1]
        gp = hi_ - lo_
        gersh = float((c[1:-1] / f[1:-1]).max()) + 1.0
        cand = [w[0] - 1.0, hi_ + 0.25 * gp, lo_ - 0.25 * gp, 0.5 * (top[0] + top[1]), 0.42, 1.0, gersh, 1e300]
        for s in cand:
            rows.append((g, c, f)); shifts.append(s); refs.append(ref_nearest(th, g, c, f, s))
    h = bo.theta_grid(N)[1] - bo.theta_grid(N)[0]
    gg, cc, ff = (np.stack([r[i] for r in rows]) for i in range(3))
    r = ctx.solve_gcf_nearest(h, gg, cc, ff, np.array(shifts), want_X=True, want_info=True)
    assert r["nbad"] == 0
    st = r["info"] >> 16
    for i, ref in enumerate(refs):
        tol_l = 4 * N * EPS * ref["nA"]
        assert r["idx"][i] == ref["idx"], (i, shifts[i], r["idx"][i], ref["idx"], r["lam"][i], ref["lam"])
        assert abs(r["lam"][i] - ref["lam"]) <= tol_l, (i, r["lam"][i], ref["lam"], tol_l)
        assert bool(st[i] & 32) == ref["tie"], (i, shifts[i], st[i], ref["tie"])
        tv = vec_tol(ref)
        assert abs(r["gam"][i] - ref["gam"]) <= tv, (i, r["gam"][i], ref["gam"], tv)
        assert x_diff(r["X"][i], ref["X"]) <= tv, (i, x_diff(r["X"][i], ref["X"]), tv)
    # the midway shifts (index 3 of every line's eight) are the undecided ones
    assert all(st[3 + 8 * m] & 32 for m in range(3))


@pytest.mark.parametrize("N", [513, 1025])
def test_certified_on_a_large_rough_batch(ctx, N):
    """2^16 systems of the rough family, sigma uniform in [lam_min, lam_max] per system.  With the library's exact division-form
    counts: idx eigenvalues above lam + t, idx + 1 above lam - t (t = 4 N eps ||A||); and none nearer to sigma than lam
    (count(sigma - |lam - sigma| + t') == count(sigma + |lam - sigma| - t'), t' = 8 N eps ||A||) unless bit 5 says undecided.
    A sample of 128 systems against the CPU reference."""
    import torch
    import bench
    dev = torch.device("cuda:0")
    n = 1 << 16
    h, g, c, f = bench.c5_family(dev, "rough", n, N, 20260 + N)
    nA = bench.norm_a(h, g, c, f)
    lmax = ctx.solve_gcf(h, g, c, f)["lam"]
    lmin = ctx.solve_gcf_nearest(h, g, c, f, -1e300)["lam"]
    gen = torch.Generator(device=dev); gen.manual_seed(7 + N)
    sig = lmin + (lmax - lmin) * torch.rand(n, dtype=torch.float64, device=dev, generator=gen)
    r = ctx.solve_gcf_nearest(h, g, c, f, sig, want_info=True)
    torch.cuda.synchronize()
    st = (r["info"] >> 16)
    assert int(((st & 3) != 0).sum()) == 0
    lam, idx = r["lam"], r["idx"]
    t = 4 * N * EPS * nA
    assert torch.equal(ctx.sturm_count(h, g, c, f, lam + t, exact=True), idx)
    assert torch.equal(ctx.sturm_count(h, g, c, f, lam - t, exact=True), idx + 1)
    t2 = 8 * N * EPS * nA
    d = (lam - sig).abs()
    a = ctx.sturm_count(h, g, c, f, sig - d + t2, exact=True)
    b = ctx.sturm_count(h, g, c, f, sig + d - t2, exact=True)
    decided = (st & 32) == 0
    assert torch.equal(a[decided], b[decided]), int((a != b)[decided].sum())
    th = bo.theta_grid(N)
    pick = np.random.default_rng(N).choice(n, 128, replace=False)
    rs = ctx.solve_gcf_nearest(h, g[pick], c[pick], f[pick], sig[pick], want_X=True)
    G_, C_, F_, S_ = (x[pick].cpu().numpy() for x in (g, c, f, sig))
    for k in range(128):
        ref = ref_nearest(th, G_[k], C_[k], F_[k], S_[k])
        assert int(rs["idx"][k]) == ref["idx"] or ref["tie"], (k, int(rs["idx"][k]), ref["idx"])
        if ref["tie"]:
            continue
        assert abs(float(rs["lam"][k]) - ref["lam"]) <= 4 * N * EPS * ref["nA"]
        tv = vec_tol(ref)
        assert abs(float(rs["gam"][k]) - ref["gam"]) <= tv * max(1.0, abs(ref["gam"])), (k, float(rs["gam"][k]), ref["gam"], tv)
        assert x_diff(rs["X"][k].cpu().numpy(), ref["X"]) <= tv


def test_k0_is_the_default_path(ctx):
    """sigma above the Gershgorin bound: the nearest eigenpair IS lam_max's, and solve_gcf_nearest returns what solve_gcf does
    (lam to 4 N eps ||A||; gam to 1e-10 on s-alpha lines, and on the rough family and G10 to the bar of an eigenvector stage,
    max(1e-10, 64 eps ||A|| / gap) x max(1, |gam|) with the gap below lam_max -- the two kernels reach lam_max's vector by different
    routes, and rough coefficients have ||A|| ~ 1e5).  G10 (tests/golden/G10_rough_pair_1025.npz: the top pair 1.5e-10 ||A|| apart)
    gives lam_max, never lam_2; with sigma between lam_2 and lam_1 the nearer of the two comes back."""
    import torch
    import bench
    dev = torch.device("cuda:0")
    cases = []
    for N in (513, 1025):
        th = bo.theta_grid(N)
        rows = [salpha_line(N, dP, shat=sh, alpha=al)[1:] for dP in (-1.0, -4.0) for sh, al in ((1.0, 0.8), (0.5, 0.6))]
        gg, cc, ff = (torch.from_numpy(np.stack([r[i] for r in rows])).to(dev) for i in range(3))
        cases.append((th[1] - th[0], gg, cc, ff, None))
        h, g, c, f = bench.c5_family(dev, "rough", 64, N, 99 + N)
        cases.append((h, g, c, f, th))
    d = np.load(os.path.join(G, "G10_rough_pair_1025.npz"))
    g10 = [torch.from_numpy(d[k][None].copy()).to(dev) for k in ("g", "c", "f")]
    cases.append((8 * np.pi / 1024, *g10, bo.theta_grid(1025)))
    for h, g, c, f, th_gap in cases:
        N = g.shape[1]
        nA = bench.norm_a(h, g, c, f)
        a = ctx.solve_gcf(h, g, c, f)
        b = ctx.solve_gcf_nearest(h, g, c, f, 1e300, want_info=True)
        assert int((b["idx"] != 0).sum()) == 0 and int(((b["info"] >> 16) != 0).sum()) == 0
        assert bool(((a["lam"] - b["lam"]).abs() <= 4 * N * EPS * nA).all()), float((a["lam"] - b["lam"]).abs().max())
        gtol = torch.full_like(a["gam"], 1e-10)
        if th_gap is not None:
            G_, C_, F_ = (x.cpu().numpy() for x in (g, c, f))
            for k in range(len(G_)):
                w, _, _, _, _, _, _, nk = spectrum(th_gap, G_[k], C_[k], F_[k])
                gtol[k] = max(1e-10, 64 * EPS * nk / (w[-1] - w[-2]))
        tol = gtol * torch.clamp(a["gam"].abs(), min=1.0)
        assert bool(((a["gam"] - b["gam"]).abs() <= tol).all()), float((a["gam"] - b["gam"]).abs().max())
    g, c, f = d["g"], d["c"], d["f"]
    th = bo.theta_grid(1025)
    w = spectrum(th, g, c, f)[0]
    l1, l2 = w[-1], w[-2]
    assert abs(l1 - float(d["lam_max"])) < 4 * 1025 * EPS * spectrum(th, g, c, f)[-1]
    r = ctx.solve_gcf_nearest(th[1] - th[0], g[None], c[None], f[None], np.array([l1 - 0.25 * (l1 - l2)]))
    assert int(r["idx"][0]) == 0 and r["lam"][0] > 0.5 * (l1 + l2)
    r = ctx.solve_gcf_nearest(th[1] - th[0], g[None], c[None], f[None], np.array([l2 + 0.25 * (l1 - l2)]))
    assert int(r["idx"][0]) == 1 and r["lam"][0] < 0.5 * (l1 + l2)


def salpha_geometry(N, n_lines):
    """s-alpha lines as the seven geometry arrays of the scan (bishop_ball_s-alpha.py:30-45 written as a field line: B = 1, gradpar = 1)"""
    th = bo.theta_grid(N)
    geo = []
    for i in range(n_lines):
        shat, alpha = 0.6 + 0.2 * i, 0.7 + 0.05 * i
        lam0 = shat * th - alpha * np.sin(th)
        geo.append(np.stack([np.ones(N), np.ones(N), alpha * (np.cos(th) + np.sin(th) * lam0), -alpha * shat * np.sin(th),
                             1 + lam0 ** 2, -shat * lam0, np.full(N, shat ** 2)]))
    return th, np.stack(geo)


def host_gcf(geo7, dP, t0):
    """(g, c, f) of one (line, theta0): ball_scan.py:267-268, utils.py:1560-1562"""
    bmag, gradpar, cvdrift, cvdrift0, gds2, gds21, gds22 = geo7
    cv = cvdrift + t0 * cvdrift0
    gd = gds2 + 2 * t0 * gds21 + t0 ** 2 * gds22
    gp = np.abs(gradpar)
    return gp * gd / bmag, -1 * dP * cv * 1 / (gp * bmag), gd / bmag ** 2 * 1 / (gp * bmag)


def test_scan_entry(ctx):
    """the coarse scan with upstream's shift 1.0 on lines whose lam_max exceeds it (G3 NCSX lines with dPdrho x 50, s-alpha lines
    driven by dPdrho = -4 / -8), 15 theta0: gamma_scan_nearest equals solve_gcf_nearest on the host-assembled (g, c, f) (to 1e-9 in
    gam: the device assembly rounds in another order, so the two solves see rows a few ulp apart), idx and lam alike; forcing at least
    three chunks (option "nearest_chunk_systems") changes no bit; one case at N = 4097."""
    d = np.load(os.path.join(G, "G3_ncsx_lines.npz"))
    theta0 = np.linspace(0.0, np.pi / 2, 15)
    cases = []
    for N in (513, 1025):
        geo = d["geo_%d" % N][:, :7]
        cases.append((bo.theta_grid(N), np.ascontiguousarray(geo), 50.0 * d["dPdrho_%d" % N]))
    th, geo = salpha_geometry(4097, 3)
    cases.append((th, geo, np.array([-4.0, -8.0, -6.0])))
    th, geo = salpha_geometry(513, 4)
    cases.append((th, geo, np.array([-4.0, -8.0, -5.0, -8.0])))
    for th, geo, dP in cases:
        N = geo.shape[-1]
        n_lines = geo.shape[0]
        h = th[1] - th[0]
        args = [np.ascontiguousarray(geo[:, k]) for k in range(7)]
        r = ctx.gamma_scan_nearest(h, *args, dP, theta0, 1.0, want_info=True)
        assert r["nbad"] == 0
        rows = [host_gcf(geo[i], dP[i], t0) for i in range(n_lines) for t0 in theta0]
        gg, cc, ff = (np.stack([x[k] for x in rows]) for k in range(3))
        ref = ctx.solve_gcf_nearest(h, gg, cc, ff, 1.0)
        assert np.array_equal(r["idx"].ravel(), ref["idx"]), (N, r["idx"].ravel(), ref["idx"])
        assert np.abs(r["gam"].ravel() - ref["gam"]).max() < 1e-9 * max(1.0, np.abs(ref["gam"]).max()), (N, np.abs(r["gam"].ravel() - ref["gam"]).max())
        assert (r["idx"] > 0).any(), N                         # (lam_max > 1 somewhere: the case the scan entry exists for)
        ctx.set_option("nearest_chunk_systems", 15 * max(1, n_lines // 3))
        try:
            r2 = ctx.gamma_scan_nearest(h, *args, dP, theta0, np.full((n_lines, 15), 1.0), want_info=True)
        finally:
            ctx.set_option("nearest_chunk_systems", None)
        for k in ("gam", "lam", "idx", "info"):
            assert np.array_equal(r[k], r2[k]), (N, k)


def test_obj_w_grad_nearest(ctx):
    """make_obj_w_grad(..., eigenpair="nearest") on a strongly driven point (synthetic field lines, dPdrho = -8) against a test-local
    restatement of utils.py:1632-1728 with the eigenpair nearest sigma00: value to 1e-8, gradient to 1e-7.  With sigma00 above lam_max
    it is the default (fused, lam_max) objective to 1e-9."""
    import ibs_amd
    from tests.helpers import synthetic_fieldlines
    N = 513
    th = bo.theta_grid(N)
    base = synthetic_fieldlines(th)
    K = 8.0

    def fieldlines(vs, rho, alphas, theta):
        out = base(rho, alphas).copy()
        out[:, 7] = out[:, 2] - 2.0 * K / out[:, 0] ** 2          # gbdrift: dPdrho = -K on every line
        return out

    def restated(x0, sigma00, del_alpha=0.004):
        al = np.array([x0[0] - 0.5 * del_alpha, x0[0], x0[0] + 0.5 * del_alpha])
        lines = fieldlines(None, 0.5, al, th)
        t0 = x0[1]

        def gcf(line):
            bmag, gradpar, cvdrift, cvdrift0, gds2, gds21, gds22, gbdrift = line
            dP = bo.dPdrho_of(cvdrift, gbdrift, bmag)
            cv, gd = bo.fold_theta0(t0, cvdrift, cvdrift0, gds2, gds21, gds22)
            return (dP,) + bo.gcf(dP, bmag, gradpar, cv, gd)
        dP, g, c, f = gcf(lines[1])
        ref = ref_nearest(th, g, c, f, sigma00)
        gam, X, dX = ref["gam"], ref["X"], ref["dX"]
        bmag, gradpar, _, cvdrift0, _, gds21, gds22, _ = lines[1]
        gp = np.abs(gradpar)
        g_t = gp * (2 * gds21 + 2 * t0 * gds22) / bmag
        c_t = -1 * dP * cvdrift0 * 1 / (gp * bmag)
        f_t = (2 * gds21 + 2 * t0 * gds22) / bmag ** 2 * 1 / (gp * bmag)
        _, g_r, c_r, f_r = gcf(lines[2])
        _, g_l, c_l, f_l = gcf(lines[0])
        ja = bo.hf_derivative(gam, X, dX, f, (g_r - g_l) / del_alpha, (c_r - c_l) / del_alpha, (f_r - f_l) / del_alpha)
        jt = bo.hf_derivative(gam, X, dX, f, g_t, c_t, f_t)
        return -gam, np.array([-ja, -jt]), ref

    near = ibs_amd.make_obj_w_grad(fieldlines, ctx=ctx, eigenpair="nearest")
    dflt = ibs_amd.make_obj_w_grad(fieldlines, ctx=ctx)
    x0 = np.array([0.4, 0.3])
    v, j = near(x0, None, 0.5, th, None, 0.42)
    rv, rj, ref = restated(x0, 0.42)
    assert ref["idx"] > 0                                  # (the point is driven hard enough for the two modes to differ)
    assert abs(v - rv) < 1e-8 and np.abs(j - rj).max() < 1e-7, (v, rv, j, rj)
    vd, jd = dflt(x0, None, 0.5, th, None, 0.42)
    assert abs(vd - v) > 0.1
    v2, j2 = near(x0, None, 0.5, th, None, 1e3)
    assert abs(v2 - vd) < 1e-9 and np.abs(j2 - jd).max() < 1e-9, (v2, vd, j2, jd)
    with pytest.raises(ValueError):
        ibs_amd.make_obj_w_grad(fieldlines, ctx=ctx, eigenpair="bogus")


def test_errors(ctx):
    """even N, N = 33 and N = 65,539 are refused; one invalid system (g < 0) or one NaN sigma gets status 2 and leaves its
    neighbours bit-identical to a clean run; eigenpair="bogus" raises ValueError"""
    import ibs_amd
    for N in (512, 33, 65539):
        z = np.ones((1, N))
        with pytest.raises(ibs_amd.IbsError):
            ctx.solve_gcf_nearest(0.05, z, z, z, 0.42)
        with pytest.raises(ibs_amd.IbsError):
            ctx.gamma_scan_nearest(0.05, z, z, z, z, z, z, z, np.array([-1.0]), np.zeros(1), 0.42)
    N = 513
    rows = [salpha_line(N, dP)[1:] for dP in (-1.0, -4.0, -8.0, -2.0)]
    g, c, f = (np.stack([r[i] for r in rows]) for i in range(3))
    h = bo.theta_grid(N)[1] - bo.theta_grid(N)[0]
    sig = np.array([0.42, 0.42, 1.0, 0.3])
    clean = ctx.solve_gcf_nearest(h, g, c, f, sig, want_X=True, want_info=True)
    assert clean["nbad"] == 0
    g_bad = g.copy(); g_bad[1, 100] = -1.0
    s_bad = sig.copy(); s_bad[2] = np.nan
    for gg, ss, k in ((g_bad, sig, 1), (g, s_bad, 2)):
        r = ctx.solve_gcf_nearest(h, gg, c, f, ss, want_X=True, want_info=True)
        assert r["nbad"] == 1 and ((r["info"][k] >> 16) & 3) == 2 and r["idx"][k] == -1 and np.isnan(r["gam"][k])
        for i in range(4):
            if i != k:
                for key in ("lam", "idx", "gam", "X", "dX", "info"):
                    assert np.array_equal(r[key][i], clean[key][i]), (k, i, key)
    th = bo.theta_grid(257)
    gg, c0 = bo.salpha_gc(th, 1.0, 0.8, 0.0)
    with pytest.raises(ValueError):
        ibs_amd.gamma_ball_full(-4.0, th, np.ones(257), np.ones(257), c0, gg, ctx=ctx, eigenpair="bogus")
