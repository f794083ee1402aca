"""GPU: the exact vector-Jacobian product of gam and lam in the (g, c, f) rows (ibs_solve_gcf_vjp_f64, Context.solve_gcf_vjp), the
torch autograd layer over it (ibs_amd.autograd) and make_obj_w_grad(..., jac="exact").  Yardsticks: the bordered-system
restatement of tests/vjp_oracle.py (itself checked against central differences of the oracle in tests/test_vjp_cpu.py), and central
differences of the GPU's own forward."""
import os

import numpy as np
import pytest

from oracle import ballooning_oracle as bo
from tests import vjp_oracle as vo
from tests.helpers import synthetic_fieldlines

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def ctx():
    import ibs_amd
    c = ibs_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ncsx():
    import ibs_amd
    w = dict(np.load(os.path.join(G, "G8_wout_ncsx_op.npz")))
    return ibs_amd.SurfaceTables.from_wout(w, np.array([0.6, 0.9]))


def gcf_of(line7, dP, t0):
    bmag, gradpar, cvdrift, cvdrift0, gds2, gds21, gds22 = line7
    cv, gd = bo.fold_theta0(t0, cvdrift, cvdrift0, gds2, gds21, gds22)
    return bo.gcf(dP, bmag, gradpar, cv, gd)


def rows_max(ctx, ncsx, N):
    """lam_max systems at N: two s-alpha lines, two synthetic lines, two NCSX_op lines from the device geometry kernel"""
    th = bo.theta_grid(N)
    rows = []
    for sh, al, t0 in ((1.0, 0.8, 0.1), (0.5, 0.6, 0.3)):
        g, c = bo.salpha_gc(th, sh, al, t0)
        rows.append((g, c, g.copy()))
    for s, a, t0 in ((0.5, 0.3, 0.2), (0.8, 1.9, -0.4)):
        ln = synthetic_fieldlines(th)(s, [a])[0]
        rows.append(gcf_of(ln[:7], bo.dPdrho_of(ln[2], ln[7], ln[0]), t0))
    r = ctx.fieldline_geometry(ncsx, np.array([0, 1], dtype=np.int32), np.array([0.3, 1.1]), th)
    for k, t0 in ((0, 0.0), (1, 0.5)):
        rows.append(gcf_of(r["geo"][:7, k], r["dPdrho"][k], t0))
    return th, [np.stack([rw[i] for rw in rows]) for i in range(3)]


def rows_nearest(N):
    """an s-alpha line driven by dPdrho = -4: its eigenvalue nearest 0.42 lies below lam_max"""
    th = bo.theta_grid(N)
    g, c = bo.salpha_gc(th, 1.0, 0.8, 0.0)
    return th, [g[None], 4.0 * c[None], g[None].copy()]


def rel_rows(got, ref):
    return max(np.linalg.norm(got[k] - ref[k]) / np.linalg.norm(ref[k]) for k in range(3))


@pytest.mark.parametrize("N", [129, 513, 969, 1025, 2049, 2561, 4097])
def test_vjp_matches_restatement(ctx, ncsx, N):
    """(a) kernel rows against the bordered-system restatement at the GPU's own eigenpairs: 1e-9 of each row's norm, for gam_bar
    and lam_bar, on s-alpha, synthetic and NCSX_op lines (lam_max) and a nearest-sigma pair (sigma = 0.42, idx >= 1)"""
    th, (g, c, f) = rows_max(ctx, ncsx, N)
    h = th[1] - th[0]
    r = ctx.solve_gcf(h, g, c, f, want_X=True)
    lam, X = r["lam"], r["X"]
    thn, (gn, cn, fn) = rows_nearest(N)
    rn = ctx.solve_gcf_nearest(h, gn, cn, fn, 0.42, want_X=True)
    assert int(rn["idx"][0]) >= 1
    G_, C_, F_ = np.vstack([g, gn]), np.vstack([c, cn]), np.vstack([f, fn])
    L_, X_ = np.r_[lam, rn["lam"]], np.vstack([X, rn["X"]])
    for gb, lb in ((1.0, None), (None, 1.0)):
        v = ctx.solve_gcf_vjp(h, G_, C_, F_, L_, X_, gam_bar=gb, lam_bar=lb, want_info=True)
        assert v["nbad"] == 0 and not (v["info"] >> 16).any()
        for k in range(len(L_)):
            ref = vo.gcf_vjp(th, G_[k], C_[k], F_[k], L_[k], X_[k], gam_bar=gb or 0.0, lam_bar=lb or 0.0)
            err = rel_rows((v["g_bar"][k], v["c_bar"][k], v["f_bar"][k]), ref)
            assert err <= 1e-9, (N, k, gb, lb, err)


@pytest.mark.parametrize("N", [257, 2049])
def test_vjp_matches_gpu_central_differences(ctx, ncsx, N):
    """(b) independent of the restatement: directional central differences of the GPU's own forward, each system against its own
    derivative -- gam: step 1e-6, 1e-6; lam: 1e-5, by Richardson extrapolation of the steps 4e-4 and 2e-4 (the forward closes lam to a
    multiple of eps ||A||, an absolute noise that a step of 1e-5 turns into 5e-5 of a small derivative) -- lam_max systems and the
    nearest-sigma pair"""
    th, (g, c, f) = rows_max(ctx, ncsx, N)
    thn, (gn, cn, fn) = rows_nearest(N)
    h = th[1] - th[0]
    rng = np.random.default_rng(N)
    for mode, (G_, C_, F_) in (("max", (g, c, f)), ("nearest", (gn, cn, fn))):
        solve = (lambda a, b, d, **kw: ctx.solve_gcf(h, a, b, d, **kw)) if mode == "max" else \
            (lambda a, b, d, **kw: ctx.solve_gcf_nearest(h, a, b, d, 0.42, **kw))
        dG = np.stack([vo.smooth_direction(rng, th, G_[k]) for k in range(len(G_))])
        dC = np.stack([vo.smooth_direction(rng, th, np.abs(C_[k]).max()) for k in range(len(G_))])
        dF = np.stack([vo.smooth_direction(rng, th, F_[k]) for k in range(len(G_))])
        r = solve(G_, C_, F_, want_X=True)
        def central(key, t):
            return (solve(G_ + t * dG, C_ + t * dC, F_ + t * dF)[key] - solve(G_ - t * dG, C_ - t * dC, F_ - t * dF)[key]) / (2 * t)
        for key, bar, tol in (("gam", dict(gam_bar=1.0), 1e-6), ("lam", dict(lam_bar=1.0), 1e-5)):
            v = ctx.solve_gcf_vjp(h, G_, C_, F_, r["lam"], r["X"], **bar)
            an = (v["g_bar"] * dG).sum(1) + (v["c_bar"] * dC).sum(1) + (v["f_bar"] * dF).sum(1)
            fd = central("gam", 1e-6) if key == "gam" else (4 * central("lam", 2e-4) - central("lam", 4e-4)) / 3
            assert (np.abs(an - fd) <= tol * np.abs(an)).all(), (mode, key, an, fd)


def synthetic_geo_torch(N, n_lines, dev):
    import torch
    th = bo.theta_grid(N)
    lines = synthetic_fieldlines(th)(0.6, np.linspace(0.2, 1.4, n_lines))
    geo = torch.from_numpy(np.ascontiguousarray(lines[:, :7].transpose(1, 0, 2))).to(dev)
    dP = torch.tensor([bo.dPdrho_of(ln[2], ln[7], ln[0]) for ln in lines], dtype=torch.float64, device=dev)
    return th, geo, dP


def test_autograd_gradcheck(ctx):
    """(c) torch.autograd.gradcheck (FP64) on autograd.solve_gcf (3 systems, N = 129, both outputs) and on growth_rate (2 lines x 2
    theta0, N = 129) in all nine tensor inputs"""
    import torch
    from ibs_amd import autograd as iag
    dev = torch.device("cuda:0")
    N = 129
    th = bo.theta_grid(N)
    rows = [bo.salpha_gc(th, 1.0, 0.8, 0.1), bo.salpha_gc(th, 0.5, 0.6, 0.3), bo.salpha_gc(th, 0.8, 0.4, 0.0)]
    g = torch.tensor(np.stack([r[0] for r in rows]), device=dev, requires_grad=True)
    c = torch.tensor(np.stack([r[1] for r in rows]), device=dev, requires_grad=True)
    f = torch.tensor(np.stack([r[0] * (1 + 0.1 * np.cos(th)) for r in rows]), device=dev, requires_grad=True)
    h = float(th[1] - th[0])
    assert torch.autograd.gradcheck(lambda a, b, d: iag.solve_gcf(h, a, b, d, ctx=ctx), (g, c, f))
    _, geo, dP = synthetic_geo_torch(N, 2, dev)
    ins = [geo[k].clone().requires_grad_(True) for k in range(7)]
    ins.append(dP.clone().requires_grad_(True))
    ins.append(torch.tensor([0.1, 0.45], dtype=torch.float64, device=dev, requires_grad=True))
    assert torch.autograd.gradcheck(lambda *a: iag.growth_rate(h, *a, ctx=ctx), tuple(ins))


@pytest.mark.parametrize("N", [129, 969])
def test_growth_rate_forward_matches_gamma_scan(ctx, N):
    """(d) growth_rate's forward (theta0 fold and coefficients as torch expressions, shared and per-line theta0) equals the scan's gam"""
    import torch
    from ibs_amd import autograd as iag
    dev = torch.device("cuda:0")
    th, geo, dP = synthetic_geo_torch(N, 3, dev)
    h = float(th[1] - th[0])
    t0 = torch.linspace(-0.5, 1.5, 5, dtype=torch.float64, device=dev)
    ref = ctx.gamma_scan(h, *[geo[k] for k in range(7)], dP, t0)["gam"]
    got = iag.growth_rate(h, *[geo[k] for k in range(7)], dP, t0, ctx=ctx)
    assert got.shape == ref.shape
    assert ((got - ref).abs() <= 1e-11 * ref.abs().clamp_min(1e-3)).all(), (got - ref).abs().max()
    got2 = iag.growth_rate(h, *[geo[k] for k in range(7)], dP, t0.expand(3, 5).contiguous(), ctx=ctx)
    assert torch.equal(got2, got)
    near = iag.growth_rate(h, *[geo[k] for k in range(7)], dP, t0, eigenpair="nearest", sigma=1.0, ctx=ctx)
    refn = ctx.gamma_scan_nearest(h, *[geo[k] for k in range(7)], dP, t0, 1.0)["gam"]
    assert ((near - refn).abs() <= 1e-11 * refn.abs().clamp_min(1e-3)).all(), (near - refn).abs().max()


def ncsx_fieldlines(ctx, tables):
    def fl(vs, rho, alphas, theta):
        r = ctx.fieldline_geometry(tables, np.zeros(len(alphas), dtype=np.int32), np.asarray(alphas, dtype=np.float64), theta)
        return r["geo"].transpose(1, 0, 2)
    return fl


@pytest.mark.parametrize("eigenpair", ["max", "nearest"])
@pytest.mark.parametrize("kind", ["synthetic", "ncsx"])
def test_obj_w_grad_exact(ctx, kind, eigenpair):
    """(e) make_obj_w_grad(..., jac="exact"): val as the default's (1e-12); d/dtheta0 against a central difference of gam (1e-6);
    d/dalpha against a central difference with the geometry recomputed at alpha +- 1e-4 (1e-4 of |jac|)"""
    import ibs_amd
    N = 513
    th = bo.theta_grid(N)
    if kind == "synthetic":
        syn = synthetic_fieldlines(th)
        fl = lambda vs, rho, alphas, theta: syn(rho, alphas)
        x0, rho = np.array([0.7, 0.3]), 0.6
    else:
        w = dict(np.load(os.path.join(G, "G8_wout_ncsx_op.npz")))
        fl = ncsx_fieldlines(ctx, ibs_amd.SurfaceTables.from_wout(w, np.array([0.9])))
        x0, rho = np.array([0.4, 0.2]), 0.9
    exact = ibs_amd.make_obj_w_grad(fl, ctx=ctx, eigenpair=eigenpair, jac="exact")
    dflt = ibs_amd.make_obj_w_grad(fl, ctx=ctx, eigenpair=eigenpair)
    sig = 0.42
    v, j = exact(x0, None, rho, th, None, sig)
    vd, jd = dflt(x0, None, rho, th, None, sig)
    assert abs(v - vd) <= 1e-12 * abs(vd), (v, vd)
    t = 1e-4
    vp = exact(x0 + [0.0, t], None, rho, th, None, sig)[0]
    vm = exact(x0 - [0.0, t], None, rho, th, None, sig)[0]
    assert abs(j[1] - (vp - vm) / (2 * t)) <= 1e-6 * abs(j[1]), (j[1], (vp - vm) / (2 * t))
    vp = exact(x0 + [t, 0.0], None, rho, th, None, sig)[0]
    vm = exact(x0 - [t, 0.0], None, rho, th, None, sig)[0]
    assert abs(j[0] - (vp - vm) / (2 * t)) <= 1e-4 * np.abs(j).max(), (j[0], (vp - vm) / (2 * t))


def test_vjp_deterministic_and_batch_independent(ctx):
    """(f) bitwise repeatable, and a system's rows are the same bits alone and in a batch of 4,096"""
    import torch
    dev = torch.device("cuda:0")
    N = 513
    th = bo.theta_grid(N)
    al = np.linspace(0.2, 1.6, 4096)
    rows = [bo.salpha_gc(th, 0.6 + 0.4 * np.sin(a), a, 0.1 * a) for a in al]
    g = torch.tensor(np.stack([r[0] for r in rows]), device=dev)
    c = torch.tensor(np.stack([r[1] for r in rows]), device=dev)
    f = g * (1 + 0.1 * torch.cos(torch.tensor(th, device=dev)))
    h = float(th[1] - th[0])
    r = ctx.solve_gcf(h, g, c, f, want_X=True)
    gb = torch.linspace(0.5, 1.5, 4096, dtype=torch.float64, device=dev)
    lb = torch.linspace(-1.0, 1.0, 4096, dtype=torch.float64, device=dev)
    a = ctx.solve_gcf_vjp(h, g, c, f, r["lam"], r["X"], gam_bar=gb, lam_bar=lb, want_info=True)
    b = ctx.solve_gcf_vjp(h, g, c, f, r["lam"], r["X"], gam_bar=gb, lam_bar=lb)
    torch.cuda.synchronize()
    assert not (a["info"] >> 16).any()
    for k in ("g_bar", "c_bar", "f_bar"):
        assert torch.equal(a[k], b[k])
    for s in (0, 1777, 4095):
        one = ctx.solve_gcf_vjp(h, g[s:s + 1], c[s:s + 1], f[s:s + 1], r["lam"][s:s + 1], r["X"][s:s + 1], gam_bar=gb[s:s + 1],
                                lam_bar=lb[s:s + 1])
        for k in ("g_bar", "c_bar", "f_bar"):
            assert torch.equal(one[k][0], a[k][s]), (s, k)


def test_vjp_errors_and_status(ctx):
    """(g) argument errors are refused; a NaN lam or an X that is no eigenvector marks its own system only (status bit 1, NaN rows)"""
    import ctypes as C
    import ibs_amd
    N = 257
    th = bo.theta_grid(N)
    h = th[1] - th[0]
    rows = [bo.salpha_gc(th, 1.0, 0.8, 0.1 * k) for k in range(4)]
    g = np.stack([r[0] for r in rows]); c = np.stack([r[1] for r in rows]); f = g.copy()
    r = ctx.solve_gcf(h, g, c, f, want_X=True)
    lam, X = r["lam"], r["X"]
    with pytest.raises(ibs_amd.IbsError):
        ctx.solve_gcf_vjp(h, g, c, f, lam, X)                                  # no cotangent
    for n_bad in (256, 65, 65539):
        z = np.ones((1, n_bad))
        with pytest.raises(ibs_amd.IbsError):
            ctx.solve_gcf_vjp(0.01, z, z, z, np.ones(1), z, gam_bar=1.0)
    lib = ibs_amd._lib.lib()
    p = lambda a: C.c_void_p(a.ctypes.data)
    gbar, outs = np.ones(4), [np.empty((4, N)) for _ in range(3)]        # (kept alive: the library writes into them)
    args = [ctx._h, 4, N, float(h), p(g), p(c), p(f), N, p(lam), p(X), p(gbar), None, p(outs[0]), p(outs[1]), p(outs[2]),
            None, ibs_amd.MEM_HOST]
    assert lib.ibs_solve_gcf_vjp_f64(*args) == 0
    for i in (4, 5, 6, 8, 9, 12):
        bad = list(args)
        bad[i] = None
        assert lib.ibs_solve_gcf_vjp_f64(*bad) == -1, i                     # IBS_ERR_ARG
    bad = list(args); bad[7] = N - 1
    assert lib.ibs_solve_gcf_vjp_f64(*bad) < 0
    bad = list(args); bad[10] = None
    assert lib.ibs_solve_gcf_vjp_f64(*bad) < 0                                 # both cotangents null
    clean = ctx.solve_gcf_vjp(h, g, c, f, lam, X, gam_bar=1.0, lam_bar=0.5, want_info=True)
    lam2, X2 = lam.copy(), X.copy()
    lam2[1] = np.nan
    X2[2] = X2[2] + 1e-4 * np.sin(3 * th)
    got = ctx.solve_gcf_vjp(h, g, c, f, lam2, X2, gam_bar=1.0, lam_bar=0.5, want_info=True)
    assert got["nbad"] == 2
    assert [int(s) >> 16 for s in got["info"]] == [0, 2, 2, 0]
    for k in ("g_bar", "c_bar", "f_bar"):
        assert np.isnan(got[k][1:3]).all()
        assert np.array_equal(got[k][[0, 3]], clean[k][[0, 3]])


def test_vjp_flags_replaced_pivots_in_either_block(ctx):
    """status bit 0 reports a pivot below pivmin in the leading block (lane 0) and in the trailing block (lane 1) alike: rows whose
    arithmetic is exact and whose eigenvector has a zero entry next to one end make that end's first pivot exactly 0"""
    import torch
    import ibs_amd
    N = 67
    g, c, f, X = vo.pivot_breaking_rows(N)
    lam = np.full(3, 0.5)
    assert (vo.residual_ratio(1.0, g, c, f, lam, X) == 0).all()
    r = ctx.solve_gcf_vjp(1.0, g, c, f, lam, X, gam_bar=1.0, want_info=True)
    assert r["nbad"] == 2
    assert [int(s) >> 16 for s in r["info"]] == [1, 1, 0]
    dev = torch.device("cuda:0")
    t = [torch.from_numpy(a).to(dev) for a in (g, c, f, lam, X)]
    rd = ctx.solve_gcf_vjp(1.0, t[0], t[1], t[2], t[3], t[4], gam_bar=1.0, want_info=True)
    assert ((rd["info"] >> 16).cpu().tolist()) == [1, 1, 0]
    for k in ("g_bar", "c_bar", "f_bar"):
        assert np.array_equal(rd[k][2].cpu().numpy(), r[k][2])
    # lam_bar alone skips the adjoint solve: nothing to flag
    r2 = ctx.solve_gcf_vjp(1.0, g, c, f, lam, X, lam_bar=1.0, want_info=True)
    assert r2["nbad"] == 0 and not (r2["info"] >> 16).any()
    # the autograd backward reports the flag (a forward that hands over these very pairs)
    from ibs_amd import autograd as iag

    class Fixed:
        def solve_gcf(self, h, g, c, f, want_X=False):
            return dict(gam=torch.zeros(3, dtype=torch.float64, device=dev), lam=t[3], X=t[4])

        def solve_gcf_vjp(self, *a, **kw):
            return ctx.solve_gcf_vjp(*a, **kw)
    ins = [a.clone().requires_grad_(True) for a in t[:3]]
    gam, _ = iag.solve_gcf(1.0, *ins, ctx=Fixed())
    with pytest.warns(ibs_amd.VjpStatusWarning, match="2 system"):
        gam.sum().backward()


def test_vjp_padded_rows(ctx):
    """rows ld > N apart: the host call returns the padding entries as 0, the device call leaves them as they were; entries 0 .. N-1
    are the bits of the unpadded call"""
    import ctypes as C
    import torch
    import ibs_amd
    N, ld = 257, 263
    th = bo.theta_grid(N)
    h = float(th[1] - th[0])
    rows = [bo.salpha_gc(th, 1.0, 0.8, 0.1 * k) for k in range(3)]
    g = np.stack([r[0] for r in rows]); c = np.stack([r[1] for r in rows]); f = g * (1 + 0.1 * np.cos(th))
    r = ctx.solve_gcf(h, g, c, f, want_X=True)
    gb, lb = np.array([1.0, 0.5, -2.0]), np.array([0.3, 0.0, 1.0])
    ref = ctx.solve_gcf_vjp(h, g, c, f, r["lam"], r["X"], gam_bar=gb, lam_bar=lb)

    def pad(a, fill):
        out = np.full((3, ld), fill)
        out[:, :N] = a
        return out
    ins = [pad(a, 7.0) for a in (g, c, f, r["X"])]
    lib = ibs_amd._lib.lib()
    p = lambda a: C.c_void_p(a.ctypes.data)
    outs = [np.full((3, ld), 5.0) for _ in range(3)]
    assert lib.ibs_solve_gcf_vjp_f64(ctx._h, 3, N, h, p(ins[0]), p(ins[1]), p(ins[2]), ld, p(r["lam"]), p(ins[3]), p(gb), p(lb),
                                     p(outs[0]), p(outs[1]), p(outs[2]), None, ibs_amd.MEM_HOST) == 0
    dev = torch.device("cuda:0")
    d_ins = [torch.from_numpy(a).to(dev) for a in ins]
    d_vec = [torch.from_numpy(a).to(dev) for a in (r["lam"], gb, lb)]
    d_outs = [torch.full((3, ld), 5.0, dtype=torch.float64, device=dev) for _ in range(3)]
    q = lambda t: C.c_void_p(t.data_ptr())
    ctx._stream_from_torch(d_ins[0])
    assert lib.ibs_solve_gcf_vjp_f64(ctx._h, 3, N, h, q(d_ins[0]), q(d_ins[1]), q(d_ins[2]), ld, q(d_vec[0]), q(d_ins[3]), q(d_vec[1]),
                                     q(d_vec[2]), q(d_outs[0]), q(d_outs[1]), q(d_outs[2]), None, ibs_amd.MEM_DEVICE) == 0
    torch.cuda.synchronize()
    for k, key in enumerate(("g_bar", "c_bar", "f_bar")):
        assert np.array_equal(outs[k][:, :N], ref[key])
        assert (outs[k][:, N:] == 0.0).all()
        dk = d_outs[k].cpu().numpy()
        assert np.array_equal(dk[:, :N], ref[key])
        assert (dk[:, N:] == 5.0).all()


def test_library_eigenpairs_stay_well_inside_the_residual_bound(ctx, ncsx):
    """the VJP refuses a pair above 1024 N eps (||A|| + |lam|) max |X| (csrc/ibs_vjp.hip): every forward form of the library -- the
    register-resident, sub-wave, direct and row-streamed lam_max kernels, the long path and the nearest-sigma kernel -- hands over
    pairs below a quarter of that (measured up to 84 on the register-resident forms: tools/vjp_residuals.py, profiles/vjp_residuals.txt)"""
    import torch
    dev = torch.device("cuda:0")
    forms = set()
    for n, N in ((6, 129), (6, 969), (6, 2049), (6, 4097), (1800, 969), (4095, 513), (30000, 257)):
        h, (g, c, f) = vo.synthetic_batch(n, N)
        r = ctx.solve_gcf(h, *(torch.from_numpy(a).to(dev) for a in (g, c, f)), want_X=True)
        forms.add(ctx.last_launch()[0])
        q = vo.residual_ratio(h, g, c, f, r["lam"].cpu().numpy(), r["X"].cpu().numpy())
        assert q.max() < 256, (n, N, ctx.last_launch()[0], q.max())
    assert len(forms) >= 5, forms
    for N in (129, 969, 4097):
        th, (gn, cn, fn) = rows_nearest(N)
        rn = ctx.solve_gcf_nearest(th[1] - th[0], gn, cn, fn, 0.42, want_X=True)
        assert vo.residual_ratio(th[1] - th[0], gn, cn, fn, rn["lam"], rn["X"]).max() < 256
