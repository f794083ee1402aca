"""GPU: the fused scan VJP (ibs_gamma_scan_vjp_f64, Context.gamma_scan_vjp) and autograd.gamma_scan over it.  Inputs: s-alpha lines
written as geometry arrays (tests/certify_oracle.py) and the moving well of tests/edge_cases.py mapped onto geometry arrays with small
theta0 planes and a NEGATIVE gradpar; theta0 dyadic.  Yardsticks: the bordered-system restatement of tests/vjp_oracle.py folded through
a numpy pullback, central differences of the C oracle's gam, and the existing torch path autograd.growth_rate."""
import ctypes as C

import numpy as np
import pytest

from oracle import c_oracle as co
from tests import certify_oracle as cert
from tests import edge_cases as ec
from tests import vjp_oracle as vo

pytestmark = pytest.mark.gpu
T5 = np.array([0.0, 0.125, 0.25, 0.5, 0.75])
T3 = np.array([0.0, 0.25, 0.5])
T15 = np.arange(15) / 16.0


@pytest.fixture(scope="module")
def ctx():
    import ibs_amd
    c = ibs_amd.Context(0)
    yield c
    c.close()


def make_lines(N, n_lines):
    """(theta, h, geo7 [7][n_lines][N], dPdrho (n_lines,)): s-alpha lines (shat, alpha) = (1.2, 1.2), (0.8, 0.9), ... driven by dPdrho = -6
    (their second eigenvalue then lies at least 0.19 above the third at every theta0 used here) and -- every third line, the
    last of three -- a moving well (centre N // 2 + 3) with theta0 planes of size 0.05 and gradpar < 0"""
    th = ec.theta_grid(N)
    k = np.arange(n_lines)
    geo7, dP = cert.salpha_geometry(th, 1.2 - 0.4 * (k % 2) + 0.0005 * k, 1.2 - 0.3 * (k % 2) + 0.0005 * k)
    geo7 = [np.array(a) for a in geo7]
    dP = -6.0 - 0.002 * k
    for l in range(2, n_lines, 3):
        g, c, f = ec.well_rows(th, N // 2 + 3)
        w7, wdP = cert.gcf_to_geometry(g, c, f, dPdrho=-1.5, th0_planes=0.05, seed=l)
        for a, b in zip(geo7, w7):
            a[l] = b[0]
        geo7[1][l] *= -1.0
        dP[l] = wdP[0]
    return th, float(th[1] - th[0]), np.stack(geo7), dP


def pullback_numpy(gb, cb, fb, v, dP, th0):
    """rows (g_bar, c_bar, f_bar) (N,) of one system -> (seven bar rows (7, N), dP_bar, theta0_bar): the chain rule through
    ball_scan.py:267-268 and utils.py:1560-1562, closed forms"""
    B, gpar, cv_, cv0, g0, g1, g2 = v
    gp, sg = np.abs(gpar), np.sign(gpar)
    cv = cv_ + th0 * cv0
    gd = g0 + 2 * th0 * g1 + th0 ** 2 * g2
    g, c, f = gp * gd / B, -dP * cv / (gp * B), gd / (gp * B ** 3)
    gd_bar = gb * gp / B + fb / (gp * B ** 3)
    cv_bar = cb * (-dP) / (gp * B)
    bar = np.stack([-(gb * g + cb * c + 3 * fb * f) / B, sg * (gb * g - cb * c - fb * f) / gp, cv_bar, th0 * cv_bar, gd_bar,
                    2 * th0 * gd_bar, th0 ** 2 * gd_bar])
    t_bar = (cv_bar * cv0 + gd_bar * (2 * g1 + 2 * th0 * g2)).sum()
    return bar, (cb * c).sum() / dP, t_bar


def top3(th, g, c, f):
    """the three largest eigenvalues, descending"""
    from scipy.linalg import eigh_tridiagonal
    from oracle import ballooning_oracle as bo
    d, e, fd = bo.assemble(th, g, c, f)[:3]
    n = len(d)
    return eigh_tridiagonal(d / fd, e[1:n] / np.sqrt(fd[:-1] * fd[1:]), eigvals_only=True, select="i", select_range=(n - 3, n - 1))[::-1]


_REF = {}


def reference(ctx, N, n_lines, t0, nearest):
    """the inputs of a shape and the restatement's bars, computed once: the library's own eigenpair of every system (solve_gcf /
    solve_gcf_nearest on the host-folded rows), vo.gcf_vjp at it, the numpy pullback, the sum over theta0"""
    key = (N, n_lines, len(t0), nearest)
    if key in _REF:
        return _REF[key]
    th, h, geo7, dP = make_lines(N, n_lines)
    g, c, f = cert.fold_rows(geo7, dP, t0)
    rng = np.random.default_rng(N + 7 * nearest)
    gbar = rng.uniform(0.5, 1.5, (n_lines, len(t0))) * rng.choice([-1.0, 1.0], (n_lines, len(t0)))
    sigma = None
    if nearest:
        # below lam_max: a quarter of the way from the second eigenvalue to the third, so that the nearest pair is the second
        sigma = np.array([(lambda w: w[1] - 0.25 * (w[1] - w[2]))(top3(th, g[k], c[k], f[k])) for k in range(len(g))]).reshape(gbar.shape)
        r = ctx.solve_gcf_nearest(h, g, c, f, sigma.reshape(-1), want_X=True)
        assert (r["idx"] == 1).all(), r["idx"]
    else:
        r = ctx.solve_gcf(h, g, c, f, want_X=True)
    assert r["nbad"] == 0
    geo_bar, dP_bar, t_bar = np.zeros_like(geo7), np.zeros(n_lines), np.zeros(gbar.shape)
    for l in range(n_lines):
        for t in range(len(t0)):
            k = l * len(t0) + t
            rows = vo.gcf_vjp(th, g[k], c[k], f[k], r["lam"][k], r["X"][k], gam_bar=gbar[l, t])
            b, d, tb = pullback_numpy(*rows, geo7[:, l], dP[l], t0[t])
            geo_bar[:, l] += b; dP_bar[l] += d; t_bar[l, t] = tb
    _REF[key] = dict(th=th, h=h, geo7=geo7, dP=dP, t0=t0, gbar=gbar, sigma=sigma, lam=r["lam"].reshape(gbar.shape),
                     gam=r["gam"].reshape(gbar.shape), geo_bar=geo_bar, dP_bar=dP_bar, t_bar=t_bar)
    return _REF[key]


def run(ctx, d, **kw):
    return ctx.gamma_scan_vjp(d["h"], *d["geo7"], d["dP"], d["t0"], d["gbar"], sigma=d["sigma"], want_info=True, **kw)


@pytest.mark.parametrize("nearest", [False, True])
@pytest.mark.parametrize("N,n_lines,t0", [(67, 3, T5), (131, 3, T5), (769, 3, T5), (2051, 2, T3)])
def test_bars_match_the_restatement(ctx, N, n_lines, t0, nearest):
    """1. each of the seven planes, dPdrho_bar and theta0_bar within 1e-9 of its own max-norm of the restatement (the bar
    tests/test_gpu_vjp.py (a) holds the raw VJP to), lam_max's pair and the second pair (sigma below lam_max).  67: one row per lane;
    769: two full 384-row LDS chunks plus one row; 2,051: the first length that was always on the long path."""
    d = reference(ctx, N, n_lines, t0, nearest)
    r = run(ctx, d)
    assert ctx.last_launch()[0] == "ibs::k_scan_vjp_reduce"
    assert r["nbad"] == 0 and not ((r["info"] >> 16) & 0xc3).any(), r["info"] >> 16
    assert np.abs(r["lam"] - d["lam"]).max() <= 1e-11 * np.abs(d["lam"]).max()
    assert np.abs(r["gam"] - d["gam"]).max() <= 1e-8
    for k in range(7):
        err = np.abs(r["geo_bar"][k] - d["geo_bar"][k]).max() / np.abs(d["geo_bar"][k]).max()
        print("N %d nearest %d plane %d: %.3g" % (N, nearest, k, err))
        assert err <= 1e-9, (N, nearest, k, err)
    for name, ref in (("dPdrho_bar", d["dP_bar"]), ("theta0_bar", d["t_bar"])):
        err = np.abs(r[name] - ref).max() / np.abs(ref).max()
        print("N %d nearest %d %s: %.3g" % (N, nearest, name, err))
        assert err <= 1e-9, (N, nearest, name, err)
    assert (r["geo_bar"][[3, 5, 6]][:, :2] != 0).any()          # (the theta0 planes of the s-alpha lines receive their share)
    if n_lines > 2:
        assert (d["geo7"][1][2] < 0).all() and np.abs(r["geo_bar"][1][2]).max() > 0


def test_bars_match_central_differences_of_the_c_oracle(ctx):
    """2. independent of the restatement: phi = sum gam_bar gam of the C oracle's scan, central differences with step 1e-6 along a
    smooth random direction in each of the seven arrays, in dPdrho and in theta0, against the contraction of the bars: 1e-6
    relative (steps and tolerance of tests/test_gpu_vjp.py (b)).  N = 131, 2 lines x 3 theta0"""
    N, n_lines, t0 = 131, 2, T3
    th, h, geo7, dP = make_lines(N, n_lines)
    rng = np.random.default_rng(11)
    gbar = rng.uniform(0.5, 1.5, (n_lines, len(t0)))
    r = ctx.gamma_scan_vjp(h, *geo7, dP, t0, gbar, want_info=True)
    assert r["nbad"] == 0

    def phi(geo, dp, t):
        return float((gbar * co.gamma_scan(h, *geo, dp, t)[0]).sum())
    step = 1e-6
    for k in range(9):
        if k < 7:
            scale = np.abs(geo7[k]).max(axis=1, keepdims=True)
            dirn = np.stack([vo.smooth_direction(rng, th, 1.0) for _ in range(n_lines)]) * np.where(scale > 0, scale, 1.0)
            e = np.zeros_like(geo7); e[k] = dirn
            fd = (phi(geo7 + step * e, dP, t0) - phi(geo7 - step * e, dP, t0)) / (2 * step)
            an = float((r["geo_bar"][k] * dirn).sum())
        elif k == 7:
            dirn = rng.standard_normal(n_lines)
            fd = (phi(geo7, dP + step * dirn, t0) - phi(geo7, dP - step * dirn, t0)) / (2 * step)
            an = float((r["dPdrho_bar"] * dirn).sum())
        else:
            dirn = rng.standard_normal(len(t0))
            fd = (phi(geo7, dP, t0 + step * dirn) - phi(geo7, dP, t0 - step * dirn)) / (2 * step)
            an = float((r["theta0_bar"].sum(0) * dirn).sum())
        print("input %d: analytic %.12g central difference %.12g rel %.3g" % (k, an, fd, abs(an - fd) / abs(an)))
        assert abs(an - fd) <= 1e-6 * abs(an), (k, an, fd)


# worst relative plane difference between the two backward paths measured on these inputs (docs/EXPERIMENTS.md, "Fused scan VJP"):
# the assertion is 8 x that (headroom for other drivers and compilers), capped at the finite-difference bar of test 2
GROWTH_RATE_MEASURED = {131: 3.54e-13, 969: 1.05e-11}


@pytest.mark.parametrize("N", [131, 969])
def test_backward_matches_growth_rate(ctx, N):
    """3. autograd.gamma_scan(...).backward() against autograd.growth_rate(...).backward() on the same inputs and cotangent, 3 x 5.
    The two forwards are different solvers (the scan kernel / the raw solve on torch-folded rows) and the two backwards solve again
    or not, so the tolerance is measured, not derived: 8 x the worst relative plane difference seen, at most 1e-6."""
    import torch
    from ibs_amd import autograd as iag
    dev = torch.device("cuda:0")
    th, h, geo7, dP = make_lines(N, 3)
    gbar = torch.from_numpy(np.random.default_rng(N).uniform(0.5, 1.5, (3, 5))).to(dev)
    grads = []
    for fn in (iag.gamma_scan, iag.growth_rate):
        ins = [torch.from_numpy(a.copy()).to(dev).requires_grad_(True) for a in (*geo7, dP, T5)]
        gam = fn(h, *ins, ctx=ctx)
        (gam * gbar).sum().backward()
        grads.append([t.grad.cpu().numpy() for t in ins])
        assert all(np.isfinite(g_).all() for g_ in grads[-1])
    worst = 0.0
    for k, (a, b) in enumerate(zip(*grads)):
        err = np.abs(a - b).max() / np.abs(b).max()
        print("N %d input %d: %.3g" % (N, k, err))
        worst = max(worst, err)
    print("N %d worst %.3g" % (N, worst))
    assert worst <= min(8 * GROWTH_RATE_MEASURED[N], 1e-6), (N, worst)


def same_bits(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


KEYS = ("geo_bar", "dPdrho_bar", "theta0_bar", "gam", "lam", "info")


def raw_host_call(ctx, d, ld):
    """the C entry point on host pointers with the input rows and geo_bar ld apart (the binding always passes ld = N)"""
    n_lines, N = d["geo7"][0].shape
    nt = len(d["t0"])
    pad = [np.full((n_lines, ld), 7.0) for _ in range(7)]
    for p_, a in zip(pad, d["geo7"]):
        p_[:, :N] = a
    out = dict(geo_bar=np.full((7, n_lines, ld), -3.0), dPdrho_bar=np.empty(n_lines), theta0_bar=np.empty((n_lines, nt)),
               gam=np.empty((n_lines, nt)), lam=np.empty((n_lines, nt)), info=np.empty((n_lines, nt), np.int32))
    ptr = lambda a: C.c_void_p(a.ctypes.data)
    keep = [np.ascontiguousarray(a, dtype=np.float64) for a in (d["dP"], d["t0"], d["gbar"])]
    sig = None if d["sigma"] is None else np.ascontiguousarray(d["sigma"])
    rc = ctx._lib.ibs_gamma_scan_vjp_f64(ctx._h, n_lines, nt, N, d["h"], *[ptr(a) for a in pad], ld, ptr(keep[0]), ptr(keep[1]),
                                         None if sig is None else ptr(sig), ptr(keep[2]), *[ptr(out[k]) for k in KEYS], 1)
    assert rc == 0, (rc, ctx._lib.ibs_last_error())
    return out


@pytest.mark.parametrize("nearest", [False, True])
def test_results_are_bitwise_repeatable_and_independent_of_the_call(ctx, nearest):
    """4. the same call twice; the lines in reversed order; 1-line chunks, and chunks of 2 and 1 lines (nearest_chunk_systems), against the default; host pointers
    with a row pitch of N + 6 (padding back as 0) against device pointers: identical bits"""
    import torch
    dev = torch.device("cuda:0")
    d = reference(ctx, 131, 3, T5, nearest)
    a = run(ctx, d)
    b = run(ctx, d)
    for k in KEYS:
        assert same_bits(a[k], b[k]), k
    rev = dict(d, geo7=np.ascontiguousarray(d["geo7"][:, ::-1]), dP=d["dP"][::-1].copy(), gbar=d["gbar"][::-1].copy(),
               sigma=None if d["sigma"] is None else d["sigma"][::-1].copy())
    r = run(ctx, rev)
    for k in KEYS:
        assert same_bits(np.ascontiguousarray(r[k][:, ::-1] if k == "geo_bar" else r[k][::-1]), a[k]), k
    ctx.set_option("nearest_chunk_systems", len(T5))
    try:
        c = run(ctx, d)
        assert ctx.last_launch() == ("ibs::k_scan_vjp_reduce", 4)          # (one line: one block of four waves)
        ctx.set_option("nearest_chunk_systems", 2 * len(T5))               # (a chunk of two lines, then a short last one)
        c2 = run(ctx, d)
    finally:
        ctx.set_option("nearest_chunk_systems", None)
    for k in KEYS:
        assert same_bits(c[k], a[k]), k
        assert same_bits(c2[k], a[k]), ("chunks of 2 and 1 lines", k)
    up = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    t = ctx.gamma_scan_vjp(d["h"], *[up(x) for x in d["geo7"]], up(d["dP"]), up(d["t0"]), up(d["gbar"]), sigma=up(d["sigma"]),
                           want_info=True)
    for k in KEYS:
        assert same_bits(t[k].cpu().numpy(), a[k]), k
    N = 131
    h = raw_host_call(ctx, d, N + 6)
    assert (h["geo_bar"][:, :, N:] == 0.0).all()
    assert same_bits(np.ascontiguousarray(h["geo_bar"][:, :, :N]), a["geo_bar"])
    for k in KEYS[1:]:
        assert same_bits(h[k], a[k]), k


def test_more_systems_than_waves(ctx):
    """5. 140 lines x 15 theta0 at N = 67: 2,100 systems, more than the persistent grid's waves.  Sampled lines equal the same lines
    run alone, bit for bit"""
    N, n_lines = 67, 140
    th, h, geo7, dP = make_lines(N, n_lines)
    gbar = np.random.default_rng(3).uniform(0.5, 1.5, (n_lines, 15))
    r = ctx.gamma_scan_vjp(h, *geo7, dP, T15, gbar, want_info=True)
    assert r["nbad"] == 0 and np.isfinite(r["geo_bar"]).all()
    for l in (0, 68, 71, 139):
        one = ctx.gamma_scan_vjp(h, *[np.ascontiguousarray(a[l:l + 1]) for a in geo7], dP[l:l + 1], T15, gbar[l:l + 1], want_info=True)
        for k in KEYS:
            assert same_bits(one[k], np.ascontiguousarray(r[k][:, l:l + 1] if k == "geo_bar" else r[k][l:l + 1])), (l, k)


def test_a_failed_system_poisons_its_own_line_only(ctx):
    """6. a NaN planted in bmag of line 1 of 3: that line's rows, dPdrho_bar and theta0_bar are NaN with status bit 1, lines 0 and
    2 are bitwise those of a clean run; with gam_bar[1, :] = 0 line 1's rows are exactly 0; a non-finite gam_bar does the same to
    its line and sets status bit 1 on its system; gam_bar all zero gives all bars exactly 0 with gam and lam still returned"""
    d = reference(ctx, 131, 3, T5, False)
    clean = run(ctx, d)
    geo7 = d["geo7"].copy()
    geo7[0, 1, 40] = np.nan
    r = run(ctx, dict(d, geo7=geo7))
    assert np.isnan(r["geo_bar"][:, 1]).all() and np.isnan(r["dPdrho_bar"][1]) and np.isnan(r["theta0_bar"][1]).all()
    assert (((r["info"][1] >> 16) & 2) != 0).all() and r["nbad"] == len(T5)
    for l in (0, 2):
        assert same_bits(np.ascontiguousarray(r["geo_bar"][:, l]), np.ascontiguousarray(clean["geo_bar"][:, l])), l
        for k in KEYS[1:]:
            assert same_bits(r[k][l], clean[k][l]), (l, k)
    gbar = d["gbar"].copy()
    gbar[1, :] = 0.0
    z = run(ctx, dict(d, geo7=geo7, gbar=gbar))
    assert (z["geo_bar"][:, 1] == 0.0).all() and z["dPdrho_bar"][1] == 0.0 and (z["theta0_bar"][1] == 0.0).all()
    assert (((z["info"][1] >> 16) & 2) != 0).all()
    for l in (0, 2):
        assert same_bits(np.ascontiguousarray(z["geo_bar"][:, l]), np.ascontiguousarray(clean["geo_bar"][:, l])), l
    gbar = d["gbar"].copy()
    gbar[2, 3] = np.inf
    i = run(ctx, dict(d, gbar=gbar))
    assert np.isnan(i["geo_bar"][:, 2]).all() and np.isnan(i["dPdrho_bar"][2]) and np.isnan(i["theta0_bar"][2, 3])
    assert np.isfinite(i["theta0_bar"][2, [0, 1, 2, 4]]).all() and ((i["info"] >> 16) & 3).tolist() == [[0] * 5, [0] * 5, [0, 0, 0, 2, 0]]
    for l in (0, 1):
        assert same_bits(np.ascontiguousarray(i["geo_bar"][:, l]), np.ascontiguousarray(clean["geo_bar"][:, l])), l
    o = run(ctx, dict(d, gbar=np.zeros_like(d["gbar"])))
    assert (o["geo_bar"] == 0.0).all() and (o["dPdrho_bar"] == 0.0).all() and (o["theta0_bar"] == 0.0).all()
    assert same_bits(o["gam"], clean["gam"]) and same_bits(o["lam"], clean["lam"]) and not (o["info"] >> 16).any()


class MovedGam:
    """a Context whose gamma_scan_vjp reports the gam of system (1, 2) 1e-6 off: what a backward that lands on another eigenpair looks like"""

    def __init__(self, ctx):
        self._ctx = ctx

    def __getattr__(self, name):
        return getattr(self._ctx, name)

    def gamma_scan_vjp(self, *args, **kw):
        r = self._ctx.gamma_scan_vjp(*args, **kw)
        r["gam"][1, 2] += 1e-6
        return r


def test_a_moved_eigenpair_gets_nan_gradients_and_a_warning(ctx):
    """autograd.gamma_scan: a backward whose own solve lands more than 1e-8 from the forward's gam on one system (stood in for by
    MovedGam) gives that system's line NaN gradients and a VjpStatusWarning; the other lines keep theirs, bit for bit"""
    import torch
    import ibs_amd
    from ibs_amd import autograd as iag
    dev = torch.device("cuda:0")
    d = reference(ctx, 131, 3, T5, True)
    sig = torch.from_numpy(d["sigma"]).to(dev)
    grads = []
    for c in (ctx, MovedGam(ctx)):
        ins = [torch.from_numpy(a.copy()).to(dev).requires_grad_(True) for a in (*d["geo7"], d["dP"], d["t0"])]
        gam = iag.gamma_scan(d["h"], *ins, eigenpair="nearest", sigma=sig, ctx=c)
        if c is ctx:
            gam.sum().backward()
        else:
            with pytest.warns(ibs_amd.VjpStatusWarning):
                gam.sum().backward()
        grads.append([t.grad.cpu().numpy() for t in ins])
    for clean, moved in zip(grads[0][:8], grads[1][:8]):
        assert np.isfinite(clean).all() and np.isnan(moved[1]).all()
        assert same_bits(np.ascontiguousarray(moved[[0, 2]]), np.ascontiguousarray(clean[[0, 2]]))
    assert np.isnan(grads[1][8]).all() and np.isfinite(grads[0][8]).all()          # (theta0 is shared: its gradient sums over the lines)
