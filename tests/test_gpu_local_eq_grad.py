"""GPU: the local-equilibrium gradients (ibs_local_eq_grad_f64, csrc/ibs_local_eq_grad.hip; Context.local_eq_grad,
Context.local_eq_boundary_grad, autograd.local_eq_lam / local_eq_crossing, BallooningScan.local_eq_boundary_sensitivity) against the numpy
restatement ibs_amd.local_eq_lam_grad on the C oracle's eigenpair (tests/local_eq_grad_cases.py), against an independent route through
autograd.solve_gcf, and against central differences of the library's own forward results.

Tolerances.  lam: |lam - lam_oracle| <= 4 N eps ||A||, the suite's own.  Derivatives: a component's deviation from the numpy formula on
the oracle's eigenpair, relative to the component's SCALE (the sum of the absolute values of its three terms, over q), measured on
these batches on an MI355X (docs/EXPERIMENTS.md R6.36; the margin is for the dependence of the mode's error on the device's reduction
order):
    dlam      largest 1.35e-9 (N = 771)   asserted at DLAM_BOUND = 1.4e-8, ten times the measured value
    geo_bar   largest 1.39e-7 (N = 4097, no ps; 5.0e-9 at N = 2051, <= 7.5e-10 up to N = 771)   ten times that is 1.4e-6, ABOVE the
              1e-6 the bound may not exceed (the suite's bound on the mode, in which the formula is first order): asserted at
              GEO_BOUND = 1e-6, a margin of 7.2 instead of 10.  The scale of a plane's entry is per grid point, so this figure is the
              RELATIVE pointwise agreement of two modes in their tails, thousands of recurrence steps from the twist row, where the
              suite bounds the mode absolutely; the sums (dlam) do not see it.
"""
import ctypes
import os

import numpy as np
import pytest

from ibs_amd import local_eq_ray_triples
from oracle import ballooning_oracle as bo
from tests import local_eq_boundary_cases as lbc
from tests import local_eq_cases as lc
from tests import local_eq_grad_cases as gc

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(__file__), "golden")
EPS = lc.EPS
DLAM_BOUND, GEO_BOUND = 1.4e-8, 1e-6      # (see the module docstring)
assert max(DLAM_BOUND, GEO_BOUND) <= 1e-6
KEYS = ("lam", "gam", "dlam", "geo_bar", "info")


@pytest.fixture(scope="module")
def ctx():
    import ibs_amd
    return ibs_amd.Context(0)


@pytest.fixture(scope="module")
def g3():
    return np.load(os.path.join(G, "G3_ncsx_lines.npz"))


def status(r):
    return np.asarray(r["info"]) >> 16


def grad_of(ctx, b, line_of=None, var=None, **kw):
    """Context.local_eq_grad on a batch of tests/local_eq_grad_cases (host pointers), planes and info included"""
    kw = dict(dict(want_geo_bar=True, want_info=True), **kw)
    return ctx.local_eq_grad(b["th"][0], b["th"][1] - b["th"][0], lc.to_geo(b["lines"]), b["dP"], b["centre"], b["sigma"],
                             b["line_of"] if line_of is None else line_of, b["var"] if var is None else var, ps=b["ps"], **kw)


def deviation(r, an):
    """largest deviation of dlam and of geo_bar (8, n, N) from the numpy formula, relative to the component's scale.  A component whose
    scale is exactly 0 -- an end point, where the mode vanishes; the gbdrift plane at p = 1; a grid point where the fold variable x is
    0 in numpy's rounding -- has no scale of its own: there the deviation is held to the bound times the largest scale of its row"""
    out = []
    for got, want, scale, bound in ((r["dlam"], an["dlam"], an["dlam_scale"], DLAM_BOUND),
                                    (np.transpose(r["geo_bar"], (1, 0, 2)), an["geo_bar"], an["geo_bar_scale"], GEO_BOUND)):
        dev = np.abs(got - want)
        row = np.broadcast_to(scale.max(axis=-1, keepdims=True), scale.shape)
        assert (dev[scale == 0] <= bound * row[scale == 0]).all()
        out.append((dev[scale > 0] / scale[scale > 0]).max())
    return out


def check_batch(ctx, b, what):
    ref = gc.oracle_pairs(b)
    an = gc.numpy_grads(b, ref)
    r = grad_of(ctx, b)
    assert "k_local_eq_grad" in ctx.last_launch()[0], ctx.last_launch()
    e_lam = (np.abs(r["lam"] - ref["lam"]) / ref["tol_lam"]).max()
    e_gam = np.abs(r["gam"] - ref["gam"]).max()
    d_lam, d_geo = deviation(r, an)
    print("%s: max |lam - oracle| / (4 N eps ||A||) %.2e, max |gam - oracle| %.2e, deviation / scale: dlam %.2e, geo_bar %.2e"
          % (what, e_lam, e_gam, d_lam, d_geo))
    assert r["nbad"] == 0 and not status(r).any()
    assert e_lam <= 1.0 and e_gam <= 1e-8, (what, e_lam, e_gam)
    assert d_lam <= DLAM_BOUND and d_geo <= GEO_BOUND, (what, d_lam, d_geo)


@pytest.mark.parametrize("N", [67, 129, 385, 387, 769, 771, 2051, 4097])
def test_values_and_gradients_against_the_cpu(ctx, N):
    """1. a dozen points on the three s-alpha lines, with and without their ps rows, at the minimum N, the 64-lane stride and both sides of
    the kVecChunk (384 rows) and kLongChunk (768 rows) edges: lam, gam, dlam and geo_bar"""
    check_batch(ctx, gc.salpha_batch(N, True), "s-alpha N=%d ps" % N)
    check_batch(ctx, gc.salpha_batch(N, False), "s-alpha N=%d" % N)


def test_ncsx_lines_against_the_cpu(ctx, g3):
    """1b. a dozen points on four committed NCSX lines at N = 513, both signs of sigma, a ps row each"""
    check_batch(ctx, gc.ncsx_batch(g3), "NCSX N=513")


def torch_rows(th, geo, dP, centre, sigma, line_of, var, ps):
    """the rule in torch, differentiably: (g, c, f), each (n_pts, N), of the points"""
    B, gp, cv, cv0, gds2, gds21, gds22, gb = (geo[k][line_of] for k in range(8))
    a = gp.abs()
    t0, e, p = var[:, 0:1], var[:, 1:2], var[:, 2:3]
    x = t0 * (1 + e) + sigma[line_of, None] * e * (th[None] - centre[line_of, None])
    if ps is not None:
        x = x + (p - 1) * ps[line_of]
    cvp = gb + p * (cv - gb) + x * cv0
    gd = gds2 + 2 * x * gds21 + x * x * gds22
    return a * gd / B, -(p * dP[line_of, None]) * cvp / (a * B), gd / (B ** 3 * a)


@pytest.mark.parametrize("N", [67, 129])
def test_independent_route_through_the_rows_vjp(ctx, N):
    """2. autograd.local_eq_lam(...).sum().backward() against the same rows built in torch from the rule and sent through
    autograd.solve_gcf (the library's exact rows-VJP, another kernel and another formula): lam bitwise-close (4 N eps ||A||) and the
    gradients in geo within GEO_BOUND, in dPdrho and var within DLAM_BOUND of the scale of the component (numpy, on the oracle's eigenpair); a line's
    cotangent is the sum over its points, whose scales add"""
    import torch
    from ibs_amd import autograd as iag
    dev = torch.device("cuda:0")
    b = gc.salpha_batch(N, True)
    ref = gc.oracle_pairs(b)
    an = gc.numpy_grads(b, ref)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    th, lo, h = t(b["th"]), float(b["th"][0]), float(b["th"][1] - b["th"][0])
    line_of = t(b["line_of"].astype(np.int64))
    grads = []
    for route in (0, 1):
        geo, dP, var = t(lc.to_geo(b["lines"])).requires_grad_(True), t(b["dP"]).requires_grad_(True), t(b["var"]).requires_grad_(True)
        if route == 0:
            lam = iag.local_eq_lam(lo, h, geo, dP, b["centre"], b["sigma"], line_of, var, ps=t(b["ps"]), ctx=ctx)
        else:
            g, c, f = torch_rows(th, geo, dP, t(b["centre"]), t(b["sigma"]), line_of, var, t(b["ps"]))
            lam = iag.solve_gcf(h, g.contiguous(), c.contiguous(), f.contiguous(), ctx=ctx)[1]
        lam.sum().backward()
        grads.append([x.detach().cpu().numpy() for x in (lam, geo.grad, dP.grad, var.grad)])
    (l0, g0, p0, v0), (l1, g1, p1, v1) = grads
    assert (np.abs(l0 - l1) <= 2 * ref["tol_lam"]).all()            # (each within tol_lam of the oracle)
    onehot = np.eye(3)[b["line_of"]]                          # (n_pts, n_lines)
    s_geo = np.einsum("pl,pkj->klj", onehot, an["geo_bar_scale"])
    s_dP = onehot.T @ an["dlam_scale"][:, 3]
    figs = [(np.abs(g0 - g1)[s_geo > 0] / s_geo[s_geo > 0]).max(), (np.abs(p0 - p1) / s_dP).max(),
            (np.abs(v0 - v1) / an["dlam_scale"][:, :3]).max()]
    print("independent route N=%d: deviation / scale in geo %.2e, dPdrho %.2e, var %.2e" % (N, *figs))
    assert (np.abs(g0 - g1)[s_geo == 0] <= GEO_BOUND * s_geo.max()).all()      # (end points, where the mode vanishes: both are ~0)
    assert figs[0] <= GEO_BOUND and max(figs[1:]) <= DLAM_BOUND, figs


def test_without_gradients_the_bits_of_the_scan(ctx, g3):
    """3. dlam and geo_bar not requested: lam and gam are Context.local_eq_scan's bits on the same lines and triples (every (line,
    triple) pair as a point), on the s-alpha lines at N = 67 and 771 and the NCSX lines at N = 513; with them requested lam, gam and info
    do not change"""
    for b in (gc.salpha_batch(67, True), gc.salpha_batch(771, False), gc.ncsx_batch(g3)):
        n, nv = len(b["lines"]), len(b["var"])
        lo, h = b["th"][0], b["th"][1] - b["th"][0]
        sc = ctx.local_eq_scan(lo, h, lc.to_geo(b["lines"]), b["dP"], b["centre"], b["sigma"], b["var"], ps=b["ps"], want_info=True)
        line_of, var = np.repeat(np.arange(n), nv).astype(np.int32), np.tile(b["var"], (n, 1))
        r = grad_of(ctx, b, line_of, var, want_grad=False, want_geo_bar=False)
        assert set(r) == {"lam", "gam", "info", "nbad"} and r["nbad"] == 0
        full = grad_of(ctx, b, line_of, var)
        for k in ("lam", "gam", "info"):
            assert np.array_equal(r[k].reshape(n, nv), sc[k]), k
            assert np.array_equal(full[k], r[k]), k


@pytest.fixture(scope="module")
def reuse(ctx):
    """4. every (line, triple) pair of tests/local_eq_cases.wave_reuse_batch as a point: 1.3 x the persistent grid at N = 67"""
    w = lc.wave_reuse_batch(lc.persistent_waves())
    n, nv = len(w["lines"]), len(w["var"])
    b = dict(w, line_of=np.repeat(np.arange(n), nv).astype(np.int32), var=np.tile(w["var"], (n, 1)))
    r = grad_of(ctx, b)
    lc.assert_wave_reuse(ctx, "k_local_eq_grad", len(b["var"]))
    assert len(b["var"]) >= 1.3 * lc.persistent_waves() and r["nbad"] == 0
    return b, r


def test_wave_reuse_and_independence_of_the_batch(ctx, reuse):
    """4a. every output bitwise equal to the same points in reverse order, in chunks of 1,000 points (option nearest_chunk_systems) and
    eight of them each run alone; the scan's lam and gam bits on the whole batch"""
    b, r = reuse
    n_pts = len(b["var"])
    rev = grad_of(ctx, b, b["line_of"][::-1].copy(), b["var"][::-1].copy())
    lc.assert_wave_reuse(ctx, "k_local_eq_grad", n_pts)
    ctx.set_option("nearest_chunk_systems", 1000)
    try:
        ch = grad_of(ctx, b)
        assert ctx.last_launch()[1] <= 1000
    finally:
        ctx.set_option("nearest_chunk_systems", None)
    for k in KEYS:
        rk = rev[k][:, ::-1] if k == "geo_bar" else rev[k][::-1]
        assert np.array_equal(rk, r[k], equal_nan=True), k
        assert np.array_equal(ch[k], r[k], equal_nan=True), k
    for p in np.linspace(0, n_pts - 1, 8).astype(int):
        one = grad_of(ctx, b, b["line_of"][p:p + 1], b["var"][p:p + 1])
        for k in KEYS:
            want = r[k][:, p:p + 1] if k == "geo_bar" else r[k][p:p + 1]
            assert np.array_equal(one[k], want, equal_nan=True), (p, k)
    w = lc.wave_reuse_batch(lc.persistent_waves())
    sc = ctx.local_eq_scan(b["th"][0], b["th"][1] - b["th"][0], lc.to_geo(w["lines"]), w["dP"], w["centre"], w["sigma"], w["var"], ps=w["ps"])
    assert np.array_equal(sc["lam"].ravel(), r["lam"]) and np.array_equal(sc["gam"].ravel(), r["gam"])


def test_faults_are_data(ctx, reuse):
    """5. mixed into the clean batch: a line with a NaN entry, a line with sigma = 0, non-finite triples, line_of = -1 and line_of =
    n_lines.  Exactly those points carry status bit 1 and NaN in lam, gam, dlam and entries 0 .. N-1 of their geo_bar rows; every other
    point -- their neighbours on the same wave among them -- is bitwise the clean run's.  No fault is provoked: an index out of range
    is never dereferenced"""
    b, clean = reuse
    n_pts, n_lines = len(b["var"]), len(b["lines"])
    lines = np.concatenate([b["lines"], b["lines"][:2]])     # lines 3 and 4: copies of 0 and 1, to be spoilt
    lines[3, 5, 40] = np.nan
    bad = dict(b, lines=lines, dP=np.append(b["dP"], b["dP"][:2]), centre=np.append(b["centre"], b["centre"][:2]),
               sigma=np.append(b["sigma"], [1.0, 0.0]), ps=np.concatenate([b["ps"], b["ps"][:2]]))
    line_of, var = b["line_of"].copy(), b["var"].copy()
    hit = np.zeros(n_pts, dtype=bool)
    k = np.arange(n_pts)
    line_of[k % 11 == 3] = 3; line_of[k % 11 == 7] = 4; line_of[k % 13 == 5] = -1; line_of[k % 13 == 9] = 5
    var[k % 17 == 2, 1] = np.nan; var[k % 17 == 6, 2] = np.inf
    hit = (line_of != b["line_of"]) | ~np.isfinite(var).all(axis=1)
    assert 0.2 < hit.mean() < 0.6
    r = grad_of(ctx, bad, line_of, var)
    lc.assert_wave_reuse(ctx, "k_local_eq_grad", n_pts)
    assert r["nbad"] == hit.sum(), (r["nbad"], hit.sum())
    assert (status(r)[hit] == 2).all() and (status(r)[~hit] == 0).all()
    for key in ("lam", "gam", "dlam"):
        assert np.isnan(r[key][hit]).all(), key
    assert np.isnan(r["geo_bar"][:, hit]).all()
    for key in KEYS:
        a, c = (r[key][:, ~hit], clean[key][:, ~hit]) if key == "geo_bar" else (r[key][~hit], clean[key][~hit])
        assert np.array_equal(a, c), key


def raw_grad(ctx, b, ld, ps_ld, ld_bar, device, sentinel=-7.0):
    """ibs_local_eq_grad_f64 itself on padded leading dimensions (NaN in the padding of the inputs, a sentinel in geo_bar), host pointers
    or device pointers -> (return value, outputs)"""
    import torch
    n_lines, N, n_pts = len(b["lines"]), len(b["th"]), len(b["var"])
    geo = np.full((8, n_lines, ld), np.nan); geo[:, :, :N] = lc.to_geo(b["lines"])
    ps = np.full((n_lines, ps_ld), np.nan); ps[:, :N] = b["ps"]
    ins = [np.ascontiguousarray(a, dtype=np.float64) for a in (geo, b["dP"], b["centre"], b["sigma"], ps)] + [
        np.ascontiguousarray(b["line_of"], dtype=np.int32), np.ascontiguousarray(b["var"], dtype=np.float64)]
    out = dict(lam=np.zeros(n_pts), gam=np.zeros(n_pts), dlam=np.zeros((n_pts, 4)), geo_bar=np.full((8, n_pts, ld_bar), sentinel),
               info=np.zeros(n_pts, np.int32))
    if device:
        ctx._stream_from_torch(torch.device("cuda:0"))
        ins = [torch.from_numpy(a).to("cuda:0") for a in ins]
        out = {k: torch.from_numpy(v).to("cuda:0") for k, v in out.items()}
        p = lambda a: ctypes.c_void_p(a.data_ptr())
    else:
        p = lambda a: ctypes.c_void_p(a.ctypes.data)
    rc = ctx._lib.ibs_local_eq_grad_f64(ctx._h, n_lines, n_pts, N, float(b["th"][0]), float(b["th"][1] - b["th"][0]), p(ins[0]), ld,
                                        p(ins[1]), p(ins[2]), p(ins[3]), p(ins[4]), ps_ld, p(ins[5]), p(ins[6]), p(out["lam"]),
                                        p(out["gam"]), p(out["dlam"]), p(out["geo_bar"]), ld_bar, p(out["info"]), 0 if device else 1)
    if device:
        torch.cuda.synchronize()
        out = {k: v.cpu().numpy() for k, v in out.items()}
    return rc, out


def test_padded_rows_through_the_raw_entry(ctx, g3):
    """6. ld = N + 5, ps_ld = N + 3, ld_bar = N + 7 on the NCSX batch at N = 513, from host pointers and from device pointers: the outputs
    are Context.local_eq_grad's bits on the packed arrays and the sentinel in entries N .. ld_bar-1 of every geo_bar row survives"""
    b = gc.ncsx_batch(g3)
    N = len(b["th"])
    packed = grad_of(ctx, b)
    assert packed["nbad"] == 0
    for device in (False, True):
        rc, r = raw_grad(ctx, b, N + 5, N + 3, N + 7, device)
        assert "k_local_eq_grad" in ctx.last_launch()[0]
        assert rc == 0 and not (r["info"] >> 16).any(), (device, rc)
        for k in ("lam", "gam", "dlam", "info"):
            assert np.array_equal(r[k], packed[k]), (device, k)
        assert np.array_equal(r["geo_bar"][:, :, :N], packed["geo_bar"]), device
        assert (r["geo_bar"][:, :, N:] == -7.0).all(), device


# ---- crossings ------------------------------------------------------------------------------------------------------------------------
FD = 1e-4                        # the step of the differences of t*


def test_crossings_and_their_derivatives(ctx):
    """7. Context.local_eq_boundary_grad on the three s-alpha lines with their ps rows at N = 129: two p-rays, the eps-ray and the oblique
    ray of tests/local_eq_boundary_cases.  |lam_at - shift| <= margin + |dlam_dt| (t_unstable - t_stable) at every crossing; dt in
    theta0, eps0, p0 and shift against central differences of t* from two further boundary calls each at xtol = 1e-12.
    DERIVED TOLERANCE: a closed bracket is xtol (t_hi - t_lo) wide, so a difference at step FD = 1e-4 carries a closing error of at most
    1e-12 range / FD; the truncation K FD^2 is measured by halving the step, |D(FD) - D(FD / 2)| = 3/4 K FD^2, and bounded by 4/3 of
    that plus the two closing errors (3 x 1e-12 range / FD in all); the formula's own share is DLAM_BOUND of the scale of dt (those of
    its numerator and of lam_t, propagated to first order, from the numpy formula on the oracle's eigenpair)"""
    b = lbc.salpha_lines(bo.theta_grid(129))
    rays = lbc.RAYS[[1, 2, 4, 5]]
    shift = 0.01
    args = lbc.call_args(b)
    r = ctx.local_eq_boundary_grad(*args, rays, ps=b["ps"], shift=shift)
    assert r["nbad"] == 0 and r["grad_nbad"] == 0
    nc = r["n_cross"]
    have = np.arange(4)[None, None, :] < nc[:, :, None]
    assert have.sum() >= 8 and np.isnan(r["dt"][~have]).all() and np.isnan(r["lam_at"][~have]).all() and np.isfinite(r["dt"][have]).all()
    il, ir, ic = np.nonzero(have)
    t = r["t"][il, ir, ic]
    tri = local_eq_ray_triples(rays[ir], t)
    bb = dict(b, line_of=il.astype(np.int32), var=tri)
    ref = gc.oracle_pairs(bb)
    width = np.abs(r["t_unstable"] - r["t_stable"])[have]
    off = np.abs(r["lam_at"][have] - shift)
    print("crossings: %d, max |lam_at - shift| %.2e, its bound at least %.2e" % (have.sum(), off.max(), ref["margin"].min()))
    assert (off <= ref["margin"] + np.abs(r["dlam_dt"][have]) * width).all()
    an = gc.numpy_grads(bb, ref)
    sc = an["dlam_scale"]
    lt = r["dlam_dt"][have]
    sc_t = np.abs(rays[ir, 3]) * sc[:, 1] + np.abs(rays[ir, 4]) * sc[:, 2]
    dt = r["dt"][have]
    dt_scale = np.concatenate([sc[:, :3], np.zeros((len(sc), 1))], axis=1) / np.abs(lt)[:, None] + np.abs(dt[:, :4]) * (sc_t / np.abs(lt))[:, None]
    rng = (rays[:, 6] - rays[:, 5])[ir]

    def t_of(col, step):
        rr, sh = rays.copy(), shift
        if col < 3:
            rr[:, col] += step
        else:
            sh += step
        q = ctx.local_eq_boundary(*args, rr, ps=b["ps"], shift=sh, xtol=1e-12)
        assert np.array_equal(q["n_cross"], nc)              # (the same crossings, moved)
        return q["t"][il, ir, ic]
    worst = 0.0
    for col, name in enumerate(("theta0", "eps0", "p0", "shift")):
        d1 = (t_of(col, FD) - t_of(col, -FD)) / (2 * FD)
        d2 = (t_of(col, 0.5 * FD) - t_of(col, -0.5 * FD)) / FD
        tol = 4.0 / 3.0 * np.abs(d1 - d2) + 3e-12 * rng / FD + DLAM_BOUND * dt_scale[:, col]
        err = np.abs(dt[:, col] - d2)
        print("crossings d t* / d %s: max |dt - difference| %.2e (%.2e of its tolerance), truncation measured %.2e, closing error %.2e"
              % (name, err.max(), (err / tol).max(), np.abs(d1 - d2).max(), (3e-12 * rng / FD).max()))
        worst = max(worst, (err / tol).max())
    assert worst <= 1.0
    # device tensors give the same bits, and the planes of t* are -geo_bar / lam_t of a point call at the crossings
    import torch
    t_ = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    d = ctx.local_eq_boundary_grad(args[0], args[1], t_(args[2]), t_(args[3]), args[4], args[5], rays, ps=t_(b["ps"]), shift=shift, want_geo_bar=True)
    for k in ("t", "lam_at", "dlam_dt", "dt"):
        assert np.array_equal(d[k].cpu().numpy(), r[k], equal_nan=True), k
    g = grad_of(ctx, bb)
    assert np.array_equal(d["pts"], np.stack([il, ir, ic], axis=1))
    assert np.array_equal(d["dt_geo"].cpu().numpy(), g["geo_bar"] * (-1.0 / lt)[None, :, None])


def test_autograd_crossing_is_the_implicit_rule(ctx):
    """7b. autograd.local_eq_crossing: t* is the first stable -> unstable crossing of local_eq_boundary_grad, and backward of sum(t*) gives
    its dt in the rays' (theta0, eps0, p0) summed over the lines, its dt in dPdrho summed over the rays and its planes summed per line"""
    import torch
    from ibs_amd import autograd as iag
    b = lbc.salpha_lines(bo.theta_grid(129))
    rays = lbc.RAYS[[1, 2, 5]]
    args = lbc.call_args(b)
    t_ = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    geo, dP, rr = t_(args[2]).requires_grad_(True), t_(args[3]).requires_grad_(True), t_(rays).requires_grad_(True)
    t = iag.local_eq_crossing(args[0], args[1], geo, dP, args[4], args[5], rr, ps=t_(b["ps"]), ctx=ctx)
    r = ctx.local_eq_boundary_grad(*args, rays, ps=b["ps"], want_geo_bar=True)
    up = r["t_stable"] < r["t_unstable"]
    first = up.argmax(axis=2)
    has = up.any(axis=2)
    assert has.all()
    il, ir = np.nonzero(has)
    assert np.array_equal(t.detach().cpu().numpy(), r["t"][il, ir, first[il, ir]].reshape(has.shape))
    t.sum().backward()
    dt = r["dt"][il, ir, first[il, ir]].reshape(has.shape + (5,))
    tt = r["t"][il, ir, first[il, ir]].reshape(has.shape)
    want = np.stack([dt[..., 0], dt[..., 1], dt[..., 2], tt * dt[..., 1], tt * dt[..., 2]], axis=-1).sum(axis=0)
    got = rr.grad.cpu().numpy()
    assert np.abs(got[:, :5] - want).max() <= 1e-13 * np.abs(want).max() and not got[:, 5:].any()
    assert np.abs(dP.grad.cpu().numpy() - dt[..., 4].sum(axis=1)).max() <= 1e-13 * np.abs(dt[..., 4]).max()
    sel = {tuple(p): k for k, p in enumerate(r["pts"].tolist())}
    planes = np.zeros_like(args[2])
    for l, q in zip(il, ir):
        planes[:, l] += r["dt_geo"][:, sel[(l, q, first[l, q])]]
    assert np.abs(geo.grad.cpu().numpy() - planes).max() <= 1e-13 * np.abs(planes).max()


# ---- the driver -----------------------------------------------------------------------------------------------------------------------
def test_scan_driver_sensitivity_on_ncsx_tables(ctx):
    """8. BallooningScan.local_eq_boundary_sensitivity on the G8 wout tables (2 surfaces, the 8 x 5 coarse grid of the other driver
    tests, N = 513, p-rays over (0, 3) at eps = -0.5 and 0): first_unstable and the raw arrays are local_eq_boundary's; the derivative in
    the scal column d_pressure_d_s against central differences of first_unstable with that column scaled by 1 -+ 1e-4 and 1 -+ 5e-5,
    asserted on the (surface, eps) pairs where all four perturbed runs keep the attaining (alpha, theta0) -- at least one; tolerance as
    in test 7: 4/3 of the measured truncation, the closing errors 3e-12 range / step, and 1e-6 of |derivative| for the formula (the mode's
    bound; no numpy oracle runs through the geometry here); dfirst_dfixed and dfirst_dshift the same way"""
    import torch
    import ibs_amd
    dev = torch.device("cuda:0")
    N = 513
    th = np.linspace(-4 * np.pi, 4 * np.pi, N)
    svals = np.array([0.6, 0.9])
    wout = dict(np.load(os.path.join(G, "G8_wout_ncsx_op.npz")))
    eps, rng = np.array([-0.5, 0.0]), (0.0, 3.0)

    def scan_of(scale=1.0):
        tabs = ibs_amd.SurfaceTables.from_wout(wout, svals)
        tabs.scal[:, 3] *= scale
        return ibs_amd.BallooningScan(ctx, None, th, svals, nalpha=8, ntheta0=5, tables=tabs, device=dev)
    scan = scan_of()
    r = scan.local_eq_boundary_sensitivity(eps, rng)
    base = scan.local_eq_boundary(eps, rng)
    for k in ("t_stable", "t_unstable", "t", "n_cross", "lo_unstable", "first_unstable"):
        assert np.array_equal(r[k], base[k], equal_nan=True), k
    assert r["mask"].shape == (2, 2) and tuple(r["scal_bar"].shape) == (2, 2, 6) and tuple(r["tab_mn_bar"].shape)[:3] == (2, 2, 6)
    m = r["mask"]
    assert m.any() and np.array_equal(m, np.isfinite(base["first_unstable"]) & ~(base["lo_unstable"] > 0).any(axis=(1, 2)))
    # (lam_max at the midpoint of a bracket 3e-12 wide: within the count margin 16 N^2 eps ||A|| ~ 7e-8 of the shift on these lines)
    assert (np.abs(r["lam_at"][m]) <= 1e-6).all() and (r["dlam_dt"][m] > 0).all()
    assert not r["dfirst_dfixed"][~m].any() and not r["scal_bar"].cpu().numpy()[~m].any()

    def where_of(q):
        cand = np.where(q["t_stable"] < q["t_unstable"], q["t"], np.inf)
        return np.moveaxis(cand, 3, 1).reshape(2, 2, -1).argmin(axis=2)
    w0 = where_of(base)
    step = 1e-4
    runs = {s: scan_of(1.0 + s).local_eq_boundary(eps, rng) for s in (step, -step, 0.5 * step, -0.5 * step)}
    same = np.all([where_of(q) == w0 for q in runs.values()], axis=0) & m
    print("driver: first_unstable %s, attaining line kept on %d of 4 (surface, eps) pairs" % (r["first_unstable"].tolist(), same.sum()))
    assert same.sum() >= 1
    d1 = (runs[step]["first_unstable"] - runs[-step]["first_unstable"]) / (2 * step)
    d2 = (runs[0.5 * step]["first_unstable"] - runs[-0.5 * step]["first_unstable"]) / step
    # d / d (relative change of the column) = scal_bar[..., 3] x the column
    got = r["scal_bar"].cpu().numpy()[..., 3] * np.asarray(scan.tables.scal)[scan._own_surf(), 3][:, None]
    tol = 4.0 / 3.0 * np.abs(d1 - d2) + 3e-12 * 3.0 / step + 1e-6 * np.abs(got)
    err = np.abs(got - d2)
    print("driver d first_unstable / d ln(d_pressure_d_s): %s, differences %s, |err| / tol %s" % (got.tolist(), d2.tolist(), (err / tol).tolist()))
    assert (err[same] <= tol[same]).all()
    # the fixed value and the shift, by differences of the same driver call
    for name, run in (("dfirst_dfixed", lambda s: scan.local_eq_boundary(eps + s, rng)),
                      ("dfirst_dshift", lambda s: scan.local_eq_boundary(eps, rng, shift=s))):
        q = {s: run(s) for s in (step, -step, 0.5 * step, -0.5 * step)}
        keep = np.all([where_of(v) == w0 for v in q.values()], axis=0) & m
        d1 = (q[step]["first_unstable"] - q[-step]["first_unstable"]) / (2 * step)
        d2 = (q[0.5 * step]["first_unstable"] - q[-0.5 * step]["first_unstable"]) / step
        tol = 4.0 / 3.0 * np.abs(d1 - d2) + 3e-12 * 3.0 / step + 1e-6 * np.abs(r[name])
        err = np.abs(r[name] - d2)
        print("driver %s: %s, differences %s, |err| / tol %s" % (name, r[name].tolist(), d2.tolist(), (err / tol).tolist()))
        assert keep.any() and (err[keep] <= tol[keep]).all(), name
