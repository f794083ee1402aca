"""CPU: the local-equilibrium gradients without a GPU -- the row tangents (ibs_amd.local_eq_fold_tangent), the Hellmann-Feynman
derivatives of lam_max (ibs_amd.local_eq_lam_grad) against central differences of the C oracle's lam_max, the implicit-function rule for
a crossing t*, and the argument rules of ibs_local_eq_grad_f64.

HOW A DIFFERENCE IS JUDGED.  D(d) = (lam(s + d) - lam(s - d)) / (2 d) = lam_s + K d^2 + K4 d^4 + r, |r| <= 2 tol_lam / (2 d) with tol_lam =
4 N eps ||A|| the oracle's own bound (tests/local_eq_cases.oracle_of).  Three steps d, d/2, d/4 give the Richardson extrapolates R1 =
(4 D(d/2) - D(d)) / 3 and R2 = (4 D(d/4) - D(d/2)) / 3, whose d^4 remainders differ 16-fold, so |R1 - R2| bounds R2's fifteen times over;
R2's rounding is (4 r(d/4) + r(d/2)) / 3 <= 6 tol_lam / d.  The formula itself is first order in the error of the oracle's mode, which
is an eigenvector to tol_lam / gap with gap >= 1e-6 ||A|| (the condition on the inputs): 2 x 4 N eps 1e6 of the component's scale.  So
    |formula - R2| <= |R1 - R2| + 6 tol_lam / d + 8e6 N eps scale,
nothing of which comes from the formula under test.  Truncation is SHOWN by e(d) / e(d/2) with e = |formula - D|: where e(d) is at least
20 times everything but truncation, (K d^2 -+ F) / (K d^2 / 4 +- F) lies in [3.1, 5.6]; asserted as [3, 5.7] wherever that holds."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ibs_amd
from ibs_amd import _lib, local_eq_fold, local_eq_fold_tangent, local_eq_lam_grad, local_eq_ray_nodes, local_eq_ray_triples
from tests import local_eq_boundary_cases as lbc
from tests import local_eq_cases as lc
from tests import local_eq_grad_cases as gc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(os.path.dirname(__file__), "golden")
IBS_ERR_ARG, IBS_ERR_UNSUPPORTED = -1, -3
NAME = "ibs_local_eq_grad_f64"
EPS = lc.EPS
D0 = 0.008                       # the largest of the three steps


@pytest.fixture(scope="module")
def g3():
    return np.load(os.path.join(G, "G3_ncsx_lines.npz"))


def batches(g3):
    yield "s-alpha N=67 ps", gc.salpha_batch(67, True)
    yield "s-alpha N=67", gc.salpha_batch(67, False)
    yield "s-alpha N=129 ps", gc.salpha_batch(129, True)
    yield "s-alpha N=129", gc.salpha_batch(129, False)


def fold_magnitude(th, line8, par, ps):
    """the three results of local_eq_fold with every term replaced by its magnitude, per grid point: what their rounding is relative to"""
    dP, centre, _, t0, e, p = par
    cv, cv0, gds2, gds21, gds22, gb = (np.abs(line8[k]) for k in (2, 3, 4, 5, 6, 7))
    x = abs(t0) * (1 + abs(e)) + np.abs(e * (th - centre)) + (0.0 if ps is None else np.abs((p - 1.0) * ps))
    return np.full_like(th, abs(p * dP)), gb + abs(p) * (cv + gb) + x * cv0, gds2 + 2 * x * gds21 + x * x * gds22


def test_row_tangents_against_differences_of_the_fold(g3):
    """local_eq_fold_tangent against central differences of local_eq_fold at two step sizes on every point of the s-alpha batches and
    of four NCSX lines at N = 513: the results are polynomials of degree <= 2 in each parameter, so a central difference is exact and
    the two steps agree with the tangent to rounding.  A result is a sum of at most three products of at most three factors, formed
    with at most eight roundings: each evaluation is within 8 eps of the sum of the magnitudes of its terms (fold_magnitude), and the
    difference of two within 8 eps (that sum, at the larger of the two) / step"""
    worst = 0.0
    for what, b in list(batches(g3)) + [("NCSX N=513", gc.ncsx_batch(g3))]:
        for l, (t0, e, p) in zip(b["line_of"], b["var"]):
            ps = None if b["ps"] is None else b["ps"][l]
            base = (b["th"], b["lines"][l])
            par = [b["dP"][l], b["centre"][l], b["sigma"][l], t0, e, p]
            tan = local_eq_fold_tangent(*base, *par, ps=ps)
            for s, k in enumerate((3, 4, 5, 0)):             # theta0, eps, p, dPdrho in the argument list
                for d in (0.25, 0.0625):
                    hi, lo = list(par), list(par)
                    hi[k] += d; lo[k] -= d
                    fd = [(np.asarray(a) - np.asarray(c)) / (2 * d) for a, c in zip(local_eq_fold(*base, *hi, ps=ps), local_eq_fold(*base, *lo, ps=ps))]
                    mag = [np.maximum(a, c) for a, c in zip(fold_magnitude(*base, hi, ps), fold_magnitude(*base, lo, ps))]
                    for r in range(3):
                        err = (np.abs(fd[r] - tan[r][s]) / (8 * EPS * mag[r] / d + 1e-300)).max()
                        worst = max(worst, err)
                        assert err <= 1.0, (what, l, s, d, r, err)
    print("row tangents: worst |difference - tangent| / (8 eps scale / step) %.2e" % worst)


def judged(an, scale, lam_of, tol_lam, N, what):
    """the rule of the module docstring for a vector of components; prints the figures; returns (worst ratio to the tolerance, number of
    components whose truncation was shown)"""
    R1, d1, d2 = gc.richardson(lam_of, D0)
    R2, _, d3 = gc.richardson(lam_of, 0.5 * D0)
    rest = 6 * tol_lam / D0 + 8e6 * N * EPS * scale
    tol = np.abs(R1 - R2) + rest
    err = np.abs(an - R2)
    e1, e2 = np.abs(an - d2), np.abs(an - d3)
    shown = e1 >= 20 * (4 * tol_lam / D0 + 8e6 * N * EPS * scale)      # (the rounding of D(d/2), D(d/4) is at most 4 tol_lam / d)
    ratio = e1[shown] / e2[shown]
    print("%s: max |formula - R2| %.2e (%.2e of its tolerance, %.2e of its scale); truncation shown on %d of %d, e(d/2) / e(d/4) in "
          "[%.2f, %.2f]" % (what, err.max(), (err / tol).max(), (err / np.maximum(scale, 1e-300)).max(), shown.sum(), shown.size,
                            ratio.min() if shown.any() else np.nan, ratio.max() if shown.any() else np.nan))
    assert (err <= tol).all(), (what, (err / tol).max())
    assert ((ratio >= 3.0) & (ratio <= 5.7)).all(), (what, ratio)
    return (err / tol).max(), int(shown.sum())


def test_parameter_derivatives_against_differences_of_the_oracle(g3):
    """d lam / d (theta0, eps, p, dPdrho) of local_eq_lam_grad on the oracle's eigenpair against differences of the oracle's lam_max, by
    the rule of the module docstring, on the dozen points of every s-alpha batch at N = 67 and 129 and of the NCSX lines at N = 513"""
    total = 0
    for what, b in list(batches(g3)) + [("NCSX N=513", gc.ncsx_batch(g3))]:
        ref = gc.oracle_pairs(b)
        an = gc.numpy_grads(b, ref)
        for s, name in enumerate(("theta0", "eps", "p", "dPdrho")):
            def lam_of(step, s=s):
                var, dP = b["var"].copy(), b["dP"][b["line_of"]].copy()
                if s < 3:
                    var[:, s] += step
                else:
                    dP += step * np.abs(dP)                  # (relative: the NCSX dPdrho are small)
                return gc.oracle_lam(b, b["line_of"], var, dP=dP)
            w = np.abs(b["dP"][b["line_of"]]) if s == 3 else 1.0
            total += judged(an["dlam"][:, s] * w, an["dlam_scale"][:, s] * w, lam_of, ref["tol_lam"], len(b["th"]), "%s d/d%s" % (what, name))[1]
    assert total > 0                                         # (the fourfold fall was seen somewhere)


def test_array_derivatives_against_differences_of_the_oracle(g3):
    """geo_bar of local_eq_lam_grad against differences of the oracle's lam_max in SINGLE entries of each of the eight arrays, at j = 0, 1,
    N - 2, N - 1 and three interior points, on the first three points (one per line) of every s-alpha batch at N = 67 and 129.  The step
    is relative to the entry, or absolute where the entry is below 1"""
    for what, b in batches(g3):
        N = len(b["th"])
        js = np.array([0, 1, N - 2, N - 1, N // 2, N // 2 + 7, N // 3])
        pts = np.arange(3)
        line_of, var = b["line_of"][pts], b["var"][pts]
        ref = gc.oracle_pairs(b, line_of, var)
        an = gc.numpy_grads(b, ref, line_of, var)
        P, K, J = np.meshgrid(pts, np.arange(8), js, indexing="ij")
        P, K, J = P.ravel(), K.ravel(), J.ravel()
        base = b["lines"][line_of[P]]                        # (n, 8, N): one copy of the line per perturbed entry
        unit = np.maximum(1.0, np.abs(base[np.arange(len(P)), K, J]))

        def lam_of(step):
            lines = base.copy()
            lines[np.arange(len(P)), K, J] += step * unit
            return gc.oracle_lam(b, line_of[P], var[P], lines=lines)
        judged(an["geo_bar"][P, K, J] * unit, an["geo_bar_scale"][P, K, J] * unit, lam_of, ref["tol_lam"][P], N, "%s d/d(entries)" % what)


def first_crossing(b, line, ray, shift):
    """t* of the first stable -> unstable crossing of one (line, ray) by bisection on the oracle's count, from the first such flip between
    two of the 64 nodes down to neighbouring doubles or 60 halvings"""
    one = dict(b, lines=b["lines"][line:line + 1], dP=b["dP"][line:line + 1], centre=b["centre"][line:line + 1],
               sigma=b["sigma"][line:line + 1], ps=None if b["ps"] is None else b["ps"][line:line + 1])
    nodes = local_eq_ray_nodes(ray[None])
    un = lbc.oracle_at(one, ray[None], nodes[None], shift)["count"][0, 0] > 0
    up = [k for k in lbc.flips(un) if not un[k]]
    assert up, "no stable -> unstable flip on the ray"
    lo, hi = nodes[0, up[0]], nodes[0, up[0] + 1]
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        if not lo < mid < hi:
            break
        if lbc.oracle_at(one, ray[None], np.array([[[mid]]]), shift)["count"][0, 0, 0] > 0:
            hi = mid
        else:
            lo = mid
    return 0.5 * (lo + hi)


def test_implicit_rule_against_differences_of_the_bisected_crossing():
    """d t* / d (theta0, eps0, p0, shift) = (-lam_theta0, -lam_eps, -lam_p, 1) / lam_t from local_eq_lam_grad at the bisected t*, against
    central differences of t* itself, on the s-alpha line theta0 = 0.1 with its ps row at N = 67: a p-ray, an eps-ray and an oblique ray.
    The count flips where lam_max is within margin = 16 N^2 eps ||A|| of the shift, so a bisected t* is off by at most margin / |lam_t| and
    the rule of the module docstring holds with that in place of tol_lam"""
    from oracle import c_oracle as co
    b = lbc.salpha_lines(gc.bo.theta_grid(67))
    line, shift = 1, 0.0
    h = float(b["th"][1] - b["th"][0])
    for ray in lbc.RAYS[[2, 4, 5]]:
        t = first_crossing(b, line, ray, shift)
        tri = local_eq_ray_triples(ray, t)
        bb = dict(b, line_of=np.array([line]), var=tri[None])
        ref = gc.oracle_pairs(bb)
        an = gc.numpy_grads(bb, ref)
        dl, sc = an["dlam"][0], an["dlam_scale"][0]
        lam_t = ray[3] * dl[1] + ray[4] * dl[2]
        dt = np.array([-dl[0], -dl[1], -dl[2], 1.0]) / lam_t
        # the scale of a component of dt: that of its numerator and of lam_t, each over its own magnitude (first-order propagation)
        sc_t = ray[3] * sc[1] + ray[4] * sc[2]
        dt_scale = np.array([sc[0], sc[1], sc[2], 0.0]) / abs(lam_t) + np.abs(dt) * sc_t / abs(lam_t)
        one = dict(b, lines=b["lines"][line:line + 1], dP=b["dP"][line:line + 1], centre=b["centre"][line:line + 1],
                   sigma=b["sigma"][line:line + 1], ps=b["ps"][line:line + 1])
        side = lbc.oracle_at(one, ray[None], np.array([[[t - 1e-3, t + 1e-3]]]), shift)["lam"][0, 0]
        lam_t_ref = (side[1] - side[0]) / 2e-3               # (the oracle's own slope along the ray: the bound uses nothing of the formula)
        assert lam_t_ref > 0 and abs(lam_t / lam_t_ref - 1.0) < 0.05, (lam_t, lam_t_ref)
        t_err = ref["margin"][0] / (0.9 * lam_t_ref)
        assert abs(ref["lam"][0] - shift) <= ref["margin"][0] + ref["tol_lam"][0], (ref["lam"][0], ref["margin"][0])

        def t_of(step):
            out = []
            for s in range(4):
                r2, sh = ray.copy(), shift
                if s < 3:
                    r2[s] += step
                else:
                    sh += step
                out.append(first_crossing(b, line, r2, sh))
            return np.array(out)
        judged(dt, dt_scale, t_of, np.full(4, t_err), 67, "implicit rule, ray %s" % (ray[:5].tolist(),))


def test_arguments_are_checked_before_any_device_work():
    """the name is declared in include/ibs.h and exported; even N, N = 65 and N = 65,539: IBS_ERR_UNSUPPORTED; a NULL required pointer, no
    output at all, ld < N, ps_ld < N, ld_bar < N with geo_bar, n_pts < 0, n_lines < 0, flags not a memory kind: IBS_ERR_ARG; n_pts = 0 does
    nothing and returns 0.  The checks come before the context is touched, so a zeroed buffer stands for it and for the arrays."""
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ibs.h")).read(), flags=re.S)
    assert "int %s(" % NAME in hdr and NAME in _lib.SYMBOLS
    lib = _lib.lib()
    fn = getattr(lib, NAME)
    buf = C.create_string_buffer(1 << 16)
    P = C.cast(buf, C.c_void_p)
    N = 513

    def call(ctx=P, n=N, ld=None, geo=P, dP=P, centre=P, sigma=P, ps=None, ps_ld=None, line_of=P, var=P, lam=P, gam=P, dlam=P, geo_bar=None,
             ld_bar=None, n_pts=1, n_lines=1, flags=0):
        return fn(ctx, n_lines, n_pts, n, -1.0, 0.05, geo, n if ld is None else ld, dP, centre, sigma, ps, n if ps_ld is None else ps_ld,
                  line_of, var, lam, gam, dlam, geo_bar, n if ld_bar is None else ld_bar, None, flags)

    for kw in (dict(ctx=None), dict(geo=None), dict(dP=None), dict(centre=None), dict(sigma=None), dict(line_of=None), dict(var=None)):
        assert call(**kw) == IBS_ERR_ARG, kw
        assert b"null" in lib.ibs_last_error()
    assert call(lam=None, gam=None, dlam=None) == IBS_ERR_ARG
    assert call(ld=N - 1) == IBS_ERR_ARG
    assert call(ps=P, ps_ld=N - 1) == IBS_ERR_ARG
    assert call(geo_bar=P, ld_bar=N - 1) == IBS_ERR_ARG
    assert call(n_pts=-1) == IBS_ERR_ARG and call(n_lines=-1) == IBS_ERR_ARG
    assert call(flags=2) == IBS_ERR_ARG
    for n in (512, 65, 65539):
        assert call(n=n) == IBS_ERR_UNSUPPORTED, n
    before = bytes(buf.raw)
    assert call(n_pts=0) == 0 and bytes(buf.raw) == before   # (nothing read into, nothing written, the zeroed "context" untouched)


def test_gradient_driver_needs_the_resident_path():
    """BallooningScan.local_eq_boundary_sensitivity without tables= and device=: ValueError before any device work; an unknown axis too"""
    th = np.linspace(-4 * np.pi, 4 * np.pi, 513)
    svals = np.array([0.6, 0.9])
    scan = ibs_amd.BallooningScan(None, None, th, svals, nalpha=3, ntheta0=2)
    with pytest.raises(ValueError):
        scan.local_eq_boundary_sensitivity([0.0], (0.2, 3.0))
    tabs = ibs_amd.SurfaceTables.from_wout(dict(np.load(os.path.join(G, "G8_wout_ncsx_op.npz"))), svals)
    with pytest.raises(ValueError):
        ibs_amd.BallooningScan(None, None, th, svals, nalpha=3, ntheta0=2, tables=tabs, device="cuda:0").local_eq_boundary_sensitivity(
            [0.0], (0.2, 3.0), axis="q")
