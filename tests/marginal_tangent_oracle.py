"""CPU restatement of ibs_marginal_obj_w_grad_tangent_f64 (the margin at geometry-fed points from ONE line per point, its gradient exact
in (alpha, theta0), and the cotangent planes geo_bar = d s* / d (the eight arrays)), from the pieces of tests/marginal_oracle.py (the
line's rows, mo.solve, mo.grad_rows, the theta0 tangent), geometry_tangent_oracle.rows_dalpha (the alpha tangent of the rows at fixed
dPdrho) and the closed form of the cotangent planes:

  with m = -dPdrho = mean((cvdrift - gbdrift) bmag^2) / 2, a = |gradpar|, B = bmag, g = a d / B, c = m (cvdrift + theta0 cvdrift0) / (a B),
  d = gds2 + 2 theta0 gds21 + theta0^2 gds22, the rows' cotangents g_bar, c_bar of mo.grad_rows and kappa = d s* / d m = -s* / m
  (sum c_bar_j c_j = -s*, c linear in m):
    bmag     -g_bar g / B - c_bar c / B + kappa B (cvdrift - gbdrift) / N        gradpar   sgn(gradpar) (g_bar g - c_bar c) / a
    cvdrift  c_bar m / (a B) + kappa B^2 / (2 N)                                 cvdrift0  theta0 c_bar m / (a B)
    gds2     g_bar a / B          gds21   2 theta0 g_bar a / B                   gds22     theta0^2 g_bar a / B
    gbdrift  -kappa B^2 / (2 N)

Test infrastructure only."""
import numpy as np

from oracle import ballooning_oracle as bo
from tests import geometry_tangent_oracle as to
from tests import marginal_oracle as mo


def scale_of_line(h, line, t0):
    """s* of one line (8, N) at theta0, through the line's own dPdrho: the function whose derivatives point() returns"""
    return mo.solve(h, *mo.line_gc(bo.dPdrho_of(line[2], line[7], line[0]), *line[:7], t0))["scale"]


def geo_bar_of(h, line, t0, r, g, c):
    """the closed form of the module docstring: (8, N) from solve()'s result r on the rows (g, c) of `line`"""
    N = line.shape[1]
    gb, cb = mo.grad_rows(h, r)
    B, a, sgn = line[0], np.abs(line[1]), np.sign(line[1])
    m = -bo.dPdrho_of(line[2], line[7], line[0])
    kap = -r["scale"] / m
    out = np.empty((8, N))
    out[0] = -gb * g / B - cb * c / B + kap * B * (line[2] - line[7]) / N
    out[1] = sgn * (gb * g - cb * c) / a
    out[2] = cb * m / (a * B) + kap * B ** 2 / (2 * N)
    out[3] = t0 * cb * m / (a * B)
    out[4] = gb * a / B
    out[5] = 2 * t0 * gb * a / B
    out[6] = t0 ** 2 * gb * a / B
    out[7] = -kap * B ** 2 / (2 * N)
    return out


def point(h, line, line_da, t0, want_grad=True, want_geo_bar=True):
    """one point: line (8, N), line_da (8, N) or None (then no alpha component: want_grad must be False).
    dict(val = -1 / s*, scale, dPdrho, u (0 with scale = inf), info[, jac (2,), dscale (2,)][, geo_bar (8, N)])"""
    N = line.shape[1]
    dP = bo.dPdrho_of(line[2], line[7], line[0])
    g, c = mo.line_gc(dP, *line[:7], t0)
    r = mo.solve(h, g, c)
    out = dict(val=0.0 - r["mu"], scale=r["scale"], dPdrho=dP, u=r.get("u", 0.0), info=0)
    if r["X"] is None:
        out.update(info=256 << 16, val=0.0)
        if want_grad:
            out.update(jac=np.zeros(2), dscale=np.zeros(2))
        if want_geo_bar:
            out.update(geo_bar=np.zeros((8, N)))
        return out
    if want_grad:
        gb, cb = mo.grad_rows(h, r)
        gt, ct = mo.theta0_tangent(line[0], line[1], line[3], line[5], line[6], dP, t0)
        g_a, c_a, _ = to.rows_dalpha(line[:, None, :], line_da[:, None, :], np.array([t0]))
        ds = np.array([float(np.sum(gb * g_a[0] + cb * c_a[0])), float(np.sum(gb * gt + cb * ct))])
        out.update(dscale=ds, jac=ds / r["scale"] ** 2)
    if want_geo_bar:
        out.update(geo_bar=geo_bar_of(h, line, t0, r, g, c))
    return out


def points(h, geo, geo_da, theta0, want_grad=True, want_geo_bar=True):
    """the batch: geo, geo_da (8, n, N), theta0 (n,) -> dict of arrays (val, scale, dPdrho, u, info[, jac, dscale][, geo_bar (8, n, N)])"""
    n = geo.shape[1]
    rs = [point(h, geo[:, k], None if geo_da is None else geo_da[:, k], float(theta0[k]), want_grad, want_geo_bar) for k in range(n)]
    out = {key: np.array([r[key] for r in rs]) for key in ("val", "scale", "dPdrho", "u")}
    out["info"] = np.array([r["info"] for r in rs], dtype=np.int32)
    if want_grad:
        out.update(jac=np.array([r["jac"] for r in rs]).reshape(n, 2), dscale=np.array([r["dscale"] for r in rs]).reshape(n, 2))
    if want_geo_bar:
        out.update(geo_bar=np.ascontiguousarray(np.stack([r["geo_bar"] for r in rs], axis=1)))
    return out


# ---- analytic test lines: tests.helpers.synthetic_fieldlines (analytic in alpha), with their own dPdrho ----------------------------
def lines_at(th, pts, shift=0.0):
    """(8, n, N): the synthetic field line of every point (s, alpha, ...) at alpha + shift"""
    from tests.helpers import synthetic_fieldlines
    base = synthetic_fieldlines(th)
    return np.ascontiguousarray(np.stack([base(p[0], np.array([p[1] + shift]))[0] for p in pts], axis=1))


def tangent_planes(th, pts):
    """d/d alpha of lines_at by the Richardson scheme of tests/test_gpu_exact_tangent.py: tangent_planes (central differences at 1e-3,
    5e-4, 2.5e-4; the two first-level combinations must agree to 1e-9 of the plane maximum everywhere)"""
    fd = lambda t: (lines_at(th, pts, t) - lines_at(th, pts, -t)) / (2 * t)
    f1, f2, f4 = fd(1e-3), fd(5e-4), fd(2.5e-4)
    r1, r1h = (4.0 * f2 - f1) / 3.0, (4.0 * f4 - f2) / 3.0
    scale = np.abs(r1h).max(axis=(1, 2), keepdims=True)
    ok = np.abs(r1 - r1h) <= 1e-9 * np.where(scale > 0, scale, 1.0)
    assert ok.all(), (int((~ok).sum()), np.abs(r1 - r1h).max(axis=(1, 2)) / np.where(scale > 0, scale, 1.0)[:, 0, 0])
    return (16.0 * r1h - r1) / 15.0
