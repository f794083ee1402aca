"""Test-only: inputs, the oracle side and the host-driven side of the tests of the local-equilibrium boundaries minimised over theta0
(tests/test_local_eq_boundary_polish_cpu.py, tests/test_gpu_local_eq_boundary_polish.py).  The lines and the ray families are those of
tests/local_eq_boundary_cases.py; entry 0 of a family is ignored by the rule (csrc/ibs_local_eq_boundary_polish.hpp)."""
import numpy as np

import ibs_amd
from ibs_amd import scan as sc
from tests import local_eq_boundary_cases as bc
from tests import local_eq_cases as lc

THETA0 = np.array([-0.5, -0.2, 0.1, 0.4])     # the coarse theta0 nodes
FAMILIES = bc.RAYS                             # four p-rays at shat = 0.1, 0.3, 0.9, 1.9, the eps-ray and the oblique ray
P_ROWS = (1, 2, 3)                             # the p-ray families with an interior valley in theta0: shat = 0.3, 0.9, 1.9


def rays_at(fam, theta0):
    """the families (n, 7) as rays folded at theta0 (a scalar or (n,))"""
    r = np.array(fam, dtype=np.float64, ndmin=2).copy()
    r[:, 0] = theta0
    return r


def one_line(b, i):
    return dict({k: b[k][i:i + 1] for k in ("lines", "dP", "centre", "sigma", "ps")}, th=b["th"])


def oracle_first_up(b, i, fam, u, shift=0.0, xtol=1e-10):
    """T of family fam (7,) at theta0 = u on line i of b from the C oracle's division-form count: the verdicts at the 64 nodes, then
    bisection of the first flip to xtol (t_hi - t_lo).  t_lo where the ray is unstable at t_lo, +inf without a flip."""
    ray = rays_at(fam, u)
    one = one_line(b, i)
    nodes = ibs_amd.local_eq_ray_nodes(ray)                                   # (1, 64)
    unst = bc.oracle_at(one, ray, nodes[None], shift)["count"][0, 0] > 0
    if unst[0]:
        return float(ray[0, 5])
    fl = bc.flips(unst)
    if not len(fl):
        return np.inf
    a, c = nodes[0, fl[0]], nodes[0, fl[0] + 1]
    tol = xtol * (ray[0, 6] - ray[0, 5])
    while c - a > tol:
        m = 0.5 * (a + c)
        if bc.oracle_at(one, ray, np.array([[[m]]]), shift)["count"][0, 0, 0] > 0:
            c = m
        else:
            a = m
    return 0.5 * (a + c)


def coarse_rows(ctx, b, fam, theta0, shift=0.0, xtol=1e-12):
    """T at the nodes, (n_lines, n_fam, n_theta0), from ONE Context.local_eq_boundary(max_cross=1) call on every (family, node) ray"""
    fam = np.asarray(fam, dtype=np.float64)
    rays = np.concatenate([rays_at(fam, t) for t in theta0])                  # node-major
    r = ctx.local_eq_boundary(*bc.call_args(b), rays, ps=b["ps"], shift=shift, max_cross=1, xtol=xtol, want_info=True)
    T = ibs_amd.local_eq_first_up(r["t_stable"], r["t_unstable"], r["lo_unstable"], rays[None, :, 5])
    return np.ascontiguousarray(np.transpose(T.reshape(len(b["lines"]), len(theta0), len(fam)), (0, 2, 1)))


def host_polish(ctx, b, i, fam, theta0, row, node, shift=0.0, xtol=1e-12, xtol_theta0=1e-5, max_eval=32):
    """the rule driven from the host for ONE slot: ibs_amd.scan.polish_first_up with every evaluation a one-ray
    Context.local_eq_boundary(max_cross=1) call on line i at the requested theta0"""
    one = one_line(b, i)
    args = bc.call_args(one)

    def boundary(u):
        r = ctx.local_eq_boundary(*args, rays_at(fam, u), ps=one["ps"], shift=shift, max_cross=1, xtol=xtol, want_info=True)
        return r["t_stable"][0, 0, 0], r["t_unstable"][0, 0, 0], r["lo_unstable"][0, 0], r["info"][0, 0] >> 16

    return sc.polish_first_up(boundary, theta0, row, node, float(fam[5]), xtol=xtol_theta0, max_eval=max_eval)


def run_polish(ctx, b, fam, theta0, t_row, **kw):
    kw = dict(dict(ps=b["ps"], shift=0.0, xtol=1e-12), **kw)
    return ctx.local_eq_boundary_polish(*bc.call_args(b), np.asarray(fam, dtype=np.float64), np.asarray(theta0, dtype=np.float64), t_row, **kw)


def status(r):
    return np.asarray(r["info"]) >> 16
