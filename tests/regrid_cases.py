"""Non-uniform theta grids and s-alpha lines for the regrid tests (test_regrid_cpu.py, test_gpu_regrid.py).  Every grid has N points on
[-4 pi, 4 pi] with exactly the end points of the uniform grid, and is strictly increasing."""
import numpy as np

from oracle import ballooning_oracle as bo
from tests import edge_cases as ec

KINDS = ("random", "clustered", "hits", "sinh", "uniform")
EPS = np.finfo(np.float64).eps


def grid(kind, N):
    tu = bo.theta_grid(N)
    if kind == "uniform":
        return tu
    if kind == "random":                 # spacings 0.2 .. 1.8 of uniform
        th = ec.geo_nonuniform_grid(N)
    elif kind == "clustered":            # log-uniform spacings over 0.02 .. 5 before normalisation: several uniform nodes in one
        rng = np.random.default_rng(11 + N)       # sample interval and many samples in one uniform cell
        d = np.exp(rng.uniform(np.log(0.02), np.log(5.0), N - 1))
        th = tu[0] + (tu[-1] - tu[0]) * np.concatenate([[0.0], np.cumsum(d)]) / d.sum()
    elif kind == "hits":                 # every even node hits a sample exactly: the x == xp[k] branch
        th = tu.copy()
        th[1:-1:2] += 0.4 * (tu[1] - tu[0])
    elif kind == "sinh":                 # packed round 0
        th = 4 * np.pi * np.sinh(3 * np.linspace(-1.0, 1.0, N)) / np.sinh(3.0)
    else:
        raise ValueError(kind)
    th = np.array(th, dtype=np.float64)
    th[0], th[-1] = tu[0], tu[-1]
    assert np.all(np.diff(th) > 0), kind
    return th


def salpha_rows(th, shat=0.8, alpha=1.2, theta0=0.0):
    """raw rows (g, c, f) of an s-alpha line on th, f = g"""
    g, c = bo.salpha_gc(th, shat, alpha, theta0)
    return g, c, g.copy()


def salpha_line(th, shat, alpha):
    """the seven geometry arrays and dPdrho of an s-alpha line with B = 1 + 0.1 cos theta, gradpar = 1 / (1 + 0.05 cos theta): at
    theta0 the fold gives gds2 = 1 + (shat (theta - theta0) - alpha sin theta)^2 and cvdrift = alpha (cos theta + sin theta (...))"""
    lam = shat * th - alpha * np.sin(th)
    bmag = 1 + 0.1 * np.cos(th)
    gradpar = 1 / (1 + 0.05 * np.cos(th))
    gds2 = 1 + lam ** 2
    gds21 = -shat * lam
    gds22 = np.full_like(th, shat ** 2)
    cvdrift = alpha * (np.cos(th) + np.sin(th) * lam)
    cvdrift0 = -alpha * shat * np.sin(th)
    return np.stack([bmag, gradpar, cvdrift, cvdrift0, gds2, gds21, gds22]), -1.0


def interval(xp, x):
    """np.interp's interval of x in xp, clamped to [0, N - 2]"""
    return np.clip(np.searchsorted(xp, x, side="right") - 1, 0, len(xp) - 2)


def interp_bound(xp, fp, x):
    """4 eps (|fp_k| + |fp_{k+1}|): the interpolated value is one difference, one quotient, one product and one sum, each rounded once,
    and |slope dx| <= |fp_k| + |fp_{k+1}|"""
    k = interval(xp, x)
    return 4 * EPS * (np.abs(fp[k]) + np.abs(fp[k + 1]))


def regrid_numpy(th, g, c, f):
    """utils.py:1565-1576 in numpy: (h, tu, th_half, g_u, gh (N, last entry 0), c_u, f_u)"""
    N = len(th)
    tu = np.linspace(th[0], th[-1], N)
    th_half = (tu[:-1] + tu[1:]) / 2
    h = np.diff(th_half)[2]
    gh = np.zeros(N)
    gh[:-1] = np.interp(th_half, th, g)
    return h, tu, th_half, np.interp(tu, th, g), gh, np.interp(tu, th, c), np.interp(tu, th, f)
