"""Test-only: inputs and the oracle side of the local-equilibrium gradient tests (tests/test_local_eq_grad_cpu.py,
tests/test_gpu_local_eq_grad.py).  Rows are ibs_amd.local_eq_fold's, eigenpairs the C oracle's, derivatives
ibs_amd.local_eq_lam_grad's on the oracle's eigenpair; differences are central differences of the oracle's lam_max."""
import numpy as np

from ibs_amd import local_eq_lam_grad
from oracle import ballooning_oracle as bo
from tests import local_eq_cases as lc

EPS = lc.EPS
T0S = (0.0, 0.1, -0.3)
# a dozen points (theta0, eps, p): both signs of theta0 and eps, p below and above 1, stable and unstable.  No point is mirror-symmetric
# on its line (theta0 = 0 at eps = 0 on the line centred at 0): there d lam / d theta0 and every one of its terms vanish, and so does the scale
POINTS = np.array([(0.17, 0.0, 1.6), (0.2, 0.5, 1.6), (0.0, -0.5, 1.2), (0.1, 0.9, 2.2), (0.0, -0.9, 3.0), (-0.3, 0.3, 0.8),
                   (0.4, -0.2, 2.0), (0.05, 0.0, 1.0), (0.0, 0.6, 0.4), (-0.1, -0.7, 2.6), (0.25, 0.2, 1.3), (0.3, 0.1, 0.5)])


# the dozen for N > 1024.  The condition on the inputs asks for a gap of 1e-6 ||A|| below lam_max, and ||A|| grows as N^2 (2.7e4 at N = 2051, 1.1e5
# at N = 4097) while the spectrum does not: the stable points above have a next eigenvalue within 0.03.  These twelve are unstable with a gap
# above 0.16 on each of the three lines, with and without the ps rows (searched on the CPU at N = 129; asserted at the N used)
LONG_POINTS = np.array([(0.17, 0.0, 2.2), (0.17, -0.5, 1.6), (0.17, 0.5, 3.0), (0.17, 0.9, 4.0), (-0.3, 0.0, 3.0), (-0.3, -0.5, 2.2),
                        (-0.3, 0.5, 4.0), (-0.3, -0.2, 1.6), (0.05, 0.0, 4.0), (0.05, -0.2, 2.2), (0.4, -0.5, 1.6), (0.4, -0.2, 3.0)])


def salpha_batch(N, with_ps=True):
    """the three s-alpha lines (theta0 = 0, 0.1, -0.3) at N points, with or without their ps rows, and the dozen POINTS (LONG_POINTS
    for N > 1024) dealt to the lines in turn: dict(th, lines (3, 8, N), dP, centre, sigma, ps (3, N) or None, line_of int32 (12,),
    var (12, 3))"""
    th = bo.theta_grid(N)
    base = [lc.salpha_base_line(th, t0) for t0 in T0S]
    return dict(th=th, lines=np.stack([b[0] for b in base]), dP=np.array([b[1] for b in base]), centre=np.array(T0S), sigma=np.ones(3),
                ps=np.stack([b[2] for b in base]) if with_ps else None, line_of=(np.arange(len(POINTS)) % 3).astype(np.int32),
                var=(LONG_POINTS if N > 1024 else POINTS).copy())


# the same for the NCSX lines, with three of the stable points moved to a higher pressure: on these lines a stable lam_max sits within 1e-5 ||A|| of
# the next eigenvalue (the count at lam - 1e-6 ||A|| is 2 at POINTS[8]), which the condition on the inputs excludes
NCSX_POINTS = POINTS.copy()
NCSX_POINTS[[2, 5, 8]] = [(0.0, -0.5, 2.2), (-0.3, 0.3, 1.8), (0.0, 0.6, 1.4)]
# the first four lines of the fixture have alpha = 0, 1, 2, pi: lines 0 and 3 are stellarator-symmetric, so the theta0 = 0 points go to lines 1 and 2
NCSX_LINE_OF = np.array([0, 1, 2, 3, 1, 1, 2, 3, 2, 1, 2, 3], dtype=np.int32)


def ncsx_batch(g3, N=513, n_lines=4):
    """n_lines committed NCSX lines at N (G3_ncsx_lines.npz) with a smooth ps row each, both signs of sigma, and the dozen NCSX_POINTS"""
    th = bo.theta_grid(N)
    k = np.arange(n_lines)[:, None]
    return dict(th=th, lines=np.array(g3["geo_%d" % N][:n_lines]), dP=g3["dPdrho_%d" % N][:n_lines].copy(),
                centre=g3["lines_%d" % N][:n_lines, 1].copy(), sigma=np.where(np.arange(n_lines) % 2, -1.0, 1.0),
                ps=0.3 * np.sin(th[None] + 0.4 * k) / (1.0 + 0.1 * k), line_of=NCSX_LINE_OF % n_lines, var=NCSX_POINTS.copy())


def point_rows(b, line_of=None, var=None):
    """(g, c, f), each (n_pts, N), of the points of a batch by the rule"""
    line_of = b["line_of"] if line_of is None else line_of
    var = b["var"] if var is None else var
    out = []
    for l, v in zip(line_of, var):
        g, c, f = lc.rows_of(b["th"], b["lines"][l:l + 1], b["dP"][l:l + 1], b["centre"][l:l + 1], b["sigma"][l:l + 1], v[None],
                             ps=None if b["ps"] is None else b["ps"][l:l + 1])
        out.append((g[0, 0], c[0, 0], f[0, 0]))
    return tuple(np.stack([o[k] for o in out]) for k in range(3))


def assert_simple(b, ref, g, c, f):
    """the condition on the inputs: exactly one eigenvalue above lam_max - 1e-6 ||A|| (lam_max is simple, with that gap)"""
    cnt = lc.counts_of(b["th"], g, c, f, ref["lam"] - 1e-6 * ref["normA"])
    assert (cnt == 1).all(), cnt


def oracle_pairs(b, line_of=None, var=None):
    """dict(lam, gam, X (n_pts, N), tol_lam, normA, margin) of the points of a batch by the C oracle; asserts lam_max simple"""
    from oracle import c_oracle as co
    g, c, f = point_rows(b, line_of, var)
    ref = lc.oracle_of(b["th"], g, c, f)
    assert_simple(b, ref, g, c, f)
    h = float(b["th"][1] - b["th"][0])
    X = np.stack([co.solve_gcf(h, g[k], c[k], f[k])[2] for k in range(len(g))])
    return dict(ref, X=X)


def numpy_grads(b, ref, line_of=None, var=None):
    """local_eq_lam_grad on the oracle's eigenpair of every point: dict(dlam (n, 4), geo_bar (n, 8, N), dlam_scale, geo_bar_scale)"""
    line_of = b["line_of"] if line_of is None else line_of
    var = b["var"] if var is None else var
    r = [local_eq_lam_grad(b["th"], b["lines"][l], b["dP"][l], b["centre"][l], b["sigma"][l], v, ref["X"][k], ref["lam"][k],
                           ps=None if b["ps"] is None else b["ps"][l]) for k, (l, v) in enumerate(zip(line_of, var))]
    return {key: np.stack([q[key] for q in r]) for key in ("dlam", "geo_bar", "dlam_scale", "geo_bar_scale")}


def oracle_lam(b, line_of, var, lines=None, dP=None):
    """the oracle's lam_max alone at points (line_of (n,), var (n, 3)) of a batch, optionally with other lines / dPdrho per POINT:
    lines (n, 8, N), dP (n,)"""
    from oracle import c_oracle as co
    n = len(var)
    bb = b if lines is None and dP is None else dict(
        b, lines=b["lines"][line_of] if lines is None else lines, dP=b["dP"][line_of] if dP is None else dP, centre=b["centre"][line_of],
        sigma=b["sigma"][line_of], ps=None if b["ps"] is None else b["ps"][line_of])
    lo = line_of if bb is b else np.arange(n)
    g, c, f = point_rows(bb, lo, var)
    return co.lam_batch(float(b["th"][1] - b["th"][0]), g, c, f)


def richardson(lam_of, delta):
    """central differences D(delta), D(delta / 2) of lam_of(step) (vectorised over a leading axis) and their Richardson extrapolate
    R = (4 D(delta / 2) - D(delta)) / 3 -> (R, D(delta), D(delta / 2))"""
    d1 = (lam_of(delta) - lam_of(-delta)) / (2 * delta)
    d2 = (lam_of(0.5 * delta) - lam_of(-0.5 * delta)) / delta
    return (4 * d2 - d1) / 3, d1, d2
