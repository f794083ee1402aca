"""Test-only restatement, in numpy and the C oracle, of what csrc/ibs_certify.hip computes: the theta0 fold and the (g, c, f) rows of a
geometry-fed system, ||A||, the certificate's tolerance and its rule -- and the mapping of any positive (g, c, f) system onto geometry
arrays, which carries the raw-system fixtures (G10, the rough family of BASELINE configs[4]) to the geometry-fed entry points."""
import numpy as np

from oracle import ballooning_oracle as bo
from oracle import c_oracle as co

EPS64 = 2.220446049250313e-16
NOT_MAX, NO_EIG, UNCHECKED, RECLOSED = 1, 2, 4, 8


def gcf_to_geometry(g, c, f, dPdrho=-1.0, th0_planes=0.0, seed=0):
    """(g, c, f) [n][N], all g, f > 0 -> the seven geometry arrays whose rows at theta0 = 0 are (g, c, f) again (utils.py:1560-1562):
    B = 1, gradpar = sqrt(g / f), gds2 = g / gradpar, cvdrift = -c gradpar / dPdrho.  th0_planes > 0 fills cvdrift0, gds21, gds22
    with small positive values of that size (they only matter at theta0 != 0; gds22 > 0 and gds21 >= 0 keep g, f > 0 there)."""
    g, c, f = (np.atleast_2d(np.asarray(a, dtype=np.float64)) for a in (g, c, f))
    gp = np.sqrt(g / f)
    gds2 = g / gp
    cv = -c * gp / dPdrho
    z = np.zeros_like(g)
    if th0_planes > 0:
        u = np.random.default_rng(seed).uniform(0.5, 1.0, size=(3,) + g.shape)
        cv0, gds21, gds22 = th0_planes * u[0], th0_planes * u[1] * gds2, th0_planes * u[2] * gds2
    else:
        cv0, gds21, gds22 = z, z.copy(), z.copy()
    return [np.ones_like(g), gp, cv, cv0, gds2, gds21, gds22], np.full(g.shape[0], float(dPdrho))


def salpha_geometry(theta, shat, alpha):
    """s-alpha lines (bishop_ball_s-alpha.py:30-45) written as geometry arrays with their theta0 planes, f = g: B = gradpar = 1,
    gds2 = 1 + L^2, gds21 = -shat L, gds22 = shat^2 (L = shat theta - alpha sin theta: gd = 1 + (L - shat theta0)^2), dPdrho = -1,
    cvdrift = alpha (cos + sin L), cvdrift0 = -alpha shat sin.  shat, alpha: (n,).  Returns (geo7 [n][N], dPdrho (n,))."""
    sh, al = np.asarray(shat, dtype=np.float64)[:, None], np.asarray(alpha, dtype=np.float64)[:, None]
    th = np.asarray(theta)[None]
    L = sh * th - al * np.sin(th)
    one = np.ones_like(L)
    return [one, one.copy(), al * (np.cos(th) + np.sin(th) * L), -al * sh * np.sin(th) * one, 1 + L ** 2, -sh * L, sh ** 2 * one], \
        -np.ones(L.shape[0])


def fold_rows(geo7, dPdrho, theta0, per_line=False):
    """host-folded rows of every (line, theta0): ball_scan.py:267-268 + utils.py:1560-1562 in the order the kernels evaluate them.
    Returns g, c, f [n_lines * n_theta0][N] (per_line: theta0 (n_lines,), one system per line)."""
    B, gpar, cv, cv0, g0, g1, g2 = (np.asarray(a, dtype=np.float64) for a in geo7)
    gp = np.abs(gpar)
    inv = 1.0 / (gp * B)
    A1, A3 = gp / B, inv / (B * B)
    mdP = -np.asarray(dPdrho, dtype=np.float64)[:, None]
    C0, C1 = mdP * cv * inv, mdP * cv0 * inv
    t0 = np.asarray(theta0, dtype=np.float64)
    t = t0[:, None, None] if per_line else t0[None, :, None]
    ex = (lambda a: a[:, None, :])
    d = ex(g0) + (2.0 * t) * ex(g1) + (t * t) * ex(g2)
    g, c, f = ex(A1) * d, ex(C0) + t * ex(C1), ex(A3) * d
    N = B.shape[1]
    return g.reshape(-1, N), c.reshape(-1, N), f.reshape(-1, N)


def norm_a(h, g, c, f):
    """||A|| = max_r (|d_r| + e_r + e_{r+1}) / f_r of the rows of utils.py:1584-1592, per system"""
    e = 0.5 * (g[:, :-1] + g[:, 1:]) / h ** 2
    d = c[:, 1:-1] - (e[:, :-1] + e[:, 1:])
    return ((np.abs(d) + e[:, :-1] + e[:, 1:]) / f[:, 1:-1]).max(axis=1)


def tolerance(h, g, c, f, tol_factor=4.0):
    return tol_factor * g.shape[1] * EPS64 * norm_a(h, g, c, f)


def cert_rule(h, g, c, f, lam, tol_factor=4.0):
    """the cert word of every system from the C oracle's division-form counts at lam +- tol"""
    lam = np.asarray(lam, dtype=np.float64)
    bad = ~np.isfinite(lam) | ~np.isfinite(g).all(axis=1) | ~np.isfinite(c).all(axis=1) | ~np.isfinite(f).all(axis=1) | \
        (g <= 0).any(axis=1) | (f <= 0).any(axis=1)
    tol = tolerance(h, g, c, f, tol_factor)
    l0 = np.where(bad, 0.0, lam)
    above = co.count_above_batch(h, g, c, f, l0 + tol)
    below = co.count_above_batch(h, g, c, f, l0 - tol)
    word = np.where(above != 0, NOT_MAX, 0) | np.where(below == 0, NO_EIG, 0)
    return np.where(bad, UNCHECKED, word).astype(np.int32)


def second_eigenvalue(h, g, c, f, lam_max, tol):
    """lam_2 of one system by bisection on the C oracle's count, between the lower Gershgorin end and lam_max - tol (count >= 1 there)"""
    g, c, f = (np.asarray(a, dtype=np.float64)[None] for a in (g, c, f))
    hi = float(lam_max - tol)
    lo = float(-norm_a(h, g, c, f)[0]) - 1.0
    cnt = lambda s: int(co.count_above_batch(h, g, c, f, np.array([s]))[0])
    if cnt(hi) >= 2:
        return hi          # (lam_2 within tol of lam_max)
    for _ in range(200):   # count(lo) >= 2, count(hi) == 1
        mid = 0.5 * (lo + hi)
        if mid <= lo or mid >= hi:
            break
        if cnt(mid) >= 2:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


def dense_top_two(h, g, c, f):
    """the two largest eigenvalues of one system from the dense symmetric form F^-1/2 T F^-1/2 (numpy eigvalsh)"""
    N = len(g)
    th = np.linspace(-h * (N - 1) / 2, h * (N - 1) / 2, N)
    d, e, fd, _, _, _, _ = bo.assemble(th, g, c, f)
    n = N - 2
    a = d / fd
    b = e[1:n] / np.sqrt(fd[:-1] * fd[1:])
    w = np.linalg.eigvalsh(np.diag(a) + np.diag(b, 1) + np.diag(b, -1))
    return w[-1], w[-2]
