"""CPU restatement of ibs_solve_gcf_vjp_f64 (the exact vector-Jacobian product of gam and lam in the (g, c, f) rows), built from the
oracle's public pieces: the pencil rows of bo.assemble, the eigenpair of bo.top_eigenpair (or of the nearest-sigma restatement) and
the FD4 / Simpson quotient of bo.rayleigh_growth (utils.py:1601-1621).  The singular adjoint system (S - lam F) z = dgam/dX is solved
here by the BORDERED system [[S - lam F, F X], [X^T F, 0]] with scipy.sparse.linalg.spsolve -- not the kernel's twisted split -- so
that the two share nothing but the formulas of include/ibs.h."""
import numpy as np
import scipy.sparse as sp
from scipy.sparse.linalg import spsolve

from oracle import ballooning_oracle as bo


def simpson_weights(N):
    """composite Simpson weights (1, 4, 2, ..., 4, 1) / 3: bo.simpson_unit(y) == simpson_weights(len(y)) @ y"""
    w = np.full(N, 2.0)
    w[1:-1:2] = 4.0
    w[0] = w[-1] = 1.0
    return w / 3.0


def fd4_matrix(N, h):
    """D with dX = D X: the stencils of bo.rayleigh_growth (second order at the ends, fourth order inside; utils.py:1610-1616)"""
    rows, cols, vals = [], [], []

    def put(i, j, v):
        rows.append(i); cols.append(j); vals.append(v)
    put(0, 0, -1.5 / h); put(0, 1, 2.0 / h); put(0, 2, -0.5 / h)
    put(1, 2, 0.5 / h); put(1, 0, -0.5 / h)
    put(N - 2, N - 1, 0.5 / h); put(N - 2, N - 3, -0.5 / h)
    put(N - 1, N - 3, 0.5 / h); put(N - 1, N - 2, -2.0 / h); put(N - 1, N - 1, 1.5 / h)
    j = np.arange(2, N - 2)
    for off, v in ((1, 2 / (3 * h)), (-1, -2 / (3 * h)), (2, -1 / (12 * h)), (-2, 1 / (12 * h))):
        rows += list(j); cols += list(j + off); vals += [v] * len(j)
    return sp.csr_matrix((vals, (rows, cols)), shape=(N, N))


def eigenpair(th, g, c, f, sigma=None):
    """(gam, lam, X) of lam_max (bo.solve_gcf) or, with sigma, of the eigenvalue nearest sigma (tests/nearest_oracle.py)"""
    if sigma is None:
        gam, lam, X, _ = bo.solve_gcf(th, g, c, f)
        return gam, lam, X
    from tests.nearest_oracle import dense_nearest
    r = dense_nearest(th, g, c, f, sigma)
    return r["gam"], r["lam"], r["X"]


def gcf_vjp(th, g, c, f, lam, X, gam_bar=1.0, lam_bar=0.0):
    """(g_bar, c_bar, f_bar), each (N,): gam_bar * d gam + lam_bar * d lam of the simple eigenpair (lam, X) of the pencil of
    utils.py:1574-1592 on the rows (g, c, f), d taken with respect to the rows (the half-grid g is the mean of neighbours)."""
    d, e, fd, h, gu, cu, fu = bo.assemble(th, g, c, f)
    N, n = len(g), len(d)
    X = np.array(X, dtype=np.float64)
    X[0] = X[-1] = 0.0
    D = fd4_matrix(N, h)
    w = simpson_weights(N)
    dX = D @ X
    Q1 = w @ (fu * X ** 2)
    gam = (w @ (cu * X ** 2 - gu * dX ** 2)) / Q1
    Q = fd @ (X[1:-1] ** 2)
    # 1. explicit terms
    gb = -w * dX ** 2 / Q1
    cb = w * X ** 2 / Q1
    fb = -gam * w * X ** 2 / Q1
    # 2. gradient in X
    r = (2.0 / Q1) * (D.T @ (-w * gu * dX) + w * cu * X - gam * w * fu * X)
    # 3. adjoint solve, bordered: [[S - lam F, F X], [X^T F, 0]] [z; mu] = [r; 0]
    FX = fd * X[1:-1]
    A = sp.diags([d - lam * fd, e[1:n], e[1:n]], [0, -1, 1])
    K = sp.bmat([[A, sp.csr_matrix(FX[:, None])], [sp.csr_matrix(FX[None, :]), None]]).tocsc()
    sol = spsolve(K, np.r_[r[1:-1], 0.0])
    z = np.zeros(N)
    z[1:-1] = sol[:n]
    # 4. implicit terms; 5. scale; 6. lam (Hellmann-Feynman); 7. half-grid chain
    dXe = np.diff(X)
    ghb = gam_bar * np.diff(z) * dXe / h ** 2 - lam_bar * dXe ** 2 / (h ** 2 * Q)
    cb = gam_bar * (cb - z * X) + lam_bar * X ** 2 / Q
    fb = gam_bar * (fb + lam * z * X) - lam_bar * lam * X ** 2 / Q
    gb = gam_bar * gb
    gb[:-1] += 0.5 * ghb
    gb[1:] += 0.5 * ghb
    return gb, cb, fb


def smooth_direction(rng, th, scale):
    """a smooth random row: a few low Fourier modes on the grid, times scale (broadcast)"""
    t = (th - th[0]) / (th[-1] - th[0])
    v = np.zeros_like(th)
    for m in range(1, 5):
        v += rng.standard_normal() * np.cos(np.pi * m * t + rng.uniform(0, np.pi)) / m
    return v * scale


EPS = 2.220446049250313e-16


def residual_ratio(h, g, c, f, lam, X):
    """max_r |((S - lam F) X)_r| / f_r of each system (rows (n_sys, N), the half-grid g the mean of neighbours as the library forms
    it) in units of N eps (||A|| + |lam|) max |X|: the quantity ibs_solve_gcf_vjp_f64 refuses above 1024 (csrc/ibs_vjp.hip)"""
    g, c, f, X = (np.asarray(a, dtype=np.float64) for a in (g, c, f, X))
    lam = np.asarray(lam, dtype=np.float64)
    N = g.shape[1]
    e = 0.5 * (g[:, :-1] + g[:, 1:]) / h ** 2
    d = c[:, 1:-1] - (e[:, :-1] + e[:, 1:])
    Xi = X[:, 1:-1]
    Xm = np.concatenate([np.zeros((len(X), 1)), Xi[:, :-1]], axis=1)
    Xp = np.concatenate([Xi[:, 1:], np.zeros((len(X), 1))], axis=1)
    r = e[:, :-1] * Xm + (d - lam[:, None] * f[:, 1:-1]) * Xi + e[:, 1:] * Xp
    res = (np.abs(r) / f[:, 1:-1]).max(1)
    na = ((np.abs(d) + e[:, :-1] + e[:, 1:]) / f[:, 1:-1]).max(1)
    return res / (N * EPS * (na + np.abs(lam)) * np.abs(Xi).max(1))


def pivot_breaking_rows(N, lam=0.5):
    """(g, c, f, X) of three systems on h = 1 whose every value is a small dyadic, so that the kernel's arithmetic is exact: X is an
    eigenvector of the rows for eigenvalue lam (residual exactly 0), its largest entry in the middle.  System 0 has X_2 = 0, which
    makes the first forward pivot d_0 - lam f_0 = -e_1 X_2 / X_1 exactly 0 (leading block); system 1 mirrors it at the other end
    (X_{N-3} = 0: the last backward pivot, trailing block); system 2 has no zero entry."""
    base = np.array([1.0 if (j // 3) % 2 == 0 else -1.0 for j in range(N)])
    out = []
    for kind in range(3):
        X = base.copy()
        X[0] = X[-1] = 0.0
        X[N // 2] = 8.0
        if kind == 0:
            X[1], X[2], X[3] = 1.0, 0.0, -1.0
        elif kind == 1:
            X[N - 2], X[N - 3], X[N - 4] = 1.0, 0.0, -1.0
        g = np.full(N, 2.0)                                  # e = (g_k + g_{k+1}) / 2 / h^2 = 2
        f = np.ones(N)
        c = np.zeros(N)
        for j in range(1, N - 1):                            # 2 X_{j-1} + (c_j - 4 - lam) X_j + 2 X_{j+1} = 0
            if X[j] != 0.0:
                c[j] = 4.0 + lam - 2.0 * (X[j - 1] + X[j + 1]) / X[j]
            else:
                assert X[j - 1] + X[j + 1] == 0.0
        out.append((g, c, f, X))
    return [np.stack([o[i] for o in out]) for i in range(4)]


def synthetic_batch(n, N, s=0.7):
    """(h, [g, c, f]) of n (line, theta0) systems of tests.helpers.synthetic_fieldlines: lines alpha in [0, pi], 15 theta0 in
    [0, pi / 2] each (ball_scan.py:223-226)"""
    from tests.helpers import synthetic_fieldlines
    th = bo.theta_grid(N)
    rows = []
    for ln in synthetic_fieldlines(th)(s, np.linspace(0, np.pi, max(1, -(-n // 15)))):
        dP = bo.dPdrho_of(ln[2], ln[7], ln[0])
        for t0 in np.linspace(0, np.pi / 2, 15):
            cv, gd = bo.fold_theta0(t0, *ln[2:7])
            rows.append(bo.gcf(dP, ln[0], ln[1], cv, gd))
    rows = rows[:n]
    return float(th[1] - th[0]), [np.stack([r[i] for r in rows]) for i in range(3)]
