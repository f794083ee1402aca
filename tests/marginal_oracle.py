"""CPU restatement of the marginal-stability entry points (ibs_marginal_gcf_f64 / ibs_marginal_scan_f64), from scipy alone.

Rows as in utils.py:1574-1592 on a uniform odd grid, interior points j = 1 .. N-2: e_k = (g_k + g_{k+1}) / 2 h^2, D the stiffness
matrix (D_jj = e_{j-1} + e_j, D_{j,j+-1} = -e), C = diag(c_j), T(s) = s C - D.  s* = inf { s > 0 : lam_max(T(s)) >= 0 }, by Brent
on LAPACK's lam_max(T(s)) from the unit-vector bound min D_jj / c_j over c_j > 0; the marginal mode X from the same call.  The
derivative rows are Hellmann-Feynman on the discrete pencil.  MarginalOracleContext lets the scan driver's marginal() run without
a GPU.  Test infrastructure only."""
import numpy as np
from scipy.linalg import eigh_tridiagonal
from scipy.optimize import brentq

from oracle import ballooning_oracle as bo
from tests.helpers import OracleContext

EPS = 2.220446049250313e-16


def rows(h, g, c):
    """(e (N-1,), Dd (n,), cj (n,)) of one system: the half-grid couplings, the diagonal of D and the interior c"""
    g = np.asarray(g, dtype=np.float64)
    e = 0.5 * (g[:-1] + g[1:]) / h ** 2
    return e, e[:-1] + e[1:], np.asarray(c, dtype=np.float64)[1:-1]


def top_pair(s, e, Dd, cj, vector=False):
    """lam_max of T(s) = s C - D (off-diagonals +e) and, optionally, its vector"""
    n = len(Dd)
    if vector:
        w, v = eigh_tridiagonal(s * cj - Dd, e[1:n], select="i", select_range=(n - 1, n - 1))
        return float(w[0]), v[:, 0]
    return float(eigh_tridiagonal(s * cj - Dd, e[1:n], eigvals_only=True, select="i", select_range=(n - 1, n - 1))[0])


def solve(h, g, c):
    """dict(scale, mu, X (N,), kappa, normT, u, q, e, Dd, cj) of one system; scale = inf (X None) when no c_j > 0.
    kappa = sum c_j X_j^2 / sum X_j^2 = d lam_max / d s at s*; normT = max_j (s* |c_j| + 2 D_jj); u = N eps normT / kappa: the unit in
    which errors of s* are measured (an eigenvalue error of N eps ||T|| moves s* by u)."""
    e, Dd, cj = rows(h, g, c)
    N = len(Dd) + 2
    if not (cj > 0).any():
        return dict(scale=np.inf, mu=0.0, X=None, e=e, Dd=Dd, cj=cj)
    pos = cj > 0
    upper = float((Dd[pos] / cj[pos]).min()) * (1 + 1e-12)
    s = brentq(lambda t: top_pair(t, e, Dd, cj), 0.0, upper, xtol=1e-300, rtol=4 * EPS, maxiter=500)
    _, v = top_pair(s, e, Dd, cj, vector=True)
    v = v / v[np.argmax(np.abs(v))]
    X = np.zeros(N)
    X[1:-1] = v
    q = float(np.sum(cj * v ** 2))
    kappa = q / float(np.sum(v ** 2))
    normT = float((s * np.abs(cj) + 2 * Dd).max())
    return dict(scale=s, mu=1.0 / s, X=X, kappa=kappa, normT=normT, u=N * EPS * normT / kappa, q=q, e=e, Dd=Dd, cj=cj)


def scale_of(h, g, c):
    return solve(h, g, c)["scale"]


def grad_rows(h, r):
    """(g_bar, c_bar), each (N,): d s* / d g and d s* / d c of solve()'s result r -- c_bar_j = -s* X_j^2 / q, e_bar_k =
    (X_{k+1} - X_k)^2 / q, g_bar_j = (e_bar_{j-1} + e_bar_j) / 2 h^2 with one cell at each end"""
    X, q, s = r["X"], r["q"], r["scale"]
    eb = np.diff(X) ** 2 / q
    gb = np.zeros(len(X))
    gb[:-1] += 0.5 * eb / h ** 2
    gb[1:] += 0.5 * eb / h ** 2
    return gb, -s * X ** 2 / q


def theta0_tangent(bmag, gradpar, cvdrift0, gds21, gds22, dP, t0):
    """(g_t, c_t) of utils.py:1669-1673"""
    gp = np.abs(gradpar)
    return gp * (2 * gds21 + 2 * t0 * gds22) / bmag, -1 * dP * cvdrift0 * 1 / (gp * bmag)


def line_gc(dP, bmag, gradpar, cvdrift, cvdrift0, gds2, gds21, gds22, t0):
    cv, gd = bo.fold_theta0(t0, cvdrift, cvdrift0, gds2, gds21, gds22)
    g, c, _ = bo.gcf(dP, bmag, gradpar, cv, gd)
    return g, c


def scan(h, geo7, dPdrho, theta0, want_grad=False):
    """dict(scale, mu, u[, dscale_dtheta0, dscale_ddPdrho]) shaped (n_lines, n_theta0) of geometry arrays geo7 (each (n_lines, N))"""
    nl, nt = len(dPdrho), len(theta0)
    out = dict(scale=np.zeros((nl, nt)), mu=np.zeros((nl, nt)), u=np.zeros((nl, nt)))
    if want_grad:
        out.update(dscale_dtheta0=np.zeros((nl, nt)), dscale_ddPdrho=np.zeros((nl, nt)))
    for i in range(nl):
        ln = [a[i] for a in geo7]
        for j, t0 in enumerate(theta0):
            g, c = line_gc(dPdrho[i], *ln, t0)
            r = solve(h, g, c)
            out["scale"][i, j], out["mu"][i, j], out["u"][i, j] = r["scale"], r["mu"], r.get("u", 0.0)
            if want_grad and r["X"] is not None:
                gb, cb = grad_rows(h, r)
                gt, ct = theta0_tangent(ln[0], ln[1], ln[3], ln[5], ln[6], dPdrho[i], t0)
                out["dscale_dtheta0"][i, j] = float(np.sum(gb * gt + cb * ct))
                out["dscale_ddPdrho"][i, j] = -r["scale"] / dPdrho[i]
    return out


class MarginalOracleContext(OracleContext):
    """OracleContext + marginal_gcf / marginal_scan (host arrays)"""

    def marginal_gcf(self, h, g, c, want_X=False, want_grad=False, want_info=False):
        n, N = g.shape
        out = dict(scale=np.zeros(n), mu=np.zeros(n), nbad=0)
        if want_X:
            out.update(X=np.full((n, N), np.nan))
        if want_grad:
            out.update(g_bar=np.zeros((n, N)), c_bar=np.zeros((n, N)))
        if want_info:
            out.update(info=np.zeros(n, dtype=np.int32))
        for k in range(n):
            r = solve(h, g[k], c[k])
            out["scale"][k], out["mu"][k] = r["scale"], r["mu"]
            if r["X"] is None:
                if want_info:
                    out["info"][k] = 256 << 16
                continue
            if want_X:
                out["X"][k] = r["X"]
            if want_grad:
                out["g_bar"][k], out["c_bar"][k] = grad_rows(h, r)
        return out

    def marginal_scan(self, h, bmag, gradpar, cvdrift, cvdrift0, gds2, gds21, gds22, dPdrho, theta0, want_grad=False, want_info=False):
        r = scan(h, [bmag, gradpar, cvdrift, cvdrift0, gds2, gds21, gds22], dPdrho, theta0, want_grad)
        out = dict(scale=r["scale"], mu=r["mu"], nbad=0)
        if want_grad:
            out.update(dscale_dtheta0=r["dscale_dtheta0"], dscale_ddPdrho=r["dscale_ddPdrho"])
        if want_info:
            out.update(info=np.where(np.isinf(r["scale"]), 256 << 16, 0).astype(np.int32))
        return out
