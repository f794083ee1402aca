"""CPU stand-in for the nearest-sigma entry points of ibs_amd.Context, built from the oracle's public pieces: the pencil rows of
bo.assemble, its full spectrum in the symmetric form bo.top_eigenpair uses (scipy eigh_tridiagonal), the eigenvalue nearest sigma
(distances within 4 N eps ||A|| of each other: the larger one), its vector, the sign that makes the largest |x| positive,
bo.rayleigh_growth and bo.hf_derivative.  Lets the scan driver's eigenpair="nearest" plumbing run without a GPU."""
import numpy as np

from oracle import ballooning_oracle as bo
from tests.helpers import OracleContext

EPS = 2.220446049250313e-16


def dense_nearest(th, g, c, f, sigma):
    """dict(lam, idx, gam, X, dX, tie, lam_max, gap, nA) of the eigenpair of utils.py:1574-1592's pencil nearest sigma"""
    from scipy.linalg import eigh_tridiagonal
    d, e, fd, h, gu, cu, fu = bo.assemble(th, g, c, f)
    n, N = len(d), len(g)
    a = d / fd
    b = e[1:n] / np.sqrt(fd[:-1] * fd[1:])
    w = eigh_tridiagonal(a, b, eigvals_only=True)
    nA = float(((np.abs(d) + e[:-1] + e[1:]) / fd).max())
    tau = 4 * N * EPS * nA
    dist = np.abs(w - min(max(sigma, w[0] - 1.0), w[-1] + 1.0))
    order = np.argsort(dist, kind="stable")
    j, tie = int(order[0]), False
    if n > 1 and dist[order[1]] - dist[j] < tau:
        j, tie = max(j, int(order[1])), True
    _, v = eigh_tridiagonal(a, b, select="i", select_range=(j, j))
    x = v[:, 0] / np.sqrt(fd)
    if x[np.argmax(np.abs(x))] < 0:
        x = -x
    gam, X, dX = bo.rayleigh_growth(x, h, gu, cu, fu)
    gap = min(w[j] - w[j - 1] if j > 0 else np.inf, w[j + 1] - w[j] if j < n - 1 else np.inf)
    return dict(lam=float(w[j]), idx=n - 1 - j, gam=gam, X=X, dX=dX, tie=tie, lam_max=float(w[-1]), gap=gap, nA=nA)


def window_nearest(th, g, c, f, sigma, radius=1.0):
    """dense_nearest without the full spectrum (minutes per system at N = 65,535): the eigenvalues above sigma - radius alone, by
    LAPACK's bisection.  Valid when the nearest of them lies within radius - 4 N eps ||A|| of sigma (asserted): every eigenvalue
    outside the window is then farther from sigma.  Same keys as dense_nearest except gap."""
    from scipy.linalg import eigh_tridiagonal
    d, e, fd, h, gu, cu, fu = bo.assemble(th, g, c, f)
    n, N = len(d), len(g)
    a = d / fd
    b = e[1:n] / np.sqrt(fd[:-1] * fd[1:])
    nA = float(((np.abs(d) + e[:-1] + e[1:]) / fd).max())
    tau = 4 * N * EPS * nA
    w = eigh_tridiagonal(a, b, eigvals_only=True, select="v", select_range=(sigma - radius, nA + 1.0))       # ascending, up to lam_max
    dist = np.abs(w - sigma)
    order = np.argsort(dist, kind="stable")
    j, tie = int(order[0]), False
    assert dist[j] < radius - tau, (sigma, radius, w)
    if len(w) > 1 and dist[order[1]] - dist[j] < tau:
        j, tie = max(j, int(order[1])), True
    idx = len(w) - 1 - j
    _, v = eigh_tridiagonal(a, b, select="i", select_range=(n - 1 - idx, n - 1 - idx))
    x = v[:, 0] / np.sqrt(fd)
    if x[np.argmax(np.abs(x))] < 0:
        x = -x
    gam, X, dX = bo.rayleigh_growth(x, h, gu, cu, fu)
    return dict(lam=float(w[j]), idx=idx, gam=gam, X=X, dX=dX, tie=tie, lam_max=float(w[-1]), nA=nA)


def grid_of(h, N):
    return np.linspace(-h * (N - 1) / 2, h * (N - 1) / 2, N)


def gcf_at(dP, bmag, gradpar, cvdrift, cvdrift0, gds2, gds21, gds22, t0):
    cv, gd = bo.fold_theta0(t0, cvdrift, cvdrift0, gds2, gds21, gds22)
    return bo.gcf(dP, bmag, gradpar, cv, gd)


def obj_w_grad_nearest_lines(th, theta0, lines, sigma, del_alpha=0.004):
    """utils.py:1632-1728 on the three lines (alpha - d/2, alpha, alpha + d/2), each (8, N), with the eigenpair nearest sigma"""
    dP = [bo.dPdrho_of(ln[2], ln[7], ln[0]) for ln in lines]
    g, c, f = gcf_at(dP[1], *lines[1][:7], theta0)
    r = dense_nearest(th, g, c, f, sigma)
    gam, X, dX = r["gam"], r["X"], r["dX"]
    bmag, gradpar, _, cvdrift0, _, gds21, gds22, _ = lines[1]
    gp = np.abs(gradpar)
    dgd = 2 * gds21 + 2 * theta0 * gds22
    jt = bo.hf_derivative(gam, X, dX, f, gp * dgd / bmag, -1 * dP[1] * cvdrift0 * 1 / (gp * bmag), dgd / bmag ** 2 * 1 / (gp * bmag))
    g_r, c_r, f_r = gcf_at(dP[2], *lines[2][:7], theta0)
    g_l, c_l, f_l = gcf_at(dP[0], *lines[0][:7], theta0)
    ja = bo.hf_derivative(gam, X, dX, f, (g_r - g_l) / del_alpha, (c_r - c_l) / del_alpha, (f_r - f_l) / del_alpha)
    return -gam, np.array([-ja, -jt]), r


class NearestOracleContext(OracleContext):
    """OracleContext + gamma_scan_nearest / obj_w_grad_nearest / gamma_points_nearest (host arrays, the dense nearest eigenpair)"""

    def gamma_scan_nearest(self, h, bmag, gradpar, cvdrift, cvdrift0, gds2, gds21, gds22, dPdrho, theta0, sigma, want_info=False):
        nl, N = bmag.shape
        th = grid_of(h, N)
        sig = np.broadcast_to(np.asarray(sigma, dtype=np.float64), (nl, len(theta0)))
        gam, lam, idx = np.zeros((nl, len(theta0))), np.zeros((nl, len(theta0))), np.zeros((nl, len(theta0)), dtype=np.int32)
        self.lam_max = np.zeros((nl, len(theta0)))
        for i in range(nl):
            for j, t0 in enumerate(theta0):
                g, c, f = gcf_at(dPdrho[i], bmag[i], gradpar[i], cvdrift[i], cvdrift0[i], gds2[i], gds21[i], gds22[i], t0)
                r = dense_nearest(th, g, c, f, sig[i, j])
                gam[i, j], lam[i, j], idx[i, j], self.lam_max[i, j] = r["gam"], r["lam"], r["idx"], r["lam_max"]
        return dict(gam=gam, lam=lam, idx=idx, nbad=0)

    def obj_w_grad_nearest(self, h, geo, theta0, sigma, del_alpha=0.004, want_info=False):
        n, _, _, N = geo.shape
        th = grid_of(h, N)
        sig = np.broadcast_to(np.asarray(sigma, dtype=np.float64), (n,))
        val, jac = np.zeros(n), np.zeros((n, 2))
        for k in range(n):
            val[k], jac[k], _ = obj_w_grad_nearest_lines(th, theta0[k], geo[k], sig[k], del_alpha)
        return val, jac

    def gamma_points_nearest(self, h, bmag, gradpar, cvdrift, cvdrift0, gds2, gds21, gds22, dPdrho, theta0, sigma,
                             want_X=False, want_info=False):
        n, N = bmag.shape
        th = grid_of(h, N)
        sig = np.broadcast_to(np.asarray(sigma, dtype=np.float64), (n,))
        gam, lam, idx = np.zeros(n), np.zeros(n), np.zeros(n, dtype=np.int32)
        for k in range(n):
            g, c, f = gcf_at(dPdrho[k], bmag[k], gradpar[k], cvdrift[k], cvdrift0[k], gds2[k], gds21[k], gds22[k], theta0[k])
            r = dense_nearest(th, g, c, f, sig[k])
            gam[k], lam[k], idx[k] = r["gam"], r["lam"], r["idx"]
        return dict(gam=gam, lam=lam, idx=idx, nbad=0)
