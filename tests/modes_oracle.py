"""CPU reference of the spectrum mode (Context.solve_gcf_modes / gamma_scan_modes), built from the oracle's public pieces exactly as
tests/nearest_oracle.py is: the pencil rows of bo.assemble, the symmetric form bo.top_eigenpair uses and scipy's eigh_tridiagonal
(the full spectrum, then the vectors by select="i"), the sign that makes the largest |x| positive, bo.rayleigh_growth.  Lets the
scan driver's modes() plumbing run without a GPU (ModesOracleContext)."""
import numpy as np

from oracle import ballooning_oracle as bo
from tests.helpers import OracleContext
from tests.nearest_oracle import gcf_at, grid_of

EPS = 2.220446049250313e-16
CLUSTER_BIT = 1 << 9


def spectrum(th, g, c, f):
    """(ascending eigenvalues, (a, b) of the symmetric form, fd, h, gu, cu, fu, ||A||) of the pencil of utils.py:1574-1592"""
    from scipy.linalg import eigh_tridiagonal
    d, e, fd, h, gu, cu, fu = bo.assemble(th, g, c, f)
    n = len(d)
    a = d / fd
    b = e[1:n] / np.sqrt(fd[:-1] * fd[1:])
    w = eigh_tridiagonal(a, b, eigvals_only=True)
    nA = float(((np.abs(d) + e[:-1] + e[1:]) / fd).max())
    return w, (a, b), fd, h, gu, cu, fu, nA


def dense_modes(th, g, c, f, K, vectors=True):
    """dict(lam (K,), gam (K,), X, dX (K, N), gap (K,) = the distance to the nearer neighbouring eigenvalue -- the first unwanted one
    included --, nA, tau = 4 N eps ||A||, w = the whole spectrum descending) of the K largest eigenpairs"""
    from scipy.linalg import eigh_tridiagonal
    w, (a, b), fd, h, gu, cu, fu, nA = spectrum(th, g, c, f)
    n, N = len(w), len(g)
    wd = w[::-1]
    lam = wd[:K].copy()
    gap = np.array([min(wd[m - 1] - wd[m] if m > 0 else np.inf, wd[m] - wd[m + 1] if m + 1 < n else np.inf) for m in range(K)])
    out = dict(lam=lam, gap=gap, nA=nA, tau=4 * N * EPS * nA, w=wd)
    if vectors:
        gam, X, dX = np.zeros(K), np.zeros((K, N)), np.zeros((K, N))
        for m in range(K):
            _, v = eigh_tridiagonal(a, b, select="i", select_range=(n - 1 - m, n - 1 - m))
            x = v[:, 0] / np.sqrt(fd)
            if x[np.argmax(np.abs(x))] < 0:
                x = -x
            gam[m], X[m], dX[m] = bo.rayleigh_growth(x, h, gu, cu, fu)
        out.update(gam=gam, X=X, dX=dX)
    return out


def cluster_rule(ref):
    """(required, forbidden) boolean (K,): the bit must be set where the reference gap is below tau / 2, must not where it is above
    2 tau, and is free in between"""
    return ref["gap"] < 0.5 * ref["tau"], ref["gap"] > 2.0 * ref["tau"]


def residual_ok(th, g, c, f, lam, X):
    """the bound ibs_solve_gcf_vjp_f64 holds a pair to: max_r |((S - lam F) X)_r| / f_r <= 1024 N eps (||A|| + |lam|) max |X|"""
    d, e, fd, h, gu, cu, fu = bo.assemble(th, g, c, f)
    n, N = len(d), len(g)
    x = np.asarray(X)[1:-1]
    r = (d - lam * fd) * x
    r[1:] += e[1:n] * x[:-1]
    r[:-1] += e[1:n] * x[1:]
    nA = float(((np.abs(d) + e[:-1] + e[1:]) / fd).max())
    res, bound = float((np.abs(r) / fd).max()), 1024 * N * EPS * (nA + abs(lam)) * float(np.abs(x).max())
    return res <= bound, res, bound


def salpha_line(N, dPdrho, shat=1.0, alpha=0.8, theta0=0.0):
    """(theta, g, c, f) of an s-alpha line with f = g"""
    th = bo.theta_grid(N)
    g, c0 = bo.salpha_gc(th, shat, alpha, theta0)
    return th, g, -dPdrho * c0, g.copy()


def double_well(N):
    """(theta, g, c, f): g = f = 1, c = 8 (exp(-(theta - 8)^2) + exp(-(theta + 8)^2)) - 0.5: even / odd doublets"""
    th = bo.theta_grid(N)
    return th, np.ones(N), 8.0 * (np.exp(-(th - 8.0) ** 2) + np.exp(-(th + 8.0) ** 2)) - 0.5, np.ones(N)


def gersh_bounds(th, g, c, f):
    """(lmin, hi, ||A||) as the kernel's long_bounds<true> forms them: min_r (d_r - e_r - e_{r+1}) / f_r - 8 eps ||A|| and
    max_r c_r / f_r + 8 eps ||A||"""
    d, e, fd, h, gu, cu, fu = bo.assemble(th, g, c, f)
    nA = float(((np.abs(d) + e[:-1] + e[1:]) / fd).max())
    return float(((d - e[:-1] - e[1:]) / fd).min()) - 8 * EPS * nA, float(((d + e[:-1] + e[1:]) / fd).max()) + 8 * EPS * nA, nA


class ModesOracleContext(OracleContext):
    """OracleContext + geo_sturm_count / gamma_scan_modes / solve_gcf_modes (host arrays, the dense spectrum)"""

    def solve_gcf_modes(self, h, g, c, f, n_modes, gh=None, want_X=False, want_info=False):
        n_sys, N = g.shape
        th = grid_of(h, N)
        out = dict(lam=np.zeros((n_sys, n_modes)), gam=np.zeros((n_sys, n_modes)), info=np.zeros((n_sys, n_modes), dtype=np.int32), nbad=0)
        if want_X:
            out.update(X=np.zeros((n_sys, n_modes, N)), dX=np.zeros((n_sys, n_modes, N)))
        for i in range(n_sys):
            r = dense_modes(th, g[i], c[i], f[i], n_modes)
            out["lam"][i], out["gam"][i] = r["lam"], r["gam"]
            out["info"][i] = np.where(r["gap"] < r["tau"], CLUSTER_BIT << 16, 0)
            if want_X:
                out["X"][i], out["dX"][i] = r["X"], r["dX"]
        if not want_info:
            del out["info"]
        return out

    def gamma_scan_modes(self, h, bmag, gradpar, cvdrift, cvdrift0, gds2, gds21, gds22, dPdrho, theta0, n_modes, want_info=False):
        nl, N = bmag.shape
        rows = [gcf_at(dPdrho[i], bmag[i], gradpar[i], cvdrift[i], cvdrift0[i], gds2[i], gds21[i], gds22[i], t0)
                for i in range(nl) for t0 in theta0]
        g, c, f = (np.stack([r[k] for r in rows]) for k in range(3))
        r = self.solve_gcf_modes(h, g, c, f, n_modes, want_info=want_info)
        return {k: (v.reshape(nl, len(theta0), n_modes) if isinstance(v, np.ndarray) else v) for k, v in r.items()}

    def geo_sturm_count(self, h, bmag, gradpar, cvdrift, cvdrift0, gds2, gds21, gds22, dPdrho, theta0, shift=0.0):
        nl, N = bmag.shape
        th = grid_of(h, N)
        sh = np.broadcast_to(np.asarray(shift, dtype=np.float64), (nl, len(theta0)))
        cnt = np.zeros((nl, len(theta0)), dtype=np.int32)
        for i in range(nl):
            for j, t0 in enumerate(theta0):
                g, c, f = gcf_at(dPdrho[i], bmag[i], gradpar[i], cvdrift[i], cvdrift0[i], gds2[i], gds21[i], gds22[i], t0)
                cnt[i, j] = int((spectrum(th, g, c, f)[0] > sh[i, j]).sum())
        return cnt
