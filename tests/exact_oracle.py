"""CPU restatement of ibs_obj_w_grad_exact_f64 (the refinement's objective with the exact gradient of the gam it returns), built from
the oracle's public pieces and tests/vjp_oracle.py: the three lines' dPdrho and rows (bo.dPdrho_of, bo.fold_theta0, bo.gcf), the
eigenpair (bo.solve_gcf, or the dense nearest-sigma restatement), its exact vector-Jacobian product in the rows (gcf_vjp: the bordered
adjoint system, not the kernel's twisted split) and the two contractions with the theta0 tangent (utils.py:1669-1673) and the alpha
tangent (right minus left line, each with its own dPdrho, over del_alpha: utils.py:1683-1718).  ExactOracleContext lets the scan
driver's jac="exact" plumbing run without a GPU."""
import numpy as np

from oracle import ballooning_oracle as bo
from tests.helpers import OracleContext
from tests.vjp_oracle import eigenpair, gcf_vjp


def grid_of(h, N):
    return np.linspace(-h * (N - 1) / 2, h * (N - 1) / 2, N)


def line_rows(line, theta0):
    """(dPdrho, g, c, f) of one field line (8, N) at theta0, the line's own dPdrho (utils.py:1657-1660, 1560-1562)"""
    dP = bo.dPdrho_of(line[2], line[7], line[0])
    cv, gd = bo.fold_theta0(theta0, line[2], line[3], line[4], line[5], line[6])
    return (dP,) + tuple(bo.gcf(dP, line[0], line[1], cv, gd))


def obj_w_grad_exact_lines(th, theta0, lines, sigma=None, del_alpha=0.004):
    """(val, jac, dict(gam, lam)) = (-gam, (-dgam/dalpha, -dgam/dtheta0)) on the three lines (alpha - d/2, alpha, alpha + d/2), each
    (8, N): lam_max's eigenpair, or with sigma the one nearest it"""
    dP, g, c, f = line_rows(lines[1], theta0)
    gam, lam, X = eigenpair(th, g, c, f, sigma)
    gb, cb, fb = gcf_vjp(th, g, c, f, lam, X)
    bmag, gradpar, _, cvdrift0, _, gds21, gds22, _ = lines[1]
    gp = np.abs(gradpar)
    dgd = 2 * gds21 + 2 * theta0 * gds22
    g_t, c_t, f_t = gp * dgd / bmag, -1 * dP * cvdrift0 * 1 / (gp * bmag), dgd / bmag ** 2 * 1 / (gp * bmag)      # utils.py:1669-1673
    jt = gb @ g_t + cb @ c_t + fb @ f_t
    _, g_r, c_r, f_r = line_rows(lines[2], theta0)
    _, g_l, c_l, f_l = line_rows(lines[0], theta0)
    ja = (gb @ (g_r - g_l) + cb @ (c_r - c_l) + fb @ (f_r - f_l)) / del_alpha
    return -gam, np.array([-ja, -jt]), dict(gam=gam, lam=lam)


class ExactOracleContext(OracleContext):
    """OracleContext + obj_w_grad_exact (host arrays): eigenpair -> gcf_vjp -> the two contractions"""

    def obj_w_grad_exact(self, h, geo, theta0, del_alpha=0.004, sigma=None, want_info=False):
        n, _, _, N = geo.shape
        th = grid_of(h, N)
        sig = None if sigma is None else np.broadcast_to(np.asarray(sigma, dtype=np.float64), (n,))
        val, jac, gam, lam = np.zeros(n), np.zeros((n, 2)), np.zeros(n), np.zeros(n)
        self.n_exact_evals = getattr(self, "n_exact_evals", 0) + n
        for k in range(n):
            val[k], jac[k], r = obj_w_grad_exact_lines(th, theta0[k], geo[k], None if sig is None else sig[k], del_alpha)
            gam[k], lam[k] = r["gam"], r["lam"]
        info = dict(gam=gam, lam=lam, idx=np.zeros(n, dtype=np.int32), info=np.zeros(n, dtype=np.int32))
        return (val, jac, info) if want_info else (val, jac)
