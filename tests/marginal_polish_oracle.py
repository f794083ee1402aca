"""CPU restatement of ibs_marginal_theta0_polish_f64 (mu = 1 / s* of every line maximised over theta0 between the nodes of its coarse
row), from ibs_amd.row_peaks, ibs_amd.polish_theta0 and tests/marginal_oracle.py: the value of a requested theta0 is 1 / mo.solve's
scale on the line's rows there (0 with scale = inf).  MarginalPolishOracleContext lets BallooningScan.marginal_envelope and
marginal(theta0_polish=True) run without a GPU.  Test infrastructure only."""
import numpy as np

import ibs_amd
from tests import marginal_oracle as mo
from tests import marginal_points_oracle as mpo


def line_scale(h, ln7, dP, t0):
    """mo.solve's s* of one line (seven arrays) at theta0 = t0"""
    return mo.solve(h, *mo.line_gc(dP, *ln7, float(t0)))["scale"]


def newton_scale(h, g, c, s0):
    """s* of one system from a nearby guess s0: Newton on lam_max(T(s)) = 0 with mo.top_pair, the oracle's own LAPACK call --
    lam_max is convex in s with slope kappa = sum c_j x_j^2 / sum x_j^2, so the iteration converges from either side; it stops on a
    step below a tenth of the oracle's unit u.  None where it does not (the caller falls back on mo.solve)"""
    e, Dd, cj = mo.rows(h, g, c)
    N, s = len(Dd) + 2, float(s0)
    for _ in range(12):
        lam, v = mo.top_pair(s, e, Dd, cj, vector=True)
        kappa = float(np.sum(cj * v * v)) / float(np.sum(v * v))
        if not (kappa > 0 and np.isfinite(s)):
            return None
        ds = lam / kappa
        s -= ds
        if abs(ds) <= 0.1 * N * mo.EPS * float((s * np.abs(cj) + 2 * Dd).max()) / kappa:
            return s
    return None


def dense_min(h, ln7, dP, lo, hi, n=201):
    """(the minimum of n oracle samples of s* on [lo, hi], mo.solve's unit u at that sample): the first sample is mo.solve's, the
    others newton_scale's from their neighbour (a fifteenth of the time of n cold mo.solve calls)"""
    ts = np.linspace(lo, hi, n) if hi > lo else np.array([lo])
    best, s = (np.inf, 0.0), None
    for t0 in ts:
        g, c = mo.line_gc(dP, *ln7, float(t0))
        s = newton_scale(h, g, c, s) if s is not None and np.isfinite(s) else None
        if s is None:
            s = mo.solve(h, g, c)["scale"]
        if s < best[0]:
            best = (s, float(t0))
    return best[0], mo.solve(h, *mo.line_gc(dP, *ln7, best[1])).get("u", 0.0)


def polish_line(h, ln7, dP, theta0, row, node, xtol=1e-5, max_eval=32):
    """one slot: ibs_amd.polish_theta0 on mu(theta0) = 1 / line_scale about `node` of `row`.  dict(theta0, mu, scale, n_eval, status,
    points): scale is the s* of the evaluation that gave mu -- or, where the node is returned, of one more solve at the node --, and
    status carries bit 8 iff that scale is inf"""
    seen = {}

    def f(u):
        seen[u] = line_scale(h, ln7, dP, u)
        return 1.0 / seen[u]

    r = ibs_amd.polish_theta0(f, theta0, row, node, xtol, max_eval)
    scale = seen[r["theta0"]] if not r["status"] & (1 << 10) else line_scale(h, ln7, dP, theta0[node])
    status = r["status"] | (256 if r["gam"] == 0.0 else 0)
    return dict(theta0=r["theta0"], mu=r["gam"], scale=scale, n_eval=r["n_eval"], status=status, points=r["points"])


def polish(h, geo7, dPdrho, theta0, mu, n_starts=1, xtol=1e-5, max_eval=32, node=None):
    """the batch: dict(theta0, mu, scale (n_lines, K), node, n_eval, info int32 (n_lines, K): status << 16, n_found (n_lines,))"""
    mu, theta0 = np.asarray(mu, dtype=np.float64), np.asarray(theta0, dtype=np.float64)
    nl, K = len(dPdrho), int(n_starts)
    if node is None:
        nodes, n_found = ibs_amd.row_peaks(mu, K)
    else:
        nodes = np.where((np.asarray(node) >= 0) & (np.asarray(node) < mu.shape[1]), node, -1).astype(np.int32)
        n_found = np.zeros(nl, dtype=np.int32)
    out = dict(theta0=np.full((nl, K), np.nan), mu=np.full((nl, K), np.nan), scale=np.full((nl, K), np.nan),
               node=np.full((nl, K), -1, dtype=np.int32), n_eval=np.zeros((nl, K), dtype=np.int32), info=np.zeros((nl, K), dtype=np.int32),
               n_found=n_found)
    for i in range(nl):
        ln7 = [a[i] for a in geo7]
        for k in range(K):
            j = int(nodes[i, k])
            if j < 0 or np.isnan(mu[i, j]):
                continue
            r = polish_line(h, ln7, dPdrho[i], theta0, mu[i], j, xtol, max_eval)
            out["theta0"][i, k], out["mu"][i, k], out["scale"][i, k] = r["theta0"], r["mu"], r["scale"]
            out["node"][i, k], out["n_eval"][i, k], out["info"][i, k] = j, r["n_eval"], r["status"] << 16
    return out


class MarginalPolishOracleContext(mpo.MarginalPointsOracleContext):
    """MarginalPointsOracleContext + marginal_theta0_polish (host arrays); n_polish_calls counts the calls"""
    n_polish_calls = 0

    def marginal_theta0_polish(self, h, bmag, gradpar, cvdrift, cvdrift0, gds2, gds21, gds22, dPdrho, theta0, mu, n_starts=1, xtol=1e-5,
                               max_eval=32, node=None, want_scale=True, want_info=False, want_found=True):
        r = polish(h, [bmag, gradpar, cvdrift, cvdrift0, gds2, gds21, gds22], dPdrho, theta0, mu, n_starts, xtol, max_eval, node)
        self.n_polish_calls += 1
        out = {k: r[k] for k in ("theta0", "mu", "node", "n_eval")}
        out["nbad"] = int((((r["info"] >> 16) & 3) != 0).sum())
        for key, want in (("scale", want_scale), ("info", want_info), ("n_found", want_found)):
            if want:
                out[key] = r[key]
        return out
