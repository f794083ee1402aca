"""Test-only: inputs and the oracle side of the local-equilibrium boundary tests (tests/test_local_eq_boundary_cpu.py,
tests/test_gpu_local_eq_boundary.py).  Every verdict is the C oracle's on rows formed by ibs_amd.local_eq_fold at
ibs_amd.local_eq_ray_triples(rays, t) (tests/local_eq_cases.py)."""
import numpy as np

from ibs_amd import local_eq_ray_nodes, local_eq_ray_triples
from oracle import ballooning_oracle as bo
from tests import local_eq_cases as lc

T0S = (0.0, 0.1, -0.3)           # the three s-alpha base lines (shat0 = 1, alpha0 = 0.5) with their ps rows
# the rays of the root-property test: p-rays over t in [0.2, 3.0] at eps = shat - 1, shat in {0.1, 0.3, 0.9, 1.9}; one eps-ray at
# p = 1.6 over eps in [-0.9, 1.0]; one oblique ray, folded at theta0 = 0.05, from (eps, p) = (-0.5, 0.3) to (0.5, 2.3)
RAYS = np.array([(0.0, sh - 1.0, 0.0, 0.0, 1.0, 0.2, 3.0) for sh in (0.1, 0.3, 0.9, 1.9)]
                + [(0.0, 0.0, 1.6, 1.0, 0.0, -0.9, 1.0), (0.05, -0.5, 0.3, 0.5, 1.0, 0.0, 2.0)])


def salpha_lines(th, t0s=T0S):
    """dict(th, lines (n, 8, N), dP, centre, sigma, ps) of the s-alpha base lines at theta0 in t0s"""
    base = [lc.salpha_base_line(th, t0) for t0 in t0s]
    return dict(th=th, lines=np.stack([b[0] for b in base]), dP=np.array([b[1] for b in base]), centre=np.array(t0s),
                sigma=np.ones(len(t0s)), ps=np.stack([b[2] for b in base]))


def call_args(b):
    """the positional arguments of Context.local_eq_boundary / local_eq_scan up to sigma"""
    return b["th"][0], b["th"][1] - b["th"][0], lc.to_geo(b["lines"]), b["dP"], b["centre"], b["sigma"]


def oracle_at(b, rays, t, shift=0.0):
    """the oracle at the parameters t (n_lines, n_ray, K) of the rays (n_ray, 7): dict(lam, margin, count), each (n_lines, n_ray, K)"""
    t = np.asarray(t, dtype=np.float64)
    n, nr, K = t.shape
    lam = np.empty(t.shape); margin = np.empty(t.shape); count = np.empty(t.shape, dtype=np.int64)
    for i in range(n):
        var = local_eq_ray_triples(rays[:, None, :], t[i]).reshape(-1, 3)
        args = (b["th"], b["lines"][i:i + 1], b["dP"][i:i + 1], b["centre"][i:i + 1], b["sigma"][i:i + 1], var)
        g, c, f = lc.rows_of(*args, ps=None if b["ps"] is None else b["ps"][i:i + 1])
        ref = lc.oracle_of(b["th"], g, c, f)
        lam[i] = ref["lam"].reshape(nr, K); margin[i] = ref["margin"].reshape(nr, K)
        count[i] = lc.counts_of(b["th"], g, c, f, shift).reshape(nr, K)
    return dict(lam=lam, margin=margin, count=count)


def oracle_nodes(b, rays, shift=0.0):
    """oracle_at the 64 pass-0 nodes of every ray, with the nodes under "t" """
    t = np.broadcast_to(local_eq_ray_nodes(rays), (len(b["lines"]),) + (len(rays), 64))
    return dict(oracle_at(b, rays, t, shift), t=t)


def flips(unstable):
    """node indices k with unstable[k] != unstable[k + 1], increasing"""
    u = np.asarray(unstable, dtype=bool)
    return np.nonzero(u[:-1] != u[1:])[0]


def status(r):
    return np.asarray(r["info"]) >> 16


def check_sides(b, rays, r, shift=0.0, delta=1e-5, what=""):
    """the root property of every returned crossing: with D = delta (t_hi - t_lo), the oracle's lam_max is below shift at t -+ D on the
    stable side and above it on the other, both farther from shift than the count margin; prints the worst ratio first.  Returns the
    parameters (n_lines, n_ray, max_cross, 2) = (stable side, unstable side), NaN where there is no crossing."""
    ts, tu, nc = np.asarray(r["t_stable"]), np.asarray(r["t_unstable"]), np.asarray(r["n_cross"])
    D = delta * (rays[:, 6] - rays[:, 5])[None, :, None]
    up = ts < tu                                             # stable below the crossing
    tm = 0.5 * (ts + tu)
    have = np.arange(ts.shape[2])[None, None, :] < nc[:, :, None]
    assert np.isfinite(tm[have]).all() and np.isnan(ts[~have]).all() and np.isnan(tu[~have]).all(), what
    side = np.stack([np.where(up, tm - D, tm + D), np.where(up, tm + D, tm - D)], axis=-1)
    q = np.where(have[..., None], side, 0.5 * (rays[:, 5] + rays[:, 6])[None, :, None, None])      # (a valid t where there is none)
    ref = oracle_at(b, rays, q.reshape(q.shape[0], q.shape[1], -1), shift)
    lam = ref["lam"].reshape(q.shape) - shift
    ratio = np.abs(lam) / ref["margin"].reshape(q.shape)
    print("%s: %d crossings, min |lam - shift| at t -+ D %.2e, min |lam - shift| / margin %.2e"
          % (what, have.sum(), np.abs(lam[have]).min() if have.any() else np.nan, ratio[have].min() if have.any() else np.nan))
    assert (ratio[have] > 1.0).all(), (what, ratio[have].min())
    assert (lam[..., 0][have] < 0).all() and (lam[..., 1][have] > 0).all(), what
    return np.where(have[..., None], side, np.nan)
