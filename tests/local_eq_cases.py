"""Test-only: inputs and the oracle side of the local-equilibrium tests (tests/test_local_eq_cpu.py, tests/test_gpu_local_eq.py).  The
oracle everywhere is ibs_amd.operators.local_eq_fold (the rule in numpy) + the (g, c, f) of utils.py:1560-1562 + the CPU oracles."""
import numpy as np

from ibs_amd import local_eq_fold
from oracle import ballooning_oracle as bo

EPS = 2.220446049250313e-16


def salpha_base_line(th, theta0, shat0=1.0, alpha0=0.5):
    """the s-alpha model as a field line for the rule: B = gradpar = 1, gbdrift = cvdrift, dPdrho = -1, centre = theta0; with
    ps = -alpha0 (sin theta - sin theta0) / shat0 the triple (0, shat / shat0 - 1, alpha / alpha0) gives bishop_ball_s-alpha.py:30-45
    at (shat, alpha, theta0).  Returns (line8 (8, N), dPdrho, ps (N,))."""
    lam0 = shat0 * (th - theta0) - alpha0 * (np.sin(th) - np.sin(theta0))
    one = np.ones_like(th)
    cv = alpha0 * (np.cos(th) + np.sin(th) * lam0)
    line = np.stack([one, one, cv, alpha0 * shat0 * np.sin(th), 1 + lam0 ** 2, shat0 * lam0, shat0 ** 2 * one, cv])
    return line, -1.0, -alpha0 * (np.sin(th) - np.sin(theta0)) / shat0


def persistent_waves():
    """the persistent grid of the long path on device 0: long_waves() of csrc/ibs_api.hip, 8 waves per CU"""
    import torch
    return 8 * torch.cuda.get_device_properties(0).multi_processor_count


def assert_wave_reuse(ctx, kernel, n_sys, at_most=None):
    """the launch before this call was `kernel` on fewer blocks than systems (a wave served more than one); returns the blocks"""
    name, blocks = ctx.last_launch()
    print("%s: %d blocks for %d systems" % (name, blocks, n_sys))
    assert kernel in name and 0 < blocks < n_sys and (at_most is None or blocks <= at_most), (name, blocks, n_sys, at_most)
    return blocks


def wave_reuse_batch(waves, factor=1.3):
    """three s-alpha lines at N = 67 (theta0 = 0, 0.1, -0.3, with their ps rows) x the product of 9 theta0, 10 eps and at least 10 p:
    2,700 systems, the p axis lengthened until the batch holds `factor` x `waves` systems.  dict(th, lines, dP, centre, sigma, ps, var)"""
    import itertools
    th = bo.theta_grid(67)
    t0s = (0.0, 0.1, -0.3)
    base = [salpha_base_line(th, t0) for t0 in t0s]
    n_p = max(10, -(-int(np.ceil(factor * waves)) // (3 * 90)))
    var = np.array(list(itertools.product(np.linspace(-0.4, 0.4, 9), np.linspace(-0.9, 1.0, 10), np.linspace(0.0, 3.0, n_p))))
    return dict(th=th, lines=np.stack([b[0] for b in base]), dP=np.array([b[1] for b in base]), centre=np.array(t0s),
                sigma=np.ones(3), ps=np.stack([b[2] for b in base]), var=var)


def to_geo(lines):
    """(n_lines, 8, N) -> the (8, n_lines, N) layout of Context.fieldline_geometry"""
    return np.ascontiguousarray(np.transpose(np.asarray(lines, dtype=np.float64), (1, 0, 2)))


def rows_of(th, lines, dP, centre, sigma, var, ps=None):
    """(g, c, f), each (n_lines, n_var, N), of every (line, triple) by the rule"""
    n, nv, N = len(lines), len(var), len(th)
    g = np.empty((n, nv, N)); c = np.empty_like(g); f = np.empty_like(g)
    for i in range(n):
        for k, (t0, eps, p) in enumerate(var):
            dPv, cv, gd = local_eq_fold(th, lines[i], dP[i], centre[i], sigma[i], t0, eps, p, ps=None if ps is None else ps[i])
            g[i, k], c[i, k], f[i, k] = bo.gcf(dPv, lines[i][0], lines[i][1], cv, gd)
    return g, c, f


def norm_a(h, g, c, f):
    """the solver's ||A|| bound of every system: max_r (|d_r| + e_r + e_{r+1}) / f_r (utils.py:1574-1592)"""
    ee = (g[..., :-2] + 2 * g[..., 1:-1] + g[..., 2:]) / (2 * h * h)
    return ((np.abs(c[..., 1:-1] - ee) + ee) / f[..., 1:-1]).max(axis=-1)


def oracle_of(th, g, c, f):
    """dict(gam, lam, normA, tol_lam = 4 N eps ||A||, margin = 16 N^2 eps ||A||) of the systems g, c, f (..., N) by the C oracle"""
    from oracle import c_oracle as co
    shape, N = g.shape[:-1], g.shape[-1]
    h = float(th[1] - th[0])
    gam, lam, _ = co.solve_gcf_batch(h, g.reshape(-1, N), c.reshape(-1, N), f.reshape(-1, N))
    nA = norm_a(h, g, c, f)
    return dict(gam=gam.reshape(shape), lam=lam.reshape(shape), normA=nA, tol_lam=4 * N * EPS * nA, margin=16.0 * N * N * EPS * nA)


def counts_of(th, g, c, f, shift):
    """eigenvalues above shift (a scalar or (...,)) of every system, by the C oracle's division-form count"""
    from oracle import c_oracle as co
    shape, N = g.shape[:-1], g.shape[-1]
    sh = np.broadcast_to(np.asarray(shift, dtype=np.float64), shape).reshape(-1)
    return co.count_above_batch(float(th[1] - th[0]), g.reshape(-1, N), c.reshape(-1, N), f.reshape(-1, N), sh).reshape(shape)
