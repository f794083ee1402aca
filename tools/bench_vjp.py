#!/usr/bin/env python3
"""The exact gam / lam vector-Jacobian product (csrc/ibs_vjp.hip: k_solve_gcf_vjp, Context.solve_gcf_vjp) against the forward
ibs_solve_gcf_f64 of the same batch (with X, as the autograd forward calls it, and without): 1,024 systems at N = 513; 1,800 at N = 969
(the coarse scan of configs[3]: 5 surfaces x 24 alphas x 15 theta0, ball_scan.py:223-226, on synthetic field lines); 64 at N = 4,097.
Median of `--reps` timed calls after one warm-up (device events).  The lam_bar-only call skips the adjoint solve (r, the serial
pass B and the projection): the difference is that solve's share of the VJP.
    python tools/bench_vjp.py [--reps 20] [--json out.json] [--profile]     (--profile: a few calls only, for rocprofv3)"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import numpy as np, torch, ibs_amd
from oracle import ballooning_oracle as bo
from tests.helpers import synthetic_fieldlines

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--json", default=None)
ap.add_argument("--profile", action="store_true")
args = ap.parse_args()
if args.profile:
    args.reps = 3
dev = torch.device("cuda", 0); ctx = ibs_amd.Context(0)


def timed(fn):
    fn(); torch.cuda.synchronize()
    ts = []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); r = fn(); b.record(); torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e-3)
    return float(np.median(ts)), r


def batch(n_sys, N, n_surf):
    """(h, g, c, f) of n_sys (line, theta0) systems: n_surf surfaces x lines x 15 theta0 in [0, pi/2] (or fewer)"""
    th = bo.theta_grid(N)
    n_t0 = 15 if n_sys % 15 == 0 else 1
    n_lines = n_sys // n_t0
    per = n_lines // n_surf
    rows = []
    for s in np.linspace(0.5, 0.95, n_surf):
        for ln in synthetic_fieldlines(th)(s, np.linspace(0, np.pi, per)):
            dP = bo.dPdrho_of(ln[2], ln[7], ln[0])
            for t0 in np.linspace(0, np.pi / 2, n_t0):
                cv, gd = bo.fold_theta0(t0, *ln[2:7])
                rows.append(bo.gcf(dP, ln[0], ln[1], cv, gd))
    g, c, f = (torch.tensor(np.stack([r[i] for r in rows]), device=dev) for i in range(3))
    return float(th[1] - th[0]), g, c, f


out = []
for n_sys, N, n_surf in ((1024, 513, 4), (1800, 969, 5), (64, 4097, 4)):
    h, g, c, f = batch(n_sys, N, n_surf)
    assert g.shape == (n_sys, N)
    t_fwd, r = timed(lambda: ctx.solve_gcf(h, g, c, f))
    k_fwd = ctx.last_launch()[0]
    t_fwdx, r = timed(lambda: ctx.solve_gcf(h, g, c, f, want_X=True))
    ones = torch.ones(n_sys, dtype=torch.float64, device=dev)
    t_vjp, v = timed(lambda: ctx.solve_gcf_vjp(h, g, c, f, r["lam"], r["X"], gam_bar=ones, lam_bar=ones, want_info=True))
    k_vjp = ctx.last_launch()[0]
    bad = int(((v["info"] >> 16) != 0).sum())
    # lam_bar alone: gam_bar = 0 skips r, the serial adjoint solve (pass B) and the projection -- what is left is the two 64-lane passes
    t_lam, _ = timed(lambda: ctx.solve_gcf_vjp(h, g, c, f, r["lam"], r["X"], lam_bar=ones))
    row = dict(n_sys=n_sys, N=N, forward_kernel=k_fwd, forward_ms=t_fwd * 1e3, forward_X_ms=t_fwdx * 1e3, vjp_kernel=k_vjp,
               vjp_ms=t_vjp * 1e3, vjp_over_forward=t_vjp / t_fwd, vjp_over_forward_X=t_vjp / t_fwdx, flagged=bad,
               vjp_lam_only_ms=t_lam * 1e3, adjoint_solve_share=(t_vjp - t_lam) / t_vjp)
    out.append(row)
    print("%5d x N = %5d   forward %-34s %8.3f ms (with X %8.3f)   vjp %-22s %8.3f ms   vjp / forward %5.2f (with X %5.2f)   flagged %d"
          "   lam_bar only %8.3f ms: adjoint solve %4.0f %%"
          % (n_sys, N, k_fwd, t_fwd * 1e3, t_fwdx * 1e3, k_vjp, t_vjp * 1e3, t_vjp / t_fwd, t_vjp / t_fwdx, bad, t_lam * 1e3,
             100 * (t_vjp - t_lam) / t_vjp), flush=True)
if args.json:
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as fh:
        json.dump(out, fh, indent=1)
