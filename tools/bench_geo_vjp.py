#!/usr/bin/env python3
"""The geometry's vector-Jacobian product (csrc/ibs_geometry_vjp.hip, Context.fieldline_geometry_vjp) against the forward
ibs_fieldline_geometry_f64 at the same shape, on device-resident tensors, NCSX mode counts (242 + 392), N = 969:
  365 lines = one line on each of 73 x 5 surfaces (the refined points of configs[3]);  5 lines = the base equilibrium alone.
Median of `--reps` timed calls after one warm-up (device events).  The split over the three kernels comes from the optional
outputs: alpha alone runs the points kernel and the line reduction, the two tables alone the points kernel and the modes kernel.
Then one AdjointStep.sensitivity call at given points, end to end (wall clock, synchronised; includes the host pull-back).
    python tools/bench_geo_vjp.py [--reps 20] [--json out.json]"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import numpy as np, torch, ibs_amd

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--json", default=None)
args = ap.parse_args()
dev = torch.device("cuda", 0); ctx = ibs_amd.Context(0)
wout = dict(np.load(os.path.join(ROOT, "tests", "golden", "G8_wout_ncsx_op.npz")))
SV = np.linspace(0.5, 0.95, 5)                                       # ball_scan.py:197
N = 969
th = ibs_amd.theta_grid(N)


def timed(fn):
    fn(); torch.cuda.synchronize()
    ts = []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e-3)
    return float(np.median(ts))


out = []
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
for n_eq in (73, 1):
    tabs = ibs_amd.SurfaceTables.from_wouts([wout] * n_eq, SV)
    n = n_eq * len(SV)
    rng = np.random.default_rng(1)
    ls, la, dth = t(np.arange(n, dtype=np.int32)), t(rng.uniform(0, np.pi, n)), t(th)
    geo = ctx.fieldline_geometry(tabs, ls, la, dth, device=dev)["geo"]
    gb = 1.0 / geo.abs().amax(dim=(1, 2), keepdim=True) * torch.randn_like(geo)
    db = torch.randn(n, dtype=torch.float64, device=dev)
    t_fwd = timed(lambda: ctx.fieldline_geometry(tabs, ls, la, dth, device=dev))
    t_fwd_plain = timed(lambda: ctx.fieldline_geometry(tabs, ls, la, dth, device=dev, use_rows=False))
    t_all = timed(lambda: ctx.fieldline_geometry_vjp(tabs, ls, la, dth, gb, db, device=dev))
    t_alpha = timed(lambda: ctx.fieldline_geometry_vjp(tabs, ls, la, dth, gb, db, device=dev, want=("alpha",)))
    t_tabs = timed(lambda: ctx.fieldline_geometry_vjp(tabs, ls, la, dth, gb, db, device=dev, want=("tab_mn", "tab_nyq")))
    row = dict(lines=n, N=N, forward_s=t_fwd, forward_plain_s=t_fwd_plain, vjp_s=t_all, vjp_alpha_only_s=t_alpha, vjp_tables_only_s=t_tabs,
               vjp_over_forward=t_all / t_fwd, vjp_over_forward_plain=t_all / t_fwd_plain)
    out.append(row)
    print("%4d lines x %d: forward %.1f us (one sincos per mode: %.1f us)  VJP %.1f us = %.1f x forward (%.2f x the plain form);  "
          "alpha alone (points + line reduction) %.1f us, tables alone (points + modes) %.1f us"
          % (n, N, t_fwd * 1e6, t_fwd_plain * 1e6, t_all * 1e6, t_all / t_fwd, t_all / t_fwd_plain, t_alpha * 1e6, t_tabs * 1e6))

step = ibs_amd.AdjointStep(ctx, th, SV, dev)
pts = np.stack([np.linspace(0.2, 2.0, len(SV)), np.linspace(0.0, 0.4, len(SV))], axis=1)
step.sensitivity(wout, points=pts); torch.cuda.synchronize()
ts = []
for _ in range(max(3, args.reps // 4)):
    t0 = time.perf_counter(); step.sensitivity(wout, points=pts); torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
out.append(dict(adjoint_step_sensitivity_s=float(np.median(ts)), surfaces=len(SV), N=N))
print("AdjointStep.sensitivity, %d surfaces at given points, N = %d: %.2f ms end to end" % (len(SV), N, np.median(ts) * 1e3))
if args.json:
    with open(args.json, "w") as fh:
        json.dump(out, fh, indent=1)
