#!/usr/bin/env python3
"""The geometry's alpha-tangent (csrc/ibs_geometry_tangent.hip, Context.fieldline_geometry_dalpha) against the forward row kernels
and against k_geo_vjp_points (the VJP with alpha_bar alone: points kernel + line reduction) at the same shape, on device-resident
tensors, NCSX mode counts (242 + 392), N = 969:
  365 lines = one line on each of 73 x 5 surfaces (the refined points of configs[3]);  5 lines = the base equilibrium alone.
Then one refinement round at those points, jac="exact_tangent" (forward on n lines + tangent + ibs_obj_w_grad_exact_tangent_f64) against
jac="exact" (forward on 3 n lines + the permuted copy + ibs_obj_w_grad_exact_f64), device time of the launches of a round.
Median of `--reps` timed calls after one warm-up (device events).
    python tools/bench_geo_tangent.py [--reps 20] [--json out.json]"""
import argparse, json, os, sys
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
h = float(th[1] - th[0])
DEL = 0.004


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
    al = rng.uniform(0.1, np.pi - 0.1, n)
    ls, la, dth = t(np.arange(n, dtype=np.int32)), t(al), t(th)
    t0 = t(rng.uniform(0.0, 0.4, n))
    geo = ctx.fieldline_geometry(tabs, ls, la, dth, device=dev)["geo"]
    gb = 1.0 / geo.abs().amax(dim=(1, 2), keepdim=True) * torch.randn_like(geo)
    t_fwd = timed(lambda: ctx.fieldline_geometry(tabs, ls, la, dth, device=dev))
    t_tan = timed(lambda: ctx.fieldline_geometry_dalpha(tabs, ls, la, dth, device=dev))
    t_vjp = timed(lambda: ctx.fieldline_geometry_vjp(tabs, ls, la, dth, gb, None, device=dev, want=("alpha",)))
    ls3 = t(np.repeat(np.arange(n, dtype=np.int32), 3))
    la3 = t(np.stack([al - 0.5 * DEL, al, al + 0.5 * DEL], axis=1).reshape(-1))

    def round_exact():
        r = ctx.fieldline_geometry(tabs, ls3, la3, dth, device=dev)
        return ctx.obj_w_grad_exact(h, r["geo"].view(8, n, 3, N).permute(1, 2, 0, 3).contiguous(), t0, DEL)

    def round_tangent():
        r = ctx.fieldline_geometry(tabs, ls, la, dth, device=dev)
        ra = ctx.fieldline_geometry_dalpha(tabs, ls, la, dth, device=dev)
        return ctx.obj_w_grad_exact_tangent(h, r["geo"], ra["geo_da"], t0)

    ja = round_exact()[1][:, 0]; jb = round_tangent()[1][:, 0]
    gap = float(((ja - jb).abs() / jb.abs().max()).max())
    t_re, t_rt = timed(round_exact), timed(round_tangent)
    g3 = ctx.fieldline_geometry(tabs, ls3, la3, dth, device=dev)["geo"].view(8, n, 3, N).permute(1, 2, 0, 3).contiguous()
    gda = ctx.fieldline_geometry_dalpha(tabs, ls, la, dth, device=dev)["geo_da"]
    t_pe = timed(lambda: ctx.obj_w_grad_exact(h, g3, t0, DEL))
    t_pt = timed(lambda: ctx.obj_w_grad_exact_tangent(h, geo, gda, t0))
    row = dict(lines=n, N=N, forward_s=t_fwd, tangent_s=t_tan, vjp_alpha_only_s=t_vjp, round_exact_s=t_re, round_exact_tangent_s=t_rt,
               points_exact_s=t_pe, points_exact_tangent_s=t_pt, jac_alpha_gap_over_max=gap)
    out.append(row)
    print("%4d lines x %d: forward (rows) %.1f us  tangent %.1f us = %.1f x forward, %.2f x the VJP's points + line reduction (%.1f us);  "
          "round: exact %.1f us (point kernel %.1f), exact_tangent %.1f us (point kernel %.1f) = %.2f x;  largest |jac_alpha(exact) - "
          "jac_alpha(exact_tangent)| / max |jac_alpha| %.2e"
          % (n, N, t_fwd * 1e6, t_tan * 1e6, t_tan / t_fwd, t_tan / t_vjp, t_vjp * 1e6, t_re * 1e6, t_pe * 1e6, t_rt * 1e6, t_pt * 1e6,
             t_rt / t_re, gap))
if args.json:
    with open(args.json, "w") as fh:
        json.dump(out, fh, indent=1)
