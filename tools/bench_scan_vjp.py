#!/usr/bin/env python3
"""The fused scan VJP beside the torch path it stands next to, same inputs, same run: autograd.gamma_scan forward + backward (the
scan kernel, then ONE ibs_gamma_scan_vjp_f64: k_scan_vjp_points + k_scan_vjp_reduce) against autograd.growth_rate forward + backward
(the theta0 fold as torch expressions, ibs_solve_gcf_f64, ibs_solve_gcf_vjp_f64, torch's backward of the fold), with the cotangent of
a smooth maximum (objective.smooth_max, beta = 20, per surface).  Shapes: 5 x 24 lines x 15 theta0 at N = 969 and 24 x 15 at
N = 2,561 (NCSX_op tables).  Per leg: wall time (host clock around work that ends in a device synchronise, median of --reps after one
warm-up, alternating) and the peak of torch.cuda.max_memory_allocated over one forward + backward, less what was allocated before
it; plus the library's own workspace of the fused backward, which torch does not see (ctx->long_ws: printed from the sizes).
No gate on speed: an analysis mode.
    python tools/bench_scan_vjp.py [--reps 31] [--out profiles/scan_vjp_bench.txt]"""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import numpy as np, torch, ibs_amd
from ibs_amd import autograd as iag
from ibs_amd.objective import smooth_max

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=31)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scan_vjp_bench.txt"))
args = ap.parse_args()
dev = torch.device("cuda", 0); ctx = ibs_amd.Context(0)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


def wall(fn):
    torch.cuda.synchronize(); t = time.perf_counter(); r = fn(); torch.cuda.synchronize()
    return time.perf_counter() - t, r


say("device: %s; forward + backward of a per-surface smooth maximum (beta = 20) of the coarse table; median of %d alternating "
    "repetitions after one warm-up of each" % (torch.cuda.get_device_name(0), args.reps))
for ns, na, nt0, N in ((5, 24, 15, 969), (1, 24, 15, 2561)):
    svals = np.linspace(0.5, 0.95, 5)[:ns]
    tabs = ibs_amd.SurfaceTables.from_wout(dict(np.load(os.path.join(ROOT, "tests", "golden", "G8_wout_ncsx_op.npz"))), svals)
    th = ibs_amd.theta_grid(N)
    h = float(th[1] - th[0])
    geo = ctx.fieldline_geometry(tabs, np.repeat(np.arange(ns), na).astype(np.int32), np.tile(np.linspace(0, np.pi, na), ns), th, device=dev)
    t0 = torch.from_numpy(np.linspace(0, np.pi / 2, nt0)).to(dev)
    base = [geo["geo"][k].clone() for k in range(7)] + [geo["dPdrho"].clone(), t0]
    grads = {}

    def leg(fn):
        def once():
            ins = [t.clone().requires_grad_(True) for t in base]
            gam = fn(h, *ins, ctx=ctx)
            smooth_max(gam.reshape(ns, na, nt0), 20.0).sum().backward()
            return [t.grad for t in ins]
        return once
    legs = dict(gamma_scan=leg(iag.gamma_scan), growth_rate=leg(iag.growth_rate))
    peak, times = {}, {k: [] for k in legs}
    for k, fn in legs.items():
        fn(); torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(); before = torch.cuda.memory_allocated()
        grads[k] = fn(); torch.cuda.synchronize()
        peak[k] = torch.cuda.max_memory_allocated() - before
    for _ in range(args.reps):
        for k, fn in legs.items():
            times[k].append(wall(fn)[0])
    n_sys = ns * na * nt0
    # (a leg whose VJP refuses a system leaves NaN rows on its line: counted, and left out of the comparison)
    bad = {k: sum(int((~torch.isfinite(t)).sum()) for t in grads[k]) for k in legs}
    both = [torch.isfinite(a) & torch.isfinite(b) for a, b in zip(grads["gamma_scan"], grads["growth_rate"])]
    rel = max(float((a - b)[m].abs().max() / b[m].abs().max()) for a, b, m in zip(grads["gamma_scan"], grads["growth_rate"], both))
    waves = min(n_sys, 8 * torch.cuda.get_device_properties(0).multi_processor_count)
    ws = 8 * (waves * (8 * N + 8) + 3 * n_sys * N) + 4 * n_sys
    say("%d x %d lines x %d theta0, N = %d (%d systems); largest relative difference of a gradient between the legs %.2e over the "
        "entries finite in both; non-finite entries: gamma_scan %d, growth_rate %d" % (ns, na, nt0, N, n_sys, rel, bad["gamma_scan"],
                                                                                      bad["growth_rate"]))
    for k in legs:
        t = np.array(times[k]) * 1e3
        say("  autograd.%-12s forward + backward %9.3f ms (min %.3f max %.3f)   peak torch memory above the inputs %8.2f MiB%s" %
            (k, np.median(t), t.min(), t.max(), peak[k] / 2 ** 20,
             "   + %.2f MiB library workspace of the fused backward" % (ws / 2 ** 20) if k == "gamma_scan" else ""))
    del geo, base, grads
    torch.cuda.empty_cache()
