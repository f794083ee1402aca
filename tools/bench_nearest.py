#!/usr/bin/env python3
"""The nearest-sigma mode (csrc/ibs_nearest.hip: k_solve_gcf_nearest) against the lam_max solvers: 2^16 s-alpha systems (bench.c5_family
"smooth") at N = 513, 1025, 4097, driven x 1 (lam_max ~ 0.1) and x 8 (lam_max up to ~5), with sigma = 0.42 (upstream's final solve,
ball_scan.py:337) and with sigma above lam_max (k = 0: the lam_max path inside the same kernel).  Growth rate wanted.  Median of
`--reps` timed calls after one warm-up.      python tools/bench_nearest.py [--reps 5] [--json out.json]"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import numpy as np, torch, ibs_amd, bench

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--n", type=int, default=1 << 16)
ap.add_argument("--json", default=None)
args = ap.parse_args()
dev = torch.device("cuda", 0); ctx = ibs_amd.Context(0)


def timed(fn):
    fn(); torch.cuda.synchronize()
    ts = []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); r = fn(); b.record(); torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e-3)
    return float(np.median(ts)), r


rows = []
for N in (513, 1025, 4097):
    h, g, c, f = bench.c5_family(dev, "smooth", args.n, N, 4242 + N)
    for drive in (1.0, 8.0):
        cd = c * drive
        t_max, rm = timed(lambda: ctx.solve_gcf(h, g, cd, f, want_info=True))
        kmax = ctx.last_launch()[0]
        above = float(rm["lam"].max()) + 1.0
        for label, sigma in (("0.42", 0.42), ("above lam_max", above)):
            t, r = timed(lambda: ctx.solve_gcf_nearest(h, g, cd, f, sigma, want_info=True))
            row = dict(N=N, n=args.n, drive=drive, sigma=label, kernel=ctx.last_launch()[0], seconds=t, solves_per_s=args.n / t,
                       passes=float((r["info"] & 0xffff).double().mean()), idx_gt0=int((r["idx"] > 0).sum()),
                       undecided=int(((r["info"] >> 16) & 32).ne(0).sum()), bad=int(((r["info"] >> 16) & 3).ne(0).sum()),
                       lam_max_kernel=kmax, lam_max_seconds=t_max, slowdown=t / t_max)
            rows.append(row)
            print("N %5d  drive x%g  sigma %-13s  %8.3f ms = %10.4g solves/s  passes %5.1f  idx>0 %6d  undecided %d  bad %d   "
                  "(lam_max: %s %7.3f ms; x %.1f)" % (N, drive, label, t * 1e3, args.n / t, row["passes"], row["idx_gt0"],
                                                       row["undecided"], row["bad"], kmax, t_max * 1e3, t / t_max), flush=True)
    del g, c, f
    torch.cuda.empty_cache()
if args.json:
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as fh:
        json.dump(rows, fh, indent=1)
