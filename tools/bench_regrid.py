#!/usr/bin/env python3
"""What the non-uniform-grid path costs: gamma_scan_theta (csrc/ibs_regrid.hip: k_assemble_regrid, then the raw solver with gh) beside
gamma_scan (the fused scan kernel: unchanged code) on the SAME arrays in the same run -- NCSX_op lines on the uniform grid, handed to
the theta path as a grid -- at 64 lines x 16 theta0, N = 513 and 120 lines x 15 theta0, N = 969.  The theta path is split into its two
launches: assemble_gcf_theta (assemble + regrid, with the allocation of its four row tensors) and solve_gcf with gh on those rows.  The
nearest existing yardstick of the first part, k_assemble_gcf_long, has no entry point of its own: it is taken as gamma_scan_nearest
minus solve_gcf_nearest on the same rows.  A clustered grid of the same window is timed as well (same arrays: only the search changes).
Device tensors throughout, device events around each call, median of `--reps` calls after one warm-up, the legs alternating; no gate on
speed: an analysis mode.
    python tools/bench_regrid.py [--reps 20] [--out profiles/regrid_bench.txt]"""
import argparse, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import numpy as np, torch, ibs_amd

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "regrid_bench.txt"))
args = ap.parse_args()
dev = torch.device("cuda", 0); ctx = ibs_amd.Context(0)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3


def clustered(N, seed=7):
    rng = np.random.default_rng(seed)
    d = np.exp(rng.uniform(np.log(0.02), np.log(5.0), N - 1))
    th = -4 * np.pi + 8 * np.pi * np.concatenate([[0.0], np.cumsum(d)]) / d.sum()
    th[0], th[-1] = -4 * np.pi, 4 * np.pi
    return th


say("device: %s; median (min .. max) of %d calls after one warm-up, legs alternating" % (torch.cuda.get_device_name(0), args.reps))
tabs = ibs_amd.SurfaceTables.from_wout(dict(np.load(os.path.join(ROOT, "tests", "golden", "G8_wout_ncsx_op.npz"))), np.linspace(0.5, 0.95, 8))
for n_lines, nt0, N in ((64, 16, 513), (120, 15, 969)):
    th = ibs_amd.theta_grid(N)
    h = th[1] - th[0]
    ls = (np.arange(n_lines) % 8).astype(np.int32)
    geo = ctx.fieldline_geometry(tabs, ls, np.linspace(0, np.pi, n_lines), th, device=dev)
    geo7, dP = [geo["geo"][k] for k in range(7)], geo["dPdrho"]
    t0 = torch.from_numpy(np.linspace(0, np.pi / 2, nt0)).to(dev)
    thd, thc, win = torch.from_numpy(th).to(dev), torch.from_numpy(clustered(N)).to(dev), (th[0], th[-1])
    n = n_lines * nt0
    rows = ctx.assemble_gcf_theta(thd, *geo7, dP, t0, window=win)
    g, gh, c, f = (rows[k].reshape(n, N) for k in ("g", "gh", "c", "f"))
    legs = {
        "gamma_scan (uniform h)": lambda: ctx.gamma_scan(h, *geo7, dP, t0),
        "gamma_scan_theta, uniform grid": lambda: ctx.gamma_scan_theta(thd, *geo7, dP, t0, window=win),
        "  assemble_gcf_theta": lambda: ctx.assemble_gcf_theta(thd, *geo7, dP, t0, window=win),
        "  solve_gcf with gh": lambda: ctx.solve_gcf(rows["h"], g, c, f, gh=gh),
        "gamma_scan_theta, clustered grid": lambda: ctx.gamma_scan_theta(thc, *geo7, dP, t0, window=win),
        "  assemble_gcf_theta, clustered": lambda: ctx.assemble_gcf_theta(thc, *geo7, dP, t0, window=win),
        "gamma_scan_nearest, sigma above": lambda: ctx.gamma_scan_nearest(h, *geo7, dP, t0, 1e3),
        "  solve_gcf_nearest on the rows": lambda: ctx.solve_gcf_nearest(h, g, c, f, 1e3),
    }
    kern = {}
    for k, fn in legs.items():
        fn(); torch.cuda.synchronize()
        kern[k] = ctx.last_launch()[0]
    ts = {k: [] for k in legs}
    for _ in range(args.reps):
        for k, fn in legs.items():
            ts[k].append(once(fn))
    med = {k: float(np.median(v)) for k, v in ts.items()}
    a, b = ctx.gamma_scan(h, *geo7, dP, t0), ctx.gamma_scan_theta(thd, *geo7, dP, t0, window=win)
    say("%d lines x %d theta0, N = %d (%d systems); |gam_theta - gam_scan| on the uniform grid %.2e"
        % (n_lines, nt0, N, n, float((a["gam"] - b["gam"]).abs().max())))
    base = med["gamma_scan (uniform h)"]
    for k in legs:
        v = np.array(ts[k]) * 1e3
        say("  %-34s %8.3f ms (%7.3f .. %7.3f)  %5.2f x gamma_scan  %s" % (k, med[k] * 1e3, v.min(), v.max(), med[k] / base, kern[k]))
    say("  %-34s %8.3f ms  (gamma_scan_nearest - solve_gcf_nearest: k_assemble_gcf_long, three rows into the workspace)"
        % ("  assemble yardstick", (med["gamma_scan_nearest, sigma above"] - med["  solve_gcf_nearest on the rows"]) * 1e3))
