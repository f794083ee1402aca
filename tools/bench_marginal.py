#!/usr/bin/env python3
"""The marginal-stability kernels (csrc/ibs_marginal.hip: k_marginal_gcf, k_marginal_scan) beside unchanged code on the same batches
in the same run: 2^16 s-alpha systems (bench.c5_family "smooth") at N = 513, 1025, 4097 -- against solve_gcf_nearest with sigma above
lam_max (k_solve_gcf_nearest: the same long-grid pieces, one multisection) and, at N = 4097, solve_gcf (k_solve_gcf_long) -- and the
reference-batch scan (5 surfaces x 24 alpha x 15 theta0 at N = 969, NCSX_op tables) against gamma_scan.  Scale alone, then with the
mode and the derivative rows.  Median of `--reps` timed calls after one warm-up; no gate on speed: an analysis mode.
    python tools/bench_marginal.py [--reps 5] [--out profiles/marginal_bench.txt]
--leg tangent (alone, into profiles/marginal_tangent_bench.txt): the refinement of the margin on the same scan (5 surfaces, 24 x 15
coarse grid, N = 969), jac="exact_tangent" against jac="reference" in the same run, alternating: one refinement round at the coarse
minima (geometry on 3 n lines + permuted copy + ibs_marginal_obj_w_grad_f64 against geometry on n lines + alpha-tangent +
ibs_marginal_obj_w_grad_tangent_f64, each with its copies back to the host), the rounds taken and the whole marginal(refine=True), and
one marginal_sensitivity(); host clock around work that ends in a device synchronise."""
import argparse, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import numpy as np, torch, ibs_amd, bench

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--n", type=int, default=1 << 16)
ap.add_argument("--leg", choices=("kernels", "tangent"), default="kernels")
ap.add_argument("--out", default=None)
args = ap.parse_args()
if args.out is None:
    args.out = os.path.join(ROOT, "profiles", "marginal_bench.txt" if args.leg == "kernels" else "marginal_tangent_bench.txt")
dev = torch.device("cuda", 0); ctx = ibs_amd.Context(0)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


def timed(fn):
    fn(); torch.cuda.synchronize()
    ts = []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); r = fn(); b.record(); torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e-3)
    return float(np.median(ts)), r


def row(label, n, t, kernel, passes=None, extra=""):
    say("%-34s %9.3f ms = %10.4g systems/s  %s  %s%s" % (label, t * 1e3, n / t, "passes %5.2f" % passes if passes is not None else " " * 12,
                                                         kernel, extra))


def tangent_leg():
    import time
    ns, na, nt0, N = 5, 24, 15, 969
    svals = np.linspace(0.5, 0.95, ns)
    tabs = ibs_amd.SurfaceTables.from_wout(dict(np.load(os.path.join(ROOT, "tests", "golden", "G8_wout_ncsx_op.npz"))), svals)
    scan = ibs_amd.BallooningScan(ctx, None, ibs_amd.theta_grid(N), svals, nalpha=na, ntheta0=nt0, tables=tabs, device=dev)

    def wall(fn):
        torch.cuda.synchronize(); t = time.perf_counter(); r = fn(); torch.cuda.synchronize()
        return time.perf_counter() - t, r
    say("device: %s; margin refinement, %d surfaces, %d x %d coarse grid, N = %d; median of %d alternating repetitions after one warm-up "
        "of each" % (torch.cuda.get_device_name(0), ns, na, nt0, N, args.reps))
    coarse = scan.marginal()
    x0 = np.stack([coarse["alpha"], coarse["theta0"]], axis=1)
    idx = np.arange(ns)
    legs = dict(reference=lambda: scan._marginal_points(idx, x0), exact_tangent=lambda: scan._marginal_points(idx, x0, tangent=True))
    full = {k: (lambda k=k: scan.marginal(refine=True, jac=k)) for k in legs}
    for fn in list(legs.values()) + list(full.values()):
        fn()
    t_round, t_full, res = {k: [] for k in legs}, {k: [] for k in legs}, {}
    for _ in range(args.reps):
        for k in legs:
            t_round[k].append(wall(legs[k])[0])
        for k in legs:
            t, res[k] = wall(full[k])
            t_full[k].append(t)
    t_coarse = float(np.median([wall(scan.marginal)[0] for _ in range(args.reps)]))
    say("coarse marginal() alone (geometry + marginal_scan + copy) %9.3f ms" % (t_coarse * 1e3))
    for k in legs:
        r, tr, tf = res[k], np.array(t_round[k]) * 1e3, np.array(t_full[k]) * 1e3
        say("jac=%-14s one round at the coarse minima %8.3f ms (min %.3f max %.3f)  rounds %2d  evals %s  marginal(refine=True) %8.3f ms "
            "(min %.3f max %.3f) = coarse + %.3f ms  scale %s" % (k, np.median(tr), tr.min(), tr.max(), r["rounds"], r["evals"], np.median(tf),
                                                                 tf.min(), tf.max(), np.median(tf) - t_coarse * 1e3,
                                                                 np.array2string(r["scale"], precision=9)))
    a, b = res["reference"], res["exact_tangent"]
    say("exact_tangent against reference: largest |scale ratio - 1| %.2e, |alpha difference| %.2e, |theta0 difference| %.2e; |dscale_dalpha| "
        "at the end point: reference %s, exact_tangent %s" % (np.abs(b["scale"] / a["scale"] - 1).max(), np.abs(b["alpha"] - a["alpha"]).max(),
                                                              np.abs(b["theta0"] - a["theta0"]).max(), np.abs(a["dscale"][:, 0]), np.abs(b["dscale"][:, 0])))
    scan.marginal_sensitivity()
    ts = np.array([wall(scan.marginal_sensitivity)[0] for _ in range(args.reps)]) * 1e3
    say("marginal_sensitivity() at the refined points (geometry + tangent + point launch with geo_bar + geometry VJP, %d surfaces) %8.3f ms "
        "(min %.3f max %.3f)" % (ns, np.median(ts), ts.min(), ts.max()))


if args.leg == "tangent":
    tangent_leg()
    sys.exit(0)

say("device: %s; %d systems per raw batch; median of %d calls" % (torch.cuda.get_device_name(0), args.n, args.reps))
for N in (513, 1025, 4097):
    h, g, c, f = bench.c5_family(dev, "smooth", args.n, N, 4242 + N)
    t, r = timed(lambda: ctx.marginal_gcf(h, g, c, want_info=True))
    st = r["info"] >> 16
    row("N %5d marginal_gcf scale" % N, args.n, t, ctx.last_launch()[0], float((r["info"] & 0xffff).double().mean()),
        "  flagged %d  infinite %d  s* median %.3f  unstable now %d" % (int((st & 3).ne(0).sum()), int((st & 256).ne(0).sum()),
                                                                       float(r["scale"][torch.isfinite(r["scale"])].median()),
                                                                       int((r["scale"] < 1).sum())))
    t, r = timed(lambda: ctx.marginal_gcf(h, g, c, want_X=True, want_grad=True))
    row("N %5d marginal_gcf + X + rows" % N, args.n, t, ctx.last_launch()[0])
    t, rm = timed(lambda: ctx.solve_gcf(h, g, c, f, want_info=True))
    row("N %5d solve_gcf (lam_max, gam)" % N, args.n, t, ctx.last_launch()[0], float((rm["info"] & 0xffff).double().mean()))
    above = float(rm["lam"].max()) + 1.0
    t, r = timed(lambda: ctx.solve_gcf_nearest(h, g, c, f, above, want_info=True))
    row("N %5d solve_gcf_nearest, sigma above" % N, args.n, t, ctx.last_launch()[0], float((r["info"] & 0xffff).double().mean()))
    del g, c, f, r, rm
    torch.cuda.empty_cache()

ns, na, nt0, N = 5, 24, 15, 969
svals = np.linspace(0.5, 0.95, ns)
tabs = ibs_amd.SurfaceTables.from_wout(dict(np.load(os.path.join(ROOT, "tests", "golden", "G8_wout_ncsx_op.npz"))), svals)
th = ibs_amd.theta_grid(N)
geo = ctx.fieldline_geometry(tabs, np.repeat(np.arange(ns), na).astype(np.int32), np.tile(np.linspace(0, np.pi, na), ns), th, device=dev)
t0 = torch.from_numpy(np.linspace(0, np.pi / 2, nt0)).to(dev)
geo7 = [geo["geo"][k] for k in range(7)]
n = ns * na * nt0
t, r = timed(lambda: ctx.marginal_scan(th[1] - th[0], *geo7, geo["dPdrho"], t0, want_info=True))
row("N %5d marginal_scan 5x24x15" % N, n, t, ctx.last_launch()[0], float((r["info"] & 0xffff).double().mean()),
    "  flagged %d  s* in [%.3f, %.3f]" % (int(((r["info"] >> 16) & 3).ne(0).sum()), float(r["scale"].min()), float(r["scale"].max())))
t, r = timed(lambda: ctx.marginal_scan(th[1] - th[0], *geo7, geo["dPdrho"], t0, want_grad=True))
row("N %5d marginal_scan + derivatives" % N, n, t, ctx.last_launch()[0])
t, r = timed(lambda: ctx.gamma_scan(th[1] - th[0], *geo7, geo["dPdrho"], t0, want_info=True))
row("N %5d gamma_scan 5x24x15" % N, n, t, ctx.last_launch()[0], float((r["info"] & 0xffff).double().mean()))
t, r = timed(lambda: ctx.gamma_scan_nearest(th[1] - th[0], *geo7, geo["dPdrho"], t0, 1e3, want_info=True))
row("N %5d gamma_scan_nearest, sigma above" % N, n, t, ctx.last_launch()[0], float((r["info"] & 0xffff).double().mean()))
