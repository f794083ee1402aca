#!/usr/bin/env python3
"""What the count-pair certificate of geometry-fed growth rates costs (csrc/ibs_certify.hip), beside the plain calls in the same run:
the headline batch of bench.py (16 surfaces x 8 alpha x 8 theta0 = 1,024 solves, N = 513) and the shape of BASELINE configs[3]
(73 x 5 surfaces x 24 alpha x 15 theta0 = 131,400 solves, N = 969: the NCSX_op lines of 5 surfaces, repeated 73 times).
Per shape: the plain scan + per-surface maximum (Context.gamma_scan_argmax), the certificate alone (certify_scan), the re-close call
alone on a table without refused systems (its list, an idle solve launch and the second certificate's early exits), the geometry-fed
count (geo_sturm_count), and the certified step = scan + certificate + re-close + per-surface maximum taken again.  Each figure is the
median over `--reps` windows of `--inner` back-to-back calls between two device synchronisations (host clock), after a warm-up.
`--plain-only` times the plain call alone: the form that also runs on a checkout without the certificate (the parent commit).
No gate on speed: a measurement.
    python tools/bench_certify.py [--reps 7] [--inner 200] [--plain-only] [--out profiles/certify_bench.txt]"""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import numpy as np, torch, ibs_amd, bench

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--inner", type=int, default=200)
ap.add_argument("--plain-only", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "certify_bench.txt"))
args = ap.parse_args()
dev = torch.device("cuda", 0); ctx = ibs_amd.Context(0)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


def timed(fn, inner):
    for _ in range(max(3, inner // 10)):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        for _ in range(inner):
            fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) / inner)
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def row(label, t, n, kernel=""):
    say("  %-46s %9.2f us  (min %8.2f, max %8.2f)  %10.4g systems/s  %s" % (label, t[0] * 1e6, t[1] * 1e6, t[2] * 1e6, n / t[0], kernel))


def shape(title, h, geo7, dP, t0, n_surf, inner):
    n = geo7[0].shape[0] * t0.shape[0]
    say("%s: %d lines x %d theta0 = %d systems, N = %d" % (title, geo7[0].shape[0], t0.shape[0], n, geo7[0].shape[1]))
    row("plain: gamma_scan_argmax", timed(lambda: ctx.gamma_scan_argmax(h, geo7, dP, t0, n_surf), inner), n, ctx.last_launch()[0])
    if args.plain_only:
        return
    sc = ctx.gamma_scan_argmax(h, geo7, dP, t0, n_surf)
    row("certificate alone: certify_scan", timed(lambda: ctx.certify_scan(h, *geo7, dP, t0, sc["lam"]), inner), n, ctx.last_launch()[0])
    cert = ctx.certify_scan(h, *geo7, dP, t0, sc["lam"])
    say("    cert words: %d certified, %d open" % (int((cert == 0).sum()), int((cert != 0).sum())))
    row("re-close alone (nothing listed)", timed(lambda: ctx.reclose_scan(h, *geo7, dP, t0, cert, sc["lam"], sc["gam"]), inner), n)
    row("count alone: geo_sturm_count(0)", timed(lambda: ctx.geo_sturm_count(h, *geo7, dP, t0, 0.0), inner), n, ctx.last_launch()[0])

    def certified():
        s = ctx.gamma_scan_argmax(h, geo7, dP, t0, n_surf)
        c = ctx.certify_scan(h, *geo7, dP, t0, s["lam"])
        ctx.reclose_scan(h, *geo7, dP, t0, c, s["lam"], s["gam"])
        return ctx.surface_argmax_pack(s["gam"].view(n_surf, -1))
    row("certified step: scan + certify + reclose + max", timed(certified, inner), n)


say("device: %s; median of %d windows%s" % (torch.cuda.get_device_name(0), args.reps, "; plain calls only" if args.plain_only else ""))
h, geo7, dP_d, th0_d, _, _, _ = bench.build_workload(0, dev)
shape("headline batch", h, geo7, dP_d, th0_d, bench.N_SURF, args.inner)

ns, na, nt0, N, n_eq = 5, 24, 15, 969, 73
svals = np.linspace(0.5, 0.95, ns)
tabs = ibs_amd.SurfaceTables.from_wout(dict(np.load(os.path.join(ROOT, "tests", "golden", "G8_wout_ncsx_op.npz"))), svals)
th = ibs_amd.theta_grid_for(11, 11)
assert len(th) == N
geo = ctx.fieldline_geometry(tabs, np.repeat(np.arange(ns), na).astype(np.int32), np.tile(np.linspace(0, np.pi, na), ns), th, device=dev)
g7 = [geo["geo"][k].repeat(n_eq, 1).contiguous() for k in range(7)]
shape("configs[3] shape", float(th[1] - th[0]), g7, geo["dPdrho"].repeat(n_eq).contiguous(), torch.from_numpy(np.linspace(0, np.pi / 2, nt0)).to(dev),
      n_eq * ns, max(10, args.inner // 20))
