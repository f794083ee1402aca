#!/usr/bin/env python3
"""The local-equilibrium scan (csrc/ibs_local_eq.hip: k_local_eq_scan) beside the routes to the same numbers that exist without it, in
the same run, alternating: lines of the G8 surface tables (2 surfaces x 12 alpha = 24 lines) at N = 969.
  full diagram    24 lines x 3 theta0 x 32 eps x 32 p = 73,728 systems: gam + lam + count, and count_only
  shear axis      the p = 1 plane (24 x 3 x 32 = 2,304 systems) by ONE local_eq_scan call on the staged lines against the route of the
                  parent commit: per eps value one fieldline_geometry launch on tables with d_iota_d_s (1 + eps) + one gamma_scan, 32 of
                  each (the 32 table sets are resident before the clock starts); the largest |gam difference| of the two routes is printed
  identity plane  eps = 0, p = 1: local_eq_scan (division form, rows in the per-wave workspace) against the register-resident
                  k_gamma_scan on the same (line, theta0) systems, 24 x 3 and 24 x 128: the price per system of the long-grid path
Host clock around calls that end in a device synchronise; median of `--reps` alternating repetitions after one warm-up of each.  No gate
on speed: an analysis mode.
    python tools/bench_local_eq.py [--reps 7] [--out profiles/local_eq_bench.txt]"""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import numpy as np, torch, ibs_amd

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--n-eps", type=int, default=32)
ap.add_argument("--n-p", type=int, default=32)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "local_eq_bench.txt"))
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


def alternating(legs):
    """{name: fn} -> {name: (median s, min s, max s, last result)}; one warm-up of each, then args.reps rounds of all legs in turn"""
    for fn in legs.values():
        wall(fn)
    ts, res = {k: [] for k in legs}, {}
    for _ in range(args.reps):
        for k, fn in legs.items():
            t, res[k] = wall(fn)
            ts[k].append(t)
    return {k: (float(np.median(v)), min(v), max(v), res[k]) for k, v in ts.items()}


def row(label, n, t, extra=""):
    say("%-52s %9.3f ms (min %8.3f max %8.3f) = %9.4g systems/s = %8.3f us per system  %s" % (
        label, t[0] * 1e3, t[1] * 1e3, t[2] * 1e3, n / t[0], t[0] / n * 1e6, extra))


N, n_t0 = 969, 3
g8 = dict(np.load(os.path.join(ROOT, "tests", "golden", "G8_surface_tables.npz")))
tabs = ibs_amd.SurfaceTables.from_arrays(g8)
surf = np.repeat(np.array([1, 2], dtype=np.int32), 12)
alpha = np.tile(np.linspace(0.0, np.pi, 12), 2)
n_lines = len(surf)
th = ibs_amd.theta_grid(N)
h = float(th[1] - th[0])
theta0 = np.linspace(0.0, 0.5 * np.pi, n_t0)
eps = np.linspace(-0.75, 1.0, args.n_eps)
p = np.linspace(0.0, 3.0, args.n_p)
sigma = np.sign(-tabs.scal[surf, 4])
base = ctx.fieldline_geometry(tabs, surf, alpha, th, device=dev)
geo7 = [base["geo"][k] for k in range(7)]
say("device: %s; %d lines of the G8 tables, N = %d; median of %d alternating repetitions after one warm-up of each; host clock around "
    "synchronised calls" % (torch.cuda.get_device_name(0), n_lines, N, args.reps))

# ---- full diagram
var = np.stack([a.ravel() for a in np.meshgrid(theta0, eps, p, indexing="ij")], axis=1)
d_var = torch.from_numpy(var).to(dev)
d_alpha, d_sigma = torch.from_numpy(alpha).to(dev), torch.from_numpy(sigma).to(dev)
scan = lambda v, **kw: ctx.local_eq_scan(th[0], h, base["geo"], base["dPdrho"], d_alpha, d_sigma, v, want_info=True, **kw)
r = alternating(dict(full=lambda: scan(d_var), count_only=lambda: scan(d_var, count_only=True)))
n = n_lines * len(var)
info = r["full"][3]["info"]
row("full diagram %d x %d x %d x %d, gam + lam + count" % (n_lines, n_t0, len(eps), len(p)), n, r["full"],
    "passes %.2f  flagged %d  unstable %d  %s" % (float((info & 0xffff).double().mean()), int(((info >> 16) & 3).ne(0).sum()),
                                                  int((r["full"][3]["count"] > 0).sum()), ctx.last_launch()[0]))
row("the same, count_only", n, r["count_only"], "counts equal: %s" % bool(torch.equal(r["count_only"][3]["count"], r["full"][3]["count"])))

# ---- shear axis: one call on the staged lines against one geometry launch + one gamma_scan per eps value
varied = [ibs_amd.SurfaceTables.from_arrays(dict(g8, d_iota_d_s=g8["d_iota_d_s"] * (1.0 + e))) for e in eps]
for t in varied:
    ctx.fieldline_geometry(t, surf, alpha, th, device=dev)          # (the table sets go up once, before the clock)
d_t0 = torch.from_numpy(theta0).to(dev)
var_s = np.stack([a.ravel() for a in np.meshgrid(theta0, eps, [1.0], indexing="ij")], axis=1)
d_var_s = torch.from_numpy(var_s).to(dev)


def baseline():
    out = []
    for t in varied:
        q = ctx.fieldline_geometry(t, surf, alpha, th, device=dev)
        out.append(ctx.gamma_scan(h, *[q["geo"][k] for k in range(7)], q["dPdrho"], d_t0)["gam"])
    return torch.stack(out, dim=2)                                   # (n_lines, n_theta0, n_eps)


r = alternating(dict(scan=lambda: scan(d_var_s), baseline=baseline))
n = n_lines * len(var_s)
diff = float((r["scan"][3]["gam"].reshape(n_lines, n_t0, len(eps)) - r["baseline"][3]).abs().max())
row("shear axis %d x %d x %d: one local_eq_scan" % (n_lines, n_t0, len(eps)), n, r["scan"])
row("the same: %d x (fieldline_geometry + gamma_scan)" % len(eps), n, r["baseline"],
    "baseline / scan %.2f  max |gam difference| %.2e" % (r["baseline"][0] / r["scan"][0], diff))

# ---- identity plane: the division-form long-grid path against the register-resident k_gamma_scan
for nt in (n_t0, 128):
    t0 = np.linspace(0.0, 0.5 * np.pi, nt)
    d_t0i = torch.from_numpy(t0).to(dev)
    d_var_i = torch.from_numpy(np.stack([t0, np.zeros(nt), np.ones(nt)], axis=1)).to(dev)
    names = {}

    def resident():
        out = ctx.gamma_scan(h, *geo7, base["dPdrho"], d_t0i)
        names["resident"] = ctx.last_launch()[0]
        return out

    r = alternating(dict(scan=lambda: scan(d_var_i), resident=resident))
    n = n_lines * nt
    diff = float((r["scan"][3]["gam"] - r["resident"][3]["gam"]).abs().max())
    row("identity plane %d x %d: local_eq_scan" % (n_lines, nt), n, r["scan"])
    row("the same: gamma_scan", n, r["resident"], "local_eq_scan / gamma_scan per system %.2f  max |gam difference| %.2e  %s" % (
        r["scan"][0] / r["resident"][0], diff, names["resident"]))
