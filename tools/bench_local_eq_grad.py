#!/usr/bin/env python3
"""What the derivatives of the local-equilibrium mode cost (csrc/ibs_local_eq_grad.hip: k_local_eq_grad), beside the calls that give
the values alone, in the same run, alternating: the 24 lines of tools/bench_local_eq.py (2 surfaces x 12 alpha of the G8 tables) at
N = 969, device tensors.
  points   the shear axis of tools/bench_local_eq.py, 24 lines x 3 theta0 x 32 eps at p = 1 = 2,304 systems: local_eq_scan (gam + lam)
           beside local_eq_grad on the same (line, triple) pairs as points -- lam + gam alone, with dlam, with dlam and the eight planes
  crossings  the 24 x 96 p-rays over [--p-lo, --p-hi] of tools/bench_local_eq_boundary.py: local_eq_boundary beside
           local_eq_boundary_grad (the boundary call, the gather on the host and one local_eq_grad call at the crossings), without and
           with the planes of t*
Host clock around calls that end in a device synchronise; median of `--reps` alternating repetitions after one warm-up of each.  No
gate on speed: an analysis mode.
    python tools/bench_local_eq_grad.py [--reps 7] [--out profiles/local_eq_grad_bench.txt]"""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import numpy as np, torch, ibs_amd

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--n-eps", type=int, default=32)
ap.add_argument("--p-lo", type=float, default=0.0)
ap.add_argument("--p-hi", type=float, default=3.0)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "local_eq_grad_bench.txt"))
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
    say("%-64s %9.3f ms (min %8.3f max %8.3f) = %8.3f us per system  %s" % (label, t[0] * 1e3, t[1] * 1e3, t[2] * 1e3, t[0] / n * 1e6, extra))


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
sigma = np.sign(-tabs.scal[surf, 4])
base = ctx.fieldline_geometry(tabs, surf, alpha, th, device=dev)
geo, dP = base["geo"], base["dPdrho"]
d_alpha, d_sigma = torch.from_numpy(alpha).to(dev), torch.from_numpy(sigma).to(dev)
say("device: %s; %d lines of the G8 tables, N = %d; median of %d alternating repetitions after one warm-up of each; host clock around "
    "synchronised calls" % (torch.cuda.get_device_name(0), n_lines, N, args.reps))

# ---- points: the shear axis
tt, ee = (a.ravel() for a in np.meshgrid(theta0, eps, indexing="ij"))
var = np.stack([tt, ee, np.ones_like(tt)], axis=1)
n_var = len(var)
d_var = torch.from_numpy(var).to(dev)
d_line_of = torch.arange(n_lines, dtype=torch.int32, device=dev).repeat_interleave(n_var)
d_pts = d_var.repeat(n_lines, 1).contiguous()
names = {}


def grad(want_grad, want_geo_bar):
    out = ctx.local_eq_grad(th[0], h, geo, dP, d_alpha, d_sigma, d_line_of, d_pts, want_grad=want_grad, want_geo_bar=want_geo_bar, want_info=True)
    names["grad"] = "%s on %d blocks" % ctx.last_launch()
    return out


r = alternating(dict(scan=lambda: ctx.local_eq_scan(th[0], h, geo, dP, d_alpha, d_sigma, d_var, want_info=True),
                     values=lambda: grad(False, False), dlam=lambda: grad(True, False), planes=lambda: grad(True, True)))
n = n_lines * n_var
same = bool(torch.equal(r["scan"][3]["lam"].reshape(-1), r["values"][3]["lam"]) and torch.equal(r["scan"][3]["gam"].reshape(-1), r["values"][3]["gam"]))
flagged = int(((r["planes"][3]["info"] >> 16) & 3).ne(0).sum())
row("%d lines x %d triples: local_eq_scan (gam + lam + count)" % (n_lines, n_var), n, r["scan"])
row("local_eq_grad, lam + gam alone", n, r["values"], "bits of the scan: %s  %s" % (same, names["grad"]))
row("local_eq_grad with dlam", n, r["dlam"], "/ scan %.2f" % (r["dlam"][0] / r["scan"][0]))
row("local_eq_grad with dlam and the eight planes", n, r["planes"], "/ scan %.2f  flagged %d" % (r["planes"][0] / r["scan"][0], flagged))

# ---- crossings: the p-rays of the boundary bench
zero, one = np.zeros_like(tt), np.ones_like(tt)
rays = np.stack([tt, ee, zero, zero, one, np.full_like(tt, args.p_lo), np.full_like(tt, args.p_hi)], axis=1)
d_rays = torch.from_numpy(rays).to(dev)
r = alternating(dict(boundary=lambda: ctx.local_eq_boundary(th[0], h, geo, dP, d_alpha, d_sigma, d_rays, want_info=True),
                     grad=lambda: ctx.local_eq_boundary_grad(th[0], h, geo, dP, d_alpha, d_sigma, d_rays),
                     planes=lambda: ctx.local_eq_boundary_grad(th[0], h, geo, dP, d_alpha, d_sigma, d_rays, want_geo_bar=True)))
n = n_lines * len(rays)
b = r["grad"][3]
n_cross = int(b["n_cross"].clamp(min=0).sum())
lt = b["dlam_dt"][torch.isfinite(b["dlam_dt"])]
row("%d lines x %d rays: local_eq_boundary" % (n_lines, len(rays)), n, r["boundary"])
row("local_eq_boundary_grad (boundary + gather + local_eq_grad)", n, r["grad"],
    "/ boundary %.2f  crossings %d  flagged points %d  |lam_t| in [%.3g, %.3g]  max |lam_at - shift| %.2e"
    % (r["grad"][0] / r["boundary"][0], n_cross, b["grad_nbad"], float(lt.abs().min()), float(lt.abs().max()),
       float(b["lam_at"][torch.isfinite(b["lam_at"])].abs().max())))
row("the same with the planes of t*", n, r["planes"], "/ boundary %.2f" % (r["planes"][0] / r["boundary"][0]))
