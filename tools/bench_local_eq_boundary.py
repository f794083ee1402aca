#!/usr/bin/env python3
"""The local-equilibrium boundaries (csrc/ibs_local_eq_boundary.hip: k_local_eq_boundary) beside the parent commit's way to the same
node-resolution diagram, in the same run, alternating: the lines of tools/bench_local_eq.py (2 surfaces x 12 alpha of the G8 tables = 24
lines) at N = 969, p-rays over p in [--p-lo, --p-hi].
  one ray per (line, theta0)    24 x 3 = 72 systems at eps = 0
  --n-eps rays per (line, theta0)   24 x 3 x 32 = 2,304 systems, eps in [-0.75, 1]
each against local_eq_scan(count_only=True) on the same 64 nodes per ray (64 systems per ray: the diagram row without any closed
crossing); the node counts of the two are compared.  Printed beside the times: mean crossings and mean passes per ray, the expectation
(1 + 6 mean n_cross) node diagrams' worth of serial work per ray, and the status bits seen.  Host clock around calls that end in a
device synchronise; median of `--reps` alternating repetitions after one warm-up of each.  No gate on speed: an analysis mode.
    python tools/bench_local_eq_boundary.py [--reps 7] [--out profiles/local_eq_boundary_bench.txt]"""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import numpy as np, torch, ibs_amd

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--n-eps", type=int, default=32)
ap.add_argument("--p-lo", type=float, default=0.0)
ap.add_argument("--p-hi", type=float, default=3.0)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "local_eq_boundary_bench.txt"))
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
    say("%-58s %9.3f ms (min %8.3f max %8.3f) = %8.3f us per ray  %s" % (label, t[0] * 1e3, t[1] * 1e3, t[2] * 1e3, t[0] / n * 1e6, extra))


N, n_t0 = 969, 3
g8 = dict(np.load(os.path.join(ROOT, "tests", "golden", "G8_surface_tables.npz")))
tabs = ibs_amd.SurfaceTables.from_arrays(g8)
surf = np.repeat(np.array([1, 2], dtype=np.int32), 12)
alpha = np.tile(np.linspace(0.0, np.pi, 12), 2)
n_lines = len(surf)
th = ibs_amd.theta_grid(N)
h = float(th[1] - th[0])
theta0 = np.linspace(0.0, 0.5 * np.pi, n_t0)
sigma = np.sign(-tabs.scal[surf, 4])
base = ctx.fieldline_geometry(tabs, surf, alpha, th, device=dev)
d_alpha, d_sigma = torch.from_numpy(alpha).to(dev), torch.from_numpy(sigma).to(dev)
say("device: %s; %d lines of the G8 tables, N = %d, p-rays over [%g, %g]; median of %d alternating repetitions after one warm-up of each; "
    "host clock around synchronised calls" % (torch.cuda.get_device_name(0), n_lines, N, args.p_lo, args.p_hi, args.reps))

for eps in (np.zeros(1), np.linspace(-0.75, 1.0, args.n_eps)):
    tt, ee = (a.ravel() for a in np.meshgrid(theta0, eps, indexing="ij"))
    zero, one = np.zeros_like(tt), np.ones_like(tt)
    rays = np.stack([tt, ee, zero, zero, one, np.full_like(tt, args.p_lo), np.full_like(tt, args.p_hi)], axis=1)
    nodes = ibs_amd.local_eq_ray_triples(rays[:, None, :], ibs_amd.local_eq_ray_nodes(rays)).reshape(-1, 3)
    d_rays, d_nodes = torch.from_numpy(rays).to(dev), torch.from_numpy(nodes).to(dev)
    names = {}

    def boundary(want_nodes):
        out = ctx.local_eq_boundary(th[0], h, base["geo"], base["dPdrho"], d_alpha, d_sigma, d_rays, want_nodes=want_nodes, want_info=True)
        names["boundary"] = "%s on %d blocks" % ctx.last_launch()
        return out

    def raster():
        # (the rays of a call are shared by its lines, so their node triples are the variations of ONE scan call)
        return ctx.local_eq_scan(th[0], h, base["geo"], base["dPdrho"], d_alpha, d_sigma, d_nodes, count_only=True)

    r = alternating(dict(boundary=lambda: boundary(False), with_nodes=lambda: boundary(True), raster=raster))
    n = n_lines * len(rays)
    b = r["with_nodes"][3]
    info, nc = b["info"], b["n_cross"]
    st = info >> 16
    passes, mean_nc = float((info & 0xffff).double().mean()), float(nc.clamp(min=0).double().mean())
    same = bool(torch.equal(b["node_count"].reshape(n_lines, -1), r["raster"][3]["count"]))
    row("%d lines x %d rays: local_eq_boundary" % (n_lines, len(rays)), n, r["boundary"],
        "passes %.2f  crossings %.3f  1 + 6 crossings = %.2f  status bits seen 0x%x  %s"
        % (passes, mean_nc, 1 + 6 * mean_nc, int(np.bitwise_or.reduce(st.cpu().numpy().ravel())), names["boundary"]))
    row("the same with node_count", n, r["with_nodes"])
    row("local_eq_scan(count_only) on the 64 nodes of every ray", n, r["raster"],
        "boundary / raster %.2f  node counts equal: %s  unstable nodes %.1f %%"
        % (r["boundary"][0] / r["raster"][0], same, 100.0 * float((r["raster"][3]["count"] > 0).double().mean())))
