#!/usr/bin/env python3
"""The local-equilibrium boundaries minimised over theta0 (csrc/ibs_local_eq_boundary_polish.hip: k_local_eq_boundary_polish) beside the
cost model of its rule, in the same run, alternating: the lines of tools/bench_local_eq_boundary.py (2 surfaces x 12 alpha of the G8
tables = 24 lines) at N = 969, p-ray families over p in [--p-lo, --p-hi], one slot per (line, family), the coarse theta0 nodes
linspace(0, pi / 2, --n-theta0).
  3 families per line    24 x 3 = 72 slots, eps in [-0.5, 0.5]
  96 families per line   24 x 96 = 2,304 slots, eps in [-0.75, 1]
Every evaluation of the search is one cold boundary closure by one wave, so the model is
  time(polish) = (mean closures per slot) x time(local_eq_boundary(max_cross=1) on the same number of (line, ray) systems)
with closures = n_eval + 1 where the node itself is returned after a search (the evaluation at the node that supplies the ends).  Printed:
the two times, mean n_eval, mean closures, the ratio time(polish) / (closures x time(boundary)) and the status bits seen.  The coarse
rows come from one boundary call outside the timed region.  Host clock around calls that end in a device synchronise; median of `--reps`
alternating repetitions after one warm-up of each.  No gate on speed: an analysis mode.
    python tools/bench_local_eq_boundary_polish.py [--reps 7] [--out profiles/local_eq_boundary_polish_bench.txt]"""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import numpy as np, torch, ibs_amd

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--n-theta0", type=int, default=5)
ap.add_argument("--p-lo", type=float, default=0.0)
ap.add_argument("--p-hi", type=float, default=3.0)
ap.add_argument("--xtol-theta0", type=float, default=1e-5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "local_eq_boundary_polish_bench.txt"))
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


N = 969
g8 = dict(np.load(os.path.join(ROOT, "tests", "golden", "G8_surface_tables.npz")))
tabs = ibs_amd.SurfaceTables.from_arrays(g8)
surf = np.repeat(np.array([1, 2], dtype=np.int32), 12)
alpha = np.tile(np.linspace(0.0, np.pi, 12), 2)
n_lines = len(surf)
th = ibs_amd.theta_grid(N)
h = float(th[1] - th[0])
theta0 = np.linspace(0.0, 0.5 * np.pi, args.n_theta0)
sigma = np.sign(-tabs.scal[surf, 4])
base = ctx.fieldline_geometry(tabs, surf, alpha, th, device=dev)
d_alpha, d_sigma = torch.from_numpy(alpha).to(dev), torch.from_numpy(sigma).to(dev)
say("device: %s; %d lines of the G8 tables, N = %d, p-ray families over [%g, %g], %d theta0 nodes, xtol_theta0 = %g, max_eval = 32; median "
    "of %d alternating repetitions after one warm-up of each; host clock around synchronised calls"
    % (torch.cuda.get_device_name(0), n_lines, N, args.p_lo, args.p_hi, len(theta0), args.xtol_theta0, args.reps))

for eps in (np.linspace(-0.5, 0.5, 3), np.linspace(-0.75, 1.0, 96)):
    nf = len(eps)
    zero, one = np.zeros(nf), np.ones(nf)
    fam = np.stack([zero, eps, zero, zero, one, np.full(nf, args.p_lo), np.full(nf, args.p_hi)], axis=1)
    rays = np.concatenate([np.concatenate([np.full((nf, 1), t), fam[:, 1:]], axis=1) for t in theta0])       # node-major
    co = ctx.local_eq_boundary(th[0], h, base["geo"], base["dPdrho"], d_alpha, d_sigma, torch.from_numpy(rays).to(dev), max_cross=1,
                               want_info=True)
    T = ibs_amd.local_eq_first_up(co["t_stable"].cpu().numpy(), co["t_unstable"].cpu().numpy(), co["lo_unstable"].cpu().numpy(), args.p_lo)
    t_row = torch.from_numpy(np.ascontiguousarray(np.transpose(T.reshape(n_lines, len(theta0), nf), (0, 2, 1)))).to(dev)
    d_fam, d_t0 = torch.from_numpy(fam).to(dev), torch.from_numpy(theta0).to(dev)
    d_mid = torch.from_numpy(rays[nf * (len(theta0) // 2):nf * (len(theta0) // 2 + 1)].copy()).to(dev)       # the families at the middle node
    names = {}

    def polish():
        out = ctx.local_eq_boundary_polish(th[0], h, base["geo"], base["dPdrho"], d_alpha, d_sigma, d_fam, d_t0, t_row, n_starts=1,
                                           xtol_theta0=args.xtol_theta0, max_eval=32, want_info=True)
        names["polish"] = "%s on %d blocks" % ctx.last_launch()
        return out

    def boundary():
        return ctx.local_eq_boundary(th[0], h, base["geo"], base["dPdrho"], d_alpha, d_sigma, d_mid, max_cross=1, want_info=True)

    r = alternating(dict(polish=polish, boundary=boundary))
    p, b = r["polish"][3], r["boundary"][3]
    n = n_lines * nf
    st = (p["info"] >> 16).cpu().numpy()
    n_eval = p["n_eval"].cpu().numpy()
    closures = n_eval + (((st & 1024) != 0) & (n_eval > 0))
    passes_p, passes_b = float((p["info"] & 0xffff).double().mean()), float((b["info"] & 0xffff).double().mean())
    gain = np.take_along_axis(t_row.cpu().numpy(), p["node"].cpu().numpy().astype(np.int64), axis=2) - p["t"].cpu().numpy()
    say("%d lines x %d families = %d slots: polish %9.3f ms (min %8.3f max %8.3f)  boundary(max_cross=1) on %d rays %8.3f ms (min %8.3f "
        "max %8.3f)" % (n_lines, nf, n, r["polish"][0] * 1e3, r["polish"][1] * 1e3, r["polish"][2] * 1e3, n, r["boundary"][0] * 1e3,
                        r["boundary"][1] * 1e3, r["boundary"][2] * 1e3))
    say("    mean n_eval %.2f (max %d), mean closures %.2f, passes per slot %.1f against %.2f per boundary ray; polish / (closures x "
        "boundary) = %.2f; polish / (n_eval x boundary) = %.2f; status bits seen 0x%x; slots that beat their node %d, largest gain %.3e; %s"
        % (n_eval.mean(), n_eval.max(), closures.mean(), passes_p, passes_b, r["polish"][0] / (closures.mean() * r["boundary"][0]),
           r["polish"][0] / (max(n_eval.mean(), 1e-300) * r["boundary"][0]), int(np.bitwise_or.reduce(st.ravel())),
           int((gain > 0).sum()), float(np.nanmax(np.where(np.isfinite(gain), gain, np.nan))) if np.isfinite(gain).any() else 0.0,
           names["polish"]))
