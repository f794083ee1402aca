#!/usr/bin/env python3
"""The scan workflow refined on the exact gradient of gam (jac="exact") against the reference's Hellmann-Feynman gradient
(jac="reference") of the same build, both in lam_max mode, on the configs[3] shape (bench.py's c4 leg: 73 emulated NCSX equilibria x 5
surfaces x 24 alpha x 15 theta0, N = 969, one AdjointStep.run()): median wall time of `--reps` runs after one warm-up, per-phase ms of
a separate pass with HIP events (`phases=`), refinement rounds and evaluations per surface, and max / min of gam_exact - gam_reference
over the 365 surfaces.  Then the batched objective ibs_obj_w_grad_exact_f64 against the host-composed make_obj_w_grad(jac="exact") on
the 365 refined points: one call against 365 calls.
    python tools/bench_exact_refine.py [--reps 3] [--json out.json]"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import numpy as np, torch, ibs_amd, bench

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--json", default=None)
args = ap.parse_args()
dev = torch.device("cuda", 0); ctx = ibs_amd.Context(0)

wout0 = dict(np.load(os.path.join(ROOT, "tests", "golden", "G8_wout_ncsx_op.npz")))
wouts, steps, _ = bench.emulated_equilibria(wout0)
wouts = [{k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in w.items()} for w in wouts]
n_eq, ns, na, nt0 = len(wouts), 5, 24, 15
svals = np.linspace(0.5, 0.95, ns)
th = ibs_amd.theta_grid_for(11, 11)
f_other = 0.8 + 0.01 * np.arange(n_eq)
out = dict(workload="configs[3]: %d equilibria x %d surfaces x %d alpha x %d theta0, N = %d, one AdjointStep.run(), lam_max mode" % (
    n_eq, ns, na, nt0, len(th)))
res = {}
for jac in ("reference", "exact"):
    step = ibs_amd.AdjointStep(ctx, th, svals, dev, nalpha=na, ntheta0=nt0, gamma_thresh=-2.0e-4, prefac=50.0, jac=jac)
    step.run(wouts, f_other, steps)                              # warm-up
    ts = []
    for _ in range(args.reps):
        t0 = time.perf_counter(); r = step.run(wouts, f_other, steps); ts.append((time.perf_counter() - t0) * 1e3)
    ph = {}
    step.run(wouts, f_other, steps, phases=ph)
    lr = step._scan.last_refine
    ne = lr["n_evals"]
    ne = np.asarray(ne.cpu() if hasattr(ne, "cpu") else ne)
    res[jac] = r
    out[jac] = dict(total_ms=float(np.median(ts)), total_ms_runs=ts, phases={k: float(v) for k, v in ph.items()},
                    refine_rounds=int(lr["rounds"]), evals_per_surface=dict(min=int(ne.min()), mean=float(ne.mean()), max=int(ne.max())),
                    fobj=r["fobj"], gam_min=float(r["gam"].min()), gam_max=float(r["gam"].max()))
    print("%-9s total %9.2f ms  phases= %s  refine_rounds= %d  evaluations per surface min/mean/max = %d / %.2f / %d" % (
        jac, out[jac]["total_ms"], " ".join("%s:%.2f" % kv for kv in sorted(out[jac]["phases"].items())), out[jac]["refine_rounds"],
        ne.min(), ne.mean(), ne.max()), flush=True)
dg = res["exact"]["gam"] - res["reference"]["gam"]
out["exact_over_reference"] = out["exact"]["total_ms"] / out["reference"]["total_ms"]
out["gam_exact_minus_reference"] = dict(max=float(dg.max()), min=float(dg.min()), n_surfaces=int(dg.size), n_larger=int((dg > 0).sum()))
print("exact / reference = %.2f   gam_exact - gam_reference over %d surfaces: max %.3e  min %.3e  (%d larger)" % (
    out["exact_over_reference"], dg.size, dg.max(), dg.min(), int((dg > 0).sum())))

# the objective on the 365 refined points of the exact run: one batched call against one host-composed call per point
tabs = ibs_amd.SurfaceTables.from_wouts(wouts, svals)                 # surface index = i_equilibrium * ns + i_surface
r = res["exact"]
pts_a, pts_t = r["alpha"].reshape(-1), r["theta0"].reshape(-1)
n = len(pts_a)
d = 0.004
al = np.stack([pts_a - 0.5 * d, pts_a, pts_a + 0.5 * d], axis=1).reshape(-1)
surf = np.repeat(np.arange(n), 3).astype(np.int32)
geo = ctx.fieldline_geometry(tabs, surf, al, th)["geo"]                 # (8, 3 n, N) host
geo = np.ascontiguousarray(np.transpose(geo.reshape(8, n, 3, len(th)), (1, 2, 0, 3)))
h = th[1] - th[0]
gd, td = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (geo, pts_t))


def batched():
    return ctx.obj_w_grad_exact(h, gd, td, d)


def per_point():
    vals = []
    for k in range(n):
        f = ibs_amd.make_obj_w_grad(lambda vs, rho, alphas, theta, k=k: geo[k], ctx=ctx, jac="exact", del_alpha=d)
        vals.append(f(np.array([pts_a[k], pts_t[k]]), None, 0.5, th, None))
    return vals


batched(); torch.cuda.synchronize()
kernel = ctx.last_launch()[0]
per_point(); torch.cuda.synchronize()
tb, tp = [], []
for _ in range(args.reps):
    t0 = time.perf_counter(); vb, jb = batched(); torch.cuda.synchronize(); tb.append((time.perf_counter() - t0) * 1e3)
    t0 = time.perf_counter(); vp = per_point(); tp.append((time.perf_counter() - t0) * 1e3)
vb, jb = vb.cpu().numpy(), jb.cpu().numpy()
dv = max(abs(vb[k] - vp[k][0]) for k in range(n)); dj = max(np.abs(jb[k] - vp[k][1]).max() for k in range(n))
out["objective_365"] = dict(points=n, kernel=kernel,
                            batched_ms=float(np.median(tb)), host_composed_ms=float(np.median(tp)),
                            speedup=float(np.median(tp) / np.median(tb)), max_abs_dval=float(dv), max_abs_djac=float(dj),
                            max_abs_jac_at_refined_points=float(np.abs(jb).max()))
print("obj_w_grad_exact, %d points: batched %.2f ms, host-composed %.2f ms (x %.1f); max |dval| %.3g, max |djac| %.3g; "
      "max |jac| at the refined points %.3g" % (n, np.median(tb), np.median(tp), np.median(tp) / np.median(tb), dv, dj, np.abs(jb).max()))
if args.json:
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as fh:
        json.dump(out, fh, indent=1)
