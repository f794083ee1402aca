"""What maximising mu = 1 / s* over theta0 on every line costs and what it finds: ibs_marginal_theta0_polish_f64 beside
ibs_marginal_scan_f64 on the same lines, on the NCSX tables of tests/golden/G8_*, N = 969, 24 alpha x 15 theta0, for 5 and for 365
surfaces, n_starts = 1 and 2.

    python tools/bench_marginal_polish.py [--reps 10] [--out FILE.json]

One process.  Per shape the geometry is made once on the device; then, after a warm-up call of each, `reps` alternating calls of the
scan and of the polish (K = 1, K = 2) between device events: median and min .. max of the milliseconds per call.  Beside them: the
mean and maximum n_eval over the slots, the multisection passes per evaluation, the share of rows whose first peak is an edge node,
the share of slots that returned the node itself, and the per-surface drop of the envelope's s* below the coarse minimum.  Needs a
GPU; prints one JSON document."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

KS = (1, 2)
NA, NT0 = 24, 15


def spread(v):
    v = np.asarray(v, dtype=np.float64)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()))


def one_shape(ctx, wout, n_surf, dev, reps):
    import torch
    import ibs_amd
    svals = np.linspace(0.5, 0.95, n_surf)
    th = ibs_amd.theta_grid_for(11, 11)
    tabs = ibs_amd.SurfaceTables.from_wout(wout, svals)
    scan = ibs_amd.BallooningScan(ctx, None, th, svals, nalpha=NA, ntheta0=NT0, tables=tabs, device=dev)
    res = scan._resident_inputs()
    geo = ctx.fieldline_geometry(tabs, res["surf"], res["al"], res["th"], device=dev)
    g7, dP, t0 = [geo["geo"][k] for k in range(7)], geo["dPdrho"], res["t0"]
    sc = ctx.marginal_scan(scan.h, *g7, dP, t0, want_info=True)
    legs = {"marginal_scan": lambda: ctx.marginal_scan(scan.h, *g7, dP, t0, want_info=True)}
    for K in KS:
        legs["marginal_theta0_polish_K%d" % K] = lambda K=K: ctx.marginal_theta0_polish(scan.h, *g7, dP, t0, sc["mu"], n_starts=K, want_info=True)
    launches = {}
    for name, fn in legs.items():                        # warm-up, and which kernel each leg launches
        fn()
        launches[name] = ctx.last_launch()
    ms = {k: [] for k in legs}
    for _ in range(max(1, reps)):
        for name, fn in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record(); torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1))
    sci = sc["info"].cpu().numpy()
    doc = dict(n_surf=n_surf, n_lines=n_surf * NA, N=len(th), ms_per_call={k: spread(v) for k, v in ms.items()},
               launches={k: str(v) for k, v in launches.items()}, scan_passes_per_system=float((sci & 0xffff).mean()),
               scan_flagged=int((((sci >> 16) & 3) != 0).sum()))
    coarse_min = sc["scale"].view(n_surf, -1).min(dim=1).values.cpu().numpy()
    for K in KS:
        r = {k: v.cpu().numpy() for k, v in legs["marginal_theta0_polish_K%d" % K]().items() if hasattr(v, "cpu")}
        status = r["info"] >> 16
        live = r["node"] >= 0
        drop = coarse_min - np.nanmin(r["scale"].reshape(n_surf, -1), axis=1)
        doc["K%d" % K] = dict(n_eval_mean=float(r["n_eval"][live].mean()), n_eval_max=int(r["n_eval"].max()),
                              passes_per_eval=float((r["info"][live] & 0xffff).sum() / max(1, r["n_eval"][live].sum())),
                              edge_rows=float(np.isin(r["node"][:, 0], (0, NT0 - 1)).mean()),
                              node_returned=float(((status & (1 << 10)) != 0)[live].mean()),
                              flagged=int(((status & 3) != 0).sum()), n_found_mean=float(r["n_found"].mean()),
                              surface_drop=dict(max=float(drop.max()), mean=float(drop.mean()), min=float(drop.min()),
                                                lowered=int((drop > 0).sum())))
    return doc


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--surfaces", type=int, nargs="*", default=[5, 365])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import ibs_amd
    assert torch.cuda.is_available(), "bench_marginal_polish.py needs a GPU"
    dev = torch.device("cuda:0")
    ctx = ibs_amd.Context(0)
    wout = dict(np.load(os.path.join(ROOT, "tests", "golden", "G8_wout_ncsx_op.npz")))
    doc = dict(workload="NCSX tables of tests/golden/G8_*, %d alpha x %d theta0; per call device events, %d alternating repetitions after a warm-up"
                        % (NA, NT0, args.reps), shapes=[one_shape(ctx, wout, n, dev, args.reps) for n in args.surfaces])
    txt = json.dumps(doc, indent=1, sort_keys=True)
    print(txt)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(txt + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
