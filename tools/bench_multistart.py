"""What the multi-start refinement costs and what it finds: AdjointStep on the configs[3] shape (73 emulated equilibria x 5 surfaces x
24 alpha x 15 theta0, N = 969: bench.py's c4_adjoint_step) with n_starts = 1, 2, 4.

    python tools/bench_multistart.py [--reps 15] [--out FILE.json]

One process, the three AdjointStep objects alternating inside every repetition (so that drift of the clocks and of the host hits all
three alike), after two warm-up runs of each.  Per K: the wall time of run() (it ends with the rows' one copy to the host) and, from
separate passes with HIP events between the phases, geometry / scan_argmax / refine / final_solve -- median and min .. max over the
repetitions.  Beside them: ibs_scan_peaks_f64 alone against ibs_surface_argmax_pack_f64 + ibs_scan_starts_f64 on the 365 coarse
tables of the step (device events around 200 back-to-back calls each, alternating), and how many of the 365 surfaces report another
maximum at K = 2 and 4 than at K = 1, and by how much.  Needs a GPU; prints one JSON document."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

KS = (1, 2, 4)
PHASES = ("geometry_ms", "scan_argmax_ms", "refine_ms", "final_solve_ms")


def spread(v):
    v = np.asarray(v, dtype=np.float64)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()))


def kernel_times(ctx, scan, dev, calls=200, reps=7):
    """device milliseconds per call of k_scan_peaks (K = 1, 2, 4, 16) and of k_surface_argmax + k_scan_starts on the coarse tables
    of `scan`'s surfaces"""
    import torch
    res = scan._resident_inputs()
    na, nt = len(scan.alpha_scan), len(scan.theta0_scan)
    geo = ctx.fieldline_geometry(scan.tables, res["surf"], res["al"], res["th"], device=dev)
    tab = ctx.gamma_scan_argmax(scan.h, [geo["geo"][k] for k in range(7)], geo["dPdrho"], res["t0"], len(scan.own))["gam"]
    tab3, tab2 = tab.view(-1, na, nt), tab.view(-1, na * nt)
    nb = torch.zeros(1, dtype=torch.int32, device=dev)

    def pair():
        ctx.scan_starts(res["alpha"], res["t0"], ctx.surface_argmax_pack(tab2), nb)
    legs = {"argmax_pack+scan_starts": pair}
    for K in (1, 2, 4, 16):
        legs["scan_peaks_K%d" % K] = lambda K=K: ctx.scan_peaks(res["alpha"], res["t0"], tab3, K, n_bad=nb)
    out = {k: [] for k in legs}
    for r in range(reps + 1):
        for name, fn in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record(); torch.cuda.synchronize()
            if r:                                        # (repetition 0 warms up)
                out[name].append(e0.elapsed_time(e1) / calls)
    return {k: spread(v) for k, v in out.items()}, int(tab3.shape[0])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import bench
    import ibs_amd
    assert torch.cuda.is_available(), "bench_multistart.py needs a GPU"
    dev = torch.device("cuda:0")
    ctx = ibs_amd.Context(0)
    wout0 = dict(np.load(os.path.join(ROOT, "tests", "golden", "G8_wout_ncsx_op.npz")))
    wouts, steps, _ = bench.emulated_equilibria(wout0)
    wouts = [{k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in w.items()} for w in wouts]
    n_eq, ns, na, nt0 = len(wouts), 5, 24, 15
    svals = np.linspace(0.5, 0.95, ns)
    th = ibs_amd.theta_grid_for(11, 11)
    f_other = 0.8 + 0.01 * np.arange(n_eq)
    step = {K: ibs_amd.AdjointStep(ctx, th, svals, dev, nalpha=na, ntheta0=nt0, gamma_thresh=-2.0e-4, prefac=50.0, n_starts=K) for K in KS}
    out = {}
    for _ in range(2):                                   # warm-up of every shape the timed window uses
        for K in KS:
            out[K] = step[K].run(wouts, f_other, steps)
    total = {K: [] for K in KS}
    phases = {K: {p: [] for p in PHASES} for K in KS}
    for _ in range(max(1, args.reps)):
        for K in KS:
            t0 = time.perf_counter()
            step[K].run(wouts, f_other, steps)
            total[K].append((time.perf_counter() - t0) * 1e3)
        for K in KS:
            ph = {}
            step[K].run(wouts, f_other, steps, phases=ph)
            for p in PHASES:
                phases[K][p].append(ph[p])
    doc = dict(workload="configs[3]: %d emulated equilibria x %d surfaces x %d alpha x %d theta0, N = %d; AdjointStep.run(), n_starts = %s "
                        "alternating in one process, %d repetitions after 2 warm-up runs each" % (n_eq, ns, na, nt0, len(th), list(KS), args.reps),
               total_ms={str(K): spread(total[K]) for K in KS},
               phases_ms={str(K): {p: spread(v) for p, v in phases[K].items()} for K in KS},
               phases_how="separate passes with HIP events between the phases (one extra synchronisation each)")
    g1 = out[1]["gam"]
    doc["maxima"] = {}
    for K in KS[1:]:
        d = out[K]["gam"] - g1
        moved = np.abs(d) > 1e-8
        doc["maxima"][str(K)] = dict(surfaces=int(d.size), changed=int(moved.sum()), raised=int((d > 1e-8).sum()), lowered=int((d < -1e-8).sum()),
                                     max_gain=float(d.max()), min_gain=float(d.min()), fobj=out[K]["fobj"], fobj_K1=out[1]["fobj"])
        scan = step[K]._scan
        nf = scan.last_peaks["n_found"].cpu().numpy()
        doc["maxima"][str(K)]["n_found_histogram"] = {str(k): int((nf == k).sum()) for k in range(K + 1)}
    kt, n_tab = kernel_times(ctx, step[1]._scan, dev)
    doc["kernel_ms_per_call"] = kt
    doc["kernel_tables"] = n_tab
    txt = json.dumps(doc, indent=1, sort_keys=True)
    print(txt)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(txt + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
