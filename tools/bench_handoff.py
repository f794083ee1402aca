#!/usr/bin/env python3
"""What the surface-maximum hand-off at the end of the one-wave scan kernels costs, by table size (EXPERIMENTS R6.9): the fused launch
(ScanPlan.scan_argmax) against the same kernel without it (ScanPlan.scan) at the headline shape (16 x 8 x 8, N = 513, n_per = 64)
and at the reference batch's shape (5 x 24 x 15, N = 969, n_per = 360: the last arriver's wave makes two rounds of loads), and --
with `legs` -- the legs of bench.py --full that share the kernel or the step (bench.py's own functions).  One JSON line.
   python tools/bench_handoff.py [legs]          A/B of two libraries: IBS_LIB_PATH=<other .so>, a process per run, alternating"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import ibs_amd  # noqa: E402
import bench  # noqa: E402

dev = torch.device("cuda", 0)
ctx = ibs_amd.Context(0)


def window_us(fn, n, windows=7):
    """median over `windows` of n back-to-back calls between two synchronisations, us per call"""
    for _ in range(max(20, n // 10)):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(windows):
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / n * 1e6)
    return float(np.median(out)), float(min(out))


def golden_plan(ns, na, nt0, N):
    """the golden NCSX lines interpolated onto N points, every line scaled a little differently (tests/test_gpu_scan_handoff.py)"""
    g3 = np.load(os.path.join(ROOT, "tests", "golden", "G3_ncsx_lines.npz"))
    th513, th = ibs_amd.theta_grid(513), ibs_amd.theta_grid(N)
    rng = np.random.default_rng(ns * 1000 + N)
    geo = np.stack([[np.interp(th, th513, g3["geo_513"][l % 16, k]) for k in range(8)] for l in range(ns * na)])
    geo[:, 4:7] *= (1 + rng.uniform(-0.08, 0.08, len(geo)))[:, None, None]
    geo[:, 2:4] *= (1 + rng.uniform(-0.08, 0.08, len(geo)))[:, None, None]
    dP = -0.5 * np.mean((geo[:, 2] - geo[:, 7]) * geo[:, 0] ** 2, axis=1)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return ibs_amd.ScanPlan(ctx, float(th[1] - th[0]), [t(geo[:, k]) for k in range(7)], t(dP), t(np.linspace(0, np.pi / 2, nt0)), ns)


out = {}
h, geo7, dP_d, th0_d, *_ = bench.build_workload(0, dev)
for tag, plan, n in (("headline_n_per_64", ibs_amd.ScanPlan(ctx, h, geo7, dP_d, th0_d, bench.N_SURF), 1000),
                     ("reference_shape_n_per_360", golden_plan(5, 24, 15, 969), 300)):
    fused = window_us(plan.scan_argmax, n)
    name = ctx.last_launch()[0]
    plain = window_us(plan.scan, n)
    two = window_us(lambda: (plan.scan(), plan.argmax()), n)
    out[tag] = dict(kernel=name, fused_us=round(fused[0], 3), fused_min_us=round(fused[1], 3), plain_us=round(plain[0], 3),
                    plain_min_us=round(plain[1], 3), two_launches_us=round(two[0], 3))
if "legs" in sys.argv[1:]:
    b = bench.batch_scaling(ctx, dev, h, geo7, dP_d, th0_d)
    out["batch_scaling_us"] = {str(r["solves_per_launch"]): round(r["us_per_launch"], 3) for r in b["one_launch"]}
    out["two_streams_us"] = round(b["two_streams"]["us_per_launch"], 3)
    p = bench.ncsx_pipeline(ctx, dev)
    out["reference_batch_scan_ms"] = p["reference_batch"]["scan_ms"]
    out["ncsx_c3_scan_ms"] = p["ncsx_c3"]["scan_ms"]
    c = bench.c4_adjoint_step(ctx, dev, n_oracle=0)
    out["c4_total_ms"] = c.get("total_ms")
print("HANDOFF " + json.dumps(out), flush=True)
