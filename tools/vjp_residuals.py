#!/usr/bin/env python3
"""How far the library's own eigenpairs are from exact ones, in the units of the exact-gradient kernel's refusal bound: the residual
max_r |((S - lam F) X)_r| / f_r over N eps (||A|| + |lam|) max |X| (tests/vjp_oracle.residual_ratio; ibs_solve_gcf_vjp_f64 refuses a
pair above 1024, csrc/ibs_vjp.hip), per forward kernel form: synthetic field-line batches that select the register-resident, sub-wave,
direct, row-streamed and long-grid lam_max kernels, and the nearest-sigma kernel on strongly driven s-alpha lines.
    python tools/vjp_residuals.py [--out profiles/vjp_residuals.txt]"""
import argparse, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import numpy as np, torch, ibs_amd
from oracle import ballooning_oracle as bo
from tests import vjp_oracle as vo

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
args = ap.parse_args()
ctx = ibs_amd.Context(0); dev = torch.device("cuda:0")
lines = []


def report(label, kernel, q):
    lines.append("%-16s %-45s ratio max %9.3g  p99 %9.3g  median %9.3g   (bound 1024)" % (label, kernel, q.max(), np.quantile(q, 0.99),
                                                                                         np.median(q)))
    print(lines[-1], flush=True)


for n, N in ((6, 129), (6, 969), (6, 2049), (6, 4097), (1800, 969), (4095, 513), (1024, 513), (64, 4097), (30000, 257)):
    h, (g, c, f) = vo.synthetic_batch(n, N)
    r = ctx.solve_gcf(h, *(torch.from_numpy(a).to(dev) for a in (g, c, f)), want_X=True)
    report("%6d x %5d" % (n, N), ctx.last_launch()[0], vo.residual_ratio(h, g, c, f, r["lam"].cpu().numpy(), r["X"].cpu().numpy()))
for N in (129, 969, 4097):
    th = bo.theta_grid(N)
    g, c = bo.salpha_gc(th, 1.0, 0.8, 0.0)
    r = ctx.solve_gcf_nearest(th[1] - th[0], g[None], 4 * c[None], g[None], 0.42, want_X=True)
    report("nearest %5d" % N, "%s (idx %d)" % (ctx.last_launch()[0], int(r["idx"][0])),
           vo.residual_ratio(th[1] - th[0], g[None], 4 * c[None], g[None], r["lam"], r["X"]))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
