#!/usr/bin/env python3
"""Spectrum mode (csrc/ibs_modes.hip): 2,048 s-alpha systems at N = 969 and N = 2,561, K = 1, 4, 8 modes, growth rates and vectors
wanted / eigenvalues only.  Beside it the only route to the same numbers without the entry point: K launches of
ibs_solve_gcf_nearest_f64 with sigma set to each wanted eigenvalue, taken from a CPU reference (scipy's bisection on the symmetric
form).  After a warm-up of every shape the routes alternate --reps times in the same run, each time as a window of as many calls
as fill --window seconds (0.1 s: 4 to 115 calls); the figures are medians per call, the spread is printed.  Mean multisection passes
per system come from the info words; the vector stage's share is 1 - (eigenvalues only) / (with gam).  "lam only" goes to the library
through ctypes directly (Context.solve_gcf_modes always asks for gam), the other routes through Context methods: the share includes
the few microseconds by which the two marshalling paths differ.
    python tools/bench_modes.py [--reps R] [--window seconds] [--systems n]"""
import argparse, ctypes as C, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import numpy as np, torch, ibs_amd
from scipy.linalg import eigvalsh_tridiagonal

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--window", type=float, default=0.1, help="seconds a timed window lasts at least: the calls per window are sized to it")
ap.add_argument("--systems", type=int, default=2048)
ap.add_argument("--distinct", type=int, default=128, help="distinct systems (tiled up to --systems): the CPU reference runs on these")
a = ap.parse_args()
dev = torch.device("cuda", 0); ctx = ibs_amd.Context(0)
KMAX = 8


def timed(fn, inner=1):
    """seconds per call, from a window of `inner` calls that ends in a device synchronise"""
    torch.cuda.synchronize(); t = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / inner


def lam_only(h, g, c, f, K):
    """ibs_solve_gcf_modes_f64 with lam and info alone (Context.solve_gcf_modes always asks for gam)"""
    n, N = g.shape
    lam = torch.empty((n, K), dtype=torch.float64, device=dev); info = torch.empty((n, K), dtype=torch.int32, device=dev)
    ctx._stream_from_torch(dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    rc = ctx._lib.ibs_solve_gcf_modes_f64(ctx._h, n, N, h, p(g), None, p(c), p(f), N, K, p(lam), None, None, None, p(info), 0)
    assert rc == 0, rc
    return dict(lam=lam, info=info)


for N in (969, 2561):
    th = np.linspace(-4 * np.pi, 4 * np.pi, N); h = float(th[1] - th[0])
    rng = np.random.default_rng(N)
    nd = min(a.distinct, a.systems)
    sh, al, dP = rng.uniform(0.6, 1.4, (nd, 1)), rng.uniform(0.5, 1.0, (nd, 1)), rng.uniform(1.0, 8.0, (nd, 1))
    lm = sh * th[None] - al * np.sin(th)[None]
    G = 1 + lm ** 2; Cc = dP * al * (np.cos(th)[None] + np.sin(th)[None] * lm)
    e = 0.5 * (G[:, :-1] + G[:, 1:]) / h ** 2                           # the pencil of utils.py:1574-1592 with f = g
    d = Cc[:, 1:-1] - (e[:, :-1] + e[:, 1:]); fd = G[:, 1:-1]
    top = np.stack([eigvalsh_tridiagonal(d[i] / fd[i], e[i, 1:-1] / np.sqrt(fd[i, :-1] * fd[i, 1:]), select="i",
                                         select_range=(N - 2 - KMAX, N - 3))[::-1] for i in range(nd)])
    rep = np.arange(a.systems) % nd
    g, c = (torch.from_numpy(x[rep]).to(dev) for x in (G, Cc)); f = g.clone()
    sig = torch.from_numpy(np.ascontiguousarray(top[rep])).to(dev)       # (systems, KMAX) descending
    for K in (1, 4, 8):
        cols = [sig[:, m].contiguous() for m in range(K)]
        routes = {
            "modes, gam + X": lambda: ctx.solve_gcf_modes(h, g, c, f, K, want_X=True, want_info=True),
            "modes, gam": lambda: ctx.solve_gcf_modes(h, g, c, f, K, want_info=True),
            "modes, lam only": lambda: lam_only(h, g, c, f, K),
            "K nearest launches, gam": lambda: [ctx.solve_gcf_nearest(h, g, c, f, s, want_info=True) for s in cols],
        }
        res = {k: fn() for k, fn in routes.items()}; torch.cuda.synchronize()          # warm-up of every shape
        r, rn = res["modes, gam"], res["K nearest launches, gam"]
        dl = max(float((rn[m]["lam"] - r["lam"][:, m]).abs().max()) for m in range(K))
        dg = max(float((rn[m]["gam"] - r["gam"][:, m]).abs().max()) for m in range(K))
        idx_ok = all(bool((rn[m]["idx"] == m).all()) for m in range(K))
        inner = {k: max(1, int(np.ceil(a.window / timed(fn, 3)))) for k, fn in routes.items()}       # calls per window of --window seconds
        times = {k: [] for k in routes}
        for _ in range(a.reps):
            for k, fn in routes.items():
                times[k].append(timed(fn, inner[k]))
        med = {k: float(np.median(v)) for k, v in times.items()}
        passes = float((r["info"][:, 0] & 0xffff).double().mean())
        passes_n = float(sum((x["info"] & 0xffff).double().mean() for x in rn))
        flagged = int((((r["info"] >> 16) & 3) != 0).sum()); clustered = int((((r["info"] >> 16) & ibs_amd.CLUSTER_BIT) != 0).sum())
        print("N %5d  %d systems  K %d   passes/system: modes %.2f, K nearest launches %.2f   max |dlam| %.2e |dgam| %.2e  idx ok %s  flagged %d clustered %d"
              % (N, a.systems, K, passes, passes_n, dl, dg, idx_ok, flagged, clustered))
        for k in routes:
            print("    %-26s %9.3f ms  (min %.3f max %.3f of %d windows of %d calls)" % (k, med[k] * 1e3, min(times[k]) * 1e3, max(times[k]) * 1e3, a.reps, inner[k]))
        print("    modes / K nearest launches (gam): %.3f    vector stage's share of 'modes, gam': %.1f %%   per mode %.3f ms"
              % (med["modes, gam"] / med["K nearest launches, gam"], 100 * (1 - med["modes, lam only"] / med["modes, gam"]),
                 (med["modes, gam"] - med["modes, lam only"]) * 1e3 / K), flush=True)
