#!/usr/bin/env python3
"""Every output bit of the raw-solve family and of spectrum mode, this build against another build of the library (the parent
commit's), each loaded through IBS_LIB_PATH in a fresh child process on the same seeded inputs.

    python tools/bitwise_vs_parent.py --parent /path/to/parent/libibs_hip.so [--new /path/to/libibs_hip.so] [--log cases.txt]

Raw solves: the lane-edge lengths EDGE_N_SHORT of tests/edge_cases.py and N = 1025 (tests/golden/G10_rough_pair_1025.npz tiled: every
system trips the re-close) x batches of 1, 5 and 4099 (the last block has idle waves; the library picks the big-batch forms itself)
x outputs {lam; lam, gam; lam, gam, X, dX} x gcf_direct {default, 0, 1} x reclose {default, 0, 2} x {FP64 rows; FP64 rows with a
half-grid g; FP32 rows}.  Rows of the config-5 rough family (bench.c5_family), row pitch N + 5 with a sentinel in the padding, device
pointers; in the batches of 5 and 4099 system 1 has a g <= 0 and system 3 a NaN in c.  Spectrum mode: ibs_solve_gcf_modes_f64 and
ibs_solve_gcf_modes_basis_f64, K in {1, 4, 8}, the well systems of tests/modes_basis_oracle.py with the double well of
tests/modes_oracle.py, and a cluster-free batch of s-alpha lines, with and without X / dX.
Outputs start from a fixed byte pattern, so an element a kernel leaves alone compares as well.  A child records every array's length
and SHA-256 over its bytes (NaNs compare by bit pattern) with the kernel ibs_last_launch names and the systems carrying status bit 1,
bit 2 (FP32 result replaced by the FP64 solve) and bit 3 (re-closed); the parent process compares the two records.

The driver family: this tree's scan.py against another version of that file (the parent commit's), on ONE build of the library.

    python tools/bitwise_vs_parent.py --parent-scan /path/to/parent/scan.py [--log cases.txt] [--cpu | --time]

A child loads the given file as the package's scan submodule and runs BallooningScan in every mode (device_rows in each eigenpair /
jac / certify / theta0_polish mode x n_starts x refine, chunked with fill and phases, the host-driven refinement by length, local_rows,
run, the coarse-grid queries, the local-equilibrium scans, the margin and its refinements, the sensitivities, a scan without an owned
surface, the fieldlines-callback path) and AdjointStep.run on the NCSX tables of tests/test_gpu_scan_peaks.py, on one Context behind a
proxy that notes every Context call (name, scalars, shape / dtype / host-or-device of arrays).  Per case the record holds that
transcript and the SHA-256 of everything returned or left on the object; the two records must be equal.  --cpu rehearses loader, proxy
and compare on tests.helpers.OracleContext.  --time instead runs children on the two files in turn and compares the wall time of
AdjointStep.run() (configs[3] shape) and local_rows() (the shape of bench.py's sharded surface pass); with --log it APPENDS its lines,
marked `time | `, so the same file can hold the case list of the run before it.  A case that raises a ValueError (a refusal on the
host) is on record as raising; any other exception ends the child and the run."""
import argparse
import ctypes as C
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PAD, SENTINEL, FILL = 5, 7.5e300, 0x5A
OUTSETS = (("lam",), ("lam", "gam"), ("lam", "gam", "X", "dX"))


def child(record_path):
    import numpy as np
    import torch
    import bench
    import ibs_amd
    from ibs_amd import _lib
    from tests import edge_cases as ec, modes_basis_oracle as mb, modes_oracle as mo

    dev = torch.device("cuda:0")
    ctx = ibs_amd.Context(0)
    record = []

    def padded(a, dtype):
        """rows of a at pitch N + PAD, the padding holding a value no kernel may read"""
        t = torch.full((a.shape[0], a.shape[1] + PAD), SENTINEL if dtype == torch.float64 else 3.0e38, dtype=dtype, device=dev)
        t[:, :a.shape[1]] = a.to(dtype)
        return t

    def run(case, name, lead, rows, tail, outs):
        """ibs_<name>(ctx, *lead, rows..., ld, *tail, outs..., MEM_DEVICE); outs: (label, shape, dtype) or None for a null pointer"""
        bufs = [None if o is None else torch.full((int(np.prod(o[1])) * o[2].itemsize,), FILL, dtype=torch.uint8, device=dev) for o in outs]
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        ctx._stream_from_torch(dev)
        rc = getattr(ctx._lib, name)(ctx._h, *lead, *[ptr(r) for r in rows], rows[0].shape[1], *tail, *[ptr(b) for b in bufs], _lib.MEM_DEVICE)
        torch.cuda.synchronize()
        entry = dict(case=case, rc=int(rc), kernel=ctx.last_launch()[0], arrays={})
        for o, b in zip(outs, bufs):
            if o is None:
                continue
            a = b.cpu().numpy().view(np.uint64 if o[2].itemsize == 8 else np.uint32)
            entry["arrays"][o[0]] = [int(a.size), hashlib.sha256(a.tobytes()).hexdigest()]
            if a.size <= 8192 and o[0] in ("lam", "gam"):
                entry.setdefault("raw", {})[o[0]] = a.tobytes().hex()      # (small enough to say by how much a difference is)
            if o[0] == "info":
                st = a.astype(np.int64) >> 16
                entry["bits"] = [int(((st >> k) & 1).sum()) for k in (1, 2, 3)]
        record.append(entry)

    g10 = np.load(os.path.join(ROOT, "tests", "golden", "G10_rough_pair_1025.npz"))
    for N in sorted(set(ec.EDGE_N_SHORT) | {1025}):
        for n in (1, 5, 4099):
            if N == 1025:
                h = 8 * np.pi / (N - 1)
                g, c, f = (torch.from_numpy(np.tile(g10[k], (n, 1))).to(dev) for k in ("g", "c", "f"))
            else:
                h, g, c, f = bench.c5_family(dev, "rough", n, N, 1000 * N + n)
            if n > 1:
                g[1, N // 2] = -1.0
                c[3, N // 3] = float("nan")
            gh = 0.5 * (g[:, :-1] + g[:, 1:]) * (1.0 + 1e-3 * torch.cos(torch.arange(N - 1, device=dev, dtype=torch.float64)))[None]
            gh = torch.cat([gh, gh[:, -1:]], dim=1)
            r64 = [padded(a, torch.float64) for a in (g, c, f, gh)]
            r32 = [padded(a, torch.float32) for a in (g, c, f)]
            for direct in (None, 0, 1):
                for reclose in (None, 0, 2):
                    ctx.set_option("gcf_direct", direct)
                    ctx.set_option("reclose", reclose)
                    for outset in OUTSETS:
                        for kind, name, rows, dt in (("f64", "ibs_solve_gcf_f64", r64[:3], np.dtype(np.float64)),
                                                     ("gh", "ibs_solve_gcfh_f64", [r64[0], r64[3], r64[1], r64[2]], np.dtype(np.float64)),
                                                     ("f32", "ibs_solve_gcf_f32", r32, np.dtype(np.float32))):
                            shapes = dict(lam=(n,), gam=(n,), X=(n, N), dX=(n, N))
                            outs = [(k, shapes[k], dt) if k in outset else None for k in ("lam", "gam", "X", "dX")]
                            run("%s N=%d n=%d direct=%s reclose=%s %s" % (kind, N, n, direct, reclose, "+".join(outset)), name,
                                (n, N, h), rows, (), outs + [("info", (n,), np.dtype(np.int32))])
            ctx.set_option("gcf_direct", None)
            ctx.set_option("reclose", None)

    N = 513
    batches = dict(wells=[mo.double_well(N), mb.triple_well(N), mb.quad_well(N), mb.asym_triple_well(N), mo.double_well(N)],
                   salpha=[mo.salpha_line(N, dP) for dP in (-1.0, -2.0, -4.0, -6.0, -8.0)])
    f8, i4 = np.dtype(np.float64), np.dtype(np.int32)
    for tag, lines in batches.items():
        h = float(lines[0][0][1] - lines[0][0][0])
        n = len(lines)
        g, c, f = (padded(torch.from_numpy(np.stack([ln[i] for ln in lines])).to(dev), torch.float64) for i in (1, 2, 3))
        for K in (1, 4, 8):
            for vec in ((), ("X",), ("X", "dX")):
                outs = [("lam", (n, K), f8), ("gam", (n, K), f8)] + [(k, (n, K, N), f8) if k in vec else None for k in ("X", "dX")]
                for basis in (False, True):
                    if basis and "X" not in vec:
                        continue                                     # (the basis entry builds the members' vectors in the caller's X)
                    name = "ibs_solve_gcf_modes_basis_f64" if basis else "ibs_solve_gcf_modes_f64"
                    extra = [("cluster_first", (n, K), i4)] if basis else []
                    # (the spectrum-mode prototypes carry a half-grid g, null here, between g and c, and n_modes behind ld)
                    run("%s %s K=%d %s" % (name, tag, K, "+".join(vec) or "no vectors"), name, (n, N, h), [g, None, c, f], (K,),
                        outs + extra + [("info", (n, K), i4)])
    with open(record_path, "w") as fh:
        json.dump(record, fh)


# ---- the driver family: this tree's scan.py against another version of that file (the parent commit's), on the same library
N_DRV, SVALS3, GRID = 513, (0.5, 0.7, 0.9), dict(nalpha=8, ntheta0=5)            # the shapes of tests/test_gpu_scan_peaks.py
STATE = ("last_candidates", "last_peaks", "last_envelope", "last_marginal_envelope", "last_refine", "last_certificate", "_cert_dev",
         "_last_rows", "_last_marginal_points", "_batched_evals", "_coarse_cert")


def load_scan(path):
    """make the file at `path` the package's `scan` submodule: the entry of sys.modules and the attribute on the package (what
    AdjointStep's in-function `from .scan import ...` reads), and the names the package re-exports from it"""
    import importlib.util
    import ibs_amd
    old = sys.modules["ibs_amd.scan"]
    spec = importlib.util.spec_from_file_location("ibs_amd.scan", path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules["ibs_amd.scan"] = mod
    spec.loader.exec_module(mod)
    ibs_amd.scan = mod
    for name, v in vars(ibs_amd).items():
        if getattr(v, "__module__", None) == "ibs_amd.scan" and getattr(old, name, None) is v:
            setattr(ibs_amd, name, getattr(mod, name))


def describe(x):
    """an argument of a Context call as it goes on record: scalars by value, arrays by shape, dtype and host or device"""
    import numpy as np
    if x is None or isinstance(x, (bool, int, str)):
        return x
    if isinstance(x, (float, np.floating)):
        return float(x).hex()
    if isinstance(x, np.integer):
        return int(x)
    if isinstance(x, np.ndarray):
        return ["host", list(x.shape), str(x.dtype)]
    if hasattr(x, "is_cuda"):
        return ["device" if x.is_cuda else "host tensor", list(x.shape), str(x.dtype)]
    if isinstance(x, (list, tuple)):
        return [describe(v) for v in x]
    if isinstance(x, dict):
        return {str(k): describe(x[k]) for k in sorted(x, key=str)}
    return type(x).__name__


class Recorder:
    """a Context behind a proxy that notes every public method call made through it: name, scalars, and the kind of every array"""

    def __init__(self, ctx, calls):
        self.__dict__["_ctx"], self.__dict__["_calls"] = ctx, calls

    def __getattr__(self, name):
        v = getattr(self._ctx, name)
        if name.startswith("_") or not callable(v):
            return v

        def call(*a, **kw):
            self._calls.append([name, [describe(x) for x in a], {k: describe(kw[k]) for k in sorted(kw)}])
            return v(*a, **kw)
        return call

    def __setattr__(self, name, value):
        setattr(self._ctx, name, value)


def digests(x, name, out):
    """[elements, SHA-256] of every array reachable from x (dicts, sequences, tensors, scalars), under dotted names"""
    import numpy as np
    if isinstance(x, dict):
        for k in x:
            digests(x[k], "%s.%s" % (name, k), out)
    elif isinstance(x, (list, tuple)) and not all(isinstance(v, (int, float)) for v in x):
        for i, v in enumerate(x):
            digests(v, "%s.%d" % (name, i), out)
    elif x is None:
        out[name] = [0, "None"]
    else:
        a = np.ascontiguousarray(x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x))
        out[name] = [int(a.size), hashlib.sha256(str((a.dtype, a.shape)).encode() + a.tobytes()).hexdigest()]


def driver_child(record_path, scan_path, cpu, timed):
    import numpy as np
    import ibs_amd
    from tests.helpers import OracleContext, synthetic_fieldlines
    if scan_path:
        load_scan(scan_path)
    calls, record = [], []

    def case(name, fn):
        """fn() -> what the case returns and leaves behind.  A ValueError -- the driver's refusal of an argument or a shape on the
        host, before or between launches -- goes on record as the case's outcome (rc 1).  Anything else, an IbsError or a
        RuntimeError that may report a failed launch among them, ends this child, and with it the run: no further case starts."""
        del calls[:]
        entry = dict(case=name, rc=0, kernel="driver", arrays={})
        try:
            digests(fn(), "out", entry["arrays"])
        except ValueError as e:
            entry["rc"], entry["arrays"] = 1, {"error": [0, "%s: %s" % (type(e).__name__, e)]}
        entry["calls"] = json.loads(json.dumps(calls))
        entry["arrays"]["calls"] = [len(calls), hashlib.sha256(json.dumps(calls).encode()).hexdigest()]
        record.append(entry)

    def left(scan, **out):
        return dict(out, **{k: getattr(scan, k, None) for k in STATE})

    def callback_scan(ctx, N, **kw):
        th = np.linspace(-4 * np.pi, 4 * np.pi, N)
        return ibs_amd.BallooningScan(ctx, synthetic_fieldlines(th), th, [0.5, 0.8], nalpha=6, ntheta0=5, **kw)

    if cpu:                                 # the rehearsal: the callback cases the oracle-backed Context supports
        ctx = Recorder(OracleContext(), calls)
        for K in (1, 2):
            for refine in (True, False):
                scan = callback_scan(ctx, 65, n_starts=K)
                case("oracle callback run(refine=%s) n_starts=%d" % (refine, K), lambda: left(scan, run=scan.run(refine=refine)))
        with open(record_path, "w") as fh:
            json.dump(record, fh)
        return
    import torch
    import bench
    dev = torch.device("cuda:0")
    real = ibs_amd.Context(0)
    ctx = Recorder(real, calls)
    wout = dict(np.load(os.path.join(ROOT, "tests", "golden", "G8_wout_ncsx_op.npz")))
    if timed:
        return driver_times(record_path, real, dev, wout)

    def resident(svals=SVALS3, N=N_DRV, **kw):
        th = np.linspace(-4 * np.pi, 4 * np.pi, N)
        tabs = ibs_amd.SurfaceTables.from_wout(wout, np.asarray(svals))
        return ibs_amd.BallooningScan(ctx, None, th, np.asarray(svals), tables=tabs, device=dev, **GRID, **kw)

    def rows(scan, **kw):
        r, bad = scan.device_rows(**kw)
        return left(scan, rows=r, bad=bad)

    modes = dict(default={}, nearest=dict(eigenpair="nearest"), exact=dict(jac="exact"), exact_tangent=dict(jac="exact_tangent"),
                 certify=dict(certify=True), theta0_polish=dict(theta0_polish=True))
    for tag, kw in modes.items():
        for K in (1,) if tag == "theta0_polish" else (1, 3):
            for refine in (True, False):
                scan = resident(n_starts=K, **kw)
                case("device_rows %s n_starts=%d refine=%s" % (tag, K, refine), lambda: rows(scan, refine=refine))
            scan, log, ph = resident(n_starts=K, **kw), [], {}
            case("device_rows %s n_starts=%d chunks, fill, phases" % (tag, K),
                 lambda: dict(rows(scan, chunks=[(0, 1), (1, 3)], fill=lambda c0, c1: log.append((c0, c1)), phases=ph),
                              fill=np.array(log), phases=np.array([ord(c) for c in ",".join(sorted(ph))])))
    scan = resident(N=2561)
    case("device_rows default N=2561 (host-driven by length)", lambda: rows(scan))
    for cert in (False, True):
        scan = resident(certify=cert)
        case("local_rows certify=%s" % cert, lambda: left(scan, rows=scan.local_rows()))
        scan = resident(certify=cert)
        case("run certify=%s" % cert, lambda: left(scan, run=scan.run()))
    eps, p = np.array([-0.1, 0.1]), np.array([0.9, 1.1])
    queries = dict(coarse=lambda s: s.coarse(), mode_count=lambda s: s.mode_count(), modes=lambda s: s.modes(2),
                   envelope=lambda s: s.envelope(2), local_eq=lambda s: s.local_eq(eps, p),
                   local_eq_count_only=lambda s: s.local_eq(eps, p, count_only=True),
                   local_eq_boundary_p=lambda s: s.local_eq_boundary(eps, (0.0, 3.0)),
                   local_eq_boundary_eps=lambda s: s.local_eq_boundary(p, (-0.5, 0.5), axis="eps"),
                   marginal_envelope=lambda s: s.marginal_envelope(2))
    for refine in (False, True):
        for jac in ("reference", "exact_tangent"):
            for K in (1, 2):
                queries["marginal refine=%s jac=%s n_starts=%d" % (refine, jac, K)] = \
                    lambda s, kw=dict(refine=refine, jac=jac, n_starts=K): s.marginal(**kw)
    queries["marginal theta0_polish"] = lambda s: s.marginal(refine=True, theta0_polish=True)
    for tag, q in queries.items():
        scan = resident()
        case(tag, lambda: left(scan, out=q(scan)))
    scan = resident()
    case("sensitivity", lambda: left(scan, rows=scan.local_rows(), out=scan.sensitivity()))
    scan = resident()
    case("marginal_sensitivity", lambda: left(scan, m=scan.marginal(refine=True, jac="exact_tangent"), out=scan.marginal_sensitivity()))
    empty = dict(queries, device_rows=lambda s: s.device_rows(), local_rows=lambda s: s.local_rows())
    for tag, q in empty.items():
        scan = resident(svals=(0.7,), rank=1, world=2)
        case("no owned surface: " + tag, lambda: left(scan, out=q(scan)))
    for tag in ("coarse", "mode_count", "modes", "envelope"):
        scan = callback_scan(ctx, 131)
        case("callback " + tag, lambda: left(scan, out=queries[tag](scan)))
    for K in (1, 2):
        scan = callback_scan(ctx, 131, n_starts=K)
        case("callback local_rows n_starts=%d" % K, lambda: left(scan, rows=scan.local_rows()))
        scan = callback_scan(ctx, 131)
        case("callback marginal refine n_starts=%d" % K, lambda: left(scan, out=scan.marginal(refine=True, n_starts=K)))
    wouts = [wout] + bench.emulated_equilibria(wout)[0][1:3]             # the equilibria of test_adjoint_step_with_two_starts
    th = np.linspace(-4 * np.pi, 4 * np.pi, N_DRV)
    for K in (1, 2):
        step = ibs_amd.AdjointStep(ctx, th, np.array(SVALS3[1:]), dev, gamma_thresh=-2.0e-4, prefac=50.0, n_starts=K, **GRID)

        def adjoint_run():
            out = step.run(wouts, np.array([0.8, 0.81, 0.82]), np.array([1.0, 1e-3, 2e-3]))
            return left(step._scan, run=out, certificate=step.last_certificate)
        case("AdjointStep.run n_starts=%d" % K, adjoint_run)
    torch.cuda.synchronize()
    with open(record_path, "w") as fh:
        json.dump(record, fh)


def driver_times(record_path, ctx, dev, wout, reps=7):
    """wall milliseconds of the two workloads the host side shows in, each ending in the rows' copy to the host: AdjointStep.run() on
    the configs[3] shape (tools/c4_host_profile.py) and BallooningScan.local_rows() on the shape of bench.py's sharded surface pass"""
    import numpy as np
    import torch
    import bench
    import ibs_amd
    wouts, steps, _ = bench.emulated_equilibria(wout)
    wouts = [{k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in w.items()} for w in wouts]
    step = ibs_amd.AdjointStep(ctx, ibs_amd.theta_grid_for(11, 11), np.linspace(0.5, 0.95, 5), dev, nalpha=24, ntheta0=15)
    f_other = 0.8 + 0.01 * np.arange(len(wouts))
    job = bench.C2Sharded
    svals = np.linspace(0.1, 0.95, job.NS)
    scan = ibs_amd.BallooningScan(ctx, None, ibs_amd.theta_grid(job.N), svals, nalpha=job.NA, ntheta0=job.NT0,
                                  tables=ibs_amd.SurfaceTables.from_wout(wout, svals), device=dev)
    out = {}
    for name, work in (("AdjointStep.run", lambda: step.run(wouts, f_other, steps)), ("local_rows", scan.local_rows)):
        work()                                                            # (the warm-up)
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize(); t0 = time.perf_counter(); work(); ts.append((time.perf_counter() - t0) * 1e3)
        out[name] = ts
    with open(record_path, "w") as fh:
        json.dump(out, fh)


def first_call_difference(p, q):
    """where two transcripts of Context calls part"""
    a, b = p.get("calls", []), q.get("calls", [])
    for i, (x, y) in enumerate(zip(a, b)):
        if x != y:
            return " (call %d: %s against %s)" % (i, json.dumps(x)[:300], json.dumps(y)[:300])
    return " (%d calls against %d)" % (len(a), len(b)) if len(a) != len(b) else ""


def worst_difference(p, q, name):
    """for an array small enough to be on record: the number of differing elements and the largest difference relative to the largest magnitude"""
    import numpy as np
    if name not in p.get("raw", {}) or name not in q.get("raw", {}):
        return ""
    x, y = (bytes.fromhex(e["raw"][name]) for e in (p, q))
    dt = np.float64 if len(x) == 8 * p["arrays"][name][0] else np.float32
    x, y = np.frombuffer(x, dt), np.frombuffer(y, dt)
    ok = np.isfinite(x) & np.isfinite(y)
    rel = float(np.abs(x[ok] - y[ok]).max() / max(np.abs(x[ok]).max(), 1e-300)) if ok.any() else float("nan")
    return " (%d of %d elements, largest difference %.2g of the largest magnitude)" % (int((x.view(np.uint8) != y.view(np.uint8)).reshape(len(x), -1).any(axis=1).sum()), len(x), rel)


def run_children(sides):
    """start one child per (command with a %s for its record file, environment), side by side in fresh processes, and return their
    records -- or None: a child that ends badly (a fault, a refused call) ends the run, the others are stopped, nothing more is
    started on the GPU"""
    tmp = tempfile.mkdtemp(prefix="ibs_bitwise_")                                # (the children's records; removed once they are read)
    files = [os.path.join(tmp, "bitwise_%d.json" % i) for i in range(len(sides))]
    procs = [subprocess.Popen([rec if arg == "%s" else arg for arg in cmd], env=env) for rec, (cmd, env) in zip(files, sides)]
    deadline, codes = time.time() + 900, [None] * len(sides)
    while None in codes and time.time() < deadline and not any(codes):
        time.sleep(0.5)
        codes = [p.poll() for p in procs]
    for p in procs:
        if p.poll() is None:
            p.kill()
            p.wait()
    recs = None
    if codes != [0] * len(sides):
        print("the children (the parent's side first) ended with", codes, "(None: stopped, or still running after 900 s)")
    else:
        recs = []
        for rec in files:
            with open(rec) as fh:
                recs.append(json.load(fh))
    shutil.rmtree(tmp, ignore_errors=True)
    return recs


def compare_times(sides, log, turns=2):
    """--time: children on the parent's and on this tree's scan.py in turn, one at a time; per workload the medians and spreads
    (largest minus smallest repetition) of all repetitions of a side.  The new median may exceed the parent's by the parent's spread."""
    import numpy as np
    ts = [{}, {}]
    for _ in range(turns):
        for side in (0, 1):
            recs = run_children([sides[side]])
            if recs is None:
                return 2
            for name, v in recs[0].items():
                ts[side].setdefault(name, []).extend(v)
    lines, slower = [], False
    for name in ts[0]:
        (pm, ps), (nm, ns) = ((float(np.median(t[name])), max(t[name]) - min(t[name])) for t in ts)
        ok = nm <= pm + ps
        slower |= not ok
        lines.append("%-16s parent median %.3f ms, spread %.3f ms | new median %.3f ms, spread %.3f ms | %d repetitions a side | %s"
                     % (name, pm, ps, nm, ns, len(ts[0][name]), "no slower" if ok else "SLOWER"))
    print("\n".join(lines))
    if log:                                 # (appended, marked: the log of a --parent-scan run keeps its case lines)
        with open(log, "a") as fh:
            fh.write("".join("time | %s\n" % ln for ln in lines))
    return 1 if slower else 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--parent", help="the other build's libibs_hip.so")
    ap.add_argument("--new", default=os.path.join(ROOT, "ideal-ballooning-solver_amd", "lib", "libibs_hip.so"))
    ap.add_argument("--log", help="write one line per case here")
    ap.add_argument("--parent-scan", help="the driver family instead: the other version of ideal-ballooning-solver_amd/scan.py, "
                    "loaded as the package's scan submodule, against this tree's, both on this build of the library")
    ap.add_argument("--cpu", action="store_true", help="with --parent-scan: the rehearsal on tests.helpers.OracleContext, no GPU")
    ap.add_argument("--time", action="store_true", help="with --parent-scan: wall time of AdjointStep.run() and local_rows(), "
                    "children on the two files in turn")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    ap.add_argument("--driver-child", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child)
    if a.driver_child:
        return driver_child(a.driver_child, a.parent_scan, a.cpu, a.time)
    me = [sys.executable, os.path.abspath(__file__)]
    if a.parent_scan:
        flags = (["--cpu"] if a.cpu else []) + (["--time"] if a.time else [])
        sides = [(me + ["--driver-child", "%s", "--parent-scan", os.path.abspath(a.parent_scan)] + flags, os.environ),
                 (me + ["--driver-child", "%s"] + flags, os.environ)]
        if a.time:
            return compare_times(sides, a.log)
    else:
        sides = [(me + ["--child", "%s"], dict(os.environ, IBS_LIB_PATH=os.path.abspath(path))) for path in (a.parent, a.new)]
    recs = run_children(sides)
    if recs is None:
        return 2
    if [e["case"] for e in recs[0]] != [e["case"] for e in recs[1]]:
        print("the two children ran different cases: %d against %d" % (len(recs[0]), len(recs[1])))
        return 2
    log = open(a.log, "w") if a.log else None
    by_kernel, n_arr, n_el, bad = {}, 0, 0, []
    for p, q in zip(*recs):
        same = p["arrays"] == q["arrays"] and p["rc"] == q["rc"] and p["kernel"] == q["kernel"]
        n_arr += len(q["arrays"]); n_el += sum(v[0] for v in q["arrays"].values())
        if not same:
            bad.append(q["case"] + " | " + q["kernel"] + " | " + ", ".join(
                name + (first_call_difference(p, q) if name == "calls" else worst_difference(p, q, name))
                for name in q["arrays"] if p["arrays"].get(name) != q["arrays"][name]))
        k = by_kernel.setdefault(q["kernel"], [0, 0, 0, 0])
        k[0] += 1
        for i, v in enumerate(q.get("bits", (0, 0, 0))):
            k[1 + i] += v
        if log and q["kernel"] == "driver":
            log.write("%s | %s | %s\n" % (q["case"], "returns" if not q["rc"] else "raises " + q["arrays"]["error"][1][:80],
                                          "same" if same else "DIFFERENT"))
        elif log:
            log.write("%s | %s | rc %d | bits 1/2/3: %s | %s\n" % (q["case"], q["kernel"], q["rc"], q.get("bits"), "same" if same else "DIFFERENT"))
    if log:
        log.close()
    print("%-52s %7s %9s %9s %9s" % ("kernel (ibs_last_launch)", "cases", "bit 1", "bit 2", "bit 3"))
    for name in sorted(by_kernel):
        print("%-52s %7d %9d %9d %9d" % (name, *by_kernel[name]))
    print("%d cases, %d arrays, %d elements: %s" % (len(recs[1]), n_arr, n_el, "all bitwise equal" if not bad else "%d cases DIFFER" % len(bad)))
    for case in bad[:40]:
        print("  differs:", case)
    for q in recs[1]:
        if q["kernel"] == "driver" and q["rc"]:
            print("  raised (on this tree's side):", q["case"], "|", q["arrays"]["error"][1][:200])
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
