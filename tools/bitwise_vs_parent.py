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
bit 2 (FP32 result replaced by the FP64 solve) and bit 3 (re-closed); the parent process compares the two records."""
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


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--parent", help="the other build's libibs_hip.so")
    ap.add_argument("--new", default=os.path.join(ROOT, "ideal-ballooning-solver_amd", "lib", "libibs_hip.so"))
    ap.add_argument("--log", help="write one line per case here")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child)
    tmp = tempfile.mkdtemp(prefix="ibs_bitwise_")                                # (the children's records; removed once they are read)
    files = [os.path.join(tmp, "bitwise_%s.json" % tag) for tag in ("parent", "new")]
    procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__), "--child", rec], env=dict(os.environ, IBS_LIB_PATH=os.path.abspath(path)))
             for rec, path in zip(files, (a.parent, a.new))]                     # (side by side: the two never share a process)
    # a child that ends badly (a fault, a refused call) ends the run: the other one is stopped, nothing more is started on the GPU
    deadline, codes = time.time() + 900, [None, None]
    while None in codes and time.time() < deadline and not any(codes):
        time.sleep(0.5)
        codes = [p.poll() for p in procs]
    for p in procs:
        if p.poll() is None:
            p.kill()
            p.wait()
    if codes != [0, 0]:
        shutil.rmtree(tmp, ignore_errors=True)
        print("the children (parent's library, this build) ended with", codes, "(None: stopped, or still running after 900 s)")
        return 2
    recs = []
    for rec in files:
        with open(rec) as fh:
            recs.append(json.load(fh))
    shutil.rmtree(tmp, ignore_errors=True)
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
                name + worst_difference(p, q, name) for name in q["arrays"] if p["arrays"].get(name) != q["arrays"][name]))
        k = by_kernel.setdefault(q["kernel"], [0, 0, 0, 0])
        k[0] += 1
        for i, v in enumerate(q.get("bits", (0, 0, 0))):
            k[1 + i] += v
        if log:
            log.write("%s | %s | rc %d | bits 1/2/3: %s | %s\n" % (q["case"], q["kernel"], q["rc"], q.get("bits"), "same" if same else "DIFFERENT"))
    if log:
        log.close()
    print("%-52s %7s %9s %9s %9s" % ("kernel (ibs_last_launch)", "cases", "bit 1", "bit 2", "bit 3"))
    for name in sorted(by_kernel):
        print("%-52s %7d %9d %9d %9d" % (name, *by_kernel[name]))
    print("%d cases, %d arrays, %d elements: %s" % (len(recs[1]), n_arr, n_el, "all bitwise equal" if not bad else "%d cases DIFFER" % len(bad)))
    for case in bad[:40]:
        print("  differs:", case)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
