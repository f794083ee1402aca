"""Per-call Python cost of the binding, without a kernel: three Context methods under the recorder's stand-in, this tree's solver.py
(child) against another version of it (parent), alternately in one process.

    python tests/tools/binding_call_cost.py host|device PARENT/solver.py [OUT.json]

Per method: five repeats of (median over 2000 parent calls, median over 2000 child calls), in microseconds, and whether the child's
median of medians stays within the parent's plus the parent's own spread (max - min) across its five repeats."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import binding_recorder as br       # noqa: E402

CALLS, REPEATS = 2000, 5


def median_us(fn):
    t = []
    for _ in range(CALLS):
        t0 = time.perf_counter_ns()
        fn()
        t.append(time.perf_counter_ns() - t0)
    return statistics.median(t) / 1e3


def main():
    mode, parent_path = sys.argv[1], sys.argv[2]
    device = None
    if mode == "device":
        import torch
        device = torch.device("cuda:0")
    parent = br.load_solver(parent_path)
    out = {}
    with br.stand_in(device is not None):
        ctxs = dict(parent=parent.Context(0), child=br.ibs_amd.Context(0))
        d = br.make_data(device)
        scan = (*d["scan7"], d["dP"], d["t0_scan"])
        work = {
            "solve_gcf(1 system, want_X)": lambda c: c.solve_gcf(0.09, d["g"][:1], d["c"][:1], d["f"][:1], want_X=True),
            "gamma_scan": lambda c: c.gamma_scan(0.09, *scan),
            "obj_w_grad_exact(want_info)": lambda c: c.obj_w_grad_exact(0.09, d["geo4"], d["t0_pts"], want_info=True),
        }
        for name, fn in work.items():
            for c in ctxs.values():
                for _ in range(3000):
                    fn(c)
            rows = {"parent": [], "child": []}
            for _ in range(REPEATS):
                for who, c in ctxs.items():
                    rows[who].append(round(median_us(lambda: fn(c)), 2))
            spread = max(rows["parent"]) - min(rows["parent"])
            rows["parent_spread"] = round(spread, 2)
            rows["within"] = statistics.median(rows["child"]) <= statistics.median(rows["parent"]) + spread
            out[name] = rows
            print(mode, name, json.dumps(rows), flush=True)
        for c in ctxs.values():
            c.close()
    if len(sys.argv) > 3:
        with open(sys.argv[3], "w") as fh:
            json.dump({mode: out}, fh, indent=1)


if __name__ == "__main__":
    main()
