"""CPU: the host layer of the spectrum mode -- the two C entry points in header, library and _lib.SYMBOLS; the marshalling of
Context.solve_gcf_modes / gamma_scan_modes against tests/golden/B2_modes_calls_host.json (transcripts of the recorder's stand-in
library: tests/tools/binding_recorder.py), error cases included; BallooningScan.modes against mode_count on the CPU stand-in context of
tests/modes_oracle.py; and that stand-in against the exact counts of the oracle."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import ibs_amd
from ibs_amd import _lib
from oracle import ballooning_oracle as bo
from tests import modes_oracle as mo
from tests.helpers import synthetic_fieldlines
from tests.test_cabi import header_prototypes
from tests.tools import binding_recorder as br

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "B2_modes_calls_host.json")
P, D, I32, I64 = C.c_void_p, C.c_double, C.c_int32, C.c_int64


def test_the_two_entry_points_and_their_argument_rows():
    rows = {
        "ibs_solve_gcf_modes_f64": [P, I64, I32, D, P, P, P, P, I64, I32, P, P, P, P, P, I32],
        "ibs_gamma_scan_modes_f64": [P, I32, I32, I32, D, P, P, P, P, P, P, P, I64, P, P, I32, P, P, P, I32],
    }
    protos = header_prototypes()
    lib = _lib.lib()
    for name, row in rows.items():
        assert _lib.SYMBOLS[name] == (C.c_int, row), name
        assert hasattr(lib, name) and name in protos and len(protos[name][1]) == len(row), name
    assert protos["ibs_solve_gcf_modes_f64"][1][9] == "int32_t" and protos["ibs_gamma_scan_modes_f64"][1][15] == "int32_t"
    # argument errors need no GPU: the order of the checks is null context, then the arguments
    z = np.ones(67)
    p = z.ctypes.data
    assert lib.ibs_solve_gcf_modes_f64(None, 1, 67, 0.1, p, None, p, p, 67, 2, p, None, None, None, None, 1) == -1
    assert b"null" in lib.ibs_last_error()
    assert ibs_amd.MAX_MODES == 16 and ibs_amd.CLUSTER_BIT == 1 << 9 == mo.CLUSTER_BIT
    txt = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ibs.h")).read()
    assert "bit 9, spectrum-mode entry points" in txt


def modes_cases(d, device=None):
    """[(case name, method, args, kwargs)] of the two methods; device: the torch.device of d, or None for the host cases"""
    h = 0.09
    g, c, f = d["g"], d["c"], d["f"]
    scan = (*d["scan7"], d["dP"], d["t0_scan"])
    out = []
    for tag, kw in br._subsets(("want_X", "want_info")):
        out.append(("solve_gcf_modes/" + tag, "solve_gcf_modes", (h, g, c, f, 4), kw))
    out.append(("solve_gcf_modes/gh-one-mode", "solve_gcf_modes", (h, g, c, f, 1), dict(gh=d["gh"], want_X=True)))
    out.append(("solve_gcf_modes/sixteen", "solve_gcf_modes", (h, g, c, f, 16), {}))
    for tag, kw in br._subsets(("want_info",)):
        out.append(("gamma_scan_modes/" + tag, "gamma_scan_modes", (h, *scan, 3), kw))
    out.append(("gamma_scan_modes/sixteen", "gamma_scan_modes", (h, *scan, 16), {}))
    for K in (0, 17, 2.5, True, "3"):
        out.append(("solve_gcf_modes/error-n_modes-%s" % K, "solve_gcf_modes", (h, g, c, f, K), {}))
        out.append(("gamma_scan_modes/error-n_modes-%s" % K, "gamma_scan_modes", (h, *scan, K), {}))
    out.append(("solve_gcf_modes/error-shape-c", "solve_gcf_modes", (h, g, c[:2], f, 2), {}))
    out.append(("solve_gcf_modes/error-shape-gh", "solve_gcf_modes", (h, g, c, f, 2), dict(gh=d["gh"][:, :-1])))
    out.append(("solve_gcf_modes/error-shape-1d", "solve_gcf_modes", (h, g[0], c[0], f[0], 2), {}))
    out.append(("gamma_scan_modes/error-shape-1d", "gamma_scan_modes", (h, *[a[0] for a in d["scan7"]], d["dP"], d["t0_scan"], 2), {}))
    out.append(("gamma_scan_modes/error-shape-geo", "gamma_scan_modes", (h, d["scan7"][0], d["scan7"][1][:1], *d["scan7"][2:], d["dP"], d["t0_scan"], 2), {}))
    out.append(("gamma_scan_modes/error-shape-dP", "gamma_scan_modes", (h, *d["scan7"], d["dP"][:1], d["t0_scan"], 2), {}))
    if device is not None:
        host = d["np"]
        out.append(("mixed/solve_gcf_modes", "solve_gcf_modes", (h, g, host["c"], f, 2), {}))
        out.append(("mixed/solve_gcf_modes-host-first", "solve_gcf_modes", (h, host["g"], c, f, 2), {}))
        out.append(("mixed/gamma_scan_modes", "gamma_scan_modes", (h, *d["scan7"], host["dP"], d["t0_scan"], 2), {}))
    return out


def record(device=None):
    with br.stand_in(device is not None) as fake:
        ctx = ibs_amd.Context(0)
        d = br.make_data(device)
        out = {name: br.run_case(ctx, fake, method, args, kw) for name, method, args, kw in modes_cases(d, device)}
        ctx.close()
    return out


@pytest.fixture(scope="module")
def recorded():
    return record()


def test_transcripts_match_the_golden(recorded):
    with open(GOLDEN) as fh:
        golden = json.load(fh)
    assert sorted(recorded) == sorted(golden) and len(golden) >= 20
    bad = [k for k in sorted(golden) if recorded[k] != golden[k]]
    assert not bad, "\n".join("%s:\n  now    %s\n  golden %s" % (k, recorded[k], golden[k]) for k in bad[:5])


def test_what_the_transcripts_say(recorded):
    """independent of the golden file: one compute call in prototype order, the outputs' shapes, nbad passed through"""
    r = recorded["solve_gcf_modes/want_X-want_info"]
    (sym, a), = r["calls"]
    assert sym == "ibs_solve_gcf_modes_f64"
    assert a == ["handle", "i:3", "i:67", "f:0.09", "in:g", "null", "in:c", "in:f", "i:67", "i:4", "out:lam:(3, 4):float64",
                 "out:gam:(3, 4):float64", "out:X:(3, 4, 67):float64", "out:dX:(3, 4, 67):float64", "out:info:(3, 4):int32", "i:1"]
    assert r["result"]["nbad"] == br.NBAD
    (sym, a), = recorded["solve_gcf_modes/gh-one-mode"]["calls"]
    assert a[5] == "in:gh" and a[9] == "i:1" and a[-2] == "null"
    (sym, a), = recorded["gamma_scan_modes/want_info"]["calls"]
    assert sym == "ibs_gamma_scan_modes_f64" and a[1:5] == ["i:2", "i:3", "i:67", "f:0.09"] and a[12] == "i:67"
    assert a[13:] == ["in:dPdrho", "in:theta0", "i:3", "out:gam:(2, 3, 3):float64", "out:lam:(2, 3, 3):float64", "out:info:(2, 3, 3):int32", "i:1"]
    assert recorded["gamma_scan_modes/plain"]["calls"][0][1][-2] == "null"
    assert not [k for k, v in recorded.items() if any(c[0] == "ibs_set_stream" for c in v["calls"])]


def test_errors_reach_no_compute_call(recorded):
    errs = [k for k, v in recorded.items() if br.is_error(v["result"])]
    assert sorted(errs) == sorted(k for k in recorded if "/error-" in k) and len(errs) == 16
    assert all(recorded[k]["result"].startswith("IbsError: ") for k in errs), [recorded[k]["result"] for k in errs]
    assert not [k for k in errs if recorded[k]["calls"]]
    for k in errs:
        if "error-n_modes" in k:
            assert recorded[k]["result"].startswith("IbsError: n_modes must be an integer in [1, 16]"), recorded[k]


# ---- the scan driver on the CPU stand-in
def driver(K=8.0, **kw):
    N = 131
    th = bo.theta_grid(N)
    base = synthetic_fieldlines(th)

    def fieldlines(rho, alphas):
        out = base(rho, alphas).copy()
        out[:, 7] = out[:, 2] - 2.0 * K / out[:, 0] ** 2          # gbdrift: dPdrho = -K on every line
        return out
    return ibs_amd.BallooningScan(mo.ModesOracleContext(), fieldlines, th, np.array([0.3, 0.7]), nalpha=3, ntheta0=2, **kw)


def test_scan_driver_modes_agree_with_mode_count():
    sc = driver()
    K = 4
    md = sc.modes(K)
    cnt = sc.mode_count()
    assert md["lam"].shape == md["gam"].shape == md["cluster"].shape == (2, 3, 2, K) and md["cluster"].dtype == bool
    assert cnt.shape == (2, 3, 2) and cnt.max() > 1 and cnt.min() < K          # (some lines have fewer unstable modes than K)
    assert np.array_equal((md["lam"] > 0).sum(-1), np.minimum(K, cnt)), ((md["lam"] > 0).sum(-1), cnt)
    assert (np.diff(md["lam"], axis=-1) < 0).all() and not md["cluster"].any()
    one = sc.modes(1)
    assert np.array_equal(one["lam"][..., 0], md["lam"][..., 0])
    # a rank that owns nothing
    empty = driver(rank=3, world=4).modes(2)
    assert empty["lam"].shape == (0, 3, 2, 2) and empty["cluster"].dtype == bool


def test_reference_counts_are_the_oracles():
    """a guard on the REFERENCE, not on the library (it passes with or without the spectrum mode): the spectrum of tests/modes_oracle.py
    against the oracle's exact Sturm count (bo.sturm_count_above) between the top eigenvalues"""
    th, g, c, f = mo.salpha_line(131, -8.0)
    ref = mo.dense_modes(th, g, c, f, 6, vectors=False)
    d, e, fd = bo.assemble(th, g, c, f)[:3]
    for m in range(5):
        assert bo.sturm_count_above(d, e, fd, 0.5 * (ref["lam"][m] + ref["lam"][m + 1])) == m + 1
    assert int((ref["lam"] > 0).sum()) == 5
