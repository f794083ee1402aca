"""CPU: the rule of the theta0 polish (csrc/ibs_theta0_polish.hpp) -- ibs_row_peaks_f64 against ibs_amd.row_peaks on hand-written and
random rows; the C state machine (ibs_theta0_polish_init / _step / _result) against ibs_amd.polish_theta0, both driven by the CPU
oracle's gam on lines whose crest lies between the nodes or on the edge of the box; the marshalling of Context.theta0_polish against
tests/golden/B5_theta0_polish_calls_host.json (transcripts of the recorder's stand-in library); the argument checks of
ibs_theta0_polish_f64 without a context."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import ibs_amd
from ibs_amd import _lib
from tests import theta0_polish_cases as tc
from tests.tools import binding_recorder as br

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "B5_theta0_polish_calls_host.json")
XTOL = 1e-5
BIT_NODE, BIT_MAXEVAL, BIT_ONE_SIDED = 1 << 10, 1 << 11, 1 << 12


# ---- row peaks
def c_row_peaks(gam, K):
    lib = _lib.lib()
    tab = np.ascontiguousarray(np.atleast_2d(gam), dtype=np.float64)
    node = np.full((tab.shape[0], K), -7, dtype=np.int32)
    nf = np.full(tab.shape[0], -7, dtype=np.int32)
    assert lib.ibs_row_peaks_f64(tab.shape[0], tab.shape[1], K, tab.ctypes.data, node.ctypes.data, nf.ctypes.data) == 0
    return node, nf


@pytest.mark.parametrize("k", range(len(tc.HAND_ROWS)))
def test_hand_rows(k):
    row, node4, nf = tc.HAND_ROWS[k]
    for K in (1, 2, 3, 4):
        want = [node4[s] if s < nf else node4[0] for s in range(K)]
        for node, n_found in (ibs_amd.row_peaks(row, K), c_row_peaks(row, K)):
            assert node.dtype == np.int32 and node.shape == (1, K)
            assert list(node[0]) == want and n_found[0] == min(nf, K), (row, K, node, n_found)


def test_random_rows_c_equals_numpy():
    rng = np.random.default_rng(715)
    for nt in (1, 2, 3, 5, 15, 64):
        tab = rng.integers(0, 4, size=(200, nt)).astype(np.float64)          # (few distinct values: plateaus and ties)
        tab[rng.random(tab.shape) < 0.15] = np.nan
        tab[0] = np.nan
        for K in (1, 2, 3, 4):
            a, b = ibs_amd.row_peaks(tab, K), c_row_peaks(tab, K)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (nt, K)
        assert a[1][0] == 0 and np.all(a[0][0] == -1)


def test_row_peaks_refuses_bad_arguments():
    lib = _lib.lib()
    tab, node = np.zeros((1, 3)), np.zeros((1, 4), dtype=np.int32)
    for n_rows, nt, K, g, nd in ((1, 3, 0, tab, node), (1, 3, 5, tab, node), (1, 0, 1, tab, node), (-1, 3, 1, tab, node)):
        assert lib.ibs_row_peaks_f64(n_rows, nt, K, g.ctypes.data, nd.ctypes.data, None) == -1
    assert lib.ibs_row_peaks_f64(1, 3, 1, None, node.ctypes.data, None) == -1
    for K in (0, 5, True, 2.0):
        with pytest.raises(ValueError):
            ibs_amd.row_peaks(tab, K)


# ---- the state machine
def drive_c(fun, theta0, row, node, xtol, max_eval):
    """the C state machine driven by fun(theta0) -> gam: dict(theta0, gam, n_eval, status, points)"""
    lib = _lib.lib()
    st = C.create_string_buffer(lib.ibs_theta0_polish_state_bytes())
    theta0 = np.ascontiguousarray(theta0, dtype=np.float64)
    row = np.ascontiguousarray(row, dtype=np.float64)
    x = C.c_double()
    more = lib.ibs_theta0_polish_init(st, len(theta0), theta0.ctypes.data, row.ctypes.data, int(node), xtol, max_eval, C.byref(x))
    pts = []
    while more == 1:
        pts.append(x.value)
        assert len(pts) <= 64
        more = lib.ibs_theta0_polish_step(st, fun(x.value), 0, C.byref(x))
    assert more == 0
    ts, gs, ne, stt = C.c_double(), C.c_double(), C.c_int32(), C.c_int32()
    assert lib.ibs_theta0_polish_result(st, C.byref(ts), C.byref(gs), C.byref(ne), C.byref(stt)) == 0
    return dict(theta0=ts.value, gam=gs.value, n_eval=ne.value, status=stt.value, points=pts)


_RUNS = {}


def run(N, nt, case, max_eval=32):
    """(C result, Python result, theta0 grid, row, node) of one case, computed once"""
    key = (N, nt, case, max_eval)
    if key not in _RUNS:
        t0, row = tc.theta0_grid(nt), tc.oracle_row(N, case, nt)
        node = int(ibs_amd.row_peaks(row, 1)[0][0, 0])
        fun = lambda t: tc.oracle_gam(N, case, t)
        _RUNS[key] = (drive_c(fun, t0, row, node, XTOL, max_eval), ibs_amd.polish_theta0(fun, t0, row, node, XTOL, max_eval), t0, row, node)
    return _RUNS[key]


ALL = [(N, nt, case) for N in (67, 131) for nt in tc.GRIDS for case in tc.CASES]


@pytest.mark.parametrize("N,nt,case", ALL)
def test_c_and_python_request_the_same_points(N, nt, case):
    c, p, t0, row, node = run(N, nt, case)
    assert c["points"] == p["points"] and len(c["points"]) == c["n_eval"] == p["n_eval"]
    assert (c["theta0"], c["gam"], c["status"]) == (p["theta0"], p["gam"], p["status"])
    lo, hi = tc.bracket(t0, row, node)
    assert all(lo <= u <= hi for u in c["points"])
    assert not any(u in t0 for u in c["points"]), "a node was evaluated again"


@pytest.mark.parametrize("N,nt,case", ALL)
def test_result_is_the_maximum_of_the_bracket(N, nt, case):
    """gam* >= the maximum of 801 oracle samples of the bracket - 1e-8 (the issue's CPU prototype: worst -5.9e-13), and >= the node"""
    c, _, t0, row, node = run(N, nt, case)
    lo, hi = tc.bracket(t0, row, node)
    dense = tc.dense_max(N, case, lo, hi)
    print("gam* - dense max = %.3e, gam* - node = %.3e, n_eval = %d" % (c["gam"] - dense, c["gam"] - row[node], c["n_eval"]))
    assert c["gam"] >= dense - 1e-8
    assert c["gam"] >= row[node]
    assert c["gam"] == tc.oracle_gam(N, case, c["theta0"])


@pytest.mark.parametrize("N,nt,case", [a for a in ALL if a[2] in tc.INTERIOR])
def test_interior_crests_take_few_evaluations(N, nt, case):
    """a cap that keeps a broken parabolic step from hiding behind golden section (the prototype needed 5-7)"""
    c, _, t0, row, node = run(N, nt, case)
    assert c["n_eval"] <= 10 and not c["status"] & (BIT_NODE | BIT_MAXEVAL | 3)
    assert c["gam"] > row[node]
    one_sided = node == 0 or node == nt - 1
    assert bool(c["status"] & BIT_ONE_SIDED) == one_sided


@pytest.mark.parametrize("N,nt,case", [a for a in ALL if a[2] in tc.EDGE])
def test_edge_cases_return_the_node(N, nt, case):
    c, _, t0, row, node = run(N, nt, case)
    assert node in (0, nt - 1)
    assert c["theta0"] == t0[node] and c["gam"] == row[node]
    assert c["status"] & BIT_NODE and c["status"] & BIT_ONE_SIDED and not c["status"] & BIT_MAXEVAL


@pytest.mark.parametrize("case", tc.CASES)
def test_max_eval_3_stops_and_keeps_the_incumbent(case):
    c, p, t0, row, node = run(67, 5, case, max_eval=3)
    assert c["n_eval"] == 3 and c["status"] & BIT_MAXEVAL
    assert (c["points"], c["theta0"], c["gam"], c["status"]) == (p["points"], p["theta0"], p["gam"], p["status"])
    best = max(tc.oracle_gam(67, case, u) for u in c["points"])
    if best > row[node]:
        assert c["gam"] == best and not c["status"] & BIT_NODE
    else:
        assert (c["theta0"], c["gam"]) == (t0[node], row[node]) and c["status"] & BIT_NODE


def test_degenerate_brackets_and_failed_evaluations():
    t0 = tc.theta0_grid(5)
    # zero length: a row of one node, and both neighbours NaN
    for th, row, node in ((t0[:1], [0.3], 0), (t0, [0.1, np.nan, 0.3, np.nan, 0.2], 2)):
        for r in (drive_c(lambda t: 9.0, th, row, node, XTOL, 32), ibs_amd.polish_theta0(lambda t: 9.0, th, row, node, XTOL, 32)):
            assert (r["theta0"], r["gam"], r["n_eval"], r["status"], r["points"]) == (th[node], row[node], 0, BIT_NODE, [])
    # one NaN neighbour beside the peak: one-sided
    row = [0.1, np.nan, 0.3, 0.2, 0.1]
    fun = lambda t: 0.32 - (t - 0.9) ** 2
    c, p = drive_c(fun, t0, row, 2, XTOL, 32), ibs_amd.polish_theta0(fun, t0, row, 2, XTOL, 32)
    assert c["points"] == p["points"] and c["status"] == p["status"] and c["status"] & BIT_ONE_SIDED
    assert abs(c["theta0"] - 0.9) < 4 * XTOL and c["gam"] > 0.32 - 1e-9
    # every evaluation fails: the node, with the status bits of the evaluations
    lib = _lib.lib()
    st = C.create_string_buffer(lib.ibs_theta0_polish_state_bytes())
    th, rw, x = np.ascontiguousarray(t0), np.array([0.1, 0.2, 0.3, 0.2, 0.1]), C.c_double()
    more, n = lib.ibs_theta0_polish_init(st, 5, th.ctypes.data, rw.ctypes.data, 2, XTOL, 32, C.byref(x)), 0
    while more == 1:
        more, n = lib.ibs_theta0_polish_step(st, float("nan"), 2, C.byref(x)), n + 1
    ts, gs, ne, stt = C.c_double(), C.c_double(), C.c_int32(), C.c_int32()
    lib.ibs_theta0_polish_result(st, C.byref(ts), C.byref(gs), C.byref(ne), C.byref(stt))
    assert (ts.value, gs.value) == (t0[2], 0.3) and ne.value == n <= 32 and stt.value & BIT_NODE and stt.value & 3 == 2
    p = ibs_amd.polish_theta0(lambda t: (float("nan"), 2), t0, rw, 2, XTOL, 32)
    assert (p["theta0"], p["gam"], p["n_eval"], p["status"]) == (ts.value, gs.value, ne.value, stt.value)


def test_a_failed_evaluation_counts_as_minus_infinity_however_finite():
    """a solve with status bit 0 or 1 and a FINITE gam above the node's must not become the result: with every evaluation failed the
    node comes back; with the evaluations right of 0.9 failed the search ends left of it; C and Python take the same steps"""
    lib = _lib.lib()
    t0, row = tc.theta0_grid(5), np.array([0.1, 0.2, 0.3, 0.2, 0.1])
    th = np.ascontiguousarray(t0)

    def c_run(fun):
        st, x, pts = C.create_string_buffer(lib.ibs_theta0_polish_state_bytes()), C.c_double(), []
        more = lib.ibs_theta0_polish_init(st, 5, th.ctypes.data, row.ctypes.data, 2, XTOL, 32, C.byref(x))
        while more == 1:
            pts.append(x.value)
            g, status = fun(x.value)
            more = lib.ibs_theta0_polish_step(st, g, status, C.byref(x))
        ts, gs, ne, stt = C.c_double(), C.c_double(), C.c_int32(), C.c_int32()
        lib.ibs_theta0_polish_result(st, C.byref(ts), C.byref(gs), C.byref(ne), C.byref(stt))
        return dict(theta0=ts.value, gam=gs.value, n_eval=ne.value, status=stt.value, points=pts)

    for bit in (1, 2):
        fun = lambda t: (5.0 - (t - 0.9) ** 2, bit)                      # far above the node's 0.3, every evaluation failed
        c, p = c_run(fun), ibs_amd.polish_theta0(fun, t0, row, 2, XTOL, 32)
        assert (c["theta0"], c["gam"]) == (t0[2], 0.3) and c["status"] & BIT_NODE and c["status"] & 3 == bit
        assert {k: c[k] for k in c} == {k: p[k] for k in c}
    # a row of the parabola itself: the first step lands on its crest 0.9, where -- as everywhere right of 0.85 -- the solve fails
    row[:] = 5.0 - (t0 - 0.9) ** 2
    fun = lambda t: (5.0 - (t - 0.9) ** 2, 1 if t > 0.85 else 0)
    c, p = c_run(fun), ibs_amd.polish_theta0(fun, t0, row, 2, XTOL, 32)
    assert {k: c[k] for k in c} == {k: p[k] for k in c}
    assert any(u > 0.85 for u in c["points"]), "no failed evaluation was met: the case shows nothing"
    assert t0[2] < c["theta0"] <= 0.85 and c["gam"] == 5.0 - (c["theta0"] - 0.9) ** 2 and c["gam"] > row[2]
    assert c["status"] & 3 == 1 and not c["status"] & BIT_NODE


def test_host_entry_points_refuse_bad_arguments():
    lib = _lib.lib()
    st = C.create_string_buffer(lib.ibs_theta0_polish_state_bytes())
    t0, row, x = tc.theta0_grid(5), np.array([0.1, 0.2, 0.3, 0.2, 0.1]), C.c_double()
    init = lambda th, rw, node, xtol, me: lib.ibs_theta0_polish_init(st, len(th), th.ctypes.data, rw.ctypes.data, node, xtol, me, C.byref(x))
    assert init(t0, row, 2, XTOL, 32) == 1
    for args in ((t0, row, -1, XTOL, 32), (t0, row, 5, XTOL, 32), (t0, row, 2, 0.0, 32), (t0, row, 2, float("nan"), 32),
                 (t0, row, 2, XTOL, 0), (t0, row, 2, XTOL, 65), (t0[::-1].copy(), row, 2, XTOL, 32),
                 (t0, np.array([0.1, 0.2, np.nan, 0.2, 0.1]), 2, XTOL, 32)):
        assert init(*args) == -1, args[2:]
    for args in ((t0, row, 5, XTOL, 32), (t0, row, 2, -1.0, 32), (t0, row, 2, XTOL, 65), (t0[::-1], row, 2, XTOL, 32)):
        with pytest.raises(ValueError):
            ibs_amd.polish_theta0(lambda t: 0.0, *args)


# ---- ibs_theta0_polish_f64: the argument checks come before the context
def test_argument_errors_need_no_context():
    lib = _lib.lib()
    N, nl, nt = 67, 2, 3
    a = np.ones((nl, N)); dP = np.ones(nl); t0 = np.array([0.0, 0.5, 1.0]); gam = np.zeros((nl, nt)); out = np.zeros((nl, 4))
    p = lambda x: None if x is None else x.ctypes.data

    def call(n_lines=nl, n_theta0=nt, n=N, h=0.1, arr=a, ld=N, theta0=t0, gam_=gam, K=1, xtol=XTOL, max_eval=32, ts=out, gs=out):
        return lib.ibs_theta0_polish_f64(None, n_lines, n_theta0, n, h, p(arr), p(a), p(a), p(a), p(a), p(a), p(a), ld, p(dP), p(theta0),
                                         p(gam_), None, None, K, xtol, max_eval, p(ts), p(gs), None, None, None, None, None, _lib.MEM_HOST)

    assert call() == -1 and b"null context" in lib.ibs_last_error()
    for kw in (dict(K=0), dict(K=5), dict(xtol=0.0), dict(xtol=-1.0), dict(xtol=float("inf")), dict(xtol=float("nan")), dict(max_eval=0),
               dict(max_eval=65), dict(n_lines=-1), dict(n_theta0=0), dict(n=0), dict(arr=None), dict(theta0=None), dict(gam_=None),
               dict(ts=None), dict(gs=None), dict(ld=N - 1), dict(theta0=np.array([0.0, 0.5, 0.5])),
               dict(theta0=np.array([0.0, np.inf, 1.0]))):
        assert call(**kw) == -1, kw
        assert b"null context" not in lib.ibs_last_error(), kw
    # (the grid length is judged before the context too: nothing of the arrays is read)
    assert call(n=2051, ld=2051) == -3 and call(n=68, ld=68) == -3 and call(n=65) == -3


# ---- the drivers' argument rules need no GPU
def test_driver_options_are_checked_up_front():
    from tests.helpers import OracleContext, synthetic_fieldlines
    th = np.linspace(-4 * np.pi, 4 * np.pi, 67)
    mk = lambda **kw: ibs_amd.BallooningScan(OracleContext(), synthetic_fieldlines(th), th, np.array([0.5]), nalpha=3, ntheta0=3, **kw)
    assert mk().theta0_polish is False and mk().last_envelope is None
    for kw in (dict(theta0_polish=True), dict(theta0_polish=True, n_starts=2), dict(theta0_polish=True, eigenpair="nearest")):
        with pytest.raises(ValueError):
            mk(**kw)                          # (the callback path: theta0_polish=True needs tables= and device=)
    with pytest.raises(ValueError):
        mk(eigenpair="nearest").envelope()
    for K in (0, 5, 2.5, True, "2"):
        with pytest.raises(ValueError):
            mk().envelope(n_starts=K)          # (refused before anything is computed, not truncated)


# ---- the launch shape (csrc/ibs_plan.hpp), compiled for the host
PLAN_PROGRAM = r"""
#include "ibs_plan.hpp"
#include <cstdio>
int main() {
  const ibs::Chip chip{256, 160 * 1024};
  const ibs::Built built = ibs::built_full();
  const int Ns[] = {67, 131, 195, 515, 969, 2049};
  for (int N : Ns)
    for (int K = 1; K <= ibs::kTheta0PolishMaxStarts; ++K) {
      const ibs::Theta0PolishPlan p = ibs::plan_theta0_polish(chip, built, N, K);
      std::printf("%d %d %d %d %d %d\n", N, K, (int)p.err, p.M, p.threads, p.lds_rows);
    }
  const ibs::Theta0PolishPlan small = ibs::plan_theta0_polish(ibs::Chip{256, 64 * 1024}, built, 2049, 1);
  std::printf("small %d\n", (int)small.err);
  return 0;
}
"""


def test_launch_shape(tmp_path):
    """one block of K waves per line; seven staged rows, and a row per wave only where the growth-rate stage goes through LDS (M < 3)"""
    import subprocess
    src = tmp_path / "plan_check.cpp"
    src.write_text(PLAN_PROGRAM)
    exe = str(tmp_path / "plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "ideal-ballooning-solver_amd", "csrc"), str(src), "-o", exe])
    lines = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines()
    rows = [tuple(int(x) for x in ln.split()) for ln in lines[:-1]]
    assert len(rows) == 24
    for N, K, err, M, threads, lds_rows in rows:
        assert err == 0 and M == (N - 2 + 63) // 64 and threads == 64 * K and lds_rows == 7 + (K if M < 3 else 0)
        assert lds_rows * (N + (N >> 3) + 1) * 8 + 1024 <= 160 * 1024
    assert lines[-1] == "small 2"          # PlanError::NoLds: seven rows of 2,049 points do not fit 64 KB


# ---- Context.theta0_polish against its golden transcripts
def polish_cases(d):
    """[(case name, args, kwargs)] of Context.theta0_polish on the recorder's data: 2 lines x 3 theta0, N = 67"""
    head = (0.1, *d["scan7"], d["dP"], d["t0_scan"], d["gam_scan"])
    node = np.array([[1, -1], [0, 2]], dtype=np.int32)
    out = []
    for tag, kw in br._subsets(("want_lam", "want_info", "want_found")):
        out.append(("theta0_polish/" + tag, head, dict(n_starts=2, **kw)))
    out.append(("theta0_polish/defaults", head, {}))
    out.append(("theta0_polish/warm", head, dict(lam=d["lam_scan"], n_starts=4, xtol=1e-3, max_eval=7)))
    out.append(("theta0_polish/node", head, dict(node=node, n_starts=2, lam=d["lam_scan"], want_lam=True)))
    for K in (0, 5, 2.5):
        out.append(("theta0_polish/error-n_starts-%s" % K, head, dict(n_starts=K)))
    out.append(("theta0_polish/error-shape-gam", head[:-1] + (d["gam_scan"][:, :2],), {}))
    out.append(("theta0_polish/error-shape-lam", head, dict(lam=d["lam_scan"][:1])))
    out.append(("theta0_polish/error-shape-node", head, dict(node=node, n_starts=1)))
    return out


@pytest.fixture(scope="module")
def recorded():
    with br.stand_in(False) as fake:
        ctx = ibs_amd.Context(0)
        d = br.make_data(None)
        out = {name: br.run_case(ctx, fake, "theta0_polish", args, kw) for name, args, kw in polish_cases(d)}
        ctx.close()
    return out


def test_transcripts_match_the_golden(recorded):
    with open(GOLDEN) as fh:
        golden = json.load(fh)
    assert sorted(recorded) == sorted(golden) and len(golden) == 14
    bad = [k for k in sorted(golden) if recorded[k] != golden[k]]
    assert not bad, "\n".join("%s:\n  now    %s\n  golden %s" % (k, recorded[k], golden[k]) for k in bad[:5])


def test_what_the_transcripts_say(recorded):
    """independent of the golden file: one call in prototype order, the outputs' shapes, errors before any call"""
    (sym, a), = recorded["theta0_polish/node"]["calls"]
    assert sym == "ibs_theta0_polish_f64"
    assert a[:5] == ["handle", "i:2", "i:3", "i:67", "f:0.1"] and a[12] == "i:67"
    assert a[5:12] == ["in:" + k for k in "bmag gradpar cvdrift cvdrift0 gds2 gds21 gds22".split()]
    assert a[13:] == ["in:dPdrho", "in:theta0", "in:gam", "in:lam", "in:node", "i:2", "f:1e-05", "i:32", "out:theta0:(2, 2):float64",
                      "out:gam:(2, 2):float64", "out:lam:(2, 2):float64", "out:node:(2, 2):int32", "out:n_eval:(2, 2):int32", "null",
                      "out:n_found:(2,):int32", "i:1"]
    (sym, a), = recorded["theta0_polish/defaults"]["calls"]
    assert a[16:21] == ["null", "null", "i:1", "f:1e-05", "i:32"]
    errs = [k for k, v in recorded.items() if br.is_error(v["result"])]
    assert sorted(errs) == sorted(k for k in recorded if "/error-" in k) and len(errs) == 6
    assert not [k for k in errs if recorded[k]["calls"]]
    assert all(recorded[k]["result"].startswith("IbsError: ") for k in errs)


def test_the_real_library_is_back():
    assert _lib.lib().ibs_version() >= 100
