"""CPU: the multi-start refinement's host layer -- ibs_amd.pick_starts (the rule in numpy) on hand-written tables and against
pick_start; the bookkeeping of csrc/ibs_scan_peaks.hpp, compiled for the host, against pick_starts on random tables; the argument
checks of ibs_scan_peaks_f64; the marshalling of Context.scan_peaks against tests/golden/B4_scan_peaks_calls_host.json (transcripts of
the recorder's stand-in library: tests/tools/binding_recorder.py); and BallooningScan / AdjointStep with n_starts on the oracle-backed
context, on a surface whose coarse table ranks the basin of its maximum second."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import ibs_amd
from ibs_amd import _lib
from tests import scan_peaks_cases as pc
from tests.helpers import OracleContext
from tests.test_cabi import header_prototypes
from tests.tools import binding_recorder as br

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ideal-ballooning-solver_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "B4_scan_peaks_calls_host.json")
P, I32 = C.c_void_p, C.c_int32


def picks(tab, K):
    al, t0 = pc.grids(*tab.shape)
    return ibs_amd.pick_starts(tab, al, t0, K), al, t0


# ---- the rule on hand-written tables
def test_single_peak_in_a_corner_pads_with_slot_0():
    r, al, t0 = picks(pc.hand_tables()["corner"], 5)
    assert r["n_found"] == 1 and r["n_bad"] == 0
    assert np.array_equal(r["index"], [0] * 5) and np.array_equal(r["peak"], [5.0] * 5)
    assert np.array_equal(r["start"], [[al[0], t0[0]]] * 5) and np.array_equal(r["sigma0"], [1.3 * 5.0 + 0.05] * 5)


def test_the_first_index_of_a_plateau_is_its_only_peak():
    r, al, t0 = picks(pc.hand_tables()["plateau"], 5)
    # the plateau of twos: (1, 1) = index 6; the plateau of ones: (2, 4) = index 14; no other entry is a peak (the zeros touch a
    # higher entry or an equal one of lower index; index 0 is beaten by the 2 at (1, 1))
    assert r["n_found"] == 2 and np.array_equal(r["index"], [6, 14, 6, 6, 6]) and np.array_equal(r["peak"], [2.0, 1.0, 2.0, 2.0, 2.0])
    assert np.array_equal(r["start"][1], [al[2], t0[4]])


def test_equal_separated_peaks_come_in_index_order():
    r, al, t0 = picks(pc.hand_tables()["equal"], 5)
    # three peaks of 0.5 at indices 0, 10, 26; the -1 entries form a plateau whose first index (1) touches index 0: no peak
    assert r["n_found"] == 3 and np.array_equal(r["index"], [0, 10, 26, 0, 0]) and np.array_equal(r["peak"], [0.5] * 5)
    assert np.array_equal(r["start"][2], [al[3], t0[5]])
    two = picks(pc.hand_tables()["equal"], 2)[0]
    assert two["n_found"] == 2 and np.array_equal(two["index"], [0, 10])


def test_nan_entries_are_no_peaks_and_beat_nothing():
    r, al, t0 = picks(pc.hand_tables()["nan"], 16)
    # the finite entries walled in by NaN are peaks -- 4 (index 13), 3 (2), 1 (0), 0.5 (11); the 2 (index 8) touches the 4 diagonally
    assert r["n_found"] == 4 and r["n_bad"] == 0
    assert np.array_equal(r["index"], [13, 2, 0, 11] + [13] * 12)
    assert np.array_equal(r["peak"][:4], [4.0, 3.0, 1.0, 0.5]) and np.isfinite(r["sigma0"]).all()


def test_all_zero_all_nan_and_thin_tables():
    t = pc.hand_tables()
    r = picks(t["zero"], 5)[0]
    assert r["n_found"] == 0 and r["n_bad"] == 0 and np.array_equal(r["start"], np.zeros((5, 2)))
    assert np.array_equal(r["sigma0"], [0.05] * 5) and np.array_equal(r["index"], [-1] * 5) and np.array_equal(r["peak"], [0.0] * 5)
    r = picks(t["all_nan"], 5)[0]
    assert r["n_found"] == 0 and r["n_bad"] == 1 and np.array_equal(r["start"], np.zeros((5, 2)))
    assert np.array_equal(r["sigma0"], [0.05] * 5) and np.isnan(r["peak"]).all() and np.array_equal(r["index"], [-1] * 5)
    inf = np.array([[1.0, np.inf], [0.0, 2.0]])
    r = picks(inf, 2)[0]
    assert r["n_found"] == 0 and r["n_bad"] == 1 and np.array_equal(r["start"], np.zeros((2, 2)))
    r, al, t0 = picks(t["1xn"], 5)          # 1 3 2 2 5 5 0: peaks 5 (index 4; index 5 is beaten by it) and 3 (index 1)
    assert r["n_found"] == 2 and np.array_equal(r["index"], [4, 1, 4, 4, 4]) and np.array_equal(r["start"][1], [al[0], t0[1]])
    r, al, t0 = picks(t["nx1"], 5)          # 2 1 1 3 -1 0: peaks 3 (3), 2 (0), 0 (5)
    assert r["n_found"] == 3 and np.array_equal(r["index"], [3, 0, 5, 3, 3]) and np.array_equal(r["start"][2], [al[5], t0[0]])
    assert np.array_equal(r["sigma0"][:3], [1.3 * 3.0 + 0.05, 1.3 * 2.0 + 0.05, 0.05])
    r = picks(t["1x1"], 2)[0]
    assert r["n_found"] == 1 and np.array_equal(r["index"], [0, 0]) and np.array_equal(r["start"], np.zeros((2, 2)))
    assert picks(t["1x1_zero"], 2)[0]["n_found"] == 0


@pytest.mark.parametrize("K", pc.STARTS)
def test_slot_0_is_pick_start(K):
    for name, tab in pc.hand_tables().items():
        r, al, t0 = picks(tab, K)
        assert r["start"].shape == (K, 2) and r["peak"].shape == r["sigma0"].shape == r["index"].shape == (K,), name
        if not np.all(np.isfinite(tab)):
            with pytest.raises(ibs_amd.IbsError):
                ibs_amd.pick_start(tab, al, t0)
            continue
        a0, th0, sg, ij = ibs_amd.pick_start(tab, al, t0)
        assert (r["start"][0, 0], r["start"][0, 1], r["sigma0"][0]) == (a0, th0, sg), name
        assert r["index"][0] == (-1 if ij is None else ij[0] * tab.shape[1] + ij[1]) and r["peak"][0] == tab.max(), name
    rng = np.random.default_rng(5)
    for _ in range(20):
        tab = rng.normal(size=(6, 5))
        r, al, t0 = picks(tab, K)
        a0, th0, sg, ij = ibs_amd.pick_start(tab, al, t0)
        assert (r["start"][0, 0], r["start"][0, 1], r["sigma0"][0], r["index"][0]) == (a0, th0, sg, ij[0] * 5 + ij[1])
        assert (np.diff(r["peak"][:r["n_found"]]) <= 0).all() and len(set(r["index"][:r["n_found"]])) == r["n_found"]


# ---- the header's bookkeeping, compiled for the host
PROGRAM = r"""
#include <cstdio>
#include <vector>
#include "ibs_scan_peaks.hpp"

// one table per line: K n_alpha n_theta0, alpha, theta0 and the table (hex floats) ->
//   "n_found n_bad" and per slot "alpha theta0 peak index sigma0"
int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::FILE* fh = std::fopen(argv[1], "r");
  if (!fh) return 2;
  int K, na, nt;
  while (std::fscanf(fh, "%d %d %d", &K, &na, &nt) == 3) {
    std::vector<double> al(na), t0(nt), tab((size_t)na * nt);
    for (double& v : al) if (std::fscanf(fh, "%la", &v) != 1) return 2;
    for (double& v : t0) if (std::fscanf(fh, "%la", &v) != 1) return 2;
    for (double& v : tab) if (std::fscanf(fh, "%la", &v) != 1) return 2;
    double pv[ibs::kMaxStarts];
    int pi[ibs::kMaxStarts];
    const int n_picks = ibs::peaks_select_serial(tab.data(), na, nt, K, pv, pi);
    std::vector<double> start(2 * K), peak(K), sigma0(K);
    std::vector<int> index(K);
    int n_found = -1;
    const bool bad = ibs::peaks_finish(K, n_picks, pv, pi, na, nt, al.data(), t0.data(), start.data(), peak.data(), index.data(),
                                       sigma0.data(), &n_found);
    std::printf("%d %d", n_found, bad ? 1 : 0);
    for (int k = 0; k < K; ++k) std::printf(" %a %a %a %d %a", start[2 * k], start[2 * k + 1], peak[k], index[k], sigma0[k]);
    std::printf("\n");
  }
  std::fclose(fh);
  return 0;
}
"""


def hexs(values):
    return " ".join(float(v).hex() for v in np.ravel(values))


def bookkeeping_tables():
    """200 random tables: normal values and integers 0 .. 3, four shapes, K in turn; then the hand-written ones"""
    out = []
    shapes = ((7, 9), (8, 8), (5, 13), (24, 15))
    for k in range(200):
        na, nt = shapes[k % 4]
        out.append((pc.STARTS[(k // 4) % 4], pc.family("ints" if (k // 16) % 2 else "normal", 1, na, nt, 1000 + k)[0]))
    for tab in pc.hand_tables().values():
        out += [(K, tab) for K in pc.STARTS]
    return out


@pytest.fixture(scope="module")
def host_rows(tmp_path_factory):
    d = tmp_path_factory.mktemp("scan_peaks_bookkeeping")
    src = d / "peaks_check.cpp"
    src.write_text(PROGRAM)
    cases = bookkeeping_tables()
    inp = d / "tables.txt"
    inp.write_text("".join("%d %d %d %s %s %s\n" % (K, *tab.shape, hexs(pc.grids(*tab.shape)[0]), hexs(pc.grids(*tab.shape)[1]), hexs(tab))
                           for K, tab in cases))
    rows = {}
    for tag, flags in (("plain", ["-O1"]), ("san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                                   "-static-libasan", "-static-libubsan"])):
        exe = str(d / ("peaks_check_" + tag))
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I", CSRC, str(src), "-o", exe])
        p = subprocess.run([exe, str(inp)], capture_output=True, text=True)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
        rows[tag] = [ln.split() for ln in p.stdout.splitlines()]
    return cases, rows


def test_host_bookkeeping_equals_pick_starts(host_rows):
    cases, rows = host_rows
    assert len(rows["plain"]) == len(cases) >= 200
    n_multi = 0
    for (K, tab), row in zip(cases, rows["plain"]):
        r = picks(tab, K)[0]
        assert (int(row[0]), int(row[1])) == (r["n_found"], r["n_bad"]), (K, tab)
        f = lambda k: np.array([float.fromhex(x) for x in row[2 + k::5]])
        start = np.stack([f(0), f(1)], axis=1)
        assert np.array_equal(pc.bits(start), pc.bits(r["start"])) and np.array_equal(pc.bits(f(2)), pc.bits(r["peak"])), (K, tab)
        assert np.array_equal(np.array([int(x) for x in row[5::5]]), r["index"]) and np.array_equal(pc.bits(f(4)), pc.bits(r["sigma0"]))
        n_multi += r["n_found"] > 1
    assert n_multi > 100          # (the tables do have several peaks)


def test_the_same_program_under_address_and_ub_sanitizers(host_rows):
    assert host_rows[1]["san"] == host_rows[1]["plain"]


# ---- the entry point: header, library, symbol table, argument checks
def test_entry_point_and_its_argument_checks():
    row = [P, I32, I32, I32, I32, P, P, P, P, P, P, P, P, P, I32]
    protos = header_prototypes()
    lib = _lib.lib()
    name = "ibs_scan_peaks_f64"
    assert _lib.SYMBOLS[name] == (C.c_int, row)
    assert hasattr(lib, name) and name in protos and len(protos[name][1]) == len(row)
    assert ibs_amd.MAX_STARTS == 16
    txt = open(os.path.join(ROOT, "include", "ibs.h")).read()
    assert "ball_scan.py:279-295" in txt[txt.index("The n_starts best local maxima"):txt.index("int ibs_scan_peaks_f64")]
    ctx = C.create_string_buffer(4096)           # zeroed: a call that touched it as a context would not return -1
    al, t0 = pc.grids(3, 2)
    gam = np.zeros((1, 3, 2)); start = np.zeros((1, 2, 2)); peak = np.zeros((1, 2)); n_bad = np.zeros(1, dtype=np.int32)
    p = lambda a: a.ctypes.data
    good = [1, 3, 2, 2, p(al), p(t0), p(gam), p(start), p(peak), None, None, None, p(n_bad), 1]

    def call(**kw):
        a = list(good)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return lib.ibs_scan_peaks_f64(ctx, *a)
    for kw in (dict(a3=0), dict(a3=17), dict(a3=-1), dict(a1=0), dict(a2=0), dict(a0=-1), dict(a6=None), dict(a7=None), dict(a8=None),
               dict(a12=None), dict(a4=None), dict(a5=None)):
        assert call(**kw) == -1, kw
        assert b"bad arguments" in lib.ibs_last_error()
    assert lib.ibs_scan_peaks_f64(None, *good) == -1 and b"null" in lib.ibs_last_error()
    assert ctx.raw == bytes(4096) and n_bad[0] == 0


# ---- the binding
def peaks_cases(d):
    """[(case name, args, kwargs, in-out names)] of Context.scan_peaks on the recorder's data: 3 surfaces of a 2 x 3 table"""
    al, t0, gam = d["alpha_scan"], d["t0_scan"], d["gam_surf"].reshape(3, 2, 3)
    out = []
    for tag, kw in br._subsets(("want_sigma0", "want_index", "want_found")):
        out.append(("scan_peaks/" + tag, (al, t0, gam, 2), kw, ()))
    out.append(("scan_peaks/n_bad", (al, t0, gam, 3), dict(n_bad=d["n_bad"], want_found=True), ("n_bad",)))
    out.append(("scan_peaks/one", (al, t0, gam, 1), {}, ()))
    out.append(("scan_peaks/sixteen", (al, t0, gam, 16), dict(want_index=True), ()))
    for K in (0, 17, 2.5, True, "3"):
        out.append(("scan_peaks/error-n_starts-%s" % K, (al, t0, gam, K), {}, ()))
    out.append(("scan_peaks/error-shape-2d", (al, t0, d["gam_surf"], 2), {}, ()))
    out.append(("scan_peaks/error-shape-grid", (al, t0[:2], gam, 2), {}, ()))
    out.append(("scan_peaks/error-n_bad-dtype", (al, t0, gam, 2), dict(n_bad=np.zeros(1)), ("n_bad",)))
    return out


def record():
    with br.stand_in(False) as fake:
        ctx = ibs_amd.Context(0)
        d = br.make_data(None)
        out = {name: br.run_case(ctx, fake, "scan_peaks", args, kw, inout) for name, args, kw, inout in peaks_cases(d)}
        ctx.close()
    return out


@pytest.fixture(scope="module")
def recorded():
    return record()


def test_transcripts_match_the_golden(recorded):
    with open(GOLDEN) as fh:
        golden = json.load(fh)
    assert sorted(recorded) == sorted(golden) and len(golden) == 16
    bad = [k for k in sorted(golden) if recorded[k] != golden[k]]
    assert not bad, "\n".join("%s:\n  now    %s\n  golden %s" % (k, recorded[k], golden[k]) for k in bad[:5])


def test_what_the_transcripts_say(recorded):
    """independent of the golden file: one call in prototype order, the outputs' shapes, n_bad made or passed through"""
    (sym, a), = recorded["scan_peaks/want_sigma0-want_index-want_found"]["calls"]
    assert sym == "ibs_scan_peaks_f64"
    assert a == ["handle", "i:3", "i:2", "i:3", "i:2", "in:alpha_scan", "in:theta0_scan", "in:gam", "out:start:(3, 2, 2):float64",
                 "out:peak:(3, 2):float64", "out:index:(3, 2):int32", "out:sigma0:(3, 2):float64", "out:n_found:(3,):int32",
                 "out:n_bad:(1,):int32", "i:1"]
    (sym, a), = recorded["scan_peaks/plain"]["calls"]
    assert a[10:13] == ["null"] * 3
    (sym, a), = recorded["scan_peaks/n_bad"]["calls"]
    assert a[4] == "i:3" and a[13] == "inout:n_bad" and a[12] == "out:n_found:(3,):int32"
    errs = [k for k, v in recorded.items() if br.is_error(v["result"])]
    assert sorted(errs) == sorted(k for k in recorded if "/error-" in k) and len(errs) == 8
    assert not [k for k in errs if recorded[k]["calls"]]
    for k in errs:
        assert recorded[k]["result"].startswith("IbsError: "), recorded[k]
        if "error-n_starts" in k:
            assert recorded[k]["result"].startswith("IbsError: n_starts must be an integer in [1, 16]"), recorded[k]


# ---- the drivers
N_BUMP = 131


def bump_scan(**kw):
    th = np.linspace(-4 * np.pi, 4 * np.pi, N_BUMP)
    al = pc.grids(7, 3)[0]
    return ibs_amd.BallooningScan(OracleContext(), pc.two_bump_fieldlines(th, al), th, [0.5], nalpha=7, ntheta0=3, **kw)


def test_two_bump_surface_second_start_finds_the_maximum():
    """The coarse 7 x 3 table has its first maximum 0.375214088834 at node (1, 0) and a second peak 0.305869936 at node (4, 0), the
    lower flank of a narrow bump whose crest lies between nodes 4 and 5.  Measured with the oracle-backed context: n_starts = 1 ends
    at gam = 0.3752140888342 (alpha = 0.5236), n_starts = 2 at gam = 0.4715516281942 (alpha = 2.356194): the single start
    under-reports the surface's growth rate by 0.0963375."""
    plain = bump_scan()
    r0 = plain.local_rows()
    one = bump_scan(n_starts=1)
    r1 = one.local_rows()
    assert np.array_equal(r0, r1) and one.last_candidates is None and one.last_peaks is None
    two = bump_scan(n_starts=2)
    r2 = two.local_rows()
    print("n_starts = 1: %r   n_starts = 2: %r" % (r1, r2))
    assert r2.shape == (1, 3) and r2[0, 2] > r1[0, 2] + 0.05 and abs(r2[0, 1] - 2.3562) < 1e-3
    assert abs(r1[0, 2] - 0.375214088834) < 1e-9 and abs(r2[0, 2] - 0.471551628194) < 1e-9
    assert np.array_equal(two.last_peaks["index"], [[3, 12]]) and np.array_equal(two.last_peaks["n_found"], [2])
    assert two.last_candidates.shape == (1, 2, 3) and np.array_equal(two.last_candidates[0, 0], r1[0])
    assert np.array_equal(two.last_candidates[0, 1], r2[0])
    four = bump_scan(n_starts=4)
    r4 = four.local_rows()
    assert np.array_equal(four.last_peaks["n_found"], [2]) and np.array_equal(r4, r2)
    assert np.array_equal(four.last_peaks["index"], [[3, 12, 3, 3]]) and np.array_equal(four.last_candidates[0, 2:], [r1[0], r1[0]])
    # without the refinement the rows are slot 0's: those of one start
    assert np.array_equal(bump_scan(n_starts=4).local_rows(refine=False), bump_scan().local_rows(refine=False))
    # run() gathers the same rows
    t, a, g = bump_scan(n_starts=2).run()
    assert np.array_equal(np.stack([t, a, g], axis=1), r2)


@pytest.mark.parametrize("K", (0, 17, -1, 2.0, True, None))
def test_bad_n_starts_raise_on_both_drivers(K):
    with pytest.raises(ValueError):
        bump_scan(n_starts=K)
    with pytest.raises(ValueError):
        ibs_amd.AdjointStep(OracleContext(), np.linspace(-4 * np.pi, 4 * np.pi, N_BUMP), [0.5], "cpu", n_starts=K)


def test_refine_batched_keeps_its_default():
    import inspect
    sig = inspect.signature(ibs_amd.BallooningScan.refine_batched)
    assert sig.parameters["surf_idx"].default is None and list(sig.parameters)[-1] == "surf_idx"
    assert inspect.signature(ibs_amd.BallooningScan.__init__).parameters["n_starts"].default == 1
    assert inspect.signature(ibs_amd.AdjointStep.__init__).parameters["n_starts"].default == 1
