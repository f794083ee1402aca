"""CPU: the theta0 polish and the multi-start refinement of the marginal-stability scale -- ibs_marginal_theta0_polish_f64's exported
name, argument checks (all before the context) and kernel resources; the marshalling of Context.marginal_theta0_polish against
tests/golden/B6_marginal_polish_calls_host.json; BallooningScan.marginal(n_starts=K) on the two-bump surface and marginal_envelope /
marginal(theta0_polish=True) on the shifted lines, on the oracle context of tests/marginal_polish_oracle.py; the drivers' option rules."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import ibs_amd
from ibs_amd import _lib
from tests import marginal_polish_oracle as mpol
from tests import scan_peaks_cases as pc
from tests import theta0_polish_cases as tc
from tests.tools import binding_recorder as br

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ideal-ballooning-solver_amd", "csrc")
LIB = os.path.join(ROOT, "ideal-ballooning-solver_amd", "lib", "libibs_hip.so")
GOLDEN = os.path.join(ROOT, "tests", "golden", "B6_marginal_polish_calls_host.json")
NEW = "ibs_marginal_theta0_polish_f64"
XTOL = 1e-5
BIT_INF, BIT_NODE, BIT_MAXEVAL, BIT_ONE_SIDED = 1 << 8, 1 << 10, 1 << 11, 1 << 12


@pytest.mark.skipif(shutil.which("nm") is None, reason="needs nm")
def test_library_exports_the_entry_point():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert NEW in names and NEW in _lib.SYMBOLS
    assert hasattr(ibs_amd.Context, "marginal_theta0_polish") and hasattr(ibs_amd.BallooningScan, "marginal_envelope")


def test_argument_checks_come_before_the_context():
    """every check on a zeroed buffer and without a context: a refused call has read nothing and touched no device"""
    lib = _lib.lib()
    fn = getattr(lib, NEW)
    buf = np.zeros(2 * 70000)
    out = np.zeros(8)
    p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)

    def call(ctx=None, n_lines=2, n_theta0=3, N=67, h=0.1, arr=buf, ld=None, dP=buf, theta0=np.array([0.0, 0.5, 1.0]), mu=buf, K=1,
             xtol=XTOL, max_eval=32, ts=out, ms=out):
        return fn(ctx, n_lines, n_theta0, N, h, p(arr), p(buf), p(buf), p(buf), p(buf), p(buf), p(buf), N if ld is None else ld, p(dP),
                  p(theta0), p(mu), None, K, xtol, max_eval, p(ts), p(ms), None, None, None, None, None, _lib.MEM_HOST)

    assert call() == -1 and b"null context" in lib.ibs_last_error()
    for kw in (dict(arr=None), dict(dP=None), dict(theta0=None), dict(mu=None), dict(ts=None), dict(ms=None), dict(ld=66), dict(K=0),
               dict(K=5), dict(xtol=0.0), dict(xtol=-1.0), dict(xtol=float("inf")), dict(xtol=float("nan")), dict(max_eval=0),
               dict(max_eval=65), dict(n_lines=-1), dict(n_theta0=0), dict(theta0=np.array([0.0, 0.5, 0.5])),
               dict(theta0=np.array([0.0, np.inf, 1.0]))):
        assert call(**kw) == -1, kw                      # IBS_ERR_ARG
        assert b"null context" not in lib.ibs_last_error(), kw
    for bad_N in (512, 65, 65539):                       # even, below 66, above 65,537
        assert call(N=bad_N) == -3, bad_N                # IBS_ERR_UNSUPPORTED
    for good_N in (2051, 65537):                         # (no 2,050 limit: only the context is missing)
        assert call(N=good_N) == -1 and b"null context" in lib.ibs_last_error()


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")
def test_kernel_resources():
    """k_marginal_theta0_polish (csrc/ibs_marginal_polish.hip) compiles for gfx950 with no scratch, the 18,432 B of LDS of
    k_marginal_scan and at most 256 VGPRs (two waves per SIMD of 512 registers per lane); it is the file's only kernel"""
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-c", "--cuda-device-only", "-o", os.devnull,
                        "-Rpass-analysis=kernel-resource-usage", os.path.join(CSRC, "ibs_marginal_polish.hip")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"remark:\s+Function Name: (\S+)", r.stderr)
    assert len(names) == 1 and "k_marginal_theta0_polish" in names[0], names
    fig = {k: int(re.search(r"remark:\s+%s: (\d+)" % re.escape(k), r.stderr).group(1))
           for k in ("VGPRs", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]", "Occupancy [waves/SIMD]")}
    print("k_marginal_theta0_polish resources:", fig)
    assert fig["ScratchSize [bytes/lane]"] == 0 and fig["LDS Size [bytes/block]"] == 18432
    assert fig["VGPRs"] <= 256 and fig["Occupancy [waves/SIMD]"] >= 2


# ---- Context.marginal_theta0_polish against its golden transcripts
def polish_cases(d):
    """[(case name, args, kwargs)] of Context.marginal_theta0_polish on the recorder's data: 2 lines x 3 theta0, N = 67"""
    head = (0.1, *d["scan7"], d["dP"], d["t0_scan"], d["gam_scan"])
    node = np.array([[1, -1], [0, 2]], dtype=np.int32)
    out = []
    for tag, kw in br._subsets(("want_scale", "want_info", "want_found")):
        out.append(("marginal_theta0_polish/" + tag, head, dict(n_starts=2, **kw)))
    out.append(("marginal_theta0_polish/defaults", head, {}))
    out.append(("marginal_theta0_polish/short", head, dict(n_starts=4, xtol=1e-3, max_eval=7)))
    out.append(("marginal_theta0_polish/node", head, dict(node=node, n_starts=2, want_info=True)))
    for K in (0, 5, 2.5):
        out.append(("marginal_theta0_polish/error-n_starts-%s" % K, head, dict(n_starts=K)))
    out.append(("marginal_theta0_polish/error-shape-mu", head[:-1] + (d["gam_scan"][:, :2],), {}))
    out.append(("marginal_theta0_polish/error-shape-node", head, dict(node=node, n_starts=1)))
    return out


@pytest.fixture(scope="module")
def recorded():
    with br.stand_in(False) as fake:
        ctx = ibs_amd.Context(0)
        d = br.make_data(None)
        out = {name: br.run_case(ctx, fake, "marginal_theta0_polish", args, kw) for name, args, kw in polish_cases(d)}
        ctx.close()
    return out


def test_transcripts_match_the_golden(recorded):
    with open(GOLDEN) as fh:
        golden = json.load(fh)
    assert sorted(recorded) == sorted(golden) and len(golden) == 13
    bad = [k for k in sorted(golden) if recorded[k] != golden[k]]
    assert not bad, "\n".join("%s:\n  now    %s\n  golden %s" % (k, recorded[k], golden[k]) for k in bad[:5])


def test_what_the_transcripts_say(recorded):
    """independent of the golden file: one call in prototype order, the outputs' shapes, errors before any call"""
    (sym, a), = recorded["marginal_theta0_polish/node"]["calls"]
    assert sym == NEW and len(a) == len(_lib.SYMBOLS[NEW][1])
    assert a[:5] == ["handle", "i:2", "i:3", "i:67", "f:0.1"] and a[12] == "i:67"
    assert a[5:12] == ["in:" + k for k in "bmag gradpar cvdrift cvdrift0 gds2 gds21 gds22".split()]
    assert a[13:] == ["in:dPdrho", "in:theta0", "in:mu", "in:node", "i:2", "f:1e-05", "i:32", "out:theta0:(2, 2):float64",
                      "out:mu:(2, 2):float64", "out:scale:(2, 2):float64", "out:node:(2, 2):int32", "out:n_eval:(2, 2):int32",
                      "out:info:(2, 2):int32", "out:n_found:(2,):int32", "i:1"]
    (sym, a), = recorded["marginal_theta0_polish/defaults"]["calls"]
    assert a[15:20] == ["in:mu", "null", "i:1", "f:1e-05", "i:32"] and a[22:27] == ["out:scale:(2, 1):float64", "out:node:(2, 1):int32",
                                                                                   "out:n_eval:(2, 1):int32", "null", "out:n_found:(2,):int32"]
    (sym, a), = recorded["marginal_theta0_polish/plain"]["calls"]
    assert a[22] == "null" and a[25:27] == ["null", "null"]
    errs = [k for k, v in recorded.items() if br.is_error(v["result"])]
    assert sorted(errs) == sorted(k for k in recorded if "/error-" in k) and len(errs) == 5
    assert not [k for k in errs if recorded[k]["calls"]]
    assert all(recorded[k]["result"].startswith("IbsError: ") for k in errs)


def test_the_real_library_is_back():
    assert _lib.lib().ibs_version() >= 100


# ---- the multi-start refinement on the two-bump surface
N_BUMP = 131


def bump_scan():
    th = np.linspace(-4 * np.pi, 4 * np.pi, N_BUMP)
    al = pc.grids(7, 3)[0]
    ctx = mpol.MarginalPolishOracleContext()
    return ctx, ibs_amd.BallooningScan(ctx, pc.two_bump_fieldlines(th, al), th, [0.5], nalpha=7, ntheta0=3)


@pytest.fixture(scope="module")
def bump():
    ctx, scan = bump_scan()
    plain = scan.marginal(refine=True)
    n_plain = ctx.n_point_evals
    one = scan.marginal(refine=True, n_starts=1)
    assert ctx.n_point_evals == 2 * n_plain and ctx.n_polish_calls == 0
    two = scan.marginal(refine=True, n_starts=2)
    four = scan.marginal(refine=True, n_starts=4)
    return scan, plain, one, two, four


def test_two_bump_surface_second_start_finds_the_margin(bump):
    """The mu = 1 / s* table (7 x 3) has its first maximum 1.78193 at node (1, 0) and a second peak 1.64123 at node (4, 0), the lower
    flank of a narrow bump whose crest lies between nodes 4 and 5.  Measured with the oracle-backed context and the library's own
    L-BFGS-B: n_starts = 1 ends where it starts, at s* = 0.561187912615 (alpha = 0.5236, one evaluation); n_starts = 2 at s* =
    0.501216845618 (alpha = 2.356194): the single start overstates the surface's margin by 0.05997."""
    scan, plain, one, two, four = bump
    assert set(plain) == set(one) and all(np.array_equal(plain[k], one[k]) for k in plain)
    print("n_starts = 1: scale %.12f at (%.6f, %.6f) evals %s   n_starts = 2: scale %.12f at (%.6f, %.6f) evals %s candidates %r"
          % (plain["scale"][0], plain["alpha"][0], plain["theta0"][0], plain["evals"], two["scale"][0], two["alpha"][0], two["theta0"][0],
             two["evals"], two["candidates"]))
    mu = 1.0 / plain["table"][0]
    ps = ibs_amd.pick_starts(mu, scan.alpha_scan, scan.theta0_scan, 2)
    assert list(ps["index"]) == [3, 12] and abs(ps["peak"][0] - 1.78193) < 1e-5 and abs(ps["peak"][1] - 1.64123) < 1e-5
    assert two["scale"].shape == (1,) and two["scale"][0] < plain["scale"][0] - 0.05 and abs(two["alpha"][0] - 2.3562) < 1e-3
    assert abs(plain["scale"][0] - 0.561187912615) < 1e-9 and abs(two["scale"][0] - 0.501216845618) < 1e-9
    assert two["candidates"].shape == (1, 2, 3) and np.array_equal(two["n_found"], [2])
    assert np.array_equal(two["candidates"][0, 0], [plain["scale"][0], plain["alpha"][0], plain["theta0"][0]])
    assert np.array_equal(two["candidates"][0, 1], [two["scale"][0], two["alpha"][0], two["theta0"][0]])
    assert two["evals"].shape == two["task"].shape == (1, 2) and two["evals"][0, 0] == plain["evals"][0]
    assert np.array_equal(two["start"], [[scan.alpha_scan[4], scan.theta0_scan[0]]]) and two["dscale"].shape == (1, 2)
    for key in ("coarse_scale", "index", "table"):
        assert np.array_equal(two[key], plain[key]), key
    # four slots, two peaks: the padded slots copy slot 0 and nothing else changes
    assert np.array_equal(four["n_found"], [2]) and four["candidates"].shape == (1, 4, 3) and four["evals"].shape == (1, 4)
    for key in ("scale", "alpha", "theta0", "start", "dscale", "dPdrho"):
        assert np.array_equal(four[key], two[key]), key
    assert np.array_equal(four["candidates"][0, :2], two["candidates"][0]) and np.array_equal(four["evals"][0, :2], two["evals"][0])
    assert np.array_equal(four["candidates"][0, 2:], [two["candidates"][0, 0]] * 2) and np.array_equal(four["evals"][0, 2:], [two["evals"][0, 0]] * 2)


def test_padded_slots_are_not_evaluated():
    ctx, scan = bump_scan()
    scan.marginal(refine=True, n_starts=2)
    n2 = ctx.n_point_evals
    scan.marginal(refine=True, n_starts=4)
    assert ctx.n_point_evals == 2 * n2
    # without the refinement the starts are not used
    assert set(scan.marginal(n_starts=4)) == {"scale", "alpha", "theta0", "index", "table"}


def test_a_stable_table_is_not_evaluated():
    """a surface without a drive (dPdrho = 0): every mu is 0, scale = inf, no evaluation, in one slot or four"""
    th = np.linspace(-4 * np.pi, 4 * np.pi, N_BUMP)
    al = pc.grids(7, 3)[0]
    base = pc.two_bump_fieldlines(th, al)

    def stable(s, alphas):
        geo = np.array(base(s, alphas))
        geo[:, 7] = geo[:, 2]                            # gbdrift = cvdrift: dPdrho = 0
        return geo

    ctx = mpol.MarginalPolishOracleContext()
    scan = ibs_amd.BallooningScan(ctx, stable, th, [0.5], nalpha=7, ntheta0=3)
    r = scan.marginal(refine=True, n_starts=4)
    assert np.isinf(r["scale"]).all() and np.isinf(r["candidates"][:, :, 0]).all() and np.array_equal(r["n_found"], [0])
    assert not r["evals"].any() and ctx.n_point_evals == 1          # (the one final launch)


# ---- the envelope on the shifted lines
def case_scan(N, nt, case):
    """a scan of ONE line: the case's (s, alpha, phi) line whatever alpha is asked for"""
    s, alpha, phi = case
    theta = tc.case_line(N, case)[0]
    fl = tc.shifted_fieldlines(theta, phi)
    ctx = mpol.MarginalPolishOracleContext()
    return ctx, ibs_amd.BallooningScan(ctx, lambda s_, alphas: fl(s_, np.full(len(np.atleast_1d(alphas)), alpha)), theta, [s], nalpha=1,
                                       ntheta0=nt)


_ENV = {}


def envelope(nt, case):
    key = (nt, case)
    if key not in _ENV:
        ctx, scan = case_scan(131, nt, case)
        coarse = scan.marginal()
        env = scan.marginal_envelope()
        assert ctx.n_polish_calls == 1
        theta, line, dP = tc.case_line(131, case)
        low = mpol.polish(scan.h, [line[k][None] for k in range(7)], np.array([dP]), scan.theta0_scan, 1.0 / coarse["table"][0])
        _ENV[key] = scan, coarse, env, low
    return _ENV[key]


ALL = [(nt, case) for nt in tc.GRIDS for case in tc.CASES]


@pytest.mark.parametrize("nt,case", ALL)
def test_envelope_is_never_below_the_row(nt, case):
    scan, coarse, env, low = envelope(nt, case)
    row = 1.0 / coarse["table"][0, 0]
    assert env["mu"].shape == env["theta0"].shape == env["scale"].shape == env["node"].shape == env["n_eval"].shape == (1, 1, 1)
    assert env["n_found"].shape == (1, 1) and env["surface"].shape == (1, 3)
    node = int(env["node"][0, 0, 0])
    print("nt = %d case %s: mu* - node = %.3e at theta0* = %.6f (node %d at %.6f), n_eval = %d"
          % (nt, case, env["mu"][0, 0, 0] - row[node], env["theta0"][0, 0, 0], node, scan.theta0_scan[node], env["n_eval"][0, 0, 0]))
    assert node == int(np.argmax(row)) and env["mu"][0, 0, 0] >= row.max()
    assert env["scale"][0, 0, 0] <= coarse["scale"][0] and env["mu"][0, 0, 0] == 1.0 / env["scale"][0, 0, 0]
    assert np.array_equal(env["surface"][0], [env["theta0"][0, 0, 0], scan.alpha_scan[0], env["scale"][0, 0, 0]])
    assert env["n_eval"][0, 0, 0] <= 32
    for key in ("theta0", "mu", "scale", "node", "n_eval"):
        assert np.array_equal(env[key].reshape(-1), low[key].reshape(-1)), key


@pytest.mark.parametrize("nt,case", [a for a in ALL if a[1] in tc.INTERIOR])
def test_interior_crests_lie_above_the_row(nt, case):
    scan, coarse, env, low = envelope(nt, case)
    row = 1.0 / coarse["table"][0, 0]
    status = int(low["info"][0, 0]) >> 16
    assert env["mu"][0, 0, 0] > row.max() and env["theta0"][0, 0, 0] not in scan.theta0_scan
    assert not status & (BIT_NODE | BIT_MAXEVAL | BIT_INF | 3)
    lo, hi = tc.bracket(scan.theta0_scan, row, int(env["node"][0, 0, 0]))
    assert lo < env["theta0"][0, 0, 0] < hi


@pytest.mark.parametrize("nt,case", [a for a in ALL if a[1] in tc.EDGE])
def test_edge_cases_return_the_node(nt, case):
    scan, coarse, env, low = envelope(nt, case)
    row = 1.0 / coarse["table"][0, 0]
    node, status = int(env["node"][0, 0, 0]), int(low["info"][0, 0]) >> 16
    assert node in (0, nt - 1)
    assert env["theta0"][0, 0, 0] == scan.theta0_scan[node] and env["mu"][0, 0, 0] == row[node]
    assert env["scale"][0, 0, 0] == coarse["table"][0, 0, node]
    assert status & BIT_NODE and status & BIT_ONE_SIDED and not status & (BIT_MAXEVAL | BIT_INF | 3)


def test_refinement_from_the_crest():
    """marginal(theta0_polish=True): one polish call, the start is the envelope's surface point, refine=False reports it, and the refined
    scale is not above the plain run's by more than 4 u"""
    from tests import marginal_oracle as mo
    ctx, scan = case_scan(131, 5, tc.INTERIOR[0])
    plain = scan.marginal(refine=True)
    assert ctx.n_polish_calls == 0 and scan.last_marginal_envelope is None
    crest = scan.marginal(theta0_polish=True)
    env = scan.last_marginal_envelope
    assert ctx.n_polish_calls == 1 and set(crest) == {"scale", "alpha", "theta0", "index", "table"}
    assert np.array_equal(np.stack([crest["theta0"], crest["alpha"], crest["scale"]], axis=1), env["surface"])
    assert crest["scale"][0] < plain["coarse_scale"][0]
    ref = scan.marginal(refine=True, theta0_polish=True)
    assert set(ref) == set(plain) and np.array_equal(ref["start"], [[crest["alpha"][0], crest["theta0"][0]]])
    assert np.array_equal(ref["coarse_scale"], plain["coarse_scale"])
    theta, line, dP = tc.case_line(131, tc.INTERIOR[0])
    u = mo.solve(scan.h, *mo.line_gc(dP, *line[:7], ref["theta0"][0]))["u"]
    print("plain %.12f (evals %d)  from the crest %.12f (evals %d)  u %.2e" % (plain["scale"][0], plain["evals"][0], ref["scale"][0], ref["evals"][0], u))
    assert ref["scale"][0] <= plain["scale"][0] + 4 * u and ref["scale"][0] <= crest["scale"][0]


# ---- the drivers' option rules
def test_bad_option_combinations_raise():
    from tests.helpers import OracleContext
    ctx, scan = bump_scan()
    for K in (0, 17, -1, 2.0, True, None):
        with pytest.raises(ValueError):
            scan.marginal(refine=True, n_starts=K)
    with pytest.raises(ValueError):
        scan.marginal(refine=True, n_starts=2, theta0_polish=True)
    for K in (0, 5, 2.5, True, "2"):
        with pytest.raises(ValueError):
            scan.marginal_envelope(n_starts=K)
    assert ctx.n_point_evals == 0 and ctx.n_polish_calls == 0        # (refused before anything is computed)
    step = ibs_amd.AdjointStep(OracleContext(), np.linspace(-4 * np.pi, 4 * np.pi, N_BUMP), [0.5], "cpu")
    for kw in (dict(n_starts=0), dict(n_starts=17), dict(n_starts=2.0), dict(n_starts=2, theta0_polish=True)):
        with pytest.raises(ValueError):
            step.marginal([], **kw)
