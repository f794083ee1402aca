"""GPU: every form of the raw (g, c, f) entry points and of the geometry-fed scan with the twist row of the eigenvector stage on the
lane edges of the register kernels, against the CPU oracles (tests/edge_cases.py: lane_targets; pinned with the oracles alone in
tests/test_edge_cases_cpu.py).

Lane L of a P-lane form owns the rows [rows_start(L), rows_start(L + 1)) (csrc/ibs_wave.hpp, csrc/ibs_group.hpp): rem lanes of M rows,
then lanes of M - 1; the forward and backward solutions cross lanes through a DPP scan whose steps change at lanes 16, 32 and 48.  The
batch of a call is the moving well at every lane-edge target of the form under test (8 ... 14 systems: the blocks of four waves have
spare waves), so twisted(), assemble(), finish_chunk and the X / dX stores meet a mode on the first and the last row of a lane, on the
lane where the chunk length drops, and on the DPP row edges, in every rows-per-lane instantiation of every form -- the big-batch
forms (rows straight from global memory, sub-wave, all-FP32 eigenvalues) included, which a small batch reaches through the options
gcf_direct, force_p and f32_lam.

Bounds: none is new, none was taken from a run.
 (a) FP64 rows against bo.solve_gcf: check_pair of tests/test_gpu_edge_lengths.py -- lam 4 N eps ||A|| (test_gpu_configs.py:
     test_config5_fp64_one_million_systems), gam 1e-10, X 1e-7, dX 1e-7 max|dX| + 1e-7 (test_gpu_parity.py:
     test_every_rows_per_lane_instantiation).
 (b) FP32 rows with a growth rate against co.solve_gcf on the FP32 values widened, with the h the kernel sees: these kernels widen
     exactly as they read, solve in FP64 and convert every output ONCE, at its store (csrc/ibs_kernels.hip: finish, finish_chunk:
     (TO)X, (TO)dX, (TO)gam, (TO)lam; csrc/ibs_kernels_group.hip: (TO)lam, (TO)gam, (TO)Xs[..]): the bound of (a) plus one rounding
     to float32, 2^-24 |reference value|, per quantity.  No form rounds twice: X and dX pass through LDS in FP64.
 (c) FP32 eigenvalues alone against co.lam_batch on the widened values: (N + 3) eps32 ||A||, the solver's stated certificate
     (test_gpu_round5.py: test_fp32_eigenvalues_alone_on_short_grids), eps32 = 2^-23; status: informational bits 2 and 3 only.
 (d) the geometry-fed scan on the mapped well against bo.solve_gcf: check_pair, as test_geometry_fed_scan_on_long_edges."""
import numpy as np
import pytest

from oracle import ballooning_oracle as bo
from oracle import c_oracle as co
from tests import edge_cases as ec
from tests.test_gpu_edge_lengths import check_pair, clean, note, tol_dX, tol_gam, tol_X, up_to_sign, well_batch

pytestmark = pytest.mark.gpu

EPS = ec.EPS
EPS32 = 2.0 ** -23           # (1.1920929e-07 of test_gpu_round5.py)
U32 = 2.0 ** -24             # one rounding to float32, relative
SHORT = ec.EDGE_N_SHORT


@pytest.fixture(scope="module")
def ctx():
    import ibs_amd
    c = ibs_amd.Context(0)
    yield c
    c.close()


_REFS = {}


def reference(N, j, fp32=False):
    """(rows (g, c, f), the oracle's (gam, lam, X, dX), ||A||) of the moving well at j, computed once per (N, j) and left unchanged:
    FP64 rows with bo.solve_gcf; fp32: the rows rounded to float32 and widened, h = float(float32(h)), with co.solve_gcf"""
    key = (N, j, fp32)
    if key not in _REFS:
        th = ec.theta_grid(N)
        h = float(th[1] - th[0])
        rows = ec.well_rows(th, j)
        if fp32:
            h32, _, rows, _ = ec.fp32_inputs(h, *rows)
            ref = co.solve_gcf(h32, *rows)
            nA = ec.norm_a(h32, *rows)[0]
        else:
            ref = bo.solve_gcf(th, *rows)
            nA = ec.norm_a(h, *rows)[0]
        for a in ref[2:]:
            a.setflags(write=False)
        _REFS[key] = (rows, ref, nA)
    return _REFS[key]


def peak_on_target(N, tag, j, X):
    kk = int(np.argmax(np.abs(np.asarray(X, dtype=np.float64))))
    assert (min(kk, N - 1 - kk) <= 6) if ec.is_end_target(N, j) else (kk == j), (N, tag, j, kk)


def figures(N, tag, errs, lam_unit="N eps ||A||"):
    """one line per (form, N): the worst of each quantity over the systems of the call, before anything is held to its bound"""
    w = [max(e[i] for e in errs) for i in range(4)]
    print("edge-case figures: lane edges N=%d %s (%d systems)  |dlam| = %.3f %s  |dgam| = %.1e  |dX| = %.1e  |ddX| = %.1e"
          % (N, tag, len(errs), w[0], lam_unit, w[1], w[2], w[3]))


def errors(N, lam, gam, X, dX, ref, nA):
    gam_o, lam_o, X_o, dX_o = ref
    e = [abs(float(lam) - lam_o) / (N * EPS * nA), abs(float(gam) - gam_o) if gam is not None else 0.0, 0.0, 0.0]
    if X is not None:
        X, dX = np.asarray(X, dtype=np.float64), np.asarray(dX, dtype=np.float64)
        s = up_to_sign(X, X_o)
        e[2], e[3] = float(np.abs(s * X - X_o).max()), float(np.abs(s * dX - dX_o).max())
    return e


def check_fp64(N, tag, targets, r, want_gam=True, want_X=True, col=None):
    """a call on FP64 rows against the oracle; col: the theta0 column of a scan's (n_lines, n_theta0[, N]) outputs"""
    pick = (lambda a, k: a[k]) if col is None else (lambda a, k: a[k, col])
    refs = [reference(N, j) for j in targets]
    errs = [errors(N, pick(r["lam"], k), pick(r["gam"], k) if want_gam else None, pick(r["X"], k) if want_X else None,
                   pick(r["dX"], k) if want_X else None, refs[k][1], refs[k][2]) for k in range(len(targets))]
    figures(N, tag, errs)
    for k, j in enumerate(targets):
        _, ref, nA = refs[k]
        if want_X:
            check_pair(N, "%s well at %d" % (tag, j), pick(r["lam"], k), pick(r["gam"], k), pick(r["X"], k), pick(r["dX"], k), ref, nA)
            peak_on_target(N, tag, j, pick(r["X"], k))
        else:
            assert errs[k][0] <= 4.0, (N, tag, j, "lam", errs[k][0])
            assert errs[k][1] < tol_gam(N), (N, tag, j, "gam", errs[k][1])


def check_fp32(N, tag, targets, r):
    """(b): FP32 outputs of the FP64 solver against the C oracle on the widened values: the bound of check_pair plus one rounding to
    float32 of the reference value, per quantity and per entry"""
    refs = [reference(N, j, fp32=True) for j in targets]
    for key in ("lam", "gam", "X", "dX"):
        assert r[key].dtype == np.float32, (N, tag, key)
    errs = [errors(N, r["lam"][k], r["gam"][k], r["X"][k], r["dX"][k], refs[k][1], refs[k][2]) for k in range(len(targets))]
    for e, (_, ref, nA) in zip(errs, refs):           # (lam of an FP32 output: as a fraction of its bound, N eps ||A|| says nothing here)
        e[0] *= N * EPS * nA / (4 * N * EPS * nA + U32 * abs(ref[1]))
    figures(N, tag, errs, lam_unit="of 4 N eps ||A|| + 2^-24 |lam|")
    for k, j in enumerate(targets):
        _, (gam_o, lam_o, X_o, dX_o), nA = refs[k]
        X, dX = r["X"][k].astype(np.float64), r["dX"][k].astype(np.float64)
        s = up_to_sign(X, X_o)
        assert abs(float(r["lam"][k]) - lam_o) <= 4 * N * EPS * nA + U32 * abs(lam_o), (N, tag, j, "lam", errs[k][0])
        assert abs(float(r["gam"][k]) - gam_o) < tol_gam(N) + U32 * abs(gam_o), (N, tag, j, "gam", errs[k][1])
        assert (np.abs(s * X - X_o) < tol_X(N) + U32 * np.abs(X_o)).all(), (N, tag, j, "X", errs[k][2])
        assert (np.abs(s * dX - dX_o) < tol_dX(N, dX_o) + U32 * np.abs(dX_o)).all(), (N, tag, j, "dX", errs[k][3])
        assert np.abs(X).max() == 1.0 and X[0] == 0.0 and X[-1] == 0.0, (N, tag, j)
        peak_on_target(N, tag, j, X)


def staged_name(N, fp32=False):
    """the small-batch kernel of ibs_solve_gcf_f64 / ibs_solve_gcf_f32 with a growth rate (csrc/ibs_plan.hpp: plan_gcf)"""
    M = ec.rows_per_lane(N)
    if fp32:
        return "ibs::k_solve_gcf_rows<double, %d, float>" % M if M >= 24 else "ibs::k_solve_gcf_wide<%d>" % M
    return "ibs::k_solve_gcf_rows<double, %d, double>" % M if M >= 24 else "ibs::k_solve_gcf<double, %d>" % M


def direct_name(N, fp32=False):
    """gcf_direct = 1: rows straight from global memory from 9 rows per lane on (IBS_DIRECT_MIN_M), capped to two waves per SIMD for
    M = 21 ... 28 (FP64 rows) / 21 ... 30 (FP32 rows) (direct_two_waves); below 9 rows the staged kernel runs, silently"""
    M = ec.rows_per_lane(N)
    if M < 9:
        return staged_name(N, fp32)
    w2 = 21 <= M <= (30 if fp32 else 28)
    return "ibs::k_solve_gcf_direct%s<double, %d, %s>" % ("_w2" if w2 else "", M, "float" if fp32 else "double")


def forms_of(N, fp32=False):
    """[(tag, options, kernel name, lanes per system)] of the raw solve with a growth rate"""
    t = "float" if fp32 else "double"
    out = [("default", {}, staged_name(N, fp32), 64), ("gcf_direct=1", {"gcf_direct": 1}, direct_name(N, fp32), 64)]
    for P in ec.lanes_allowed(N):
        out.append(("force_p=%d" % P, {"force_p": P}, "ibs::k_solve_gcf_g<double, %d, %d, %s>" % ((N - 2 + P - 1) // P, P, t), P))
    return out


def run_with(ctx, opts, call):
    """call() under the options, every one of them back at the context's default afterwards; (result, kernel name)"""
    try:
        for k, v in opts.items():
            ctx.set_option(k, v)
        r = call()
        return r, ctx.last_launch()[0]
    finally:
        for k in opts:
            ctx.set_option(k, None)


# ------------------------------------------------------------------------------------------------ (a) FP64 rows
@pytest.mark.parametrize("N", SHORT)
def test_fp64_rows_on_lane_edges(ctx, N):
    """ibs_solve_gcf_f64 in the small-batch form, with the rows read straight from global memory (k_solve_gcf_direct / _direct_w2; below
    9 rows per lane the staged kernel, whose name pins the silent fallback) and in the 32- / 16-lane forms on their own targets;
    each with X / dX, without them, and eigenvalues alone"""
    for tag, opts, name, P in forms_of(N):
        targets = ec.lane_targets(N, P)
        th, (g, c, f) = well_batch(N, targets)
        h = float(th[1] - th[0])
        for way, kw in (("X", dict(want_X=True)), ("gam", dict()), ("lam", dict(want_gam=False))):
            r, got = run_with(ctx, opts, lambda: ctx.solve_gcf(h, g, c, f, want_info=True, **kw))
            assert got == name, (N, tag, way, got, name)
            note("solve_gcf_f64 %s, %s (%d targets)" % (tag, way, len(targets)), N, name=got)
            assert r["nbad"] == 0, (N, tag, way)
            clean(r["info"], N)
            check_fp64(N, "f64 %s, %s" % (tag, way), targets, r, want_gam=way != "lam", want_X=way == "X")


# ------------------------------------------------------------------------------------------------ (b) FP32 rows, growth rate
@pytest.mark.parametrize("N", SHORT)
def test_fp32_rows_with_a_growth_rate_on_lane_edges(ctx, N):
    """ibs_solve_gcf_f32 with gam, X and dX -- FP32 in memory, FP64 in the solver -- in the small-batch form (k_solve_gcf_wide,
    k_solve_gcf_rows<double, M, float> from 24 rows on), with the rows from global memory (k_solve_gcf_direct[_w2]<double, M, float>)
    and in the sub-wave forms (k_solve_gcf_g<double, Mg, P, float>), against the C oracle on the same FP32 values"""
    for tag, opts, name, P in forms_of(N, fp32=True):
        targets = ec.lane_targets(N, P)
        th, rows = well_batch(N, targets)
        h = float(th[1] - th[0])
        _, (g32, c32, f32), _, _ = ec.fp32_inputs(h, *rows)
        r, got = run_with(ctx, opts, lambda: ctx.solve_gcf(h, g32, c32, f32, want_X=True, want_info=True, dtype=np.float32))
        assert got == name, (N, tag, got, name)
        note("solve_gcf_f32 %s (%d targets)" % (tag, len(targets)), N, name=got)
        assert r["nbad"] == 0, (N, tag)
        clean(r["info"], N)
        check_fp32(N, "f32 rows %s" % tag, targets, r)


# ------------------------------------------------------------------------------------------------ (c) FP32 eigenvalues alone
@pytest.mark.parametrize("N", SHORT)
def test_fp32_eigenvalues_alone_on_lane_edges(ctx, N):
    """ibs_solve_gcf_f32 without gam: the all-FP32 iteration with its FP64 certificate, staged (k_solve_gcf<float, M>) and with the rows
    from global memory (f32_lam = 1 and gcf_direct = 1: k_solve_gcf_f32lam_direct, _w2 for M = 21 ... 30; at M = 2 the staged kernel,
    name asserted), against co.lam_batch on the widened FP32 values with the kernel's h"""
    M = ec.rows_per_lane(N)
    targets = ec.lane_targets(N)
    th, rows = well_batch(N, targets)
    h = float(th[1] - th[0])
    h32, (g32, c32, f32), wide, _ = ec.fp32_inputs(h, *rows)
    lam_o = co.lam_batch(h32, *wide)
    nA = ec.norm_a(h32, *wide)
    staged = "ibs::k_solve_gcf<float, %d>" % M
    direct = staged if M < 3 else "ibs::k_solve_gcf_f32lam_direct%s<%d>" % ("_w2" if 21 <= M <= 30 else "", M)
    for tag, opts, name in (("default", {}, staged), ("f32_lam=1 gcf_direct=1", {"f32_lam": 1, "gcf_direct": 1}, direct)):
        r, got = run_with(ctx, opts, lambda: ctx.solve_gcf(h, g32, c32, f32, want_info=True, dtype=np.float32, want_gam=False))
        assert got == name, (N, tag, got, name)
        note("solve_gcf_f32 eigenvalues alone, %s (%d targets)" % (tag, len(targets)), N, name=got)
        assert r["lam"].dtype == np.float32 and r["nbad"] == 0, (N, tag)
        st = np.asarray(r["info"]) >> 16
        assert ((st & ~(4 | 8)) == 0).all(), (N, tag, st)
        e = np.abs(r["lam"].astype(np.float64) - lam_o) / (EPS32 * nA)
        print("edge-case figures: lane edges N=%d f32 lam %s (%d systems)  |dlam| = %.3f eps32 ||A|| (bound %d)  status bits %s"
              % (N, tag, len(targets), e.max(), N + 3, sorted(set(int(s) for s in st))))
        assert (e <= N + 3).all(), (N, tag, e.max())


# ------------------------------------------------------------------------------------------------ (d) geometry-fed scan
@pytest.mark.parametrize("N", SHORT)
def test_geometry_fed_scan_on_lane_edges(ctx, N):
    """ibs_gamma_scan_f64 with X / dX on the wells mapped onto geometry arrays (one line per target; the mapped rows do not depend on
    theta0, so a repeated theta0 repeats the system): k_gamma_scan, its lean and resident forms for 3 <= M <= 8, two theta0 chained
    through a wave, and the 32- / 16-lane forms plain and chained -- every column of every call against the oracle"""
    M = ec.rows_per_lane(N)
    plain = "ibs::k_gamma_scan<double, %d>" % M
    calls = [("default", {}, plain, 64, 1)]
    if 3 <= M <= 8:
        calls += [("scan_resident=0", {"scan_resident": 0}, "ibs::k_gamma_scan_lean<double, %d>" % M, 64, 1),
                  ("scan_resident=1", {"scan_resident": 1}, plain, 64, 1)]
    calls.append(("scan_chain=2", {"scan_chain": 2}, "ibs::k_gamma_scan_chain<double, %d>" % M, 64, 2))
    for P in ec.lanes_allowed(N):
        Mg, G = (N - 2 + P - 1) // P, 64 // P
        calls += [("force_p=%d" % P, {"force_p": P, "scan_chain": 1}, "ibs::k_gamma_scan_g<double, %d, %d>" % (Mg, P), P, G),
                  ("force_p=%d scan_chain=2" % P, {"force_p": P, "scan_chain": 2}, "ibs::k_gamma_scan_g_chain<double, %d, %d>" % (Mg, P), P, 2 * G)]
    for tag, opts, name, P, n_t0 in calls:
        targets = ec.lane_targets(N, P)
        th, (g, c, f) = well_batch(N, targets)
        h = float(th[1] - th[0])
        geo = [np.stack(x) for x in zip(*[ec.to_geometry(g[k], c[k], f[k]) for k in range(len(targets))])]
        r, got = run_with(ctx, opts, lambda: ctx.gamma_scan(h, *geo, np.full(len(targets), -1.0), np.zeros(n_t0), want_X=True, want_info=True))
        assert got == name, (N, tag, got, name)
        note("gamma_scan_f64 mapped well, %s (%d targets x %d theta0)" % (tag, len(targets), n_t0), N, name=got)
        assert r["nbad"] == 0, (N, tag)
        clean(r["info"], N)
        for col in range(n_t0):
            check_fp64(N, "scan %s, theta0 %d" % (tag, col), targets, r, col=col)
