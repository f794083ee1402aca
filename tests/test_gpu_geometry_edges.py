"""GPU: the field-line geometry kernels (csrc/ibs_geometry.hip) and their VJP (csrc/ibs_geometry_vjp.hip) on wave-item, tail, block
and ballot edges, against oracle/geometry_oracle.py and tests/geometry_vjp_oracle.py on tables from tests/golden/G8_wout_ncsx_op.npz.
The inputs and the reason for each are in tests/edge_cases.py; tests/test_edge_cases_cpu.py pins the dispatch arithmetic they rest on.

Forward against the oracle: 1e-10 of each (line, array) maximum, dPdrho to 1e-12 max(1, |dPdrho|) (test_geometry_on_other_mode_sets);
form against form where not bit for bit: 1e-11 (test_F1_geometry_lanes_per_point_variants_agree); VJP: BAR = 3.1e-12 per column
(test_vjp_against_the_oracle).  Every test prints its worst figure before it asserts it."""
import ctypes as C
import os

import numpy as np
import pytest

import ibs_amd
from ibs_amd import _lib
from tests import edge_cases as ec
from tests import geometry_vjp_oracle as vo
from tests.test_gpu_geometry_vjp import BAR, LINE_ALPHA, LINE_SURF, NAMES, SVALS, _col_ratios, _subset_wout

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FWD_TOL, DP_TOL = 1e-10, 1e-12
FORMS = ["1", "-2", "2", "4", "8", "default", "general"]          # geo_lpp, the library's choice, use_rows=False
GENERAL = "ibs::k_fieldline_geometry"


@pytest.fixture(scope="module")
def ctx():
    return ibs_amd.Context(0)


@pytest.fixture(autouse=True)
def _default_dispatch(ctx):
    ctx.reset_options()
    yield
    ctx.reset_options()


@pytest.fixture(scope="module")
def wout():
    return dict(np.load(os.path.join(G, "G8_wout_ncsx_op.npz")))


@pytest.fixture(scope="module")
def tabs2(wout):
    return ibs_amd.SurfaceTables.from_wout(wout, [0.5, 0.8])


@pytest.fixture(scope="module")
def n_cu():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


_ORACLE = {}


def oracle_lines(tabs, ls, la, th, key):
    """(geo (8, n, N), dPdrho (n,)) of the numpy oracle for the given lines, computed once per key and never modified"""
    if key not in _ORACLE:
        modes = dict(xm=tabs.xm, xn=tabs.xn, xm_nyq=tabs.xm_nyq, xn_nyq=tabs.xn_nyq)
        geo, dP = vo.numpy_forward(modes, tabs.tab_mn, tabs.tab_nyq, tabs.scal, np.asarray(ls), np.asarray(la), th)
        geo.setflags(write=False); dP.setflags(write=False)
        _ORACLE[key] = (geo, dP)
    return _ORACLE[key]


def fwd_ratios(geo, dP, ref_geo, ref_dP):
    """(max over (line, array) of max|delta| / max|oracle| along the line, max |delta dPdrho| / max(1, |dPdrho|))"""
    assert np.isfinite(geo).all() and np.isfinite(dP).all()
    r = np.abs(geo - ref_geo).max(axis=2) / np.abs(ref_geo).max(axis=2)
    return float(r.max()), float((np.abs(dP - ref_dP) / np.maximum(1.0, np.abs(ref_dP))).max())


def set_form(ctx, form):
    """steer the form; returns use_rows"""
    ctx.set_option("geo_lpp", form if form in ec.GEO_FORMS else None)
    return form != "general"


def expected_kernel(form, n_lines, N, n_cu, nrows_mn):
    if form == "general":
        return GENERAL
    return ec.geo_kernel_name(*ec.geo_pick_form(n_lines, N, n_cu, 0 if form == "default" else form), nrows_mn)


def t_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda:0"))


def run_dev(ctx, tabs, ls, la, th, use_rows=True):
    """device pointers in and out; numpy back"""
    import torch
    r = ctx.fieldline_geometry(tabs, t_dev(np.asarray(ls, dtype=np.int32)), t_dev(np.asarray(la, dtype=np.float64)), t_dev(th),
                               device=torch.device("cuda:0"), use_rows=use_rows)
    return r["geo"].cpu().numpy(), r["dPdrho"].cpu().numpy()


# ---- 1. grid lengths, every form --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_grid_lengths_on_item_tail_and_unit_edges(ctx, tabs2, n_cu, form):
    """all eight arrays and dPdrho of five lines on two surfaces (order 1 0 1 1 0) at every length of ec.GEO_EDGE_N: for each item
    size pts the lengths pts - 1, pts, pts + 1, pts + 16, pts + 17, 8 pts, 8 pts + 1, 8 pts + 17, and 2, 3, 7, 66.  The tail
    kernel's launch is not recorded by ibs_last_launch (the row kernel's is): that it runs where expected is the CPU pin of the
    arithmetic, here its points are compared like all others."""
    use_rows = set_form(ctx, form)
    ls, la = ec.GEO_EDGE_SURF, ec.GEO_EDGE_ALPHA
    worst = (0.0, 0.0)
    for N in ec.GEO_EDGE_N:
        th = ibs_amd.theta_grid(N)
        ref = oracle_lines(tabs2, ls, la, th, ("lengths", N))
        r = ctx.fieldline_geometry(tabs2, ls, la, th, use_rows=use_rows)
        name = ctx.last_launch()[0]
        rg, rd = fwd_ratios(r["geo"], r["dPdrho"], *ref)
        tail = ec.geo_dispatch(N, *ec.geo_pick_form(len(ls), N, n_cu, 0 if form == "default" else form))["tail"] if use_rows else 0
        print("lengths N=%4d form %-7s %-28s tail points %2d: geo %.2e  dPdrho %.2e" % (N, form, name, tail, rg, rd))
        assert name == expected_kernel(form, len(ls), N, n_cu, len(tabs2.rows_mn)), (N, form, name)
        worst = max(worst, (rg, rd))
        assert rg <= FWD_TOL and rd <= DP_TOL, (N, form, rg, rd)
    print("lengths form %s: worst geo %.2e (dPdrho %.2e)" % (form, *worst))


# ---- 2. alpha and theta outside the tested box --------------------------------------------------------------------------------------
def _window_grids():
    out = [("[%.2f, %.2f] N=%d" % (lo, hi, N), np.linspace(lo, hi, N)) for lo, hi in ec.GEO_WINDOWS for N in ec.GEO_WINDOW_N]
    return out + [("non-uniform N=131", ec.geo_nonuniform_grid())]


@pytest.mark.parametrize("form", ec.GEO_WINDOW_FORMS)
def test_alpha_and_theta_outside_the_scan_window(ctx, tabs2, n_cu, form):
    """alpha = -3 pi, -7.3, 0, pi, 9.1 on the windows [-4 pi, 4 pi], [2 pi, 10 pi], [-pi, pi] at N = 131 and N = 65, and one
    non-uniform grid of 131 points"""
    set_form(ctx, form)
    ls, la = ec.GEO_EDGE_SURF, ec.GEO_ALPHAS
    for label, th in _window_grids():
        ref = oracle_lines(tabs2, ls, la, th, ("window", label))
        r = ctx.fieldline_geometry(tabs2, ls, la, th)
        name = ctx.last_launch()[0]
        rg, rd = fwd_ratios(r["geo"], r["dPdrho"], *ref)
        print("window %-26s form %-2s %-28s: geo %.2e  dPdrho %.2e" % (label, form, name, rg, rd))
        assert name == expected_kernel(form, len(ls), len(th), n_cu, len(tabs2.rows_mn))
        assert rg <= FWD_TOL and rd <= DP_TOL, (label, form, rg, rd)


# ---- 3. many lines, alternating surfaces ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ec.GEO_MANY_FORMS)
@pytest.mark.parametrize("n_lines,N", ec.GEO_MANY)
def test_many_lines_on_alternating_surfaces(ctx, tabs2, n_cu, n_lines, N, form):
    """line_surf[i] = i % 2, device pointers: (a) the first line, the last and every 17th against the oracle; (b) the same lines in
    reversed order give every line bit for bit what it was: a line depends neither on its position nor on the block that staged it"""
    set_form(ctx, form)
    rng = np.random.default_rng(29)
    ls = (np.arange(n_lines) % 2).astype(np.int32)
    la = rng.uniform(-np.pi, np.pi, n_lines)
    th = ibs_amd.theta_grid(N)
    geo, dP = run_dev(ctx, tabs2, ls, la, th)
    name, waves = ctx.last_launch()
    d = ec.geo_dispatch(N, *ec.GEO_FORMS[form])
    assert name == ec.geo_kernel_name(*ec.GEO_FORMS[form], len(tabs2.rows_mn))
    assert n_lines * d["units"] > n_cu and waves == 8 * n_cu, (n_lines, d, n_cu, waves)      # more units than blocks: blocks own several
    pick = sorted(set(range(0, n_lines, 17)) | {n_lines - 1})
    ref = oracle_lines(tabs2, ls[pick], la[pick], th, ("many", n_lines, N))
    rg, rd = fwd_ratios(geo[:, pick], dP[pick], *ref)
    geo_r, dP_r = run_dev(ctx, tabs2, ls[::-1], la[::-1], th)
    same = np.array_equal(geo_r[:, ::-1], geo) and np.array_equal(dP_r[::-1], dP)
    diff = np.flatnonzero((geo_r[:, ::-1] != geo).any(axis=(0, 2)))
    print("many %d x %d form %-2s %s, %d lines checked: geo %.2e  dPdrho %.2e; reversed order: %d lines differ %s"
          % (n_lines, N, form, name, len(pick), rg, rd, len(diff), diff[:8]))
    assert rg <= FWD_TOL and rd <= DP_TOL, (rg, rd)
    assert same, diff


# ---- 4. the default form on both sides of each threshold ----------------------------------------------------------------------------
@pytest.mark.parametrize("k", [8, 16, 32, 64])
def test_default_form_on_both_sides_of_a_threshold(ctx, tabs2, n_cu, k):
    """N = 131, the largest line count with at most k points per wave slot (8 n_cu slots) and the next one: the instantiation
    ibs_last_launch names, 20 sampled lines against the oracle, and every line bit for bit the forced form of that name"""
    N = 131
    th = ibs_amd.theta_grid(N)
    (_, below, above), = [t for t in ec.geo_threshold_lines(N, n_cu) if t[0] == k]
    rng = np.random.default_rng(31)
    la_all = rng.uniform(-np.pi, np.pi, above)
    forms = []
    for n_lines in (below, above):
        ppl, lpp = ec.geo_pick_form(n_lines, N, n_cu)
        forms.append((ppl, lpp))
        ls, la = (np.arange(n_lines) % 2).astype(np.int32), la_all[:n_lines]
        ctx.reset_options()
        geo, dP = run_dev(ctx, tabs2, ls, la, th)
        name = ctx.last_launch()[0]
        pick = np.unique(np.linspace(0, n_lines - 1, 20).astype(int))
        ref = oracle_lines(tabs2, ls[pick], la[pick], th, ("threshold", k, n_lines))
        rg, rd = fwd_ratios(geo[:, pick], dP[pick], *ref)
        ctx.set_option("geo_lpp", -2 if ppl == 2 else lpp)
        geo_f, dP_f = run_dev(ctx, tabs2, ls, la, th)
        name_f = ctx.last_launch()[0]
        print("threshold %2d points per slot, %4d lines x %d on %d CUs: default %s, forced %s: geo %.2e  dPdrho %.2e"
              % (k, n_lines, N, n_cu, name, name_f, rg, rd))
        assert name == name_f == ec.geo_kernel_name(ppl, lpp, len(tabs2.rows_mn)), (name, name_f, ppl, lpp)
        assert rg <= FWD_TOL and rd <= DP_TOL, (rg, rd)
        assert np.array_equal(geo, geo_f) and np.array_equal(dP, dP_f)
    assert forms[0] != forms[1] and 64 * forms[1][0] // forms[1][1] == 2 * (64 * forms[0][0] // forms[0][1])


# ---- 5. row pitch -----------------------------------------------------------------------------------------------------------------
SENTINEL = -7.25e300


def _raw_forward(ctx, tabs, ls, la, th, ld, device):
    """ibs_fieldline_geometry_f64 through ctypes with a row pitch ld >= N, output pre-filled with SENTINEL; numpy back"""
    import torch
    n_lines, N = len(ls), len(th)
    host = [tabs.xm, tabs.xn, tabs.xm_nyq, tabs.xn_nyq, tabs.tab_mn, tabs.tab_nyq, tabs.scal]
    ls = np.ascontiguousarray(ls, dtype=np.int32); la = np.ascontiguousarray(la, dtype=np.float64); th = np.ascontiguousarray(th)
    fn = _lib.lib().ibs_fieldline_geometry_f64
    head = (ctx._h, len(tabs.s), len(tabs.xm), len(tabs.xm_nyq))
    tail = (float(tabs.dn_mn), float(tabs.dn_nyq))
    if not device:
        geo = np.full((8, n_lines, ld), SENTINEL); dP = np.full(n_lines, SENTINEL)
        p = lambda a: C.c_void_p(a.ctypes.data)
        _lib.check(fn(*head, *[p(a) for a in host], n_lines, p(ls), p(la), N, p(th), ld, p(geo), p(dP), len(tabs.rows_mn), p(tabs.rows_mn),
                      len(tabs.rows_nyq), p(tabs.rows_nyq), *tail, _lib.MEM_HOST), "ibs_fieldline_geometry_f64")
        return geo, dP
    dev = torch.device("cuda:0")
    allc = ctx._device_tables(tabs, dev)
    d_ls, d_la, d_th = t_dev(ls), t_dev(la), t_dev(th)
    geo = torch.full((8, n_lines, ld), SENTINEL, dtype=torch.float64, device=dev)
    dP = torch.full((n_lines,), SENTINEL, dtype=torch.float64, device=dev)
    ctx._stream_from_torch(geo)
    p = lambda t: C.c_void_p(t.data_ptr())
    _lib.check(fn(*head, *[p(t) for t in allc[:7]], n_lines, p(d_ls), p(d_la), N, p(d_th), ld, p(geo), p(dP), len(tabs.rows_mn), p(allc[7]),
                  len(tabs.rows_nyq), p(allc[8]), *tail, _lib.MEM_DEVICE), "ibs_fieldline_geometry_f64")
    torch.cuda.synchronize()
    return geo.cpu().numpy(), dP.cpu().numpy()


@pytest.mark.parametrize("form", ["1", "-2"])
@pytest.mark.parametrize("N,ld", ec.GEO_PITCH)
def test_row_pitch_beyond_the_grid_length(ctx, tabs2, N, ld, form):
    """ld = N + 5 through the C entry point, host and device pointers: the first N entries of every row are bit for bit the ld = N
    result, and no padding entry is written.  (Host calls once copied the whole padded buffer back from the workspace and so overwrote
    all 200 padding entries of each of these cases; the rows themselves were right.)"""
    set_form(ctx, form)
    ls, la = ec.GEO_EDGE_SURF, ec.GEO_EDGE_ALPHA
    th = ibs_amd.theta_grid(N)
    for device in (False, True):
        geo0, dP0 = _raw_forward(ctx, tabs2, ls, la, th, N, device)
        geo, dP = _raw_forward(ctx, tabs2, ls, la, th, ld, device)
        name = ctx.last_launch()[0]
        bad_rows = int((geo[:, :, :N] != geo0).sum())
        bad_pad = int((geo[:, :, N:] != SENTINEL).sum())
        print("pitch N=%d ld=%d form %-2s %s %s pointers: %d entries differ from ld = N, %d of %d padding entries written"
              % (N, ld, form, name, "device" if device else "host", bad_rows, bad_pad, geo[:, :, N:].size))
        assert name == ec.geo_kernel_name(*ec.GEO_FORMS[form], len(tabs2.rows_mn))
        assert not (geo0 == SENTINEL).any() and np.isfinite(geo0).all()
        assert bad_rows == 0 and np.array_equal(dP, dP0)
        assert bad_pad == 0


# ---- 6. few used surfaces out of many ---------------------------------------------------------------------------------------------
def test_few_used_surfaces_out_of_many(ctx, wout):
    """40 surfaces, device pointers, five lines: images are built for the surfaces the call's lines lie on only (k_geo_mark).  A
    second call on the same tables object with other surfaces must build theirs."""
    m = ec.GEO_MARK
    tabs = ibs_amd.SurfaceTables.from_wout(wout, np.linspace(0.1, 0.95, m["n_surf"]))
    th = ibs_amd.theta_grid(131)
    for which in ("first", "second"):
        ls = np.array(m[which], dtype=np.int32)
        ref = oracle_lines(tabs, ls, ec.GEO_EDGE_ALPHA, th, ("mark", which))
        geo, dP = run_dev(ctx, tabs, ls, ec.GEO_EDGE_ALPHA, th)
        rg, rd = fwd_ratios(geo, dP, *ref)
        print("mark %s call, surfaces %s of %d, %s: geo %.2e  dPdrho %.2e" % (which, sorted(set(m[which])), m["n_surf"], ctx.last_launch()[0], rg, rd))
        assert ctx.last_launch()[0].startswith("ibs::k_geo_rows<")
        assert rg <= FWD_TOL and rd <= DP_TOL, (which, rg, rd)


# ---- VJP ------------------------------------------------------------------------------------------------------------------------------
_VCASES = {}


def few_modes(wout, n_mn, n_nyq):
    """fewer than 8 modes per table: the four leading ones (m = 0, n = 0 .. 3 nfp) and the m = 1 modes nearest n = 0.  The leading
    modes alone (as _case keeps them) have m = 0 throughout: a surface without poloidal dependence, grad s = 0, planes of zeros."""
    def keep(xm, xn, n):
        step = np.abs(xn[xn != 0]).min()
        m1 = np.flatnonzero((xm == 1) & (np.abs(xn) <= step))
        return np.sort(np.concatenate([np.arange(n - len(m1)), m1]))
    return _subset_wout(wout, keep(wout["xm"], wout["xn"], n_mn), keep(wout["xm_nyq"], wout["xn_nyq"], n_nyq))


def subset_modes(wout, n_mn, n_nyq, seed=3):
    """the eight leading modes and a random choice of the others, as _case's "subset" """
    rng = np.random.default_rng(seed)
    kmn = np.sort(np.concatenate([np.arange(8), 8 + rng.choice(len(wout["xm"]) - 8, n_mn - 8, replace=False)]))
    knq = np.sort(np.concatenate([np.arange(8), 8 + rng.choice(len(wout["xm_nyq"]) - 8, n_nyq - 8, replace=False)]))
    return _subset_wout(wout, kmn, knq)


def vcase(key, w, ls, la, N):
    """tables, lines, a fixed random (geo_bar, dPdrho_bar) scaled by each plane's maximum, the oracle's VJPs: once per key"""
    if key in _VCASES:
        return _VCASES[key]
    tabs = ibs_amd.SurfaceTables.from_wout(w, SVALS)
    ls = np.asarray(ls, dtype=np.int32); la = np.asarray(la, dtype=np.float64)
    th = ibs_amd.theta_grid(N)
    modes = dict(xm=tabs.xm, xn=tabs.xn, xm_nyq=tabs.xm_nyq, xn_nyq=tabs.xn_nyq)
    geo, dP = vo.numpy_forward(modes, tabs.tab_mn, tabs.tab_nyq, tabs.scal, ls, la, th)
    rng = np.random.default_rng(17)
    gb = rng.standard_normal(geo.shape) / np.abs(geo).max(axis=(1, 2), keepdims=True)
    db = rng.standard_normal(len(ls)) / np.abs(dP).max()
    assert np.isfinite(gb).all() and np.isfinite(db).all()
    args = (tabs.xm, tabs.xn, tabs.xm_nyq, tabs.xn_nyq, tabs.tab_mn, tabs.tab_nyq, tabs.scal, ls, la, th)
    c = dict(tabs=tabs, ls=ls, la=la, th=th, gb=gb, db=db, ref=vo.vjp(*args, gb, None), ref_dp=vo.vjp(*args, gb, db))
    _VCASES[key] = c
    return c


def check_vjp(ctx, label, c):
    """both VJPs of a case against the oracle per column; returns the run with dPdrho_bar"""
    tabs, ls, la, th = c["tabs"], c["ls"], c["la"], c["th"]
    got = ctx.fieldline_geometry_vjp(tabs, ls, la, th, c["gb"])
    got_dp = ctx.fieldline_geometry_vjp(tabs, ls, la, th, c["gb"], c["db"])
    name = ctx.last_launch()[0]
    r0, r1 = _col_ratios(got, c["ref"]), _col_ratios(got_dp, c["ref_dp"])
    print("vjp %-34s %d lines x %d, %d + %d modes, %s: vjp %.2e  with dPdrho_bar %.2e  bar %.2e"
          % (label, len(ls), len(th), len(tabs.xm), len(tabs.xm_nyq), name, r0.max(), r1.max(), BAR))
    assert np.isfinite(r0).all() and np.isfinite(r1).all(), (r0, r1)
    assert r0.max() <= BAR and r1.max() <= BAR, (r0, r1)
    unused = sorted(set(range(len(SVALS))) - set(int(k) for k in ls))
    for g in (got, got_dp):
        for nm in NAMES[:3]:
            assert np.all(g[nm][unused] == 0.0), (nm, unused)
    return got_dp


def lines_case(wout, n_lines):
    return vcase(("lines", n_lines), wout, ec.geo_vjp_line_surf(n_lines), ec.geo_vjp_line_alpha(n_lines), ec.GEO_VJP_LINES_N)


# ---- 7. line counts on ballot-word edges --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_lines", ec.GEO_VJP_LINES)
def test_vjp_line_counts_on_ballot_word_edges(ctx, wout, n_lines):
    """63, 64, 65 and 130 lines of 35 points on four surfaces, alpha over [-3 pi, 3 pi]: surface 1 holds no line (cotangents exactly
    0), surface 3 only lines at index >= 64, surface 2 lines on both sides of index 64"""
    c = lines_case(wout, n_lines)
    assert 1 not in c["ls"]
    check_vjp(ctx, "ballot words", c)


# ---- 8. grid lengths ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", ec.GEO_VJP_N)
def test_vjp_grid_lengths_on_lane_edges(ctx, wout, N):
    """N = 2, 63, 64, 65 with the seven lines of test_vjp_against_the_oracle (shuffled surfaces, one without lines)"""
    check_vjp(ctx, "grid length", vcase(("N", N), wout, LINE_SURF, LINE_ALPHA, N))


# ---- 9. mode tables -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", sorted(ec.GEO_VJP_MODES))
def test_vjp_mode_tables_on_group_edges(ctx, wout, which):
    """41 + 50 modes: 6 + 7 = 13 groups of 8, so the last block of k_geo_vjp_modes has one wave with work and three that leave;
    7 + 7 modes: one partly filled group per table (the clamp of the mode index).  The oracle's root solve converges on both."""
    n_mn, n_nyq = ec.GEO_VJP_MODES[which]
    w = few_modes(wout, n_mn, n_nyq) if which == "few" else subset_modes(wout, n_mn, n_nyq)
    c = vcase(("modes", which), w, LINE_SURF, LINE_ALPHA, 67)
    assert (len(c["tabs"].xm), len(c["tabs"].xm_nyq)) == (n_mn, n_nyq)
    check_vjp(ctx, "mode tables " + which, c)


# ---- 10. position independence ----------------------------------------------------------------------------------------------------
def test_vjp_does_not_depend_on_the_position_of_a_line(ctx, wout):
    """the 65-line case with its lines permuted: alpha_bar of every line bit for bit what it was; the table and scalar cotangents,
    whose summation order follows the line order by design, within BAR of the oracle and of the first run"""
    c = lines_case(wout, 65)
    first = check_vjp(ctx, "65 lines", c)
    perm = np.random.default_rng(41).permutation(65)
    assert (c["ls"][perm][:64] == 3).any()                      # the surface that had one line in the second ballot word has it in the first
    got = ctx.fieldline_geometry_vjp(c["tabs"], c["ls"][perm], c["la"][perm], c["th"], c["gb"][:, perm], c["db"][perm])
    n_diff = int((got["alpha_bar"] != first["alpha_bar"][perm]).sum())
    back = dict(got, alpha_bar=got["alpha_bar"][np.argsort(perm)])
    r_ref, r_first = _col_ratios(back, c["ref_dp"]), _col_ratios(back, first)
    print("vjp 65 lines permuted: %d alpha_bar entries differ; against the oracle %.2e, against the first run %.2e, bar %.2e"
          % (n_diff, r_ref.max(), r_first.max(), BAR))
    assert n_diff == 0
    assert r_ref.max() <= BAR and r_first.max() <= BAR, (r_ref, r_first)
