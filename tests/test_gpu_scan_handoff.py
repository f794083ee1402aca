"""GPU: the per-surface maximum that the one-wave scan kernels hand over at the end of a launch (ScanPlan.scan_argmax: the block
whose arrival completes a surface lets its wave 0 read the surface's growth rates back and reduce them) against the two-launch
path, bit for bit.

Expected values never come from the code under test: `plan.scan(); plan.argmax()` (two launches, no hand-off) gives gam and the
pair, and numpy's argmax -- the FIRST maximum, ball_scan.py:283-288 -- of the returned gam gives the index.  The hand-off holds
comparisons only, so every check is for equal bits; each case runs under pack_mode 0 (the library's choice), 1 (write-through
stores + sc1 loads) and 2 (release / acquire fences).

Geometry: the golden NCSX lines (tests/golden/G3_ncsx_lines.npz) interpolated linearly onto N = 193 (3 rows per lane) and N = 257
(4 rows per lane), the shortest grids that take the resident form k_gamma_scan<double, M>; every line scaled a little differently
so that no two lines of a case agree by accident.

Shapes (lines per surface x theta0 = n_per growth rates per surface, the table one wave reads, lane l taking l, l + 64, ...):
1 (one lane, one block), 7 (part of a wave), 64 (every lane once), 65 (one lane twice), 135 (third round partly filled), 360 (six
rounds, the second group of four loads partly filled), each with 1 and with 3 surfaces.  theta0 counts 5, 7 and 15 are no multiple
of the waves per block wherever a block holds more than one wave: the launches of 1,080 solves (3 x 24 x 15) run four waves per
block and those of 675 (5 x 9 x 15) two, the last block of every line with an invalid wave that must neither count as an arrival
nor shift an index; all smaller launches run one wave per block."""
import functools
import os

import numpy as np
import pytest

from oracle import ballooning_oracle as bo

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
MODES = [0, 1, 2]
# (surfaces, lines per surface, theta0, N)
SHAPES = [(ns, na, nt0, N) for (na, nt0, N) in [(1, 1, 193), (1, 7, 257), (8, 8, 257), (13, 5, 193), (9, 15, 257), (24, 15, 193)]
          for ns in (1, 3)] + [(5, 9, 15, 257)]


def rows_per_lane(N):
    return (N - 2 + 63) // 64


@pytest.fixture(scope="module")
def ctx():
    import ibs_amd
    c = ibs_amd.Context(0)
    yield c
    c.reset_options()
    c.close()


@functools.lru_cache(maxsize=None)
def golden_lines(N):
    """the 16 golden lines on the N-point grid: (16, 8, N)"""
    g3 = np.load(os.path.join(G, "G3_ncsx_lines.npz"))
    th513, th = bo.theta_grid(513), bo.theta_grid(N)
    return np.stack([np.stack([np.interp(th, th513, ln[k]) for k in range(8)]) for ln in g3["geo_513"]])


def host_case(n_lines, N, seed):
    """(geo (n_lines, 8, N), dPdrho (n_lines,)): line l is golden line l % 16 with its drifts and its gds arrays scaled by factors
    of its own (the recipe of test_fused_scan_argmax_equals_two_launches)"""
    rng = np.random.default_rng(seed)
    geo = golden_lines(N)[np.arange(n_lines) % 16].copy()
    geo[:, 4:7] *= (1 + rng.uniform(-0.08, 0.08, n_lines))[:, None, None]
    geo[:, 2:4] *= (1 + rng.uniform(-0.08, 0.08, n_lines))[:, None, None]
    dP = -0.5 * np.mean((geo[:, 2] - geo[:, 7]) * geo[:, 0] ** 2, axis=1)
    return geo, dP


def make_plan(ctx, geo, dP, nt0, ns):
    import torch
    import ibs_amd
    dev = torch.device("cuda:0")
    N = geo.shape[2]
    th = bo.theta_grid(N)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return ibs_amd.ScanPlan(ctx, float(th[1] - th[0]), [t(geo[:, k]) for k in range(7)], t(dP), t(np.linspace(0, np.pi / 2, nt0)), ns)


def two_launches(plan):
    """(pack, gam) of the two-launch path, with the index checked against numpy's first maximum; plan.pack is left poisoned"""
    import torch
    plan.scan(); plan.argmax()
    torch.cuda.synchronize()
    pack, gam = plan.pack.clone(), plan.gam.clone()
    tab = gam.reshape(plan.n_surf, -1).cpu().numpy()
    assert np.isfinite(tab).all()
    assert np.array_equal(pack[:, 1].cpu().numpy(), tab.argmax(axis=1).astype(np.float64))
    assert np.array_equal(pack[:, 0].cpu().numpy(), tab.max(axis=1))
    plan.pack.fill_(-7.0)
    return pack, gam


_cases = {}


def case_seed(ns, na, nt0, N, variant):
    return 1000 * ns + 10 * na + nt0 + N + 7919 * variant


def case(ctx, ns, na, nt0, N, variant=0):
    """plan and two-launch reference of one shape: built once, shared by the modes and forms that run it, never changed"""
    key = (ns, na, nt0, N, variant)
    if key not in _cases:
        geo, dP = host_case(ns * na, N, case_seed(ns, na, nt0, N, variant))
        plan = make_plan(ctx, geo, dP, nt0, ns)
        _cases[key] = (plan,) + two_launches(plan)
    return _cases[key]


def fused_equals(ctx, plan, want_pack, want_gam, mode, name, tag):
    """one fused launch under pack_mode `mode`: pack and gam carry the reference's bits, the index is numpy's first maximum of the
    gam this launch returned, and the launch ran under `name`"""
    import torch
    try:
        ctx.set_option("pack_mode", mode)
        plan.pack.fill_(-7.0)
        plan.scan_argmax()
        torch.cuda.synchronize()
        launched = ctx.last_launch()[0]
    finally:
        ctx.set_option("pack_mode", None)
    assert launched == name, (tag, launched)
    assert torch.equal(plan.gam, want_gam), tag
    assert torch.equal(plan.pack, want_pack), (tag, plan.pack, want_pack)
    tab = plan.gam.reshape(plan.n_surf, -1).cpu().numpy()
    assert np.array_equal(plan.pack[:, 1].cpu().numpy(), tab.argmax(axis=1).astype(np.float64)), tag


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("ns,na,nt0,N", SHAPES)
def test_table_sizes_on_the_edges_of_the_one_wave_read(ctx, ns, na, nt0, N, mode):
    plan, want_pack, want_gam = case(ctx, ns, na, nt0, N)
    fused_equals(ctx, plan, want_pack, want_gam, mode, "ibs::k_gamma_scan<double, %d>" % rows_per_lane(N), (ns, na, nt0, N, mode))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("ns,na,nt0,N", [(3, 8, 8, 257), (1, 9, 15, 257), (3, 9, 15, 257)])
def test_lean_form_hands_over_the_same_pair(ctx, ns, na, nt0, N, mode):
    """scan_resident = 0: the same body under the name k_gamma_scan_lean, n_per = 64 and 135"""
    plan, want_pack, want_gam = case(ctx, ns, na, nt0, N)
    try:
        ctx.set_option("scan_resident", 0)
        fused_equals(ctx, plan, want_pack, want_gam, mode, "ibs::k_gamma_scan_lean<double, %d>" % rows_per_lane(N), (ns, na, nt0, N, mode))
    finally:
        ctx.set_option("scan_resident", None)


N_TIE = 257
# name: (lines per surface, theta0, lines that receive the copy)
TIES = {"line 0 and line 3": (8, 5, [0, 3]), "line 0 and the last line": (8, 5, [0, 7]), "all lines": (8, 5, list(range(8))),
        "line 0 and line 8": (9, 8, [0, 8])}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("copies", list(TIES))
def test_equal_maxima_in_different_blocks_return_the_lower_index(ctx, copies, mode):
    """surface 1 of two: the line that holds its maximum is copied (arrays and dPdrho) into line 0 and into line 3 / the last line /
    every line.  Equal inputs give equal bits, one block per (line, theta0) here, so the same maximum sits in two (or eight) blocks
    and the pair must name line 0's.  With 8 theta0, line 0 and line 8 lie 64 entries apart: the equal maxima are then the first and
    the second load of ONE lane of the reducing wave"""
    na, nt0, dst = TIES[copies]
    key = ("tie", copies)
    if key not in _cases:
        plain = case(ctx, 2, na, nt0, N_TIE)                             # the surfaces before any line is copied
        geo0, dP0 = host_case(2 * na, N_TIE, case_seed(2, na, nt0, N_TIE, 0))
        geo, dP = geo0.copy(), dP0.copy()
        top = int(plain[1][1, 1].item()) // nt0                          # line (within surface 1) of its maximum
        for d in dst:
            geo[na + d], dP[na + d] = geo0[na + top], dP0[na + top]
        plan = make_plan(ctx, geo, dP, nt0, 2)
        want_pack, want_gam = two_launches(plan)
        tab = want_gam.reshape(2, na, nt0)[1].cpu().numpy()
        j = int(want_pack[1, 1].item())
        assert j < nt0, (copies, j)                                      # the first maximum lies on line 0 ...
        for d in dst:                                                    # ... and every copy carries the same bits
            assert tab[d, j] == tab.max() and np.array_equal(tab[d], tab[0]), (copies, d)
        _cases[key] = (plan, want_pack, want_gam)
    plan, want_pack, want_gam = _cases[key]
    fused_equals(ctx, plan, want_pack, want_gam, mode, "ibs::k_gamma_scan<double, %d>" % rows_per_lane(N_TIE), (copies, mode))


@pytest.mark.parametrize("mode", MODES)
def test_alternating_plans_reset_the_counter_and_read_nothing_stale(ctx, mode):
    """two plans with different data on one context (one set of arrival counters), launched alternately 40 times, pack cloned in
    stream order after each launch: every clone is its own plan's pair.  Before each launch, in stream order, the plan's pack is
    poisoned (a launch that does not write it shows) and so is its gam, with a value above every growth rate (a growth rate read
    back before this launch's store of it has arrived would win the maximum)"""
    import torch
    ns, na, nt0, N = 3, 13, 5, 193
    a, b = case(ctx, ns, na, nt0, N), case(ctx, ns, na, nt0, N, variant=1)
    assert not torch.equal(a[1], b[1])
    assert float(max(a[2].max(), b[2].max())) < 1e300
    got = []
    try:
        ctx.set_option("pack_mode", mode)
        for r in range(40):
            k = r & 1
            plan = (a, b)[k][0]
            plan.pack.fill_(-7.0); plan.gam.fill_(1e300)
            plan.scan_argmax()
            got.append((k, plan.pack.clone(), plan.gam.clone()))
        torch.cuda.synchronize()
    finally:
        ctx.set_option("pack_mode", None)
    for r, (k, pk, gm) in enumerate(got):
        assert torch.equal(pk, (a, b)[k][1]), (mode, r, k)
        assert torch.equal(gm, (a, b)[k][2]), (mode, r, k)
