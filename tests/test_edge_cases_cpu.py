"""CPU: the inputs of tests/test_gpu_edge_lengths.py pinned with the oracle alone (tests/edge_cases.py), so that a GPU failure there
cannot be blamed on the systems: the moving well keeps its gap and puts the mode on the chosen grid point at every edge length, the
second mode of two_wells sits on the shallow well, the geometry mapping reproduces the rows, the length lists cover the lane / chunk /
path edges they claim, and the two CPU oracles (LAPACK on the symmetrised pencil; division-form bisection + twisted factorisation in
C) agree on this family far inside every tolerance the GPU tests apply.  For tests/test_gpu_geometry_edges.py: the dispatch arithmetic of
the geometry kernels restated, and every edge class its lists claim found in them."""
import numpy as np
import pytest

from oracle import ballooning_oracle as bo
from tests import edge_cases as ec

ALL_N = ec.EDGE_N_SHORT + ec.EDGE_N_LONG + ec.EDGE_N_COUNT


@pytest.mark.parametrize("N", ALL_N)
def test_moving_well_keeps_its_gap_and_peaks_on_the_target(N):
    th = ec.theta_grid(N)
    h = th[1] - th[0]
    for j in ec.twist_targets(N):
        g, c, f = ec.well_rows(th, j)
        w, V = ec.top_pairs(th, g, c, f)
        nA = ec.norm_a(h, g, c, f)[0]
        assert 13.3 < nA < 13.6 and 0.1 < w[1] < 0.74, (N, j, nA, w)
        assert w[1] - w[0] >= 0.02 * nA, (N, j, (w[1] - w[0]) / nA)
        k = int(np.argmax(np.abs(V[:, 1])))
        if ec.is_end_target(N, j):
            assert min(k, N - 1 - k) <= 6 and (k < N // 2) == (j < N // 2), (N, j, k)
        else:
            assert k == j, (N, j, k)


def shallow_partner(N, j_shallow):
    """a deep-well position at least 40 rows from the shallow one and 8 points inside the grid"""
    d = 40 if N < 200 else 60
    return j_shallow + d if j_shallow + d < N - 8 else j_shallow - d


@pytest.mark.parametrize("N", [67, 131, 2049] + ec.EDGE_N_LONG)
def test_two_wells_second_mode_sits_on_the_shallow_well(N):
    th = ec.theta_grid(N)
    h = th[1] - th[0]
    for js in ec.twist_targets(N):
        jd = shallow_partner(N, js)
        g, c, f = ec.two_wells(th, jd, js)
        w, V = ec.top_pairs(th, g, c, f, 3)
        nA = ec.norm_a(h, g, c, f)[0]
        assert min(w[2] - w[1], w[1] - w[0]) >= 0.003 * nA, (N, js, w)
        k1, k0 = int(np.argmax(np.abs(V[:, 1]))), int(np.argmax(np.abs(V[:, 2])))
        assert k0 == jd, (N, js, jd, k0)
        if ec.is_end_target(N, js):
            assert min(k1, N - 1 - k1) <= 6 and (k1 < N // 2) == (js < N // 2), (N, js, k1)
        else:
            assert k1 == js, (N, js, k1)
            assert w[0] < 0.28 and w[1] > 0.6, (N, js, w)


@pytest.mark.parametrize("N", [67, 643, 2307])
def test_geometry_mapping_reproduces_the_rows(N):
    th = ec.theta_grid(N)
    for j in ec.twist_targets(N)[:4]:
        for rows in (ec.well_rows(th, j), ec.two_wells(th, shallow_partner(N, j), j)):
            bmag, gradpar, cvdrift, cvdrift0, gds2, gds21, gds22 = ec.to_geometry(*rows)
            for a, b in zip(bo.gcf(-1.0, bmag, gradpar, cvdrift, gds2), rows):
                assert np.abs(a - b).max() <= 1e-14 * np.abs(b).max()
            cv, gd = bo.fold_theta0(0.7, cvdrift, cvdrift0, gds2, gds21, gds22)       # (no theta0 dependence)
            assert np.array_equal(cv, cvdrift) and np.array_equal(gd, gds2)
            gam_geo = bo.gamma_ball_full(-1.0, th, bmag, gradpar, cvdrift, gds2)[0]
            assert abs(gam_geo - bo.solve_gcf(th, *rows)[0]) < 1e-14


def test_length_lists_cover_the_edges_they_claim():
    S, L, Cn = ec.EDGE_N_SHORT, ec.EDGE_N_LONG, ec.EDGE_N_COUNT
    assert all(N % 2 == 1 and 67 <= N <= 2049 for N in S) and all(N % 2 == 1 and 2050 < N <= 65537 for N in L)
    assert all(N % 2 == 0 and 66 <= N for N in Cn) and len(set(S + L + Cn)) == len(S + L + Cn)
    # every rows-per-lane instantiation of the geometry-fed register kernels
    assert {ec.rows_per_lane(N) for N in S} == set(range(2, 33))
    assert ec.rows_per_lane(129) == 2 and ec.rows_per_lane(131) == 3 and {ec.rows_per_lane(N) for N in (66, 130, 2050)} == {1, 2, 32}
    assert all((N - 2) % 64 == 0 for N in (66, 130, 2050))
    # the sub-wave forms on both sides of their limits
    assert ec.lanes_allowed(97) == [16] and ec.lanes_allowed(99) == [32, 16]
    assert ec.lanes_allowed(257) == [32, 16] and ec.lanes_allowed(259) == [32]
    assert ec.lanes_allowed(641) == [32] and ec.lanes_allowed(643) == []
    # last chunk of the long path: one row, one row short, exactly full; tails of the unroll by 8 other than 7
    m768 = {N: (N - 2) % ec.LONG_CHUNK for N in L + Cn if N > 2050}
    m384 = {N: (N - 2) % ec.VEC_CHUNK for N in L + Cn if N > 2050}
    assert m768[2307] == 1 and m384[2307] == 1 and m768[3075] == 1 and m384[3075] == 1
    assert m768[2305] == 767 and m384[3073] == 383 and m384[2305] == 383
    assert m768[2306] == 0 and m768[3074] == 0 and m384[2306] == 0
    assert {1, 767, 0} <= set(m768.values()) and {1, 383, 0} <= set(m384.values())
    assert {m % 8 for m in m768.values()} >= {0, 1, 7} and {m % 8 for m in m384.values()} >= {0, 1, 7}
    # both branches of the two-grid start
    on = {N for N in L if (N - 1) % 16 == 0}
    assert on == {2305, 3073} and {(N - 1) % 16 for N in (2313, 2889)} == {8}
    assert 2313 == 8 * 17 * 17 + 1 and 2889 == 8 * 19 * 19 + 1
    # twist targets: both ends, and the points about every multiple of 384 taken
    for N in [67, 131, 1985, 2049] + L:
        t = ec.twist_targets(N)
        assert t[:2] == [1, N - 2] and len(t) <= 24 and len(set(t)) == len(t) and all(1 <= j <= N - 2 for j in t)
        ms = sorted({j for j in t if j % ec.VEC_CHUNK == 0})
        assert ms == [m for m in range(ec.VEC_CHUNK, N - 8, ec.VEC_CHUNK)] or (len(t) > 20 and ms[0] == ec.VEC_CHUNK and ms[-1] == (N - 9) // ec.VEC_CHUNK * ec.VEC_CHUNK)
        for m in ms:
            assert {m - 1, m, m + 1, m + 2} <= set(t)
    assert len(ec.twist_targets(67)) == 2 and len(ec.twist_targets(2049)) == 22 and len(ec.twist_targets(65535)) == 22


@pytest.mark.parametrize("N", [67, 2307, 65535])
def test_the_two_oracles_agree_on_the_moving_well(N):
    """two independent references: their agreement is what licenses the fast one on the GPU side.  lam to 4 N eps ||A||, gam to
    1e-10; and X, dX, the count at lam +- 4 N eps ||A|| far inside the GPU tests' tolerances (a tenth of each)"""
    from oracle import c_oracle as co
    th = ec.theta_grid(N)
    h = float(th[1] - th[0])
    targets = ec.twist_targets(N)[:10]
    rows = [ec.well_rows(th, j) for j in targets] + [ec.two_wells(th, shallow_partner(N, targets[-1]), targets[-1])]
    g, c, f = (np.stack([r[i] for r in rows]) for i in range(3))
    nA = ec.norm_a(h, g, c, f)
    gam_b, lam_b, _ = co.solve_gcf_batch(h, g, c, f)
    tol = 4 * N * ec.EPS * nA
    assert (co.count_above_batch(h, g, c, f, np.zeros(len(rows))) >= 1).all()
    for k in range(len(rows)):
        gam, lam, X, dX = bo.solve_gcf(th, g[k], c[k], f[k])
        gc, lc, Xc, dXc = co.solve_gcf(h, g[k], c[k], f[k])
        assert abs(lam - lc) <= tol[k] and abs(lam - lam_b[k]) <= tol[k], (N, k, abs(lam - lc) / tol[k])
        assert abs(gam - gc) < 1e-10 and abs(gam - gam_b[k]) < 1e-10, (N, k, gam - gc)
        short = N <= 2050
        assert np.abs(X - Xc).max() < 0.1 * (1e-7 if short else 1e-6)
        assert np.abs(dX - dXc).max() < 0.1 * ((1e-7 * np.abs(dX).max() + 1e-7) if short else 1e-5 * max(1.0, np.abs(dX).max()))
    lam = np.array([bo.solve_gcf(th, g[k], c[k], f[k])[1] for k in range(len(rows))])
    assert np.array_equal(co.count_above_batch(h, g, c, f, lam + tol), np.zeros(len(rows), dtype=np.int32))
    assert np.array_equal(co.count_above_batch(h, g, c, f, lam - tol), np.ones(len(rows), dtype=np.int32))


@pytest.mark.parametrize("N", [131, 2307])
def test_window_reference_of_the_nearest_eigenpair_equals_the_dense_one(N):
    """tests/nearest_oracle.py: window_nearest (the eigenvalues above sigma - radius alone; used at 65,535 points, where the full
    spectrum takes minutes per system) returns what dense_nearest returns"""
    from tests.nearest_oracle import dense_nearest, window_nearest
    th = ec.theta_grid(N)
    g1, c1 = bo.salpha_gc(th, 1.0, 0.8, 0.0)
    cases = [((g1, 4.0 * c1, g1.copy()), 0.42)]
    for js in ec.twist_targets(N)[:3]:
        rows = ec.two_wells(th, shallow_partner(N, js), js)
        w = ec.top_pairs(th, *rows)[0]
        cases.append((rows, w[0] + (w[1] - w[0]) / 3.0))
    for rows, sigma in cases:
        a, b = dense_nearest(th, *rows, sigma), window_nearest(th, *rows, sigma, radius=0.25)
        assert a["idx"] == b["idx"] >= 1 and a["tie"] == b["tie"] and a["nA"] == b["nA"]
        assert abs(a["lam"] - b["lam"]) <= 4 * N * ec.EPS * a["nA"] and abs(a["lam_max"] - b["lam_max"]) <= 4 * N * ec.EPS * a["nA"]
        assert abs(a["gam"] - b["gam"]) < 1e-12 and np.abs(a["X"] - b["X"]).max() < 1e-10


# ---- the inputs of tests/test_gpu_geometry_edges.py -----------------------------------------------------------------------------------
def test_geometry_dispatch_arithmetic():
    """geo_dispatch / geo_pick_form restate launch_geometry, k_geo_rows and geo_pick_form (csrc/ibs_geometry.hip) on known values"""
    assert ec.GEO_PTS == [8, 16, 32, 64, 128] and {k: 64 * p // l for k, (p, l) in ec.GEO_FORMS.items()} == {"1": 64, "-2": 128, "2": 32, "4": 16, "8": 8}
    # N = 1025 = 8 * 128 + 1 (test_F1_geometry_lanes_per_point_variants_agree): one tail point per line with one lane per point
    assert ec.geo_dispatch(1025, 2, 1) == dict(pts=128, rem=1, tail=1, j_end=1024, items=8, units=1, spare=0, last=128)
    assert ec.geo_dispatch(1025, 1, 1) == dict(pts=64, rem=1, tail=1, j_end=1024, items=16, units=2, spare=0, last=64)
    assert ec.geo_dispatch(1025, 1, 4) == dict(pts=16, rem=1, tail=0, j_end=1025, items=65, units=9, spare=7, last=1)
    assert ec.geo_dispatch(67, 2, 1)["tail"] == 0 and ec.geo_dispatch(67, 1, 1)["tail"] == 3 and ec.geo_dispatch(2, 1, 8)["last"] == 2
    # tools/geo_form_sweep.py: 30 / 54 / 84 / 201 lines of 969 points on 256 CUs -> 4 / 2 / 1 lanes per point / two points per lane
    assert [ec.geo_pick_form(n, 969, 256) for n in (16, 30, 54, 84, 201)] == [(1, 8), (1, 4), (1, 2), (1, 1), (2, 1)]
    assert ec.geo_pick_form(5, 131, 256, "-2") == (2, 1) and ec.geo_pick_form(10 ** 6, 131, 256, 8) == (1, 8)
    assert ec.geo_kernel_name(2, 1) == "ibs::k_geo_rows<2, 1, 12>" and ec.geo_kernel_name(1, 4, 13) == "ibs::k_geo_rows<1, 1, 24>"


def test_geometry_length_list_covers_the_edges_it_claims():
    Ns = ec.GEO_EDGE_N
    assert Ns == sorted(set(Ns)) and min(Ns) == 2 and max(Ns) == 1041 and {2, 3, 7} <= set(Ns) and sum(N < 150 for N in Ns) > len(Ns) // 2
    assert any(N % 2 == 0 and all(N % p for p in ec.GEO_PTS[1:]) for N in Ns)
    for key, (ppl, lpp) in ec.GEO_FORMS.items():
        d = {N: ec.geo_dispatch(N, ppl, lpp) for N in Ns}
        pts = 64 * ppl // lpp
        for N in (pts - 1, pts, pts + 1, pts + 16, pts + 17, 8 * pts, 8 * pts + 1, 8 * pts + 17):
            assert N in d, (key, N)
        tails = {v["tail"] for v in d.values()}
        assert tails >= ({0, 1, 16} if lpp == 1 else {0}) and max(tails) <= (16 if lpp == 1 else 0), (key, tails)
        for N, v in d.items():             # the tail kernel runs exactly where the item arithmetic says, and never on a whole line
            assert v["tail"] == (N % pts if lpp == 1 and N > pts and 1 <= N % pts <= 16 else 0) and v["j_end"] >= min(N, pts)
            assert v["tail"] + v["j_end"] == N and (v["items"] - 1) * pts < v["j_end"] <= v["items"] * pts and 1 <= v["last"] <= pts
        assert d[pts - 1]["items"] == 1 and d[pts - 1]["last"] == pts - 1 and d[pts - 1]["tail"] == 0        # N < pts
        assert d[pts]["rem"] == 0 and d[pts]["items"] == 1 and d[pts]["last"] == pts                          # N = pts
        assert d[pts + 17]["tail"] == 0 and d[pts + 16]["tail"] == (16 if lpp == 1 else 0)
        if pts > 17:                           # (items of 8 and 16 points, four and eight lanes per point: 16 and 17 more points are whole items)
            assert d[pts + 16]["rem"] == 16 and d[pts + 17]["rem"] == 17 and d[pts + 17]["items"] == 2 and d[pts + 17]["last"] == 17
        else:
            assert d[pts + 16]["rem"] == 0 and d[pts + 17]["last"] == 1 and d[pts + 17]["items"] == 2 + 16 // pts
        assert d[8 * pts]["rem"] == 0 and (d[8 * pts]["items"], d[8 * pts]["units"], d[8 * pts]["spare"]) == (8, 1, 0)
        more = (17 + pts - 1) // pts             # 1, or 2 / 3 with items of 16 / 8 points
        assert (d[8 * pts + 17]["items"], d[8 * pts + 17]["units"], d[8 * pts + 17]["spare"]) == (8 + more, 2, 8 - more)
        assert d[8 * pts + 1]["items"] == (8 if lpp == 1 else 9)
        assert {v["items"] for v in d.values()} >= {1, 2, 8, 9}
        assert any(N < pts for N in Ns) and d[2]["last"] == 2 and d[3]["last"] == 3
    # the window cases: a tail point with one lane per point, a line shorter than the item with two points per lane
    assert ec.geo_dispatch(65, 1, 1)["tail"] == 1 and ec.geo_dispatch(65, 2, 1)["items"] == 1 and ec.geo_dispatch(65, 1, 4)["last"] == 1
    assert ec.GEO_WINDOW_N == [131, 65] and 65 in Ns and ec.GEO_WINDOW_FORMS == ["1", "-2", "4"]
    assert min(ec.GEO_ALPHAS) < -np.pi and max(ec.GEO_ALPHAS) > 2 * np.pi and {0.0, np.pi} <= set(ec.GEO_ALPHAS)
    assert any(lo > 0 for lo, hi in ec.GEO_WINDOWS) and any(hi - lo < 7 for lo, hi in ec.GEO_WINDOWS)
    th = ec.geo_nonuniform_grid()
    dth = np.diff(th)
    assert len(th) == 131 and abs(th[0] + 4 * np.pi) < 1e-12 and abs(th[-1] - 4 * np.pi) < 1e-12 and dth.min() > 0 and dth.max() > 3 * dth.min()


def test_geometry_batches_cover_the_block_and_threshold_edges():
    n_cu = 256                                               # MI355X; the GPU test takes the count from the device
    for n_lines, N in ec.GEO_MANY:
        for key in ec.GEO_MANY_FORMS:
            d = ec.geo_dispatch(N, *ec.GEO_FORMS[key])
            U = n_lines * d["units"]
            own = {U * (b + 1) // n_cu - U * b // n_cu for b in range(n_cu)}         # units of block b: [U b / B, U (b + 1) / B)
            assert U > n_cu and len(own) == 2 and min(own) >= 1, (n_lines, N, key, own)
            assert d["spare"] > 0                            # every unit has spare items: item < ipl decides
    assert {ec.geo_dispatch(67, *ec.GEO_FORMS[k])["tail"] for k in ec.GEO_MANY_FORMS} == {3, 0}
    assert {ec.geo_dispatch(145, *ec.GEO_FORMS[k])["last"] for k in ec.GEO_MANY_FORMS} == {17}
    # default form: every threshold from both sides, the item doubling across it
    seen = []
    for k, below, above in ec.geo_threshold_lines(131, n_cu):
        fb, fa = ec.geo_pick_form(below, 131, n_cu), ec.geo_pick_form(above, 131, n_cu)
        assert below * 131 <= 8 * n_cu * k < above * 131 and above == below + 1
        assert 64 * fa[0] // fa[1] == 2 * (64 * fb[0] // fb[1])
        seen += [fb, fa]
    assert [k for k, _, _ in ec.geo_threshold_lines(131, n_cu)] == [8, 16, 32, 64] and set(seen) == set(ec.GEO_FORMS.values())
    assert [(b, a) for _, b, a in ec.geo_threshold_lines(131, n_cu)] == [(125, 126), (250, 251), (500, 501), (1000, 1001)]
    assert all(ld == N + 5 for N, ld in ec.GEO_PITCH) and {N for N, _ in ec.GEO_PITCH} == {145, 67}
    m = ec.GEO_MARK                                          # ibs_fieldline_geometry_f64: marks when n_surf >= 32 and n_lines < 8 n_surf
    assert m["n_surf"] >= 32 and len(m["first"]) == len(m["second"]) == 5 < 8 * m["n_surf"]
    assert set(m["first"]) == {3, 39, 17} and set(m["second"]) == {0, 5} and max(m["first"]) == m["n_surf"] - 1


def test_geometry_vjp_cases_cover_the_ballot_and_group_edges():
    assert ec.GEO_VJP_LINES == [63, 64, 65, 130] and ec.GEO_VJP_N == [2, 63, 64, 65]
    assert {(n + 63) // 64 for n in ec.GEO_VJP_LINES} == {1, 2, 3}
    for n in ec.GEO_VJP_LINES:
        ls, la = ec.geo_vjp_line_surf(n), ec.geo_vjp_line_alpha(n)
        assert len(ls) == len(la) == n and 1 not in ls and set(ls) <= {0, 2, 3}
        assert la.min() == -3 * np.pi and la.max() == 3 * np.pi
        at3, at2 = np.flatnonzero(ls == 3), np.flatnonzero(ls == 2)
        assert (at3 >= 64).all() and (at2 < 64).any()
        if n > 64:
            assert len(at3) >= 1
        if n == 130:                                         # lines of one surface in all three ballot words, of another in two
            assert {i // 64 for i in at2} == {0, 1, 2} and {i // 64 for i in at3} == {1, 2}
    assert list(ec.geo_vjp_line_surf(65)[63:]) == [2, 3]
    # mode tables: the two in use so far fill the last block of four waves, the new ones do not
    assert ec.geo_vjp_groups(242, 392) % 4 == 0 and ec.geo_vjp_groups(37, 53) % 4 == 0
    assert ec.geo_vjp_groups(*ec.GEO_VJP_MODES["odd_groups"]) == 13 and ec.geo_vjp_groups(*ec.GEO_VJP_MODES["few"]) == 2
    assert max(ec.GEO_VJP_MODES["few"]) < ec.GEO_VJP_G


# ---- the inputs of tests/test_gpu_lane_edges.py ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", ec.EDGE_N_SHORT)
def test_lane_rows_start_tiles_the_rows(N):
    """lane_rows_start restates rows_start (csrc/ibs_wave.hpp, csrc/ibs_group.hpp): the chunks tile [0, n), the first rem lanes hold M
    rows and the others M - 1; the edge lanes and the targets drawn from them are what tests/edge_cases.py says"""
    n = N - 2
    for P in ec.lane_forms(N):
        M = (n + P - 1) // P
        rem = n - P * (M - 1)
        assert 1 <= rem <= P and (P != 64 or M == ec.rows_per_lane(N))
        start = [ec.lane_rows_start(L, n, P) for L in range(P + 1)]
        assert start[0] == 0 and start[P] == n
        assert [b - a for a, b in zip(start, start[1:])] == [M] * rem + [M - 1] * (P - rem), (N, P)
        assert start == [L * (M - 1) + (L if L < rem else rem) for L in range(P + 1)]          # the kernels' own expression
        lanes = ec.lane_edge_lanes(N, P)
        want = {1, rem, rem + 1, P - 1} | {16, 32, 48} | ({8} if P == 16 else set())
        assert lanes == sorted(L for L in want if 1 <= L <= P - 1), (N, P, lanes)
        t = ec.lane_targets(N, P)
        assert len(t) == len(set(t)) and 2 <= len(t) <= 14 and all(1 <= j <= N - 2 for j in t), (N, P, t)
        assert set(t) == {j for L in lanes for j in (start[L], start[L] + 1) if 1 <= j <= N - 2}
        for L in lanes:          # grid point start[L] is row start[L] - 1, the last of lane L - 1; start[L] + 1 the first row of lane L
            assert start[L] - 1 == start[L - 1] + (M if L - 1 < rem else M - 1) - 1
    if N == ec.EDGE_N_SHORT[0]:
        assert sum(len(ec.lane_targets(K, P)) for K in ec.EDGE_N_SHORT for P in ec.lane_forms(K)) == 555
        assert max(len(ec.lane_targets(K)) for K in ec.EDGE_N_SHORT) == 14
        assert ec.lane_targets(2049) == [32, 33, 512, 513, 1024, 1025, 1536, 1537, 2016, 2017]
        assert ec.lane_targets(131, 16) == [9, 10, 17, 18, 65, 66, 121, 122]


def lane_edge_systems(N):
    """[(P, targets)] of a length and the union of the targets (several forms share grid points)"""
    forms = [(P, ec.lane_targets(N, P)) for P in ec.lane_forms(N)]
    return forms, sorted({j for _, t in forms for j in t})


@pytest.mark.parametrize("N", ec.EDGE_N_SHORT)
def test_moving_well_on_lane_edges_keeps_its_gap_and_peaks_on_the_target(N):
    """every (N, P, target) case of tests/test_gpu_lane_edges.py, none left out: the oracle's mode peaks on the target (within 6 points of
    an end for end targets), lam_max lies in [0.149, 0.732] and the second eigenvalue at least 0.39 below it"""
    th = ec.theta_grid(N)
    forms, union = lane_edge_systems(N)
    seen = {}
    for j in union:
        g, c, f = ec.well_rows(th, j)
        gam, lam, X, dX = bo.solve_gcf(th, g, c, f)
        w = ec.top_pairs(th, g, c, f)[0]
        # (the interval and the gap are figures printed to three and two digits: the smallest lam_max is 0.14895 at N = 67, j = 65)
        assert abs(w[1] - lam) < 1e-12 and 0.149 <= round(lam, 3) <= 0.732, (N, j, lam)
        assert round(w[1] - w[0], 2) >= 0.39, (N, j, w)
        seen[j] = int(np.argmax(np.abs(X)))
    for P, targets in forms:
        for j in targets:
            k = seen[j]
            if ec.is_end_target(N, j):
                assert min(k, N - 1 - k) <= 6 and (k < N // 2) == (j < N // 2), (N, P, j, k)
            else:
                assert k == j, (N, P, j, k)


@pytest.mark.parametrize("N", ec.EDGE_N_SHORT)
def test_the_two_oracles_agree_on_the_lane_edge_wells(N):
    """the pattern of test_the_two_oracles_agree_on_the_moving_well on the lane-edge systems, in FP64 and on the FP32-valued inputs
    of the FP32 entry point (g, c, f rounded to float32 and widened, h = float(float32(h))): a tenth of each bound
    tests/test_gpu_lane_edges.py applies -- lam 4 N eps ||A||, gam 1e-10, X 1e-7, dX 1e-7 max|dX| + 1e-7, and for the FP32 eigenvalues
    (N + 3) eps32 ||A||"""
    from oracle import c_oracle as co
    th = ec.theta_grid(N)
    h = float(th[1] - th[0])
    _, union = lane_edge_systems(N)
    rows = [ec.well_rows(th, j) for j in union]
    g, c, f = (np.stack([r[i] for r in rows]) for i in range(3))
    h32, _, (gw, cw, fw), th32 = ec.fp32_inputs(h, g, c, f)
    assert abs((th32[1] - th32[0]) - h32) <= 4 * ec.EPS * h32 and abs(h32 - h) <= 2.0 ** -24 * h
    assert np.array_equal(gw, g) and np.abs(cw - c).max() <= 2.0 ** -24 * np.abs(c).max() and not np.array_equal(cw, c)
    for what, (thx, hx, gx, cx, fx) in (("FP64", (th, h, g, c, f)), ("FP32 values", (th32, h32, gw, cw, fw))):
        nA = ec.norm_a(hx, gx, cx, fx)
        lam_c = co.lam_batch(hx, gx, cx, fx)
        for k, j in enumerate(union):
            gam, lam, X, dX = bo.solve_gcf(thx, gx[k], cx[k], fx[k])
            gc, lc, Xc, dXc = co.solve_gcf(hx, gx[k], cx[k], fx[k])
            assert abs(lam - lc) <= 0.4 * N * ec.EPS * nA[k] and abs(lam - lam_c[k]) <= 0.4 * N * ec.EPS * nA[k], (N, what, j)
            assert abs(lam - lam_c[k]) <= 0.1 * (N + 3) * 2.0 ** -23 * nA[k]
            assert abs(gam - gc) < 1e-11, (N, what, j, gam - gc)
            assert np.abs(X - Xc).max() < 1e-8 and np.abs(dX - dXc).max() < 0.1 * (1e-7 * np.abs(dX).max() + 1e-7), (N, what, j)
            kk = int(np.argmax(np.abs(Xc)))
            assert (min(kk, N - 1 - kk) <= 6) if ec.is_end_target(N, j) else (kk == j), (N, what, j, kk)


def test_check_pair_notices_a_shift_by_one_point_and_one_entry_off():
    """the checker of the GPU tests (tests/test_gpu_edge_lengths.py: check_pair) passes on the reference itself and fails when X is
    the reference shifted by one grid point, or has one entry off by 1e-6"""
    from tests.test_gpu_edge_lengths import check_pair
    N = 259
    th = ec.theta_grid(N)
    for j in ec.lane_targets(N)[:4]:
        g, c, f = ec.well_rows(th, j)
        nA = ec.norm_a(float(th[1] - th[0]), g, c, f)[0]
        ref = bo.solve_gcf(th, g, c, f)
        gam, lam, X, dX = ref
        check_pair(N, "reference", lam, gam, X.copy(), dX.copy(), ref, nA)
        for shift in (1, -1):
            with pytest.raises(AssertionError):
                check_pair(N, "X one point off", lam, gam, X, dX, (gam, lam, np.roll(X, shift), np.roll(dX, shift)), nA)
            Xs = np.roll(X, shift)
            with pytest.raises(AssertionError):
                check_pair(N, "GPU X one point off", lam, gam, Xs, np.roll(dX, shift), ref, nA)
        for k in (j, j + 1, 1, N - 2):
            Xb = X.copy()
            Xb[k] += 1e-6 if k != j else -1e-6                    # (at the peak downwards: max |X| stays one)
            with pytest.raises(AssertionError):
                check_pair(N, "one entry off", lam, gam, Xb, dX, ref, nA)
        dXb = dX.copy()
        dXb[j + 1] += 2 * (1e-7 * np.abs(dX).max() + 1e-7)
        with pytest.raises(AssertionError):
            check_pair(N, "one dX entry off", lam, gam, X, dXb, ref, nA)
