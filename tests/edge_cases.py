"""Grid lengths on lane, chunk and path edges, and two families of raw systems whose mode sits where the caller puts it: the inputs of
tests/test_gpu_edge_lengths.py, pinned with the oracle alone in tests/test_edge_cases_cpu.py, and the lane edges of the register kernels the
same well is put on in tests/test_gpu_lane_edges.py (lane_rows_start, lane_targets); below them the item, tail, block and
ballot edges of the field-line geometry kernels, the inputs of tests/test_gpu_geometry_edges.py.  Test infrastructure only.

Rows per lane of the register kernels: M = ceil((N - 2) / 64), N <= 2050.  Beyond that the long path (csrc/ibs_long.hpp) passes the
n = N - 2 rows through LDS in chunks of 768 (counts) and 384 (pivots, eigenvector, adjoint solve, nearest sigma): the last chunk
holds n mod 768 / n mod 384 rows, the inner loops are unrolled by 8, and the coarse-grid start of long_lam_max needs
(N - 1) % 16 == 0."""
import numpy as np

EPS = 2.220446049250313e-16
LONG_CHUNK, VEC_CHUNK = 768, 384                    # kLongChunk, kVecChunk of csrc/ibs_long.hpp

EDGE_N_SHORT = [
    67, 69,      # smallest odd lengths: the M = 2 branch, 65 / 67 rows = one full register row plus one / three
    99,          # N - 2 = 97: the first length the 32-lane form takes (pick_lanes: 32 * 3 + 1 rows)
    129, 131,    # last length of M = 2, first of M = 3 (the M >= 3 code)
    195,         # M = 4
    257, 259,    # N - 2 = 255 / 257: last length the 16-lane form takes (16 * 16 rows), first without it; M = 4 / 5
    323,         # M = 6
    387,         # M = 7, one row in the last register row
    451,         # M = 8
    577,         # M = 9
    641, 643,    # N - 2 = 639 / 641: last length the 32-lane form takes (32 * 20 rows), first without it; M = 10 / 11
    705,         # M = 11
    707,         # M = 12, one row in the last register row
    833,         # M = 13
    835,         # M = 14, one row in the last register row
    961,         # M = 15
    963,         # M = 16, one row in the last register row
    1089,        # M = 17
    1091,        # M = 18, one row in the last register row
    1217,        # M = 19
    1219,        # M = 20, one row in the last register row
    1283,        # M = 21, one row in the last register row
    1347,        # M = 22, one row in the last register row
    1473,        # M = 23
    1475,        # M = 24, one row in the last register row (first length of the row-streamed raw solve)
    1539,        # M = 25, one row in the last register row
    1603,        # M = 26, one row in the last register row
    1729,        # M = 27
    1731,        # M = 28, one row in the last register row
    1795,        # M = 29, one row in the last register row
    1859,        # M = 30, one row in the last register row
    1985,        # M = 31
    2047, 2049,  # M = 32, three rows short of full and one row short
]
EDGE_N_LONG = [
    2051,        # first long length; n mod 768 = 513, n mod 384 = 129 (both = 1 mod 8); (N - 1) % 16 = 2: two-grid start off
    2305,        # n mod 768 = 767: the last count chunk one row short; two-grid start on
    2307,        # n mod 768 = n mod 384 = 1: one row in the last chunk of both sizes; two-grid start off
    2313,        # the reference's grid rule N = 8 mpol ntor + 1 with mpol = ntor = 17: (N - 1) % 16 = 8, two-grid start off
    2889,        # the same with mpol = ntor = 19: (N - 1) % 16 = 8
    3073,        # n mod 384 = 383: the last vector chunk one row short; two-grid start on
    3075,        # n mod 768 = n mod 384 = 1 again, one count chunk further; two-grid start off
    65535,       # largest odd length below the limit; (N - 1) % 16 = 14: two-grid start off
]
EDGE_N_COUNT = [
    66, 130, 2050,   # even: every lane full (N - 2 = 64 M, M = 1, 2, 32); 66 is the one-row-per-lane sweep
    2052,            # first even long length
    2306, 3074,      # even and long: N - 2 = 3 * 768 and 4 * 768 fill the last chunk exactly
]
# (no (N, target) case is dropped: on every length above the two CPU oracles agree to far less than a tenth of each tolerance the GPU
#  tests apply -- tests/test_edge_cases_cpu.py::test_the_two_oracles_agree_on_the_moving_well)


def rows_per_lane(N):
    return (N - 2 + 63) // 64


def lanes_allowed(N):
    """the lanes-per-system forms pick_lanes (csrc/ibs_plan.hpp) admits at this length besides 64"""
    n = N - 2
    return [P for P, lo, hi in ((32, 97, 640), (16, 49, 256)) if lo <= n <= hi]


def theta_grid(N):
    return np.linspace(-4 * np.pi, 4 * np.pi, N)


def well_rows(theta, j_star, wr=6.0, depth=0.3):
    """(g, c, f) of the moving well: g = 1, f = depth / h^2, c = (depth / h^2) exp(-((j - j_star) / wr)^2) - 0.5 over the grid index
    j.  One Gaussian well, wr grid rows wide, centred on grid point j_star: lam_max is 0.40 ... 0.73, ||A|| about 13.5 and the mode
    peaks on j_star at every N (X is zero at the ends, so a well centred next to an end peaks 4 to 6 points inside)."""
    theta = np.asarray(theta, dtype=np.float64)
    N = len(theta)
    h = theta[1] - theta[0]
    j = np.arange(N, dtype=np.float64)
    a = depth / h ** 2
    return np.ones(N), a * np.exp(-((j - j_star) / wr) ** 2) - 0.5, np.full(N, a)


def two_wells(theta, j_deep, j_shallow, wr=6.0):
    """the moving well of depth 0.3 on j_deep plus one of depth 0.27 on j_shallow (at least 40 rows apart; f as in well_rows): the top
    mode sits on j_deep, the second on j_shallow, the third eigenvalue lies well below both"""
    assert abs(j_deep - j_shallow) >= 40
    g, c, f = well_rows(theta, j_deep, wr, 0.3)
    h = theta[1] - theta[0]
    j = np.arange(len(theta), dtype=np.float64)
    return g, c + (0.27 / h ** 2) * np.exp(-((j - j_shallow) / wr) ** 2), f


def to_geometry(g, c, f, dPdrho=-1.0):
    """the geometry arrays (bmag, gradpar, cvdrift, cvdrift0, gds2, gds21, gds22) whose coefficients (utils.py:1560-1562) are the rows
    (g, c, f): bmag = 1, gradpar = sqrt(g / f), gds2 = g / gradpar, cvdrift = -c gradpar / dPdrho, the theta0 terms zero"""
    g, c, f = (np.asarray(a, dtype=np.float64) for a in (g, c, f))
    gradpar = np.sqrt(g / f)
    z = np.zeros_like(g)
    return np.ones_like(g), gradpar, -c * gradpar / dPdrho, z, g / gradpar, z.copy(), z.copy()


def twist_targets(N, cap=24):
    """the j_star list of a length: grid points 1 and N - 2 (the mode then peaks 4 to 6 points from that end: one direction of the
    twisted split has almost no rows) and, for multiples m of 384 below N - 8, the points m - 1, m, m + 1, m + 2 (the row index is the
    point index minus one, so the twist row lands on and next to a chunk edge counted either way).  At most `cap` per N: the first and
    the last multiples are taken first."""
    ms = list(range(VEC_CHUNK, N - 8, VEC_CHUNK))
    order = []
    lo, hi = 0, len(ms) - 1
    while lo <= hi:
        order.append(ms[lo])
        if hi != lo:
            order.append(ms[hi])
        lo += 1; hi -= 1
    out = [1, N - 2]
    for m in order:
        if len(out) + 4 > cap:
            break
        out += [m - 1, m, m + 1, m + 2]
    return out


def is_end_target(N, j_star):
    return j_star < 6 or j_star > N - 7


def lane_rows_start(L, n, P=64):
    """first row (0-based, row r = grid point r + 1) of lane L when P lanes share the n rows: WaveSolver::rows_start (csrc/ibs_wave.hpp)
    and GroupSolver::rows_start (csrc/ibs_group.hpp) restated with M = ceil(n / P): rem = n - P (M - 1) lanes of M rows, then lanes of
    M - 1 rows; L = P gives n"""
    M = (n + P - 1) // P
    rem = n - P * (M - 1)
    return L * (M - 1) + min(L, rem)


def lane_edge_lanes(N, P=64):
    """the lanes whose first row is an edge of the register kernels: lane 1 and the last lane, the lane where the chunk length drops
    from M to M - 1 and the one after it, the lanes at which the DPP scan changes its step (row_shr within 16 lanes, row_bcast at 16,
    32 and 48), and the middle lane of a 16-lane group; all within 1 ... P - 1"""
    rem = N - 2 - P * ((N - 2 + P - 1) // P - 1)
    lanes = {1, rem, rem + 1, P - 1} | set(range(16, P, 16)) | ({P // 2} if P == 16 else set())
    return sorted(L for L in lanes if 1 <= L <= P - 1)


def lane_targets(N, P=64):
    """the j_star list that puts the twist row of the eigenvector stage on the lane edges of the P-lane register kernels: for every
    lane L of lane_edge_lanes the grid points rows_start(L) (the last row of lane L - 1) and rows_start(L) + 1 (the first row of lane
    L), within 1 ... N - 2, without duplicates: at most 14 per (N, P)"""
    out = []
    for L in lane_edge_lanes(N, P):
        a = lane_rows_start(L, N - 2, P)
        out += [j for j in (a, a + 1) if 1 <= j <= N - 2 and j not in out]
    return out


def lane_forms(N):
    """the lanes-per-system forms whose lane edges a length is tested on: the full wave and what lanes_allowed admits"""
    return [64] + lanes_allowed(N)


def fp32_inputs(h, g, c, f):
    """what the FP32 entry point sees: (h, g, c, f) rounded to float32, and the same values widened again -- (h32, (g, c, f) as
    float32 arrays, (g, c, f) as float64 arrays, a theta grid whose spacing is h32) -- the reference of an FP32 call solves THESE"""
    h32 = float(np.float32(h))
    r32 = tuple(np.ascontiguousarray(a, dtype=np.float32) for a in (g, c, f))
    N = r32[0].shape[-1]
    return h32, r32, tuple(a.astype(np.float64) for a in r32), np.linspace(-0.5 * h32 * (N - 1), 0.5 * h32 * (N - 1), N)


def norm_a(h, g, c, f):
    """the solver's bound on ||A||: max over the rows of (|d| + e_lo + e_hi) / f (utils.py:1574-1592 with the half-grid g the mean of
    neighbours); g, c, f (n_sys, N)"""
    g, c, f = (np.atleast_2d(np.asarray(a, dtype=np.float64)) for a in (g, c, f))
    ee = (g[:, :-2] + 2 * g[:, 1:-1] + g[:, 2:]) / (2 * h * h)
    return ((np.abs(c[:, 1:-1] - ee) + ee) / f[:, 1:-1]).max(axis=1)


def top_pairs(theta, g, c, f, k=2):
    """(w, V): the k largest eigenvalues of the pencil (ascending) and their vectors as grid functions (N, k) with zero ends, by LAPACK
    on the symmetrised tridiagonal (as bo.top_eigenpair); any N, even lengths included"""
    from scipy.linalg import eigh_tridiagonal
    from oracle import ballooning_oracle as bo
    d, e, fd = bo.assemble(theta, g, c, f)[:3]
    n = len(d)
    w, v = eigh_tridiagonal(d / fd, e[1:n] / np.sqrt(fd[:-1] * fd[1:]), select="i", select_range=(n - k, n - 1))
    V = np.zeros((n + 2, k))
    V[1:-1] = v / np.sqrt(fd)[:, None]
    return w, V


# ---- field-line geometry (csrc/ibs_geometry.hip, csrc/ibs_geometry_vjp.hip): the inputs of tests/test_gpu_geometry_edges.py ----------
# A wave-item of k_geo_rows<PPL, LPP, MAXR> is 64 PPL / LPP consecutive grid points of one line, a unit eight items of one line (one
# per wave of a 512-thread block).  launch_geometry hands the rem = N % pts points beyond a multiple of the item to the
# one-point-per-wave tail kernel only if LPP == 1, 0 < rem <= 16 and N > pts; otherwise the last item of a line is partial.
GEO_FORMS = {"1": (1, 1), "-2": (2, 1), "2": (1, 2), "4": (1, 4), "8": (1, 8)}     # option geo_lpp -> (PPL, LPP)
GEO_TAIL_MAX = 16
GEO_WAVES_PER_BLOCK = 8
GEO_PTS = sorted({64 * p // l for p, l in GEO_FORMS.values()})                     # 8, 16, 32, 64, 128


def geo_dispatch(N, ppl, lpp):
    """launch_geometry's arithmetic for one line of N points in the form (ppl, lpp): item size, remainder, the points the tail kernel
    takes, the end of the row kernel's range, and the row kernel's items and units per line"""
    pts = 64 * ppl // lpp
    rem = N % pts
    tail = rem if (lpp == 1 and 0 < rem <= GEO_TAIL_MAX and N > pts) else 0
    j_end = N - tail
    items = (j_end + pts - 1) // pts
    return dict(pts=pts, rem=rem, tail=tail, j_end=j_end, items=items, units=(items + GEO_WAVES_PER_BLOCK - 1) // GEO_WAVES_PER_BLOCK,
                spare=(-items) % GEO_WAVES_PER_BLOCK, last=j_end - (items - 1) * pts)


def geo_pick_form(n_lines, N, n_cu, lpp_opt=0):
    """geo_pick_form: the option if set, else the smallest item that gives none of the 8 n_cu wave slots a second item"""
    if str(lpp_opt) in GEO_FORMS:
        return GEO_FORMS[str(lpp_opt)]
    pts, slots = n_lines * N, 8 * n_cu
    for k, form in ((64, (2, 1)), (32, (1, 1)), (16, (1, 2)), (8, (1, 4))):
        if pts > slots * k:
            return form
    return (1, 8)


def geo_kernel_name(ppl, lpp, nrows_mn=11):
    """what ibs_last_launch reports for the row kernel of a form (tables of more than 12 rows run <1, 1, 24> whatever the form)"""
    return "ibs::k_geo_rows<1, 1, 24>" if nrows_mn > 12 else "ibs::k_geo_rows<%d, %d, 12>" % (ppl, lpp)


def geo_threshold_lines(N, n_cu):
    """[(points per wave slot k, line count just below, line count just above)]: the largest n_lines with n_lines N <= 8 n_cu k (the
    form of the smaller item still serves it) and the next one, for the four thresholds of geo_pick_form"""
    return [(k, (8 * n_cu * k) // N, (8 * n_cu * k) // N + 1) for k in (8, 16, 32, 64)]


GEO_EDGE_REASONS = {
    -1: "pts - 1: one item, one lane (lane group) short of full; N < pts, so no tail kernel in any form",
    0: "pts: exactly one full item, rem = 0",
    1: "pts + 1: rem = 1; one lane per point: the tail kernel takes one point; else a second item with one live point",
    16: "pts + 16: rem = 16, the most the tail kernel takes",
    17: "pts + 17: rem = 17, the first remainder that stays a partial item in every form",
}
GEO_EDGE_REASONS_8 = {
    0: "8 pts: exactly one unit per line, no spare item, rem = 0",
    1: "8 pts + 1: one lane per point: the tail kernel keeps the line at 8 items; else 9 items = two units, seven spare items",
    17: "8 pts + 17: two units in every form, the second with one item (two / three with items of 16 / 8 points), the last one partial",
}
GEO_EDGE_N = sorted(
    {pts + d for pts in GEO_PTS for d in GEO_EDGE_REASONS} | {8 * pts + d for pts in GEO_PTS for d in GEO_EDGE_REASONS_8}
    | {2, 3,     # the shortest grids the entry point takes: two and three live points in the only item
       7,        # one point short of the smallest item
       66})      # an even length that is no edge of any item size (the lists above hold even lengths on the edges)
GEO_EDGE_SURF = [1, 0, 1, 1, 0]                       # two surfaces, the staged image changes on every line but one
GEO_EDGE_ALPHA = [0.3, 2.9, 1.1, 0.0, 2.2]

# alpha and theta outside [0, pi] and off the symmetric window (the kernels see theta[j] and alpha only through
# phi = (theta - alpha) / iota and the root solve started at theta)
GEO_WINDOWS = [(-4 * np.pi, 4 * np.pi),               # the scan's window
               (2 * np.pi, 10 * np.pi),               # all theta > 0: |phi| up to ~70, the angles m theta - n phi up to ~2e3
               (-np.pi, np.pi)]                       # one poloidal turn
GEO_ALPHAS = [-3 * np.pi, -7.3, 0.0, np.pi, 9.1]      # negative, beyond one turn, and the two ends of the box tested so far
GEO_WINDOW_N = [131, 65]                              # 65 = 64 + 1: a tail point for LPP = 1, N < pts for two points per lane
GEO_WINDOW_FORMS = ["1", "-2", "4"]


def geo_nonuniform_grid(N=131, seed=5):
    """an increasing grid on [-4 pi, 4 pi] with spacings between 0.2 and 1.8 of the uniform one"""
    rng = np.random.default_rng(seed)
    d = rng.uniform(0.2, 1.8, N - 1)
    return -4 * np.pi + 8 * np.pi * np.concatenate([[0.0], np.cumsum(d)]) / d.sum()


# many lines on alternating surfaces: (n_lines, N); more units than an MI355X has CUs (256) in both forms, so blocks own two or three
# lines and re-stage on every unit
GEO_MANY = [(700, 67),      # one item per line; one lane per point: 64 points + 3 tail points, two points per lane: N < pts
            (300, 145)]     # rem = 17 in both forms: 3 / 2 items, the last one partial
GEO_MANY_FORMS = ["1", "-2"]
GEO_PITCH = [(145, 150), (67, 72)]                    # (N, ld = N + 5)
GEO_MARK = dict(n_surf=40, first=[3, 39, 17, 3, 39], second=[0, 5, 5, 0, 5])      # k_geo_mark: n_surf >= 32, n_lines < 8 n_surf

# VJP: for_points_of_surface ballots line_surf 64 entries at a time; k_geo_vjp_modes gives a wave 8 modes and a block 4 waves
GEO_VJP_G = 8
GEO_VJP_LINES = [63, 64, 65, 130]      # one word one short, one word full, a second word with one entry, a third word
GEO_VJP_LINES_N = 35
GEO_VJP_N = [2, 63, 64, 65]            # the points of a line are strided over 64 lanes: two lanes, one short, full, one lane twice
GEO_VJP_MODES = {"odd_groups": (41, 50),   # 6 + 7 = 13 groups: the last block of k_geo_vjp_modes has one wave with work
                 "few": (7, 7)}            # fewer than 8 modes in each table: min(k0 + g, n - 1) clamps in the only group


def geo_vjp_line_surf(n_lines):
    """four surfaces: surface 1 holds no line, surface 3 only lines at index >= 64 (the even ones), surface 2 every third line below
    64 and the odd ones from 64 on (both sides of a ballot word), surface 0 the rest"""
    i = np.arange(n_lines)
    return np.where(i >= 64, np.where(i % 2 == 0, 3, 2), np.where(i % 3 == 0, 2, 0)).astype(np.int32)


def geo_vjp_line_alpha(n_lines):
    return np.linspace(-3 * np.pi, 3 * np.pi, n_lines)


def geo_vjp_groups(mnmax, mnmax_nyq):
    return (mnmax + GEO_VJP_G - 1) // GEO_VJP_G + (mnmax_nyq + GEO_VJP_G - 1) // GEO_VJP_G


# ---- Sturm counts across the spectrum and across input magnitudes: the inputs of tests/test_count_spectrum_cpu.py and
# tests/test_gpu_count_spectrum.py ------------------------------------------------------------------------------------------------------
# The prefix-product sweep k_sturm_count (csrc/ibs_kernels.hip) runs the three-term recurrence u[r+1] = -(d - sig f) u[r] - e^2 u[r-1]
# over a lane's M = ceil((N - 2) / 64) rows; its magnitudes grow like max(|d - sig f|, e)^rows between two renormalisations, so what it
# can be fed depends on the units of (g, c) and on where in the spectrum the shift lies.
COUNT_N_CPU = [
    67,      # M = 2
    513,     # M = 8
    1025,    # M = 16
    2049,    # M = 32
    2050,    # even, every lane full (count only)
    2051,    # first long grid: division forms only
]
COUNT_N_GPU = [67, 513, 2049, 2050, 2051]
COUNT_N_GEO = [513, 2049]
COUNT_SCALES = [(-40, 0), (-12, 0), (0, 0), (8, 0), (12, 0), (16, 0), (40, 0),      # (k, m): (g, c) 2^k, f 2^m
                (0, 20)]     # f alone: it enters the recurrence only through sig f, so this case must behave like (0, 0)
COUNT_SCALES_GEO = [(-12, 0), (0, 0), (16, 0)]
COUNT_FAMILIES = ["salpha", "well", "rough"]
COUNT_ROUGH_SEED = 5         # (see count_family_rows)
COUNT_NEAR = 32              # a target's qualifying gap lies within this many indices of it


def count_targets(N):
    """the indices k (count of eigenvalues above the probe shift) asked for at a length: the top of the spectrum, a few below it, the
    quarters and the bottom"""
    n = N - 2
    return [1, 2, 3, 8, 64, n // 4, n // 2, 3 * n // 4, n - 1]


def all_eigenvalues(theta, g, c, f):
    """every eigenvalue of the pencil, ascending, by LAPACK on the symmetrised tridiagonal (as top_pairs)"""
    from scipy.linalg import eigh_tridiagonal
    from oracle import ballooning_oracle as bo
    d, e, fd = bo.assemble(theta, g, c, f)[:3]
    n = len(d)
    return eigh_tridiagonal(d / fd, e[1:n] / np.sqrt(fd[:-1] * fd[1:]), eigvals_only=True)


def count_probe_shifts(h, g, c, f, targets, near=COUNT_NEAR):
    """(shifts, counts, used): for each target index k the midpoint of the gap below the k-th largest eigenvalue (count there: k), then
    one shift 0.01 ||A|| below the spectrum (count n = N - 2) and one as far above it (count 0).  A midpoint is used only if the
    half-gap is at least 8 N^2 eps ||A|| (eight times the worst case DESIGN section 7 states for the sweep next to an eigenvalue of iid
    rows: both count forms are exact there); where a target's own gap is narrower the nearest index whose gap qualifies takes its
    place, and none within `near` indices is an error.  `used` lists the index taken for each target."""
    g, c, f = (np.asarray(a, dtype=np.float64) for a in (g, c, f))
    N = len(g)
    n = N - 2
    theta = h * (np.arange(N) - 0.5 * (N - 1))
    w = all_eigenvalues(theta, g, c, f)[::-1]                 # descending: w[k - 1] is the k-th largest
    nA = float(norm_a(h, g, c, f)[0])
    need = 8.0 * N * N * EPS * nA
    half = 0.5 * (w[:-1] - w[1:])                             # half[k - 1]: half of the gap below the k-th largest, k = 1 ... n - 1
    shifts, counts, used = [], [], []
    for k in targets:
        assert 1 <= k <= n - 1, (N, k)
        cand = sorted((kk for kk in range(max(1, k - near), min(n - 1, k + near) + 1) if half[kk - 1] >= need), key=lambda kk: (abs(kk - k), kk))
        assert cand, "no half-gap of 8 N^2 eps ||A|| within %d indices of target %d at N = %d" % (near, k, N)
        kk = cand[0]
        shifts.append(0.5 * (w[kk - 1] + w[kk])); counts.append(kk); used.append(kk)
    shifts += [w[-1] - 0.01 * nA, w[0] + 0.01 * nA]
    counts += [n, 0]
    return np.array(shifts), np.array(counts, dtype=np.int32), used


def scaled_rows(g, c, f, k, m):
    """(g 2^k, c 2^k, f 2^m): exact scalings, the spectrum scales by exactly 2^(k - m)"""
    return np.ldexp(np.asarray(g, dtype=np.float64), k), np.ldexp(np.asarray(c, dtype=np.float64), k), np.ldexp(np.asarray(f, dtype=np.float64), m)


def count_family_rows(N, family):
    """one system of each family of the count tests: (theta, g, c, f)"""
    from oracle import ballooning_oracle as bo
    th = theta_grid(N)
    if family == "salpha":                       # s-alpha (shat, alpha, theta0) = (1.0, 0.8, 0.3), f = g
        g, c = bo.salpha_gc(th, 1.0, 0.8, 0.3)
        return th, g, c, g.copy()
    if family == "well":                         # the moving well on the last target of the length
        return (th,) + tuple(well_rows(th, twist_targets(N)[-1]))
    # iid per point inside the envelopes of BASELINE configs[4], drawn UNIFORMLY in each: with the log-uniform draw of bench.py the top
    # ~150 eigenvalues at N = 2049 lie within 1e-3 of each other just below zero (rows of large f) while the gap rule of
    # count_probe_shifts asks for 0.04 there, whatever the seed; with uniform draws most seeds qualify at every length (this one: a
    # qualifying gap within 0 / 0 / 5 / 16 / 14 / 27 indices of every target at N = 67 ... 2051, min f = 0.21 ... 24, ||A|| up to 1e6)
    assert family == "rough"
    rng = np.random.default_rng([COUNT_ROUGH_SEED, N])
    return th, rng.uniform(0.01, 50.0, N), rng.uniform(-2.5, 3.5, N), rng.uniform(0.2, 3e3, N)


_COUNT_CASES = {}


def count_cases(N):
    """{family: (h, (g, c, f), shifts, counts, used)} of a length on the unscaled rows, computed once and shared (read only)"""
    if N not in _COUNT_CASES:
        out = {}
        for fam in COUNT_FAMILIES:
            th, g, c, f = count_family_rows(N, fam)
            h = float(th[1] - th[0])
            out[fam] = (h, (g, c, f)) + count_probe_shifts(h, g, c, f, count_targets(N))
        _COUNT_CASES[N] = out
    return _COUNT_CASES[N]


def count_batch(N, k, m):
    """the batch of one (N, scale): every family's rows repeated for each of its eleven shifts, scaled by (k, m), with the shifts
    scaled by 2^(k - m): (h, g, c, f, shift, count), 33 systems in the order of COUNT_FAMILIES"""
    G, Cc, F, S, K = [], [], [], [], []
    h = None
    for fam in COUNT_FAMILIES:
        h, rows, shifts, counts, _ = count_cases(N)[fam]
        g, c, f = scaled_rows(*rows, k, m)
        for s, cnt in zip(shifts, counts):
            G.append(g); Cc.append(c); F.append(f); S.append(np.ldexp(s, k - m)); K.append(cnt)
    return h, np.stack(G), np.stack(Cc), np.stack(F), np.array(S), np.array(K, dtype=np.int32)
