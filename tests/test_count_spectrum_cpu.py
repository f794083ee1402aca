"""CPU: the inputs of tests/test_gpu_count_spectrum.py pinned without a GPU (tests/edge_cases.py: count_probe_shifts, scaled_rows,
count_batch), and the lane arithmetic of the prefix-product sweep k_sturm_count (csrc/ibs_kernels.hip) restated in numpy.

Every expected count comes from two independent methods: LAPACK's eigenvalues of the symmetrised pencil (the shift is the midpoint of
a gap of at least 16 N^2 eps ||A||, so the count is the index of the gap) and the C oracle's division-form count on the SCALED rows.

The restatement follows the kernel operation for operation except for the fused multiply-adds (numpy rounds the product first; the
probe shifts sit far enough from every eigenvalue that this cannot move a count): the rows of a lane from lane_rows_start, the
un-normalised chunk transfer matrix, the 2x2 scan with the kernel's own pattern of normalised and un-normalised steps, and the replay
that counts sign changes from the incoming pair.  `every` is the number of rows between two exact power-of-two renormalisations
inside a lane: None restates the sweep as it was before it renormalised there (one renormalisation after the whole chunk), RENORM_ROWS
restates it as it is: the chunk product is multiplied after rows 7, 15, 23 by 2^-ex, ex the exponent of its largest entry `lag` rows
earlier (the kernel folds the factor into the row's coefficients, which is the same arithmetic: powers of two commute with every
rounding), and the replay is multiplied by the same factors.  The restatement records the largest and smallest magnitude a lane produces and whether any value left the
normal FP64 range (non-finite, subnormal, or a zero out of non-zero operands)."""
import numpy as np
import pytest

from oracle import c_oracle as co
from tests import edge_cases as ec

RENORM_ROWS = 8                  # kSturmRenormRows of csrc/ibs_kernels.hip
RENORM_LAG = 2                   # kSturmRenormLag
TINY = 2.2250738585072014e-308   # DBL_MIN
SCALES = ec.COUNT_SCALES


class Range:
    """largest and smallest non-zero magnitude seen, and whether anything left the normal range"""

    def __init__(self):
        self.hi, self.lo, self.left = 0.0, np.inf, False

    def see(self, x, lost_zero=None):
        ax = np.abs(x)
        if not np.isfinite(ax).all():
            self.left = True
        fin = ax[np.isfinite(ax) & (ax > 0)]
        if fin.size:
            self.hi, self.lo = max(self.hi, float(fin.max())), min(self.lo, float(fin.min()))
            if fin.min() < TINY:
                self.left = True
        if lost_zero is not None and lost_zero.any():
            self.left = True

    def decades(self):
        return (np.log10(self.hi) if self.hi > 0 else -np.inf, np.log10(self.lo) if np.isfinite(self.lo) else np.inf)


def step(t, e2, zc, zp, rng):
    """zn = -t zc - e2 zp with the range bookkeeping: a zero out of non-zero operands is an underflow"""
    zn = -t * zc - e2 * zp
    rng.see(zn, lost_zero=(zn == 0) & (((t != 0) & (zc != 0)) | ((e2 != 0) & (zp != 0))))
    return zn


def norm_common(vals):
    """the values divided by 2^ex, ex the binary exponent of the largest magnitude among them (muls(..., true): frexp_exp + ldexp;
    the hardware returns exponent 0 for zero and for non-finite values, as numpy's frexp does)"""
    m = np.abs(vals[0])
    for v in vals[1:]:
        m = np.maximum(m, np.abs(v))
    ex = np.frexp(m)[1]
    return [np.ldexp(v, -ex) for v in vals]


def mul2(A, B):
    """2x2 product of (a, b, c, d) tuples, elementwise over the leading axes"""
    a, b, c, d = A
    p, q, r, s = B
    return [a * p + b * r, a * q + b * s, c * p + d * r, c * q + d * s]


def lane_rows(h, g, c, f, sig):
    """(t, e2, act): t = d - sig f and e_lo^2 of every lane's rows, padded to M per lane with zeros as the kernel pads them;
    t, e2 (S, 64, M), act (64, M)"""
    N = len(g)
    n, M = N - 2, ec.rows_per_lane(N)
    ih2 = 1.0 / (h * h)
    e = 0.5 * (g[:-1] + g[1:]) * ih2                         # e[k] couples grid points k and k + 1
    d = c[1:-1] - (e[:n] + e[1:n + 1])
    t_all = d[None, :] - sig[:, None] * f[1:-1][None, :]
    e2_all = e[:n] ** 2
    start = [ec.lane_rows_start(L, n) for L in range(65)]
    S = len(sig)
    t = np.zeros((S, 64, M)); e2 = np.zeros((S, 64, M)); act = np.zeros((64, M), dtype=bool)
    for L in range(64):
        a, cnt = start[L], start[L + 1] - start[L]
        assert cnt in (M, M - 1)
        t[:, L, :cnt] = t_all[:, a:a + cnt]; e2[:, L, :cnt] = e2_all[a:a + cnt][None]; act[L, :cnt] = True
    return t, e2, act


def sweep_restated(h, g, c, f, sig, every, lag=RENORM_LAG):
    """the count of k_sturm_count<double, M> at every shift of sig (S,), and the Range of everything its lanes produced"""
    N = len(g)
    M = ec.rows_per_lane(N)
    assert N <= 2050
    sig = np.asarray(sig, dtype=np.float64)
    S = len(sig)
    rng = Range()
    with np.errstate(all="ignore"):
        t, e2, act = lane_rows(h, g, c, f, sig)
        # chunk transfer matrix
        fA, fAp, fB, fBp = np.ones((S, 64)), np.zeros((S, 64)), np.zeros((S, 64)), np.ones((S, 64))
        scale = []                                            # the powers of two the chunk product was multiplied by, in order
        for i in range(M):
            on = act[:, i][None]
            nA, nB = step(t[:, :, i], e2[:, :, i], fA, fAp, rng), step(t[:, :, i], e2[:, :, i], fB, fBp, rng)
            fAp, fBp = np.where(on, fA, fAp), np.where(on, fB, fBp)
            fA, fB = np.where(on, nA, fA), np.where(on, nB, fB)
            if every and (i + lag) % every == every - 1 and i + lag + 1 < M:      # the scale row i + lag applies: from the state after row i
                m = np.maximum(np.maximum(np.abs(fA), np.abs(fAp)), np.maximum(np.abs(fB), np.abs(fBp)))
                scale.append(np.ldexp(1.0, -np.frexp(m)[1]))
            if every and i % every == every - 1 and i + 1 < M:
                fA, fAp, fB, fBp = (v * scale[i // every] for v in (fA, fAp, fB, fBp))
        P = norm_common([fA, fB, fAp, fBp])
        # the scan: row_shr 1, 2, 4, 8 within 16 lanes, then lane 15 of the row before into rows 1 and 3, lane 31 into rows 2 and 3;
        # every second step normalised
        lane = np.arange(64)
        l16, rw = lane & 15, lane >> 4

        def scan_step(P, src, take, norm):
            F = [np.where(src[None] >= 0, p[:, np.maximum(src, 0)], 0.0) for p in P]
            R = mul2(P, F)
            for r in R:
                rng.see(r[:, take])
            if norm:
                R = norm_common(R)
            return [np.where(take[None], r, p) for r, p in zip(R, P)]
        for sh, norm in ((1, False), (2, True), (4, False), (8, True)):
            P = scan_step(P, np.where(l16 >= sh, lane - sh, -1), l16 >= sh, norm)
        P = scan_step(P, np.where(rw & 1, (rw - 1) * 16 + 15, -1), (rw & 1) == 1, False)
        P = scan_step(P, np.where(rw >= 2, 31, -1), rw >= 2, True)
        # incoming pair of every lane: first column of the left neighbour's inclusive product, (1, 0) at the left end
        zc = np.concatenate([np.ones((S, 1)), P[0][:, :-1]], axis=1)
        zp = np.concatenate([np.zeros((S, 1)), P[2][:, :-1]], axis=1)
        has_last = act[:, M - 1]
        ncount = np.where(has_last, M, M - 1) - np.where(lane == 63, 0, 1)
        cnt = (np.signbit(zc) != np.signbit(zp)).sum(axis=1)
        for i in range(M):
            on = act[:, i][None]
            zn = step(t[:, :, i], e2[:, :, i], zc, zp, rng)
            flip = ((i < M - 2) | (i < ncount))[None] & (np.signbit(zn) != np.signbit(zc))
            cnt = cnt + flip.sum(axis=1)
            zp = np.where(on, zc, zp); zc = np.where(on, zn, zc)
            if every and i % every == every - 1 and i + 1 < M:          # the replay takes the chunk product's scales
                zc, zp = zc * scale[i // every], zp * scale[i // every]
    return cnt.astype(np.int32), rng


def scaled_row_chunk_range(h, g, c, f, sig):
    """the magnitudes of the chunk product of WaveSolver::sweep_fwd (csrc/ibs_wave.hpp): rows scaled so that the off-diagonals are 1
    (s_0 = 1 in every lane, e s_i s_{i+1} = 1), D = d s^2, Ph = f s^2, tf = D - sig Ph, u[r+1] = -tf u[r] - u[r-1].  The two columns
    of the chunk product are the replay from the incoming pairs (1, 0) and (0, 1); the replay from any normalised pair stays within
    twice their magnitudes."""
    N = len(g)
    n, M = N - 2, ec.rows_per_lane(N)
    sig = np.asarray(sig, dtype=np.float64)
    S = len(sig)
    rng = Range()
    with np.errstate(all="ignore"):
        ih2 = 1.0 / (h * h)
        e = 0.5 * (g[:-1] + g[1:]) * ih2
        d = c[1:-1] - (e[:n] + e[1:n + 1])
        start = [ec.lane_rows_start(L, n) for L in range(65)]
        fA, fAp, fB, fBp = np.ones((S, 64)), np.zeros((S, 64)), np.zeros((S, 64)), np.ones((S, 64))
        sc = np.ones(64)
        for i in range(M):
            r = np.array([start[L] + i for L in range(64)])
            on = np.array([start[L] + i < start[L + 1] for L in range(64)])
            r = np.where(on, r, 0)
            s2 = sc * sc
            D, Ph = d[r] * s2, f[1:-1][r] * s2
            rng.see(D[on]); rng.see(Ph[on])
            tf = D[None] - sig[:, None] * Ph[None]
            nA, nB = -tf * fA - fAp, -tf * fB - fBp
            rng.see(nA[:, on]); rng.see(nB[:, on])
            fAp, fBp = np.where(on[None], fA, fAp), np.where(on[None], fB, fBp)
            fA, fB = np.where(on[None], nA, fA), np.where(on[None], nB, fB)
            sc = np.where(on, 1.0 / (e[r + 1] * sc), sc)
            rng.see(sc[on])
    return rng


_RECORD = {}


def record(N):
    """per (family, (k, m)): the oracle-confirmed batch and both restatements' results at a length, computed once"""
    if N not in _RECORD:
        out = {}
        for k, m in SCALES:
            h, g, c, f, shift, want = ec.count_batch(N, k, m)
            conf = co.count_above_batch(h, g, c, f, shift)
            for j, fam in enumerate(ec.COUNT_FAMILIES):
                sl = slice(11 * j, 11 * j + 11)
                row = dict(h=h, rows=(g[sl.start], c[sl.start], f[sl.start]), shift=shift[sl], want=want[sl], oracle=conf[sl])
                if N <= 2050:
                    row["old"] = sweep_restated(h, *row["rows"], row["shift"], None)
                    row["new"] = sweep_restated(h, *row["rows"], row["shift"], RENORM_ROWS)
                out[fam, (k, m)] = row
        _RECORD[N] = out
    return _RECORD[N]


@pytest.mark.parametrize("N", ec.COUNT_N_CPU)
def test_every_target_has_a_qualifying_gap_and_both_methods_agree(N):
    """no target dropped: every family has a gap of half-width >= 8 N^2 eps ||A|| within 32 indices of each target (count_probe_shifts
    asserts it), the counts are what the target list says up to that move, and the C oracle's division-form count of the SCALED rows
    at the SCALED shift equals the index of the gap at every scale"""
    n = N - 2
    targets = ec.count_targets(N)
    assert len(targets) == 9 and targets[:5] == [1, 2, 3, 8, 64] and targets[-1] == n - 1
    for fam in ec.COUNT_FAMILIES:
        h, rows, shifts, counts, used = ec.count_cases(N)[fam]
        assert len(shifts) == len(counts) == 11 and list(counts[:9]) == used and counts[9] == n and counts[10] == 0
        assert all(abs(u - k) <= ec.COUNT_NEAR for u, k in zip(used, targets)), (N, fam, used)
        print("count-spectrum targets: N=%d %-6s asked %s taken %s" % (N, fam, targets, used))
        # the gaps really are that wide, measured on the eigenvalues themselves
        w = ec.all_eigenvalues(ec.theta_grid(N), *rows)[::-1]
        nA = ec.norm_a(h, *rows)[0]
        for s, k in zip(shifts[:9], counts[:9]):
            assert w[k - 1] - s >= 8 * N * N * ec.EPS * nA and s - w[k] >= 8 * N * N * ec.EPS * nA and (w > s).sum() == k
        assert shifts[9] < w[-1] and shifts[10] > w[0]
    for (fam, km), row in record(N).items():
        assert np.array_equal(row["oracle"], row["want"]), (N, fam, km, row["oracle"], row["want"])


def test_scaled_rows_are_exact_powers_of_two():
    th, g, c, f = ec.count_family_rows(513, "rough")
    for k, m in SCALES:
        gs, cs, fs = ec.scaled_rows(g, c, f, k, m)
        assert np.array_equal(gs * 2.0 ** -k, g) and np.array_equal(cs * 2.0 ** -k, c) and np.array_equal(fs * 2.0 ** -m, f)
    assert [s for s in SCALES if s[1]] == [(0, 20)] and sorted(k for k, m in SCALES if m == 0) == [-40, -12, 0, 8, 12, 16, 40]
    h, G, C_, F, S, K = ec.count_batch(513, 12, 0)
    h0, G0, C0, F0, S0, K0 = ec.count_batch(513, 0, 0)
    assert G.shape == (33, 513) and np.array_equal(G, 4096 * G0) and np.array_equal(S, 4096 * S0) and np.array_equal(K, K0) and h == h0
    assert {ec.rows_per_lane(N) for N in ec.COUNT_N_CPU if N <= 2050} == {2, 8, 16, 32} and (2050 - 2) % 64 == 0 and 2051 in ec.COUNT_N_CPU
    assert set(ec.COUNT_N_GPU) <= set(ec.COUNT_N_CPU) and set(ec.COUNT_N_GEO) <= set(ec.COUNT_N_GPU)


@pytest.mark.parametrize("N", [N for N in ec.COUNT_N_CPU if N <= 2050])
def test_restated_sweep_stays_in_range_and_counts_exactly(N):
    """the sweep as it is (rescaled every RENORM_ROWS rows inside a lane, the scale RENORM_LAG rows old): every value of every lane stays in the normal FP64
    range on every (family, scale, shift) of the list, and the count is the oracle's.  The sweep as it was is run alongside for the
    record (docs/EXPERIMENTS.md): where its lanes stayed in range it must count exactly too -- the renormalisation changes no sign."""
    for (fam, km), row in record(N).items():
        cnt_old, r_old = row["old"]
        cnt_new, r_new = row["new"]
        print("count-spectrum magnitudes: N=%d M=%d %-6s (g, c) 2^%d f 2^%d   one renormalisation per chunk: 1e%+.0f .. 1e%+.0f %s, %d of 11 "
              "counts wrong   every %d rows, lag %d: 1e%+.0f .. 1e%+.0f %s, %d wrong"
              % (N, ec.rows_per_lane(N), fam, km[0], km[1], r_old.decades()[1], r_old.decades()[0], "LEFT THE RANGE" if r_old.left else "in range",
                 int((cnt_old != row["want"]).sum()), RENORM_ROWS, RENORM_LAG, r_new.decades()[1], r_new.decades()[0], "LEFT THE RANGE" if r_new.left else "in range",
                 int((cnt_new != row["want"]).sum())))
        assert not r_new.left, (N, fam, km, r_new.decades())
        assert np.array_equal(cnt_new, row["want"]), (N, fam, km, cnt_new, row["want"])
        if not r_old.left:
            assert np.array_equal(cnt_old, row["want"]), (N, fam, km, cnt_old, row["want"])
    # f alone scaled: the recurrence sees f only through sig f, which is unchanged
    for fam in ec.COUNT_FAMILIES:
        a, b = record(N)[fam, (0, 0)]["new"], record(N)[fam, (0, 20)]["new"]
        assert np.array_equal(a[0], b[0]) and abs(a[1].decades()[0] - b[1].decades()[0]) < 0.01 and abs(a[1].decades()[1] - b[1].decades()[1]) < 0.01


def test_the_sweep_without_renormalisation_inside_a_lane_overflows_on_scaled_rows():
    """why the sweep renormalises inside a lane: at 32 rows per lane the s-alpha rows in units 4096 times smaller ((g, c) 2^12)
    overflow the un-normalised chunk product and counts come back wrong with no status"""
    cnt, rng = record(2049)["salpha", (12, 0)]["old"]
    assert rng.left and (cnt != record(2049)["salpha", (12, 0)]["want"]).any()
    cnt, rng = record(2049)["salpha", (0, 0)]["old"]
    assert not rng.left and rng.decades()[0] > 150


@pytest.mark.parametrize("N", [N for N in ec.COUNT_N_CPU if N <= 2050])
def test_scaled_row_sweep_magnitudes(N):
    """the scaled-row forward sweep of the solvers (WaveSolver::sweep_fwd) on the same inputs, shifts at both Gershgorin ends
    (-||A||, +||A||): every value stays in the normal range at every scale"""
    for fam in ec.COUNT_FAMILIES:
        base = None
        for k, m in SCALES:
            h, rows = ec.count_cases(N)[fam][:2]
            g, c, f = ec.scaled_rows(*rows, k, m)
            nA = ec.norm_a(h, g, c, f)[0]
            rng = scaled_row_chunk_range(h, g, c, f, np.array([-nA, nA]))
            hi, lo = rng.decades()
            if (k, m) == (0, 0):
                base = (hi, lo)
            print("scaled-row sweep magnitudes: N=%d M=%d %-6s (g, c) 2^%d f 2^%d   1e%+.0f .. 1e%+.0f %s"
                  % (N, ec.rows_per_lane(N), fam, k, m, lo, hi, "LEFT THE RANGE" if rng.left else "in range"))
            assert not rng.left, (N, fam, k, m, hi, lo)
        assert base is not None
