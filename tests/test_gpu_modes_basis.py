"""GPU: the spectrum mode with an F-orthonormal Ritz basis of every cluster (ibs_solve_gcf_modes_basis_f64,
Context.solve_gcf_modes(basis=True), autograd.solve_gcf_modes(cluster="mean")) against the contract of tests/modes_basis_oracle.py:
(a) residual, (b) F-orthogonality, (c) the Ritz property, (d) the distance from the reference subspace of tight clusters, (e) gam;
(f) identity with ibs_solve_gcf_modes_f64 outside the clusters; (g) bitwise repeatability and independence of the batch -- of a batch
of four times the persistent grid as well, where every wave serves four systems from one slice of workspace.

Every test recomputes the reference clusters with scipy and asserts its own precondition -- the clusters it is about are at most
tau / 8 wide and at least 2 tau from the rest of the spectrum -- before it looks at the GPU's output.  Groups the oracle finds
barely clustered (between tau / 8 and a few tau: the fourth to eighth modes of some wells at N >= 2,049) are held to (a)-(c)."""
import ctypes
import os
import warnings

import numpy as np
import pytest

from oracle import ballooning_oracle as bo
from tests import modes_basis_oracle as mb
from tests import modes_oracle as mo
from tests.test_gpu_nearest_sigma import host_gcf

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = mo.EPS
CL, BASIS, OPEN = mo.CLUSTER_BIT, mb.BASIS_BIT, mb.OPEN_BIT
KEYS = ("lam", "gam", "X", "dX", "cluster_first", "info")
WORST = {}      # the largest ratio to each bound of the contract seen by this module's tests (printed)


@pytest.fixture(scope="module")
def ctx():
    import ibs_amd
    c = ibs_amd.Context(0)
    yield c
    c.close()


def stack(lines):
    return tuple(np.stack([ln[k] for ln in lines]) for k in (1, 2, 3))


def mixed(N):
    """a double well, the three well families and two s-alpha lines (no clusters) on one grid"""
    return [mo.double_well(N), mo.salpha_line(N, -4.0), mb.triple_well(N), mb.quad_well(N), mo.salpha_line(N, -8.0), mb.asym_triple_well(N)]


def spacing(line):
    return float(line[0][1] - line[0][0])


def check_system(tag, r, i, line, K):
    """system i of a basis result: the partition and the status bits against the reference clusters, then the contract"""
    ref, groups = mb.reference_clusters(*line, K)
    tau = ref["tau"]
    st, first = r["info"][i] >> 16, r["cluster_first"][i]
    assert (st & 3 == 0).all() and np.abs(r["lam"][i] - ref["lam"]).max() <= tau, (tag, st, r["lam"][i], ref["lam"])
    if all(g["width"] <= tau / 8 and g["gap_out"] >= 2 * tau for g in groups):      # unambiguous: the partition is the reference's
        want, is_open = mb.expected_partition(groups, K)
        assert first.tolist() == want.tolist(), (tag, first, want)
    else:
        is_open = bool(st[K - 1] & OPEN)
    sizes = np.array([(first == first[m]).sum() for m in range(K)])
    assert all(first[m] <= m and first[first[m]] == first[m] and (m == 0 or first[m] in (m, first[m - 1])) for m in range(K)), (tag, first)
    last_group = first == first[K - 1]
    in_cluster = (sizes > 1) | (last_group & is_open)
    assert (((st & CL) != 0) == in_cluster).all() and (((st & BASIS) != 0) == in_cluster).all(), (tag, st, first)
    assert (((st & OPEN) != 0) == (last_group & is_open)).all(), (tag, st, first)
    mb.check_contract(*line, K, r["lam"][i], r["gam"][i], r["X"][i], r["dX"][i], first, is_open, WORST)


def assert_named_clusters(line, K, named):
    """the precondition: the clusters `named` ([(first, last)], reference indices) exist among the first K modes, tight and isolated"""
    ref, groups = mb.reference_clusters(*line, K)
    for first, last in named:
        gr = [g for g in groups if g["first"] == first]
        assert gr and gr[0]["last"] == last and gr[0]["width"] <= ref["tau"] / 8 and gr[0]["gap_out"] >= 2 * ref["tau"], (first, last, groups)


SHORT = (67, 131, 195)      # n = N - 2 = 65, 129, 193 interior rows: one row beyond one, two and three blocks of 64 of the recurrences


@pytest.mark.parametrize("N", [67, 131, 195, 513, 771, 2049, 4097])
def test_contract_on_a_mixed_batch(ctx, N):
    """K = 2, 4, 8 on host pointers, K = 4 on device pointers as well (the same bits): (a)-(e) on every system of the mixed batch; K = 1 and
    16 as well at N = 131.  On the short grids the wells are resolved by a few points each and their spectra differ from grid to grid:
    the clusters a line is tested on are the reference's own at that length -- the tight, isolated ones, of which the double well and
    the two triple wells have at least one; the rest (the quad well's second pair at N = 131, its first four modes and the triple
    well's second triplet at N = 195) are ambiguous partitions to check_system"""
    import torch
    lines = mixed(N)
    Ks = (1, 2, 4, 8, 16) if N == 131 else (2, 4, 8)
    if N in SHORT:
        named = [mb.tight_clusters(*line, max(Ks)) for line in lines]
        assert all(named[i] for i in (0, 2, 5)) and not named[1] and not named[4], named
    else:
        named = [[(0, 1)], [], [(0, 2), (3, 5)], [(0, 3)], [], [(1, 2)]]
    for line, nm in zip(lines, named):
        assert_named_clusters(line, max(Ks), nm)
    for line in (lines[1], lines[4]):
        ref, groups = mb.reference_clusters(*line, max(Ks))
        assert all(g["first"] == g["last"] and g["gap_out"] >= 2 * ref["tau"] for g in groups)      # the s-alpha lines have no cluster
    g, c, f = stack(lines)
    h = spacing(lines[0])
    for K in Ks:
        r = ctx.solve_gcf_modes(h, g, c, f, K, want_info=True, basis=True)
        assert r["nbad"] == 0 and r["X"].shape == (len(lines), K, N) and r["cluster_first"].dtype == np.int32
        for i, line in enumerate(lines):
            check_system((N, K, i), r, i, line, K)
        assert not ((r["info"][[1, 4]] >> 16) & (CL | BASIS | OPEN)).any()
        if K == 4:
            dev = torch.device("cuda:0")
            rd = ctx.solve_gcf_modes(h, *(torch.from_numpy(a).to(dev) for a in (g, c, f)), K, want_info=True, basis=True)
            for k in KEYS:
                assert np.array_equal(rd[k].cpu().numpy(), r[k], equal_nan=True), (N, k)
    print("N=%d worst ratios to the bounds so far: %s" % (N, {k: "%.2e" % v for k, v in sorted(WORST.items())}))


@pytest.mark.parametrize("N", [769, 2051])
def test_identity_with_the_modes_entry(ctx, N):
    """(f): lam and the pass count of every mode, status bits 0, 1 and 9, and every output of every unclustered mode are
    Context.solve_gcf_modes' bits on the same batch -- with the half-grid g as the mean of neighbours and as a caller's array"""
    lines = mixed(N)
    g, c, f = stack(lines)
    h = spacing(lines[0])
    gh = np.zeros_like(g)
    gh[:, :-1] = np.sqrt(g[:, :-1] * g[:, 1:])              # (another half-grid rule than the mean: the array is really read)
    for K in (2, 8):
        lams = []
        for half in (None, gh):
            old = ctx.solve_gcf_modes(h, g, c, f, K, gh=half, want_X=True, want_info=True)
            new = ctx.solve_gcf_modes(h, g, c, f, K, gh=half, want_info=True, basis=True)
            assert np.array_equal(old["lam"], new["lam"]) and np.array_equal(old["info"] & 0xffff, new["info"] & 0xffff)
            keep = (0x203 << 16)
            assert np.array_equal(old["info"] & keep, new["info"] & keep) and old["nbad"] == new["nbad"] == 0
            free = ((new["info"] >> 16) & CL) == 0
            assert free.any() and not free.all()
            assert np.array_equal(old["info"][free], new["info"][free])
            for k in ("gam", "X", "dX"):
                assert np.array_equal(old[k][free], new[k][free]), (N, K, k)
            lams.append(new["lam"])
        assert not np.array_equal(lams[0][5], lams[1][5])      # (g of the asymmetric well is not constant)


def test_bitwise_repeatable_and_independent_of_the_batch(ctx):
    """(g): a triple well alone, and at positions 0 and 8 of a batch of 9; a second run of the batch"""
    N, K = 771, 8
    lines = mixed(N)
    assert_named_clusters(lines[2], K, [(0, 2), (3, 5)])
    batch = [lines[2]] + lines + [lines[0], lines[2]]
    assert len(batch) == 9
    g, c, f = stack(batch)
    h = spacing(lines[0])
    alone = ctx.solve_gcf_modes(h, g[:1], c[:1], f[:1], K, want_info=True, basis=True)
    runs = [ctx.solve_gcf_modes(h, g, c, f, K, want_info=True, basis=True) for _ in range(2)]
    for k in KEYS:
        assert np.array_equal(runs[0][k], runs[1][k], equal_nan=True), k
        assert np.array_equal(runs[0][k][0], alone[k][0]) and np.array_equal(runs[0][k][8], alone[k][0]), k
    assert ((alone["info"][0, :6] >> 16) & BASIS).all()


@pytest.mark.parametrize("N", [513, 2561])
def test_open_clusters(ctx, N):
    """the triple well with K = 2 and the double well with K = 1: the cluster continues below the last mode -- bits 9, 13 and 14 on the
    members, (a)-(c), and (d) against the WHOLE reference cluster"""
    for line, K, whole in ((mb.triple_well(N), 2, (0, 2)), (mo.double_well(N), 1, (0, 1))):
        assert_named_clusters(line, K, [whole])
        g, c, f = stack([line, mo.salpha_line(N, -4.0)])
        r = ctx.solve_gcf_modes(spacing(line), g, c, f, K, want_info=True, basis=True)
        assert r["nbad"] == 0
        st = r["info"] >> 16
        assert (st[0] & (CL | BASIS | OPEN) == (CL | BASIS | OPEN)).all() and not st[1].any(), st
        assert (r["cluster_first"][0] == 0).all() and r["cluster_first"][1].tolist() == list(range(K))
        w = {}
        mb.check_contract(*line, K, r["lam"][0], r["gam"][0], r["X"][0], r["dX"][0], r["cluster_first"][0], True, w)
        assert "d" in w and (K == 1 or ("b" in w and "c" in w))
        for k, v in w.items():
            WORST[k] = max(WORST.get(k, 0.0), v)
    print("N=%d worst ratios to the bounds so far: %s" % (N, {k: "%.2e" % v for k, v in sorted(WORST.items())}))


def test_c_entry(ctx):
    """the raw entry point: X = NULL -> IBS_ERR_ARG; even N, N = 65 and N = 65,539 -> IBS_ERR_UNSUPPORTED; an invalid system (g < 0) gets
    status bit 1 and NaN on all its modes and no other system changes by a bit"""
    lib = ctx._lib
    N, K = 513, 4
    lines = [mb.triple_well(N), mo.salpha_line(N, -4.0), mo.double_well(N)]
    g, c, f = stack(lines)
    h = spacing(lines[0])

    def call(g, n_sys, N, with_x=True):
        out = dict(lam=np.zeros((n_sys, K)), gam=np.zeros((n_sys, K)), X=np.zeros((n_sys, K, N)), dX=np.zeros((n_sys, K, N)),
                   cluster_first=np.zeros((n_sys, K), np.int32), info=np.zeros((n_sys, K), np.int32))
        p = lambda a: ctypes.c_void_p(a.ctypes.data)
        rows = np.ascontiguousarray(g)
        cc, ff = (np.ascontiguousarray(np.resize(a, rows.shape)) for a in (c, f))
        rc = lib.ibs_solve_gcf_modes_basis_f64(ctx._h, n_sys, N, h, p(rows), None, p(cc), p(ff), N, K, p(out["lam"]), p(out["gam"]),
                                               p(out["X"]) if with_x else None, p(out["dX"]), p(out["cluster_first"]), p(out["info"]), 1)
        return rc, out

    assert call(g, 3, N, with_x=False)[0] == -1                                     # IBS_ERR_ARG
    for bad_n in (512, 65, 65539):
        assert call(np.ones((1, bad_n)), 1, bad_n)[0] == -3, bad_n                   # IBS_ERR_UNSUPPORTED
    rc, clean = call(g, 3, N)
    assert rc == 0 and ((clean["info"][0] >> 16) & BASIS).any()
    g_bad = g.copy()
    g_bad[1, 200] = -1.0
    rc, r = call(g_bad, 3, N)
    assert rc == K and ((r["info"][1] >> 16) == 2).all()
    assert all(np.isnan(r[k][1]).all() for k in ("lam", "gam", "X", "dX"))
    for i in (0, 2):
        for k in KEYS:
            assert np.array_equal(r[k][i], clean[k][i]), (i, k)
    ref = ctx.solve_gcf_modes(h, g, c, f, K, want_info=True, basis=True)
    for k in KEYS:
        assert np.array_equal(ref[k], clean[k]), k


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def test_more_systems_than_waves(ctx):
    """N = 67, K = 4: the six lines of the mixed batch and an invalid system (g < 0 at one inner point) drawn in a fixed pseudo-random order
    to four times the persistent grid (8 waves per CU), so that every wave serves four systems and the lam, gam, status and cluster rows
    and the open flag it keeps in its workspace pass from a clustered system to an invalid one, from an invalid one to a clustered one
    and from a clustered one to one without a cluster (asserted on the launch's own grid).  Every system: the bits of its kind in the
    batch of seven"""
    from tests.local_eq_cases import assert_wave_reuse, persistent_waves
    N, K, INVALID = 67, 4, 6
    lines = mixed(N)
    assert all(mb.tight_clusters(*lines[i], K) for i in (0, 2, 3, 5)) and not mb.tight_clusters(*lines[1], K)
    g, c, f = (np.concatenate([a, a[2:3]]) for a in stack(lines))
    g[INVALID, 33] = -1.0
    h = spacing(lines[0])
    seven = ctx.solve_gcf_modes(h, g, c, f, K, want_info=True, basis=True)
    st7 = seven["info"] >> 16
    assert seven["nbad"] == K and (st7[INVALID] == 2).all() and not (st7[:INVALID] & 3).any()
    assert all(np.isnan(seven[k][INVALID]).all() for k in ("lam", "gam", "X", "dX"))
    clustered = [i for i in range(INVALID) if (st7[i] & BASIS).any()]
    plain = [i for i in range(INVALID) if not (st7[i] & (CL | BASIS | OPEN)).any()]
    assert set(clustered) >= {0, 2, 3, 5} and set(plain) >= {1}, (clustered, plain)
    n_sys = 4 * persistent_waves()
    kind = np.random.default_rng(67).integers(0, 7, n_sys)
    r = ctx.solve_gcf_modes(h, g[kind], c[kind], f[kind], K, want_info=True, basis=True)
    blocks = assert_wave_reuse(ctx, "k_solve_gcf_modes_basis", n_sys)
    steps = set(zip(kind[:-blocks].tolist(), kind[blocks:].tolist()))      # (system, the next system of the same wave)
    assert any((a, INVALID) in steps for a in clustered) and any((INVALID, b) in steps for b in clustered)
    assert any((a, b) in steps for a in clustered for b in plain)
    assert r["nbad"] == K * (kind == INVALID).sum() and ((r["info"][kind == INVALID] >> 16) == 2).all()
    for k in KEYS:
        assert np.array_equal(bits(r[k]), bits(seven[k][kind])), k


def test_c_entry_padded_rows_and_no_dX(ctx):
    """the raw entry point with ld = N + 7 for g, c, f and a caller's half-grid g, NaN in every padding element, N = 131, K = 4: with dX
    and with dX = NULL (the derivative of a cluster's members then goes through a work row) every output is the packed call's, bit for bit"""
    lib = ctx._lib
    N, K, ld = 131, 4, 131 + 7
    lines = [mb.triple_well(N), mo.salpha_line(N, -4.0), mo.double_well(N)]
    assert mb.tight_clusters(*lines[0], K) and mb.tight_clusters(*lines[2], K)
    g, c, f = stack(lines)
    h = spacing(lines[0])
    gh = np.zeros_like(g)
    gh[:, :-1] = np.sqrt(g[:, :-1] * g[:, 1:])
    packed = ctx.solve_gcf_modes(h, g, c, f, K, gh=gh, want_info=True, basis=True)
    assert packed["nbad"] == 0 and ((packed["info"][[0, 2]] >> 16) & BASIS).any(axis=1).all()

    def pad(a):
        out = np.full((3, ld), np.nan)
        out[:, :N] = a
        return out

    rows = [pad(a) for a in (g, gh, c, f)]
    p = lambda a: ctypes.c_void_p(a.ctypes.data)
    for with_dx in (True, False):
        out = dict(lam=np.zeros((3, K)), gam=np.zeros((3, K)), X=np.zeros((3, K, N)), dX=np.zeros((3, K, N)),
                   cluster_first=np.zeros((3, K), np.int32), info=np.zeros((3, K), np.int32))
        rc = lib.ibs_solve_gcf_modes_basis_f64(ctx._h, 3, N, h, *[p(a) for a in rows], ld, K, p(out["lam"]), p(out["gam"]), p(out["X"]),
                                               p(out["dX"]) if with_dx else None, p(out["cluster_first"]), p(out["info"]), 1)
        assert rc == 0 and "k_solve_gcf_modes_basis<true>" in ctx.last_launch()[0], (with_dx, rc, ctx.last_launch())
        for k in KEYS:
            if k != "dX" or with_dx:
                assert np.array_equal(bits(out[k]), bits(packed[k])), (with_dx, k)
        assert with_dx or not out["dX"].any()               # (not written)


def test_autograd_cluster_mean(ctx):
    """autograd.solve_gcf_modes(cluster="mean") on the asymmetric triple well, K = 3: the members of the cluster (modes 1-2) return
    one lam; the gradient of (lam[1] + lam[2]) / 2 in c and f, contracted with a smooth direction, against central differences
    of the oracle's spectrum at step 1e-4, to 1e-6 relative; cluster="refuse" (the default) behaves as before"""
    import torch
    import ibs_amd
    from ibs_amd import autograd as iag
    from tests import vjp_oracle as vo
    dev = torch.device("cuda:0")
    N, K = 513, 3
    line = mb.asym_triple_well(N)
    th, G_, C_, F_ = line
    assert_named_clusters(line, K, [(1, 2)])
    h = spacing(line)
    rng = np.random.default_rng(513)
    dC, dF = vo.smooth_direction(rng, th, 1.0), vo.smooth_direction(rng, th, 0.05 * F_)
    g, c, f = (torch.from_numpy(a[None]).to(dev).requires_grad_(True) for a in (G_, C_, F_))
    gam, lam = iag.solve_gcf_modes(h, g, c, f, K, ctx=ctx, cluster="mean")
    assert lam[0, 1].item() == lam[0, 2].item() and lam[0, 0].item() > lam[0, 1].item()
    ref = mo.dense_modes(th, G_, C_, F_, K, vectors=False)
    assert abs(lam[0, 1].item() - ref["lam"][1:3].mean()) <= ref["tau"]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        ((lam[0, 1] + lam[0, 2]) / 2).backward()
    an = float((c.grad.cpu().numpy()[0] * dC).sum() + (f.grad.cpu().numpy()[0] * dF).sum())
    mean_at = lambda t: mo.dense_modes(th, G_, C_ + t * dC, F_ + t * dF, K, vectors=False)["lam"][1:3].mean()
    fd = (mean_at(1e-4) - mean_at(-1e-4)) / 2e-4
    print("cluster mean: analytic %.12g, central differences %.12g, relative difference %.3g" % (an, fd, abs(an - fd) / abs(fd)))
    assert abs(an - fd) <= 1e-6 * abs(fd), (an, fd)
    assert np.isfinite(g.grad.cpu().numpy()).all()
    # a cotangent on one member's gam stays refused; so does everything with cluster="refuse"
    for kind, pick in (("mean", lambda gam, lam: gam[0, 1]), ("refuse", lambda gam, lam: lam[0, 1] + lam[0, 2])):
        g, c, f = (torch.from_numpy(a[None]).to(dev).requires_grad_(True) for a in (G_, C_, F_))
        gam, lam = iag.solve_gcf_modes(h, g, c, f, K, ctx=ctx, cluster=kind)
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            pick(gam, lam).backward()
        assert [x for x in w if issubclass(x.category, ibs_amd.VjpStatusWarning)], kind
        assert all(np.isnan(x.grad.cpu().numpy()).all() for x in (g, c, f)), kind
    old = iag.solve_gcf_modes(h, g.detach(), c.detach(), f.detach(), K, ctx=ctx)
    raw = ctx.solve_gcf_modes(h, G_[None], C_[None], F_[None], K)
    assert np.array_equal(old[1].cpu().numpy(), raw["lam"]) and np.array_equal(old[0].cpu().numpy(), raw["gam"], equal_nan=True)
    with pytest.raises(ValueError):
        iag.solve_gcf_modes(h, g, c, f, K, ctx=ctx, cluster="sum")


def test_real_lines(ctx):
    """K = 8 on the alpha = 0 lines of the NCSX golden set at theta0 = 0 (stellarator-symmetric: even / odd pairs wherever two wells
    decouple): whatever clusters appear, (a)-(c) and (f) hold.  Prints what it found."""
    d = np.load(os.path.join(ROOT, "tests", "golden", "G3_ncsx_lines.npz"))
    K = 8
    for N in (513, 1025):
        geo, ln, dP = d["geo_%d" % N], d["lines_%d" % N], d["dPdrho_%d" % N]
        pick = [i for i in range(len(ln)) if ln[i, 1] == 0.0][:9]
        assert pick, (N, ln)
        th = bo.theta_grid(N)
        rows = [host_gcf(geo[i][:7], dP[i], 0.0) for i in pick]
        g, c, f = (np.stack([r[k] for r in rows]) for k in range(3))
        h = th[1] - th[0]
        old = ctx.solve_gcf_modes(h, g, c, f, K, want_X=True, want_info=True)
        new = ctx.solve_gcf_modes(h, g, c, f, K, want_info=True, basis=True)
        assert new["nbad"] == 0 and np.array_equal(old["lam"], new["lam"]) and np.array_equal(old["info"] & (0x203 << 16 | 0xffff), new["info"] & (0x203 << 16 | 0xffff))
        free = ((new["info"] >> 16) & CL) == 0
        for k in ("gam", "X", "dX"):
            assert np.array_equal(old[k][free], new[k][free]), (N, k)
        found = []
        for i in range(len(pick)):
            st, first = new["info"][i] >> 16, new["cluster_first"][i]
            is_open = bool(st[K - 1] & OPEN)
            w = mb.check_contract(th, g[i], c[i], f[i], K, new["lam"][i], new["gam"][i], new["X"][i], new["dX"][i], first, is_open,
                                  subspace=False)
            sizes = [int((first == m0).sum()) for m0 in sorted(set(first.tolist()))]
            if max(sizes) > 1 or is_open:
                found.append((pick[i], first.tolist(), is_open, {k: "%.1e" % v for k, v in w.items()}))
        print("N=%d: %d alpha = 0 lines, clusters among the top %d modes: %s" % (N, len(pick), K, found or "none"))
