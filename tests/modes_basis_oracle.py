"""CPU reference of the cluster bases of the spectrum mode (Context.solve_gcf_modes(basis=True), csrc/ibs_modes_basis.hpp): the
inputs with clustered spectra, the reference clusters of scipy's spectrum (tests/modes_oracle.py) and the contract of a cluster's
returned vectors, bound by bound:
  (a) every pair (lam_m, x_m) meets the residual bound of ibs_solve_gcf_vjp_f64 (modes_oracle.residual_ok);
  (b) |<x^_i, x^_j>_F| <= 64 N eps for two members of a cluster, x^ = x / sqrt(<x, x>_F), F over the interior rows;
  (c) |x^_i^T S x^_j| <= 64 N eps ||A||;
  (d) clusters of reference width <= tau / 8: the F-distance of x^_i from the reference subspace of the WHOLE cluster (members that
      were not asked for included) <= max(1e-8, 64 eps ||A|| / gap_out), gap_out = the distance to the nearest eigenvalue outside;
  (e) gam within 1e-8 of bo.rayleigh_growth of the returned vector; the entry of largest magnitude +1, zero ends."""
import numpy as np

from oracle import ballooning_oracle as bo
from tests import modes_oracle as mo

EPS = mo.EPS
BASIS_BIT, OPEN_BIT = 1 << 13, 1 << 14
_REF = {}
MAX_MODES = 16      # kMaxModes of the library: the reference of a line is computed once, for this many modes


def wells(N, centres):
    """(theta, g, c, f): g = f = 1, c = -30 + 40 sum_x exp(-((theta - x) / 0.8)^2): one eigenfunction per well and level"""
    th = bo.theta_grid(N)
    c = -30.0 + 40.0 * sum(np.exp(-((th - x) / 0.8) ** 2) for x in centres)
    return th, np.ones(N), c, np.ones(N)


def triple_well(N):
    return wells(N, (-8.0, 0.0, 8.0))


def quad_well(N):
    return wells(N, (-9.0, -3.0, 3.0, 9.0))


def asym_triple_well(N):
    """the triple well with g = 1 + 0.1 cos(theta), f = 1 + 0.2 sin(theta)^2: mode 0 isolated, modes 1-2 a cluster, F non-trivial"""
    th, _, c, _ = triple_well(N)
    return th, 1.0 + 0.1 * np.cos(th), c, 1.0 + 0.2 * np.sin(th) ** 2


def reference_clusters(th, g, c, f, K):
    """the clusters of scipy's spectrum that touch modes 0 .. K-1, consecutive eigenvalues less than tau apart being linked:
    (ref = modes_oracle.dense_modes(.., vectors=False), [dict(first, last = the last member in the whole spectrum, width, gap_out)])"""
    key = (np.asarray(g).tobytes(), np.asarray(c).tobytes(), np.asarray(f).tobytes())
    if key not in _REF:                                     # (one dense spectrum per line, shared by the tests that need it)
        _REF[key] = mo.dense_modes(th, g, c, f, MAX_MODES, vectors=False)
    ref = dict(_REF[key])
    ref.update(lam=ref["lam"][:K], gap=ref["gap"][:K])
    w, tau = ref["w"], ref["tau"]
    groups, m = [], 0
    while m < K:
        last = m
        while last + 1 < len(w) and w[last] - w[last + 1] < tau:
            last += 1
        out = min(w[m - 1] - w[m] if m else np.inf, w[last] - w[last + 1] if last + 1 < len(w) else np.inf)
        groups.append(dict(first=m, last=last, width=w[m] - w[last], gap_out=out))
        m = last + 1
    return ref, groups


def expected_partition(groups, K):
    """(cluster_first (K,), open) a kernel must report where every reference cluster is tight and well separated"""
    first = np.arange(K)
    for gr in groups:
        first[gr["first"]:min(gr["last"], K - 1) + 1] = gr["first"]
    return first, groups[-1]["last"] > K - 1


def assert_tight(groups, tau):
    """the precondition of a test on clustered input: every reference cluster is at most tau / 8 wide and at least 2 tau from the rest"""
    for gr in groups:
        assert gr["width"] <= tau / 8 and gr["gap_out"] >= 2 * tau, (gr, tau)


def tight_clusters(th, g, c, f, K):
    """[(first, last)] of the reference clusters of two or more modes that touch modes 0 .. K-1 and are at most tau / 8 wide and at
    least 2 tau from the rest of the spectrum"""
    ref, groups = reference_clusters(th, g, c, f, K)
    return [(gr["first"], gr["last"]) for gr in groups
            if gr["last"] > gr["first"] and gr["width"] <= ref["tau"] / 8 and gr["gap_out"] >= 2 * ref["tau"]]


def subspace_of(th, g, c, f, first, last):
    """F-orthonormal reference basis (n, last - first + 1) of modes first .. last of the whole spectrum"""
    from scipy.linalg import eigh_tridiagonal
    _, (a, b), fd, *_ = mo.spectrum(th, g, c, f)
    n = len(a)
    _, v = eigh_tridiagonal(a, b, select="i", select_range=(n - 1 - last, n - 1 - first))
    return v / np.sqrt(fd)[:, None]


def check_contract(th, g, c, f, K, lam, gam, X, dX, cluster_first, open_last, worst=None, subspace=True):
    """asserts (a)-(e) on one system's output ((d) only with `subspace`); `worst` (a dict) collects the largest ratio to each bound"""
    worst = {} if worst is None else worst
    d, e, fd, h, gu, cu, fu = bo.assemble(th, g, c, f)
    n, N = len(d), len(g)
    ref, groups = reference_clusters(th, g, c, f, K)
    nA, tau = ref["nA"], ref["tau"]

    def note(key, value, bound):
        worst[key] = max(worst.get(key, 0.0), value / bound)
        assert value <= bound, (key, value, bound)

    def S(x):
        y = d * x
        y[1:] += e[1:n] * x[:-1]
        y[:-1] += e[1:n] * x[1:]
        return y

    xh = []
    for m in range(K):
        ok, res, bound = mo.residual_ok(th, g, c, f, lam[m], X[m])
        note("a", res, bound)
        x = X[m][1:-1]
        assert X[m][0] == 0.0 and X[m][-1] == 0.0 and abs(x.max() - 1.0) <= 2 * EPS and x.max() == np.abs(x).max(), m      # (x / m is x * (1 / m): an ulp)
        gm, Xr, dXr = bo.rayleigh_growth(x, h, gu, cu, fu)
        note("e", abs(gam[m] - gm), 1e-8)
        assert np.abs(dX[m] - dXr).max() <= 1e-9 * max(1.0, np.abs(dXr).max()), m
        xh.append(x / np.sqrt((fd * x * x).sum()))
    for m0 in sorted(set(int(v) for v in cluster_first)):
        mem = [m for m in range(K) if cluster_first[m] == m0]
        for i in mem:
            for j in mem:
                if i < j:
                    note("b", abs((fd * xh[i] * xh[j]).sum()), 64 * N * EPS)
                    note("c", abs((xh[i] * S(xh[j])).sum()), 64 * N * EPS * nA)
        if len(mem) < 2 and not (open_last and mem[-1] == K - 1):
            continue
        gr = [q for q in groups if q["first"] <= m0 <= q["last"]][0]
        if subspace and gr["width"] <= tau / 8:
            V = subspace_of(th, g, c, f, gr["first"], gr["last"])
            for i in mem:
                r = xh[i] - V @ (V.T @ (fd * xh[i]))
                note("d", float(np.sqrt((fd * r * r).sum())), max(1e-8, 64 * EPS * nA / gr["gap_out"]))
    return worst
