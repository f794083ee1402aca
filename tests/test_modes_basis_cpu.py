"""CPU: the cluster partition and the basis construction of csrc/ibs_modes_basis.hpp, driven by a stand-alone C++ program (host
compiler only, no GPU) with a SERIAL wave -- one lane, plain sums -- on rows written out by this test.

The eigenvalues handed to the program are scipy's (tests/modes_oracle.py); on the device they are the multisection's, within
2 eps ||A|| of these.  Every group of the partition, single modes included, goes through modes_cluster_basis (on the device a single
unclustered mode keeps its twisted factorisation).  Lines: the double well at N = 67, 129, 513; the triple, quad and asymmetric triple
wells at N = 513.  Checked on the output: the partition against the reference clusters and the contract (a)-(e) of
tests/modes_basis_oracle.py.  Partition cases on written-out eigenvalue lists: two clusters separated by a gap >= tau, one cluster of
16, an open cluster, K = 1 with probe > 1, no cluster.  The same program runs once more built with -fsanitize=address,undefined, the
sanitizers' runtimes linked statically."""
import os
import subprocess

import numpy as np
import pytest

from tests import modes_basis_oracle as mb
from tests import modes_oracle as mo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ideal-ballooning-solver_amd", "csrc")
EPS = mo.EPS

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "ibs_modes_basis.hpp"

struct HostWave {
  int n_pts; double step;
  std::vector<double> gg, cg, fg, X, dX, W, sm;
  int lane() const { return 0; }
  int lanes() const { return 1; }
  double sum(double v) const { return v; }
  double max(double v) const { return v; }
  double bcast(double v, int) const { return v; }
  void sync() const {}
  int N() const { return n_pts; }
  double h() const { return step; }
  double g(int j) const { return gg.at(j); }
  double c(int j) const { return cg.at(j); }
  double f(int j) const { return fg.at(j); }
  double e(int k) const { return 0.5 * (gg.at(k) + gg.at(k + 1)) * (1.0 / (step * step)); }
  double& x(int i, int j) { return X.at((size_t)i * n_pts + j); }
  double& dx(int i, int j) { return dX.at((size_t)i * n_pts + j); }
  double& ws(int k, int r) { return W.at((size_t)k * n_pts + r); }
  double* small() { return sm.data(); }
};

static bool read(std::FILE* fh, std::vector<double>& v) {
  for (double& x : v) if (std::fscanf(fh, "%la", &x) != 1) return false;
  return true;
}

// "P K tau probe lam_0 .. lam_{K-1}"                      -> "open first_0 .. first_{K-1}"
// "S K N h normA tau probe  g[N] c[N] f[N] lam[K]"        -> the same line, then per mode "found gam X[N] dX[N]"
int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::FILE* fh = std::fopen(argv[1], "r");
  if (!fh) return 2;
  char kind;
  while (std::fscanf(fh, " %c", &kind) == 1) {
    int K, N = 0, probe, first[ibs::kMaxModes];
    double h = 0.0, normA = 0.0, tau;
    if (kind == 'P') { if (std::fscanf(fh, "%d %la %d", &K, &tau, &probe) != 3) return 2; }
    else if (std::fscanf(fh, "%d %d %la %la %la %d", &K, &N, &h, &normA, &tau, &probe) != 6) return 2;
    if (K < 1 || K > ibs::kMaxModes) return 2;
    HostWave w;
    if (kind == 'S') {
      w.n_pts = N; w.step = h;
      w.gg.resize(N); w.cg.resize(N); w.fg.resize(N);
      if (!read(fh, w.gg) || !read(fh, w.cg) || !read(fh, w.fg)) return 2;
    }
    std::vector<double> lam(K);
    if (!read(fh, lam)) return 2;
    const bool open = ibs::modes_partition(lam.data(), K, tau, probe, first);
    std::printf("%d", open ? 1 : 0);
    for (int m = 0; m < K; ++m) std::printf(" %d", first[m]);
    std::printf("\n");
    if (kind != 'S') continue;
    for (int m0 = 0; m0 < K;) {
      int m = 1;
      while (m0 + m < K && first[m0 + m] == m0) ++m;
      w.X.assign((size_t)m * N, 0.0); w.dX.assign((size_t)m * N, 0.0); w.W.assign((size_t)5 * N, 0.0);
      w.sm.assign(ibs::kBasisSmallDoubles, 0.0);
      double gam[ibs::kMaxModes];
      const unsigned found = ibs::modes_cluster_basis(w, m, lam.data() + m0, normA, tau, gam);
      for (int i = 0; i < m; ++i) {
        const bool ok = (found >> i) & 1u;
        std::printf("%d %a", ok ? 1 : 0, ok ? gam[i] : 0.0);
        for (int j = 0; j < N; ++j) std::printf(" %a", ok ? w.x(i, j) : 0.0);
        for (int j = 0; j < N; ++j) std::printf(" %a", ok ? w.dx(i, j) : 0.0);
        std::printf("\n");
      }
      m0 += m;
    }
  }
  std::fclose(fh);
  return 0;
}
"""


def hexs(values):
    return " ".join(float(v).hex() for v in np.ravel(values))


def lines():
    """[(name, K, (theta, g, c, f))]"""
    out = [("double well N=%d" % N, 2, mo.double_well(N)) for N in (67, 129, 513)]
    out += [("double well N=513, K=1 (open)", 1, mo.double_well(513)),
            ("triple well N=513", 6, mb.triple_well(513)), ("triple well N=513, K=2 (open)", 2, mb.triple_well(513)),
            ("quad well N=513", 4, mb.quad_well(513)), ("asymmetric triple well N=513", 3, mb.asym_triple_well(513))]
    return out


def partition_cases():
    """[(name, K, tau, probe, lam, open, cluster_first)]"""
    tau = 1e-10
    two = [3.0, 3.0 - tau / 4, 2.0, 2.0 - tau / 2, 1.0]
    sixteen = [1.0 - k * tau / 3 for k in range(16)]
    return [("two clusters a gap >= tau apart", 5, tau, 5, two, 0, [0, 0, 2, 2, 4]),
            ("adjacent clusters exactly tau apart", 4, 0.25, 4, [2.0, 1.875, 1.625, 1.5], 0, [0, 0, 2, 2]),
            ("one cluster of 16", 16, tau, 16, sixteen, 0, [0] * 16),
            ("an open cluster", 3, tau, 5, [2.0, 1.0, 1.0 - tau / 8], 1, [0, 1, 1]),
            ("K = 1 with probe > 1", 1, tau, 2, [1.0], 1, [0]),
            ("K = 1, probe not taken", 1, tau, -1, [1.0], 0, [0]),
            ("no cluster", 4, tau, 4, [4.0, 3.0, 2.0, 1.0], 0, [0, 1, 2, 3])]


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    d = tmp_path_factory.mktemp("modes_basis")
    src = d / "basis_check.cpp"
    src.write_text(PROGRAM)
    exes = {}
    for tag, flags in (("plain", ["-O1"]), ("san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"])):
        exes[tag] = str(d / ("basis_check_" + tag))
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I", CSRC, str(src), "-o", exes[tag]])
    text = []
    for _, K, tau, probe, lam, _, _ in partition_cases():
        text.append("P %d %s %d %s\n" % (K, float(tau).hex(), probe, hexs(lam)))
    cases = []
    for name, K, (th, g, c, f) in lines():
        ref, groups = mb.reference_clusters(th, g, c, f, K)
        N, h = len(g), float(th[1] - th[0])
        probe = int((ref["w"] > ref["lam"][K - 1] - ref["tau"]).sum())
        text.append("S %d %d %s %s %s %d %s %s %s %s\n" % (K, N, h.hex(), float(ref["nA"]).hex(), float(ref["tau"]).hex(), probe,
                                                         hexs(g), hexs(c), hexs(f), hexs(ref["lam"])))
        cases.append((name, K, (th, g, c, f), ref, groups))
    inp = d / "cases.txt"
    inp.write_text("".join(text))
    return exes, str(inp), cases


def run(exe, inp):
    p = subprocess.run([exe, inp], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    return [ln.split() for ln in p.stdout.splitlines()]


def test_partition_of_written_out_eigenvalues(built):
    exes, inp, _ = built
    rows = run(exes["plain"], inp)
    for (name, K, tau, probe, lam, is_open, first), row in zip(partition_cases(), rows):
        assert [int(v) for v in row] == [is_open] + first, (name, row)


def test_cluster_bases_meet_the_contract(built):
    exes, inp, cases = built
    rows = run(exes["plain"], inp)[len(partition_cases()):]
    worst, at = {}, 0
    for name, K, (th, g, c, f), ref, groups in cases:
        N = len(g)
        mb.assert_tight(groups, ref["tau"])                     # the precondition: tight, well separated reference clusters
        first, is_open = mb.expected_partition(groups, K)
        assert [int(v) for v in rows[at]] == [int(is_open)] + list(first), (name, rows[at])
        assert len(set(first)) < K or is_open, name             # (every line has a cluster among its K modes)
        out = [[float.fromhex(v) for v in r[1:]] for r in rows[at + 1:at + 1 + K]]
        assert all(int(r[0]) == 1 for r in rows[at + 1:at + 1 + K]), (name, "a member was refused")
        at += 1 + K
        gam = np.array([r[0] for r in out])
        X, dX = np.array([r[1:1 + N] for r in out]), np.array([r[1 + N:] for r in out])
        w = mb.check_contract(th, g, c, f, K, ref["lam"], gam, X, dX, first, is_open)
        print("%-34s worst ratio to the bounds: %s" % (name, {k: "%.2e" % v for k, v in sorted(w.items())}))
        for k, v in w.items():
            worst[k] = max(worst.get(k, 0.0), v)
    assert at == len(rows)
    print("all lines:", {k: "%.2e" % v for k, v in sorted(worst.items())})


def test_the_same_program_under_address_and_ub_sanitizers(built):
    exes, inp, _ = built
    assert run(exes["san"], inp) == run(exes["plain"], inp)
