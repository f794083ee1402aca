"""CPU: the bookkeeping of the simultaneous multisection (csrc/ibs_modes.hpp: which lane takes which shift, how the brackets tighten,
when a pass is the last, which modes form a cluster) against spectra written out by this test.

A stand-alone C++ program (host compiler only, no GPU) includes the header, drives it exactly as k_solve_gcf_modes does -- with an
EXACT count function over the eigenvalue list of the case in place of the device's count_above_chunked -- and prints passes, lam and
status of every mode.  Cases: the named lines (s-alpha, shat = 1, alpha = 0.8, dPdrho -1 and -8, N = 67, 513, 2,561; the double well
at N = 131 and 513) with their spectra from scipy, K = 1, 2, 4, 8, 16, bracketed as the kernel's bounds bracket them; and adversarial
lists (K equal values, two values tau / 8 apart, fewer distinct values than K, a spectrum of width 0).  Asserted:
  * every mode is closed within 2 eps ||A|| of the list's m-th largest value;
  * the cluster bit is set where the gap to the nearer neighbour (the first unwanted value included) is below tau / 2 and clear where it
    is above 2 tau, tau = 4 N eps ||A||;
  * passes <= 20 for K <= 8 on the named lines, and below the cap of 32 everywhere.
The same program runs once more built with -fsanitize=address,undefined, as a stand-alone binary with the sanitizers' runtimes linked
statically: it needs nothing from the environment it is started in."""
import os
import subprocess

import numpy as np
import pytest

from tests import modes_oracle as mo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ideal-ballooning-solver_amd", "csrc")
EPS = mo.EPS

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "ibs_modes.hpp"

struct HostWave {
  double sig[64]; int cnt[64];
  unsigned long long inside_ge(double lo, double hi, int k) const {
    unsigned long long m = 0;
    for (int l = 0; l < 64; ++l) if (sig[l] > lo && sig[l] < hi && cnt[l] >= k) m |= 1ull << l;
    return m;
  }
  unsigned long long inside_lt(double lo, double hi, int k) const {
    unsigned long long m = 0;
    for (int l = 0; l < 64; ++l) if (sig[l] > lo && sig[l] < hi && cnt[l] < k) m |= 1ull << l;
    return m;
  }
  double shift(int lane) const { return sig[lane]; }
};

// one case per line: K N normA lo hi n v_1 .. v_n (hex floats) -> "passes ascending lam_0 status_0 ... "
int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::FILE* fh = std::fopen(argv[1], "r");
  if (!fh) return 2;
  int K, N, n;
  double normA, lo, hi;
  while (std::fscanf(fh, "%d %d %la %la %la %d", &K, &N, &normA, &lo, &hi, &n) == 6) {
    std::vector<double> v(n);
    for (int i = 0; i < n; ++i) if (std::fscanf(fh, "%la", &v[i]) != 1) return 2;
    auto count = [&](double s) { int c = 0; for (double x : v) c += x > s ? 1 : 0; return c; };
    const double eps = 2.220446049250313e-16, stop = 2.0 * eps * normA, tau = 4.0 * N * eps * normA;
    ibs::ModesBrackets br;
    ibs::modes_init(br, K, lo, hi);
    HostWave w;
    int passes = 0, ascending = 1;
    while (passes < ibs::kModesPassCap) {
      bool any = false;
      for (int l = 0; l < 64; ++l) any = ibs::modes_lane_shift(br, stop, l, w.sig[l]);
      if (!any) break;
      for (int l = 0; l < 64; ++l) { w.cnt[l] = count(w.sig[l]); if (l && w.sig[l] < w.sig[l - 1]) ascending = 0; }
      ++passes;
      ibs::modes_tighten(br, stop, w);
      for (int m = 0; m < K; ++m)
        if (!(count(br.lo[m]) >= m + 1 && count(br.hi[m]) < m + 1 && br.lo[m] < br.hi[m])) { std::printf("INVARIANT broken at mode %d\n", m); return 1; }
    }
    int probe = -1;
    if (ibs::modes_all_closed(br, stop)) { probe = count(ibs::modes_probe_shift(br, tau)); ++passes; }
    double lam[ibs::kMaxModes];
    int status[ibs::kMaxModes];
    ibs::modes_finish(br, stop, tau, probe, lam, status);
    std::printf("%d %d", passes, ascending);
    for (int m = 0; m < K; ++m) std::printf(" %a %d", lam[m], status[m]);
    std::printf("\n");
  }
  std::fclose(fh);
  return 0;
}
"""


def hexs(values):
    return " ".join(float(v).hex() for v in values)


def named_lines():
    out = []
    for N in (67, 513, 2561):
        for dP in (-1.0, -8.0):
            out.append(("salpha N=%d dP=%g" % (N, dP), N) + mo.salpha_line(N, dP))
    for N in (131, 513):
        out.append(("double well N=%d" % N, N) + mo.double_well(N))
    return out


def make_cases():
    """[(name, named, K, N, normA, lo, hi, values descending)]"""
    cases = []
    for name, N, th, g, c, f in named_lines():
        w = mo.spectrum(th, g, c, f)[0][::-1]
        lo, hi, nA = mo.gersh_bounds(th, g, c, f)
        assert lo < w[-1] and w[0] < hi
        for K in (1, 2, 4, 8, 16):
            cases.append((name, True, K, N, nA, lo, hi, w))
    N, nA = 67, 100.0
    tau = 4 * N * EPS * nA
    bulk = np.linspace(-90.0, -1.0, 60)
    lo, hi = -100.0 - 8 * EPS * nA, 3.0 + 8 * EPS * nA
    for K in (1, 3, 8, 16):
        cases.append(("%d equal values" % K, False, K, N, nA, lo, hi, np.concatenate([np.full(K, 1.25), bulk])))
        cases.append(("equal values across the cut", False, K, N, nA, lo, hi, np.concatenate([np.full(K + 2, 1.25), bulk])))
        cases.append(("two values tau / 8 apart", False, K, N, nA, lo, hi, np.concatenate([[2.0, 1.5 + tau / 8, 1.5], bulk])))
        cases.append(("fewer distinct values than K", False, K, N, nA, lo, hi, np.concatenate([np.full(9, 2.0), np.full(9, 0.5), bulk])))
        cases.append(("two values 3 tau apart", False, K, N, nA, lo, hi, np.concatenate([[2.0, 1.5 + 3 * tau, 1.5], bulk])))
        cases.append(("width 0", False, K, N, 1.0, 1.0 - 8 * EPS, 1.0 + 8 * EPS, np.full(65, 1.0)))
        cases.append(("width 0 at 0", False, K, N, 1.0, -8 * EPS, 8 * EPS, np.zeros(65)))
    return [c[:7] + (np.sort(c[7])[::-1],) for c in cases]


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    d = tmp_path_factory.mktemp("modes_bookkeeping")
    src = d / "modes_check.cpp"
    src.write_text(PROGRAM)
    exes = {}
    for tag, flags in (("plain", ["-O1"]), ("san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"])):
        exes[tag] = str(d / ("modes_check_" + tag))
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I", CSRC, str(src), "-o", exes[tag]])
    cases = make_cases()
    inp = d / "cases.txt"
    inp.write_text("".join("%d %d %s %s %s %d %s\n" % (K, N, float(nA).hex(), float(lo).hex(), float(hi).hex(), len(w), hexs(w))
                           for _, _, K, N, nA, lo, hi, w in cases))
    return exes, str(inp), cases


def run(exe, inp):
    p = subprocess.run([exe, inp], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    return [ln.split() for ln in p.stdout.splitlines()]


def test_brackets_close_on_the_spectrum(built):
    exes, inp, cases = built
    rows = run(exes["plain"], inp)
    assert len(rows) == len(cases)
    worst = {}
    for (name, named, K, N, nA, lo, hi, w), row in zip(cases, rows):
        passes, ascending = int(row[0]), int(row[1])
        lam = np.array([float.fromhex(x) for x in row[2::2]])
        status = np.array([int(x) for x in row[3::2]])
        assert len(lam) == K and ascending == 1, (name, K)
        assert not (status & 1).any(), (name, K, status)
        assert np.abs(lam - w[:K]).max() <= 2 * EPS * nA, (name, K, lam, w[:K])
        tau = 4 * N * EPS * nA
        gap = np.array([min(w[m - 1] - w[m] if m else np.inf, w[m] - w[m + 1]) for m in range(K)])
        bit = (status & mo.CLUSTER_BIT) != 0
        assert bit[gap < 0.5 * tau].all() and not bit[gap > 2 * tau].any(), (name, K, gap / tau, bit)
        assert passes < 32, (name, K, passes)
        if named and K <= 8:
            assert passes <= 20, (name, K, passes)
        if named:
            worst[K] = max(worst.get(K, 0), passes)
    print("passes on the named lines, worst per K (the cluster probe included):", worst)


def test_the_same_program_under_address_and_ub_sanitizers(built):
    exes, inp, cases = built
    assert run(exes["san"], inp) == run(exes["plain"], inp)
