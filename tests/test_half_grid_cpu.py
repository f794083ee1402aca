"""CPU: the half-grid row e_{j+1} = 0.5 (g_j + g_{j+1}) / h^2 of csrc/ibs_half_grid.hpp against a transcription of the expression
WaveSolver::setup compiled to before the rounding was written down, bit for bit.

Where g = a1 * d is a product, the sum of the mean adds two products and one of them went into an fma.  Which one is recorded below
per rows-per-lane value M as it was read off the gfx950 listing of k_gamma_scan<double, M> (tools/half_grid_pattern.py; the lean
scan, the chained scan, k_obj_w_grad, k_refine_eval and the sub-wave scans held the same rows): entry k of LISTING[M] is
"F<p>/R<q>" -- mean k, between chunk points k and k + 1, is 0.5 * fma(a1_p, d_p, round(a1_q * d_q)).  The stand-alone C++ program
(host compiler only, no GPU, no sanitizer) walks chunks over real rows and compares, for every mean of every chunk,
    ibs::half_grid_e(k, M, ...)    with    (0.5 * fma(a1_F, d_F, a1_R * d_R)) * ih2    placed by the table,
and ibs::half_grid_mean_plain with 0.5 * (g_lo + g_hi) on the rounded products (the stored-g sources).

Rows (a1, d on a 513-point grid, h its spacing): two s-alpha rows, a1 = 1 / (1 + 0.18 cos theta), d = 1 + (shat (theta - theta0)
- alpha sin theta)^2; four golden NCSX lines (tests/golden/G3_ncsx_lines.npz) at theta0 = 0 and 0.8, a1 = |gradpar| / bmag,
d = gds2 + 2 theta0 gds21 + theta0^2 gds22; and every one of them with a1 scaled by 2^40 and by 2^-40.  Chunks: M = 3 .. 8, every
start a in [0, 40) (both parities), with and without a last row (M + 1 or M means).  Bit equality is required; the program also
counts how many means the OTHER placement would have changed, which must be a good share of them (else the comparison sees nothing).
"""
import os
import subprocess

import numpy as np

from oracle import ballooning_oracle as bo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ideal-ballooning-solver_amd", "csrc")
G = os.path.join(ROOT, "tests", "golden")
N = 513

LISTING = {
    3: "F0/R1 F2/R1 F2/R3 F4/R3",
    4: "F0/R1 F1/R2 F3/R2 F3/R4 F5/R4",
    5: "F0/R1 F2/R1 F2/R3 F4/R3 F4/R5 F6/R5",
    6: "F0/R1 F1/R2 F3/R2 F3/R4 F5/R4 F5/R6 F7/R6",
    7: "F0/R1 F2/R1 F2/R3 F4/R3 F4/R5 F6/R5 F6/R7 F8/R7",
    8: "F0/R1 F1/R2 F3/R2 F3/R4 F5/R4 F5/R6 F7/R6 F7/R8 F9/R8",
}

PROGRAM = r"""
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include "ibs_half_grid.hpp"

static const int kN = %(N)d;
// LISTING: per M = 3 .. 8 and mean k = 0 .. M the chunk points (fused, rounded)
static const int kTab[6][9][2] = %(TABLE)s;

static bool same(double x, double y) { return std::memcmp(&x, &y, sizeof x) == 0; }

int main(int argc, char** argv) {
  std::FILE* fp = std::fopen(argv[1], "rb");
  if (!fp) return 2;
  double head[2];
  if (std::fread(head, sizeof(double), 2, fp) != 2) return 2;
  const int rows = (int)head[0];
  const double h = head[1], ih2 = 1.0 / (h * h);
  std::vector<double> a1((size_t)rows * kN), d((size_t)rows * kN);
  if (std::fread(a1.data(), sizeof(double), a1.size(), fp) != a1.size()) return 2;
  if (std::fread(d.data(), sizeof(double), d.size(), fp) != d.size()) return 2;
  std::fclose(fp);
  long cases = 0, bad = 0, other = 0, pcases = 0, pbad = 0;
  for (int r = 0; r < rows; ++r) {
    const double* A = &a1[(size_t)r * kN];
    const double* Dd = &d[(size_t)r * kN];
    for (int M = 3; M <= 8; ++M)
      for (int a = 0; a < 40; ++a)
        for (int has_last = 0; has_last < 2; ++has_last) {
          const int means = has_last ? M + 1 : M;
          for (int k = 0; k < means; ++k) {
            const int lo = a + k, hi = lo + 1;
            const int F = a + kTab[M - 3][k][0], R = a + kTab[M - 3][k][1];
            const double gR = A[R] * Dd[R];
            const double want = (0.5 * std::fma(A[F], Dd[F], gR)) * ih2;
            const double got = ibs::half_grid_e(k, M, A[lo], Dd[lo], A[hi], Dd[hi], ih2);
            const double gF = A[F] * Dd[F];
            const double swapped = (0.5 * std::fma(A[R], Dd[R], gF)) * ih2;
            ++cases;
            if (!same(swapped, want)) ++other;
            if (!same(got, want)) {
              if (bad < 10) std::printf("MISMATCH row %%d M %%d a %%d k %%d: %%a, listing %%a\n", r, M, a, k, got, want);
              ++bad;
            }
            const double p_want = 0.5 * (gF + gR), p_got = ibs::half_grid_mean_plain(A[lo] * Dd[lo], A[hi] * Dd[hi]);
            ++pcases;
            if (!same(p_got, p_want)) ++pbad;
          }
        }
  }
  std::printf("fused cases %%ld bad %%ld other-placement-differs %%ld\n", cases, bad, other);
  std::printf("plain cases %%ld bad %%ld\n", pcases, pbad);
  return (bad || pbad) ? 1 : 0;
}
"""


def table():
    out = []
    for M in range(3, 9):
        ent = [(int(e.split("/")[0][1:]), int(e.split("/")[1][1:])) for e in LISTING[M].split()]
        assert len(ent) == M + 1 and all(sorted(p) == [k, k + 1] for k, p in enumerate(ent)), (M, ent)
        ent += [(0, 0)] * (9 - len(ent))
        out.append("{" + ", ".join("{%d, %d}" % p for p in ent) + "}")
    return "{" + ",\n  ".join(out) + "}"


def rows():
    th = bo.theta_grid(N)
    a1, d = [], []
    for shat, alpha, t0 in ((1.0, 0.8, 0.0), (0.5, 1.4, 0.3)):
        a1.append(1.0 / (1.0 + 0.18 * np.cos(th)))
        d.append(1.0 + (shat * (th - t0) - alpha * np.sin(th)) ** 2)
    geo = np.load(os.path.join(G, "G3_ncsx_lines.npz"))["geo_513"][:4]          # bmag, gradpar, cvdrift, cvdrift0, gds2, gds21, gds22, gbdrift
    for ln in geo:
        for t0 in (0.0, 0.8):
            a1.append(np.abs(ln[1]) / ln[0])
            d.append(ln[4] + 2.0 * t0 * ln[5] + t0 * t0 * ln[6])
    a1, d = np.array(a1), np.array(d)
    assert (a1 > 0).all() and (d > 0).all()
    a1 = np.concatenate([a1, a1 * 2.0 ** 40, a1 * 2.0 ** -40])
    d = np.concatenate([d, d, d])
    return float(th[1] - th[0]), a1, d


def test_helper_equals_the_listing_of_set_up(tmp_path):
    h, a1, d = rows()
    data = tmp_path / "rows.bin"
    with open(data, "wb") as fp:
        np.array([len(a1), h]).tofile(fp)
        np.ascontiguousarray(a1).tofile(fp)
        np.ascontiguousarray(d).tofile(fp)
    src, exe = tmp_path / "half_grid_check.cpp", tmp_path / "half_grid_check"
    src.write_text(PROGRAM % dict(N=N, TABLE=table()))
    # (contraction off for the transcription too: its one fma is std::fma; the header's pragma is clang's, so not -Werror here)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas", "-I", CSRC, str(src), "-o", str(exe)])
    p = subprocess.run([str(exe), str(data)], capture_output=True, text=True)
    print(p.stdout)
    assert p.returncode == 0, p.stdout + p.stderr
    lines = dict((ln.split(" cases ")[0], ln.split()) for ln in p.stdout.splitlines() if " cases " in ln)
    n_cases = len(a1) * 40 * sum(M + (M + 1) for M in range(3, 9))
    assert int(lines["fused"][2]) == n_cases and int(lines["fused"][4]) == 0
    assert int(lines["plain"][2]) == n_cases and int(lines["plain"][4]) == 0
    assert int(lines["fused"][6]) > n_cases // 10, lines["fused"]          # the placement is visible in these rows


def test_the_rule_is_the_listing():
    """half_grid_fuses_lower(k, M), transcribed: k = 0 fuses the lower point; above, the rounded point has the parity of M"""
    for M in range(3, 9):
        for k, e in enumerate(LISTING[M].split()):
            fused = int(e.split("/")[0][1:])
            lower = k == 0 or ((k ^ M) & 1) != 0
            assert fused == (k if lower else k + 1), (M, k, e)
