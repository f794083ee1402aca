"""CPU: the integer part of the resident solver's forward sweep (csrc/ibs_sweep_count.hpp: the per-lane ownership mask, the count
from one word of sign bits, the two-ballot rule) against the row-by-row rule of WaveSolver::sweep_fwd, exhaustively.

A stand-alone C++ program (host compiler only, no GPU, no sanitizer) includes the header and
  * for M = 3 .. 8, has_last in {0, 1}, lane class in {lane 0, interior, lane 63} and EVERY sign pattern of the M + 2 values
    (u_-1, u_0, z_1 .. z_M) builds the word as sweep_fwd_min2 does -- seed with the sign of u_-1, then one shift per value -- and
    compares sweep_count_lane(word, sweep_count_mask(...), M) with the count of the loop transcribed from sweep_fwd:
        ncount = (has_last ? M : M - 1) - (lane == 63 ? 0 : 1)
        count  = differs(u_0, u_-1) + sum_i [(i < M - 2 || i < ncount) && differs(z_{i+1}, z_i)]
    (lane 0 receives the fill (1, 0): its class differs from `interior` in nothing the integer rule sees, and is run all the same,
    with every pattern, as the issue's case list has it);
  * set bits above bit M + 1 of the word must not matter (the device seeds the word with one bit, so it has none; the mask is
    what makes the count independent of them, and that is checked);
  * for 20000 random vectors of 64 per-lane counts (most lanes 0, so that totals of 0, 1 and 2 are all frequent) compares
    sweep_count_min2(ballot(c != 0), ballot(c > 1)) with min(sum, 2)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ideal-ballooning-solver_amd", "csrc")

PROGRAM = r"""
#include <cstdio>
#include <cstdint>
#include "ibs_sweep_count.hpp"

static int rule(int M, bool has_last, bool last_lane, const bool* neg) {      // neg[0] = u_-1, neg[1] = u_0, neg[2 + i] = z_{i+1}
  const int ncount = (has_last ? M : M - 1) - (last_lane ? 0 : 1);
  int count = neg[1] != neg[0] ? 1 : 0;
  for (int i = 0; i < M; ++i) {
    const bool flip = (i < M - 2 || i < ncount) && (neg[2 + i] != neg[1 + i]);
    count += flip ? 1 : 0;
  }
  return count;
}

int main() {
  long cases = 0, bad = 0;
  for (int M = 3; M <= 8; ++M)
    for (int has_last = 0; has_last < 2; ++has_last)
      for (int cls = 0; cls < 3; ++cls) {                   // lane 0, interior, lane 63
        const bool last_lane = cls == 2;
        const unsigned mask = ibs::sweep_count_mask(M, has_last != 0, last_lane);
        for (unsigned pat = 0; pat < (1u << (M + 2)); ++pat) {
          bool neg[10];
          for (int k = 0; k < M + 2; ++k) neg[k] = (pat >> k) & 1u;
          for (unsigned junk = 0; junk < 2; ++junk) {
            unsigned w = junk ? 0xffffffffu : 0u;           // what the word held before: shifted up and out of the mask's reach
            for (int k = 0; k < M + 2; ++k) w = (w << 1) | (neg[k] ? 1u : 0u);
            const int got = ibs::sweep_count_lane(w, mask, M), want = rule(M, has_last != 0, last_lane, neg);
            ++cases;
            if (got != want) {
              if (bad < 10) std::printf("MISMATCH M=%d has_last=%d class=%d pattern=%#x junk=%u: %d, rule %d\n", M, has_last, cls, pat, junk, got, want);
              ++bad;
            }
          }
        }
      }
  std::printf("count cases %ld bad %ld\n", cases, bad);
  uint64_t s = 0x9e3779b97f4a7c15ull;
  auto rnd = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; };
  long bcases = 0, bbad = 0, seen[3] = {0, 0, 0};
  for (int t = 0; t < 20000; ++t) {
    int c[64], sum = 0;
    const int busy = (int)(rnd() % 4);                      // how many lanes may be non-zero
    for (int l = 0; l < 64; ++l) c[l] = 0;
    for (int k = 0; k < busy; ++k) c[rnd() % 64] = (int)(rnd() % 4);          // 0 .. 3 changes in a lane
    if (t % 97 == 0) for (int l = 0; l < 64; ++l) c[l] = (int)(rnd() % 10);   // and dense vectors
    unsigned long long b1 = 0, b2 = 0;
    for (int l = 0; l < 64; ++l) { sum += c[l]; if (c[l] != 0) b1 |= 1ull << l; if (c[l] > 1) b2 |= 1ull << l; }
    const int want = sum < 2 ? sum : 2, got = ibs::sweep_count_min2(b1, b2);
    ++bcases; ++seen[want];
    if (got != want) { if (bbad < 10) std::printf("BALLOT MISMATCH sum=%d got %d\n", sum, got); ++bbad; }
  }
  std::printf("ballot cases %ld bad %ld seen %ld %ld %ld\n", bcases, bbad, seen[0], seen[1], seen[2]);
  return (bad || bbad) ? 1 : 0;
}
"""


def test_sign_word_count_equals_the_row_rule(tmp_path):
    src, exe = tmp_path / "sweep_count_check.cpp", tmp_path / "sweep_count_check"
    src.write_text(PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)])
    p = subprocess.run([str(exe)], capture_output=True, text=True)
    print(p.stdout)
    assert p.returncode == 0, p.stdout + p.stderr
    lines = dict((ln.split(" cases ")[0], ln.split()) for ln in p.stdout.splitlines() if " cases " in ln)
    # every pattern of every (M, has_last, lane class), with clean and with set upper bits: 2 * 2 * 3 * sum_M 2^(M + 2)
    assert int(lines["count"][2]) == 2 * 2 * 3 * sum(1 << (M + 2) for M in range(3, 9)) and int(lines["count"][4]) == 0
    assert int(lines["ballot"][2]) == 20000 and int(lines["ballot"][4]) == 0
    assert all(int(x) > 1000 for x in lines["ballot"][6:9]), lines["ballot"]          # totals 0, 1 and >= 2 all exercised
