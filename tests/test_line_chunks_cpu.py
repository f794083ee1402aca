"""CPU: the chunk rule of the whole-line chunked scans (csrc/ibs_plan.hpp: plan_line_chunks, Carve, pad256), walked on the host.

A stand-alone C++ program (host compiler only, no HIP, no GPU) includes the header and prints `lines bytes` for every case of a
sweep with the synthetic workspace bytes_of(L) = fixed + per_line * L under the budget kLineChunkBudget (1 GiB; its budget branch,
the halving, takes more than that much device memory to reach through the library).  The Python side restates the rule on its own
and compares every line, then pins a few cases by hand at a budget of 1000 bytes, and one case through Carve itself: the workspace
of scan_rows_chunked (per-wave workspace, then three rows per system), whose counting pass and carving pass must give the same
offsets as pad256 arithmetic written out here."""
import itertools
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ideal-ballooning-solver_amd", "csrc")

BUDGET = 1 << 30
N_LINES = (1, 2, 3, 7, 10, 64, 1000, 16384)
N_THETA0 = (1, 3, 15)
OPTION = (0, 1, 2, 7, 45, 10 ** 9)
PER_LINE = (32212255, 322122547, 2 * BUDGET + 1234)        # about 0.03, 0.3 and 2 times the budget
FIXED = (0, 4096)
# by hand, at a budget of 1000 bytes and fixed = 0: (n_lines, n_theta0, option, per_line) -> (lines, bytes)
HAND = [((10, 1, 0, 300), (3, 900)),            # 10 -> 5 -> 3
        ((7, 1, 0, 300), (2, 600)),             # 7 -> 4 -> 2, although 3 lines would fit
        ((10, 1, 0, 2000), (1, 2000)),          # one line over the budget stays one line
        ((10, 1, 0, 50), (10, 500)),
        ((10, 3, 7, 50), (2, 100)),             # the option counts systems: whole lines, rounded down
        ((10, 3, 2, 50), (1, 50)),              # ... and at least one
        ((10, 1, 10 ** 9, 50), (10, 500))]
# the Carve case: 10 lines x 3 theta0 at N = 7, 5 doubles of workspace per wave, at most 4 waves, under 4000 bytes
CARVE = dict(n_lines=10, n_theta0=3, N=7, ws=5, max_waves=4, budget=4000)

PROGRAM = r"""
#include <cstdio>
#include <initializer_list>
#include "ibs_plan.hpp"
using namespace ibs;

static void show(long n_lines, int n_theta0, long option, size_t budget, size_t fixed, size_t per_line) {
  const LineChunks ch = plan_line_chunks(n_lines, n_theta0, option, budget, [&](long L) { return fixed + per_line * (size_t)L; });
  std::printf("%%ld %%zu\n", ch.lines, ch.bytes);
}

// the workspace of scan_rows_chunked: nw * ws doubles, then three rows of S * N doubles
struct Rows { double *work, *G, *C, *F; };
static Rows rows(Carve& cv, long L, int n_theta0, int N, size_t ws, long max_waves) {
  const long S = L * n_theta0, nw = S < max_waves ? S : max_waves;
  Rows r;
  r.work = cv.take<double>((size_t)nw * ws);
  r.G = cv.take<double>((size_t)S * N); r.C = cv.take<double>((size_t)S * N); r.F = cv.take<double>((size_t)S * N);
  return r;
}

int main() {
  std::printf("%%zu\n", kLineChunkBudget);
  for (long n_lines : {%(n_lines)s}) for (int n_theta0 : {%(n_theta0)s}) for (long option : {%(option)s})
    for (size_t per_line : {%(per_line)s}) for (size_t fixed : {%(fixed)s})
      show(n_lines, n_theta0, option, kLineChunkBudget, fixed, per_line);
%(hand)s
  const LineChunks ch = plan_line_chunks(%(c_n_lines)dL, %(c_n_theta0)d, 0, %(c_budget)d,
                                         [&](long L) { Carve sz{nullptr}; rows(sz, L, %(c_n_theta0)d, %(c_N)d, %(c_ws)d, %(c_max_waves)d); return sz.off; });
  alignas(256) static char buf[8192];
  Carve cv{buf};
  const Rows r = rows(cv, ch.lines, %(c_n_theta0)d, %(c_N)d, %(c_ws)d, %(c_max_waves)d);
  std::printf("%%ld %%zu %%td %%td %%td %%td %%zu\n", ch.lines, ch.bytes, (char*)r.work - buf, (char*)r.G - buf, (char*)r.C - buf, (char*)r.F - buf, cv.off);
  std::printf("%%zu %%zu %%zu %%zu\n", pad256(0), pad256(1), pad256(256), pad256(257));
  return 0;
}
"""


def plan_line_chunks(n_lines, n_theta0, option, budget, bytes_of):
    """the rule, restated: the option's systems in whole lines; else n_lines halved, rounding up, while over the budget; then [1, n_lines]"""
    if option > 0:
        lines = option // n_theta0
    else:
        lines = n_lines
        while lines > 1 and bytes_of(lines) > budget:
            lines = (lines + 1) // 2
    lines = min(max(lines, 1), n_lines)
    return lines, bytes_of(lines)


def pad256(b):
    return -(-b // 256) * 256


def run(tmp_path):
    lst = lambda v, suffix="": ", ".join("%d%s" % (x, suffix) for x in v)
    hand = "\n".join("  show(%d, %d, %dL, 1000, 0, %d);" % case for case, _ in HAND)
    src, exe = tmp_path / "line_chunks.cpp", tmp_path / "line_chunks"
    src.write_text(PROGRAM % dict(n_lines=lst(N_LINES, "L"), n_theta0=lst(N_THETA0), option=lst(OPTION, "L"), per_line=lst(PER_LINE, "ull"),
                                  fixed=lst(FIXED, "ull"), hand=hand, **{"c_" + k: v for k, v in CARVE.items()}))
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()
    return [tuple(int(x) for x in ln.split()) for ln in out]


def test_chunk_rule_and_carve(tmp_path):
    out = run(tmp_path)
    assert out[0] == (BUDGET,)
    sweep = list(itertools.product(N_LINES, N_THETA0, OPTION, PER_LINE, FIXED))
    got, rest = out[1:1 + len(sweep)], out[1 + len(sweep):]
    halved = 0
    for (n_lines, n_theta0, option, per_line, fixed), g in zip(sweep, got):
        want = plan_line_chunks(n_lines, n_theta0, option, BUDGET, lambda L: fixed + per_line * L)
        assert g == want, (n_lines, n_theta0, option, per_line, fixed, g, want)
        assert 1 <= g[0] <= n_lines and (option > 0 or g[0] == 1 or g[1] <= BUDGET)
        halved += option == 0 and g[0] < n_lines
    assert halved > 20, halved                      # (the budget branch is walked, not only the option)
    # the cases by hand
    for (case, want), g in zip(HAND, rest):
        assert g == want, (case, g, want)
        assert plan_line_chunks(case[0], case[1], case[2], 1000, lambda L: case[3] * L) == want, case
    # through Carve: counting pass = carving pass = pad256 arithmetic (take() aligns, then takes)
    c = CARVE

    def offsets(L):
        S = L * c["n_theta0"]
        work = 0
        G = pad256(work + 8 * min(S, c["max_waves"]) * c["ws"])
        C = pad256(G + 8 * S * c["N"])
        F = pad256(C + 8 * S * c["N"])
        return work, G, C, F, F + 8 * S * c["N"]

    lines, nbytes = plan_line_chunks(c["n_lines"], c["n_theta0"], 0, c["budget"], lambda L: offsets(L)[4])
    assert 1 < lines < c["n_lines"] and offsets(lines)[1] % 256 == 0 and 8 * min(lines * c["n_theta0"], c["max_waves"]) * c["ws"] % 256 != 0
    assert rest[len(HAND)] == (lines, nbytes) + offsets(lines), (rest[len(HAND)], lines, nbytes, offsets(lines))
    assert rest[len(HAND) + 1] == (0, 256, 256, 512)
