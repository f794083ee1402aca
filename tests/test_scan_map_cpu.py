"""CPU: the block -> (line, part) map of the one-wave theta0 scans (csrc/ibs_scan_map.hpp: the grid launch_scan / launch_scan_chain
launch and what a block of k_gamma_scan, k_gamma_scan_lean and k_gamma_scan_chain reads from its indices), walked block by block.

A stand-alone C++ program (host compiler only, no GPU, no sanitizer) includes the header and, for n_lines = 1 .. 41, 64, 65 and
nparts = 1, 2, 3, 5, 8, checks of the 3-D form that
  * the live blocks cover every (line, part) exactly once, the others have line >= n_lines, and the grid holds
    min(8, n_lines) * nparts * ceil(n_lines / 8) blocks (no idle block when n_lines < 8 or n_lines % 8 == 0);
  * in the linear order of the workgroups, x + gx (y + gy z), the blocks of one line lie a multiple of 8 apart whenever the launch
    has more than one chunk (they share an XCD's L2), and wherever every chunk is full the block at linear place b is the block b of
    the 1-D form;
and of the 1-D form -- selected with the grid limit lowered to 4 so that small launches take it, and at the real limit of 65,535
chunks or parts -- that every block is live and the cover is exact as well.  The limit itself: 8 * 65,535 lines still launch 3-D,
one line more, or 65,536 parts, launch 1-D with nparts * n_lines blocks."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ideal-ballooning-solver_amd", "csrc")

PROGRAM = r"""
#include <cstdio>
#include <vector>
#include "ibs_scan_map.hpp"

static long bad = 0;
#define CHECK(c, ...) do { if (!(c)) { if (bad < 20) { std::printf("FAIL %s: ", #c); std::printf(__VA_ARGS__); std::printf("\n"); } ++bad; } } while (0)

static void walk_3d(int n_lines, int nparts) {
  const ibs::ScanGrid g = ibs::scan_grid(n_lines, nparts);
  const int chunks = (n_lines + 7) / 8, gx = n_lines < 8 ? n_lines : 8;
  CHECK(g.flat == 0 && (int)g.x == gx && (int)g.y == nparts && (int)g.z == chunks, "grid %d %d: %u %u %u flat %d", n_lines, nparts, g.x, g.y, g.z, g.flat);
  CHECK(g.blocks() == (long)gx * nparts * chunks, "blocks %d %d", n_lines, nparts);
  std::vector<int> seen(n_lines * nparts, 0);
  std::vector<long> first(n_lines, -1);
  long live = 0;
  const bool full = n_lines < 8 || n_lines % 8 == 0;
  for (unsigned z = 0; z < g.z; ++z) for (unsigned y = 0; y < g.y; ++y) for (unsigned x = 0; x < g.x; ++x) {
    const long b = x + (long)g.x * (y + (long)g.y * z);
    const ibs::ScanBlock s = ibs::scan_block_3d(n_lines, x, y, z, g.y);
    CHECK(s.nparts == nparts && s.part == (int)y, "part %d %d", n_lines, nparts);
    CHECK(s.live == (s.line < n_lines), "live %d %d line %d", n_lines, nparts, s.line);
    if (!s.live) { CHECK(z == g.z - 1 && !full, "idle block outside a partial last chunk %d %d", n_lines, nparts); continue; }
    ++live;
    CHECK(s.line >= 0 && s.part >= 0 && s.part < nparts, "range %d %d", n_lines, nparts);
    ++seen[s.line * nparts + s.part];
    if (first[s.line] < 0) first[s.line] = b;
    if (chunks > 1) CHECK((b - first[s.line]) % 8 == 0, "line %d of %d x %d: blocks %ld and %ld on different XCDs", s.line, n_lines, nparts, first[s.line], b);
    if (full || (int)z < chunks - 1) {
      const ibs::ScanBlock o = ibs::scan_block_1d(n_lines, nparts, (unsigned)b);
      CHECK(o.live && o.line == s.line && o.part == s.part, "1-D order %d %d block %ld: (%d, %d) vs (%d, %d)", n_lines, nparts, b, o.line, o.part, s.line, s.part);
    }
  }
  CHECK(live == (long)n_lines * nparts, "live count %d %d", n_lines, nparts);
  if (full) CHECK(live == g.blocks(), "idle blocks in a launch of full chunks %d %d", n_lines, nparts);
  for (int v : seen) CHECK(v == 1, "cover %d %d", n_lines, nparts);
}

static void walk_1d(int n_lines, int nparts, long limit) {
  const ibs::ScanGrid g = ibs::scan_grid(n_lines, nparts, limit);
  CHECK(g.flat == 1 && g.x == (unsigned)(n_lines * nparts) && g.y == 1 && g.z == 1, "flat grid %d %d", n_lines, nparts);
  std::vector<int> seen(n_lines * nparts, 0);
  for (unsigned b = 0; b < g.x; ++b) {
    const ibs::ScanBlock s = ibs::scan_block_1d(n_lines, nparts, b);
    CHECK(s.live && s.nparts == nparts && s.line >= 0 && s.line < n_lines && s.part >= 0 && s.part < nparts, "1-D range %d %d block %u", n_lines, nparts, b);
    if (s.line >= 0 && s.line < n_lines && s.part >= 0 && s.part < nparts) ++seen[s.line * nparts + s.part];
  }
  for (int v : seen) CHECK(v == 1, "1-D cover %d %d", n_lines, nparts);
}

int main() {
  long cases = 0;
  const int parts[] = {1, 2, 3, 5, 8};
  for (int n_lines = 1; n_lines <= 65; ++n_lines) {
    if (n_lines > 41 && n_lines < 64) continue;
    for (int np : parts) { walk_3d(n_lines, np); ++cases; }
  }
  // the 1-D form, on launches a lowered limit sends there: 5 chunks or more, or 5 parts or more
  for (int n_lines : {33, 40, 41, 47, 65}) for (int np : parts) { walk_1d(n_lines, np, 4); ++cases; }
  for (int n_lines : {1, 7, 9}) for (int np : {5, 8}) { walk_1d(n_lines, np, 4); ++cases; }
  CHECK(ibs::scan_grid(32, 4, 4).flat == 0 && ibs::scan_grid(33, 4, 4).flat == 1 && ibs::scan_grid(32, 5, 4).flat == 1, "lowered limit");
  // the real limit
  const long L = ibs::kScanGridLimit;
  CHECK(L == 65535, "limit");
  { const ibs::ScanGrid g = ibs::scan_grid(8 * L, 3); CHECK(g.flat == 0 && g.x == 8 && g.y == 3 && g.z == (unsigned)L, "largest 3-D launch in z"); }
  { const ibs::ScanGrid g = ibs::scan_grid(5, L); CHECK(g.flat == 0 && g.x == 5 && g.y == (unsigned)L && g.z == 1, "largest 3-D launch in y"); }
  { const ibs::ScanGrid g = ibs::scan_grid(5, L + 1); CHECK(g.flat == 1 && g.x == (unsigned)(5 * (L + 1)) && g.y == 1 && g.z == 1, "first 1-D launch in y"); }
  {
    const int n_lines = (int)(8 * L + 1), np = 3;
    const ibs::ScanGrid g = ibs::scan_grid(n_lines, np);
    CHECK(g.flat == 1 && g.x == (unsigned)((long)n_lines * np) && g.y == 1 && g.z == 1, "first 1-D launch in z");
    // its last chunk holds one line: the last three blocks are that line's three parts; the block before them ends the last full chunk
    for (int k = 0; k < np; ++k) {
      const ibs::ScanBlock s = ibs::scan_block_1d(n_lines, np, g.x - np + k);
      CHECK(s.live && s.line == n_lines - 1 && s.part == k, "last chunk, block %d: (%d, %d)", k, s.line, s.part);
    }
    const ibs::ScanBlock p = ibs::scan_block_1d(n_lines, np, g.x - np - 1);
    CHECK(p.live && p.line == n_lines - 2 && p.part == np - 1, "end of the last full chunk: (%d, %d)", p.line, p.part);
    const ibs::ScanBlock f = ibs::scan_block_1d(n_lines, np, 8 * np + 9);
    CHECK(f.live && f.line == 9 && f.part == 1, "second chunk: (%d, %d)", f.line, f.part);
    ++cases;
  }
  std::printf("map cases %ld bad %ld\n", cases, bad);
  return bad ? 1 : 0;
}
"""


def test_scan_block_map_covers_every_line_and_part_once(tmp_path):
    src, exe = tmp_path / "scan_map_check.cpp", tmp_path / "scan_map_check"
    src.write_text(PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)])
    p = subprocess.run([str(exe)], capture_output=True, text=True)
    print(p.stdout)
    assert p.returncode == 0, p.stdout + p.stderr
    words = [ln.split() for ln in p.stdout.splitlines() if ln.startswith("map cases")][0]
    assert int(words[2]) == 43 * 5 + 5 * 5 + 3 * 2 + 1 and int(words[4]) == 0, words
