"""CPU: launch planning (csrc/ibs_plan.hpp: which kernel form and launch shape serves a call), walked over its thresholds.

A stand-alone C++ program (host compiler only, no HIP, no GPU) includes the header and sweeps plan_scan and plan_gcf on
Chip{256 CUs, 160 KB} with built_full(), one line per case.  The lines are compared with tests/golden/P1_scan_plans.txt and
P1_gcf_plans.txt, which were written from the decision code as it stood in the C-ABI layer before it was cut into the header
(stored as the distinct plan lines plus nested, run-length coded blocks of their indices: compact()).  A change of a threshold or a form changes the golden: then
regenerate it ON PURPOSE (python tests/test_plan_cpu.py --regenerate) and say so in the commit.

Scan sweep: N x n_lines x n_theta0 x warm x want_x x force_p x scan_chain as listed in SCAN_COUNTS below (77,760 cases), then
t0_per_line at n_theta0 = 1, scan_resident = 0 / 1 at N = 195, 513, the fused argmax under pack_mode = 0, 1, 2, and Chip{256, 64 KB}
at N = 1025, 2049 (the "does not fit the LDS staging" exit).  Raw-solve sweep: elem x N (the same list and the rows / direct thresholds
1537, 1795) x n_sys x has_gh x want_gam x want_x x gcf_rows x gcf_direct x f32_lam x force_p.

Independent of the golden, the program asserts on every plan without an error: 1 <= wpb <= the waves of the chosen kernel's
__launch_bounds__; the LDS bytes its launcher will request fit the chip; 1 <= chain <= theta0 slots on chained plans and chain = 0
elsewhere; n_theta0 % G == 0 on sub-wave scan plans; resident only on form Wave with 3 <= M <= 8; the fused argmax only on Wave /
WaveLean; lists_suspects only on direct or group forms; and the form is one `built` holds -- also on slices of both sweeps with the
16-lane forms, and then the direct forms, cleared from `built`."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ideal-ballooning-solver_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden")

SCAN_FORMS = ("Wave", "WaveLean", "WaveChain", "Group", "GroupChain", "Long")
GCF_FORMS = ("Staged", "Rows", "Direct", "F32", "F32Wide", "F32WideRows", "F32WideDirect", "F32LamDirect", "Group", "GroupWide", "Long")
# the main scan sweep: 18 N x 10 n_lines x 9 n_theta0 x 2 x 2 x 4 force_p x 3 scan_chain, and the cases per form in it
SCAN_MAIN = 18 * 10 * 9 * 2 * 2 * 4 * 3
SCAN_COUNTS = dict(Wave=42906, WaveLean=3854, WaveChain=10420, Group=3724, GroupChain=8216, Long=8640)
SCAN_EXTRA = 18 * 10 * 2 + 2 * 10 * 9 * 2 * 2 + 10 * 9 * 3 + 2 * 10 * 9 * 2 * 2
GCF_CASES = 2 * 20 * 10 * 2 * 2 * 2 * 3 * 3 * 3 * 4

PROGRAM = r"""
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include "ibs_plan.hpp"
using namespace ibs;

static long bad = 0;
#define CHECK(c, ...) do { if (!(c)) { if (bad < 20) { std::fprintf(stderr, "FAIL %s: ", #c); std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); } ++bad; } } while (0)

static const int kN[] = {67, 97, 99, 129, 131, 195, 257, 259, 513, 577, 579, 641, 643, 1025, 1475, 2049, 2051, 4097};
static const int kLines[] = {1, 3, 8, 9, 64, 256, 257, 1024, 4096, 16384};
static const int kT0[] = {1, 2, 3, 4, 7, 8, 16, 33, 64};
static const char* kScanForm[] = {"Wave", "WaveLean", "WaveChain", "Group", "GroupChain", "Long"};
static const char* kGcfForm[] = {"Staged", "Rows", "Direct", "F32", "F32Wide", "F32WideRows", "F32WideDirect", "F32LamDirect", "Group", "GroupWide", "Long"};

static bool scan_built(const Built& b, const ScanPlan& p) {
  const int pi = p.P == 32 ? 0 : 1;
  switch (p.form) {
    case ScanForm::Wave: case ScanForm::WaveLean: case ScanForm::Long: return has(b.scan, p.M);
    case ScanForm::WaveChain: return has(b.scan_chain, p.M);
    case ScanForm::Group: return has(b.scan_g[pi], p.M);
    case ScanForm::GroupChain: return has(b.scan_chain_g[pi], p.M);
  }
  return false;
}

static void scan_case(const Chip& chip, const PlanOpts& o, const Built& b, int n_lines, int n_t0, int N, bool warm, bool want_x, bool per_line,
                      bool want_pack, bool print) {
  const ScanPlan p = plan_scan(chip, o, b, n_lines, n_t0, N, warm, want_x, per_line, want_pack);
  if (p.err != PlanError::None) {
    if (print) { if (p.err == PlanError::NotBuilt) std::printf("ERR NotBuilt M=%d\n", p.M); else std::printf("ERR NoLds\n"); }
    return;
  }
  if (print)
    std::printf("%s P%d M%d wpb%d chain%d res%d pack%d%d\n", kScanForm[(int)p.form], p.P, p.M, p.wpb, p.chain, p.resident, (int)p.fused_pack, p.pack_mode);
#define WHERE "N=%d %dx%d warm=%d x=%d P=%d chain=%d form=%s", N, n_lines, n_t0, (int)warm, (int)want_x, o.force_p, o.scan_chain, kScanForm[(int)p.form]
  CHECK(scan_built(b, p), WHERE);
  const bool group = p.form == ScanForm::Group || p.form == ScanForm::GroupChain;
  const bool chained = p.form == ScanForm::WaveChain || p.form == ScanForm::GroupChain;
  const bool wave1 = p.form == ScanForm::Wave || p.form == ScanForm::WaveLean;
  CHECK(group == (p.P != 64) && (p.P == 64 || p.P == 32 || p.P == 16), WHERE);
  CHECK(p.resident == 0 || (p.form == ScanForm::Wave && p.M >= 3 && p.M <= 8), WHERE);
  CHECK(p.form != ScanForm::WaveLean || (p.M >= 3 && p.M <= 8), WHERE);
  CHECK(!p.fused_pack || (wave1 && want_pack), WHERE);
  CHECK((p.pack_mode != 0) == p.fused_pack && p.pack_mode >= 0 && p.pack_mode <= 2, WHERE);
  if (p.form == ScanForm::Long) { CHECK(p.wpb == 1 && p.chain == 0 && p.M == 1, WHERE); return; }
  const int G = 64 / p.P, cap = (group ? scan_max_threads_g(p.M) : scan_max_threads(p.M)) / 64;
  CHECK(p.M == (group ? group_rows(N, p.P) : rows_per_lane(N)), WHERE);
  CHECK(p.wpb >= 1 && p.wpb <= cap, WHERE);
  if (group) CHECK(n_t0 % G == 0, WHERE);
  if (chained) CHECK(p.chain >= 1 && p.chain <= n_t0 / G, WHERE); else CHECK(p.chain == 0, WHERE);
  const bool need_x = p.form == ScanForm::WaveChain ? scan_chain_need_x(p.M, want_x) : (p.form == ScanForm::GroupChain ? want_x : true);
  const size_t lds = (size_t)scan_lds_rows(p.wpb, G, need_x) * lds_pitch(N) * sizeof(double);
  CHECK(lds <= (size_t)chip.lds_per_block, WHERE);
#undef WHERE
}

static void gcf_case(const Chip& chip, const PlanOpts& o, const Built& b, int elem, long n_sys, int N, bool gh, bool want_gam, bool want_x, bool print) {
  const GcfPlan p = plan_gcf(chip, o, b, elem, n_sys, N, gh, want_gam, want_x);
  if (p.err != PlanError::None) {
    if (print) { if (p.err == PlanError::NotBuilt) std::printf("ERR NotBuilt M=%d\n", p.M); else std::printf("ERR NoLds pw=%zu\n", p.per_wave); }
    return;
  }
  if (print)
    std::printf("%s P%d M%d wpb%d pw%zu lists%d direct%d\n", kGcfForm[(int)p.form], p.P, p.M, p.wpb, p.per_wave, (int)p.lists_suspects, (int)p.direct_form);
#define WHERE "elem=%d N=%d n=%ld gh=%d gam=%d x=%d rows=%d direct=%d f32lam=%d P=%d form=%s", elem, N, n_sys, (int)gh, (int)want_gam, (int)want_x, \
              o.gcf_rows, o.gcf_direct, o.f32_lam, o.force_p, kGcfForm[(int)p.form]
  const int pi = p.P == 32 ? 0 : 1, G = 64 / p.P;
  const size_t row = (size_t)lds_pitch(N) * sizeof(double);
  size_t lds = 0; bool built = false, f64_form = true;
  switch (p.form) {
    case GcfForm::Staged: built = has(b.gcf_f64, p.M); lds = 3 * row * p.wpb; break;
    case GcfForm::Rows: built = has(b.gcf_rows, p.M); lds = row * p.wpb; break;
    case GcfForm::Direct: built = has(b.gcf_direct, p.M); lds = want_x ? row * p.wpb : 0; break;
    case GcfForm::Group: built = has(b.gcf_g[pi], p.M); lds = row * G * p.wpb; break;
    case GcfForm::F32: built = has(b.gcf_f32, p.M); lds = 3 * row / 2 * p.wpb; f64_form = false; break;
    case GcfForm::F32Wide: built = has(b.gcf_f32_wide, p.M); lds = 3 * row * p.wpb; f64_form = false; break;
    case GcfForm::F32WideRows: built = has(b.gcf_f32w_rows, p.M); lds = row * p.wpb; f64_form = false; break;
    case GcfForm::F32WideDirect: built = has(b.gcf_f32w_direct, p.M); lds = want_x ? row * p.wpb : 0; f64_form = false; break;
    case GcfForm::F32LamDirect: built = has(b.gcf_f32lam_direct, p.M); lds = 0; f64_form = false; CHECK(!want_gam && !want_x, WHERE); break;
    case GcfForm::GroupWide: built = has(b.gcf_f32w_g[pi], p.M); lds = row * G * p.wpb; f64_form = false; break;
    case GcfForm::Long: built = has(elem == 8 ? b.gcf_f64 : b.gcf_f32, 1); f64_form = elem == 8; CHECK(p.M == 1 && N > 2050, WHERE); break;
  }
  CHECK(built, WHERE);
  CHECK(f64_form == (elem == 8), WHERE);
  CHECK(p.wpb >= 1 && p.wpb <= kGcfMaxWaves, WHERE);
  if (p.form != GcfForm::Long) CHECK(lds == p.per_wave * p.wpb && lds <= (size_t)chip.lds_per_block, WHERE);
  const bool grp = p.form == GcfForm::Group || p.form == GcfForm::GroupWide;
  const bool direct = p.form == GcfForm::Direct || p.form == GcfForm::F32WideDirect || p.form == GcfForm::F32LamDirect;
  CHECK(grp == (p.P != 64) && (!grp || p.M == group_rows(N, p.P)), WHERE);
  CHECK(!p.lists_suspects || grp || direct, WHERE);
  CHECK(p.direct_form == direct, WHERE);
  CHECK(!gh || p.form == GcfForm::Staged || p.form == GcfForm::Long, WHERE);
#undef WHERE
}

static void scan_main(const Chip& chip, const Built& b, bool print, bool slice) {
  for (int N : kN) for (int nl : kLines) for (int nt : kT0) for (int warm = 0; warm < 2; ++warm) for (int x = 0; x < 2; ++x)
    for (int fp : {0, 16, 32, 64}) for (int ch : {0, 1, 2}) {
      if (slice && N != 131 && N != 257 && N != 513) continue;
      PlanOpts o; o.force_p = fp; o.scan_chain = ch;
      scan_case(chip, o, b, nl, nt, N, warm, x, false, false, print);
    }
}

static void gcf_main(const Chip& chip, const Built& b, bool print, bool slice) {
  static const int extra[] = {1537, 1795};
  static const long kSys[] = {1, 255, 256, 1024, 1025, 2047, 2048, 4096, 65536, 1L << 19};
  for (int elem : {8, 4}) for (int k = 0; k < 20; ++k) {
    const int N = k < 18 ? kN[k] : extra[k - 18];
    if (slice && N != 131 && N != 257 && N != 1025 && N != 1795) continue;
    for (long n : kSys) for (int fp : {0, 16, 32, 64}) for (int x = 0; x < 2; ++x) for (int dir : {-1, 0, 1}) for (int rows : {-1, 0, 1})
      for (int gh = 0; gh < 2; ++gh) for (int gam = 0; gam < 2; ++gam) for (int fl : {0, 1, 2}) {
        PlanOpts o; o.gcf_rows = rows; o.gcf_direct = dir; o.f32_lam = fl; o.force_p = fp;
        gcf_case(chip, o, b, elem, n, N, gh && elem == 8, gam, x, print);      // (the FP32 entry point takes no half-grid g)
      }
  }
}

int main(int argc, char** argv) {
  const Chip chip{256, 160 * 1024};
  const Built full = built_full();
  if (argc > 1 && !std::strcmp(argv[1], "scan")) {
    scan_main(chip, full, true, false);
    // one theta0 per line (ibs_gamma_points_f64)
    for (int N : kN) for (int nl : kLines) for (int x = 0; x < 2; ++x) scan_case(chip, PlanOpts{}, full, nl, 1, N, false, x, true, false, true);
    // option scan_resident
    for (int N : {195, 513}) for (int nl : kLines) for (int nt : kT0) for (int warm = 0; warm < 2; ++warm) for (int r = 0; r < 2; ++r) {
      PlanOpts o; o.scan_resident = r;
      scan_case(chip, o, full, nl, nt, N, warm, false, false, false, true);
    }
    // the fused argmax and its hand-off mode
    for (int nl : kLines) for (int nt : kT0) for (int pm = 0; pm < 3; ++pm) {
      PlanOpts o; o.pack_mode = pm;
      scan_case(chip, o, full, nl, nt, 513, false, false, false, true, true);
    }
    // a chip with 64 KB of LDS: the staged line does not fit
    for (int N : {1025, 2049}) for (int nl : kLines) for (int nt : kT0) for (int warm = 0; warm < 2; ++warm) for (int x = 0; x < 2; ++x)
      scan_case(Chip{256, 64 * 1024}, PlanOpts{}, full, nl, nt, N, warm, x, false, false, true);
  } else if (argc > 1 && !std::strcmp(argv[1], "gcf")) {
    gcf_main(chip, full, true, false);
  } else {
    // fall-backs of a partial build: without the 16-lane forms, then without the direct forms
    Built no16 = full;
    no16.gcf_g[1] = no16.gcf_f32w_g[1] = no16.scan_g[1] = no16.scan_chain_g[1] = 0;
    Built nodirect = full;
    nodirect.gcf_direct = nodirect.gcf_f32w_direct = nodirect.gcf_f32lam_direct = 0;
    for (const Built& b : {no16, nodirect}) { scan_main(chip, b, false, true); gcf_main(chip, b, false, true); }
    // ... and a build without the chained sub-wave kernels: a warm start then stays with one wave per system
    Built nochain = full;
    nochain.scan_chain_g[0] = nochain.scan_chain_g[1] = 0;
    scan_main(chip, nochain, false, true);
    CHECK(check_grid_length(65, true) == GridCheck::Range && check_grid_length(67, false) == GridCheck::Ok && check_grid_length(68, true) == GridCheck::Even, "grid");
    CHECK(check_grid_length(2051, false) == GridCheck::Range && check_grid_length(65537, true) == GridCheck::Ok && check_grid_length(65539, true) == GridCheck::Range, "grid");
    std::printf("slices done\n");
  }
  std::fprintf(stderr, "bad %ld\n", bad);
  return bad ? 1 : 0;
}
"""


def build(tmp_path):
    src, exe = tmp_path / "plan_check.cpp", tmp_path / "plan_check"
    src.write_text(PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)])
    return str(exe)


def run(exe, what):
    p = subprocess.run([exe, what], capture_output=True, text=True)
    assert p.returncode == 0 and p.stderr.strip().endswith("bad 0"), p.stderr[-4000:]
    return p.stdout.splitlines()


# block sizes of the golden form, innermost loops first.  Scan: scan_chain | force_p | warm x want_x | n_theta0; raw solves:
# f32_lam x want_gam | has_gh x gcf_rows | gcf_direct x want_x
LEVELS = dict(scan=(3, 4, 4, 9), gcf=(6, 6, 6))


def rle(seq):
    runs = []
    for k in seq:
        if runs and runs[-1][0] == k:
            runs[-1][1] += 1
        else:
            runs.append([k, 1])
    return " ".join("%d*%d" % (k, n) if n > 1 else "%d" % k for k, n in runs)


def compact(lines, levels):
    """the golden form of a sweep: the case count; the distinct lines in order of first appearance; then, per level, the distinct
    blocks of that many consecutive indices of the level below (run-length coded, index*count; ten blocks per row), again in order of first appearance;
    last the sequence of the top level's block indices, 24 runs per row"""
    out = ["cases %d" % len(lines)]
    seq = lines
    for size in (1,) + tuple(levels):
        index, order, nxt = {}, [], []
        for i in range(0, len(seq), size):
            b = seq[i] if size == 1 else rle(seq[i:i + size])
            if b not in index:
                index[b] = len(order)
                order.append(b)
            nxt.append(index[b])
        if size == 1:
            out += ["plans %d" % len(order)] + order
        else:
            out += ["blocks of %d: %d" % (size, len(order))] + [" ; ".join(order[i:i + 10]) for i in range(0, len(order), 10)]
        seq = nxt
    top = rle(seq).split(" ")
    out += ["top %d" % len(top)] + [" ".join(top[i:i + 24]) for i in range(0, len(top), 24)]
    return "\n".join(out) + "\n"


def counts(lines, forms):
    c = {f: 0 for f in forms}
    c["ERR"] = 0
    for ln in lines:
        c[ln.split(" ", 1)[0]] += 1
    return c


def test_scan_plans_equal_the_golden(tmp_path):
    lines = run(build(tmp_path), "scan")
    assert len(lines) == SCAN_MAIN + SCAN_EXTRA, len(lines)
    main = counts(lines[:SCAN_MAIN], SCAN_FORMS)
    print(main, len(set(lines[:SCAN_MAIN])))
    assert main == dict(SCAN_COUNTS, ERR=0), main
    assert counts(lines[SCAN_MAIN:], SCAN_FORMS)["ERR"] == 2 * 10 * 9 * 2 * 2            # the 64 KB pass
    with open(os.path.join(GOLDEN, "P1_scan_plans.txt")) as fh:
        golden = fh.read()
    assert golden.startswith("cases %d\n" % (SCAN_MAIN + SCAN_EXTRA))
    assert compact(lines, LEVELS["scan"]) == golden


def test_gcf_plans_equal_the_golden(tmp_path):
    lines = run(build(tmp_path), "gcf")
    assert len(lines) == GCF_CASES, len(lines)
    c = counts(lines, GCF_FORMS)
    print(c, len(set(lines)))
    assert c["ERR"] == 0 and all(c[f] > 0 for f in GCF_FORMS), c
    with open(os.path.join(GOLDEN, "P1_gcf_plans.txt")) as fh:
        golden = fh.read()
    assert golden.startswith("cases %d\n" % GCF_CASES)
    assert compact(lines, LEVELS["gcf"]) == golden


def test_plan_invariants_on_partial_builds(tmp_path):
    assert run(build(tmp_path), "slices") == ["slices done"]


if __name__ == "__main__":
    import pathlib
    import tempfile
    assert sys.argv[1:] == ["--regenerate"], __doc__
    with tempfile.TemporaryDirectory() as d:
        exe = build(pathlib.Path(d))
        for what in ("scan", "gcf"):
            with open(os.path.join(GOLDEN, "P1_%s_plans.txt" % what), "w") as fh:
                fh.write(compact(run(exe, what), LEVELS[what]))
