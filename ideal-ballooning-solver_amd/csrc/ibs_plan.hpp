// Launch planning: which kernel form and launch shape serves a call -- lanes per system, staged / row-streamed / direct rows,
// chained or not, resident or lean, waves per block, chain length.  The single definition: the C-ABI layer (ibs_api.hip) calls
// the planners and maps the form to a launcher, the launchers (ibs_kernels.hip, ibs_kernels_group.hip) size their LDS with the
// functions below.  Plain C++17, no HIP, no allocation, so that the host can walk every threshold without a GPU
// (tests/test_plan_cpu.py, whose golden tables have to be regenerated ON PURPOSE when a form or a threshold changes here).
#pragma once
#include <cstddef>
#include <cstdint>

// fewest rows per lane for which a form of the raw solves is built (the registrar of ibs_kernels.hip): the row-streamed
// k_solve_gcf_rows from N >= 1475; of the read-from-global-memory forms k_solve_gcf_direct (FP64 solver) where the staging limits
// the occupancy (N > 578; below, the sub-wave forms are faster: tools/bench_forms.py), the all-FP32 eigenvalue-only form
// k_solve_gcf_f32lam_direct on every big batch
#ifndef IBS_ROWS_MIN_M
#define IBS_ROWS_MIN_M 24
#endif
#ifndef IBS_DIRECT_MIN_M
#define IBS_DIRECT_MIN_M 9
#endif
#ifndef IBS_F32LAM_DIRECT_MIN_M
#define IBS_F32LAM_DIRECT_MIN_M 3
#endif

namespace ibs {

constexpr int kMaxM = 32;   // rows per lane: N - 2 <= 64 * kMaxM  (N <= 2050)
constexpr int kMaxLongN = 65537;   // longer grids, up to this many points, run on the generic division-form path (ibs_long.hip)
constexpr int kMaxModes = 16;      // eigenpairs per system of the spectrum mode (ibs_modes.hpp, ibs_modes.hip)

// LDS rows of the wave kernels are padded by one element per 8 (element j lives at j + (j >> 3)): a lane reads a
// contiguous chunk of ~M rows, i.e. lanes are M elements apart, and for even M (8 at N = 513) an unpadded row
// puts 16 lanes on the same banks.  Row pitch in elements:
constexpr int lds_pitch(int N) { return N + (N >> 3) + 1; }

// threads per block the scan kernel is compiled for (register budget: 5M doubles per lane)
constexpr int scan_max_threads(int M) { return M <= 16 ? 512 : 256; }
constexpr int scan_max_threads_g(int M) { return M <= 8 ? 512 : 256; }   // sub-wave kernels (ibs_group.hpp)
constexpr int kGcfMaxWaves = 4;     // waves per block of the raw-solve, Sturm and objective kernels (__launch_bounds__(256))

// k_gamma_scan is built in two forms for these rows per lane: resident (set-up rows carried in registers) and k_gamma_scan_lean
constexpr bool scan_resident_built(int M) { return M >= 3 && M <= 8; }

// ---------------------------------------------------------------- inputs
struct Chip { int n_cu; int lds_per_block; };

// Diagnostic overrides of the dispatch heuristics that steer planning (C ABI: ibs_set_option)
struct PlanOpts {
  int force_p = 0;        // lanes per system: 64 | 32 | 16
  int scan_chain = 0;     // theta0 values chained through one wave / group
  int scan_resident = -1; // k_gamma_scan, 3 <= rows per lane <= 8: -1 = the resident form up to two waves per SIMD and k_gamma_scan_lean above, 0 = lean everywhere, 1 = resident wherever built
  int gcf_rows = -1;      // raw systems on long grids: -1 / 1 = row-streamed kernel, 0 = the 3-row staging of k_solve_gcf
  int gcf_direct = -1;    // raw systems, one wave per system: rows read straight from global memory (k_solve_gcf_direct): -1 = by batch size, 0 = never, 1 = always
  int f32_lam = 0;        // FP32 eigenvalue-only requests: 0 = by grid size, 1 = all-FP32 iteration + FP64 certificate, 2 = FP32 in HBM + FP64 solver
  int pack_mode = 0;      // hand-off of the fused scan + argmax: 1 = write-through + sc1 loads, 2 = release / acquire fences
  int sturm_form = 0;     // ibs_sturm_count_f64: 0 = by size (plan_sturm), 1 = prefix-product sweep (N <= 2050), 2 = division form, lanes as systems, 3 = division form, one wave per system
};

// Which forms exist in this build: bit M of a mask = the form is built for M rows per lane (sub-wave forms: index 0 = 32 lanes per
// system, 1 = 16).  The API fills it once per context from the non-null entries of launch_table(), so partial builds keep working.
struct Built {
  uint64_t gcf_f64, gcf_f32, gcf_f32_wide, scan, scan_chain;        // ibs_kernels.hip, every M it is compiled for
  uint64_t gcf_rows, gcf_f32w_rows;                                 // ... M >= IBS_ROWS_MIN_M
  uint64_t gcf_direct, gcf_f32w_direct, gcf_f32lam_direct;          // ... M >= IBS_DIRECT_MIN_M / IBS_F32LAM_DIRECT_MIN_M
  uint64_t gcf_g[2], gcf_f32w_g[2], scan_g[2], scan_chain_g[2];     // ibs_kernels_group.hip
};
constexpr bool has(uint64_t mask, int M) { return M >= 0 && M < 64 && ((mask >> M) & 1); }
constexpr uint64_t m_range(int lo, int hi) { return ((~uint64_t(0)) >> (63 - hi)) & ~((uint64_t(1) << lo) - 1); }   // bits lo .. hi
// the full build of the Makefile and the registrars: wave kernels M = 1 .. 32, 32 lanes per system M = 4 .. 20, 16 lanes M = 4 .. 16
constexpr Built built_full() {
  const uint64_t w = m_range(1, kMaxM), p32 = m_range(4, 20), p16 = m_range(4, 16);
  return Built{w, w, w, w, w,
               m_range(IBS_ROWS_MIN_M, kMaxM), m_range(IBS_ROWS_MIN_M, kMaxM),
               m_range(IBS_DIRECT_MIN_M, kMaxM), m_range(IBS_DIRECT_MIN_M, kMaxM), m_range(IBS_F32LAM_DIRECT_MIN_M, kMaxM),
               {p32, p16}, {p32, p16}, {p32, p16}, {p32, p16}};
}

// ---------------------------------------------------------------- grid lengths
// long: the entry point has the generic long-grid path behind it (ibs_long.hip)
constexpr bool is_long(int N) { return N > 64 * kMaxM + 2; }
constexpr int rows_per_lane(int N) { return (N - 2 + 63) / 64; }
constexpr int grid_n_max(bool long_ok) { return long_ok ? kMaxLongN : 64 * kMaxM + 2; }
enum class GridCheck { Ok, Range, Even };     // Range: N outside [66, grid_n_max]; Even: the Simpson rule is restated for odd N only
constexpr GridCheck check_grid_length(int N, bool long_ok) {
  return (N < 66 || N > grid_n_max(long_ok)) ? GridCheck::Range : ((N & 1) == 0 ? GridCheck::Even : GridCheck::Ok);
}

// lanes per system.  64 = one wave per system (lowest latency, any N).  Large batches of short grids are
// throughput (VALU-issue) bound: 32 / 16 lanes per system amortise the scan over 2 / 4 systems per wave.
// option force_p = 64|32|16 overrides (tests).
inline int pick_lanes(const Chip& chip, const PlanOpts& opts, int N, long n_sys) {
  const int n = N - 2;
  const bool can32 = n <= 32 * 20 && n >= 32 * 3 + 1, can16 = n <= 16 * 16 && n >= 16 * 3 + 1;
  if (opts.force_p) {
    const int f = opts.force_p;
    if (f == 32 && can32) return 32;
    if (f == 16 && can16) return 16;
    return 64;
  }
  // Measured (tools/bench_lanes.py, r01_f): every iteration of the shift search is exactly one forward sweep, so
  // the systems sharing a wave stay in step (15 +- 2 iterations) and the cheaper sweeps pay off as soon as the
  // sub-wave launch still fills the chip: P = 32 from one wave per SIMD (N = 513: 2,048 systems 42 vs 50 us,
  // 65,536 systems 0.77 vs 1.00 ms), P = 16 (whose 16-row chunks make a lone wave twice as slow) from two
  // waves per SIMD (N = 257: 65,536 systems 0.38 vs 0.62 ms).  Smaller batches keep one wave per system.
  const long simds = 4L * chip.n_cu;
  if (can16 && n_sys / 4 >= 2 * simds) return 16;
  // (17..20 rows per lane, i.e. N up to the 641-point D3D grid: a lone wave is slower, pays off from 4 waves per SIMD:
  //  N = 641: 65,536 systems 0.82 vs 1.05 ms, 8,192 systems 147 vs 150 us, 2,048 systems 72 vs 52 us)
  const int m32 = (n + 31) / 32;
  if (can32 && n_sys / 2 >= (m32 > 16 ? 4 : 1) * simds) return 32;
  return 64;
}
constexpr int group_rows(int N, int P) { return (N - 2 + P - 1) / P; }       // rows per lane at P lanes per system

// Waves per block: as many as the LDS admits (`fit`), at most `cap`; then small batches are spread over all CUs (the solvers are
// issue-bound, one wave per SIMD is the fastest placement) instead of packed onto few.  0 = not even one wave fits.
inline int spread_wpb(long fit, int cap, long waves, int n_cu) {
  long wpb = fit < cap ? fit : cap;
  if (wpb < 1) return 0;
  long per_blk = waves / n_cu;
  if (per_blk < 1) per_blk = 1;
  return (int)(per_blk < wpb ? per_blk : wpb);
}
constexpr int ceil_div(int a, int b) { return (a + b - 1) / b; }
// `n` waves of a line in blocks of at most `w`: the block size that balances them over the same number of blocks
constexpr int balanced(int n, int w) { return ceil_div(n, ceil_div(n, w)); }

// ---------------------------------------------------------------- geometry-fed scans
enum class ScanForm { Wave, WaveLean, WaveChain, Group, GroupChain, Long };
enum class PlanError { None, NotBuilt, NoLds };      // (the messages are the API's)
struct ScanPlan {
  ScanForm form; PlanError err;
  int P, M;                 // lanes per system, rows per lane of the kernel (err != None: of the one-wave kernel, for the message)
  int wpb, chain;           // waves per block; theta0 values per wave / group position (0 = not a chained form)
  int resident;             // form Wave, scan_resident_built(M): the resident k_gamma_scan (otherwise form WaveLean)
  bool fused_pack;          // the per-surface argmax runs in the scan kernel's epilogue (Wave, WaveLean), in pack_mode
  int pack_mode;
};

// LDS rows (of lds_pitch(N) elements) of a scan block: the staged line's seven arrays, and one row per system of the block that the
// eigenfunction stage works in -- which the chained kernels need only when X / dX are written (need_x)
constexpr int kScanLineRows = 7;
constexpr int scan_lds_rows(int wpb, int G = 1, bool need_x = true) { return kScanLineRows + (need_x ? wpb * G : 0); }
// ... and the most waves per block the LDS admits under it
inline long scan_lds_waves(const Chip& chip, int N, int G) {
  const size_t row = (size_t)lds_pitch(N) * sizeof(double);
  return (long)(((size_t)chip.lds_per_block - kScanLineRows * row) / (row * G));
}
// k_gamma_scan_chain: the LDS-round-trip finish of M < 3 always uses the row
constexpr bool scan_chain_need_x(int M, bool want_x) { return M < 3 || want_x; }

// Batches much larger than the chip (no caller-supplied guesses): chain consecutive theta0 values of a line through one wave or
// group position, each solve warm-started from the previous eigenvalue (k_gamma_scan_chain, k_gamma_scan_g_chain).  `slots` =
// theta0 values per wave position of a line, `min2` = the fewest slots chained by 2 (twice that: by 4), `rows` = rows per lane, `cap`
// = waves per block of the kernel.  4 per wave once that still leaves two waves per SIMD, 2 from there down to two waves of chained
// work per SIMD (tools/bench_chain_sizes.py; N = 1025: 2,048 solves 70 vs 95 us, 4,096: 111 vs 105 us).  option scan_chain = n overrides.
inline int chain_length(const Chip& chip, const PlanOpts& opts, int N, long n_lines, int slots, int min2, int rows, int cap) {
  const long waves = n_lines * slots, simds = 4L * chip.n_cu;
  int chain = 1;
  if (slots >= 2 * min2 && waves >= 8 * simds) chain = 4;
  else if (slots >= min2 && waves >= 4 * simds) chain = 2;
  // A chain shortens the blocks (a line's waves = theta0 slots / chain) while every block still stages the whole line:
  // the LDS then limits the waves per CU.  Shorten the chain until the blocks that fit a CU hold as many waves as the
  // registers allow (tools/batch_sweep.py, 8 theta0 per line, N = 513, 65,536 solves: chain 4 = one wave per block =
  // 4 waves per CU: 6.5e7 solves/s; chain 2: 1.0e8).
  const int occ = rows <= 4 ? 4 : (rows <= 8 ? 3 : (rows <= 16 ? 2 : 1));        // waves per SIMD the VGPRs allow
  const long blocks_per_cu = (long)((size_t)chip.lds_per_block / (scan_lds_rows(0) * (size_t)lds_pitch(N) * sizeof(double)));
  while (chain > 1) {
    long w = ceil_div(slots, chain);
    if (w > cap) w = cap;
    if (blocks_per_cu * w >= 4L * occ) break;
    chain >>= 1;
  }
  if (opts.scan_chain >= 1 && opts.scan_chain <= slots) chain = opts.scan_chain;
  return chain;
}
// waves per block of a chained launch: what the LDS admits when the eigenfunction rows are needed, the kernel's cap otherwise,
// balanced over the blocks of a line.  (At least 1: plan_scan has checked that one wave of the unchained form fits.)
inline int chain_wpb(const Chip& chip, int N, int G, int slots, int chain, int cap, bool need_x) {
  const int wpl = ceil_div(slots, chain);          // waves per line
  long w = need_x ? scan_lds_waves(chip, N, G) : cap;
  if (w > cap) w = cap;
  if (w > wpl) w = wpl;
  return balanced(wpl, (int)w);
}

// warm: caller-supplied guesses (ibs_gamma_scan_warm_f64); want_x: X or dX is written; t0_per_line: n_theta0 = 1 and one theta0 per
// line (ibs_gamma_points_f64), one wave per system; want_pack: the per-surface argmax is wanted (ibs_gamma_scan_argmax_f64)
inline ScanPlan plan_scan(const Chip& chip, const PlanOpts& opts, const Built& built, int n_lines, int n_theta0, int N, bool warm,
                          bool want_x, bool t0_per_line, bool want_pack) {
  ScanPlan p{ScanForm::Wave, PlanError::None, 64, 1, 1, 0, 0, false, 0};
  const bool lng = is_long(N);                 // grids beyond 2050 points: launch_scan_long
  p.M = lng ? 1 : rows_per_lane(N);
  if (!has(built.scan, p.M)) { p.err = PlanError::NotBuilt; return p; }     // (on long grids only a check that the build is complete)
  if (lng) { p.form = ScanForm::Long; return p; }
  if ((size_t)(kScanLineRows + 1) * lds_pitch(N) * sizeof(double) > (size_t)chip.lds_per_block) { p.err = PlanError::NoLds; return p; }
  int G = 1, cap = scan_max_threads(p.M) / 64;
  bool g_chain = false;                        // the chained / warm-started sub-wave kernel of the same (P, M) is built
  const int P = t0_per_line ? 64 : pick_lanes(chip, opts, N, (long)n_lines * n_theta0);
  if (P != 64 && n_theta0 % (64 / P) == 0) {
    const int Mg = group_rows(N, P), pi = P == 32 ? 0 : 1;
    g_chain = has(built.scan_chain_g[pi], Mg);
    if (has(built.scan_g[pi], Mg) && (g_chain || !warm)) {
      p.form = ScanForm::Group; p.P = P; p.M = Mg; G = 64 / P; cap = scan_max_threads_g(Mg) / 64;
    }
  }
  // wpb = waves per block; each wave solves G theta0 values of the block's line
  const int waves_per_line = ceil_div(n_theta0, G);
  p.wpb = spread_wpb(scan_lds_waves(chip, N, G), cap < waves_per_line ? cap : waves_per_line, (long)n_lines * waves_per_line, chip.n_cu);
  if (p.wpb < 1) { p.err = PlanError::NoLds; p.M = rows_per_lane(N); return p; }
  p.wpb = balanced(waves_per_line, p.wpb);
  if (G > 1 && g_chain) {
    // sub-wave kernels: the chain over the theta0 slots of a group position; caller-supplied guesses go through the same
    // kernel with a chain of one
    const int slots = n_theta0 / G;
    const int chain = warm ? 1 : chain_length(chip, opts, N, n_lines, slots, 2, p.M, cap);
    if (chain > 1 || warm) { p.form = ScanForm::GroupChain; p.chain = chain; p.wpb = chain_wpb(chip, N, G, slots, chain, cap, want_x); }
  } else if (G == 1 && !warm && !t0_per_line) {
    const int chain = chain_length(chip, opts, N, n_lines, n_theta0, 4, p.M, cap);
    if (chain > 1 && has(built.scan_chain, p.M)) {
      p.form = ScanForm::WaveChain; p.chain = chain;
      p.wpb = chain_wpb(chip, N, 1, n_theta0, chain, cap, scan_chain_need_x(p.M, want_x));
    }
  }
  if (p.form != ScanForm::Wave) return p;
  // One wave per system, unchained, 3 <= M <= 8: the resident form of k_gamma_scan (186 VGPRs at M = 8: two waves per SIMD) while the
  // launch holds no more than that -- its time is then a lone wave's latency --, k_gamma_scan_lean (four at M = 8) above.
  const long nblocks = (long)ceil_div(n_theta0, p.wpb) * n_lines;
  if (scan_resident_built(p.M)) {
    p.resident = opts.scan_resident == 0 ? 0 : (opts.scan_resident == 1 ? 1 : (nblocks * p.wpb <= 2L * 4 * chip.n_cu ? 1 : 0));
    if (!p.resident) p.form = ScanForm::WaveLean;
  }
  // one launch: the block that completes a surface reduces it (k_gamma_scan's epilogue)
  p.fused_pack = want_pack;
  if (want_pack) p.pack_mode = opts.pack_mode == 1 ? 1 : ((nblocks <= chip.n_cu && opts.pack_mode != 2) ? 1 : 2);
  return p;
}

// ---------------------------------------------------------------- gam maximised over theta0 (k_theta0_polish)
// One block per line on a plain 1-D grid, one wave per start slot.  LDS rows: the staged line's seven arrays, and a row per wave only
// where the growth-rate stage goes through LDS (M < 3: finish()); the search states and the gam words are static (< 1 KB).
constexpr int kTheta0PolishMaxStarts = 4;
constexpr int theta0_polish_lds_rows(int M, int n_starts) { return kScanLineRows + (M < 3 ? n_starts : 0); }
struct Theta0PolishPlan { PlanError err; int M, threads, lds_rows; };
inline Theta0PolishPlan plan_theta0_polish(const Chip& chip, const Built& built, int N, int n_starts) {
  Theta0PolishPlan p{PlanError::None, rows_per_lane(N), 64 * n_starts, 0};
  p.lds_rows = theta0_polish_lds_rows(p.M, n_starts);
  if (!has(built.scan_chain, p.M)) p.err = PlanError::NotBuilt;      // (registered beside k_gamma_scan_chain, for every M)
  else if ((size_t)p.lds_rows * lds_pitch(N) * sizeof(double) + 1024 > (size_t)chip.lds_per_block) p.err = PlanError::NoLds;
  return p;
}

// ---------------------------------------------------------------- raw (g, c, f) solves
enum class GcfForm {
  Staged,          // k_solve_gcf<double, M>: one wave per system, the three rows staged in LDS
  Rows,            // k_solve_gcf_rows: the rows streamed through one LDS row per wave (long grids)
  Direct,          // k_solve_gcf_direct: the rows read straight from global memory
  F32,             // k_solve_gcf<float, M>: the all-FP32 iteration + FP64 certificate, staged likewise
  F32Wide,         // k_solve_gcf_wide: FP32 in HBM, widened as read, the FP64 solver
  F32WideRows, F32WideDirect,
  F32LamDirect,    // k_solve_gcf_f32lam_direct: eigenvalues only, all-FP32 iteration + FP64 certificate, rows from global memory
  Group,           // k_solve_gcf_g: P = 32 / 16 lanes per system
  GroupWide,       // ... on FP32 arrays
  Long             // launch_gcf_long: N > 2050
};
struct GcfPlan {
  GcfForm form; PlanError err;
  int P, M, wpb;            // (err != None: M of the one-wave kernel, for the message)
  size_t per_wave;          // bytes of LDS per wave
  bool lists_suspects;      // the big-batch forms only LIST their suspect systems; k_fix_gcf re-closes them afterwards
  bool direct_form;         // stages nothing: LDS only for the row X / dX are written from
};

// One wave per system on a long grid: k_solve_gcf's three staged rows are 24.6 KB of LDS per wave at N = 1025 -- five waves
// per CU where the registers admit eight.  A batch that fills the chip at more waves than the staging admits reads its rows
// straight from global memory instead (k_solve_gcf_direct: no LDS).  Option gcf_direct: -1 = this rule, 0 = never, 1 = always.
inline bool use_direct(const Chip& chip, const PlanOpts& opts, int N, long n_sys) {
  if (opts.gcf_direct == 0) return false;
  if (opts.gcf_direct == 1) return true;
  // (measured, tools/bench_direct.py, 2^19 systems: 1.45-1.65 x the staged / row-streamed kernels at N_zeta = 768 .. 1536, 1.2-1.3 x at 2048)
  const long staged_waves_per_cu = (long)(chip.lds_per_block / ((size_t)3 * lds_pitch(N) * sizeof(double)));
  return staged_waves_per_cu < 8 && n_sys > (staged_waves_per_cu > 4 ? staged_waves_per_cu : 4) * chip.n_cu;
}

// elem_bytes: 8 = ibs_solve_gcf(h)_f64, 4 = ibs_solve_gcf_f32; has_gh: a caller-supplied half-grid g (one wave per system, staged)
inline GcfPlan plan_gcf(const Chip& chip, const PlanOpts& opts, const Built& built, int elem_bytes, long n_sys, int N, bool has_gh,
                        bool want_gam, bool want_x) {
  const bool lng = is_long(N), f64 = elem_bytes == 8;
  GcfPlan p{f64 ? GcfForm::Staged : GcfForm::F32, PlanError::None, 64, 1, 0, 0, false, false};
  const int M = lng ? 1 : rows_per_lane(N);
  p.M = M;
  if (!has(f64 ? built.gcf_f64 : built.gcf_f32, M)) { p.err = PlanError::NotBuilt; return p; }
  const size_t row = (size_t)lds_pitch(lng ? 66 : N);
  p.per_wave = 3 * row * elem_bytes;
  auto group = [&](GcfForm form, const uint64_t (&masks)[2], int P) {       // the sub-wave form, where built
    const int Mg = group_rows(N, P);
    if (!has(masks[P == 32 ? 0 : 1], Mg)) return;
    p.form = form; p.P = P; p.M = Mg; p.per_wave = (size_t)(64 / P) * row * sizeof(double);
  };
  if (lng) {
    // grids beyond 2050 points: the generic division-form path (ibs_long.hip), FP64 arithmetic on either element type
    p.form = GcfForm::Long;
  } else if (f64) {
    const int P = has_gh ? 64 : pick_lanes(chip, opts, N, n_sys);
    if (P != 64) group(GcfForm::Group, built.gcf_g, P);
    if (p.form == GcfForm::Staged && !has_gh) {
      // long grids, one wave per system: stream the three rows through ONE LDS row per wave (k_solve_gcf_rows) -- the
      // 3-row staging of k_solve_gcf leaves two waves per CU at N_zeta = 2048 and five at 1024
      if (has(built.gcf_rows, M) && opts.gcf_rows != 0) p.form = GcfForm::Rows;
      if (has(built.gcf_direct, M) && use_direct(chip, opts, N, n_sys)) p.form = GcfForm::Direct;
      if (p.form != GcfForm::Staged) p.per_wave = row * sizeof(double);
    }
  } else {
    // FP32 systems whose growth rate or eigenfunction is wanted: FP32 in HBM, widened to FP64 as they are read, solved by the
    // FP64 solver -- in the same three forms as the FP64 entry point (sub-wave for large batches of short grids, row-streamed
    // for long grids, else one wave per system with the three rows staged).  lam alone stays with the all-FP32 kernel, whose
    // result is certified by an FP64 count pair (k_solve_gcf<float, M>).
    // lam alone: the all-FP32 iteration with its FP64 certificate.  A batch that would get the 32-lane sub-wave form takes it with
    // the rows read straight from global memory (k_solve_gcf_f32lam_direct: 1.12-1.15 x the FP64 sub-wave solver on FP32 bytes on
    // smooth coefficients, 2.1 x on rough ones; 2,048 ... 10^6 systems, N_zeta = 256 ... 640, tools/bench_forms.py).  Where the
    // 16-lane form runs (N <= 258, big batches) the FP64 sub-wave solver without its growth-rate stage stays: 1.5 x the all-FP32
    // form on smooth coefficients, 0.83 x on rough ones.  Also where the direct form is not built or gcf_direct = 0; option
    // f32_lam overrides.
    const int P = pick_lanes(chip, opts, N, n_sys);
    const bool fl_ok = has(built.gcf_f32lam_direct, M) && opts.gcf_direct != 0;
    const bool wide_lam = opts.f32_lam == 2 || (opts.f32_lam == 0 && (P == 16 || (P == 32 && !fl_ok)));
    if (want_gam || want_x || wide_lam) {
      if (has(built.gcf_f32_wide, M)) { p.form = GcfForm::F32Wide; p.per_wave = 3 * row * sizeof(double); }
      if (P != 64) group(GcfForm::GroupWide, built.gcf_f32w_g, P);
      else {
        const GcfForm one_wave = p.form;
        if (has(built.gcf_f32w_rows, M) && opts.gcf_rows != 0) p.form = GcfForm::F32WideRows;
        if (has(built.gcf_f32w_direct, M) && use_direct(chip, opts, N, n_sys)) p.form = GcfForm::F32WideDirect;
        if (p.form != one_wave) p.per_wave = row * sizeof(double);
      }
    } else if (!has_gh && fl_ok && (P != 64 || use_direct(chip, opts, N, n_sys))) {
      // eigenvalues only, all-FP32 iteration + FP64 certificate: big batches read their rows from global memory
      p.form = GcfForm::F32LamDirect;
    }
  }
  // the direct forms stage nothing: four waves per block, LDS only for the row X / dX are written from (ibs_kernels.hip: launch_gcf_direct,
  // launch_gcf_f32lam_direct take the block shape from the wpb argument)
  p.direct_form = p.form == GcfForm::Direct || p.form == GcfForm::F32WideDirect || p.form == GcfForm::F32LamDirect;
  p.lists_suspects = p.form == GcfForm::Direct || p.form == GcfForm::F32WideDirect || p.form == GcfForm::Group || p.form == GcfForm::GroupWide;
  if (p.direct_form) p.per_wave = want_x ? row * sizeof(double) : 0;
  int wpb = p.per_wave ? (int)((size_t)chip.lds_per_block / p.per_wave) : kGcfMaxWaves;
  if (wpb > kGcfMaxWaves) wpb = kGcfMaxWaves;
  // keep >= 3 blocks per CU resident when LDS allows it
  while (!p.direct_form && wpb > 1 && (size_t)wpb * p.per_wave * 3 > (size_t)chip.lds_per_block) --wpb;
  p.wpb = wpb;
  if (wpb < 1) { p.err = PlanError::NoLds; p.M = M; }
  return p;
}

// ---------------------------------------------------------------- Sturm count, objective
// forms: 1 = the prefix-product sweep (one wave per system, N <= 2050: the bandwidth kernel of rounds 1-5), and two division-form
// kernels for any N (ibs_long.hip): 2 = lanes as systems (batches), 3 = one wave per system (a handful of systems on a long grid).
// By size: the sweep up to 2,050 points -- except where its lanes sit 128 / 256 bytes apart (16 / 32 rows per lane: 4.2 / 2.8 TB/s
// against 6.3 at 8, 12, 24 rows) and the batch fills the chip with 64 systems per wave: there the division form is exact AND faster
// (4.9-5.1 TB/s; tools/experiments/sturm_crossover.py)
struct SturmPlan { int form, M, wpb; size_t per_wave; };       // wpb = 0: one wave's row (per_wave bytes) does not fit the LDS
inline SturmPlan plan_sturm(const Chip& chip, const PlanOpts& opts, long n_sys, int N) {
  int form = opts.sturm_form;
  if (form == 0) {
    if (is_long(N)) form = n_sys >= 64 ? 2 : 3;
    else {
      const int Mr = rows_per_lane(N);
      form = ((Mr == 16 && n_sys >= 65536) || (Mr == 32 && n_sys >= 32768)) ? 2 : 1;
    }
  }
  if (form == 1 && is_long(N)) form = 2;
  SturmPlan p{form, form != 1 ? 1 : rows_per_lane(N), 1, (size_t)N * sizeof(double)};
  if (form == 1) p.wpb = (int)((size_t)chip.lds_per_block / p.per_wave);
  if (p.wpb > kGcfMaxWaves) p.wpb = kGcfMaxWaves;
  return p;
}

// k_obj_w_grad: waves per block (one point per wave, eight staged rows each); 0 = one point does not fit the LDS
inline int plan_grad_wpb(const Chip& chip, int n_pts, int N) {
  const size_t per_wave = (size_t)8 * lds_pitch(is_long(N) ? 66 : N) * sizeof(double);
  return spread_wpb((long)((size_t)chip.lds_per_block / per_wave), kGcfMaxWaves, n_pts, chip.n_cu);
}

// ---------------------------------------------------------------- whole-line chunks under one workspace budget
inline size_t pad256(size_t b) { return (b + 255) & ~size_t(255); }
// Device buffers carved out of one workspace, sized by the very sequence of take() calls that carves them: a first pass without a
// buffer only counts (Carve{nullptr}), the second carves.
struct Carve {
  char* base; size_t off = 0;
  template <typename T> T* take(size_t n) {
    off = pad256(off);
    T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
    off += n * sizeof(T);
    return p;
  }
};

// The geometry-fed scans that keep per-system rows in a workspace (nearest, modes, the scan VJP, the non-uniform-grid scans) work
// through their lines in chunks of whole lines: a chunk's workspace (rows + the solver's per-wave workspace) stays within this many
// bytes, or the chunk holds option "nearest_chunk_systems" systems.
constexpr size_t kLineChunkBudget = size_t(1) << 30;
struct LineChunks { long lines; size_t bytes; };      // lines per chunk (the last chunk may be shorter), bytes_of(lines)
// bytes_of(L) = the workspace of a chunk of L lines.  chunk_systems > 0 (the option): that many systems, rounded down to whole lines.
// Otherwise n_lines is halved, rounding up, while it is over the budget: NOT the largest count that fits (7 lines of which 3 would fit
// go 4, 2).  Launch shapes follow from this sequence.  One line over the budget stays one line: the caller tries the allocation.
template <class BytesOf>
LineChunks plan_line_chunks(long n_lines, int n_theta0, long chunk_systems, size_t budget, BytesOf&& bytes_of) {
  long L = n_lines;
  if (chunk_systems > 0) L = chunk_systems / n_theta0;
  else while (L > 1 && bytes_of(L) > budget) L = (L + 1) / 2;
  if (L < 1) L = 1;
  if (L > n_lines) L = n_lines;
  return LineChunks{L, bytes_of(L)};
}

}  // namespace ibs
