// Grids beyond the register-resident kernels (N > 64 * kMaxM + 2 = 2050 points, up to kMaxLongN): the generic path that keeps the
// drop-in from refusing what the reference computes -- utils.py:1556-1624 accepts any length, and the reference's own grid rule
// N = 2 mpol ntor 4 + 1 (ball_scan.py:201-208) passes 2050 from mpol ntor > 256 on.
//
// One wavefront per system, everything in DIVISION form on the original rows (no scaled rows, nothing register-resident):
//   1. bounds        lam_max <= max c/f (Gershgorin), lam_max >= max d/f (unit vectors) and >= the Rayleigh
//                    quotients of four trial vectors sin^p(pi j / (N - 1)) taken in the same pass, ||A||; data checks
//   2. eigenvalue    64-way multisection on division-form Sturm counts (ibs_wave.hpp: multisect; the recurrence of SURVEY Appendix A /
//                    LAPACK dstebz, the rows passed through LDS in chunks: count_above_chunked) to a bracket of 2 eps ||A||: first on
//                    every 16th and every 8th grid point (two-grid start), then 3-5 passes on all rows (9 from the Gershgorin bracket alone)
//   3. eigenvector   twisted factorisation N_k D_k N_k^T of T - lam F (the getvec step of MRRR): forward pivots D+ (lane 0) and
//                    backward pivots D- (lane 1) in one serial pass, gamma_r = D+_r + D-_r - (d_r - lam f_r) in parallel, twist row
//                    k = argmin |gamma_r|, then z_k = 1, z_{r-1} = -e_r z_r / D+_{r-1} downwards (lane 0) and
//                    z_{r+1} = -e_{r+1} z_r / D-_{r+1} upwards (lane 1)
//   4. growth rate   X = z / max |z| with zero end points, FD2/FD4 derivative, composite Simpson quotient: the arithmetic of
//                    finish() in ibs_kernels.hip, i.e. utils.py:1601-1621
// Per-wave workspace in global memory: 3 N doubles (D+, D-, d - lam f; the last becomes z).  The grid is persistent: a fixed
// number of waves, each taking systems blockIdx.x, blockIdx.x + gridDim.x, ...  The device pieces of stages 1-4 live in ibs_long.hpp,
// shared with the nearest-sigma kernel (ibs_nearest.hip).
#include "ibs_long.hpp"
#include "ibs_geo_line.hpp"
#include "ibs_launch.hpp"

namespace ibs {

template <typename TI, bool HAS_GH>
__device__ __forceinline__ void solve_long_one(const SrcLong<TI, HAS_GH>& src, int N, double h, long sys, double* work, TI* lam_out,
                                               TI* gam_out, TI* X_out, TI* dX_out, int* info_out, double* lds) {
  const int lane = threadIdx.x & 63;
  const double ih2 = 1.0 / (h * h);
  // ---- 1. bounds and data checks (ibs_long.hpp: long_bounds)
  const LongBounds b = long_bounds<false>(src, N, ih2, lane);
  int status = 0, passes = 0;
  double lam = 0.0;
  const bool want_vec = gam_out || X_out || dX_out;        // (kernel-uniform)
  if (b.bad) {
    status = 2;
    lam = __builtin_nan("");
  } else if (!long_lam_max(src, N, ih2, b.lo, b.hi, b.normA, lds, lane, lam, passes)) {      // ---- 2. eigenvalue (long_lam_max)
    status = 1;
  }
  double gam = __builtin_nan("");
  if (want_vec && status == 0) gam = long_vector_growth<false, TI>(src, N, h, lam, sys, work, X_out, dX_out, lds, lane);   // ---- 3-4.
  if (lane == 0) {
    if (lam_out) lam_out[sys] = (TI)lam;
    if (gam_out) gam_out[sys] = (TI)gam;
    if (info_out) info_out[sys] = passes | (status << 16);
  }
}

template <typename TI>
__global__ void __launch_bounds__(64) k_solve_gcf_long(long n_sys, int N, double h, const TI* __restrict__ g, const TI* __restrict__ c,
                                                       const TI* __restrict__ f, const TI* __restrict__ gh, long ld, TI* lam_out,
                                                       TI* gam_out, TI* X_out, TI* dX_out, int* info_out, double* work) {
  __shared__ double lds[3 * kLongChunk];
  double* my = work + (size_t)blockIdx.x * 3 * (size_t)N;
  for (long sys = blockIdx.x; sys < n_sys; sys += gridDim.x) {
    if (gh) {
      const SrcLong<TI, true> src{g + sys * ld, c + sys * ld, f + sys * ld, gh + sys * ld};
      solve_long_one<TI, true>(src, N, h, sys, my, lam_out, gam_out, X_out, dX_out, info_out, lds);
    } else {
      const SrcLong<TI, false> src{g + sys * ld, c + sys * ld, f + sys * ld, nullptr};
      solve_long_one<TI, false>(src, N, h, sys, my, lam_out, gam_out, X_out, dX_out, info_out, lds);
    }
    long_fence();                                           // (the workspace is reused by this wave's next system)
  }
}

// eigenvalues of (T, F) above shift[sys]: one wave per system, every lane the same shift (division form: exact for a pencil a few
// ulp away, whatever N).  Replaces check_ball's verdict (bishop_ball_s-alpha.py:20-115) on grids beyond 2050 points.
__global__ void __launch_bounds__(64) k_sturm_count_long(long n_sys, int N, double h, const double* __restrict__ g,
                                                         const double* __restrict__ c, const double* __restrict__ f, long ld,
                                                         const double* __restrict__ shift, int* count_out) {
  __shared__ double lds[3 * kLongChunk];
  const double ih2 = 1.0 / (h * h);
  for (long sys = blockIdx.x; sys < n_sys; sys += gridDim.x) {
    const SrcLong<double, false> src{g + sys * ld, c + sys * ld, f + sys * ld, nullptr};
    const int cnt = count_above_chunked(src, N - 2, ih2, shift[sys], lds, (int)(threadIdx.x & 63));
    if ((threadIdx.x & 63) == 0) count_out[sys] = cnt;
  }
}

// Division-form Sturm count with LANES AS SYSTEMS (round 6): every lane walks its own system's rows serially -- q_r = (d_r - sig f_r) -
// e_r^2 / q_{r-1}, IEEE division, pivmin guard: exact for a pencil a few ulp away, any N (the prefix-product sweep k_sturm_count is
// exact only for ~N eps ||A||, ~N^2 eps ||A|| on iid-random coefficients) -- while the rows reach it through an LDS transpose: per chunk
// the wave loads, for 64 systems, ONE 128-byte line of g, c and f per system (four systems per load instruction), writes them to LDS as
// [system][point] and reads them back one system per lane.  The next chunk's 48 loads are in flight while the current one is worked on.
// Rows of N doubles start at any multiple of 8 bytes: a chunk of 16 grid points at the same j in every system straddled two lines per
// system and array, and the second half was gone from the L2 by the time the next chunk asked for it (PMC: 1.82 x the algorithmic bytes).
// So every system is walked from ITS OWN line boundary: lane s runs a_s = (its row's first element) mod 16 points behind the chunk index
// -- the systems are independent, nothing needs them at the same grid point at the same time -- and a row is eliminated one step late,
// when g of the next point has arrived (c and f of the row wait one step in registers).  Steps before point 1 / after point N - 2 of a
// lane are masked.
constexpr int kDivChunk = 16, kDivPitch = kDivChunk + 1, kDivWaves = 2;      // (2 waves per block: 52 KB of LDS, three blocks per CU)
__global__ void __launch_bounds__(64 * kDivWaves) k_sturm_count_div(long n_sys, int N, double h, const double* __restrict__ g,
                                                         const double* __restrict__ c, const double* __restrict__ f, long ld,
                                                         const double* __restrict__ shift, int* count_out) {
  constexpr double pivmin = 2.2250738585072014e-292;
  __shared__ double tile[kDivWaves][3][kWave * kDivPitch];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long base = ((long)blockIdx.x * kDivWaves + wave) * kWave;    // first system of this wave
  if (base >= n_sys) return;                                           // (wave-uniform; no block-level barrier below)
  const int sub = lane >> 4, rr = lane & 15;                           // loader role: system 4 k + sub, element rr of its line
  const long mine = base + lane < n_sys ? base + lane : n_sys - 1;     // worker role: this lane's system
  const double sig = shift[mine];
  const double ih2 = 1.0 / (h * h);
  auto phase = [&](long sy) { return (int)((reinterpret_cast<unsigned long long>(g + sy * ld) >> 3) & 15ull); };   // in doubles, of g's row
  double* tg = tile[wave][0]; double* tc = tile[wave][1]; double* tf = tile[wave][2];
  double vg[16], vc[16], vf[16];
  auto load_chunk = [&](int B) {                                       // system sy: grid points 16 B - a_sy + (0 .. 15), clamped into the row
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      long sy = base + 4 * k + sub; sy = sy < n_sys ? sy : n_sys - 1;
      int pnt = 16 * B - phase(sy) + rr;
      pnt = pnt < 0 ? 0 : (pnt > N - 1 ? N - 1 : pnt);
      const long o = sy * ld + pnt;
      vg[k] = g[o]; vc[k] = c[o]; vf[k] = f[o];
    }
  };
  const int a_m = phase(mine);
  double gm2 = 0.0, gm1 = 0.0, cprev = 0.0, fprev = 1.0, q = 1.0;
  int cnt = 0;
  const int nB = (N - 1 + 15) / 16 + 1;                                // chunks until every lane has seen its point N - 1
  load_chunk(0);
  for (int B = 0; B < nB; ++B) {
    wave_lds_sync();                                                   // (the previous chunk has been consumed)
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const int o = (4 * k + sub) * kDivPitch + rr;
      tg[o] = vg[k]; tc[o] = vc[k]; tf[o] = vf[k];
    }
    wave_lds_sync();
    if (B + 1 < nB) load_chunk(B + 1);                                 // in flight during the recurrence below
    const int p0 = 16 * B - a_m;                                       // this lane's grid point at i = 0
#pragma unroll 4
    for (int i = 0; i < kDivChunk; ++i) {
      const double gp = tg[lane * kDivPitch + i], cp = tc[lane * kDivPitch + i], fp = tf[lane * kDivPitch + i];
      const int j = p0 + i - 1;                                        // the row that can be eliminated now: g[j + 1] has arrived
      const double e_lo = 0.5 * (gm2 + gm1) * ih2, e_hi = 0.5 * (gm1 + gp) * ih2;      // utils.py:1574-1576
      const double a = xfma(-sig, fprev, cprev - (e_lo + e_hi));                       // utils.py:1584-1592
      double qn = (j == 1) ? a : a - (e_lo * e_lo) / q;
      qn = xabs(qn) < pivmin ? -pivmin : qn;
      const bool row = j >= 1 && j <= N - 2;
      q = row ? qn : q;
      cnt += (row && qn > 0.0) ? 1 : 0;
      gm2 = gm1; gm1 = gp; cprev = cp; fprev = fp;
    }
  }
  if (base + lane < n_sys) count_out[base + lane] = cnt;
}

// (g, c, f) of every (line, theta0) system of a geometry-fed scan, and their theta0 tangents, written out as rows: the long-grid
// form of the staging the scan kernels do in LDS -- the same expressions in the same order (k_gamma_scan, SrcGeo), i.e.
// ball_scan.py:267-268 + utils.py:1560-1562 and utils.py:1669-1673.
__global__ void __launch_bounds__(256) k_assemble_gcf_long(int n_lines, int n_theta0, int N, const double* __restrict__ bmag,
                                                           const double* __restrict__ gradpar, const double* __restrict__ cvdrift,
                                                           const double* __restrict__ cvdrift0, const double* __restrict__ gds2,
                                                           const double* __restrict__ gds21, const double* __restrict__ gds22, long ld,
                                                           const double* __restrict__ dPdrho, const double* __restrict__ theta0,
                                                           int t0_stride, double* g, double* c, double* f, double* gt, double* ct,
                                                           double* ft) {
  const long n_sys = (long)n_lines * n_theta0;
  for (long sys = blockIdx.y; sys < n_sys; sys += gridDim.y) {
    const int line = (int)(sys / n_theta0), it0 = (int)(sys - (long)line * n_theta0);
    const double th0 = theta0[(long)line * t0_stride + it0];
    const double mdP = -dPdrho[line];
    const GeoLine7 ln{{bmag, gradpar, cvdrift, cvdrift0, gds2, gds21, gds22}, (long)line * ld};
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < N; j += gridDim.x * blockDim.x) {
      const long o = sys * N + j;
      double gj, cj, fj, gtj, ctj, ftj;                     // (all loads before the first store: the outputs are not __restrict__)
      line_gcf(ln, j, mdP, th0, gj, cj, fj);
      line_gcf_dtheta0(ln, j, mdP, th0, gtj, ctj, ftj);
      g[o] = gj; c[o] = cj; f[o] = fj;
      if (gt) { gt[o] = gtj; ct[o] = ctj; ft[o] = ftj; }
    }
  }
}

hipError_t launch_gcf_long(const LongGcfArgs& a, hipStream_t st) {
  const unsigned grid = (unsigned)(a.n_sys < a.n_waves ? a.n_sys : a.n_waves);
  if (a.f32) {
    hipLaunchKernelGGL(k_solve_gcf_long<float>, dim3(grid), dim3(64), 0, st, a.n_sys, a.N, a.h, (const float*)a.g, (const float*)a.c,
                       (const float*)a.f, (const float*)a.gh, a.ld, (float*)a.lam, (float*)a.gam, (float*)a.X, (float*)a.dX, a.info, a.work);
    note_launch(grid, 64, "ibs::k_solve_gcf_long<float>");
  } else {
    hipLaunchKernelGGL(k_solve_gcf_long<double>, dim3(grid), dim3(64), 0, st, a.n_sys, a.N, a.h, (const double*)a.g, (const double*)a.c,
                       (const double*)a.f, (const double*)a.gh, a.ld, (double*)a.lam, (double*)a.gam, (double*)a.X, (double*)a.dX, a.info,
                       a.work);
    note_launch(grid, 64, "ibs::k_solve_gcf_long<double>");
  }
  return hipGetLastError();
}

hipError_t launch_sturm_long(const SturmArgs<double>& a, hipStream_t st) {
  const long cap = 16384;
  const unsigned grid = (unsigned)(a.n_sys < cap ? a.n_sys : cap);
  hipLaunchKernelGGL(k_sturm_count_long, dim3(grid), dim3(64), 0, st, a.n_sys, a.N, a.h, a.g, a.c, a.f, a.ld, a.shift, a.count);
  note_launch(grid, 64, "ibs::k_sturm_count_long");
  return hipGetLastError();
}

hipError_t launch_sturm_div(const SturmArgs<double>& a, hipStream_t st) {
  const long per = 64 * kDivWaves, nblk = (a.n_sys + per - 1) / per;
  hipLaunchKernelGGL(k_sturm_count_div, dim3((unsigned)nblk), dim3((unsigned)per), 0, st, a.n_sys, a.N, a.h, a.g, a.c, a.f, a.ld, a.shift, a.count);
  note_launch(nblk, (int)per, "ibs::k_sturm_count_div");
  return hipGetLastError();
}

hipError_t launch_assemble_long(const ScanArgs<double>& a, double* g, double* c, double* f, double* gt, double* ct, double* ft,
                                hipStream_t st) {
  const long n_sys = (long)a.n_lines * a.n_theta0;
  int bx = (a.N + 255) / 256;
  if (bx > 64) bx = 64;
  hipLaunchKernelGGL(k_assemble_gcf_long, dim3((unsigned)bx, (unsigned)(n_sys < 32768 ? n_sys : 32768)), dim3(256), 0, st, a.n_lines, a.n_theta0, a.N, a.bmag,
                     a.gradpar, a.cvdrift, a.cvdrift0, a.gds2, a.gds21, a.gds22, a.ld, a.dPdrho, a.theta0, a.t0_stride, g, c, f, gt, ct, ft);
  return hipGetLastError();
}

}  // namespace ibs
