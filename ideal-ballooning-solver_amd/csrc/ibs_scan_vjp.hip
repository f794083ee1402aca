// Vector-Jacobian product of a whole (line, theta0) table of growth rates, FP64, every odd N in [66, 65,537]: a cotangent
// gam_bar[n_lines][n_theta0] becomes cotangent planes of the seven geometry arrays, of dPdrho and of theta0, without the (g, c, f) rows
// of the systems ever leaving the device code.  gam is the FD4 / Simpson quotient the call returns (utils.py:1601-1621) and the
// derivative is exact for it (ibs_vjp.hpp).  Nothing upstream corresponds.  Two launches per chunk of whole lines:
//
// k_scan_vjp_points<NEAREST>: one wavefront per (line, theta0) on the persistent grid of the long path (long_waves()), the stages of
// k_exact_points (ibs_exact_grad.hip) on a GeoLine7 line with dPdrho given:
//   1. rows        theta0 folded into the line and its (g, c, f) rows written to the wave's workspace (line_gcf)
//   2. eigenpair   exact_eigenpair<NEAREST>: the pair nearest sigma[sys], else lam_max's; X stays in the workspace
//   3. adjoint     exact_adjoint with the system's gam_bar: g_bar, c_bar, f_bar = gam_bar d gam / d (g, c, f)
//   4. outputs     theta0_bar = S(g_bar g_t + c_bar c_t + f_bar f_t) with the theta0 tangent of the line (line_gcf_dtheta0); the
//                  three cotangent rows to the chunk workspace rows[sys][3][N]; the verdict flag[sys]; optional gam, lam, info
// A system with gam_bar exactly 0 skips stages 3-4 (flag kScanVjpSkip, theta0_bar 0) whatever its solve did.  A non-zero cotangent
// on a failed solve (status bits 0-1), on a refused adjoint (bit 7) or a non-finite gam_bar (which sets bit 1) gives theta0_bar = NaN
// and flag kScanVjpPoison.  info = the solve's word with the adjoint's flags at status bits 6 and 7, as k_exact_points reports them.
//
// k_scan_vjp_reduce: one block per line, a thread per grid point (block-strided), a loop over theta0 ASCENDING that pulls each used
// system's (g_bar, c_bar, f_bar)_j back through the fold (scan_pullback_point, ibs_scan_pullback.hpp: the transpose of line_gcf) and
// adds; dPdrho_bar of the line from the threads' partial sums (grid points block-strided, theta0 ascending), the wave_sum ladder per
// wave and the four wave sums added in order.  A line with a poisoned system is NaN throughout; no other line sees it.  The seven
// planes are never stored per system: the workspace holds 3 rows per system, not 7.
//
// No floating-point atomics and every sum in a fixed order: results are bitwise repeatable and do not depend on the batch, on the
// order of the lines or on the chunking.
#include "ibs_exact_stages.hpp"
#include "ibs_geo_line.hpp"
#include "ibs_scan_pullback.hpp"

namespace ibs {

template <bool NEAREST>
__global__ void __launch_bounds__(64) k_scan_vjp_points(const ScanVjpArgs a) {
  __shared__ double lds[3 * kLongChunk];                    // (the LDS budget of the long path: static_assert at kLongChunk)
  static_assert(sizeof(lds) * 8 <= 160 * 1024, "eight blocks per CU");
  const int lane = threadIdx.x & 63;
  const int N = a.N;
  const ExactPointsWs L = exact_points_ws(N);
  double* my = a.work + (size_t)blockIdx.x * L.total;
  double* G = my + L.g; double* C = my + L.c; double* F = my + L.f;
  const double* gb = my + L.gb; const double* cb = my + L.cb; const double* fb = my + L.fb;
  ExactPointsArgs ea{};                                     // what the shared stages read: N, h, sigma (idx: not wanted)
  ea.N = N; ea.h = a.h; ea.sigma = a.sigma;
  const long n_sys = (long)a.n_lines * a.n_theta0;
  for (long p = blockIdx.x; p < n_sys; p += gridDim.x) {
    const int l = (int)(p / a.n_theta0), t = (int)(p - (long)l * a.n_theta0);
    const double th0 = uniform(a.theta0[t]), mdP = -uniform(a.dPdrho[l]), gbar = uniform(a.gam_bar[p]);
    const GeoLine7 ln = geo_line7(a.geo7, (long)l * a.ld);
    // ---- 1. the line's rows at theta0
    for (int j = lane; j < N; j += kWave) {
      double g, c, f;
      line_gcf(ln, j, mdP, th0, g, c, f);
      G[j] = g; C[j] = c; F[j] = f;
    }
    long_fence();                                           // (rows written by every lane, read by every lane below)
    const SrcLong<double, false> src{G, C, F, nullptr};
    // ---- 2. the eigenpair
    ExactPair e = exact_eigenpair<NEAREST>(src, ea, p, my, L, lds, lane);
    int flag = kScanVjpSkip;
    double tb = 0.0;
    if (gbar != 0.0) {                                      // (a NaN cotangent comes this way too)
      flag = kScanVjpPoison; tb = __builtin_nan("");
      if (!finite_of(gbar)) e.word |= 2 << 16;
      // ---- 3. gam_bar d gam / d (g, c, f)
      else if (((e.word >> 16) & 3) == 0 && (exact_adjoint(src, ea, e, my, L, lds, lane, gbar) & 2) == 0) {
        // ---- 4. contraction with the theta0 tangent; the cotangent rows leave the wave's workspace
        flag = kScanVjpUse;
        double* R = a.rows ? a.rows + (size_t)p * 3 * (size_t)N : nullptr;
        double st = 0.0;
        for (int j = lane; j < N; j += kWave) {
          const double gbj = gb[j], cbj = cb[j], fbj = fb[j];
          double gt, ct, ft;
          line_gcf_dtheta0(ln, j, mdP, th0, gt, ct, ft);
          st += gbj * gt + cbj * ct + fbj * ft;
          if (R) { R[j] = gbj; R[(size_t)N + j] = cbj; R[2 * (size_t)N + j] = fbj; }
        }
        tb = wave_sum(st);
      }
    }
    if (lane == 0) {
      a.flag[p] = flag;
      if (a.theta0_bar) a.theta0_bar[p] = tb;
      if (a.gam) a.gam[p] = e.gam;
      if (a.lam) a.lam[p] = e.lam;
      if (a.info) a.info[p] = e.word;
    }
    long_fence();                                           // (the workspace is reused by this wave's next system)
  }
}

__global__ void __launch_bounds__(256) k_scan_vjp_reduce(const ScanVjpArgs a) {
  __shared__ double part[4];
  const int l = blockIdx.x, N = a.N, nt = a.n_theta0;
  const int* flag = a.flag + (size_t)l * nt;
  bool poison = false;
  for (int t = 0; t < nt; ++t) poison = poison || flag[t] == kScanVjpPoison;
  constexpr double qnan = __builtin_nan("");
  const double mdP = -a.dPdrho[l];
  const GeoLine7 ln = geo_line7(a.geo7, (long)l * a.ld);
  const double* rows = a.rows + (size_t)l * nt * 3 * (size_t)N;
  double dP = 0.0;
  for (int j = threadIdx.x; j < N; j += 256) {
    double v[7], bar[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) { v[k] = ln.at(k, j); bar[k] = 0.0; }
    for (int t = 0; t < nt; ++t) {                          // theta0 ascending
      if (flag[t] != kScanVjpUse) continue;                 // (uniform over the block)
      const double* r = rows + (size_t)t * 3 * (size_t)N;
      scan_pullback_point(r[j], r[(size_t)N + j], r[2 * (size_t)N + j], v, mdP, a.theta0[t], bar, dP);
    }
    if (a.geo_bar[0]) {
#pragma unroll
      for (int k = 0; k < 7; ++k) a.geo_bar[k][(long)l * a.ld_bar + j] = poison ? qnan : bar[k];
    }
  }
  if (a.dPdrho_bar) {
    dP = wave_sum(dP);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = dP;
    __syncthreads();
    if (threadIdx.x == 0) a.dPdrho_bar[l] = poison ? qnan : ((part[0] + part[1]) + part[2]) + part[3];
  }
}

hipError_t launch_scan_vjp(const ScanVjpArgs& a, hipStream_t st) {
  const long n_sys = (long)a.n_lines * a.n_theta0;
  if (n_sys <= 0) return hipSuccess;
  const long grid = persistent_grid(n_sys, a.n_waves, a.work, a.work_doubles, exact_points_ws(a.N).total);
  if (!grid || !a.dPdrho || !a.theta0 || !a.gam_bar || !a.flag) return hipErrorInvalidValue;
  for (int k = 0; k < 7; ++k) if (!a.geo7[k] || (a.geo_bar[0] && !a.geo_bar[k])) return hipErrorInvalidValue;
  if ((a.geo_bar[0] || a.dPdrho_bar) && !a.rows) return hipErrorInvalidValue;
  if (a.sigma) {
    hipLaunchKernelGGL(k_scan_vjp_points<true>, dim3((unsigned)grid), dim3(64), 0, st, a);
    note_launch(grid, 64, "ibs::k_scan_vjp_points<true>");
  } else {
    hipLaunchKernelGGL(k_scan_vjp_points<false>, dim3((unsigned)grid), dim3(64), 0, st, a);
    note_launch(grid, 64, "ibs::k_scan_vjp_points<false>");
  }
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  if (a.rows) {
    hipLaunchKernelGGL(k_scan_vjp_reduce, dim3((unsigned)a.n_lines), dim3(256), 0, st, a);
    note_launch(a.n_lines, 256, "ibs::k_scan_vjp_reduce");
  }
  return hipGetLastError();
}

}  // namespace ibs
