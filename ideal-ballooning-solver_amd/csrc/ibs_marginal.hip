// Marginal stability: the factor s* by which the pressure gradient of a line may be scaled, at fixed geometry arrays, before the
// line goes unstable.  c is linear in dPdrho (utils.py:1561) and f > 0 only scales rows, so with D the stiffness matrix of
// utils.py:1574-1592 (D_jj = e_{j-1} + e_j, D_{j,j+-1} = -e, e_k = (g_k + g_{k+1}) / 2 h^2) and C = diag(c):
//   T(s) = s C - D,   s* = inf { s > 0 : lam_max(T(s)) >= 0 } = 1 / mu_max of C x = mu D x;   s* < 1: the line is unstable now.
// Nothing upstream corresponds; the quantity generalises the marginal-stability scan of bishop_ball_s-alpha.py:90-115.  FP64, every
// odd N in [66, 65,537], one wavefront per system on the persistent grid of the long path, division form throughout (ibs_long.hpp):
//   1. bounds        a rigorous upper bound of s* from unit vectors and four trial vectors, and the data checks, in one parallel pass
//                    (marginal_bounds); no c_j > 0: s* = +inf, mu = 0, informational status bit 8, no multisection
//   2. scale         64-way multisection on "the inertia count of T(s) at 0 is >= 1" from [0, upper] to a width of 8 eps s
//                    (marginal_multisect; the count is count_above_chunked on an adapter of the rows); cap 24 passes (status bit 0)
//   3. mode          long_vector_growth on T(s*) at lam = 0: X with zero ends and largest entry +1 (the Perron vector has one sign)
//                    and its FD4 / Simpson quotient gam0, which is O(h^2) from 0
//   4. derivatives   q = sum_j c_j X_j^2;  d s* / d c_j = -s* X_j^2 / q;  d s* / d e_k = (X_{k+1} - X_k)^2 / q, folded onto g:
//                    d s* / d g_j = (ebar_{j-1} + ebar_j) / 2 h^2 (the end rows have one cell): Hellmann-Feynman on the discrete pencil,
//                    exact for it; no adjoint solve, no floating-point atomics, bitwise repeatable and independent of the batch.
//                    k_marginal_scan contracts them with the theta0 tangent of the rows (utils.py:1669-1673) as it is formed.
// Outputs: scale, mu = 1 / s*, gam0, X, g_bar, c_bar (k_marginal_gcf); scale, mu, d s* / d theta0, d s* / d dPdrho = -s* / dPdrho
// (k_marginal_scan); info (bits 0-15 = multisection passes, status bits as in include/ibs.h).  Systems with status bit 0 or 1 get
// NaN vectors and derivatives; with bit 8 the derivatives are 0 (s* is locally constant) and X, gam0 are NaN.
// Per-wave workspace: marginal_ws(N, scan) (ibs_launch.hpp), in global memory.
#include "ibs_marginal.hpp"
#include "ibs_geo_line.hpp"
#include "ibs_launch.hpp"

namespace ibs {

__global__ void __launch_bounds__(64) k_marginal_gcf(const MarginalArgs a) {
  __shared__ double lds[3 * kLongChunk];                    // (the LDS budget of the long path: static_assert at kLongChunk)
  static_assert(sizeof(lds) * 8 <= 160 * 1024, "eight blocks per CU");
  const int lane = threadIdx.x & 63;
  const int N = a.N;
  const MarginalWs L = marginal_ws(N, false);
  double* my = a.work + (size_t)blockIdx.x * L.total;
  double* Xw = my + L.X;
  const bool want_grad = a.g_bar || a.c_bar;
  const bool want_vec = want_grad || a.X || a.gam0;         // (kernel-uniform)
  const double ih2 = 1.0 / (a.h * a.h);
  for (long sys = blockIdx.x; sys < a.n_sys; sys += gridDim.x) {
    const double* G = a.g + sys * a.ld; const double* C = a.c + sys * a.ld;
    int status, passes;
    double gam0;
    const double s = marginal_one(G, C, N, a.h, my + L.work, Xw, want_vec, lds, status, passes, gam0);
    if (lane == 0) {
      a.scale[sys] = s;
      if (a.mu) a.mu[sys] = 1.0 / s;                        // (0 with s* = +inf, NaN with invalid data)
      if (a.gam0) a.gam0[sys] = gam0;
      if (a.info) a.info[sys] = passes | (status << 16);
    }
    if (want_vec) {
      const double fill = (status & 256) ? 0.0 : __builtin_nan("");
      double q = 0.0;
      if (status == 0 && want_grad) {
        for (int j = lane; j < N; j += kWave) q = xfma(C[j] * Xw[j], Xw[j], q);
        q = wave_sum(q);
      }
      const double rq = 1.0 / q;
      for (int j = lane; j < N; j += kWave) {
        const long o = sys * N + j;
        if (status == 0) {
          const double x0 = Xw[j];
          if (a.X) a.X[o] = x0;
          if (want_grad) {
            const double dm = j > 0 ? x0 - Xw[j - 1] : 0.0, dp = j < N - 1 ? Xw[j + 1] - x0 : 0.0;
            if (a.g_bar) a.g_bar[o] = 0.5 * ih2 * xfma(dm, dm, dp * dp) * rq;
            if (a.c_bar) a.c_bar[o] = -s * (x0 * x0) * rq;
          }
        } else {
          if (a.X) a.X[o] = __builtin_nan("");
          if (a.g_bar) a.g_bar[o] = fill;
          if (a.c_bar) a.c_bar[o] = fill;
        }
      }
    }
    long_fence();                                           // (the workspace is reused by this wave's next system)
  }
}

__global__ void __launch_bounds__(64) k_marginal_scan(const MarginalScanArgs a) {
  __shared__ double lds[3 * kLongChunk];
  static_assert(sizeof(lds) * 8 <= 160 * 1024, "eight blocks per CU");
  const int lane = threadIdx.x & 63;
  const int N = a.N;
  const MarginalWs L = marginal_ws(N, true);
  double* my = a.work + (size_t)blockIdx.x * L.total;
  double* Xw = my + L.X; double* G = my + L.g; double* C = my + L.c;
  const bool want_vec = a.dth0 != nullptr;                  // (kernel-uniform)
  const double ih2 = 1.0 / (a.h * a.h);
  const long n_sys = (long)a.n_lines * a.n_theta0;
  for (long sys = blockIdx.x; sys < n_sys; sys += gridDim.x) {
    const int line = (int)(sys / a.n_theta0), it0 = (int)(sys - (long)line * a.n_theta0);
    const double th0 = uniform(a.theta0[it0]), dP = uniform(a.dPdrho[line]), mdP = -dP;
    const GeoLine7 ln = geo_line7(a.geo7, (long)line * a.ld);
    // ---- the rows at theta0
    for (int j = lane; j < N; j += kWave) line_gcf(ln, j, mdP, th0, G[j], C[j]);
    long_fence();                                           // (rows written by every lane, read by every lane below)
    int status, passes;
    double gam0;
    const double s = marginal_one(G, C, N, a.h, my + L.work, Xw, want_vec, lds, status, passes, gam0);
    double dth = (status & 256) ? 0.0 : __builtin_nan("");
    if (want_vec && status == 0) {
      // d s* / d theta0 = sum_j (d s* / d g_j) g_t,j + (d s* / d c_j) c_t,j with the tangents of utils.py:1669-1673
      double q = 0.0, sg = 0.0, sc = 0.0;
      for (int j = lane; j < N; j += kWave) {
        const double x0 = Xw[j], x2 = x0 * x0;
        double gt, ct;
        line_gcf_dtheta0(ln, j, mdP, th0, gt, ct);
        q = xfma(C[j], x2, q);
        sg = xfma(gt, pencil_weight(Xw, j, N), sg);
        sc = xfma(ct, x2, sc);
      }
      q = wave_sum(q); sg = wave_sum(sg); sc = wave_sum(sc);
      dth = (0.5 * ih2 * sg - s * sc) / q;
    }
    if (lane == 0) {
      a.scale[sys] = s;
      if (a.mu) a.mu[sys] = 1.0 / s;
      if (a.dth0) a.dth0[sys] = dth;
      if (a.ddP) a.ddP[sys] = (status & 256) ? 0.0 : -s / dP;        // c is linear in dPdrho: s*(k dPdrho) = s* / k
      if (a.info) a.info[sys] = passes | (status << 16);
    }
    long_fence();                                           // (the workspace is reused by this wave's next system)
  }
}

hipError_t launch_marginal_gcf(const MarginalArgs& a, hipStream_t st) {
  if (a.n_sys <= 0) return hipSuccess;
  const long grid = persistent_grid(a.n_sys, a.n_waves, a.work, a.work_doubles, marginal_ws(a.N, false).total);
  if (!grid || !a.g || !a.c || !a.scale) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_marginal_gcf, dim3((unsigned)grid), dim3(64), 0, st, a);
  note_launch(grid, 64, "ibs::k_marginal_gcf");
  return hipGetLastError();
}

hipError_t launch_marginal_scan(const MarginalScanArgs& a, hipStream_t st) {
  const long n_sys = (long)a.n_lines * a.n_theta0;
  if (n_sys <= 0) return hipSuccess;
  const long grid = persistent_grid(n_sys, a.n_waves, a.work, a.work_doubles, marginal_ws(a.N, true).total);
  if (!grid || !a.dPdrho || !a.theta0 || !a.scale) return hipErrorInvalidValue;
  for (int k = 0; k < 7; ++k) if (!a.geo7[k]) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_marginal_scan, dim3((unsigned)grid), dim3(64), 0, st, a);
  note_launch(grid, 64, "ibs::k_marginal_scan");
  return hipGetLastError();
}

}  // namespace ibs
