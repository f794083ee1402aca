// Device pieces of the exact vector-Jacobian product of gam and lam (stages A-C of ibs_vjp.hip's header): shared by k_solve_gcf_vjp
// (ibs_vjp.hip: rows and eigenpair in memory) and the geometry-fed point kernel of ibs_exact_grad.hip.
#pragma once
#include "ibs_long.hpp"

namespace ibs {

// residual bound in units of N eps (||A|| + |lam|) max |X|: the library's own eigenpairs reach 84 on the register-resident forms (their X is the
// twisted vector at the last shift of the iteration, lam its Rayleigh polish; 53 on the sub-wave, 42 on the row-streamed form) and 0.05 on the
// division-form paths (long grids, nearest sigma): 2^10 leaves a margin of 12 (the bound at N = 257 is 6e-11 (||A|| + |lam|) max |X|)
constexpr double kVjpResTol = 1024.0;

// Row j of D (utils.py:1610-1616): dX_j = (A_j (X_{j+1} - X_{j-1}) + B_j (X_{j+2} - X_{j-2})) / h, the one-sided forms on the end rows.
// Plain functions of compile-time constants: a select among run-time values (lambdas over A_j / h) was turned into a table in scratch.
__device__ __forceinline__ double fd_a(int j, int N) { return (j == 0 || j == N - 1) ? 2.0 : ((j == 1 || j == N - 2) ? 0.5 : 2.0 / 3.0); }
__device__ __forceinline__ double fd_b(int j, int N) { return (j == 0 || j == N - 1) ? -0.5 : ((j == 1 || j == N - 2) ? 0.0 : -1.0 / 12.0); }
__device__ __forceinline__ double x_at(const double* Xr, int j, int N) { return (j <= 0 || j >= N - 1) ? 0.0 : Xr[j]; }   // X_0 = X_{N-1} = 0
__device__ __forceinline__ double dx_at(const double* Xr, int j, int N, double ih) {
  const int jm1 = j > 0 ? j - 1 : 0, jm2 = j > 1 ? j - 2 : 0, jp1 = j < N - 1 ? j + 1 : N - 1, jp2 = j < N - 2 ? j + 2 : N - 1;
  return ih * xfma(fd_a(j, N), x_at(Xr, jp1, N) - x_at(Xr, jm1, N), fd_b(j, N) * (x_at(Xr, jp2, N) - x_at(Xr, jm2, N)));
}
__device__ __forceinline__ double simpson_wt(int j, int N) { return (j == 0 || j == N - 1) ? 1.0 : ((j & 1) ? 4.0 : 2.0); }   // (the 1/3 cancels)
// the projected adjoint z^_j = z_j - (z^T F X / Q) X_j (0 at the ends and where the solve was skipped)
__device__ __forceinline__ double zh_at(const double* Y, const double* Xr, int j, int N, double pz, bool solve) {
  return (!solve || j <= 0 || j >= N - 1) ? 0.0 : xfma(-pz, Xr[j], Y[j - 1]);
}

template <class Src>
__device__ __forceinline__ void vjp_one(const Src& src, int N, double h, double lam, const double* Xr, double gbar, double lbar,
                                        double* gb_out, double* cb_out, double* fb_out, int* info_out, long sys, double* work,
                                        double* lds, int lane) {
  constexpr double pivmin = 2.2250738585072014e-292;
  const int n = N - 2;
  const double ih = 1.0 / h, ih2 = ih * ih;
  double* V = work;                  // -w g dX, later the pivots D+ (rows < k) / D- (rows > k)
  double* B = work + N;              // r on the interior rows
  double* Y = work + 2 * (size_t)N;  // forward-eliminated right-hand side, then z
  // ---- A. quotient, residual, r
  double P = 0.0, Q1 = 0.0, Q = 0.0, res = 0.0, na = 0.0, best = -1.0;
  int bi = 0;
  bool bad = !finite_of(lam) || !finite_of(gbar) || !finite_of(lbar);
  for (int j = lane; j < N; j += kWave) {
    const double X = x_at(Xr, j, N), dX = dx_at(Xr, j, N, ih), w = simpson_wt(j, N);
    const double gj = src.g(j), cj = src.c(j), fj = src.f(j);
    const double X2 = w * (X * X), dX2 = w * (dX * dX);
    P += cj * X2 - gj * dX2;                                                       // utils.py:1618
    Q1 = xfma(fj, X2, Q1);                                                         // utils.py:1619
    V[j] = -(w * gj) * dX;
    bad = bad || !(gj > 0.0) || !(fj > 0.0) || !finite_of(gj) || !finite_of(cj) || !finite_of(fj);
    if (j >= 1 && j <= N - 2) {
      bad = bad || !finite_of(X);
      const double e_lo = src.e(j - 1, ih2), e_hi = src.e(j, ih2);
      const double d = cj - (e_lo + e_hi);
      const double rj = xfma(e_lo, x_at(Xr, j - 1, N), xfma(xfma(-lam, fj, d), X, e_hi * x_at(Xr, j + 1, N)));
      const double rf = 1.0 / fj;
      res = xmax(res, xabs(rj) * rf);
      na = xmax(na, (xabs(d) + e_lo + e_hi) * rf);
      Q = xfma(fj * X, X, Q);
      if (xabs(X) > best) { best = xabs(X); bi = j; }
    }
  }
  P = wave_sum(P); Q1 = wave_sum(Q1); Q = wave_sum(Q);
  res = uniform(wave_max(res)); na = uniform(wave_max(na));
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {                     // row of largest |X|, the first of equals
    const double b2 = __shfl_xor(best, d);
    const int i2 = __shfl_xor(bi, d);
    if (b2 > best || (b2 == best && i2 < bi)) { best = b2; bi = i2; }
  }
  const double xm = uniform(best);
  const int k = __builtin_amdgcn_readfirstlane(bi) - 1;    // (interior row index)
  const double gam = P / Q1;
  bad = __any(bad) || !(Q1 > 0.0) || !(Q > 0.0) || !(xm > 0.0) || !finite_of(gam) || !finite_of(na) ||
        !(res <= kVjpResTol * (double)N * Eps<double>::v * (na + xabs(lam)) * xm);
  if (bad) {
    constexpr double qnan = __builtin_nan("");
    for (int j = lane; j < N; j += kWave) { gb_out[j] = qnan; cb_out[j] = qnan; fb_out[j] = qnan; }
    if (info_out && lane == 0) info_out[sys] = 2 << 16;
    return;
  }
  const bool solve = gbar != 0.0;
  bool tiny = false;
  double zs = 0.0;                                        // z^T F X
  if (solve) {
    long_fence();                                         // (V is read across lanes)
    const double rq = 2.0 / Q1;
    for (int j = 1 + lane; j <= N - 2; j += kWave) {
      double dt = fd_a(j - 1, N) * V[j - 1] - fd_a(j + 1, N) * V[j + 1];           // h (D^T V)_j
      if (j >= 2) dt = xfma(fd_b(j - 2, N), V[j - 2], dt);
      if (j <= N - 3) dt = xfma(-fd_b(j + 2, N), V[j + 2], dt);
      const double wX = simpson_wt(j, N) * x_at(Xr, j, N);
      B[j - 1] = rq * xfma(ih, dt, wX * xfma(-gam, src.f(j), src.c(j)));
    }
    long_fence();                                         // (V is overwritten by the pivots below)
    // ---- B1. elimination: lane 0 rows 0 .. k-1 upwards (D+), lane 1 rows n-1 .. k+1 downwards (D-).  LDS per direction:
    // [a = d - lam f | e to the previous row of the direction | right-hand side]; the pivot replaces a, the eliminated rhs b.
    const int nl = k, nt = n - 1 - k, smax = nl > nt ? nl : nt;
    const int dsel = lane & 1;
    {
      double* xa = lds + dsel * 3 * kVecChunk; const double* xe = xa + kVecChunk; double* xb = xa + 2 * kVecChunk;
      double Dq = 1.0, yq = 0.0;
      for (int c0 = 0; c0 < smax; c0 += kVecChunk) {
        const int ml = nl - c0 < 0 ? 0 : (nl - c0 < kVecChunk ? nl - c0 : kVecChunk);
        const int mt = nt - c0 < 0 ? 0 : (nt - c0 < kVecChunk ? nt - c0 : kVecChunk);
        for (int i = lane; i < kVecChunk; i += kWave) {
          if (i < ml) {
            const int r = c0 + i;
            const double e_lo = src.e(r, ih2), e_hi = src.e(r + 1, ih2);
            lds[i] = xfma(-lam, src.f(r + 1), src.c(r + 1) - (e_lo + e_hi)); lds[kVecChunk + i] = e_lo; lds[2 * kVecChunk + i] = B[r];
          }
          if (i < mt) {
            const int r = n - 1 - (c0 + i);
            const double e_lo = src.e(r, ih2), e_hi = src.e(r + 1, ih2);
            lds[3 * kVecChunk + i] = xfma(-lam, src.f(r + 1), src.c(r + 1) - (e_lo + e_hi)); lds[4 * kVecChunk + i] = e_hi;
            lds[5 * kVecChunk + i] = B[r];
          }
        }
        wave_lds_sync();
        if (lane < 2) {
          const int m = dsel ? mt : ml;
          for (int i0 = 0; i0 < m; i0 += 8) {
            double av[8], ev[8], bv[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) { const int i = i0 + u < m ? i0 + u : m - 1; av[u] = xa[i]; ev[u] = xe[i]; bv[u] = xb[i]; }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
              if (i0 + u < m) {
                if (c0 + i0 + u == 0) { Dq = av[u]; yq = bv[u]; }
                else { const double l = ev[u] * fast_rcp(Dq); Dq = xfma(-l, ev[u], av[u]); yq = xfma(-l, yq, bv[u]); }
                if (xabs(Dq) < pivmin) { Dq = -pivmin; tiny = true; }
              }
              av[u] = Dq; bv[u] = yq;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) if (i0 + u < m) { xa[i0 + u] = av[u]; xb[i0 + u] = bv[u]; }
          }
        }
        wave_lds_sync();
        for (int i = lane; i < kVecChunk; i += kWave) {
          if (i < ml) { const int r = c0 + i; V[r] = lds[i]; Y[r] = lds[2 * kVecChunk + i]; }
          if (i < mt) { const int r = n - 1 - (c0 + i); V[r] = lds[3 * kVecChunk + i]; Y[r] = lds[5 * kVecChunk + i]; }
        }
        wave_lds_sync();
      }
    }
    long_fence();
    // ---- B2. back substitution from the twist row outwards, z_k = 0: rows k-1 .. 0 (lane 0), z_r = y_r / D+_r - e_{r+1} / D+_r
    // z_{r+1}; rows k+1 .. n-1 (lane 1), z_r = y_r / D-_r - e_r / D-_r z_{r-1}.  LDS per direction [u = y / D | m = e / D]: formed
    // by all lanes, the chain is one fma per row; z replaces u.
    {
      double* xu = lds + dsel * 3 * kVecChunk; const double* xm_ = xu + kVecChunk;
      double z = 0.0;
      for (int c0 = 0; c0 < smax; c0 += kVecChunk) {
        const int ml = nl - c0 < 0 ? 0 : (nl - c0 < kVecChunk ? nl - c0 : kVecChunk);
        const int mt = nt - c0 < 0 ? 0 : (nt - c0 < kVecChunk ? nt - c0 : kVecChunk);
        for (int i = lane; i < kVecChunk; i += kWave) {
          if (i < ml) { const int r = k - 1 - (c0 + i); const double Dr = V[r]; lds[i] = Y[r] / Dr; lds[kVecChunk + i] = src.e(r + 1, ih2) / Dr; }
          if (i < mt) { const int r = k + 1 + (c0 + i); const double Dr = V[r]; lds[3 * kVecChunk + i] = Y[r] / Dr; lds[4 * kVecChunk + i] = src.e(r, ih2) / Dr; }
        }
        wave_lds_sync();
        if (lane < 2) {
          const int m = dsel ? mt : ml;
          for (int i0 = 0; i0 < m; i0 += 8) {
            double uv[8], mv[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) { const int i = i0 + u < m ? i0 + u : m - 1; uv[u] = xu[i]; mv[u] = xm_[i]; }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
              if (i0 + u < m) z = xfma(-mv[u], z, uv[u]);
              uv[u] = z;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) if (i0 + u < m) xu[i0 + u] = uv[u];
          }
        }
        wave_lds_sync();
        for (int i = lane; i < kVecChunk; i += kWave) {
          if (i < ml) Y[k - 1 - (c0 + i)] = lds[i];
          if (i < mt) Y[k + 1 + (c0 + i)] = lds[3 * kVecChunk + i];
        }
        wave_lds_sync();
      }
      if (lane == 0) Y[k] = 0.0;
    }
    long_fence();
    for (int j = 1 + lane; j <= N - 2; j += kWave) zs = xfma(Y[j - 1] * src.f(j), x_at(Xr, j, N), zs);
    zs = wave_sum(zs);
  }
  // ---- C. projection and the cotangent rows
  const double pz = zs / Q;
  const double gq = gbar / Q1, lq = lbar / Q;
  for (int j = lane; j < N; j += kWave) {
    const double X = x_at(Xr, j, N), dX = dx_at(Xr, j, N, ih), w = simpson_wt(j, N), z = zh_at(Y, Xr, j, N, pz, solve);
    const double X2 = X * X;
    // cotangents of the half-grid g between points j - 1, j and j, j + 1 (0 beyond the ends: X and z^ vanish there)
    const double xm1 = x_at(Xr, j - 1, N), xp1 = x_at(Xr, j + 1, N);
    const double zm1 = zh_at(Y, Xr, j - 1, N, pz, solve), zp1 = zh_at(Y, Xr, j + 1, N, pz, solve);
    const double dlo = X - xm1, dhi = xp1 - X;
    const double ghm = j >= 1 ? ih2 * dlo * xfma(gbar, z - zm1, -lq * dlo) : 0.0;
    const double ghp = j <= N - 2 ? ih2 * dhi * xfma(gbar, zp1 - z, -lq * dhi) : 0.0;
    gb_out[j] = xfma(-gq * w, dX * dX, 0.5 * (ghm + ghp));
    cb_out[j] = xfma(gq * w, X2, xfma(-gbar * z, X, lq * X2));
    fb_out[j] = xfma(-gam * gq * w, X2, xfma(gbar * lam * z, X, -lq * lam * X2));
  }
  const bool any_tiny = __any(tiny);                      // (all lanes: tiny is lane 0's leading and lane 1's trailing block)
  if (info_out && lane == 0) info_out[sys] = any_tiny ? (1 << 16) : 0;
}

}  // namespace ibs
