// Device pieces of the division-form long-grid path shared by ibs_long.hip (lam_max: k_solve_gcf_long) and ibs_nearest.hip (the
// eigenpair nearest a shift: k_solve_gcf_nearest).  One wavefront per system, the rows read from memory; see ibs_long.hip's header.
#pragma once
#include "ibs_wave.hpp"

namespace ibs {

template <typename TI, bool HAS_GH>
struct SrcLong {
  static constexpr bool kHasGh = HAS_GH;
  const TI* gg; const TI* cg; const TI* fg; const TI* ghg;
  __device__ __forceinline__ double g(int j) const { return (double)gg[j]; }
  __device__ __forceinline__ double c(int j) const { return (double)cg[j]; }
  __device__ __forceinline__ double f(int j) const { return (double)fg[j]; }
  __device__ __forceinline__ double gh(int k) const { return (double)ghg[k]; }
  // e_k = half-grid g between grid points k and k + 1, over h^2 (utils.py:1574-1576, 1584-1592)
  __device__ __forceinline__ double e(int k, double ih2) const {
    if constexpr (HAS_GH) return (double)ghg[k] * ih2;
    else return 0.5 * ((double)gg[k] + (double)gg[k + 1]) * ih2;
  }
};

// Every S-th grid point of a system: the same operator on a coarser grid (two-grid start of the multisection, long_lam_max)
template <class Src>
struct SrcCoarse {
  static constexpr bool kHasGh = false;
  const Src& s; int S;
  __device__ __forceinline__ double g(int j) const { return s.g(S * j); }
  __device__ __forceinline__ double c(int j) const { return s.c(S * j); }
  __device__ __forceinline__ double f(int j) const { return s.f(S * j); }
  __device__ __forceinline__ double e(int k, double ih2c) const { return 0.5 * (s.g(S * k) + s.g(S * (k + 1))) * ih2c; }
};

// Division-form count of one system at 64 shifts (lane L = shift L) with the rows passed through LDS in chunks of kLongChunk: the 64
// lanes form d_r, e_r^2, f_r of a chunk together (coalesced loads), then every lane runs the recurrence over the chunk from LDS (all
// lanes read the same address: broadcast) -- the serial chain never waits for global memory (read per row it cost one exposed memory
// latency per four rows: 27 ms per system at N = 8,193; so: 3).  Same arithmetic as count_above_rows (ibs_wave.hpp).
constexpr int kLongChunk = 768;      // 18 KB per block: eight blocks per CU (the persistent grid of long_waves(), ibs_api.hip) stay resident -- the
                                     // recurrence is a chain of dependent divisions, two waves per SIMD overlap almost freely.  Chunks of 1,024: six
                                     // blocks per CU, 2,048 systems ran as 1,536 + 512 (24 ms at N = 16,385 against 15); chunks of 384, sixteen
                                     // blocks: one system 25 % slower (twice the chunk boundaries), 8,192 systems no faster
static_assert(8 * 3 * kLongChunk * sizeof(double) <= 160 * 1024, "eight blocks per CU");
constexpr int kVecChunk = kLongChunk / 2;      // pivots / eigenvector: two directions x (two operands + one result) in the same LDS
template <class Src>
__device__ __forceinline__ int count_above_chunked(const Src& src, int n, double ih2, double sig, double* lds, int lane) {
  constexpr double pivmin = 2.2250738585072014e-292;
  double* rd = lds; double* re2 = lds + kLongChunk; double* rf = lds + 2 * kLongChunk;
  int cnt = 0;
  double q = 1.0;
  for (int r0 = 0; r0 < n; r0 += kLongChunk) {
    const int m = n - r0 < kLongChunk ? n - r0 : kLongChunk;
    for (int i = lane; i < m; i += kWave) {
      const int r = r0 + i;
      const double e_lo = src.e(r, ih2), e_hi = src.e(r + 1, ih2);
      rd[i] = src.c(r + 1) - (e_lo + e_hi); re2[i] = e_lo * e_lo; rf[i] = src.f(r + 1);
    }
    wave_lds_sync();
    int i = 0;
    if (r0 == 0) {
      q = xfma(-sig, rf[0], rd[0]);
      q = xabs(q) < pivmin ? -pivmin : q;
      cnt += q > 0.0 ? 1 : 0;
      i = 1;
    }
#pragma unroll 8
    for (; i < m; ++i) {
      const double a = xfma(-sig, rf[i], rd[i]);
      q = xfma(-re2[i], fast_rcp(q), a);
      q = xabs(q) < pivmin ? -pivmin : q;
      cnt += q > 0.0 ? 1 : 0;
    }
    wave_lds_sync();
  }
  return cnt;
}

__device__ __forceinline__ void long_fence() {      // stores of two lanes, read by all lanes of the same wave afterwards
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
}

// ---- 1. bounds and data checks (lanes strided over the rows; the results are wave-uniform)
//   hi: Gershgorin upper bound of the spectrum, max_r c_r / f_r, + 8 eps ||A||
//   lo: lower bound of lam_max -- max_r d_r / f_r (unit vectors) or the best Rayleigh quotient of four trial vectors
//   lmin: lower bound of the whole spectrum, min_r (d_r - e_r - e_{r+1}) / f_r, - 8 eps ||A||
//   normA = max_r (|d_r| + e_r + e_{r+1}) / f_r;  bad: invalid data (non-finite, g <= 0 or f <= 0)
//   (LMIN: lmin is wanted; else it is left 0 and costs nothing)
struct LongBounds { double normA, lo, hi, lmin; bool bad; };
template <bool LMIN, class Src>
__device__ __forceinline__ LongBounds long_bounds(const Src& src, int N, double ih2, int lane) {
  // The Gershgorin-type lower end max_r d_r / f_r is ~ -||A|| (d_r = c_r - 2 g / h^2) while lam_max is O(1): every factor 64 of
  // bracket is a pass over the rows.  Rayleigh quotients of four trial vectors x_j = sin^p(pi j / (N - 1)), p = 1, 4, 16, 64 (zero at
  // both ends like the eigenfunctions, ever more localised about the middle of the grid where ballooning modes sit) are rigorous
  // lower bounds of lam_max (Courant-Fischer) and cost this one parallel pass: on s-alpha and geometry lines the bracket starts
  // O(1) wide instead of O(||A||), three passes of nine less; on rough coefficients the bounds are poor and nothing changes.
  const int n = N - 2;
  double vhi = -1e300, vlo = -1e300, vna = 0.0, vmn = -1e300;
  double tn[4] = {0.0, 0.0, 0.0, 0.0}, td[4] = {0.0, 0.0, 0.0, 0.0};
  bool bad = false;
  const double dth = 3.141592653589793 / (double)(N - 1);
  double sdl, cdl;
  sincos(dth, &sdl, &cdl);
  for (int r = lane; r < n; r += kWave) {
    const int j = r + 1;
    const double e_lo = src.e(r, ih2), e_hi = src.e(j, ih2);
    const double cj = src.c(j), fj = src.f(j), gj = src.g(j);
    const double d = cj - (e_lo + e_hi);
    const double rf = 1.0 / fj;
    vhi = xmax(vhi, cj * rf); vlo = xmax(vlo, d * rf); vna = xmax(vna, (xabs(d) + e_lo + e_hi) * rf);
    if constexpr (LMIN) vmn = xmax(vmn, -((d - (e_lo + e_hi)) * rf));
    bad = bad || !(fj > 0.0) || !(gj > 0.0) || !(e_lo > 0.0) || !(e_hi > 0.0) || !finite_of(cj) || !finite_of(fj) || !finite_of(e_lo + e_hi);
    double sj, cjs;
    sincos(dth * (double)j, &sj, &cjs);
    double xm = sj * cdl - cjs * sdl, x0 = sj, xp = sj * cdl + cjs * sdl;      // sin at j - 1, j, j + 1
    xm = j == 1 ? 0.0 : xm; xp = j == N - 2 ? 0.0 : xp;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      tn[k] = xfma(x0, xfma(e_lo, xm, xfma(d, x0, e_hi * xp)), tn[k]);
      td[k] = xfma(fj * x0, x0, td[k]);
      xm *= xm; xm *= xm; x0 *= x0; x0 *= x0; xp *= xp; xp *= xp;               // p -> 4 p
    }
  }
  if (lane == 0) bad = bad || !(src.g(0) > 0.0) || !(src.g(N - 1) > 0.0);
  LongBounds b;
  b.normA = uniform(wave_max(vna));
  b.hi = uniform(wave_max(vhi)) + 8.0 * Eps<double>::v * b.normA;
  b.lo = uniform(wave_max(vlo)) - 8.0 * Eps<double>::v * b.normA;
  b.lmin = 0.0;
  if constexpr (LMIN) b.lmin = -uniform(wave_max(vmn)) - 8.0 * Eps<double>::v * b.normA;
  {
    double rho = -1e300;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const double a = wave_sum(tn[k]), bb = wave_sum(td[k]);
      const double q = a / bb;
      rho = (bb > 0.0 && finite_of(q) && q > rho) ? q : rho;
    }
    rho = uniform(rho) - (8.0 + 0.5 * (double)N) * Eps<double>::v * b.normA;       // (rounding of the sums: N terms)
    if (rho > b.lo && rho < b.hi) b.lo = rho;
  }
  b.bad = __any(bad) || !finite_of(b.normA);
  return b;
}

// ---- 2. lam_max from the bracket [lo, hi] of long_bounds, to 2 eps ||A||.  Two-grid start: where the trial vectors have brought the
// bracket down from O(||A||) to O(1) -- smooth coefficients -- lam_max of the same operator on every 16th and every 8th grid point (a
// sixteenth / an eighth of a pass per multisection pass, closed to 1e-7 of the bracket) differ from the fine grid's by C (16 h)^2 and
// C (8 h)^2: their Richardson extrapolate, +- a quarter of their difference, is where the fine multisection starts (a bracket that
// misses is moved and widened by multisect itself, at a pass per miss).  6 fine passes become 3-4 + 0.6.
// passes: in units of a fine pass; returns false if the multisection did not close.
template <class Src>
__device__ __forceinline__ bool long_lam_max(const Src& src, int N, double ih2, double lo, double hi, double normA, double* lds, int lane,
                                             double& lam, int& passes) {
  const int n = N - 2;
  int coarse_passes = 0;
  if ((N - 1) % 16 == 0 && N >= 1025 && (hi - lo) < 1e-3 * normA) {
    double l16 = 0.0, l8 = 0.0;
    int p16 = 0, p8 = 0;
    const double stop_c = 1e-7 * (hi - lo) / (Eps<double>::v * normA);      // multisect ends at width <= stop eps ||A||
    const SrcCoarse<Src> c16{src, 16}, c8{src, 8};
    const int n16 = (N - 1) / 16 - 1, n8 = (N - 1) / 8 - 1;
    const bool ok16 = multisect<double>([&](double sig) { return count_above_chunked(c16, n16, ih2 * (1.0 / 256.0), sig, lds, lane); },
                                        lo, hi, normA, stop_c, lane, l16, p16);
    bool ok8 = false;
    if (ok16) {
      const double w8 = 1e-2 * (hi - lo);                                  // (the two coarse grids differ by far less on smooth data)
      ok8 = multisect<double>([&](double sig) { return count_above_chunked(c8, n8, ih2 * (1.0 / 64.0), sig, lds, lane); },
                              xmax(lo, l16 - w8), xmin(hi, l16 + w8), normA, stop_c, lane, l8, p8);
    }
    coarse_passes = (p16 + 15) / 16 + (p8 + 7) / 8;                         // (in units of a fine pass, rounded up)
    if (ok16 && ok8) {
      const double dl = l16 - l8;
      const double est = l8 - dl * (1.0 / 3.0);
      const double w = xmax(0.25 * xabs(dl), 8.0 * 1e-7 * (hi - lo));
      const double lo2 = xmax(lo, est - w), hi2 = xmin(hi, est + w);
      if (lo2 < hi2) { lo = lo2; hi = hi2; }
    }
  }
  const bool ok = multisect<double>([&](double sig) { return count_above_chunked(src, n, ih2, sig, lds, lane); }, lo, hi, normA, 2.0, lane, lam, passes);
  passes += coarse_passes;
  return ok;
}

// ---- 3-4. eigenvector and growth rate at an eigenvalue lam (closed to a few eps ||A||); returns gam, writes X / dX (optional).
// Per-wave workspace `work`: 3 N doubles (D+, D-, d - lam f; the last becomes z).
//   3. twisted factorisation N_k D_k N_k^T of T - lam F (the getvec step of MRRR): forward pivots D+ (lane 0) and backward pivots D-
//      (lane 1) in one serial pass, gamma_r = D+_r + D-_r - (d_r - lam f_r) in parallel, twist row k = argmin |gamma_r|, then z_k = 1,
//      z_{r-1} = -e_r z_r / D+_{r-1} downwards (lane 0) and z_{r+1} = -e_{r+1} z_r / D-_{r+1} upwards (lane 1)
//   4. X = z / max |z| with zero end points, FD2/FD4 derivative, composite Simpson quotient: the arithmetic of finish() in
//      ibs_kernels.hip, i.e. utils.py:1601-1621.
// SIGNED: divide by the entry of largest magnitude itself (so that it becomes +1) instead of by its magnitude -- the same thing for
// lam_max, whose eigenvector has one sign (the off-diagonal of T is positive); an interior eigenvector changes sign.
template <bool SIGNED, typename TI, class Src>
__device__ __forceinline__ double long_vector_growth(const Src& src, int N, double h, double lam, long sys, double* work, TI* X_out,
                                                     TI* dX_out, double* lds, int lane) {
  constexpr double pivmin = 2.2250738585072014e-292;
  const int n = N - 2;
  const double ih2 = 1.0 / (h * h);
  double* Dp = work; double* Dm = work + N; double* A = work + 2 * (size_t)N;     // A[r] = d_r - lam f_r, later z_r
  // ---- 3a. pivots: lane 0 walks the rows upwards (D+), lane 1 downwards (D-).  The rows pass through LDS in chunks of kVecChunk
  // per direction: all 64 lanes form a_r and e_r^2 (coalesced loads), lanes 0 / 1 run the two recurrences from LDS eight rows at a
  // time (operands in registers before the dependent chain starts), all lanes write the pivots out (coalesced).  Read and written
  // row by row from the two lanes the chain waited for global memory at every step: 400 cycles per row, as long as the whole
  // multisection.
  {
    const int dsel = lane & 1;
    const double* xa = lds + dsel * 3 * kVecChunk; const double* xe = xa + kVecChunk; double* xq = lds + dsel * 3 * kVecChunk + 2 * kVecChunk;
    double q = 1.0;
    for (int c0 = 0; c0 < n; c0 += kVecChunk) {
      const int m = n - c0 < kVecChunk ? n - c0 : kVecChunk;
      for (int i = lane; i < m; i += kWave) {
        {
          const int r = c0 + i, j = r + 1;
          const double e_lo = src.e(r, ih2), e_hi = src.e(j, ih2);
          lds[i] = xfma(-lam, src.f(j), src.c(j) - (e_lo + e_hi)); lds[kVecChunk + i] = e_lo * e_lo;
        }
        {
          const int r = n - 1 - (c0 + i), j = r + 1;
          const double e_lo = src.e(r, ih2), e_hi = src.e(j, ih2);
          lds[3 * kVecChunk + i] = xfma(-lam, src.f(j), src.c(j) - (e_lo + e_hi)); lds[4 * kVecChunk + i] = e_hi * e_hi;
        }
      }
      wave_lds_sync();
      if (lane < 2) {
        for (int i0 = 0; i0 < m; i0 += 8) {
          double av[8], ev[8], qv[8];
#pragma unroll
          for (int u = 0; u < 8; ++u) { const int i = i0 + u < m ? i0 + u : m - 1; av[u] = xa[i]; ev[u] = xe[i]; }
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            if (i0 + u < m) {
              q = (c0 + i0 + u == 0) ? av[u] : xfma(-ev[u], fast_rcp(q), av[u]);      // (the arithmetic of the counts)
              q = xabs(q) < pivmin ? -pivmin : q;
            }
            qv[u] = q;
          }
#pragma unroll
          for (int u = 0; u < 8; ++u) if (i0 + u < m) xq[i0 + u] = qv[u];
        }
      }
      wave_lds_sync();
      for (int i = lane; i < m; i += kWave) {
        Dp[c0 + i] = lds[2 * kVecChunk + i]; A[c0 + i] = lds[i]; Dm[n - 1 - (c0 + i)] = lds[5 * kVecChunk + i];
      }
      wave_lds_sync();
    }
  }
  long_fence();
  // ---- 3b. twist row: the smallest |gamma_r|
  double best = 1e300;
  int bi = 0;
  for (int r = lane; r < n; r += kWave) {
    const double gm = xabs(Dp[r] + Dm[r] - A[r]);
    if (gm < best) { best = gm; bi = r; }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const double b2 = __shfl_xor(best, d);
    const int i2 = __shfl_xor(bi, d);
    if (b2 < best || (b2 == best && i2 < bi)) { best = b2; bi = i2; }
  }
  const int k = __builtin_amdgcn_readfirstlane(bi);
  long_fence();                                           // (A is overwritten by z below: every lane has read it)
  // ---- 3c. eigenvector from the twist row outwards (staged like 3a: lane 0 downwards from row k, lane 1 upwards)
  //   downwards: z_t = -e_{t+1} z_{t+1} / D+_t;  upwards: z_t = -e_t z_{t-1} / D-_t
  {
    const int dsel = lane & 1;
    const double* xe = lds + dsel * 3 * kVecChunk; double* xz = lds + dsel * 3 * kVecChunk + 2 * kVecChunk;
    const int steps_dn = k, steps_up = n - 1 - k;
    const int smax = steps_dn > steps_up ? steps_dn : steps_up;
    double z = 1.0;
    if (lane == 0) A[k] = 1.0;
    for (int c0 = 0; c0 < smax; c0 += kVecChunk) {
      const int md = steps_dn - c0 < 0 ? 0 : (steps_dn - c0 < kVecChunk ? steps_dn - c0 : kVecChunk);
      const int mu = steps_up - c0 < 0 ? 0 : (steps_up - c0 < kVecChunk ? steps_up - c0 : kVecChunk);
      for (int i = lane; i < kVecChunk; i += kWave) {
        if (i < md) { const int t = k - 1 - (c0 + i); lds[i] = -src.e(t + 1, ih2) / Dp[t]; }        // z_t / z_{t+1}: formed by all lanes,
        if (i < mu) { const int t = k + 1 + (c0 + i); lds[3 * kVecChunk + i] = -src.e(t, ih2) / Dm[t]; } // the chain is one product per row
      }
      wave_lds_sync();
      if (lane < 2) {
        const int m = dsel ? mu : md;
        for (int i0 = 0; i0 < m; i0 += 8) {
          double rv[8], zv[8];
#pragma unroll
          for (int u = 0; u < 8; ++u) rv[u] = xe[i0 + u < m ? i0 + u : m - 1];
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            if (i0 + u < m) z *= rv[u];
            zv[u] = z;
          }
#pragma unroll
          for (int u = 0; u < 8; ++u) if (i0 + u < m) xz[i0 + u] = zv[u];
        }
      }
      wave_lds_sync();
      for (int i = lane; i < kVecChunk; i += kWave) {
        if (i < md) A[k - 1 - (c0 + i)] = lds[2 * kVecChunk + i];
        if (i < mu) A[k + 1 + (c0 + i)] = lds[5 * kVecChunk + i];
      }
      wave_lds_sync();
    }
  }
  long_fence();
  // ---- 4. growth rate (utils.py:1601-1621; the arithmetic of finish() in ibs_kernels.hip)
  double m = 0.0;
  for (int r = lane; r < n; r += kWave) m = xmax(m, xabs(A[r]));
  m = uniform(wave_max(m));
  if constexpr (SIGNED) {
    double mp = -1e300;                                     // the largest signed entry: m itself iff the largest |z| is positive
    for (int r = lane; r < n; r += kWave) mp = xmax(mp, A[r]);
    mp = uniform(wave_max(mp));
    m = mp == m ? m : -m;
  }
  const double rm = 1.0 / m;
  auto Xat = [&](int j) { return (j <= 0 || j >= N - 1) ? 0.0 : A[j - 1] * rm; };     // utils.py:1605, 1607-1608
  const double ih = 1.0 / h;
  const double A_in = (2.0 / 3.0) * ih, B_in = -ih / 12.0, A_e1 = 0.5 * ih, A_e0 = 2.0 * ih, B_e0 = -0.5 * ih;
  double y0 = 0.0, y1 = 0.0;
  for (int j0 = 0; j0 < N; j0 += kWave) {
    const int j = j0 + lane;
    const bool in = j < N;
    const int jc = in ? j : N - 1;
    const int jm1 = jc > 0 ? jc - 1 : 0, jm2 = jc > 1 ? jc - 2 : 0;
    const int jp1 = jc < N - 1 ? jc + 1 : N - 1, jp2 = jc < N - 2 ? jc + 2 : N - 1;
    const double X = Xat(jc);
    const double d1 = Xat(jp1) - Xat(jm1), d2 = Xat(jp2) - Xat(jm2);
    const bool end0 = (jc == 0) || (jc == N - 1), end1 = (jc == 1) || (jc == N - 2);
    const double Ac = end0 ? A_e0 : (end1 ? A_e1 : A_in), Bc = end0 ? B_e0 : (end1 ? 0.0 : B_in);
    const double dX = xfma(Ac, d1, Bc * d2);                                       // utils.py:1610-1616
    const double w = in ? (end0 ? 1.0 : ((jc & 1) ? 4.0 : 2.0)) : 0.0;             // Simpson weights (the 1/3 cancels)
    const double X2 = w * (X * X), dX2 = w * (dX * dX);
    y0 += src.c(jc) * X2 - src.g(jc) * dX2;                                        // utils.py:1618
    y1 = xfma(src.f(jc), X2, y1);                                                  // utils.py:1619
    if (X_out && in) X_out[sys * N + j] = (TI)X;
    if (dX_out && in) dX_out[sys * N + j] = (TI)dX;
  }
  y0 = wave_sum(y0); y1 = wave_sum(y1);
  return y0 / y1;                                                                  // utils.py:1621
}

}  // namespace ibs
