// The marginal-stability solve of one system (the stages listed in ibs_marginal.hip's header): shared by k_marginal_gcf (rows in
// memory) and k_marginal_scan (rows formed from the geometry at theta0).  Composed from the long-grid pieces of ibs_long.hpp.
#pragma once
#include "ibs_long.hpp"

namespace ibs {

// T(s) = s C - D presented to count_above_chunked, which forms d_r - sig f_r with d_r = c_r - D_rr: c = 0 in the diagonal and the
// role of f taken by c, so that the count at sig = -s is the number of positive eigenvalues of -D + s C.
struct SrcMargCount {
  static constexpr bool kHasGh = false;
  const double* gg; const double* cg;
  __device__ __forceinline__ double g(int j) const { return gg[j]; }
  __device__ __forceinline__ double c(int) const { return 0.0; }
  __device__ __forceinline__ double f(int j) const { return cg[j]; }
  __device__ __forceinline__ double e(int k, double ih2) const { return 0.5 * (gg[k] + gg[k + 1]) * ih2; }
};
// T(s*) presented to long_vector_growth at lam = 0: c -> s* c, f -> 1
struct SrcMargVec {
  static constexpr bool kHasGh = false;
  const double* gg; const double* cg; double s;
  __device__ __forceinline__ double g(int j) const { return gg[j]; }
  __device__ __forceinline__ double c(int j) const { return s * cg[j]; }
  __device__ __forceinline__ double f(int) const { return 1.0; }
  __device__ __forceinline__ double e(int k, double ih2) const { return 0.5 * (gg[k] + gg[k + 1]) * ih2; }
};

// ---- 1. bounds and data checks (lanes strided over the rows; the results are wave-uniform)
//   upper: a rigorous upper bound of s* = min x'Dx / x'Cx over x'Cx > 0 -- the unit vectors (D_jj / c_j over the rows with c_j > 0)
//          and the trial vectors sin^p(pi j / (N - 1)), p = 1, 4, 16, 64, of long_bounds, those with x'Cx > 0; x'Dx is summed as
//          sum_k e_k (x_{k+1} - x_k)^2 (the row form x_j (D x)_j cancels to N^2 eps), and the bound carries the rounding of the sums
//   any_pos: some c_j > 0 (else no s makes T(s) indefinite: s* = +inf);  bad: invalid data (non-finite entry or g <= 0; c of any sign)
struct MargBounds { double upper; bool any_pos, bad; };
__device__ __forceinline__ MargBounds marginal_bounds(const double* G, const double* C, int N, double ih2, int lane) {
  const int n = N - 2;
  double vup = -1e300;                                        // (-upper: wave_max reduces it)
  double tn[4] = {0.0, 0.0, 0.0, 0.0}, td[4] = {0.0, 0.0, 0.0, 0.0};
  bool bad = false, pos = false;
  const double dth = 3.141592653589793 / (double)(N - 1);
  double sdl, cdl;
  sincos(dth, &sdl, &cdl);
  for (int r = lane; r < n; r += kWave) {
    const int j = r + 1;
    const double gm = G[j - 1], g0 = G[j], gp = G[j + 1];
    const double e_lo = 0.5 * (gm + g0) * ih2, e_hi = 0.5 * (g0 + gp) * ih2;
    const double D = e_lo + e_hi, cj = C[j];
    bad = bad || !(g0 > 0.0) || !(e_lo > 0.0) || !(e_hi > 0.0) || !finite_of(cj) || !finite_of(D);
    if (cj > 0.0) { pos = true; vup = xmax(vup, -(D / cj)); }
    double sj, cjs;
    sincos(dth * (double)j, &sj, &cjs);
    double xm = sj * cdl - cjs * sdl, x0 = sj;                // sin at j - 1, j
    xm = j == 1 ? 0.0 : xm;
    const double e_end = j == N - 2 ? e_hi : 0.0;             // the last row also owns the cell to the zero end point
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const double dm = x0 - xm;
      tn[k] = xfma(e_lo * dm, dm, xfma(e_end * x0, x0, tn[k]));
      td[k] = xfma(cj * x0, x0, td[k]);
      xm *= xm; xm *= xm; x0 *= x0; x0 *= x0;                 // p -> 4 p
    }
  }
  if (lane == 0) bad = bad || !(G[0] > 0.0) || !(G[N - 1] > 0.0);
  MargBounds b;
  double up = -uniform(wave_max(vup));
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double a = wave_sum(tn[k]), bb = wave_sum(td[k]);
    const double q = a / bb;
    up = (bb > 0.0 && finite_of(q) && q > 0.0 && q < up) ? q : up;
  }
  b.upper = uniform(up) * (1.0 + (8.0 + 0.5 * (double)N) * Eps<double>::v);
  b.bad = __any(bad) != 0;
  b.any_pos = __any(pos) != 0 && finite_of(b.upper);
  return b;
}

// ---- 2. s* = inf { s > 0 : count(s) >= 1 } by 64-way multisection from [0, hi] (lane 0 at lo, lane 63 at hi).  lam_max(T(s)) is
// convex in s and negative at 0, so count >= 1 holds exactly above s*; the count itself is not monotone in s (C is indefinite) and
// only this predicate steers.  Each pass keeps the interval between the LOWEST scale that reports >= 1 and the scale below it: in a
// bracket a few ulp wide the predicate is noisy, and lanes above the first hit are never looked at, so the result stays inside the
// bracket that was valid.  A bracket that misses is moved and widened 64-fold, as multisect does.  Ends at width <= 8 eps s.
// passes: sweeps used; returns false if 24 passes did not close.
template <class CountF>
__device__ __forceinline__ bool marginal_multisect(CountF&& count, double hi, int lane, double& s, int& passes) {
  double lo = 0.0;
  bool ok = false;
  passes = 0;
  while (passes < 24) {
    ++passes;
    const double w = hi - lo;
    const double sc = lane == kWave - 1 ? hi : xfma((double)lane * (1.0 / 63.0), w, lo);
    const int cnt = count(sc);
    const unsigned long long m = __builtin_amdgcn_ballot_w64(cnt >= 1);
    if (m == 0ull) { lo = hi; hi = hi + 64.0 * w; continue; }                      // s* >= hi
    if (m & 1ull) { hi = lo; lo = xmax(0.0, lo - 64.0 * w); continue; }             // s* < lo
    const int first = __builtin_ctzll(m);                                           // the lowest scale with a positive eigenvalue
    lo = readlane_t(sc, first - 1); hi = readlane_t(sc, first);
    if (!(hi - lo > 8.0 * Eps<double>::v * hi)) { ok = true; break; }
  }
  s = 0.5 * (lo + hi);
  return ok;
}

// ---- 1-3 of one system with rows G, C (N entries each): returns s* (NaN: invalid data; +inf: no c_j > 0), wave-uniform.
// status (as in include/ibs.h): bit 0 = the multisection did not close, bit 1 = invalid data, bit 8 = s* infinite (informational).
// want_vec: the marginal mode -- X (N entries, zero ends, largest entry +1) to Xw and its FD4 / Simpson quotient to gam0 -- where
// status is 0; work = nearest_ws_doubles(N) doubles.  Xw is written by all lanes and fenced on return.
__device__ __forceinline__ double marginal_one(const double* G, const double* C, int N, double h, double* work, double* Xw, bool want_vec,
                                               double* lds, int& status, int& passes, double& gam0) {
  const int lane = threadIdx.x & 63;
  const int n = N - 2;
  const double ih2 = 1.0 / (h * h);
  const MargBounds b = marginal_bounds(G, C, N, ih2, lane);
  status = 0; passes = 0;
  gam0 = __builtin_nan("");
  double s = __builtin_nan("");
  if (b.bad) {
    status = 2;
  } else if (!b.any_pos) {
    status = 256;
    s = __builtin_inf();
  } else {
    const SrcMargCount sc{G, C};
    if (!marginal_multisect([&](double t) { return count_above_chunked(sc, n, ih2, -t, lds, lane); }, b.upper, lane, s, passes)) status = 1;
  }
  if (want_vec && status == 0) {
    const SrcMargVec sv{G, C, s};
    gam0 = long_vector_growth<false, double>(sv, N, h, 0.0, 0, work, Xw, static_cast<double*>(nullptr), lds, lane);
    long_fence();
  }
  return s;
}

// ---- 4: the weight of g_j in the pencil's quadratic form, w_j = (X_j - X_{j-1})^2 + (X_{j+1} - X_j)^2 (the end rows have one cell):
// d s* / d g_j = 1/2 h^-2 w_j / q
__device__ __forceinline__ double pencil_weight(const double* Xw, int j, int N) {
  const double x0 = Xw[j];
  const double dm = j > 0 ? x0 - Xw[j - 1] : 0.0, dp = j < N - 1 ? Xw[j + 1] - x0 : 0.0;
  return xfma(dm, dm, dp * dp);
}

// lane-0 outputs of the margin's point kernels (A = MarginalPointsArgs | MarginalTangentArgs): val = -mu = -1 / s*, jac = dscale / s*^2,
// scale, dscale = (dal, dth), dPdrho = -mdP, info.  A failed solve (s NaN or status bit 0): every floating-point output NaN; status
// bit 8 (s* = +inf): val = 0, and dal = dth = 0 as the caller filled them
template <class A>
__device__ __forceinline__ void marginal_store(const A& a, long p, double s, int status, int passes, double dal, double dth, double mdP) {
  const bool failed = s != s || (status & 1);               // (the centre solve: iteration cap or invalid data)
  if (failed) s = __builtin_nan("");
  const double rs = 1.0 / s;                                // mu: 0 with s* = +inf
  a.val[p] = (status & 256) ? 0.0 : -rs;
  if (a.jac) { a.jac[2 * p] = dal * rs * rs; a.jac[2 * p + 1] = dth * rs * rs; }
  if (a.scale) a.scale[p] = s;
  if (a.dscale) { a.dscale[2 * p] = dal; a.dscale[2 * p + 1] = dth; }
  if (a.dPdrho) a.dPdrho[p] = failed ? __builtin_nan("") : -mdP;
  if (a.info) a.info[p] = passes | (status << 16);
}

}  // namespace ibs
