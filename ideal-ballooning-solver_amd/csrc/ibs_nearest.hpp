// The solve of one system for the eigenpair nearest a shift (the stages listed in ibs_nearest.hip's header): shared by
// k_solve_gcf_nearest (ibs_nearest.hip: rows in memory) and the geometry-fed point kernels of ibs_nearest_grad.hip.
#pragma once
#include "ibs_long.hpp"

namespace ibs {

// Outputs at index sys of the given arrays (each optional; X / dX at sys * N); returns gam, NaN where status bits 0-1 are set
// or no growth rate was wanted (wave-uniform).
template <bool HAS_GH>
__device__ __forceinline__ double solve_nearest_one(const SrcLong<double, HAS_GH>& src, int N, double h, double s_in, long sys, double* work,
                                                    double* lam_out, int* idx_out, double* gam_out, double* X_out, double* dX_out,
                                                    int* info_out, double* lds) {
  const int lane = threadIdx.x & 63;
  const int n = N - 2;
  const double ih2 = 1.0 / (h * h);
  const double s = uniform(s_in);
  const LongBounds b = long_bounds<true>(src, N, ih2, lane);
  int status = 0, passes = 0, idx = 0;
  double lam = __builtin_nan("");
  if (b.bad || !finite_of(s)) {
    status = 2;
  } else {
    auto count = [&](double sig) { return count_above_chunked(src, n, ih2, sig, lds, lane); };
    const double tau = 4.0 * (double)N * Eps<double>::v * b.normA;
    // (s beyond the spectrum: the counts at s are the same as at the bound, and the multisections start from finite brackets)
    const double sc = xmax(b.lmin, xmin(b.hi, s));
    const int k = __builtin_amdgcn_readfirstlane(count(sc));
    ++passes;
    if (k == 0) {
      int p = 0;
      if (!long_lam_max(src, N, ih2, b.lo, b.hi, b.normA, lds, lane, lam, p)) status = 1;
      passes += p;
    } else {
      double lk = 0.0;
      int p = 0;
      if (!multisect_k<double>(count, k, sc, b.hi, b.normA, 2.0, lane, lk, p)) status = 1;
      passes += p;
      lam = lk; idx = k - 1;
      const double delta = lk - s;
      if (status == 0 && k < n) {
        const double lo2 = s - delta - tau;
        const int k2 = __builtin_amdgcn_readfirstlane(count(lo2));
        ++passes;
        if (k2 != k) {                                      // an eigenvalue below s within delta + tau: lam_{k+1}
          double lk1 = 0.0;
          if (!multisect_k<double>(count, k + 1, lo2, sc, b.normA, 2.0, lane, lk1, p)) status = 1;
          passes += p;
          const double d1 = delta, d2 = s - lk1;
          if (xabs(d1 - d2) < tau) status |= 32;            // (undecided: the larger one, lam_k, stays)
          else if (d2 < d1) { lam = lk1; idx = k; }
        }
      }
    }
  }
  double gam = __builtin_nan("");
  if ((gam_out || X_out || dX_out) && (status & 3) == 0)
    gam = long_vector_growth<true, double>(src, N, h, lam, sys, work, X_out, dX_out, lds, lane);
  if (lane == 0) {
    if (lam_out) lam_out[sys] = lam;
    if (idx_out) idx_out[sys] = (status & 3) ? -1 : idx;
    if (gam_out) gam_out[sys] = gam;
    if (info_out) info_out[sys] = (passes & 0xffff) | (status << 16);
  }
  return gam;
}

}  // namespace ibs
