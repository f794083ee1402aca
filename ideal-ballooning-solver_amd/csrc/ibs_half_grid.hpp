// The half-grid row of the pencil, e_{j+1} = 0.5 * (g_j + g_{j+1}) / h^2 (utils.py:1574-1576), with its rounding written down.
// Plain C++ on both sides, so that the host can check it (tests/test_half_grid_cpu.py).
//
// Where g is a product (the geometry-fed sources: g = a1 * d, d the theta0 fold of gds2 / gds21 / gds22) the sum g_j + g_{j+1}
// adds two products, and a compiler that contracts takes ONE of them into an fma -- which one is its own choice, made from the
// use counts in the basic block, and it decides the last bit of e, of D and Ph, and of the diagonal scaling s.  Set-up, the
// rebuild of s in assemble() and the sub-wave solver all have to agree on it, so it is fixed here instead:
//
//   chunk point p = grid point a + p of a lane whose rows start at a (WaveSolver::rows_start), p = 0 .. M + 1, M rows per lane.
//   mean k lies between chunk points k and k + 1, k = 0 .. M:  mean k = 0.5 * fma(a1_F, d_F, g_R), g_R = the rounded a1_R * d_R.
//   k = 0:  F = 0, R = 1.
//   k >= 1: R is the point of the pair whose parity is M's, F the other one -- counted down from the top of the chunk, every
//           second point (M, M - 2, ...) is rounded once and that value enters the means on both sides of it, the points between
//           (M + 1, M - 1, ...) never form their product for a mean.  With M even, point 1 is rounded in mean 0 and fused in mean 1.
//
// This is what the gfx950 listings of set-up held at every rows-per-lane value M = 1 .. 32, in the one-wave and the sub-wave
// solver alike, before the rule was written down (tools/half_grid_pattern.py reads it off a listing), so D, Ph, the bounds and
// every shift are bit for bit what they were.
// Where g is a stored value (raw rows) there is nothing to contract in the mean, 0.5 * (g_lo + g_hi): half_grid_mean_plain() for
// the host check; the device code of those sources keeps its expression where it was.
//
// Contraction is off inside the helpers: every fma here is a __builtin_fma and nothing else becomes one.  half_grid_e() is the
// whole row, mean / h^2, and what the host check runs.  The device callers (HalfGridWalk in ibs_wave.hpp) take the mean from
// here and multiply by 1 / h^2 at the call site, set-up and assemble() alike: in set-up that product also feeds the diagonal
// c - (e_lo + e_hi) and the Gershgorin norm, into which the compiler contracts it, and a product formed in here -- or merged
// by common-subexpression elimination with one formed in here, which leaves the intersection of the two sets of flags -- could
// not be; D, Ph and the bounds would move.  The rounded value of that product is the same either way, so s is.
#pragma once

// (always inlined: the device code is to be what it would be with these bodies written out at the call)
#if defined(__HIPCC__) || defined(__CUDACC__)
#define IBS_HG_HD __host__ __device__ __attribute__((always_inline))
#else
#define IBS_HG_HD __attribute__((always_inline))
#endif

namespace ibs {

IBS_HG_HD inline double half_grid_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }
IBS_HG_HD inline float half_grid_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }

// of mean k of a chunk of M rows, the chunk point that goes into the fma: true = the lower one (k), false = the upper one (k + 1)
IBS_HG_HD constexpr bool half_grid_fuses_lower(int k, int M) { return k == 0 || ((k ^ M) & 1) != 0; }

// g of a rounded chunk point: the one product
template <typename T>
IBS_HG_HD inline T half_grid_product(T a1, T d) {
#pragma clang fp contract(off)
  return a1 * d;
}

// mean of a product g (the factors of point F of the pair) and a rounded g (point R)
template <typename T>
IBS_HG_HD inline T half_grid_mean_fused(T a1_f, T d_f, T g_r) {
#pragma clang fp contract(off)
  return T(0.5) * half_grid_fma(a1_f, d_f, g_r);
}

// mean k of a chunk of M rows from the factors of both points
template <typename T>
IBS_HG_HD inline T half_grid_mean(int k, int M, T a1_lo, T d_lo, T a1_hi, T d_hi) {
  return half_grid_fuses_lower(k, M) ? half_grid_mean_fused(a1_lo, d_lo, half_grid_product(a1_hi, d_hi))
                                  : half_grid_mean_fused(a1_hi, d_hi, half_grid_product(a1_lo, d_lo));
}

// mean of two stored values
template <typename T>
IBS_HG_HD inline T half_grid_mean_plain(T g_lo, T g_hi) {
#pragma clang fp contract(off)
  return T(0.5) * (g_lo + g_hi);
}

// e = mean / h^2 as one rounded product (ih2 = 1 / (h * h))
template <typename T>
IBS_HG_HD inline T half_grid_scale(T mean, T ih2) {
#pragma clang fp contract(off)
  return mean * ih2;
}
template <typename T>
IBS_HG_HD inline T half_grid_e(int k, int M, T a1_lo, T d_lo, T a1_hi, T d_hi, T ih2) {
  return half_grid_scale(half_grid_mean(k, M, a1_lo, d_lo, a1_hi, d_hi), ih2);
}

}  // namespace ibs
