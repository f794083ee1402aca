// The regrid of utils.py:1565-1576: a line given on ANY increasing theta_PEST grid is moved onto the uniform grid of the same end
// points before it is solved -- g, c, f by np.interp onto np.linspace(theta[0], theta[-1], N), g once more at the uniform half
// points, and h from that half grid.  Written down here with its rounding, in plain C++ on both sides, so that the host can check it
// against numpy (tests/test_regrid_cpu.py); the kernels of ibs_regrid.hip and the host side of the entry points run these bodies.
//
//   nodes        step = (hi - lo) / (N - 1), tu[j] = round(j * step) + lo, tu[N - 1] = hi: np.linspace (product and sum rounded
//                separately: contraction is off inside the helpers)
//   half nodes   0.5 * (tu[j] + tu[j + 1])                                   utils.py:1574
//   spacing      h = th_half[3] - th_half[2]                                 utils.py:1575, np.diff(th_half)[2]
//   interval     for a node x the k with xp[k] <= x < xp[k + 1], clamped to [0, N - 2]: a bisection on (lo = 0, hi = N - 1) that moves
//                lo only where x >= xp[mid] holds -- whatever the row holds (NaN, a decreasing pair, equal neighbours) the result stays
//                in [0, N - 2], so that an invalid grid can never index outside its rows
//   value        np.interp: fp[k] where x == xp[k], fp[N - 1] where x == xp[N - 1], else slope * (x - xp[k]) + fp[k] with
//                slope = (fp[k + 1] - fp[k]) / (xp[k + 1] - xp[k]): one difference, one quotient, one product and one sum
//   validity     a row is a grid when it is finite, strictly increasing and has theta[0] == lo and theta[N - 1] == hi
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define IBS_RG_HD __host__ __device__ __attribute__((always_inline))
#else
#define IBS_RG_HD __attribute__((always_inline))
#endif

namespace ibs {

// up to this length the theta row of a line is staged in LDS for the search (16.4 KB); beyond, it is searched in global memory
constexpr int kRegridLdsN = 2050;

IBS_RG_HD inline double regrid_step(double lo, double hi, int N) { return (hi - lo) / (double)(N - 1); }

// node j of np.linspace(lo, hi, N)
IBS_RG_HD inline double regrid_node(int j, int N, double lo, double hi, double step) {
#pragma clang fp contract(off)
  const double p = (double)j * step;
  return j == N - 1 ? hi : p + lo;
}

// half node j, between nodes j and j + 1 (j <= N - 2)
IBS_RG_HD inline double regrid_half_node(int j, int N, double lo, double hi, double step) {
#pragma clang fp contract(off)
  return 0.5 * (regrid_node(j, N, lo, hi, step) + regrid_node(j + 1, N, lo, hi, step));
}

// the spacing the solvers are handed (N >= 5)
IBS_RG_HD inline double regrid_spacing(int N, double lo, double hi) {
  const double step = regrid_step(lo, hi, N);
  return regrid_half_node(3, N, lo, hi, step) - regrid_half_node(2, N, lo, hi, step);
}

// the window every line of a call shares
IBS_RG_HD inline bool regrid_finite(double x) { return x - x == 0.0; }
IBS_RG_HD inline bool regrid_window_ok(double lo, double hi) { return regrid_finite(lo) && regrid_finite(hi) && hi > lo; }

// k in [0, N - 2] with xp[k] <= x < xp[k + 1] on a valid row (N >= 2); in that range on any row
template <class Row>
IBS_RG_HD inline int regrid_interval(const Row& xp, int N, double x) {
  int lo = 0, hi = N - 1;
  while (hi - lo > 1) {
    const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
    if (x >= xp[mid]) lo = mid; else hi = mid;
  }
  return lo;
}

// np.interp at x in interval k, from the end values of the interval (x0 = xp[k], x1 = xp[k + 1], f0 = fp[k], f1 = fp[k + 1]);
// k = N - 2 holds the last node, x == xp[N - 1], which takes fp[N - 1]
IBS_RG_HD inline double regrid_value(double x, double x0, double x1, double f0, double f1) {
#pragma clang fp contract(off)
  if (x == x0) return f0;
  if (x == x1) return f1;
  const double slope = (f1 - f0) / (x1 - x0);
  const double t = slope * (x - x0);
  return t + f0;
}

// one neighbouring pair of a valid row
IBS_RG_HD inline bool regrid_pair_ok(double a, double b) { return regrid_finite(a) && regrid_finite(b) && a < b; }

// the whole row (host side and tests; the kernels apply regrid_pair_ok across a block)
template <class Row>
IBS_RG_HD inline bool regrid_row_ok(const Row& xp, int N, double lo, double hi) {
  if (!(xp[0] == lo && xp[N - 1] == hi)) return false;
  for (int j = 0; j + 1 < N; ++j)
    if (!regrid_pair_ok(xp[j], xp[j + 1])) return false;
  return true;
}

}  // namespace ibs
