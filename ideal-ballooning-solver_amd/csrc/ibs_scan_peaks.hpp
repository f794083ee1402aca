// The K best local maxima ("peaks") of one coarse (alpha, theta0) table, as the starts of a multi-start refinement.  Slot 0 is the
// first maximum with the start and shift of ball_scan.py:279-295 (what k_scan_starts gives); slots >= 1 have no upstream counterpart.
//
// The rule (ibs_amd.scan.pick_starts restates it in numpy and is the oracle of everything here):
//   beats    a neighbour w of entry v beats it if w > v, or w == v and w has the smaller row-major index.  A NaN never beats anything
//            (both comparisons are false).
//   peak     an entry that is not NaN and that none of its up to eight neighbours (i +- 1, j +- 1) inside the table beats.  No
//            wrap-around in either direction: alpha in [0, pi] and theta0 in [0, pi / 2] are a box, as in the refinement's bounds.
//   ranking  peaks by value descending, ties by index ascending: the first maximum of the table is always peak 0.
//   rounds   round r picks the best peak that ranks strictly after the pick of round r - 1: the previous pick is the threshold and no
//            list of peaks is kept.  A round without a candidate ends the selection.
//   slots    peaks_finish: slot k < n_found starts at its peak's node with sigma0 = 1.3 |peak| + 0.05; a first maximum of exactly 0
//            starts at (0, 0) with sigma0 = 0.05 (ball_scan.py:279-282), one that is not finite (or a table without a peak: all NaN)
//            is reported (n_bad) and starts at (0, 0); both give n_found = 0.  Slots from n_found on repeat slot 0.
//
// Plain C++ on both sides: k_scan_peaks (ibs_scan_peaks.hip) walks the entries with a block and reduces a round with wave ladders,
// peaks_select_serial below does the same with one loop -- tests/test_scan_peaks_cpu.py runs it against written-out tables.
#pragma once
#include <cmath>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define IBS_PK_HD __host__ __device__
#else
#define IBS_PK_HD
#endif

namespace ibs {

constexpr int kMaxStarts = 16;
constexpr int kPeaksNoIndex = 0x7fffffff;        // the index of "no candidate" (its value: -inf): every real candidate beats it

// (no short circuit: selects, not branches -- the rule of wave_argmax_first, ibs_wave.hpp)
IBS_PK_HD inline bool peaks_beats(double w, int iw, double v, int iv) { return (w > v) | ((w == v) & (iw < iv)); }

IBS_PK_HD inline bool peaks_is_peak(const double* tab, int n_alpha, int n_theta0, int idx) {
  const double v = tab[idx];
  const int i = idx / n_theta0, j = idx - i * n_theta0;
  bool beaten = !(v == v);
  for (int di = -1; di <= 1; ++di)
    for (int dj = -1; dj <= 1; ++dj) {
      const int ii = i + di, jj = j + dj;
      if ((di == 0 && dj == 0) || ii < 0 || ii >= n_alpha || jj < 0 || jj >= n_theta0) continue;
      const int k = ii * n_theta0 + jj;
      beaten |= peaks_beats(tab[k], k, v, idx);
    }
  return !beaten;
}

// (v, i) ranks strictly after the pick (pv, pi) of the round before; the first round's threshold is (+inf, -1)
IBS_PK_HD inline bool peaks_ranks_after(double v, int i, double pv, int pi) { return (v < pv) | ((v == pv) & (i > pi)); }

// a peak (v, i) is offered to a round whose best so far is (bv, bi)
IBS_PK_HD inline void peaks_offer(double v, int i, double pv, int pi, double& bv, int& bi) {
  const bool take = peaks_ranks_after(v, i, pv, pi) & peaks_beats(v, i, bv, bi);
  bv = take ? v : bv; bi = take ? i : bi;
}

// upstream's shift of a start, ball_scan.py:289, 295: 1.3 * abs(gam) + 0.05 as Python rounds it -- the product, then the sum
// (the device compiler contracts a * b + c into one fused multiply-add unless told not to -- also through __dmul_rn / __dadd_rn,
// which are plain operators there)
IBS_PK_HD inline double peaks_sigma0(double gam) {
#if defined(__clang__)
#pragma clang fp contract(off)
  const double p = 1.3 * std::fabs(gam);
#else
  const volatile double p = 1.3 * std::fabs(gam);
#endif
  return p + 0.05;
}

// The slots of one surface from the n_picks <= n_starts picks (pv, pi) of the rounds, in rank order.  start [n_starts][2], peak
// [n_starts]; index [n_starts] (-1 where the start is no node of the table), sigma0 [n_starts] and n_found optional.  Returns true
// when the surface counts in n_bad.
IBS_PK_HD inline bool peaks_finish(int n_starts, int n_picks, const double* pv, const int* pi, int n_alpha, int n_theta0,
                                   const double* alpha, const double* theta0, double* start, double* peak, int* index,
                                   double* sigma0, int* n_found) {
  (void)n_alpha;
  const double m = n_picks > 0 ? pv[0] : __builtin_nan("");
  const bool ok = (m == m) && std::fabs(m) <= 1.7976931348623157e308;
  const bool node = ok && m != 0.0;
  const int nf = node ? n_picks : 0;
  for (int k = 0; k < n_starts; ++k) {
    const int src = k < nf ? k : 0;
    double a = 0.0, t = 0.0, sg = 0.05, val = m;                            // ball_scan.py:279-282: an all-zero table
    int ix = -1;
    if (node) {
      ix = pi[src]; val = pv[src];
      const int i = ix / n_theta0, j = ix - i * n_theta0;                   // row-major (ball_scan.py:283-288)
      a = alpha[i]; t = theta0[j]; sg = peaks_sigma0(val);
    }
    start[2 * k] = a; start[2 * k + 1] = t; peak[k] = val;
    if (index) index[k] = ix;
    if (sigma0) sigma0[k] = sg;
  }
  if (n_found) *n_found = nf;
  return !ok;
}

// The selection of one surface with one loop per round (the host's form of k_scan_peaks): fills pv, pi [n_starts], returns n_picks
inline int peaks_select_serial(const double* tab, int n_alpha, int n_theta0, int n_starts, double* pv, int* pi) {
  double tv = HUGE_VAL;
  int ti = -1, n = 0;
  for (int r = 0; r < n_starts; ++r) {
    double bv = -HUGE_VAL;
    int bi = kPeaksNoIndex;
    for (int e = 0; e < n_alpha * n_theta0; ++e)
      if (peaks_is_peak(tab, n_alpha, n_theta0, e)) peaks_offer(tab[e], e, tv, ti, bv, bi);
    if (bi == kPeaksNoIndex) break;
    pv[n] = tv = bv; pi[n] = ti = bi; ++n;
  }
  return n;
}

}  // namespace ibs
