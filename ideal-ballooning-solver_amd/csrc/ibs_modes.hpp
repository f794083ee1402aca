// The K largest eigenvalues of one system by SIMULTANEOUS multisection: one bracket per wanted mode m = 0 .. K-1 (mode m = the
// (m+1)-th largest eigenvalue), all refined by the same passes of 64 shifts.  K runs of multisect_k (ibs_wave.hpp) cost about nine
// passes each, a pass being n dependent divisions per lane; here a pass serves every mode at once.
//
// Invariant of a bracket: count(lo_m) >= m + 1 > count(hi_m), count(s) = the number of eigenvalues above s.  All brackets start at
// [lmin, hi] of long_bounds<true>.  One pass:
//   1. modes_lane_shift   the 64 lanes are shared out over the DISTINCT brackets still wider than `stop` (= 2 eps ||A||), as equally
//                         as 64 divides, lowest bracket first; inside its bracket a lane takes an interior, evenly spaced shift.  So
//                         the shifts ascend with the lane.  Brackets that have seen the same passes are identical or disjoint (they
//                         are cells of the partition the shifts so far have cut), and identical ones belong to consecutive modes.
//   2. the count at the lane's shift (device: count_above_chunked; host model: anything monotone)
//   3. modes_tighten      EVERY open bracket is tightened from all 64 (shift, count) pairs: the highest shift inside it with at
//                         least m + 1 eigenvalues above becomes lo_m, then the lowest shift above that with fewer becomes hi_m.
//                         Only shifts strictly inside a bracket touch it and hi_m is looked for above the new lo_m, so the invariant
//                         and lo_m < hi_m survive counts that are not monotone to the last ulp.
// modes_lane_shift returns false when no bracket is open: the pass before was the last.  kModesPassCap passes, then status bit 0.
// One more count, at lam_{K-1} - tau (modes_probe_shift), tells whether the first unwanted eigenvalue lies within tau of the last
// wanted one.  modes_finish: lam_m = the midpoint; adjacent modes less than tau = 4 N eps ||A|| apart (the probe included) form a
// cluster and carry the informational status bit kModesClusterBit: their lam hold to tau, their vectors are some vector of the
// cluster's invariant subspace.
//
// Plain C++ on both sides (tests/test_modes_bookkeeping_cpu.py runs it against exact counts of written-out spectra).  The wave is
// a template argument W with
//   unsigned long long inside_ge(double lo, double hi, int k)   lanes with lo < shift < hi and count >= k
//   unsigned long long inside_lt(double lo, double hi, int k)   lanes with lo < shift < hi and count <  k
//   double shift(int lane)
// -- two ballots and a readlane on the device (ibs_modes.hip), three loops on the host.
#pragma once
#include "ibs_plan.hpp"      // kMaxModes

#if defined(__HIPCC__) || defined(__CUDACC__)
#define IBS_MD_HD __host__ __device__
#define IBS_MD_UNROLL _Pragma("unroll")
#else
#define IBS_MD_HD
#define IBS_MD_UNROLL
#endif

namespace ibs {

constexpr int kModesPassCap = 32;
constexpr int kModesClusterBit = 9;      // status bit (include/ibs.h, conventions)

// (every loop over the modes runs to kMaxModes under a guard, fully unrolled: the arrays are indexed by constants and stay in registers)
struct ModesBrackets {
  int K;
  double lo[kMaxModes], hi[kMaxModes];
};

IBS_MD_HD inline void modes_init(ModesBrackets& b, int K, double lo, double hi) {
  b.K = K;
IBS_MD_UNROLL
  for (int m = 0; m < kMaxModes; ++m) { b.lo[m] = lo; b.hi[m] = hi; }
}

IBS_MD_HD inline bool modes_open(const ModesBrackets& b, int m, double stop) { return m < b.K && b.hi[m] - b.lo[m] > stop; }

// mode m's bracket is open and not the bracket of mode m + 1 as well: it takes a share of the lanes
IBS_MD_HD inline bool modes_takes_lanes(const ModesBrackets& b, int m, double stop) {
  if (!modes_open(b, m, stop)) return false;
  if (m + 1 >= b.K) return true;
  const int nx = m + 1 < kMaxModes ? m + 1 : m;            // (m + 1 < K <= kMaxModes here: the index is in range when it is read)
  return b.lo[m] != b.lo[nx] || b.hi[m] != b.hi[nx];
}

// the shift of `lane` in the next pass; false = every bracket is closed (sig is left alone)
IBS_MD_HD inline bool modes_lane_shift(const ModesBrackets& b, double stop, int lane, double& sig) {
  int D = 0;
IBS_MD_UNROLL
  for (int m = 0; m < kMaxModes; ++m) D += modes_takes_lanes(b, m, stop) ? 1 : 0;
  if (D == 0) return false;
  const int base = 64 / D, rem = 64 - base * D;
  int start = 0, bi = 0, j = 0, p = 1;
  double lo = 0.0, hi = 0.0;
IBS_MD_UNROLL
  for (int m = kMaxModes - 1; m >= 0; --m) {               // the lowest bracket first: the shifts ascend with the lane
    if (modes_takes_lanes(b, m, stop)) {
      const int pm = base + (bi < rem ? 1 : 0);
      if (lane >= start && lane < start + pm) { lo = b.lo[m]; hi = b.hi[m]; j = lane - start; p = pm; }
      start += pm; ++bi;
    }
  }
  sig = lo + (hi - lo) * ((double)(j + 1) / (double)(p + 1));
  return true;
}

template <class W>
IBS_MD_HD inline void modes_tighten(ModesBrackets& b, double stop, const W& w) {
IBS_MD_UNROLL
  for (int m = 0; m < kMaxModes; ++m) {
    if (modes_open(b, m, stop)) {
      double lo = b.lo[m];
      const double hi = b.hi[m];
      const unsigned long long ge = w.inside_ge(lo, hi, m + 1);
      if (ge) lo = w.shift(63 - __builtin_clzll(ge));
      const unsigned long long lt = w.inside_lt(lo, hi, m + 1);
      if (lt) b.hi[m] = w.shift(__builtin_ctzll(lt));
      b.lo[m] = lo;
    }
  }
}

IBS_MD_HD inline bool modes_all_closed(const ModesBrackets& b, double stop) {
  bool open = false;
IBS_MD_UNROLL
  for (int m = 0; m < kMaxModes; ++m) open = open || modes_open(b, m, stop);
  return !open;
}

// where the count tells whether eigenvalue K (the first unwanted one) lies within tau of mode K - 1
IBS_MD_HD inline double modes_probe_shift(const ModesBrackets& b, double tau) {
  double mid = 0.0;
IBS_MD_UNROLL
  for (int m = 0; m < kMaxModes; ++m) if (m == b.K - 1) mid = 0.5 * (b.lo[m] + b.hi[m]);
  return mid - tau;
}

// lam[K], status[K] (bit 0: the bracket did not close; bit kModesClusterBit: clustered).  probe_count: the count at
// modes_probe_shift, or -1 where it was not taken (a cap hit).
IBS_MD_HD inline void modes_finish(const ModesBrackets& b, double stop, double tau, int probe_count, double* lam, int* status) {
  double l[kMaxModes];
  int s[kMaxModes];
IBS_MD_UNROLL
  for (int m = 0; m < kMaxModes; ++m) { l[m] = 0.5 * (b.lo[m] + b.hi[m]); s[m] = modes_open(b, m, stop) ? 1 : 0; }
IBS_MD_UNROLL
  for (int m = 0; m + 1 < kMaxModes; ++m)
    if (m + 1 < b.K && l[m] - l[m + 1] < tau) { s[m] |= 1 << kModesClusterBit; s[m + 1] |= 1 << kModesClusterBit; }
IBS_MD_UNROLL
  for (int m = 0; m < kMaxModes; ++m) {
    if (m == b.K - 1 && probe_count > b.K) s[m] |= 1 << kModesClusterBit;
    if (m < b.K) { lam[m] = l[m]; status[m] = s[m]; }
  }
}

}  // namespace ibs
