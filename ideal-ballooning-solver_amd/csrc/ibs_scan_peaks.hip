// k_scan_peaks: the K best peaks of every surface's coarse (alpha, theta0) table and the refinement's starts from them, on the
// device (ibs_scan_peaks_f64).  The rule and its bookkeeping are ibs_scan_peaks.hpp's; this file is the block's way through it.
//
// One block per surface, blockDim a multiple of 64.  Thread t owns entries t, t + blockDim, ...: it reads each with its up to eight
// neighbours once (the table is a few KB and stays in L2) and keeps the peak predicate of its first 64 entries as one bit each; a
// table beyond 64 * blockDim entries forms the predicate of the later ones again in every round.  Round r: every thread offers its
// peaks that rank strictly after the pick of round r - 1, a wave reduces them with the (value, index) ladder of wave_argmax_first,
// the waves' winners meet in LDS (double-buffered by the round's parity: one barrier per round) and every thread ends the round
// with the same pick, which is the next round's threshold.  No list of peaks, no atomics but the one n_bad add, a fixed order of
// comparisons that are selects of whole pairs: the bits of a surface's result do not depend on the other surfaces, on the number
// of blocks or on the block size.  The loop ends for all threads at once (the pick is block-uniform) and no thread returns before
// the last ladder, so every DPP step runs with all 64 lanes.
#include <hip/hip_runtime.h>
#include "ibs_launch.hpp"
#include "ibs_wave.hpp"
#include "ibs_scan_peaks.hpp"

namespace ibs {

__global__ void __launch_bounds__(256) k_scan_peaks(ScanPeaksArgs a) {
  __shared__ double sv[2][4];
  __shared__ int si[2][4];
  __shared__ double pv[kMaxStarts];      // the picks, in rank order: written and read by thread 0 alone
  __shared__ int pi[kMaxStarts];
  const int na = a.n_alpha, nt = a.n_theta0, n_per = na * nt;
  const double* g = a.gam + (size_t)blockIdx.x * n_per;
  unsigned long long mask = 0;
  {
    int e = 0;
    for (int i = threadIdx.x; i < n_per && e < 64; i += blockDim.x, ++e)
      mask |= (unsigned long long)peaks_is_peak(g, na, nt, i) << e;
  }
  const int w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  double tv = HUGE_VAL;
  int ti = -1, n_picks = 0;
  for (int r = 0; r < a.n_starts; ++r) {
    double bv = -HUGE_VAL;
    int bi = kPeaksNoIndex;
    int e = 0;
    for (int i = threadIdx.x; i < n_per; i += blockDim.x, ++e) {
      const bool pk = e < 64 ? (bool)((mask >> e) & 1ull) : peaks_is_peak(g, na, nt, i);
      if (pk) peaks_offer(g[i], i, tv, ti, bv, bi);
    }
    wave_argmax_first(bv, bi);
    if (nw > 1) {                        // (one wave per surface when the table has at most 64 entries: no LDS round trip, no barrier)
      const int b = r & 1;
      if ((threadIdx.x & 63) == 0) { sv[b][w] = bv; si[b][w] = bi; }
      __syncthreads();
      bv = sv[b][0]; bi = si[b][0];
      for (int k = 1; k < nw; ++k) {
        const double v2 = sv[b][k];
        const int i2 = si[b][k];
        const bool take = peaks_beats(v2, i2, bv, bi);
        bv = take ? v2 : bv; bi = take ? i2 : bi;
      }
    }
    if (bi == kPeaksNoIndex) break;      // no peak is left: block-uniform
    if (threadIdx.x == 0) { pv[n_picks] = bv; pi[n_picks] = bi; }
    tv = bv; ti = bi; ++n_picks;
  }
  if (threadIdx.x == 0) {
    const size_t s = blockIdx.x, K = (size_t)a.n_starts;
    const bool bad = peaks_finish(a.n_starts, n_picks, pv, pi, na, nt, a.alpha, a.theta0, a.start + 2 * s * K, a.peak + s * K,
                                  a.index ? a.index + s * K : nullptr, a.sigma0 ? a.sigma0 + s * K : nullptr,
                                  a.n_found ? a.n_found + s : nullptr);
    if (bad) atomicAdd(a.n_bad, 1);      // a NaN / flagged table: reported once per surface (k_scan_starts)
  }
}

hipError_t launch_scan_peaks(const ScanPeaksArgs& a, int threads, hipStream_t st) {
  hipLaunchKernelGGL(k_scan_peaks, dim3((unsigned)a.n_surf), dim3((unsigned)threads), 0, st, a);
  return hipGetLastError();
}

}  // namespace ibs
