// Sign changes of a lane's forward solution, counted from ONE word of sign bits: the integer part of the resident solver's forward
// sweep (WaveSolver<T, M, true>::sweep_fwd_min2 in ibs_wave.hpp).  Plain C++ on both sides, so that the host can check it
// against the row-by-row rule of WaveSolver::sweep_fwd (tests/test_sweep_count_cpu.py).
//
// The word: a lane shifts in, one bit each and in this order, the signs of u_-1 and u_0 (the incoming pair, as the scan delivers
// it) and of z_1 .. z_M (row i of the lane's chunk forms z_{i+1} from z_i and z_{i-1}; z_0 = u_0).  So bit M + 1 is the sign of
// u_-1, bit M that of u_0, bit M - 1 - i that of the value row i forms, and the transition INTO bit k -- from the value shifted in
// just before it -- is bit k of w ^ (w >> 1):
//   bit M          the incoming pair (u_-1 -> u_0),
//   bit M - 1 - i  row i (z_i -> z_{i+1}).
// Bit M + 1 of w ^ (w >> 1) compares u_-1 with nothing and is never owned.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define IBS_SC_HD __host__ __device__
#else
#define IBS_SC_HD
#endif

namespace ibs {

// The transitions a lane owns (WaveSolver::sweep_fwd): its incoming pair and the rows i < ncount,
//   ncount = (rows the lane holds: M with has_last, else M - 1) - (1, unless it is the last lane of the wave)
// -- the step out of a lane's last row belongs to the next lane, which counts it from ITS incoming pair; only the last lane
// counts its final step, into the shooting value.  ncount >= M - 2, so sweep_fwd's `i < M - 2 || i < ncount` is `i < ncount`.
// Loop-invariant: formed once per solve.
IBS_SC_HD inline unsigned sweep_count_mask(int M, bool has_last, bool last_lane) {
  const int ncount = (has_last ? M : M - 1) - (last_lane ? 0 : 1);
  return ((2u << ncount) - 1u) << (M - ncount);          // bits M - ncount .. M
}

// sign changes this lane owns: the word of M + 2 sign bits (anything above bit M + 1 is ignored with it) and the lane's mask
IBS_SC_HD inline int sweep_count_lane(unsigned w, unsigned mask, int M) {
  (void)M;                                               // (the mask ends at bit M: nothing above it has to be cleared first)
  return __builtin_popcount((w ^ (w >> 1)) & mask);
}

// What the shift iteration asks of the wave's count C = sum of the lanes' counts -- C == 0, C != 0, C == 1 -- from two ballots:
// b1 = lanes with c != 0, b2 = lanes with c > 1.  Returns min(C, 2), NOT the count.
IBS_SC_HD inline int sweep_count_min2(unsigned long long b1, unsigned long long b2) {
  if (b1 == 0ull) return 0;
  return (__builtin_popcountll(b1) == 1 && b2 == 0ull) ? 1 : 2;       // one lane, and that lane with one change
}

}  // namespace ibs
