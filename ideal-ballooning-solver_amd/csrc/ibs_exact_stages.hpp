// The solver-side stages k_exact_points (ibs_exact_grad.hip) and k_exact_tangent_points (ibs_exact_tangent.hip) share: the eigenpair
// of the rows in the wave's workspace, the adjoint d gam / d (g, c, f) and the lane-0 outputs.  What differs between the two kernels
// -- the lines they read and the contraction of the cotangent rows with the tangents -- stays written out in each.
// my = the wave's workspace, carved by L = exact_points_ws(N); its scalars: lam of lane 0, then the solve's word and the adjoint's.
#pragma once
#include "ibs_nearest.hpp"
#include "ibs_vjp.hpp"
#include "ibs_launch.hpp"

namespace ibs {

struct ExactPair { double gam, lam; int word, idx; };       // word: bits 0-15 passes, status from bit 16

// NEAREST: solve_nearest_one at sigma[p] (utils.py:1597); else lam_max as k_solve_gcf_long takes it.  X stays in the workspace,
// fenced on return.  A failed solve (status bits 0-1) leaves gam = NaN
template <bool NEAREST>
__device__ __forceinline__ ExactPair exact_eigenpair(const SrcLong<double, false>& src, const ExactPointsArgs& a, long p, double* my,
                                                     const ExactPointsWs& L, double* lds, int lane) {
  const int N = a.N;
  double* Xw = my + L.X;
  ExactPair e{__builtin_nan(""), __builtin_nan(""), 0, -1};
  if constexpr (NEAREST) {
    double* s_lam = my + L.scal;                             // scalars of lane 0, read back by the wave behind a fence
    int* s_info = reinterpret_cast<int*>(my + L.scal + 1);
    e.gam = solve_nearest_one<false>(src, N, a.h, a.sigma[p], 0, my + L.work, s_lam, a.idx ? a.idx + p : nullptr, nullptr, Xw, nullptr,
                                     s_info, lds);
    long_fence();                                           // (X of every lane, lam and the word of lane 0)
    e.lam = uniform(s_lam[0]);
    e.word = __builtin_amdgcn_readfirstlane(s_info[0]);
  } else {
    const double ih2 = 1.0 / (a.h * a.h);
    const LongBounds b = long_bounds<false>(src, N, ih2, lane);
    int status = 0, passes = 0;
    if (b.bad) status = 2;
    else if (!long_lam_max(src, N, ih2, b.lo, b.hi, b.normA, lds, lane, e.lam, passes)) status = 1;
    if (status == 0) {
      e.gam = long_vector_growth<false, double>(src, N, a.h, e.lam, 0, my + L.work, Xw, (double*)nullptr, lds, lane);
      e.idx = 0;
    }
    if (status == 2) e.lam = __builtin_nan("");           // (status 1: lam is where the multisection stopped, as solve_long_one leaves it)
    e.word = passes | (status << 16);
    long_fence();                                           // (X of every lane)
  }
  return e;
}

// vjp_one with gam_bar = gbar (1 unless given), lam_bar = 0 on the rows and the pair: g_bar, c_bar, f_bar in the workspace (g_bar and c_bar in the adjoint's
// own first two work rows, dead by then), fenced on return.  Returns the adjoint's status (bit 0 a replaced pivot: informational,
// bit 1 refused: no gradient) and merges it into e.word at status bits 6-7
__device__ __forceinline__ int exact_adjoint(const SrcLong<double, false>& src, const ExactPointsArgs& a, ExactPair& e, double* my,
                                             const ExactPointsWs& L, double* lds, int lane, double gbar = 1.0) {
  int* s_info = reinterpret_cast<int*>(my + L.scal + 1);
  vjp_one(src, a.N, a.h, e.lam, my + L.X, gbar, 0.0, my + L.gb, my + L.cb, my + L.fb, s_info + 1, 0, my + L.work, lds, lane);
  long_fence();                                             // (the cotangent rows of every lane, the adjoint's word of lane 0)
  const int vw = __builtin_amdgcn_readfirstlane(s_info[1]) >> 16;
  e.word |= (vw & 3) << (16 + 6);
  return vw;
}

// lane 0: val = -gam, jac = (-dgam/dalpha, -dgam/dtheta0) (utils.py:1728); optional gam, lam, idx, info
template <bool NEAREST>
__device__ __forceinline__ void exact_store(const ExactPointsArgs& a, long p, const ExactPair& e, double ja, double jt) {
  a.val[p] = -e.gam; a.jac[2 * p] = -ja; a.jac[2 * p + 1] = -jt;
  if (a.gam) a.gam[p] = e.gam;
  if (a.lam) a.lam[p] = e.lam;
  if (!NEAREST && a.idx) a.idx[p] = e.idx;
  if (a.info) a.info[p] = e.word;
}

}  // namespace ibs
