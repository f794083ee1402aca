// Spectrum mode with an F-orthonormal Ritz basis of every cluster of modes (ibs_solve_gcf_modes_basis_f64).  Stages 1-3 are those of
// k_solve_gcf_modes (ibs_modes.hip), statement for statement: bounds, simultaneous multisection, the cluster probe -- lam, the pass
// count and status bits 0, 1 and 9 are that kernel's bits.  Stage 4:
//   * a mode outside every cluster: the same long_vector_growth<true> call, hence the same bits in gam, X and dX;
//   * a cluster (modes_partition, ibs_modes_basis.hpp: a run of linked modes, or the last mode alone where the probe found the
//     cluster to continue below it): the header's construction, run by the wave.  The member vectors live in the caller's X rows
//     (hence X is required; no row of N doubles per member enters the workspace), the elimination's five rows in the per-wave
//     workspace, the m x m matrices of the Ritz step in the LDS the counts have left.  Sums and maxima run on the DPP ladders of
//     ibs_wave.hpp in their fixed order; nothing is accumulated by atomics: the results are bitwise repeatable and do not depend on
//     the system's place in the batch.  Members get status bit 13, those of an open cluster bit 14 as well; a member whose vector
//     was refused gets bit 0 and NaN in gam, X and dX, its lam stays.
// A cluster with a member whose bracket did not close (status bit 0 of the multisection) is left to the per-mode path.
// Per-wave workspace: basis_ws_doubles(N) (ibs_launch.hpp).
#include "ibs_long.hpp"
#include "ibs_modes.hpp"
#include "ibs_modes_basis.hpp"
#include "ibs_launch.hpp"

namespace ibs {

// the 64 (shift, count) pairs of a pass, as modes_tighten reads them (the wave of ibs_modes.hip)
struct BasisCountWave {
  double sig; int cnt;
  __device__ __forceinline__ unsigned long long inside_ge(double lo, double hi, int k) const {
    return __builtin_amdgcn_ballot_w64(sig > lo && sig < hi && cnt >= k);
  }
  __device__ __forceinline__ unsigned long long inside_lt(double lo, double hi, int k) const {
    return __builtin_amdgcn_ballot_w64(sig > lo && sig < hi && cnt < k);
  }
  __device__ __forceinline__ double shift(int lane) const { return readlane_t(sig, lane); }
};

// the wave of ibs_modes_basis.hpp: the rows of one system, the X / dX rows of one cluster's members
template <bool HAS_GH>
struct BasisWave {
  SrcLong<double, HAS_GH> src;
  int n_pts, ln; double step, ih2;
  double* X; double* dX;      // member 0's rows; dX null: the derivative goes to work row 0 (free once the solves are done)
  double* work; double* sm;
  __device__ __forceinline__ int lane() const { return ln; }
  __device__ __forceinline__ int lanes() const { return kWave; }
  __device__ __forceinline__ double sum(double v) const { return wave_sum(v); }
  __device__ __forceinline__ double max(double v) const { return wave_max(v); }
  __device__ __forceinline__ double bcast(double v, int l) const { return readlane_t(v, l); }
  __device__ __forceinline__ void sync() const { long_fence(); }      // (agent scope: orders the LDS accesses of the wave as well)
  __device__ __forceinline__ int N() const { return n_pts; }
  __device__ __forceinline__ double h() const { return step; }
  __device__ __forceinline__ double g(int j) const { return src.g(j); }
  __device__ __forceinline__ double c(int j) const { return src.c(j); }
  __device__ __forceinline__ double f(int j) const { return src.f(j); }
  __device__ __forceinline__ double e(int k) const { return src.e(k, ih2); }
  __device__ __forceinline__ double& x(int i, int j) const { return X[(size_t)i * n_pts + j]; }
  __device__ __forceinline__ double& dx(int i, int j) const { return dX ? dX[(size_t)i * n_pts + j] : work[j]; }
  __device__ __forceinline__ double& ws(int k, int r) const { return work[(size_t)k * n_pts + r]; }
  __device__ __forceinline__ double* small() const { return sm; }
};

template <bool HAS_GH>
__global__ void __launch_bounds__(64) k_solve_gcf_modes_basis(long n_sys, int N, double h, const double* __restrict__ g,
                                                              const double* __restrict__ c, const double* __restrict__ f,
                                                              const double* __restrict__ gh, long ld, int K, double* lam_out,
                                                              double* gam_out, double* X_out, double* dX_out, int* first_out,
                                                              int* info_out, double* work) {
  __shared__ double lds[3 * kLongChunk];                    // (the LDS budget of the long path: static_assert at kLongChunk)
  static_assert(sizeof(lds) * 8 <= 160 * 1024, "eight blocks per CU");
  static_assert(kBasisSmallDoubles <= 3 * kLongChunk, "the Ritz step's matrices fit the LDS of the counts");
  const int lane = threadIdx.x & 63;
  const int n = N - 2;
  const double ih2 = 1.0 / (h * h);
  double* my = work + (size_t)blockIdx.x * basis_ws_doubles(N);
  double* lam_ws = my + basis_rows_doubles(N);
  double* gam_ws = lam_ws + kMaxModes;
  int* st_ws = reinterpret_cast<int*>(gam_ws + kMaxModes);
  int* cf_ws = st_ws + kMaxModes;                           // cluster_first, then the open flag
  for (long sys = blockIdx.x; sys < n_sys; sys += gridDim.x) {
    const SrcLong<double, HAS_GH> src{g + sys * ld, c + sys * ld, f + sys * ld, HAS_GH ? gh + sys * ld : nullptr};
    const LongBounds b = long_bounds<true>(src, N, ih2, lane);
    int passes = 0;
    double tau = 0.0;
    if (!b.bad) {
      const double stop = 2.0 * Eps<double>::v * b.normA;
      tau = 4.0 * (double)N * Eps<double>::v * b.normA;
      ModesBrackets br;
      modes_init(br, K, b.lmin, b.hi);
      BasisCountWave w{0.0, 0};
      while (passes < kModesPassCap && modes_lane_shift(br, stop, lane, w.sig)) {
        w.cnt = count_above_chunked(src, n, ih2, w.sig, lds, lane);
        ++passes;
        modes_tighten(br, stop, w);
      }
      int probe = -1;
      if (modes_all_closed(br, stop)) {
        probe = __builtin_amdgcn_readfirstlane(count_above_chunked(src, n, ih2, modes_probe_shift(br, tau), lds, lane));
        ++passes;
      }
      if (lane == 0) {
        modes_finish(br, stop, tau, probe, lam_ws, st_ws);
        cf_ws[kMaxModes] = modes_partition(lam_ws, K, tau, probe, cf_ws) ? 1 : 0;
      }
      long_fence();
    }
    const bool open_last = !b.bad && __builtin_amdgcn_readfirstlane(cf_ws[kMaxModes]) != 0;
    for (int m0 = 0; m0 < K;) {
      // the group of mode m0: the modes of its cluster, or m0 alone
      int m = 1, st_any = b.bad ? 2 : __builtin_amdgcn_readfirstlane(st_ws[m0]);
      if (!b.bad)
        while (m0 + m < K && __builtin_amdgcn_readfirstlane(cf_ws[m0 + m]) == m0) { st_any |= __builtin_amdgcn_readfirstlane(st_ws[m0 + m]); ++m; }
      const bool open = open_last && m0 + m == K;
      const long o0 = sys * K + m0;
      if ((m > 1 || open) && (st_any & 3) == 0) {
        BasisWave<HAS_GH> bw{src, N, lane, h, ih2, X_out + o0 * N, dX_out ? dX_out + o0 * N : nullptr, my, lds};
        const unsigned found = modes_cluster_basis(bw, m, lam_ws + m0, b.normA, tau, gam_ws);
        long_fence();
        for (int i = 0; i < m; ++i) {
          const bool ok = (found >> i) & 1u;
          if (!ok)
            for (int j = lane; j < N; j += kWave) {
              X_out[(o0 + i) * N + j] = __builtin_nan("");
              if (dX_out) dX_out[(o0 + i) * N + j] = __builtin_nan("");
            }
          if (lane == 0) {
            const int status = __builtin_amdgcn_readfirstlane(st_ws[m0 + i]) | (ok ? 1 << kModesBasisBit : 1) | (open ? 1 << kModesOpenBit : 0);
            if (lam_out) lam_out[o0 + i] = lam_ws[m0 + i];
            if (gam_out) gam_out[o0 + i] = ok ? gam_ws[i] : __builtin_nan("");
            if (first_out) first_out[o0 + i] = m0;
            if (info_out) info_out[o0 + i] = (passes & 0xffff) | (status << 16);
          }
        }
      } else {
        for (int i = 0; i < m; ++i) {                       // the per-mode path of k_solve_gcf_modes
          const long o = o0 + i;
          const double lam = b.bad ? __builtin_nan("") : uniform(lam_ws[m0 + i]);
          const int status = b.bad ? 2 : __builtin_amdgcn_readfirstlane(st_ws[m0 + i]);
          double gam = __builtin_nan("");
          if ((status & 3) == 0) {
            gam = long_vector_growth<true, double>(src, N, h, lam, o, my, X_out, dX_out, lds, lane);
          } else {
            for (int j = lane; j < N; j += kWave) {
              X_out[o * N + j] = __builtin_nan("");
              if (dX_out) dX_out[o * N + j] = __builtin_nan("");
            }
          }
          if (lane == 0) {
            if (lam_out) lam_out[o] = lam;
            if (gam_out) gam_out[o] = gam;
            if (first_out) first_out[o] = b.bad ? m0 + i : __builtin_amdgcn_readfirstlane(cf_ws[m0 + i]);
            if (info_out) info_out[o] = (passes & 0xffff) | (status << 16);
          }
        }
      }
      m0 += m;
    }
    long_fence();                                           // (the workspace is reused by this wave's next system)
  }
}

hipError_t launch_gcf_modes_basis(const ModesBasisArgs& a, hipStream_t st) {
  if (a.n_sys <= 0) return hipSuccess;
  if (a.n_modes < 1 || a.n_modes > kMaxModes || !a.X) return hipErrorInvalidValue;
  const long grid = persistent_grid(a.n_sys, a.n_waves, a.work, a.work_doubles, basis_ws_doubles(a.N));
  if (!grid) return hipErrorInvalidValue;
  if (a.gh) {
    hipLaunchKernelGGL(k_solve_gcf_modes_basis<true>, dim3((unsigned)grid), dim3(64), 0, st, a.n_sys, a.N, a.h, a.g, a.c, a.f, a.gh, a.ld,
                       a.n_modes, a.lam, a.gam, a.X, a.dX, a.cluster_first, a.info, a.work);
    note_launch(grid, 64, "ibs::k_solve_gcf_modes_basis<true>");
  } else {
    hipLaunchKernelGGL(k_solve_gcf_modes_basis<false>, dim3((unsigned)grid), dim3(64), 0, st, a.n_sys, a.N, a.h, a.g, a.c, a.f, a.gh, a.ld,
                       a.n_modes, a.lam, a.gam, a.X, a.dX, a.cluster_first, a.info, a.work);
    note_launch(grid, 64, "ibs::k_solve_gcf_modes_basis<false>");
  }
  return hipGetLastError();
}

}  // namespace ibs
