// Local-equilibrium scan: gam, lam_max and the Sturm count at a shift of every (line, variation) system, a variation being a triple
// (theta0, relative change of the surface's shear, factor on its pressure gradient) applied to the line's eight arrays by the rule of
// ibs_local_eq.hpp -- the s-alpha diagram of a real field line from ONE staged line, no geometry launch per shear value.  FP64, every odd
// N in [66, 65,537], one wavefront per system on the persistent grid of the long path, division form throughout (ibs_long.hpp):
//   0. rows          the wave forms its system's g, c, f rows from the line (lane-strided, coalesced loads of the eight arrays and the ps
//                    row) into its workspace; the line's dPdrho, centre, sigma and the triple are read once per system, wave-uniformly
//   1. bounds        long_bounds on the rows: bracket of lam_max, ||A||, data checks
//   2. count         count_above_chunked at `shift`, where the count is requested
//   3. eigenvalue    long_lam_max, where gam or lam is requested
//   4. growth rate   long_vector_growth, where gam is requested
// With the count alone requested stages 3-4 are skipped: the stable / unstable diagram costs one pass over the rows per system.
// Status 2 (NaN outputs, count -1): a line with non-finite data, sigma not +-1, a non-finite triple -- of those systems only.  No
// atomics; a system's outputs depend on its line and its triple alone.
// Per-wave workspace: local_eq_ws(N) (ibs_local_eq.hpp), in global memory.
#include "ibs_local_eq.hpp"
#include "ibs_geo_line.hpp"
#include "ibs_long.hpp"

namespace ibs {

__global__ void __launch_bounds__(64) k_local_eq_scan(const LocalEqArgs a) {
  __shared__ double lds[3 * kLongChunk];
  static_assert(sizeof(lds) * 8 <= 160 * 1024, "eight blocks per CU");
  const int lane = threadIdx.x & 63;
  const int N = a.N;
  const LocalEqWs L = local_eq_ws(N);
  double* my = a.work + (size_t)blockIdx.x * L.total;
  double* G = my + L.g; double* C = my + L.c; double* F = my + L.f;
  const bool want_lam = a.gam || a.lam;                     // (kernel-uniform)
  const double ih2 = 1.0 / (a.h * a.h);
  const long n_sys = (long)a.n_lines * a.n_var;
  for (long sys = blockIdx.x; sys < n_sys; sys += gridDim.x) {
    const int line = (int)(sys / a.n_var), iv = (int)(sys - (long)line * a.n_var);
    const double dP = uniform(a.dPdrho[line]), thc = uniform(a.centre[line]), sg = uniform(a.sigma[line]);
    const double th0 = uniform(a.var[3 * (long)iv]), eps = uniform(a.var[3 * (long)iv + 1]), p = uniform(a.var[3 * (long)iv + 2]);
    const LocalEqFold v = local_eq_fold_of(dP, sg, th0, eps, p);
    const GeoLine ln{a.geo + (long)line * a.ld, (long)a.plane};
    const double* ps = a.ps ? a.ps + (long)line * a.ps_ld : nullptr;
    // ---- 0. the rows of the variation
    bool bad = !(xabs(sg) == 1.0) || !finite_of(dP) || !finite_of(thc) || !finite_of(th0) || !finite_of(eps) || !finite_of(p);
    for (int j = lane; j < N; j += kWave) {
      const double dth = xfma((double)j, a.h, a.theta_lo) - thc;
      double g, c, f;
      local_eq_gcf(ln, j, v, dth, ps ? ps[j] : 0.0, g, c, f);
      bad = bad || !finite_of(g) || !finite_of(c) || !finite_of(f);      // (long_bounds looks at the inner rows only)
      G[j] = g; C[j] = c; F[j] = f;
    }
    long_fence();                                           // (rows written by every lane, read by every lane below)
    const SrcLong<double, false> src{G, C, F, nullptr};
    // ---- 1. bounds and data checks
    const LongBounds b = long_bounds<false>(src, N, ih2, lane);
    int status = (__any(bad) || b.bad) ? 2 : 0, passes = 0, cnt = -1;
    double lam = __builtin_nan(""), gam = __builtin_nan("");
    if (status == 0) {
      // ---- 2. eigenvalues above the shift (every lane the same shift)
      if (a.count) cnt = count_above_chunked(src, N - 2, ih2, a.shift, lds, lane);
      // ---- 3-4. lam_max and its growth rate
      if (want_lam) {
        if (!long_lam_max(src, N, ih2, b.lo, b.hi, b.normA, lds, lane, lam, passes)) status = 1;
        else if (a.gam)
          gam = long_vector_growth<false, double>(src, N, a.h, lam, 0, my + L.work, static_cast<double*>(nullptr),
                                                  static_cast<double*>(nullptr), lds, lane);
      }
    }
    if (lane == 0) {
      if (a.gam) a.gam[sys] = gam;
      if (a.lam) a.lam[sys] = lam;
      if (a.count) a.count[sys] = cnt;
      if (a.info) a.info[sys] = passes | (status << 16);
    }
    long_fence();                                           // (the workspace is reused by this wave's next system)
  }
}

hipError_t launch_local_eq_scan(const LocalEqArgs& a, hipStream_t st) {
  const long n_sys = (long)a.n_lines * a.n_var;
  if (n_sys <= 0) return hipSuccess;
  const long grid = persistent_grid(n_sys, a.n_waves, a.work, a.work_doubles, local_eq_ws(a.N).total);
  if (!grid || !a.geo || !a.dPdrho || !a.centre || !a.sigma || !a.var || !(a.gam || a.lam || a.count)) return hipErrorInvalidValue;
  if (a.ld < a.N || (a.ps && a.ps_ld < a.N) || a.plane < (size_t)a.n_lines * (size_t)a.ld) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_local_eq_scan, dim3((unsigned)grid), dim3(64), 0, st, a);
  note_launch(grid, 64, "ibs::k_local_eq_scan");
  return hipGetLastError();
}

}  // namespace ibs
