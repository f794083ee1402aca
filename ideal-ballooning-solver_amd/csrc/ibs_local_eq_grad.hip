// Local-equilibrium gradients: lam_max, gam and the exact derivatives of lam_max at points (line, theta0, eps, p) of the rule of
// ibs_local_eq.hpp (the formulas: ibs_local_eq_grad.hpp).  FP64, every odd N in [66, 65,537], one wavefront per point on the persistent
// grid of the long path, division form throughout (ibs_long.hpp): k_local_eq_scan's stages with the mode kept, then stages 4-5 of
// k_marginal_tangent_points for this pencil.
//   0. rows          local_eq_gcf of the point's line at its triple into the wave's workspace, exactly as k_local_eq_scan
//   1. bounds        long_bounds on the rows: bracket of lam_max, ||A||, data checks
//   2. eigenvalue    long_lam_max
//   3. mode          long_vector_growth with X kept in the wave's workspace; gam comes from the same call.  With dlam and geo_bar both
//                    null no mode is kept: lam and gam are k_local_eq_scan's bits at that line and triple
//   4. derivatives   the five Hellmann-Feynman sums and q, the tangents formed as they are summed: lane-strided partial sums, then the
//                    wave reduction -- a fixed order, no atomics
//   5. geo_bar       the eight cotangent planes in closed form per grid point; each lane writes its own points j = lane, lane + 64, ...
//                    with vector stores; entries N .. ld_bar-1 are never written
// Status bit 0 (iteration cap) or 1 (non-finite data, g or f <= 0, sigma not +-1, a non-finite triple, line_of outside [0, n_lines)): NaN
// in every floating-point output of that point, entries 0 .. N-1 of its geo_bar rows included; the line of a point whose index is out
// of range is never read.  A point's outputs depend on the point and its line alone, bit for bit.
// Per-wave workspace: local_eq_grad_ws(N) (ibs_local_eq_grad.hpp), in global memory.
#include "ibs_local_eq_grad.hpp"
#include "ibs_geo_line.hpp"
#include "ibs_long.hpp"
#include "ibs_marginal.hpp"

namespace ibs {

__global__ void __launch_bounds__(64) k_local_eq_grad(const LocalEqGradArgs a) {
  __shared__ double lds[3 * kLongChunk];
  static_assert(sizeof(lds) * 8 <= 160 * 1024, "eight blocks per CU");
  const int lane = threadIdx.x & 63;
  const int N = a.N;
  const LocalEqGradWs L = local_eq_grad_ws(N);
  double* my = a.work + (size_t)blockIdx.x * L.total;
  double* G = my + L.rows.g; double* C = my + L.rows.c; double* F = my + L.rows.f; double* Xw = my + L.X;
  const bool want_mode = a.dlam || a.geo_bar;               // (kernel-uniform)
  const bool want_vec = want_mode || a.gam;
  const double ih2 = 1.0 / (a.h * a.h);
  const double nan = __builtin_nan("");
  for (long pt = blockIdx.x; pt < a.n_pts; pt += gridDim.x) {
    const int line = __builtin_amdgcn_readfirstlane(a.line_of[pt]);
    const double th0 = uniform(a.var[3 * pt]), eps = uniform(a.var[3 * pt + 1]), p = uniform(a.var[3 * pt + 2]);
    int status = 2, passes = 0;
    double lam = nan, gam = nan, d0 = nan, d1 = nan, d2 = nan, d3 = nan, q = 1.0;
    double dP = 0.0, thc = 0.0, sg = 0.0;
    LocalEqFold v{};
    GeoLine ln{a.geo, (long)a.plane};
    const double* ps = nullptr;
    if (line >= 0 && line < a.n_lines) {                    // (wave-uniform; else the point names no line and nothing of geo is read)
      dP = uniform(a.dPdrho[line]); thc = uniform(a.centre[line]); sg = uniform(a.sigma[line]);
      v = local_eq_fold_of(dP, sg, th0, eps, p);
      ln = GeoLine{a.geo + (long)line * a.ld, (long)a.plane};
      ps = a.ps ? a.ps + (long)line * a.ps_ld : nullptr;
      // ---- 0. the rows of the point
      bool bad = !(xabs(sg) == 1.0) || !finite_of(dP) || !finite_of(thc) || !finite_of(th0) || !finite_of(eps) || !finite_of(p);
      for (int j = lane; j < N; j += kWave) {
        const double dth = xfma((double)j, a.h, a.theta_lo) - thc;
        double g, c, f;
        local_eq_gcf(ln, j, v, dth, ps ? ps[j] : 0.0, g, c, f);
        bad = bad || !finite_of(g) || !finite_of(c) || !finite_of(f);      // (long_bounds looks at the inner rows only)
        G[j] = g; C[j] = c; F[j] = f;
      }
      long_fence();                                         // (rows written by every lane, read by every lane below)
      const SrcLong<double, false> src{G, C, F, nullptr};
      // ---- 1. bounds and data checks
      const LongBounds b = long_bounds<false>(src, N, ih2, lane);
      status = (__any(bad) || b.bad) ? 2 : 0;
      if (status == 0) {
        // ---- 2-3. lam_max, its mode and its growth rate
        if (!long_lam_max(src, N, ih2, b.lo, b.hi, b.normA, lds, lane, lam, passes)) { status = 1; lam = nan; }
        else if (want_vec) {
          gam = long_vector_growth<false, double>(src, N, a.h, lam, 0, my + L.rows.work, want_mode ? Xw : static_cast<double*>(nullptr),
                                                  static_cast<double*>(nullptr), lds, lane);
          long_fence();                                     // (X of every lane)
        }
      }
    }
    const bool ok = status == 0;
    // ---- 4. the derivatives
    if (want_mode && ok) {
      double sK = 0.0, sKd = 0.0, sKp = 0.0, sP = 0.0, sD = 0.0;
      q = 0.0;
      for (int j = lane; j < N; j += kWave) {
        const double x0 = Xw[j], x2 = x0 * x0, w = pencil_weight(Xw, j, N);
        const double B = ln.at(0, j), gp = xabs(ln.at(1, j)), gb = ln.at(7, j);
        const double dth = xfma((double)j, a.h, a.theta_lo) - thc, psj = ps ? ps[j] : 0.0;
        const double x = xfma(v.pm1, psj, xfma(v.xs, dth, v.x0));
        const double cmg = ln.at(2, j) - gb, pcg = v.p * cmg, cv0 = ln.at(3, j);
        const double cv = xfma(x, cv0, xfma(v.p, cmg, gb));                        // cv' of the rule
        const double inv = 1.0 / (gp * B);
        const double Wc = x2 * inv, Wg = gp / B * w, Wf = x2 / (B * B) * inv;
        const double K = xfma(2.0 * xfma(x, ln.at(6, j), ln.at(5, j)), -(xfma(0.5 * ih2, Wg, lam * Wf)), v.mdP * cv0 * Wc);
        q = xfma(F[j], x2, q);
        sK += K; sKd = xfma(K, dth, sKd); sKp = xfma(K, psj, sKp);
        sP = xfma(cv + pcg, Wc, sP); sD = xfma(cv, Wc, sD);
      }
      q = wave_sum(q); sK = wave_sum(sK); sKd = wave_sum(sKd); sKp = wave_sum(sKp); sP = wave_sum(sP); sD = wave_sum(sD);
      d0 = (1.0 + eps) * sK / q;
      d1 = xfma(th0, sK, sg * sKd) / q;
      d2 = xfma(-dP, sP, sKp) / q;
      d3 = -(p * sD) / q;
    }
    // ---- 5. the cotangent planes
    if (a.geo_bar) {
      double* gbp = a.geo_bar + (size_t)pt * a.ld_bar;
      const long pb = (long)a.plane_bar;
      if (!ok) {
        for (int j = lane; j < N; j += kWave) {
#pragma unroll
          for (int k = 0; k < 8; ++k) gbp[(long)k * pb + j] = nan;
        }
      } else {
        const double iq = 1.0 / q;
        for (int j = lane; j < N; j += kWave) {
          const double x0 = Xw[j], x2 = x0 * x0 * iq, w = pencil_weight(Xw, j, N);
          const double gbar = -0.5 * ih2 * w * iq, cbar = x2, fbar = -lam * x2;
          const double B = ln.at(0, j), gpr = ln.at(1, j), gp = xabs(gpr);
          const double iB = 1.0 / B, ia = 1.0 / gp;
          const double dth = xfma((double)j, a.h, a.theta_lo) - thc, psj = ps ? ps[j] : 0.0;
          const double x = xfma(v.pm1, psj, xfma(v.xs, dth, v.x0));
          const double gg = gbar * G[j], cc = cbar * C[j], ff = fbar * F[j];
          const double gdb = xfma(gbar * gp, iB, fbar * (iB * iB * iB) * ia);      // gd_bar
          const double cvb = v.mdP * cbar * ia * iB;                               // cv_bar
          const double dgp = (gg - cc - ff) * ia;
          gbp[j] = -(gg + cc + 3.0 * ff) * iB;
          gbp[1 * pb + j] = gpr < 0.0 ? -dgp : dgp;
          gbp[2 * pb + j] = v.p * cvb;
          gbp[3 * pb + j] = x * cvb;
          gbp[4 * pb + j] = gdb;
          gbp[5 * pb + j] = (2.0 * x) * gdb;
          gbp[6 * pb + j] = (x * x) * gdb;
          gbp[7 * pb + j] = -v.pm1 * cvb;
        }
      }
    }
    // ---- outputs
    if (lane == 0) {
      if (a.lam) a.lam[pt] = lam;
      if (a.gam) a.gam[pt] = gam;
      if (a.dlam) { a.dlam[4 * pt] = d0; a.dlam[4 * pt + 1] = d1; a.dlam[4 * pt + 2] = d2; a.dlam[4 * pt + 3] = d3; }
      if (a.info) a.info[pt] = passes | (status << 16);
    }
    long_fence();                                           // (the workspace is reused by this wave's next point)
  }
}

hipError_t launch_local_eq_grad(const LocalEqGradArgs& a, hipStream_t st) {
  if (a.n_pts <= 0) return hipSuccess;
  const long grid = persistent_grid(a.n_pts, a.n_waves, a.work, a.work_doubles, local_eq_grad_ws(a.N).total);
  if (!grid || !a.line_of || !a.var || !(a.lam || a.gam || a.dlam || a.geo_bar)) return hipErrorInvalidValue;
  if (a.n_lines > 0 && (!a.geo || !a.dPdrho || !a.centre || !a.sigma)) return hipErrorInvalidValue;
  if (a.n_lines < 0 || a.ld < a.N || (a.ps && a.ps_ld < a.N) || a.plane < (size_t)a.n_lines * (size_t)a.ld) return hipErrorInvalidValue;
  if (a.geo_bar && (a.ld_bar < a.N || a.plane_bar < (size_t)a.ld_bar)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_local_eq_grad, dim3((unsigned)grid), dim3(64), 0, st, a);
  note_launch(grid, 64, "ibs::k_local_eq_grad");
  return hipGetLastError();
}

}  // namespace ibs
