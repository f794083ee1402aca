// Geometry-fed points with the EXACT gradient of gam in BOTH variables, FP64, every odd N in [66, 65,537]: k_exact_points
// (ibs_exact_grad.hip) with the alpha-derivative of the rows taken from the alpha-tangent of the geometry
// (ibs_fieldline_geometry_dalpha_f64) in place of the reference's difference of two side lines over del_alpha (utils.py:1641-1646 /
// 1683-1718): ONE field line per point.  A sibling kernel on the same stage functions; k_exact_points itself is untouched.
// k_exact_tangent_points<NEAREST>, per point p (geo and geo_da in the [8][n_pts][ld] layout of the two geometry calls):
//   1. dPdrho      of the line, -1/2 mean((cvdrift - gbdrift) bmag^2) as a wave reduction (ball_scan.py:262); it has no alpha-tangent
//   2. rows        theta0 folded into the line and its (g, c, f) rows written to the wave's workspace
//   3. eigenpair   NEAREST: solve_nearest_one at sigma[p]; else lam_max as k_solve_gcf_long takes it
//   4. adjoint     vjp_one with gam_bar = 1, lam_bar = 0: g_bar, c_bar, f_bar in the workspace            (1-4: as k_exact_points)
//   5. contraction jac_theta0 = S(g_bar g_t + c_bar c_t + f_bar f_t) as k_exact_points; jac_alpha = S(g_bar g_a + c_bar c_a + f_bar f_a)
//                  with the tangent rows of line_gcf_tangent, formed from the two plane sets as they are summed
//   6. outputs     val = -gam, jac = (-dgam/dalpha, -dgam/dtheta0) (utils.py:1728); optional gam, lam, idx, info
// No floating-point atomics; every sum has a fixed order (lane-strided partial sums, then the DPP reduction).  Status word and
// workspace (exact_points_ws) as k_exact_points.  A non-finite entry of geo_da reaches jac[.][0] alone.
#include "ibs_nearest.hpp"
#include "ibs_vjp.hpp"
#include "ibs_geo_line.hpp"
#include "ibs_launch.hpp"

namespace ibs {

template <bool NEAREST>
__global__ void __launch_bounds__(64) k_exact_tangent_points(const ExactTangentArgs a) {
  __shared__ double lds[3 * kLongChunk];                    // (the LDS budget of the long path: static_assert at kLongChunk)
  static_assert(sizeof(lds) * 8 <= 160 * 1024, "eight blocks per CU");
  const int lane = threadIdx.x & 63;
  const int N = a.N;
  const ExactPointsWs L = exact_points_ws(N);
  double* my = a.work + (size_t)blockIdx.x * L.total;
  double* G = my + L.g; double* C = my + L.c; double* F = my + L.f; double* Xw = my + L.X;
  double* gb = my + L.gb; double* cb = my + L.cb; double* fb = my + L.fb;
  double* s_lam = my + L.scal;                               // scalars of lane 0, read back by the wave behind a fence
  int* s_info = reinterpret_cast<int*>(my + L.scal + 1);     // [0] the solve's word (NEAREST), [1] the adjoint's
  const long plane = (long)a.n_pts * a.ld;
  for (long p = blockIdx.x; p < a.n_pts; p += gridDim.x) {
    const double th0 = uniform(a.theta0[p]);
    const GeoLine ln{a.geo + (size_t)p * a.ld, plane}, lt{a.geo_da + (size_t)p * a.ld, plane};
    // ---- 1. dPdrho of the line
    double mdP;
    {
      double s = 0.0;
      for (int j = lane; j < N; j += kWave) {
        const double B = ln.at(0, j);
        s += (ln.at(2, j) - ln.at(7, j)) * B * B;
      }
      mdP = 0.5 * wave_sum(s) / (double)N;                  // -dPdrho
    }
    // ---- 2. the line's rows
    for (int j = lane; j < N; j += kWave) {
      double g, c, f;
      line_gcf(ln, j, mdP, th0, g, c, f);
      G[j] = g; C[j] = c; F[j] = f;
    }
    long_fence();                                           // (rows written by every lane, read by every lane below)
    const SrcLong<double, false> src{G, C, F, nullptr};
    // ---- 3. the eigenpair
    double gam = __builtin_nan(""), lam = __builtin_nan("");
    int word = 0, idx = -1;
    if constexpr (NEAREST) {
      gam = solve_nearest_one<false>(src, N, a.h, a.sigma[p], 0, my + L.work, s_lam, a.idx ? a.idx + p : nullptr, nullptr, Xw, nullptr,
                                     s_info, lds);
      long_fence();                                         // (X of every lane, lam and the word of lane 0)
      lam = uniform(s_lam[0]);
      word = __builtin_amdgcn_readfirstlane(s_info[0]);
    } else {
      const double ih2 = 1.0 / (a.h * a.h);
      const LongBounds b = long_bounds<false>(src, N, ih2, lane);
      int status = 0, passes = 0;
      if (b.bad) status = 2;
      else if (!long_lam_max(src, N, ih2, b.lo, b.hi, b.normA, lds, lane, lam, passes)) status = 1;
      if (status == 0) {
        gam = long_vector_growth<false, double>(src, N, a.h, lam, 0, my + L.work, Xw, (double*)nullptr, lds, lane);
        idx = 0;
      }
      if (status == 2) lam = __builtin_nan("");           // (status 1: lam is where the multisection stopped, as solve_long_one leaves it)
      word = passes | (status << 16);
      long_fence();                                         // (X of every lane)
    }
    // ---- 4. d gam / d (g, c, f)
    double ja = __builtin_nan(""), jt = __builtin_nan("");
    if (((word >> 16) & 3) == 0) {
      vjp_one(src, N, a.h, lam, Xw, 1.0, 0.0, gb, cb, fb, s_info + 1, 0, my + L.work, lds, lane);
      long_fence();                                         // (the cotangent rows of every lane, the adjoint's word of lane 0)
      const int vw = __builtin_amdgcn_readfirstlane(s_info[1]) >> 16;
      word |= (vw & 3) << (16 + 6);
      // ---- 5. contraction with the theta0 and alpha tangents
      if ((vw & 2) == 0) {
        double st = 0.0, sa = 0.0;
        for (int j = lane; j < N; j += kWave) {
          const double gbj = gb[j], cbj = cb[j], fbj = fb[j];
          // theta0 tangent of the line (utils.py:1669-1673)
          const double B = ln.at(0, j), gp = xabs(ln.at(1, j));
          const double inv = 1.0 / (gp * B);
          const double A1 = gp / B, A3 = inv / (B * B);
          const double dp = 2.0 * ln.at(5, j) + (2.0 * th0) * ln.at(6, j);
          const double gt = A1 * dp, ct = mdP * ln.at(3, j) * inv, ft = A3 * dp;
          // alpha tangent: the derivative of the rows, dPdrho fixed
          double ga, ca, fa;
          line_gcf_tangent(ln, lt, j, mdP, th0, ga, ca, fa);
          st += gbj * gt + cbj * ct + fbj * ft;
          sa += gbj * ga + cbj * ca + fbj * fa;
        }
        jt = wave_sum(st);
        ja = wave_sum(sa);
      }
    }
    // ---- 6. utils.py:1728
    if (lane == 0) {
      a.val[p] = -gam; a.jac[2 * p] = -ja; a.jac[2 * p + 1] = -jt;
      if (a.gam) a.gam[p] = gam;
      if (a.lam) a.lam[p] = lam;
      if (!NEAREST && a.idx) a.idx[p] = idx;
      if (a.info) a.info[p] = word;
    }
    long_fence();                                           // (the workspace is reused by this wave's next point)
  }
}

hipError_t launch_obj_w_grad_exact_tangent(const ExactTangentArgs& a, hipStream_t st) {
  if (a.n_pts <= 0) return hipSuccess;
  const long grid = a.n_pts < a.n_waves ? a.n_pts : a.n_waves;
  if (grid < 1 || !a.work || a.work_doubles < (size_t)grid * exact_points_ws(a.N).total) return hipErrorInvalidValue;
  if (!a.geo || !a.geo_da || !a.theta0 || !a.val || !a.jac) return hipErrorInvalidValue;
  if (a.sigma) {
    hipLaunchKernelGGL(k_exact_tangent_points<true>, dim3((unsigned)grid), dim3(64), 0, st, a);
    note_launch(grid, 64, "ibs::k_exact_tangent_points<true>");
  } else {
    hipLaunchKernelGGL(k_exact_tangent_points<false>, dim3((unsigned)grid), dim3(64), 0, st, a);
    note_launch(grid, 64, "ibs::k_exact_tangent_points<false>");
  }
  return hipGetLastError();
}

}  // namespace ibs
