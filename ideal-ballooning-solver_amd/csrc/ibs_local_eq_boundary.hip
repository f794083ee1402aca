// Local-equilibrium boundaries: the parameters t at which a field line crosses the stability boundary along rays (theta0, eps0 + t d_eps,
// p0 + t d_p) of the rule of ibs_local_eq.hpp, closed on the device.  FP64, every odd N in [66, 65,537], one wavefront per (line, ray) on
// the persistent grid of the long path; the 64 lanes are 64 values of t of ONE system.  The rule for a ray, the staged form (seven
// polynomial coefficients in t per grid point), the passes and the status bits: ibs_local_eq_boundary.hpp.
//   staging   a chunk of kBoundaryChunk grid points at a time, by all lanes: coalesced loads of the eight arrays and the ps row, the
//             t-invariant factors and the seven coefficients formed once per point, written to LDS point-major ([point][7])
//   chain     every lane walks the chunk: gt, c, f of its own t from the coefficients (LDS reads at wave-uniform addresses: broadcasts),
//             the half-grid e = gt_j + gt_{j+1} carried from point to point, then the division-form pivot of count_above_chunked (the
//             same guard, the same fast_rcp recurrence).  A lane always counts: the verdict costs the same instruction
// The line is staged again for every pass (a sixty-fourth of the chain's work); nothing is written to global memory but the results.
#include "ibs_local_eq_boundary.hpp"
#include "ibs_geo_line.hpp"
#include "ibs_long.hpp"

namespace ibs {

namespace {

// one (line, ray), wave-uniform: what the staging needs beside the arrays
struct RaySystem {
  GeoLine ln; const double* ps; int N; double theta_lo, h, thc;
  double x0, x0s, pm1;      // X0_j = x0 + x0s dth_j + pm1 ps_j
  double x1, x1s, dp;       // X1_j = x1 + x1s dth_j + dp ps_j
  double p0, mdP;           // p(t) = p0 + t dp; -dPdrho
  double hh2;               // 0.5 / h^2
};

// eigenvalues above sig of the system at this lane's t; bad: non-finite coefficients (any lane's points), g <= 0 or a non-finite
// pivot at this lane's t
__device__ __forceinline__ int count_at_t(const RaySystem& s, double t, double sig, double* lds, int lane, bool& bad) {
  constexpr double pivmin = 2.2250738585072014e-292;
  const int N = s.N;
  int cnt = 0;
  double q = 1.0, g_prev = 0.0, c_prev = 0.0, f_prev = 0.0, e_lo = 0.0, gmin = 1e300;
  auto point = [&](const double* v, double& g, double& c, double& f) {
    g = xfma(xfma(v[2], t, v[1]), t, v[0]);
    c = xfma(xfma(v[6], t, v[5]), t, v[4]);
    f = v[3] * g;
    gmin = xmin(gmin, g);
  };
  for (int j0 = 0; j0 < N; j0 += kBoundaryChunk) {
    const int m = N - j0 < kBoundaryChunk ? N - j0 : kBoundaryChunk;
    // ---- staging: the seven coefficients of every point of the chunk
    for (int i = lane; i < m; i += kWave) {
      const int j = j0 + i;
      const double B = s.ln.at(0, j), gp = xabs(s.ln.at(1, j)), gb = s.ln.at(7, j);
      const double dth = xfma((double)j, s.h, s.theta_lo) - s.thc;
      const double psj = s.ps ? s.ps[j] : 0.0;
      const double X0 = xfma(s.pm1, psj, xfma(s.x0s, dth, s.x0)), X1 = xfma(s.dp, psj, xfma(s.x1s, dth, s.x1));
      const double inv = 1.0 / (gp * B);
      const double A1 = gp / B * s.hh2;
      const double g21 = 2.0 * s.ln.at(5, j), g22 = s.ln.at(6, j), cv0 = s.ln.at(3, j), D = s.ln.at(2, j) - gb;
      double* v = lds + kBoundaryVals * i;
      v[0] = A1 * xfma(X0, xfma(X0, g22, g21), s.ln.at(4, j));
      v[1] = A1 * (X1 * xfma(2.0 * X0, g22, g21));
      v[2] = A1 * (X1 * X1 * g22);
      v[3] = inv * inv / s.hh2;
      const double K = s.mdP * inv;
      const double Ac = xfma(X0, cv0, xfma(s.p0, D, gb)), Bc = xfma(X1, cv0, s.dp * D);      // cv'(t) = Ac + t Bc
      v[4] = K * (s.p0 * Ac);
      v[5] = K * xfma(s.p0, Bc, s.dp * Ac);
      v[6] = K * (s.dp * Bc);
      bad = bad || !finite_of(v[0]) || !finite_of(v[1]) || !finite_of(v[2]) || !(v[3] > 0.0) || !finite_of(v[3]) || !finite_of(v[4]) ||
            !finite_of(v[5]) || !finite_of(v[6]);
    }
    wave_lds_sync();
    // ---- chain: at point k the row of point k - 1 is complete (its e_hi needs gt_k)
    int i = 0;
    if (j0 == 0) {                                          // (N >= 66: points 0, 1, 2 lie in the first chunk)
      double g0, g1, g2, c0, f0, c1, f1;
      point(lds, g0, c0, f0);
      point(lds + kBoundaryVals, g1, c1, f1);
      point(lds + 2 * kBoundaryVals, g2, c_prev, f_prev);
      e_lo = g0 + g1;
      const double e_hi = g1 + g2;
      q = xfma(-sig, f1, c1 - (e_lo + e_hi));
      q = xabs(q) < pivmin ? -pivmin : q;
      cnt += q > 0.0 ? 1 : 0;
      e_lo = e_hi; g_prev = g2;
      i = 3;
    }
#pragma unroll 4
    for (; i < m; ++i) {
      double g, c, f;
      point(lds + kBoundaryVals * i, g, c, f);
      const double e_hi = g_prev + g;
      const double a = xfma(-sig, f_prev, c_prev - (e_lo + e_hi));
      q = xfma(-(e_lo * e_lo), fast_rcp(q), a);
      q = xabs(q) < pivmin ? -pivmin : q;
      cnt += q > 0.0 ? 1 : 0;
      e_lo = e_hi; g_prev = g; c_prev = c; f_prev = f;
    }
    wave_lds_sync();
  }
  bad = bad || !(gmin > 0.0) || !finite_of(q);
  return cnt;
}

__device__ __forceinline__ double lane_value(double v, int l) { return readlane_t(v, __builtin_amdgcn_readfirstlane(l)); }

}  // namespace

__global__ void __launch_bounds__(64) k_local_eq_boundary(const LocalEqBoundaryArgs a) {
  __shared__ double lds[kBoundaryVals * kBoundaryChunk];
  static_assert(sizeof(lds) <= 20 * 1024 && sizeof(lds) * 8 <= 160 * 1024, "eight blocks per CU");
  const int lane = threadIdx.x & 63;
  const long n_sys = (long)a.n_lines * a.n_ray;
  const double nan = __builtin_nan("");
  for (long sys = blockIdx.x; sys < n_sys; sys += gridDim.x) {
    const int line = (int)(sys / a.n_ray), ir = (int)(sys - (long)line * a.n_ray);
    const double dP = uniform(a.dPdrho[line]), thc = uniform(a.centre[line]), sg = uniform(a.sigma[line]);
    const double* ry = a.rays + 7 * (long)ir;
    const double th0 = uniform(ry[0]), e0 = uniform(ry[1]), p0 = uniform(ry[2]), de = uniform(ry[3]), dp = uniform(ry[4]);
    const double t_lo = uniform(ry[5]), t_hi = uniform(ry[6]);
    const double range = t_hi - t_lo;
    RaySystem s;
    s.ln = GeoLine{a.geo + (long)line * a.ld, (long)a.plane};
    s.ps = a.ps ? a.ps + (long)line * a.ps_ld : nullptr;
    s.N = a.N; s.theta_lo = a.theta_lo; s.h = a.h; s.thc = thc;
    s.x0 = th0 * (1.0 + e0); s.x0s = sg * e0; s.pm1 = p0 - 1.0;
    s.x1 = th0 * de; s.x1s = sg * de; s.dp = dp;
    s.p0 = p0; s.mdP = -dP;
    s.hh2 = 0.5 / (a.h * a.h);
    bool bad = !(xabs(sg) == 1.0) || !finite_of(dP) || !finite_of(thc) || !finite_of(th0) || !finite_of(e0) || !finite_of(p0) ||
               !finite_of(de) || !finite_of(dp) || !finite_of(t_lo) || !finite_of(t_hi) || !(t_lo < t_hi) || !finite_of(range);
    int status = 0, passes = 0, n_cross = 0, lo_unst = -1, cnt0 = -1;
    double ts = nan, tu = nan;                              // lane i: the two ends of crossing i
    if (!bad) {
      // ---- pass 0: the 64 nodes
      const double t0 = lane == 63 ? t_hi : xfma((double)lane, range / 63.0, t_lo);
      cnt0 = count_at_t(s, t0, a.shift, lds, lane, bad);
      passes = 1;
      bad = __any(bad);
      if (!bad) {
        const unsigned long long U = __ballot(cnt0 > 0);
        unsigned long long X = (U ^ (U >> 1)) & 0x7fffffffffffffffULL;      // bit k: nodes k and k + 1 differ
        lo_unst = (int)(U & 1);
        const int n_all = __popcll(X);
        n_cross = n_all < a.max_cross ? n_all : a.max_cross;
        if (n_all > a.max_cross) status |= 4;
        const double tol = a.xtol * range;
        // ---- closing, one crossing after the other
        for (int ic = 0; ic < n_cross && !bad; ++ic) {
          const int k = __builtin_ctzll(X);
          X &= X - 1;
          const bool ua = (U >> k) & 1;                       // the verdict at the bracket's lower end, and of every later lower end
          double ta = lane_value(t0, k), tb = lane_value(t0, k + 1);
          for (int np = 0;; ++np) {
            const double w = tb - ta;
            if (w <= tol) break;
            if (np == kBoundaryPassCap) { status |= 1; break; }
            const double tl = xfma((double)(lane + 1), w / 65.0, ta);
            const bool below = tl <= ta, above = tl >= tb;      // (the ends are FP64 neighbours, or nearly: such a lane stands for its end)
            if (!__any(!below && !above)) { status |= 8; break; }
            const double te = below ? ta : (above ? tb : tl);
            const int c = count_at_t(s, te, a.shift, lds, lane, bad);
            ++passes;
            bad = __any(bad);
            if (bad) break;
            const bool v = below ? ua : (above ? !ua : c > 0);
            const unsigned long long V = __ballot(v);
            const unsigned long long D = V ^ ((V << 1) | (ua ? 1ULL : 0ULL));      // bit l: lane l differs from lane l - 1 (lane -1 = the lower end)
            if (D) {
              const int l = __builtin_ctzll(D);
              const double nb = lane_value(te, l);
              if (l > 0) ta = lane_value(te, l - 1);
              tb = nb;
            } else {
              ta = lane_value(te, 63);                         // (every lane has the lower end's verdict: the flip is before tb)
            }
          }
          if (lane == ic) { ts = ua ? tb : ta; tu = ua ? ta : tb; }
        }
      }
    }
    if (bad) { status = 2; n_cross = -1; lo_unst = -1; cnt0 = -1; ts = tu = nan; }
    if (lane < a.max_cross) {
      a.t_stable[sys * a.max_cross + lane] = ts;
      a.t_unstable[sys * a.max_cross + lane] = tu;
    }
    if (a.node_count) a.node_count[sys * 64 + lane] = cnt0;
    if (lane == 0) {
      a.n_cross[sys] = n_cross;
      if (a.lo_unstable) a.lo_unstable[sys] = lo_unst;
      if (a.info) a.info[sys] = passes | (status << 16);
    }
  }
}

hipError_t launch_local_eq_boundary(const LocalEqBoundaryArgs& a, hipStream_t st) {
  const long n_sys = (long)a.n_lines * a.n_ray;
  if (n_sys <= 0) return hipSuccess;
  const long grid = n_sys < a.n_waves ? n_sys : a.n_waves;      // the persistent grid (persistent_grid, ibs_launch.hpp) without a workspace
  if (grid < 1 || !a.geo || !a.dPdrho || !a.centre || !a.sigma || !a.rays || !a.t_stable || !a.t_unstable || !a.n_cross)
    return hipErrorInvalidValue;
  if (a.ld < a.N || (a.ps && a.ps_ld < a.N) || a.plane < (size_t)a.n_lines * (size_t)a.ld || a.N < 66 || a.max_cross < 1 ||
      a.max_cross > kMaxCross)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_local_eq_boundary, dim3((unsigned)grid), dim3(64), 0, st, a);
  note_launch(grid, 64, "ibs::k_local_eq_boundary");
  return hipGetLastError();
}

}  // namespace ibs
