// The stages k_local_eq_boundary (ibs_local_eq_boundary.hip) and k_local_eq_boundary_polish (ibs_local_eq_boundary_polish.hip) share, one
// definition of each: the wave-uniform set-up of a (line, ray), the coefficient staging with the per-lane division-form count over the
// chunks (count_at_t), the placement of the 64 nodes of pass 0 and the closing of one bracket.  The rule for a ray, the staged form and
// the status bits: ibs_local_eq_boundary.hpp.  Device code only; included by those two files.
//   staging   a chunk of kBoundaryChunk grid points at a time, by all lanes: coalesced loads of the eight arrays and the ps row, the
//             t-invariant factors and the seven coefficients formed once per point, written to LDS point-major ([point][7])
//   chain     every lane walks the chunk: gt, c, f of its own t from the coefficients (LDS reads at wave-uniform addresses: broadcasts),
//             the half-grid e = gt_j + gt_{j+1} carried from point to point, then the division-form pivot of count_above_chunked (the
//             same guard, the same fast_rcp recurrence).  A lane always counts: the verdict costs the same instruction
// The line is staged again for every pass (a sixty-fourth of the chain's work); nothing is written to global memory.
#pragma once
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

// the system of line `line` of the launch arguments a (geo, ld, plane, ps, ps_ld, N, theta_lo, h) on the ray (th0, e0, p0, de, dp) over
// [t_lo, t_hi]; returns bad: sigma not +-1, a non-finite scalar or ray, t_lo >= t_hi
template <class Args>
__device__ __forceinline__ bool ray_setup(RaySystem& s, const Args& a, int line, double dP, double thc, double sg, double th0, double e0,
                                          double p0, double de, double dp, double t_lo, double t_hi, double range) {
  s.ln = GeoLine{a.geo + (long)line * a.ld, (long)a.plane};
  s.ps = a.ps ? a.ps + (long)line * a.ps_ld : nullptr;
  s.N = a.N; s.theta_lo = a.theta_lo; s.h = a.h; s.thc = thc;
  s.x0 = th0 * (1.0 + e0); s.x0s = sg * e0; s.pm1 = p0 - 1.0;
  s.x1 = th0 * de; s.x1s = sg * de; s.dp = dp;
  s.p0 = p0; s.mdP = -dP;
  s.hh2 = 0.5 / (a.h * a.h);
  return !(xabs(sg) == 1.0) || !finite_of(dP) || !finite_of(thc) || !finite_of(th0) || !finite_of(e0) || !finite_of(p0) ||
         !finite_of(de) || !finite_of(dp) || !finite_of(t_lo) || !finite_of(t_hi) || !(t_lo < t_hi) || !finite_of(range);
}

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

// pass 0: this lane's node of [t_lo, t_hi], range = t_hi - t_lo (lane 63: t_hi itself)
__device__ __forceinline__ double ray_node(int lane, double t_lo, double t_hi, double range) {
  return lane == 63 ? t_hi : xfma((double)lane, range / 63.0, t_lo);
}

// The closing passes of ONE crossing: [ta, tb] is a bracket whose lower end has the verdict ua and whose upper end has the other.  Each
// pass puts the lanes at ta + (l + 1) (tb - ta) / 65 and keeps the first adjacent pair (ends included) whose verdicts differ, until
// tb - ta <= tol, no lane point lies strictly inside (status bit 3), kBoundaryPassCap passes were made (status bit 0) or a pass met
// invalid data (bad).  At most kBoundaryPassCap passes whatever the data; every value that leaves is wave-uniform
__device__ __forceinline__ void close_crossing(const RaySystem& s, double shift, double tol, bool ua, double& ta, double& tb, double* lds,
                                               int lane, bool& bad, int& status, int& passes) {
  for (int np = 0;; ++np) {
    const double w = tb - ta;
    if (w <= tol) break;
    if (np == kBoundaryPassCap) { status |= 1; break; }
    const double tl = xfma((double)(lane + 1), w / 65.0, ta);
    const bool below = tl <= ta, above = tl >= tb;      // (the ends are FP64 neighbours, or nearly: such a lane stands for its end)
    if (!__any(!below && !above)) { status |= 8; break; }
    const double te = below ? ta : (above ? tb : tl);
    const int c = count_at_t(s, te, shift, lds, lane, bad);
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
}

}  // namespace

}  // namespace ibs
