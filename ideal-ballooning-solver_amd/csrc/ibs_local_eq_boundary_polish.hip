// The first-stability parameter of every (line, ray family) minimised over theta0 between the nodes of the family's coarse row, about the
// row's K <= 4 best peaks of f = -T.  The rule -- T(theta0), the search, the early return, the outputs and the status bits --:
// ibs_local_eq_boundary_polish.hpp; peaks, bracket, Brent's bounded search and the incumbent are ibs_theta0_polish.hpp's, used unchanged,
// as k_theta0_polish runs them on gam and k_marginal_theta0_polish on mu.  FP64, every odd N in [66, 65,537].
// One wavefront per (line, family, slot) on the persistent grid of the long path.  Every requested theta0 is ONE cold evaluation by the
// stages of ibs_local_eq_boundary_stages.hpp, the statements of k_local_eq_boundary with max_cross = 1: pass 0 at the 64 nodes, then the
// closing passes of the first crossing; the coefficients are staged per (chunk, pass) in the block's 20,160 bytes of LDS.
// The search state is held by every lane alike (all 64 lanes execute the same scalar statements on the same values).  No atomics, no
// global workspace; a slot's arithmetic depends on its line, its family, its row and its slot alone.
#include "ibs_local_eq_boundary_polish.hpp"
#include "ibs_local_eq_boundary_stages.hpp"

namespace ibs {

namespace {

struct FirstUp { double T, ts, tu; int lo, status, passes; };

// T of the family (e0, p0, de, dp, t_lo, t_hi) at th0 on line `line`: k_local_eq_boundary's statements with max_cross = 1.  Loops: pass
// 0 and at most kBoundaryPassCap closing passes (close_crossing), each ceil(N / kBoundaryChunk) chunks, whatever the data
__device__ __forceinline__ FirstUp first_up(const LocalEqBoundaryPolishArgs& a, int line, double dP, double thc, double sg, double th0,
                                            double e0, double p0, double de, double dp, double t_lo, double t_hi, double* lds, int lane) {
  const double nan = __builtin_nan("");
  const double range = t_hi - t_lo;
  RaySystem s;
  bool bad = ray_setup(s, a, line, dP, thc, sg, th0, e0, p0, de, dp, t_lo, t_hi, range);
  FirstUp r{nan, nan, nan, -1, 0, 0};
  int n_all = 0;
  if (!bad) {
    const double t0 = ray_node(lane, t_lo, t_hi, range);
    const int cnt0 = count_at_t(s, t0, a.shift, lds, lane, bad);
    r.passes = 1;
    bad = __any(bad);
    if (!bad) {
      const unsigned long long U = __ballot(cnt0 > 0);
      const unsigned long long X = (U ^ (U >> 1)) & 0x7fffffffffffffffULL;      // bit k: nodes k and k + 1 differ
      r.lo = (int)(U & 1);
      n_all = __popcll(X);
      if (n_all > 0) {
        const int k = __builtin_ctzll(X);
        const bool ua = (U >> k) & 1;
        double ta = lane_value(t0, k), tb = lane_value(t0, k + 1);
        close_crossing(s, a.shift, a.xtol * range, ua, ta, tb, lds, lane, bad, r.status, r.passes);
        r.ts = ua ? tb : ta; r.tu = ua ? ta : tb;
      }
    }
  }
  if (bad) { r.status = 2; r.lo = -1; r.ts = r.tu = nan; return r; }
  r.T = r.lo ? t_lo : (n_all > 0 ? 0.5 * (r.ts + r.tu) : HUGE_VAL);
  return r;
}

}  // namespace

__global__ void __launch_bounds__(64) k_local_eq_boundary_polish(const LocalEqBoundaryPolishArgs a) {
  __shared__ double lds[kBoundaryVals * kBoundaryChunk];
  static_assert(sizeof(lds) <= 20 * 1024 && sizeof(lds) * 8 <= 160 * 1024, "eight blocks per CU");
  static_assert(kBoundaryPolishMaxTheta0 * sizeof(double) <= sizeof(lds), "the coarse row of a slot fits the block's LDS");
  const int lane = threadIdx.x & 63;
  const int n_theta0 = a.n_theta0, K = a.n_starts;
  const long n_sys = (long)a.n_lines * a.n_ray * K;
  const double nan = __builtin_nan("");
  const bool grid_ok = t0p::grid_ok(a.theta0, n_theta0);
  for (long sys = blockIdx.x; sys < n_sys; sys += gridDim.x) {
    const long fam = sys / K;                               // (line, family)
    const int k = (int)(sys - fam * K);
    const int line = (int)(fam / a.n_ray), ir = (int)(fam - (long)line * a.n_ray);
    // ---- f = -T of the slot's coarse row into LDS (free until the first evaluation), its peaks and the slot's node
    const double* trow = a.t_row + (size_t)fam * n_theta0;
    for (int j = lane; j < n_theta0; j += kWave) lds[j] = -trow[j];
    wave_lds_sync();
    int nodes[t0p::kMaxSlots];
    const int n_found = t0p::row_peaks(lds, n_theta0, K, nodes);
    int node = nodes[0];
#pragma unroll
    for (int r = 1; r < t0p::kMaxSlots; ++r) node = (r == k) ? nodes[r] : node;
    node = __builtin_amdgcn_readfirstlane(node);
    if (a.n_found && k == 0 && lane == 0) a.n_found[fam] = n_found;
    const double dP = uniform(a.dPdrho[line]), thc = uniform(a.centre[line]), sg = uniform(a.sigma[line]);
    const double* ry = a.rays + 7 * (long)ir;
    const double e0 = uniform(ry[1]), p0 = uniform(ry[2]), de = uniform(ry[3]), dp = uniform(ry[4]);
    const double t_lo = uniform(ry[5]), t_hi = uniform(ry[6]);
    double x = nan, T = nan, ts = nan, tu = nan;
    int lo = -1, status = 0, n_eval = 0, passes_all = 0;
    if (node >= 0 && grid_ok) {                             // (wave-uniform)
      const double xn = uniform(a.theta0[node]), Tn = uniform(trow[node]);
      RaySystem chk;
      const bool bad = ray_setup(chk, a, line, dP, thc, sg, xn, e0, p0, de, dp, t_lo, t_hi, t_hi - t_lo);
      if (bad) {
        status = 2;
      } else if (Tn == t_lo) {                              // the addition to the rule: nothing can beat the node
        x = xn; T = Tn; lo = 1; status = t0p::kNodeReturned;
      } else {
        t0p::State st;
        bool more = t0p::init_row(st, a.theta0, lds, n_theta0, node, nan, a.xtol_theta0, a.max_eval);
        wave_lds_sync();                                    // (the row is read; the evaluations stage over it)
        int lo_x = -1;
        double ts_x = nan, tu_x = nan;                      // the ends and the verdict at t_lo of the evaluation that gave st.x
        bool at_node = false;
        // at most max_eval <= t0p::kMaxEval evaluations of the search and one at the node, each (1 + kBoundaryPassCap) passes of
        // ceil(N / kBoundaryChunk) chunks: every bound is independent of the data
        for (int it = 0; it <= t0p::kMaxEval; ++it) {
          if (!__builtin_amdgcn_readfirstlane((int)more)) {
            // the search is over: the node's own ends where the node is the result
            double rx, rf, rtag;
            int rs;
            t0p::result(st, rx, rf, rtag, rs);
            at_node = (rs & t0p::kNodeReturned) != 0;
            if (!__builtin_amdgcn_readfirstlane((int)at_node)) break;
          }
          const double th0 = uniform(at_node ? st.xn : st.u);
          const FirstUp r = first_up(a, line, dP, thc, sg, th0, e0, p0, de, dp, t_lo, t_hi, lds, lane);
          if (at_node) { status |= r.status & 11; ts_x = r.ts; tu_x = r.tu; lo_x = r.lo; break; }
          passes_all += r.passes;
          status |= r.status & 8;
          more = t0p::step(st, -r.T, nan, r.status);
          if (st.x == th0) { ts_x = r.ts; tu_x = r.tu; lo_x = r.lo; }      // (the point became the best one: Brent never asks for x again)
        }
        double rf, rtag;
        int rs;
        t0p::result(st, x, rf, rtag, rs);
        status |= rs;
        T = -rf; ts = ts_x; tu = tu_x; lo = lo_x; n_eval = st.n_eval;
      }
      if (status & 2) { x = T = ts = tu = nan; lo = -1; }
    } else if (!grid_ok) {
      status = 2;
    }
    if (lane == 0) {
      a.theta0_out[sys] = x; a.t_out[sys] = T; a.t_stable_out[sys] = ts; a.t_unstable_out[sys] = tu;
      if (a.node) a.node[sys] = node;
      if (a.n_eval) a.n_eval[sys] = n_eval;
      if (a.lo_unstable) a.lo_unstable[sys] = lo;
      if (a.info) a.info[sys] = (passes_all > 0xffff ? 0xffff : passes_all) | (status << 16);
    }
    wave_lds_sync();                                        // (the next slot's row is written over the last evaluation's coefficients)
  }
}

hipError_t launch_local_eq_boundary_polish(const LocalEqBoundaryPolishArgs& a, hipStream_t st) {
  const long n_sys = (long)a.n_lines * a.n_ray * a.n_starts;
  if (n_sys <= 0) return hipSuccess;
  const long grid = n_sys < a.n_waves ? n_sys : a.n_waves;      // the persistent grid (persistent_grid, ibs_launch.hpp) without a workspace
  if (grid < 1 || !a.geo || !a.dPdrho || !a.centre || !a.sigma || !a.rays || !a.theta0 || !a.t_row || !a.theta0_out || !a.t_out ||
      !a.t_stable_out || !a.t_unstable_out)
    return hipErrorInvalidValue;
  if (a.ld < a.N || (a.ps && a.ps_ld < a.N) || a.plane < (size_t)a.n_lines * (size_t)a.ld || a.N < 66 || a.n_ray < 1 || a.n_theta0 < 1 ||
      a.n_theta0 > kBoundaryPolishMaxTheta0 || a.n_starts < 1 || a.n_starts > t0p::kMaxSlots || a.max_eval < 1 ||
      a.max_eval > t0p::kMaxEval)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_local_eq_boundary_polish, dim3((unsigned)grid), dim3(64), 0, st, a);
  note_launch(grid, 64, "ibs::k_local_eq_boundary_polish");
  return hipGetLastError();
}

}  // namespace ibs
