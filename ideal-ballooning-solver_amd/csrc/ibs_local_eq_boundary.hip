// Local-equilibrium boundaries: the parameters t at which a field line crosses the stability boundary along rays (theta0, eps0 + t d_eps,
// p0 + t d_p) of the rule of ibs_local_eq.hpp, closed on the device.  FP64, every odd N in [66, 65,537], one wavefront per (line, ray) on
// the persistent grid of the long path; the 64 lanes are 64 values of t of ONE system.  The rule for a ray, the staged form (seven
// polynomial coefficients in t per grid point), the passes and the status bits: ibs_local_eq_boundary.hpp.
// Staging, the per-lane count, node placement and the closing of a bracket: ibs_local_eq_boundary_stages.hpp, shared with
// k_local_eq_boundary_polish.  Nothing is written to global memory but the results.
#include "ibs_local_eq_boundary_stages.hpp"

namespace ibs {

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
    bool bad = ray_setup(s, a, line, dP, thc, sg, th0, e0, p0, de, dp, t_lo, t_hi, range);
    int status = 0, passes = 0, n_cross = 0, lo_unst = -1, cnt0 = -1;
    double ts = nan, tu = nan;                              // lane i: the two ends of crossing i
    if (!bad) {
      // ---- pass 0: the 64 nodes
      const double t0 = ray_node(lane, t_lo, t_hi, range);
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
          close_crossing(s, a.shift, tol, ua, ta, tb, lds, lane, bad, status, passes);
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
