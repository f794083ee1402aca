// The margin maximised over theta0 on every line: mu = 1 / s* (ibs_marginal.hip) between the nodes of the line's coarse row
// mu[line][:], about the row's K <= 4 best peaks or about the nodes the caller names.  The rule -- peaks, bracket, Brent's bounded
// search, incumbent -- is ibs_theta0_polish.hpp's, used unchanged: k_theta0_polish (ibs_kernels.hip) runs it on gam, this kernel on mu.
// Nothing upstream corresponds.  FP64, every odd N in [66, 65,537].
// One wavefront per (line, slot) on the persistent grid of the long path, with the per-wave workspace and the LDS of k_marginal_scan.
// Every requested theta0 is ONE cold evaluation, the statements of k_marginal_scan: the rows g, c by line_gcf, then marginal_one
// without the mode, then mu = 1 / s.  s* = +inf is the VALUE mu = 0; an evaluation with status bit 0 or 1 counts as -inf and its bits
// are OR-ed into the slot's word (t0p::step).  The tag of a point is its s*, so scale_star is the s* of the evaluation that gave
// mu_star, bit for bit what k_marginal_scan gives at theta0_star.  Where the node itself is returned (status bit 10) mu_star is the
// row's entry and, if scale_star is asked for, one more evaluation at the node supplies it: it is not a step of the search and enters
// neither n_eval nor the pass count of info.
// The search state is held by every lane alike (all 64 lanes execute the same scalar statements on the same values); the loop has
// the fixed bound t0p::kMaxEval + 1.  No floating-point atomics; a slot's arithmetic depends on its line, its node and the row alone.
#include "ibs_marginal.hpp"
#include "ibs_geo_line.hpp"
#include "ibs_launch.hpp"
#include "ibs_theta0_polish.hpp"

namespace ibs {

__global__ void __launch_bounds__(64) k_marginal_theta0_polish(const MarginalPolishArgs a) {
  __shared__ double lds[3 * kLongChunk];
  static_assert(sizeof(lds) * 8 <= 160 * 1024, "eight blocks per CU");
  const int lane = threadIdx.x & 63;
  const int N = a.N, n_theta0 = a.n_theta0, K = a.n_starts;
  const MarginalWs L = marginal_ws(N, true);
  double* my = a.work + (size_t)blockIdx.x * L.total;
  double* Xw = my + L.X; double* G = my + L.g; double* C = my + L.c;
  const double nan = __builtin_nan("");
  const bool grid_ok = t0p::grid_ok(a.theta0, n_theta0);
  const long n_slots = (long)a.n_lines * K;
  for (long slot = blockIdx.x; slot < n_slots; slot += gridDim.x) {
    const int line = (int)(slot / K), k = (int)(slot - (long)line * K);
    // ---- the slot's node: the row's own peak of this rank, or the caller's
    const double* row = a.mu + (size_t)line * n_theta0;
    int node = -1, n_found = 0;
    if (a.node_in) {
      node = a.node_in[slot];
      if (node >= n_theta0) node = -1;
    } else {
      int nodes[t0p::kMaxSlots];
      n_found = t0p::row_peaks(row, n_theta0, K, nodes);
      node = nodes[0];
#pragma unroll
      for (int r = 1; r < t0p::kMaxSlots; ++r) node = (r == k) ? nodes[r] : node;
    }
    node = __builtin_amdgcn_readfirstlane(node);
    if (a.n_found && k == 0 && lane == 0) a.n_found[line] = n_found;
    if (node >= 0 && !(row[node] == row[node])) node = -1;               // (a caller's node without a value)
    if (node < 0 || !grid_ok) {                                           // (wave-uniform)
      if (lane == 0) {
        a.theta0_star[slot] = nan; a.mu_star[slot] = nan;
        if (a.scale_star) a.scale_star[slot] = nan;
        if (a.node) a.node[slot] = grid_ok ? -1 : node;
        if (a.n_eval) a.n_eval[slot] = 0;
        if (a.info) a.info[slot] = grid_ok ? 0 : (2 << 16);
      }
      continue;
    }
    const double dP = uniform(a.dPdrho[line]), mdP = -dP;
    const GeoLine7 ln = geo_line7(a.geo7, (long)line * a.ld);
    t0p::State st;
    bool more = t0p::init_row(st, a.theta0, row, n_theta0, node, nan, a.xtol, a.max_eval);
    int passes_all = 0;
    bool at_node = false;
    for (int it = 0; it <= t0p::kMaxEval; ++it) {
      if (!__builtin_amdgcn_readfirstlane((int)more)) {
        // the search is over: the node's own s* where the node is the result and scale_star is wanted
        double x, f, tag;
        int status;
        t0p::result(st, x, f, tag, status);
        at_node = a.scale_star != nullptr && (status & t0p::kNodeReturned) != 0;
        if (!__builtin_amdgcn_readfirstlane((int)at_node)) break;
      }
      const double th0 = uniform(at_node ? st.xn : st.u);
      // ---- the rows at theta0 and the cold solve, as k_marginal_scan
      for (int j = lane; j < N; j += kWave) line_gcf(ln, j, mdP, th0, G[j], C[j]);
      long_fence();                                           // (rows written by every lane, read by every lane below)
      int status, passes;
      double gam0;
      const double s = marginal_one(G, C, N, a.h, my + L.work, Xw, false, lds, status, passes, gam0);
      long_fence();                                           // (the rows are overwritten by this wave's next evaluation)
      if (at_node) { st.ln = s; break; }
      passes_all += passes;
      more = t0p::step(st, 1.0 / s, s, status);
    }
    if (lane == 0) {
      double x, f, tag;
      int status;
      t0p::result(st, x, f, tag, status);
      if (f == 0.0) status |= 256;                            // mu = 0: the returned point has s* = +inf
      a.theta0_star[slot] = x; a.mu_star[slot] = f;
      if (a.scale_star) a.scale_star[slot] = tag;
      if (a.node) a.node[slot] = node;
      if (a.n_eval) a.n_eval[slot] = st.n_eval;
      if (a.info) a.info[slot] = (passes_all > 0xffff ? 0xffff : passes_all) | (status << 16);
    }
  }
}

hipError_t launch_marginal_theta0_polish(const MarginalPolishArgs& a, hipStream_t st) {
  const long n_slots = (long)a.n_lines * a.n_starts;
  if (n_slots <= 0) return hipSuccess;
  const long grid = persistent_grid(n_slots, a.n_waves, a.work, a.work_doubles, marginal_ws(a.N, true).total);
  if (!grid || !a.dPdrho || !a.theta0 || !a.mu || !a.theta0_star || !a.mu_star || a.n_theta0 < 1 || a.n_starts > t0p::kMaxSlots)
    return hipErrorInvalidValue;
  for (int k = 0; k < 7; ++k) if (!a.geo7[k]) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_marginal_theta0_polish, dim3((unsigned)grid), dim3(64), 0, st, a);
  note_launch(grid, 64, "ibs::k_marginal_theta0_polish");
  return hipGetLastError();
}

}  // namespace ibs
