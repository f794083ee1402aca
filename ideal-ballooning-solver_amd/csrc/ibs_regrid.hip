// Lines on a non-uniform theta grid: the regrid of utils.py:1565-1576 on the device (ibs_regrid.hpp states it with its rounding).
// Upstream interpolates the FORMED rows g, c, f -- not the geometry arrays -- onto the uniform grid of the same end points, and g once
// more at the uniform half points; the raw solvers take the result as (g, gh, c, f) with h = regrid_spacing().
//
// Both kernels are built on one routine, regrid_locate: the interval of the line's own grid that holds uniform node j and the one that
// holds half node j.  A thread owns node j of ONE line and finds the two intervals ONCE, by bisection of the line's theta row -- staged
// in LDS up to kRegridLdsN points (16.4 KB a block), read from global memory beyond --, then walks the systems that share that grid (the
// theta0 values of a line; every system of a raw batch on one shared grid) with the intervals, the abscissae and, in the geometry-fed
// kernel, the geometry at the four samples held in registers.  The search therefore costs the same whatever n_theta0 is; blockIdx.z
// only splits the walk where a launch would otherwise leave most of the chip idle.
//   grid   x: nodes of a line (256 a block, grid-stride), y: lines (grid-stride), z: a share of the systems of a line
//   LDS    bisection reads are ds_read_b64 at neighbouring or equal indices across a wave (neighbouring nodes fall into neighbouring
//          intervals): equal addresses broadcast, neighbours sit on different banks
// A line whose grid is not one (regrid_pair_ok on every neighbouring pair, the two ends on the window: every block checks the row it
// staged, one __syncthreads_or) gets NaN rows and status bit 1; the bisection stays inside [0, N - 2] on any row, so nothing is read or
// written out of bounds either way.  No sums, no atomics: every output entry is a function of its own line alone, hence bit for bit
// independent of the batch, of the order of the lines and of the launch shape.
#include "ibs_regrid.hpp"
#include "ibs_geo_line.hpp"
#include "ibs_launch.hpp"

namespace ibs {

constexpr int kRegridThreads = 256;

// the interval k of node j and kh of half node j with the abscissae interpolation needs (x0 = row[k], x1 = row[k + 1]; likewise h0, h1)
struct RegridCell {
  int k, kh;
  double x, x0, x1, xh, h0, h1;
};
template <class Row>
__device__ __forceinline__ RegridCell regrid_locate(const Row& row, int N, int j, double lo, double hi, double step) {
  RegridCell c;
  c.x = regrid_node(j, N, lo, hi, step);
  c.k = regrid_interval(row, N, c.x);
  c.x0 = row[c.k]; c.x1 = row[c.k + 1];
  const int jh = j < N - 1 ? j : N - 2;              // (the last node has no half node: gh[N - 1] = 0)
  c.xh = regrid_half_node(jh, N, lo, hi, step);
  c.kh = regrid_interval(row, N, c.xh);
  c.h0 = row[c.kh]; c.h1 = row[c.kh + 1];
  return c;
}

// stages the row (LDS form) and says whether it is a grid on [lo, hi]: block-uniform
template <bool LDS>
__device__ __forceinline__ bool regrid_stage(const double* __restrict__ th, double* sth, int N, double lo, double hi) {
  if (LDS) {
    for (int i = threadIdx.x; i < N; i += blockDim.x) sth[i] = th[i];
    __syncthreads();
  }
  int bad = 0;
  for (int i = threadIdx.x; i < N - 1; i += blockDim.x) {
    const double a = LDS ? sth[i] : th[i], b = LDS ? sth[i + 1] : th[i + 1];
    bad |= regrid_pair_ok(a, b) ? 0 : 1;
  }
  if (threadIdx.x == 0) {
    const double a = LDS ? sth[0] : th[0], b = LDS ? sth[N - 1] : th[N - 1];
    bad |= (a == lo && b == hi) ? 0 : 1;
  }
  return __syncthreads_or(bad) == 0;
}

// the geometry of one sample of a line, in registers: line_gcf's accessor
struct GeoSample {
  double v[7];
  __device__ __forceinline__ double at(int k, int) const { return v[k]; }
};
__device__ __forceinline__ GeoSample geo_sample(const GeoLine7& ln, int j) {
  GeoSample s;
#pragma unroll
  for (int k = 0; k < 7; ++k) s.v[k] = ln.at(k, j);
  return s;
}

// raw rows (g, c, f)[n_sys][ld] on theta -> g_u, gh, c_u, f_u [n_sys][ld_out]; c / c_u and f / f_u optional as pairs
template <bool LDS>
__global__ void __launch_bounds__(kRegridThreads) k_regrid_rows(RegridArgs a) {
  __shared__ double sth[LDS ? kRegridLdsN : 1];
  const int N = a.N;
  const double step = regrid_step(a.lo, a.hi, N), nan = __builtin_nan("");
  for (long line = blockIdx.y; line < a.n_lines; line += gridDim.y) {
    const double* th = a.theta + line * a.theta_ld;
    const bool ok = regrid_stage<LDS>(th, sth, N, a.lo, a.hi);
    if (a.info && blockIdx.x == 0 && threadIdx.x == 0)
      for (long s = blockIdx.z; s < a.per_line; s += gridDim.z) a.info[line * a.per_line + s] = ok ? 0 : (2 << 16);
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < N; j += gridDim.x * blockDim.x) {
      const RegridCell cl = LDS ? regrid_locate(sth, N, j, a.lo, a.hi, step) : regrid_locate(th, N, j, a.lo, a.hi, step);
      for (long s = blockIdx.z; s < a.per_line; s += gridDim.z) {
        const long sys = line * a.per_line + s, o = sys * a.ld, oo = sys * a.ld_out + j;
        double gu = nan, gh = nan, cu = nan, fu = nan;
        if (ok) {                                       // (all loads before the first store: the outputs are not __restrict__)
          gu = regrid_value(cl.x, cl.x0, cl.x1, a.g[o + cl.k], a.g[o + cl.k + 1]);
          gh = j < N - 1 ? regrid_value(cl.xh, cl.h0, cl.h1, a.g[o + cl.kh], a.g[o + cl.kh + 1]) : 0.0;
          if (a.c) cu = regrid_value(cl.x, cl.x0, cl.x1, a.c[o + cl.k], a.c[o + cl.k + 1]);
          if (a.f) fu = regrid_value(cl.x, cl.x0, cl.x1, a.f[o + cl.k], a.f[o + cl.k + 1]);
        }
        a.g_u[oo] = gu; a.gh[oo] = gh;
        if (a.c_u) a.c_u[oo] = cu;
        if (a.f_u) a.f_u[oo] = fu;
      }
    }
    __syncthreads();                                    // (the staged row is replaced by the block's next line)
  }
}

// the geometry-fed form: for every (line, theta0) system g, c, f are formed at the samples k, k + 1 (kh, kh + 1) with line_gcf -- the
// expressions of every other kernel -- and interpolated; rows [n_lines * per_line][ld_out].  t0_per_line: per_line = 1, theta0[n_lines]
template <bool LDS>
__global__ void __launch_bounds__(kRegridThreads) k_assemble_regrid(RegridArgs a) {
  __shared__ double sth[LDS ? kRegridLdsN : 1];
  const int N = a.N;
  const double step = regrid_step(a.lo, a.hi, N), nan = __builtin_nan("");
  for (long line = blockIdx.y; line < a.n_lines; line += gridDim.y) {
    const double* th = a.theta + line * a.theta_ld;
    const bool ok = regrid_stage<LDS>(th, sth, N, a.lo, a.hi);
    if (a.info && blockIdx.x == 0 && threadIdx.x == 0)
      for (long s = blockIdx.z; s < a.per_line; s += gridDim.z) a.info[line * a.per_line + s] = ok ? 0 : (2 << 16);
    const double mdP = -a.dPdrho[line];
    const GeoLine7 ln = geo_line7(a.geo7, line * a.ld);
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < N; j += gridDim.x * blockDim.x) {
      const RegridCell cl = LDS ? regrid_locate(sth, N, j, a.lo, a.hi, step) : regrid_locate(th, N, j, a.lo, a.hi, step);
      const GeoSample p0 = geo_sample(ln, cl.k), p1 = geo_sample(ln, cl.k + 1), q0 = geo_sample(ln, cl.kh), q1 = geo_sample(ln, cl.kh + 1);
      for (long s = blockIdx.z; s < a.per_line; s += gridDim.z) {
        const long sys = line * a.per_line + s, oo = sys * a.ld_out + j;
        const double th0 = a.theta0[a.t0_per_line ? line : s];
        double gu = nan, gh = nan, cu = nan, fu = nan;
        if (ok) {
          double g0, c0, f0, g1, c1, f1, e0, e1, ce;          // (ce: c at the half node's samples, unused)
          line_gcf(p0, 0, mdP, th0, g0, c0, f0);
          line_gcf(p1, 0, mdP, th0, g1, c1, f1);
          line_gcf(q0, 0, mdP, th0, e0, ce);
          line_gcf(q1, 0, mdP, th0, e1, ce);
          gu = regrid_value(cl.x, cl.x0, cl.x1, g0, g1);
          cu = regrid_value(cl.x, cl.x0, cl.x1, c0, c1);
          fu = regrid_value(cl.x, cl.x0, cl.x1, f0, f1);
          gh = j < N - 1 ? regrid_value(cl.xh, cl.h0, cl.h1, e0, e1) : 0.0;
        }
        a.g_u[oo] = gu; a.gh[oo] = gh; a.c_u[oo] = cu; a.f_u[oo] = fu;
      }
    }
    __syncthreads();
  }
}

// The solvers flag a system of NaN rows (status bit 1) but leave its outputs as their set-up found them (lam = 0 in the staged kernel):
// the systems of a line that was not a grid (flag: the info words k_assemble_regrid wrote) get NaN in every floating-point output
__global__ void __launch_bounds__(64) k_regrid_poison(long n_sys, int N, const int* __restrict__ flag, double* lam, double* gam, double* X,
                                                      double* dX) {
  const double nan = __builtin_nan("");
  for (long sys = blockIdx.x; sys < n_sys; sys += gridDim.x) {
    if (((flag[sys] >> 16) & 2) == 0) continue;
    if (threadIdx.x == 0) {
      if (lam) lam[sys] = nan;
      if (gam) gam[sys] = nan;
    }
    for (int j = threadIdx.x; j < N; j += blockDim.x) {
      if (X) X[sys * N + j] = nan;
      if (dX) dX[sys * N + j] = nan;
    }
  }
}

hipError_t launch_regrid_poison(long n_sys, int N, const int* flag, double* lam, double* gam, double* X, double* dX, hipStream_t st) {
  if (n_sys <= 0 || !(lam || gam || X || dX)) return hipSuccess;
  LaunchNote keep = last_launch();                   // (ibs_last_launch names the solver kernel)
  hipLaunchKernelGGL(k_regrid_poison, dim3((unsigned)(n_sys < 4096 ? n_sys : 4096)), dim3(64), 0, st, n_sys, N, flag, lam, gam, X, dX);
  last_launch() = keep;
  return hipGetLastError();
}

// x: up to 64 blocks of nodes; y: lines; z: shares of a line's systems, only while the launch holds fewer than two blocks per CU
static dim3 regrid_grid(const RegridArgs& a) {
  long bx = (a.N + kRegridThreads - 1) / kRegridThreads;
  if (bx > 64) bx = 64;
  const long by = a.n_lines < 32768 ? a.n_lines : 32768;
  long bz = (2L * (a.n_cu > 0 ? a.n_cu : 256) + bx * by - 1) / (bx * by);
  if (bz > a.per_line) bz = a.per_line;
  if (bz > 64) bz = 64;
  if (bz < 1) bz = 1;
  return dim3((unsigned)bx, (unsigned)by, (unsigned)bz);
}

hipError_t launch_regrid_rows(const RegridArgs& a, hipStream_t st) {
  if (a.n_lines <= 0 || a.per_line <= 0) return hipSuccess;
  const dim3 grid = regrid_grid(a);
  if (a.N <= kRegridLdsN) hipLaunchKernelGGL(k_regrid_rows<true>, grid, dim3(kRegridThreads), 0, st, a);
  else hipLaunchKernelGGL(k_regrid_rows<false>, grid, dim3(kRegridThreads), 0, st, a);
  note_launch((long)grid.x * grid.y * grid.z, kRegridThreads, "ibs::k_regrid_rows<%s>", a.N <= kRegridLdsN ? "true" : "false");
  return hipGetLastError();
}

hipError_t launch_assemble_regrid(const RegridArgs& a, hipStream_t st) {
  if (a.n_lines <= 0 || a.per_line <= 0) return hipSuccess;
  const dim3 grid = regrid_grid(a);
  if (a.N <= kRegridLdsN) hipLaunchKernelGGL(k_assemble_regrid<true>, grid, dim3(kRegridThreads), 0, st, a);
  else hipLaunchKernelGGL(k_assemble_regrid<false>, grid, dim3(kRegridThreads), 0, st, a);
  note_launch((long)grid.x * grid.y * grid.z, kRegridThreads, "ibs::k_assemble_regrid<%s>", a.N <= kRegridLdsN ? "true" : "false");
  return hipGetLastError();
}

}  // namespace ibs
