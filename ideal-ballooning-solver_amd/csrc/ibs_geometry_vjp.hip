// Vector-Jacobian product of the field-line geometry (ibs_geometry.hip): from cotangents of the eight arrays (and of
// dPdrho) back to the per-surface Fourier tables, the per-surface scalars and the line label alpha.  Nothing upstream
// corresponds; the arithmetic differentiated is the reference's vmec_fieldlines (utils.py:359-720) as k_fieldline_geometry
// restates it.
//
// Three kernels, no floating-point atomics, every sum in a fixed order (bitwise repeatable for the same call):
//   k_geo_vjp_points   one lane per grid point: recomputes the forward (phi, the secant solve of utils.py:391-416, the two
//                      Fourier syntheses of utils.py:420-468), runs the metric algebra (utils.py:474-720) backwards, turns the
//                      adjoints of the 19 synthesised quantities into those of theta_vmec and phi by a second pass over the
//                      modes (angle m theta_vmec - n phi), and closes the root solve by the implicit-function theorem.  Writes
//                      kGeoVjpW values per point to the workspace [n_lines][kGeoVjpW][N].
//   k_geo_vjp_modes    one wave per (surface, group of kGeoVjpG modes): its lanes stride over the points of the surface's lines
//                      (lines taken in index order: a ballot over line_surf, no lists), one sincos per (point, mode), and a
//                      butterfly reduction over the wave closes each table entry.
//   k_geo_vjp_reduce   one wave per line (alpha_bar) and one per surface (scal_bar).
// Any mode ordering: no use of the row structure.
#include <hip/hip_runtime.h>
#include "ibs_launch.hpp"
#include "ibs_geometry_vjp.hpp"

namespace ibs {

namespace {

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  return v;
}

}  // namespace

__global__ void __launch_bounds__(64) k_geo_vjp_points(GeoVjpArgs a) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j < a.N) geo_vjp_point(a, blockIdx.y, j);
}

// The points of surface js, in a fixed order: lines by index (a ballot over 64 line_surf entries at a time), grid points of a
// line strided over the lanes.  f(line, j) runs on the lane that owns the point.
template <typename F>
__device__ __forceinline__ void for_points_of_surface(const GeoVjpArgs& a, int js, F&& f) {
  const int lane = threadIdx.x & 63;
  for (int base = 0; base < a.n_lines; base += 64) {
    const int i = base + lane;
    const bool mine = i < a.n_lines && min(max(a.line_surf[i], 0), a.n_surf - 1) == js;
    unsigned long long mask = __ballot(mine);
    while (mask) {
      const int b = __ffsll((long long)mask) - 1;
      mask &= mask - 1;
      const int line = base + b;
      for (int j = lane; j < a.N; j += 64) f(line, j);
    }
  }
}

// table cotangents: tab_bar[col][k] = sum over the surface's points of weight_col(point) * cos | sin(angle_k(point))
__global__ void __launch_bounds__(256) k_geo_vjp_modes(GeoVjpArgs a) {
  constexpr int G = kGeoVjpG;
  const int js = blockIdx.y;
  const int g1 = (a.mnmax + G - 1) / G, g2 = (a.mnmax_nyq + G - 1) / G;
  const int grp = blockIdx.x * 4 + (threadIdx.x >> 6);                         // (wave-uniform)
  if (grp >= g1 + g2) return;
  const int lane = threadIdx.x & 63;
  const size_t N = a.N;
  if (grp < g1) {
    if (!a.tab_mn_bar) return;
    const int k0 = grp * G, n1 = a.mnmax;
    double m[G], n[G], acc[G][6];
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const int k = min(k0 + g, n1 - 1);
      m[g] = a.xm[k]; n[g] = a.xn[k];
#pragma unroll
      for (int c = 0; c < 6; ++c) acc[g][c] = 0.0;
    }
    for_points_of_surface(a, js, [&](int line, int j) {
      const double* W = a.ws + (size_t)line * kGeoVjpW * N + j;
      const double R_b = W[W_R * N], Rs_b = W[W_Rs * N], Rt_b = W[W_Rt * N], Rp_b = W[W_Rp * N];
      const double Zs_b = W[W_Zs * N], Zt_b = W[W_Zt * N], Zp_b = W[W_Zp * N];
      const double ls_b = W[W_ls * N], lt_b = W[W_lt * N], lp_b = W[W_lp * N], w = W[W_w * N];
      const double tv = W[W_tv * N], phi = W[W_phi * N];
#pragma unroll
      for (int g = 0; g < G; ++g) {
        double sa, ca;
        vjp_sincos(m[g] * tv - n[g] * phi, &sa, &ca);
        acc[g][0] += R_b * ca + (n[g] * Rp_b - m[g] * Rt_b) * sa;              // rmnc: R, R_t = -m rmnc sin, R_p = n rmnc sin
        acc[g][1] += (m[g] * Zt_b - n[g] * Zp_b) * ca;                         // zmns: Z_t = m zmns cos, Z_p = -n zmns cos
        acc[g][2] += (m[g] * lt_b - n[g] * lp_b) * ca + w * sa;                // lmns: l_t, l_p and the root solve
        acc[g][3] += Rs_b * ca;                                                // d_rmnc_d_s
        acc[g][4] += Zs_b * sa;                                                // d_zmns_d_s
        acc[g][5] += ls_b * sa;                                                // d_lmns_d_s
      }
    });
    double* out = a.tab_mn_bar + (size_t)js * 6 * n1;
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
      for (int c = 0; c < 6; ++c) {
        const double v = wave_sum(acc[g][c]);
        if (lane == 0 && k0 + g < n1) out[(size_t)c * n1 + k0 + g] = v;
      }
  } else {
    if (!a.tab_nyq_bar) return;
    const int k0 = (grp - g1) * G, n2 = a.mnmax_nyq;
    double m[G], n[G], acc[G][7];
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const int k = min(k0 + g, n2 - 1);
      m[g] = a.xm_nyq[k]; n[g] = a.xn_nyq[k];
#pragma unroll
      for (int c = 0; c < 7; ++c) acc[g][c] = 0.0;
    }
    for_points_of_surface(a, js, [&](int line, int j) {
      const double* W = a.ws + (size_t)line * kGeoVjpW * N + j;
      const double sqg_b = W[W_sqg * N], B_b = W[W_B * N], Bs_b = W[W_Bs * N], Bt_b = W[W_Bt * N], Bp_b = W[W_Bp * N];
      const double Bsup_b = W[W_Bsup * N], Bss_b = W[W_Bss * N], Bst_b = W[W_Bst * N], Bsp_b = W[W_Bsp * N];
      const double tv = W[W_tv * N], phi = W[W_phi * N];
#pragma unroll
      for (int g = 0; g < G; ++g) {
        double sa, ca;
        vjp_sincos(m[g] * tv - n[g] * phi, &sa, &ca);
        acc[g][0] += sqg_b * ca;                                               // gmnc
        acc[g][1] += B_b * ca + (n[g] * Bp_b - m[g] * Bt_b) * sa;              // bmnc: |B|, B_t, B_p
        acc[g][2] += Bs_b * ca;                                                // d_bmnc_d_s
        acc[g][3] += Bsup_b * ca;                                              // bsupvmnc
        acc[g][4] += Bss_b * sa;                                               // bsubsmns
        acc[g][5] += Bst_b * ca;                                               // bsubumnc
        acc[g][6] += Bsp_b * ca;                                               // bsubvmnc
      }
    });
    double* out = a.tab_nyq_bar + (size_t)js * 7 * n2;
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
      for (int c = 0; c < 7; ++c) {
        const double v = wave_sum(acc[g][c]);
        if (lane == 0 && k0 + g < n2) out[(size_t)c * n2 + k0 + g] = v;
      }
  }
}

// blocks [0, n_lines): alpha_bar of a line; blocks [n_lines, n_lines + n_surf): scal_bar of a surface.  One wave each.
__global__ void __launch_bounds__(64) k_geo_vjp_reduce(GeoVjpArgs a) {
  const int lane = threadIdx.x;
  const size_t N = a.N;
  if ((int)blockIdx.x < a.n_lines) {
    if (!a.alpha_bar) return;
    const int line = blockIdx.x;
    const double* W = a.ws + ((size_t)line * kGeoVjpW + W_alpha) * N;
    double acc = 0.0;
    for (int j = lane; j < a.N; j += 64) acc += W[j];
    acc = wave_sum(acc);
    if (lane == 0) a.alpha_bar[line] = acc;
    return;
  }
  if (!a.scal_bar) return;
  const int js = blockIdx.x - a.n_lines;
  double acc[6] = {0, 0, 0, 0, 0, 0};
  for_points_of_surface(a, js, [&](int line, int j) {
    const double* W = a.ws + ((size_t)line * kGeoVjpW + W_scal) * N + j;
#pragma unroll
    for (int c = 0; c < 6; ++c) acc[c] += W[c * N];
  });
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    const double v = wave_sum(acc[c]);
    if (lane == 0) a.scal_bar[6 * js + c] = v;
  }
}

hipError_t launch_geometry_vjp(GeoVjpArgs& a, hipStream_t st) {
  if (!a.plane) a.plane = (size_t)a.n_lines * a.ld;
  hipError_t e = hipSuccess;
  if (a.n_lines > 0) {
    hipLaunchKernelGGL(k_geo_vjp_points, dim3((a.N + 63) / 64, a.n_lines), dim3(64), 0, st, a);
    note_launch((long)((a.N + 63) / 64) * a.n_lines, 64, "ibs::k_geo_vjp_points");
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  if (a.tab_mn_bar || a.tab_nyq_bar) {
    const int groups = (a.mnmax + kGeoVjpG - 1) / kGeoVjpG + (a.mnmax_nyq + kGeoVjpG - 1) / kGeoVjpG;
    hipLaunchKernelGGL(k_geo_vjp_modes, dim3((groups + 3) / 4, a.n_surf), dim3(256), 0, st, a);
    note_launch((long)((groups + 3) / 4) * a.n_surf, 256, "ibs::k_geo_vjp_modes");
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  if (a.alpha_bar || a.scal_bar) {
    hipLaunchKernelGGL(k_geo_vjp_reduce, dim3(a.n_lines + a.n_surf), dim3(64), 0, st, a);
    e = hipGetLastError();
  }
  return e;
}

}  // namespace ibs
