// Per-point part of the vector-Jacobian product of the field-line geometry (ibs_geometry_vjp.hip).
#pragma once
#include <cmath>
#include "ibs_launch.hpp"

namespace ibs {

// workspace slots of one point
enum {
  W_R = 0, W_Rs, W_Rt, W_Rp, W_Zs, W_Zt, W_Zp, W_ls, W_lt, W_lp,           // adjoints of the non-Nyquist sums
  W_sqg, W_B, W_Bs, W_Bt, W_Bp, W_Bsup, W_Bss, W_Bst, W_Bsp,              // adjoints of the Nyquist sums
  W_w,                                                                     // -theta_vmec_bar / (1 + l_t): weight of sin(angle) in lmns_bar
  W_tv, W_phi,                                                             // the angles' two factors
  W_alpha,                                                                 // -phi_bar / iota
  W_scal                                                                   // 6: s iota d_iota_d_s d_pressure_d_s phiedge Aminor_p
};
static_assert(W_scal + 6 == kGeoVjpW, "workspace slots");

// sin and cos: for |x| < 1e5 (every angle of a VMEC table on a ballooning grid) the Cody-Waite reduction by pi/2 in three 33-bit
// pieces and the fdlibm kernels on [-pi/4, pi/4] that the forward row kernels use (geo_sincos in ibs_geometry.hip: ~1 ulp, a
// third of the instructions of the general-range routine); beyond, the library's.
__host__ __device__ inline void vjp_sincos(double x, double* sn, double* cs) {
  if (!(fabs(x) < 1.0e5)) { sincos(x, sn, cs); return; }
  const double k = rint(x * 6.36619772367581382433e-01);
  double r = fma(-k, 1.57079632673412561417e+00, x);
  r = fma(-k, 6.07710050650619224932e-11, r);
  r = fma(-k, 2.02226624879595063154e-21, r);
  const double z = r * r;
  double ps = fma(z, 1.58969099521155010221e-10, -2.50507602534068634195e-08);
  ps = fma(z, ps, 2.75573137070700676789e-06); ps = fma(z, ps, -1.98412698298579493134e-04);
  ps = fma(z, ps, 8.33333333332248946124e-03); ps = fma(z, ps, -1.66666666666666324348e-01);
  const double s = fma(z * r, ps, r);
  double pc = fma(z, -1.13596475577881948265e-11, 2.08757232129817482790e-09);
  pc = fma(z, pc, -2.75573143513906633035e-07); pc = fma(z, pc, 2.48015872894767294178e-05);
  pc = fma(z, pc, -1.38888888888741095749e-03); pc = fma(z, pc, 4.16666666666666019037e-02);
  const double c = fma(z * z, pc, fma(-0.5, z, 1.0));
  const int q = (int)k;
  const double s1 = (q & 1) ? c : s, c1 = (q & 1) ? s : c;
  *sn = (q & 2) ? -s1 : s1;
  *cs = ((q + 1) & 2) ? -c1 : c1;
}

struct V3 { double x, y, z; };
__host__ __device__ inline V3 cross(const V3& a, const V3& b) { return V3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__host__ __device__ inline double dot(const V3& a, const V3& b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__host__ __device__ inline V3 operator*(double s, const V3& a) { return V3{s * a.x, s * a.y, s * a.z}; }
__host__ __device__ inline V3 operator+(const V3& a, const V3& b) { return V3{a.x + b.x, a.y + b.y, a.z + b.z}; }

// theta_vmec of one grid point: the forward's secant from (theta_p, theta_p + 0.1)       utils.py:391-416
__host__ __device__ inline double geo_theta_vmec(const double* xm, const double* xn, const double* lmns, int n1, double tp, double phi) {
  auto resid = [&](double tv) {
    double acc = 0.0;
    for (int k = 0; k < n1; ++k) {
      double sa, ca;
      vjp_sincos(xm[k] * tv - xn[k] * phi, &sa, &ca);
      acc += lmns[k] * sa;
    }
    return tp - (tv + acc);
  };
  double p0 = tp, p1 = tp + 0.1;
  double q0 = resid(p0), q1 = resid(p1);
  bool last = false;
  for (int it = 0; it < 40; ++it) {
    const double den = q1 - q0;
    if (den == 0.0) break;
    const double step = q1 * (p1 - p0) / den;
    p0 = p1; q0 = q1;
    p1 = p1 - step;
    if (last) break;
    last = fabs(step) <= 1e-9 * fmax(1.0, fabs(p1));
    q1 = resid(p1);
  }
  return p1;
}

// One grid point: forward recomputed, reverse pass, workspace written.  Plain C++ (host and device): the arithmetic can be
// checked on a CPU.
__host__ __device__ inline void geo_vjp_point(const GeoVjpArgs& a, int line, int j) {
  const int ls_raw = a.line_surf[line];
  const int js = ls_raw < 0 ? 0 : (ls_raw >= a.n_surf ? a.n_surf - 1 : ls_raw);
  const double* sc = a.scal + 6 * js;
  const double s = sc[0], iota = sc[1], diota = sc[2], dp = sc[3], phiedge = sc[4], L = sc[5];
  const double alpha = a.line_alpha[line];
  const double tp = a.theta[j];
  const double phi = (tp - alpha) / iota;                                    // utils.py:373 (phi_center = 0)
  const int n1 = a.mnmax, n2 = a.mnmax_nyq;
  const double* rmnc = a.tab_mn + (size_t)js * 6 * n1;
  const double* zmns = rmnc + n1; const double* lmns = zmns + n1;
  const double* drmnc = lmns + n1; const double* dzmns = drmnc + n1; const double* dlmns = dzmns + n1;
  const double tv = geo_theta_vmec(a.xm, a.xn, lmns, n1, tp, phi);
  // ---- forward syntheses                                                    utils.py:420-468
  double R = 0, R_s = 0, R_t = 0, R_p = 0, Z_s = 0, Z_t = 0, Z_p = 0, l_s = 0, l_t = 0, l_p = 0;
  for (int k = 0; k < n1; ++k) {
    const double m = a.xm[k], n = a.xn[k];
    double sa, ca;
    vjp_sincos(m * tv - n * phi, &sa, &ca);
    R += rmnc[k] * ca; R_s += drmnc[k] * ca; R_t -= rmnc[k] * m * sa; R_p += rmnc[k] * n * sa;
    Z_s += dzmns[k] * sa; Z_t += zmns[k] * m * ca; Z_p -= zmns[k] * n * ca;
    l_s += dlmns[k] * sa; l_t += lmns[k] * m * ca; l_p -= lmns[k] * n * ca;
  }
  const double* gmnc = a.tab_nyq + (size_t)js * 7 * n2;
  const double* bmnc = gmnc + n2; const double* dbmnc = bmnc + n2;
  const double* bsupv = dbmnc + n2; const double* bsubs = bsupv + n2;
  const double* bsubu = bsubs + n2; const double* bsubv = bsubu + n2;
  double sqg = 0, modB = 0, B_s = 0, B_t = 0, B_p = 0, Bsup_phi = 0, Bsub_s = 0, Bsub_t = 0, Bsub_p = 0;
  for (int k = 0; k < n2; ++k) {
    const double m = a.xm_nyq[k], n = a.xn_nyq[k];
    double sa, ca;
    vjp_sincos(m * tv - n * phi, &sa, &ca);
    sqg += gmnc[k] * ca; modB += bmnc[k] * ca; B_s += dbmnc[k] * ca;
    B_t -= bmnc[k] * m * sa; B_p += bmnc[k] * n * sa;
    Bsup_phi += bsupv[k] * ca; Bsub_s += bsubs[k] * sa; Bsub_t += bsubu[k] * ca; Bsub_p += bsubv[k] * ca;
  }
  // ---- metric algebra forward (GEO_TAIL of ibs_geometry.hip)                utils.py:474-720
  const double etf = -phiedge / (2 * M_PI);
  double sp, cp;
  sincos(phi, &sp, &cp);
  const V3 e_t{R_t * cp, R_t * sp, Z_t}, e_p{R_p * cp - R * sp, R_p * sp + R * cp, Z_p}, e_s{R_s * cp, R_s * sp, Z_s};
  const double isg = 1.0 / sqg;
  const V3 Gs = cross(e_t, e_p), Gt = cross(e_p, e_s), Gp = cross(e_s, e_t);
  const V3 gs = isg * Gs, gt = isg * Gt, gp = isg * Gp;
  const double ls = l_s - phi * diota, c1 = 1 + l_t, c2 = -iota + l_p;
  const V3 ga = ls * gs + (c1 * gt + c2 * gp);
  const V3 ps = etf * gs;
  const double V = Bsub_s * B_t * c2 + Bsub_t * B_p * ls + Bsub_p * B_s * c1 - Bsub_p * B_t * ls - Bsub_t * B_s * c2 - Bsub_s * B_p * c1;
  const double BA = V * isg;
  const double Wp = Bsub_t * B_p - Bsub_p * B_t;
  const double BP = Wp * isg * etf;
  const double Bref = 2 * fabs(etf) / (L * L);
  const double sgn = etf > 0 ? 1.0 : (etf < 0 ? -1.0 : 0.0);
  const double sq = sqrt(s);
  const double shat = (-2 * s / iota) * diota;
  const double iB = 1.0 / modB, iB3 = iB * iB * iB;
  const double mu0 = 4 * M_PI * 1.0e-7;
  const double bmag = modB / Bref;
  const double gradpar = L * (iota * Bsup_phi) * iB;
  const double A2 = dot(ga, ga), A21 = dot(ga, ps), A22 = dot(ps, ps);
  const double gds2 = A2 * L * L * s;
  const double gds21 = A21 * shat / Bref;
  const double F22 = shat * shat / (L * L * Bref * Bref * s);
  const double gds22 = A22 * F22;
  const double G0 = -2.0 * sgn * iB3;
  const double gbdrift = G0 * Bref * L * L * sq * BA;
  const double gbdrift0 = G0 * BP * shat / sq;
  const double T0 = 2 * mu0 * sgn / (etf * modB * modB);
  const double T = Bref * L * L * sq * dp * T0;                                // cvdrift = gbdrift - T
  const double all8 = bmag + gradpar + gds2 + gds21 + gds22 + gbdrift + gbdrift0 + T;
  const bool finite = all8 - all8 == 0.0;                                    // neither infinite nor NaN
  // ---- cotangents of the eight arrays, dPdrho folded in                      ball_scan.py:262
  const size_t o = (size_t)line * a.ld + j, plane = a.plane;
  double b0 = a.geo_bar[o], b1 = a.geo_bar[plane + o], b2 = a.geo_bar[2 * plane + o], b3 = a.geo_bar[3 * plane + o];
  const double b4 = a.geo_bar[4 * plane + o], b5 = a.geo_bar[5 * plane + o], b6 = a.geo_bar[6 * plane + o];
  double b7 = a.geo_bar[7 * plane + o];
  if (a.dPdrho_bar) {
    const double c = a.dPdrho_bar[line] * (-0.5 / a.N);                        // dPdrho = -0.5 mean((cvdrift - gbdrift) bmag^2)
    b2 += c * bmag * bmag; b7 -= c * bmag * bmag; b0 += c * (-T) * 2 * bmag;
  }
  // ---- metric algebra backwards
  double s_b = 0, iota_b = 0, diota_b = 0, dp_b = 0, etf_b = 0, L_b = 0, Bref_b = 0, sq_b = 0, shat_b = 0, phi_b = 0;
  double modB_b = b0 / Bref; Bref_b -= b0 * bmag / Bref;
  L_b += b1 * iota * Bsup_phi * iB; iota_b += b1 * L * Bsup_phi * iB;
  const double Bsup_b = b1 * L * iota * iB; modB_b -= b1 * gradpar * iB;
  const double gb_b = b7 + b2, T_b = -b2;
  Bref_b += T_b * L * L * sq * dp * T0; L_b += T_b * Bref * 2 * L * sq * dp * T0; sq_b += T_b * Bref * L * L * dp * T0;
  dp_b += T_b * Bref * L * L * sq * T0; etf_b -= T_b * T / etf; modB_b -= 2 * T_b * T * iB;
  Bref_b += gb_b * G0 * L * L * sq * BA; L_b += gb_b * G0 * Bref * 2 * L * sq * BA; sq_b += gb_b * G0 * Bref * L * L * BA;
  const double BA_b = gb_b * G0 * Bref * L * L * sq; modB_b -= 3 * gb_b * gbdrift * iB;
  const double BP_b = b3 * G0 * shat / sq; shat_b += b3 * G0 * BP / sq; sq_b -= b3 * gbdrift0 / sq; modB_b -= 3 * b3 * gbdrift0 * iB;
  V3 ga_b = (b4 * L * L * s * 2) * ga; L_b += b4 * A2 * 2 * L * s; s_b += b4 * A2 * L * L;
  const double k21 = b5 * shat / Bref;
  ga_b = ga_b + k21 * ps; V3 ps_b = k21 * ga; shat_b += b5 * A21 / Bref; Bref_b -= b5 * gds21 / Bref;
  ps_b = ps_b + (b6 * F22 * 2) * ps; shat_b += b6 * A22 * 2 * shat / (L * L * Bref * Bref * s);
  L_b -= 2 * b6 * gds22 / L; Bref_b -= 2 * b6 * gds22 / Bref; s_b -= b6 * gds22 / s;
  s_b += sq_b / (2 * sq);
  s_b += shat_b * (-2 * diota / iota); diota_b += shat_b * (-2 * s / iota); iota_b -= shat_b * shat / iota;
  etf_b += Bref_b * 2 * sgn / (L * L); L_b -= 2 * Bref_b * Bref / L;                  // d|etf| = sgn d etf
  const double Wp_b = BP_b * isg * etf;
  double isg_b = BP_b * Wp * etf; etf_b += BP_b * Wp * isg;
  const double V_b = BA_b * isg; isg_b += BA_b * V;
  const double Bss_b = V_b * (B_t * c2 - B_p * c1);
  const double Bst_b = V_b * (B_p * ls - B_s * c2) + Wp_b * B_p;
  const double Bsp_b = V_b * (B_s * c1 - B_t * ls) - Wp_b * B_t;
  const double Bt_b = V_b * (Bsub_s * c2 - Bsub_p * ls) - Wp_b * Bsub_p;
  const double Bp_b = V_b * (Bsub_t * ls - Bsub_s * c1) + Wp_b * Bsub_t;
  const double Bs_b = V_b * (Bsub_p * c1 - Bsub_t * c2);
  double c2_b = V_b * (Bsub_s * B_t - Bsub_t * B_s), ls_b = V_b * Wp, c1_b = V_b * (Bsub_p * B_s - Bsub_s * B_p);
  V3 gs_b = etf * ps_b; etf_b += dot(ps_b, gs);
  ls_b += dot(ga_b, gs); c1_b += dot(ga_b, gt); c2_b += dot(ga_b, gp);
  gs_b = gs_b + ls * ga_b;
  const V3 gt_b = c1 * ga_b, gp_b = c2 * ga_b;
  const double lt_b0 = c1_b, lp_b0 = c2_b, lsum_b = ls_b;
  iota_b -= c2_b; phi_b -= ls_b * diota; diota_b -= ls_b * phi;
  const V3 Gs_b = isg * gs_b, Gt_b = isg * gt_b, Gp_b = isg * gp_b;
  isg_b += dot(gs_b, Gs) + dot(gt_b, Gt) + dot(gp_b, Gp);
  const double sqg_b = -isg_b * isg * isg;
  const V3 et_b = cross(e_p, Gs_b) + cross(Gp_b, e_s);
  const V3 ep_b = cross(Gs_b, e_t) + cross(e_s, Gt_b);
  const V3 es_b = cross(Gt_b, e_p) + cross(e_t, Gp_b);
  const double Rt_b = et_b.x * cp + et_b.y * sp, Zt_b = et_b.z;
  const double Rs_b = es_b.x * cp + es_b.y * sp, Zs_b = es_b.z;
  const double Rp_b = ep_b.x * cp + ep_b.y * sp, R_b = -ep_b.x * sp + ep_b.y * cp, Zp_b = ep_b.z;
  const double cp_b = et_b.x * R_t + es_b.x * R_s + ep_b.x * R_p + ep_b.y * R;
  const double sp_b = et_b.y * R_t + es_b.y * R_s - ep_b.x * R + ep_b.y * R_p;
  phi_b += sp_b * cp - cp_b * sp;
  const double phiedge_b = -etf_b / (2 * M_PI);
  // ---- angle adjoints: every term's angle is m theta_vmec - n phi (second angular derivatives of the sums)
  double tv_b = 0.0;
  for (int k = 0; k < n1; ++k) {
    const double m = a.xm[k], n = a.xn[k];
    double sa, ca;
    vjp_sincos(m * tv - n * phi, &sa, &ca);
    const double wc = rmnc[k] * (n * Rp_b - m * Rt_b) + dzmns[k] * Zs_b + dlmns[k] * lsum_b;            // weight of cos
    const double ws = -rmnc[k] * R_b - drmnc[k] * Rs_b + zmns[k] * (n * Zp_b - m * Zt_b) + lmns[k] * (n * lp_b0 - m * lt_b0);
    const double D = wc * ca + ws * sa;
    tv_b += m * D; phi_b -= n * D;
  }
  for (int k = 0; k < n2; ++k) {
    const double m = a.xm_nyq[k], n = a.xn_nyq[k];
    double sa, ca;
    vjp_sincos(m * tv - n * phi, &sa, &ca);
    const double wc = bmnc[k] * (n * Bp_b - m * Bt_b) + bsubs[k] * Bss_b;
    const double ws = -(gmnc[k] * sqg_b + bmnc[k] * modB_b + dbmnc[k] * Bs_b + bsupv[k] * Bsup_b + bsubu[k] * Bst_b + bsubv[k] * Bsp_b);
    const double D = wc * ca + ws * sa;
    tv_b += m * D; phi_b -= n * D;
  }
  // ---- root solve, implicit-function theorem at theta_vmec + Lambda(theta_vmec, phi) = theta_pest        utils.py:391-416
  const double w = -tv_b / c1;
  phi_b += w * l_p;
  iota_b -= phi * phi_b / iota;                                               // phi = (theta_pest - alpha) / iota
  double* W = a.ws + (size_t)line * kGeoVjpW * a.N + j;
  const size_t N = a.N;
  const double nan = __builtin_nan("");
  auto put = [&](int slot, double v) { W[slot * N] = finite ? v : nan; };
  put(W_R, R_b); put(W_Rs, Rs_b); put(W_Rt, Rt_b); put(W_Rp, Rp_b); put(W_Zs, Zs_b); put(W_Zt, Zt_b); put(W_Zp, Zp_b);
  put(W_ls, lsum_b); put(W_lt, lt_b0); put(W_lp, lp_b0);
  put(W_sqg, sqg_b); put(W_B, modB_b); put(W_Bs, Bs_b); put(W_Bt, Bt_b); put(W_Bp, Bp_b); put(W_Bsup, Bsup_b);
  put(W_Bss, Bss_b); put(W_Bst, Bst_b); put(W_Bsp, Bsp_b);
  put(W_w, w); put(W_tv, tv); put(W_phi, phi);
  put(W_alpha, -phi_b / iota);
  put(W_scal, s_b); put(W_scal + 1, iota_b); put(W_scal + 2, diota_b); put(W_scal + 3, dp_b); put(W_scal + 4, phiedge_b);
  put(W_scal + 5, L_b);
}

}  // namespace ibs
