// Per-point part of the alpha-tangent of the field-line geometry (ibs_geometry_tangent.hip): d/d alpha of the eight arrays at one
// grid point of one line, by forward-mode differentiation of the plain form that geo_vjp_point recomputes.
#pragma once
#include <cmath>
#include "ibs_launch.hpp"
#include "ibs_geometry_vjp.hpp"

namespace ibs {

// a value and its derivative in alpha
struct Dual { double v, d; };
__host__ __device__ inline Dual operator+(const Dual& a, const Dual& b) { return Dual{a.v + b.v, a.d + b.d}; }
__host__ __device__ inline Dual operator-(const Dual& a, const Dual& b) { return Dual{a.v - b.v, a.d - b.d}; }
__host__ __device__ inline Dual operator*(const Dual& a, const Dual& b) { return Dual{a.v * b.v, a.d * b.v + a.v * b.d}; }
__host__ __device__ inline Dual operator*(double s, const Dual& a) { return Dual{s * a.v, s * a.d}; }
__host__ __device__ inline Dual operator+(double s, const Dual& a) { return Dual{s + a.v, a.d}; }
__host__ __device__ inline Dual recip(const Dual& a) { const double r = 1.0 / a.v; return Dual{r, -a.d * r * r}; }
struct DV3 { Dual x, y, z; };
__host__ __device__ inline DV3 cross(const DV3& a, const DV3& b) { return DV3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__host__ __device__ inline Dual dot(const DV3& a, const DV3& b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__host__ __device__ inline DV3 operator*(const Dual& s, const DV3& a) { return DV3{s * a.x, s * a.y, s * a.z}; }
__host__ __device__ inline DV3 operator*(double s, const DV3& a) { return DV3{s * a.x, s * a.y, s * a.z}; }
__host__ __device__ inline DV3 operator+(const DV3& a, const DV3& b) { return DV3{a.x + b.x, a.y + b.y, a.z + b.z}; }

// One grid point: forward recomputed as geo_vjp_point does (one sincos per mode, the forward's secant, GEO_TAIL), every synthesised
// sum together with its two angular partial sums in ONE pass over the modes (S' = S_theta theta_vmec' + S_phi phi', the root's
// theta_vmec' being known only once l_t and l_p are complete), then the metric algebra on (value, tangent) pairs.  Plain C++ (host
// and device): the arithmetic can be checked on a CPU.
__host__ __device__ inline void geo_dalpha_point(const GeoDalphaArgs& a, int line, int j) {
  const int ls_raw = a.line_surf[line];
  const int js = ls_raw < 0 ? 0 : (ls_raw >= a.n_surf ? a.n_surf - 1 : ls_raw);
  const double* sc = a.scal + 6 * js;
  const double s = sc[0], iota = sc[1], diota = sc[2], dp = sc[3], phiedge = sc[4], L = sc[5];
  const double alpha = a.line_alpha[line];
  const double tp = a.theta[j];
  const double phi = (tp - alpha) / iota;                                    // utils.py:373 (phi_center = 0)
  const double dphi = -1.0 / iota;
  const int n1 = a.mnmax, n2 = a.mnmax_nyq;
  const double* rmnc = a.tab_mn + (size_t)js * 6 * n1;
  const double* zmns = rmnc + n1; const double* lmns = zmns + n1;
  const double* drmnc = lmns + n1; const double* dzmns = drmnc + n1; const double* dlmns = dzmns + n1;
  const double tv = geo_theta_vmec(a.xm, a.xn, lmns, n1, tp, phi);                 // the forward's secant, utils.py:391-416
  // ---- the non-Nyquist sums with their theta_vmec (_t) and phi (_p) partial sums      utils.py:420-468
  // (angle m theta_vmec - n phi: d cos / d theta_vmec = -m sin, d cos / d phi = n sin, d sin / d theta_vmec = m cos, d sin / d phi = -n cos;
  //  R_t and R_p are R's own two partial sums, and likewise for l and |B|)
  double R = 0, R_s = 0, R_t = 0, R_p = 0, Z_s = 0, Z_t = 0, Z_p = 0, l_s = 0, l_t = 0, l_p = 0;
  double R_st = 0, R_sp = 0, R_tt = 0, R_tp = 0, R_pp = 0, Z_st = 0, Z_sp = 0, Z_tt = 0, Z_tp = 0, Z_pp = 0;
  double l_st = 0, l_sp = 0, l_tt = 0, l_tp = 0, l_pp = 0;
  for (int k = 0; k < n1; ++k) {
    const double m = a.xm[k], n = a.xn[k];
    double sa, ca;
    vjp_sincos(m * tv - n * phi, &sa, &ca);
    const double ms = m * sa, ns = n * sa, mc = m * ca, nc = n * ca;
    R += rmnc[k] * ca; R_s += drmnc[k] * ca; R_t -= rmnc[k] * ms; R_p += rmnc[k] * ns;
    Z_s += dzmns[k] * sa; Z_t += zmns[k] * mc; Z_p -= zmns[k] * nc;
    l_s += dlmns[k] * sa; l_t += lmns[k] * mc; l_p -= lmns[k] * nc;
    R_st -= drmnc[k] * ms; R_sp += drmnc[k] * ns;
    R_tt -= rmnc[k] * (m * mc); R_tp += rmnc[k] * (m * nc); R_pp -= rmnc[k] * (n * nc);
    Z_st += dzmns[k] * mc; Z_sp -= dzmns[k] * nc;
    Z_tt -= zmns[k] * (m * ms); Z_tp += zmns[k] * (m * ns); Z_pp -= zmns[k] * (n * ns);
    l_st += dlmns[k] * mc; l_sp -= dlmns[k] * nc;
    l_tt -= lmns[k] * (m * ms); l_tp += lmns[k] * (m * ns); l_pp -= lmns[k] * (n * ns);
  }
  // ---- root solve, implicit-function theorem at theta_vmec + Lambda(theta_vmec, phi) = theta_pest        utils.py:391-416
  const double dtv = -l_p * dphi / (1 + l_t);
  auto tan2 = [&](double v, double v_t, double v_p) { return Dual{v, v_t * dtv + v_p * dphi}; };
  const Dual dR = tan2(R, R_t, R_p), dR_s = tan2(R_s, R_st, R_sp), dR_t = tan2(R_t, R_tt, R_tp), dR_p = tan2(R_p, R_tp, R_pp);
  const Dual dZ_s = tan2(Z_s, Z_st, Z_sp), dZ_t = tan2(Z_t, Z_tt, Z_tp), dZ_p = tan2(Z_p, Z_tp, Z_pp);
  const Dual dl_s = tan2(l_s, l_st, l_sp), dl_t = tan2(l_t, l_tt, l_tp), dl_p = tan2(l_p, l_tp, l_pp);
  // ---- the Nyquist sums
  const double* gmnc = a.tab_nyq + (size_t)js * 7 * n2;
  const double* bmnc = gmnc + n2; const double* dbmnc = bmnc + n2;
  const double* bsupv = dbmnc + n2; const double* bsubs = bsupv + n2;
  const double* bsubu = bsubs + n2; const double* bsubv = bsubu + n2;
  double sqg = 0, modB = 0, B_s = 0, B_t = 0, B_p = 0, Bsup_phi = 0, Bsub_s = 0, Bsub_t = 0, Bsub_p = 0;
  double sqg_t = 0, sqg_p = 0, B_st = 0, B_sp = 0, B_tt = 0, B_tp = 0, B_pp = 0, Bsup_t = 0, Bsup_p = 0;
  double Bss_t = 0, Bss_p = 0, Bst_t = 0, Bst_p = 0, Bsp_t = 0, Bsp_p = 0;
  for (int k = 0; k < n2; ++k) {
    const double m = a.xm_nyq[k], n = a.xn_nyq[k];
    double sa, ca;
    vjp_sincos(m * tv - n * phi, &sa, &ca);
    const double ms = m * sa, ns = n * sa, mc = m * ca, nc = n * ca;
    sqg += gmnc[k] * ca; modB += bmnc[k] * ca; B_s += dbmnc[k] * ca;
    B_t -= bmnc[k] * ms; B_p += bmnc[k] * ns;
    Bsup_phi += bsupv[k] * ca; Bsub_s += bsubs[k] * sa; Bsub_t += bsubu[k] * ca; Bsub_p += bsubv[k] * ca;
    sqg_t -= gmnc[k] * ms; sqg_p += gmnc[k] * ns;
    B_st -= dbmnc[k] * ms; B_sp += dbmnc[k] * ns;
    B_tt -= bmnc[k] * (m * mc); B_tp += bmnc[k] * (m * nc); B_pp -= bmnc[k] * (n * nc);
    Bsup_t -= bsupv[k] * ms; Bsup_p += bsupv[k] * ns;
    Bss_t += bsubs[k] * mc; Bss_p -= bsubs[k] * nc;
    Bst_t -= bsubu[k] * ms; Bst_p += bsubu[k] * ns;
    Bsp_t -= bsubv[k] * ms; Bsp_p += bsubv[k] * ns;
  }
  const Dual dsqg = tan2(sqg, sqg_t, sqg_p), dmodB = tan2(modB, B_t, B_p), dB_s = tan2(B_s, B_st, B_sp);
  const Dual dB_t = tan2(B_t, B_tt, B_tp), dB_p = tan2(B_p, B_tp, B_pp), dBsup = tan2(Bsup_phi, Bsup_t, Bsup_p);
  const Dual dBss = tan2(Bsub_s, Bss_t, Bss_p), dBst = tan2(Bsub_t, Bst_t, Bst_p), dBsp = tan2(Bsub_p, Bsp_t, Bsp_p);
  // ---- metric algebra in tangent form (GEO_TAIL of ibs_geometry.hip)         utils.py:474-720
  const double etf = -phiedge / (2 * M_PI);
  double sp0, cp0;
  sincos(phi, &sp0, &cp0);
  const Dual sp{sp0, cp0 * dphi}, cp{cp0, -sp0 * dphi};
  const DV3 e_t{dR_t * cp, dR_t * sp, dZ_t}, e_p{dR_p * cp - dR * sp, dR_p * sp + dR * cp, dZ_p}, e_s{dR_s * cp, dR_s * sp, dZ_s};
  const Dual isg = recip(dsqg);
  const DV3 gs = isg * cross(e_t, e_p), gt = isg * cross(e_p, e_s), gp = isg * cross(e_s, e_t);
  const Dual ls = dl_s - Dual{phi * diota, dphi * diota}, c1 = 1.0 + dl_t, c2 = -iota + dl_p;
  const DV3 ga = ls * gs + (c1 * gt + c2 * gp);
  const DV3 ps = etf * gs;
  const Dual V = dBss * dB_t * c2 + dBst * dB_p * ls + dBsp * dB_s * c1 - dBsp * dB_t * ls - dBst * dB_s * c2 - dBss * dB_p * c1;
  const Dual BA = V * isg;
  const Dual Wp = dBst * dB_p - dBsp * dB_t;
  const Dual BP = etf * (Wp * isg);
  const double Bref = 2 * fabs(etf) / (L * L);
  const double sgn = etf > 0 ? 1.0 : (etf < 0 ? -1.0 : 0.0);              // (a constant: d|etf| plays no part in alpha)
  const double sq = sqrt(s);
  const double shat = (-2 * s / iota) * diota;
  const Dual iB = recip(dmodB), iB3 = iB * iB * iB;
  const double mu0 = 4 * M_PI * 1.0e-7;
  const Dual bmag = (1.0 / Bref) * dmodB;
  const Dual gradpar = (L * iota) * (dBsup * iB);
  const Dual A2 = dot(ga, ga), A21 = dot(ga, ps), A22 = dot(ps, ps);
  const Dual gds2 = (L * L * s) * A2;
  const Dual gds21 = (shat / Bref) * A21;
  const Dual gds22 = (shat * shat / (L * L * Bref * Bref * s)) * A22;
  const Dual G0 = (-2.0 * sgn) * iB3;
  const Dual gbdrift = (Bref * L * L * sq) * (G0 * BA);
  const Dual gbdrift0 = (shat / sq) * (G0 * BP);
  const Dual T = (Bref * L * L * sq * dp * 2 * mu0 * sgn / etf) * (iB * iB);   // cvdrift = gbdrift - T
  const Dual cvdrift = gbdrift - T;
  const double all8 = bmag.v + gradpar.v + gds2.v + gds21.v + gds22.v + gbdrift.v + gbdrift0.v + T.v;
  const bool finite = all8 - all8 == 0.0;                                    // neither infinite nor NaN
  const size_t plane = a.plane;
  double* out = a.geo_da + (size_t)line * a.ld + j;
  const double nan = __builtin_nan("");
  out[0] = finite ? bmag.d : nan; out[plane] = finite ? gradpar.d : nan; out[2 * plane] = finite ? cvdrift.d : nan;
  out[3 * plane] = finite ? gbdrift0.d : nan; out[4 * plane] = finite ? gds2.d : nan; out[5 * plane] = finite ? gds21.d : nan;
  out[6 * plane] = finite ? gds22.d : nan; out[7 * plane] = finite ? gbdrift.d : nan;
}

}  // namespace ibs
