// Geometry-fed Sturm counts and the count-pair certificate of geometry-fed growth rates (nothing upstream corresponds to the
// certificate; the count is the isunstable of tests/shifted-circle-s-alpha/bishop_ball_s-alpha.py:110-115 for real field lines).
//
// The scan, objective and refinement kernels close lam_max with the scaled-row shift iteration (WaveSolver::solve) and carry no a-priori
// bound.  This file states one afterwards, independently of that arithmetic: in DIVISION form on the rows of SURVEY Appendix A
// (q_r = (d_r - sig f_r) - e_r^2 / q_{r-1}, IEEE division, the pivot guard of k_sturm_count_div) the number of eigenvalues above
// lam + tol must be 0 and above lam - tol at least 1, tol = tol_factor N eps ||A||, ||A|| = max_r (|d_r| + e_r + e_{r+1}) / f_r.
//
// k_geo_certify: LANES ARE SYSTEMS.  A wave takes 64 consecutive systems -- (line, theta0 index) pairs of a scan, so the theta0 values of
// a line sit on adjacent lanes, or points with a theta0 each -- which lie on 64 / n_theta0 (+1) lines, 64 in the points form.  Chunk by
// chunk of kCertChunk grid points the wave loads the seven geometry rows of those lines (16 lanes per line: one 128-byte segment per
// row and load), reduces them to the theta0-free factors of ball_scan.py:267-268 + utils.py:1560-1562 and leaves them in LDS as
// [line][row][point]; every lane then folds its theta0 and eliminates its rows from LDS -- the lanes of a line read the same address
// (broadcast), lanes on different lines different banks (odd pitch).  A row is eliminated one step late, when g of the next point has
// arrived.  Pass 1 over the line takes ||A|| and validates the data, pass 2 runs the recurrence at both shifts as two independent
// chains; the count form runs one chain at the caller's shift and no pass 1.  The chunk loop makes the kernel independent of N.
// PRE_G > 0: the next chunk's loads (PRE_G groups of four lines) are in flight during the recurrence; waves on more lines load in place.
//
// k_geo_reclose: the systems a certificate refused, listed on the device (k_reclose_list), are solved again by one wave each with the
// long-grid pieces (ibs_long.hpp: bounds, division-form multisection to 2 eps ||A||, twisted-factorisation eigenvector, growth rate) on
// rows the wave writes to its workspace with the arithmetic of k_assemble_gcf_long; k_geo_certify then looks at exactly those again.
#include "ibs_certify.hpp"
#include "ibs_long.hpp"
#include "ibs_geo_line.hpp"
#include "ibs_launch.hpp"

namespace ibs {

constexpr int kCertRaw = 8;      // per staged point: the seven geometry values and the line's dPdrho

template <bool CERT, int PRE_G>
__global__ void __launch_bounds__(64) k_geo_certify(CertifyArgs a, int lw) {
  extern __shared__ __attribute__((aligned(16))) double cert_lds[];
  constexpr double pivmin = 2.2250738585072014e-292;
  constexpr int P = kCertPitch;
  const int lane = threadIdx.x, N = a.N;
  const long n_sys = (long)a.n_lines * a.n_theta0;
  const long base = (long)blockIdx.x * kWave;                           // first system of this wave
  if (base >= n_sys) return;
  const bool active = base + lane < n_sys;
  const long mine = active ? base + lane : n_sys - 1;                   // this lane's system
  const long last = base + kWave - 1 < n_sys ? base + kWave - 1 : n_sys - 1;
  const int line_lo = (int)(base / a.n_theta0);
  const int nl = (int)(last / a.n_theta0) - line_lo + 1;                // lines of this wave (<= lw: launch_cert)
  const int my_line = (int)(mine / a.n_theta0), it0 = (int)(mine - (long)my_line * a.n_theta0);
  const double th0 = a.theta0[a.t0_stride ? my_line : it0], two_th0 = 2.0 * th0, th0sq = th0 * th0;
  const double ih2 = 1.0 / (a.h * a.h);
  int old = 0;
  double lam = 0.0;
  if constexpr (CERT) {
    old = a.cert[mine];
    lam = a.lam[mine];
    if (a.recheck && !__any(active && (old & kCertPending))) return;    // (wave-uniform)
  }
  // ---- staging: loader role = line 4 gi + sub of the wave, point rr of the chunk
  const int sub = lane >> 4, rr = lane & 15;
  const int ng = (nl + 3) >> 2;
  auto load_pt = [&](int gi, int B, double* raw) {
    int l = 4 * gi + sub; l = l < nl ? l : nl - 1;
    int p = kCertChunk * B + rr; p = p > N - 1 ? N - 1 : p;             // (points past the line: masked in the recurrence)
    const long o = (long)(line_lo + l) * a.ld + p;
#pragma unroll
    for (int k = 0; k < 7; ++k) raw[k] = a.geo7[k][o];
    raw[7] = a.dPdrho[line_lo + l];
  };
  auto store_pt = [&](int gi, const double* raw) {                      // the theta0-free factors, as k_assemble_gcf_long forms them
    const int l = 4 * gi + sub;
    if (l < nl && l < lw) {
      const double mdP = -raw[7];
      const double B = raw[0], gp = xabs(raw[1]);
      const double inv = 1.0 / (gp * B);
      double* o = cert_lds + (l * kCertRows) * P + rr;
      o[0] = gp / B; o[P] = inv / (B * B); o[2 * P] = mdP * raw[2] * inv; o[3 * P] = mdP * raw[3] * inv;
      o[4 * P] = raw[4]; o[5 * P] = raw[5]; o[6 * P] = raw[6];
    }
  };
  const double* my = cert_lds + ((my_line - line_lo) * kCertRows) * P;
  const int nB = (N + kCertChunk - 1) / kCertChunk;
  // one pass over the line: row_fn(j, e_lo, e_hi, c_j, f_j, p, g_p, c_p, f_p) for every staged point p, j = p - 1 the row that can be
  // eliminated now (valid for 1 <= j <= N - 2)
  auto sweep = [&](auto&& row_fn) {
    double pre[(PRE_G > 0 ? PRE_G : 1) * kCertRaw];
    if constexpr (PRE_G > 0) {
#pragma unroll
      for (int gi = 0; gi < PRE_G; ++gi) if (gi < ng) load_pt(gi, 0, pre + gi * kCertRaw);
    }
    double gm2 = 0.0, gm1 = 0.0, cprev = 0.0, fprev = 1.0;
    for (int B = 0; B < nB; ++B) {
      wave_lds_sync();                                                   // (the previous chunk has been consumed)
      if constexpr (PRE_G > 0) {
#pragma unroll
        for (int gi = 0; gi < PRE_G; ++gi) if (gi < ng) store_pt(gi, pre + gi * kCertRaw);
      } else {
        for (int gi = 0; gi < ng; ++gi) { load_pt(gi, B, pre); store_pt(gi, pre); }
      }
      wave_lds_sync();
      if constexpr (PRE_G > 0) {
        if (B + 1 < nB) {
#pragma unroll
          for (int gi = 0; gi < PRE_G; ++gi) if (gi < ng) load_pt(gi, B + 1, pre + gi * kCertRaw);
        }
      }
      const int p0 = kCertChunk * B;
#pragma unroll 4
      for (int i = 0; i < kCertChunk; ++i) {
        const double* r = my + i;
        const double d = r[4 * P] + two_th0 * r[5 * P] + th0sq * r[6 * P];          // ball_scan.py:267-268
        const double gp = r[0] * d, cp = r[2 * P] + th0 * r[3 * P], fp = r[P] * d;     // utils.py:1560-1562
        const double e_lo = 0.5 * (gm2 + gm1) * ih2, e_hi = 0.5 * (gm1 + gp) * ih2; // utils.py:1574-1576
        row_fn(p0 + i - 1, e_lo, e_hi, cprev, fprev, p0 + i, gp, cp, fp);
        gm2 = gm1; gm1 = gp; cprev = cp; fprev = fp;
      }
    }
  };
  // ---- pass 1: ||A|| and the data checks
  bool bad = false;
  double sig0, sig1 = 0.0;
  if constexpr (CERT) {
    double vna = 0.0;
    sweep([&](int j, double e_lo, double e_hi, double cj, double fj, int p, double gp, double cp, double fp) {
      const double v = (xabs(cj - (e_lo + e_hi)) + e_lo + e_hi) * (1.0 / fj);
      vna = (j >= 1 && j <= N - 2 && v > vna) ? v : vna;
      bad = bad || (p <= N - 1 && (!(gp > 0.0) || !(fp > 0.0) || !finite_of(gp) || !finite_of(cp) || !finite_of(fp)));
    });
    bad = bad || !finite_of(vna) || !finite_of(lam);
    const double tol = a.tol_factor * (double)N * Eps<double>::v * vna;
    sig0 = lam + tol; sig1 = lam - tol;
  } else {
    sig0 = a.shift[mine];
  }
  // ---- pass 2: the division-form recurrence (k_sturm_count_div's), one chain per shift
  double q0 = 1.0, q1 = 1.0;
  int cnt0 = 0, cnt1 = 0;
  sweep([&](int j, double e_lo, double e_hi, double cj, double fj, int, double, double, double) {
    const bool row = j >= 1 && j <= N - 2;
    const double dd = cj - (e_lo + e_hi), e2 = e_lo * e_lo;                          // utils.py:1584-1592
    {
      const double s = xfma(-sig0, fj, dd);
      double qn = (j == 1) ? s : s - e2 / q0;
      qn = xabs(qn) < pivmin ? -pivmin : qn;
      q0 = row ? qn : q0;
      cnt0 += (row && qn > 0.0) ? 1 : 0;
    }
    if constexpr (CERT) {
      const double s = xfma(-sig1, fj, dd);
      double qn = (j == 1) ? s : s - e2 / q1;
      qn = xabs(qn) < pivmin ? -pivmin : qn;
      q1 = row ? qn : q1;
      cnt1 += (row && qn > 0.0) ? 1 : 0;
    }
  });
  if (!active) return;
  if constexpr (CERT) {
    const int word = bad ? kCertUnchecked : ((cnt0 != 0 ? kCertNotMax : 0) | (cnt1 == 0 ? kCertNoEig : 0));
    if (!a.recheck) a.cert[mine] = word;
    else if (old & kCertPending) a.cert[mine] = word == 0 ? kCertReclosed : (old & ~kCertPending);
  } else {
    a.count[mine] = cnt0;
  }
}

// lines a wave of 64 consecutive systems can touch
static int cert_lines_per_wave(const CertifyArgs& a) {
  long l = (kWave % a.n_theta0 == 0) ? kWave / a.n_theta0 : (kWave - 2 + a.n_theta0) / a.n_theta0 + 1;
  if (l > a.n_lines) l = a.n_lines;
  if (l > kCertMaxLines) l = kCertMaxLines;
  return (int)(l < 1 ? 1 : l);
}

template <bool CERT>
static hipError_t launch_cert(const CertifyArgs& a, hipStream_t st) {
  const long n_sys = (long)a.n_lines * a.n_theta0, nblk = (n_sys + kWave - 1) / kWave;
  const int lw = cert_lines_per_wave(a);
  const size_t lds = cert_lds_bytes(lw);
  if (lw <= 16) {
    hipLaunchKernelGGL((k_geo_certify<CERT, 4>), dim3((unsigned)nblk), dim3(64), lds, st, a, lw);
    note_launch(nblk, 64, "ibs::k_geo_certify<%d, 4>", (int)CERT);
  } else {
    hipLaunchKernelGGL((k_geo_certify<CERT, 0>), dim3((unsigned)nblk), dim3(64), lds, st, a, lw);
    note_launch(nblk, 64, "ibs::k_geo_certify<%d, 0>", (int)CERT);
  }
  return hipGetLastError();
}
hipError_t launch_geo_count(const CertifyArgs& a, hipStream_t st) { return launch_cert<false>(a, st); }
hipError_t launch_geo_certify(const CertifyArgs& a, hipStream_t st) { return launch_cert<true>(a, st); }

// ---- re-close
// list[0] = number of listed systems (zeroed by the launch), list[1 ..] = their indices (any order: each is solved on its own)
__global__ void k_reclose_list(long n_sys, const int* __restrict__ cert, int* list) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_sys) {
    const int w = cert[i];
    if ((w & (kCertNotMax | kCertNoEig)) && !(w & kCertUnchecked)) list[1 + atomicAdd(list, 1)] = (int)i;
  }
}

__global__ void __launch_bounds__(64) k_geo_reclose(RecloseArgs a) {
  __shared__ double lds[3 * kLongChunk];
  const CertifyArgs& s = a.c;
  const int lane = threadIdx.x, N = s.N;
  const double ih2 = 1.0 / (s.h * s.h);
  double* G = a.work + (size_t)blockIdx.x * reclose_ws_doubles(N);
  double* Cc = G + N; double* F = G + 2 * (size_t)N; double* work = G + 3 * (size_t)N;
  const int n_list = a.list[0];
  for (int k = blockIdx.x; k < n_list; k += gridDim.x) {
    const long sys = a.list[1 + k];
    const int line = (int)(sys / s.n_theta0), it0 = (int)(sys - (long)line * s.n_theta0);
    const double th0 = s.theta0[s.t0_stride ? line : it0];
    const double mdP = -s.dPdrho[line];
    const GeoLine7 ln = geo_line7(s.geo7, (long)line * s.ld);
    for (int j = lane; j < N; j += kWave) line_gcf(ln, j, mdP, th0, G[j], Cc[j], F[j]);     // the rows, as k_assemble_gcf_long writes them
    long_fence();
    const SrcLong<double, false> src{G, Cc, F, nullptr};
    const LongBounds b = long_bounds<false>(src, N, ih2, lane);
    double lam = 0.0;
    int passes = 0;
    if (!b.bad && long_lam_max(src, N, ih2, b.lo, b.hi, b.normA, lds, lane, lam, passes)) {
      const double gam = long_vector_growth<false, double>(src, N, s.h, lam, sys, work, a.X, a.dX, lds, lane);
      if (lane == 0) { a.lam[sys] = lam; a.gam[sys] = gam; s.cert[sys] |= kCertPending; }
    }
    long_fence();                                                        // (the workspace is reused by this wave's next system)
  }
}

hipError_t launch_geo_reclose(const RecloseArgs& a, hipStream_t st) {
  const long n_sys = (long)a.c.n_lines * a.c.n_theta0;
  hipError_t e = hipMemsetAsync(a.list, 0, sizeof(int), st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_reclose_list, dim3((unsigned)((n_sys + 255) / 256)), dim3(256), 0, st, n_sys, a.c.cert, a.list);
  hipLaunchKernelGGL(k_geo_reclose, dim3((unsigned)a.n_waves), dim3(64), 0, st, a);
  note_launch(a.n_waves, 64, "ibs::k_geo_reclose");
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  CertifyArgs c = a.c;
  c.lam = a.lam; c.recheck = 1;
  return launch_geo_certify(c, st);
}

}  // namespace ibs
