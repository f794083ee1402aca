// Spectrum mode, clustered modes: an F-orthonormal Ritz basis of every cluster.  A cluster is a run of consecutive modes linked by
// modes_finish's rule (adjacent eigenvalues less than tau = 4 N eps ||A|| apart, the probe below the last mode included): their
// eigenvalues are what the multisection closed, but a twisted factorisation run once per mode at eigenvalues closer than rounding is
// the same factorisation twice -- two members may get one vector.  Here the m <= kMaxModes returned members of a cluster get m
// vectors x_0 .. x_{m-1} with
//   <x_i, x_j>_F = sum_r f_r x_i,r x_j,r = delta_ij to rounding (two passes of modified Gram-Schmidt),
//   x_i^T S x_j = 0 to rounding for i != j (an m x m Rayleigh-Ritz step: the choice is canonical wherever the splitting is resolvable),
//   the Ritz values descending with the mode index,
// every one of them in the cluster's invariant subspace, scaled at the end so that the entry of largest magnitude is +1.
//
//   1. modes_partition     cluster_first[m] = the first mode of m's cluster (m itself: unclustered), from the closed eigenvalues;
//                          returns whether the cluster of mode K - 1 continues below the last mode asked for (an OPEN cluster: its
//                          basis spans part of the subspace).  Status bit 9 alone cannot say this: modes 0-1 and 2-3 may be two
//                          clusters with all four bits set.
//   2. basis::member       inverse iteration as LAPACK's dstein runs it: a deterministic start vector (an integer hash of the row
//                          and the member's index: no state, the same for every system), kBasisIters times { Gram-Schmidt against the
//                          members found so far, normalise, solve (S - sigma_i F) y = F x } at the member's own eigenvalue sigma_i,
//                          by Gaussian elimination with partial pivoting on the tridiagonal rows (dlagtf / dlagts: a tiny pivot is
//                          replaced by eps ||A|| f_r; the solves multiply by the pivots' reciprocals).
//                          Twisting at the m smallest local minima of |gamma_k| -- one factorisation per member and no solve --
//                          is NOT enough: on the double well at N = 2,049 the two best rows lie in
//                          the same well and give one vector twice, and on symmetric triple and quad wells the list of strict
//                          local minima runs out because mirror rows tie.  A solve with the orthogonalisation INSIDE the iteration
//                          cannot stall that way: whatever the start vector has outside the span of the members found so far is
//                          amplified by 1 / |lam_j - sigma_i| >= 1 / (cluster width) against 1 / gap_out for everything else.
//                          A member is refused when its vector is not finite or when the last solve grew the F-norm by less than
//                          1 / (64 tau) -- the residual of the normalised vector is the reciprocal of that growth.
//   3. basis::ritz         H = X^T (S - sigma_0 F) X of the members found (the shift takes the common lam out of every entry: what
//                          is left is the splitting), cyclic Jacobi with a fixed sweep order and count, the Ritz values sorted
//                          descending (ties: the lower index first), X <- X U.
//   4. basis::finish       the entry of largest magnitude +1, zero ends, the FD2/FD4 derivative and the composite Simpson quotient:
//                          the arithmetic of stage 4 of long_vector_growth (ibs_long.hpp), i.e. utils.py:1601-1621.
//
// Plain C++ on both sides (tests/test_modes_basis_cpu.py runs it with a serial wave on written-out rows).  The wave W:
//   int lane(), lanes()                    this lane and their number (device: 64; a serial host wave: 0 and 1)
//   double sum(double), max(double)        over the lanes, in a fixed order, wave-uniform
//   double bcast(double v, int l)          lane l's v, l the same in all lanes
//   void sync()                            what one lane stored, all lanes may read afterwards
//   int N(); double h()                    grid points and spacing; the pencil has n = N - 2 interior rows
//   double g(int j), c(int j), f(int j)    the coefficient rows at grid point j
//   double e(int k)                        half-grid g between grid points k and k + 1, over h^2 (couples interior rows k - 1 and k)
//   double& x(int i, int j), dx(int i, int j)   member i's vector and derivative at grid point j (the caller's X / dX rows)
//   double& ws(int k, int r)               five work rows of N doubles (k = 0 .. 4)
//   double* small()                        2 * kMaxModes * kMaxModes + kMaxModes doubles every lane can reach
// Rows are shared out lane-strided (j = lane, lane + lanes, ..): a lane updates and sums rows of its own only, so those steps need no
// sync; the elimination and the substitutions are serial recurrences the wave steps through a block of lanes() rows at a time.
#pragma once
#include "ibs_modes.hpp"

namespace ibs {

constexpr int kModesBasisBit = 13;       // status bit: the vector is a member of its cluster's Ritz basis (include/ibs.h)
constexpr int kModesOpenBit = 14;        // status bit: the cluster continues below the last mode asked for
constexpr int kBasisIters = 3;           // solves per member (dstein: the growth test passes after one or two, then two more)
constexpr int kBasisJacobiSweeps = 10;   // cyclic sweeps of the m x m Jacobi iteration (m <= 16: converged to rounding after 6-8)
constexpr int kBasisSmallDoubles = 2 * kMaxModes * kMaxModes + kMaxModes;

// cluster_first[0 .. K-1] from the closed eigenvalues lam[0 .. K-1] (modes_finish's midpoints) and the probe's count (-1: not taken);
// returns true when the cluster that holds mode K - 1 is open
IBS_MD_HD inline bool modes_partition(const double* lam, int K, double tau, int probe_count, int* cluster_first) {
  cluster_first[0] = 0;
  for (int m = 1; m < K; ++m) cluster_first[m] = (lam[m - 1] - lam[m] < tau) ? cluster_first[m - 1] : m;
  return probe_count > K;
}

namespace basis {

template <class W> IBS_MD_HD inline double diag(const W& w, int r) { return w.c(r + 1) - (w.e(r) + w.e(r + 1)); }      // d_r as the counts form it

// deterministic start vector: a 32-bit integer hash of (row, member) mapped to [-1, 1)
IBS_MD_HD inline double start_value(int j, int i) {
  unsigned u = (unsigned)j * 2654435761u ^ ((unsigned)(i + 1) * 0x9E3779B9u);
  u ^= u >> 16; u *= 0x85EBCA6Bu; u ^= u >> 13; u *= 0xC2B2AE35u; u ^= u >> 16;
  return (double)(int)u * (1.0 / 2147483648.0);
}

template <class W>
IBS_MD_HD inline double dot_f(W& w, int a, int b) {
  const int N = w.N();
  double s = 0.0;
  for (int j = 1 + w.lane(); j < N - 1; j += w.lanes()) s = __builtin_fma(w.f(j) * w.x(a, j), w.x(b, j), s);
  return w.sum(s);
}

// two passes of modified Gram-Schmidt of member i against the members of `found` (a bit per member, F-orthonormal), then
// normalisation to F-norm 1; returns the F-norm before the normalisation (0 or non-finite: nothing was normalised)
template <class W>
IBS_MD_HD inline double orthonormalise(W& w, int i, unsigned found) {
  const int N = w.N();
  for (int pass = 0; pass < 2; ++pass)
    for (int p = 0; p < kMaxModes; ++p) {
      if (!((found >> p) & 1u)) continue;
      const double s = dot_f(w, p, i);
      for (int j = 1 + w.lane(); j < N - 1; j += w.lanes()) w.x(i, j) = __builtin_fma(-s, w.x(p, j), w.x(i, j));
    }
  const double nn = dot_f(w, i, i);
  const double nrm = __builtin_sqrt(nn);
  if (!(nrm > 0.0) || !(nrm <= 1.7976931348623157e308)) return nrm;
  const double rn = 1.0 / nrm;
  for (int j = 1 + w.lane(); j < N - 1; j += w.lanes()) w.x(i, j) *= rn;
  return nrm;
}

// Gaussian elimination with partial pivoting of S - sigma F (LAPACK dlagtf): ws 0 = the pivots (on return: their reciprocals), 1 =
// the first and 3 = the second superdiagonal of U, 2 = the multipliers, 4 = 1.0 where rows r and r + 1 were interchanged.
// The recurrence is serial in the rows; the wave runs it a block of lanes() rows at a time: lane l loads the operands of row r0 + l
// (coalesced), every lane then steps through the block on the SAME values (w.bcast: the operands of row r0 + u, from lane u) and lane
// u keeps row u's results, which the lanes store together.  So the chain waits for memory once per block, and nothing diverges.
template <class W>
IBS_MD_HD inline void factor(W& w, double sigma, double normA) {
  const int n = w.N() - 2, L = w.lanes(), me = w.lane();
  double a = __builtin_fma(-sigma, w.f(1), diag(w, 0));        // the row being eliminated with: diagonal a, superdiagonal b
  double b = w.e(1);
  for (int r0 = 0; r0 + 1 < n; r0 += L) {
    const int r = r0 + me + 1 < n ? r0 + me : n - 2;
    const double sub_l = w.e(r + 1), e_hi = w.e(r + 2);         // the entry below the diagonal of row r; row r + 1: a1, b1
    const double a1_l = __builtin_fma(-sigma, w.f(r + 2), w.c(r + 2) - (sub_l + e_hi));
    const double b1_l = r + 2 < n ? e_hi : 0.0;
    double o0 = 0.0, o1 = 0.0, o2 = 0.0, o3 = 0.0, o4 = 0.0;
    const int cnt = n - 1 - r0 < L ? n - 1 - r0 : L;
    for (int u = 0; u < cnt; ++u) {
      const double sub = w.bcast(sub_l, u), a1 = w.bcast(a1_l, u), b1 = w.bcast(b1_l, u);
      double p0, p1, p2, p3, p4;
      if (__builtin_fabs(a) >= __builtin_fabs(sub)) {           // no interchange (sub > 0 here: a != 0)
        const double mult = sub / a;
        p0 = a; p1 = b; p3 = 0.0; p2 = mult; p4 = 0.0;
        a = __builtin_fma(-mult, b, a1); b = b1;
      } else {                                                  // rows r and r + 1 change places
        const double mult = a / sub;
        p0 = sub; p1 = a1; p3 = b1; p2 = mult; p4 = 1.0;
        a = __builtin_fma(-mult, a1, b); b = -mult * b1;
      }
      const bool mine = u == me;
      o0 = mine ? p0 : o0; o1 = mine ? p1 : o1; o2 = mine ? p2 : o2; o3 = mine ? p3 : o3; o4 = mine ? p4 : o4;
    }
    if (me < cnt) { w.ws(0, r0 + me) = o0; w.ws(1, r0 + me) = o1; w.ws(2, r0 + me) = o2; w.ws(3, r0 + me) = o3; w.ws(4, r0 + me) = o4; }
  }
  if (me == 0) { w.ws(0, n - 1) = a; w.ws(1, n - 1) = 0.0; w.ws(3, n - 1) = 0.0; w.ws(2, n - 1) = 0.0; w.ws(4, n - 1) = 0.0; }
  w.sync();
  const double tiny = 2.220446049250313e-16 * normA;            // (dlagts, job = -1: a pivot below the rounding of its row is replaced)
  for (int r = me; r < n; r += L) {                             // ... and the pivots become their reciprocals: no division in the solves
    const double floor_r = tiny * w.f(r + 1), p = w.ws(0, r);
    w.ws(0, r) = 1.0 / (!(__builtin_fabs(p) >= floor_r) ? (p < 0.0 ? -floor_r : floor_r) : p);
  }
  w.sync();
}

// x_i <- (S - sigma F)^-1 F x_i from the rows factor() left: the elimination's row operations on the right-hand side, then the back
// substitution, each a serial recurrence run a block of lanes() rows at a time as in factor()
template <class W>
IBS_MD_HD inline void solve(W& w, int i) {
  const int n = w.N() - 2, L = w.lanes(), me = w.lane();
  w.sync();
  double y = w.f(1) * w.x(i, 1);
  for (int r0 = 0; r0 + 1 < n; r0 += L) {
    const int r = r0 + me + 1 < n ? r0 + me : n - 2;
    const double y1_l = w.f(r + 2) * w.x(i, r + 2), mu_l = w.ws(2, r), fl_l = w.ws(4, r);
    double out = 0.0;
    const int cnt = n - 1 - r0 < L ? n - 1 - r0 : L;
    for (int u = 0; u < cnt; ++u) {
      const double y1 = w.bcast(y1_l, u), mu = w.bcast(mu_l, u), fl = w.bcast(fl_l, u);
      double o;
      if (fl == 0.0) { o = y; y = __builtin_fma(-mu, y, y1); }
      else { o = y1; y = __builtin_fma(-mu, y1, y); }
      out = u == me ? o : out;
    }
    if (me < cnt) w.x(i, r0 + me + 1) = out;                    // (row r0 + me + 1 was loaded by lane me - 1 before this store)
  }
  if (me == 0) w.x(i, n) = y;
  w.sync();
  double z1 = 0.0, z2 = 0.0;
  for (int r0 = n - 1; r0 >= 0; r0 -= L) {
    const int r = r0 - me >= 0 ? r0 - me : 0;
    const double y_l = w.x(i, r + 1), u1_l = w.ws(1, r), u2_l = w.ws(3, r), rp_l = w.ws(0, r);
    double out = 0.0;
    const int cnt = r0 + 1 < L ? r0 + 1 : L;
    for (int u = 0; u < cnt; ++u) {
      const double z = (w.bcast(y_l, u) - w.bcast(u1_l, u) * z1 - w.bcast(u2_l, u) * z2) * w.bcast(rp_l, u);
      out = u == me ? z : out;
      z2 = z1; z1 = z;
    }
    if (me < cnt) w.x(i, r0 - me + 1) = out;
  }
  w.sync();
}

// member i of a cluster at its eigenvalue sigma, orthogonal to the members of `found`; false = refused (the row is left as it is)
template <class W>
IBS_MD_HD inline bool member(W& w, int i, double sigma, double normA, double tau, unsigned found) {
  const int N = w.N();
  for (int j = w.lane(); j < N; j += w.lanes()) w.x(i, j) = (j == 0 || j == N - 1) ? 0.0 : start_value(j, i);
  factor(w, sigma, normA);
  double grown = 0.0;
  for (int it = 0; it < kBasisIters; ++it) {
    const double nrm = orthonormalise(w, i, found);
    if (!(nrm > 0.0) || !(nrm <= 1.7976931348623157e308)) return false;
    solve(w, i);
    // scaled into range before the sums of squares (the solve grows a unit vector by up to 1 / (eps ||A|| f))
    double mx = 0.0;
    for (int j = 1 + w.lane(); j < N - 1; j += w.lanes()) mx = __builtin_fmax(mx, __builtin_fabs(w.x(i, j)));
    mx = w.max(mx);
    if (!(mx > 0.0) || !(mx <= 1.7976931348623157e308)) return false;
    const double rm = 1.0 / mx;
    for (int j = 1 + w.lane(); j < N - 1; j += w.lanes()) w.x(i, j) *= rm;
    grown = mx;
  }
  const double nrm = orthonormalise(w, i, found);               // of the last solve's vector over its largest entry: grown * nrm = its F-norm
  w.sync();
  return nrm > 0.0 && nrm <= 1.7976931348623157e308 && grown * nrm * (64.0 * tau) >= 1.0;
}

// the Rayleigh-Ritz step over the members of `found` (bits below m, F-orthonormal): afterwards they are Ritz vectors, Ritz values
// descending with the member index.  H and U are indexed by the member index; a member that was not found has no row or column.
template <class W>
IBS_MD_HD inline void ritz(W& w, int m, unsigned found, double sigma) {
  const int N = w.N();
  if ((found & (found - 1u)) == 0u) return;                     // fewer than two members
  double* H = w.small();
  double* U = H + kMaxModes * kMaxModes;
  auto has = [&](int p) { return ((found >> p) & 1u) != 0u; };
  w.sync();
  for (int a = 0; a < m; ++a)
    for (int b = a; b < m; ++b) {
      if (!has(a) || !has(b)) continue;
      double s = 0.0;
      for (int j = 1 + w.lane(); j < N - 1; j += w.lanes()) {
        const double t = __builtin_fma(__builtin_fma(-sigma, w.f(j), diag(w, j - 1)), w.x(b, j),
                                       __builtin_fma(w.e(j - 1), w.x(b, j - 1), w.e(j) * w.x(b, j + 1)));
        s = __builtin_fma(w.x(a, j), t, s);
      }
      s = w.sum(s);
      if (w.lane() == 0) { H[a * kMaxModes + b] = s; H[b * kMaxModes + a] = s; }
    }
  w.sync();
  if (w.lane() == 0) {
    for (int a = 0; a < m; ++a) for (int b = 0; b < m; ++b) U[a * kMaxModes + b] = a == b ? 1.0 : 0.0;
    for (int sweep = 0; sweep < kBasisJacobiSweeps; ++sweep)
      for (int p = 0; p + 1 < m; ++p)
        for (int q = p + 1; q < m; ++q) {
          if (!has(p) || !has(q)) continue;
          const double hpq = H[p * kMaxModes + q];
          if (hpq == 0.0) continue;
          const double theta = (H[q * kMaxModes + q] - H[p * kMaxModes + p]) / (2.0 * hpq);
          const double t = (theta < 0.0 ? -1.0 : 1.0) / (__builtin_fabs(theta) + __builtin_sqrt(__builtin_fma(theta, theta, 1.0)));
          const double cs = 1.0 / __builtin_sqrt(__builtin_fma(t, t, 1.0)), sn = t * cs;
          for (int k = 0; k < m; ++k) {                         // H <- H J
            if (!has(k)) continue;
            const double hkp = H[k * kMaxModes + p], hkq = H[k * kMaxModes + q];
            H[k * kMaxModes + p] = cs * hkp - sn * hkq; H[k * kMaxModes + q] = sn * hkp + cs * hkq;
          }
          for (int k = 0; k < m; ++k) {                         // H <- J^T H
            if (!has(k)) continue;
            const double hpk = H[p * kMaxModes + k], hqk = H[q * kMaxModes + k];
            H[p * kMaxModes + k] = cs * hpk - sn * hqk; H[q * kMaxModes + k] = sn * hpk + cs * hqk;
          }
          H[p * kMaxModes + q] = 0.0; H[q * kMaxModes + p] = 0.0;
          for (int k = 0; k < m; ++k) {                         // U <- U J
            const double ukp = U[k * kMaxModes + p], ukq = U[k * kMaxModes + q];
            U[k * kMaxModes + p] = cs * ukp - sn * ukq; U[k * kMaxModes + q] = sn * ukp + cs * ukq;
          }
        }
    // column order: the Ritz values descending, on equal values the lower column first (selection sort, columns swapped in place)
    for (int a = 0; a + 1 < m; ++a) {
      if (!has(a)) continue;
      int best = a;
      for (int b = a + 1; b < m; ++b) if (has(b) && H[b * kMaxModes + b] > H[best * kMaxModes + best]) best = b;
      if (best != a) {
        const double t = H[a * kMaxModes + a]; H[a * kMaxModes + a] = H[best * kMaxModes + best]; H[best * kMaxModes + best] = t;
        for (int k = 0; k < m; ++k) { const double u = U[k * kMaxModes + a]; U[k * kMaxModes + a] = U[k * kMaxModes + best]; U[k * kMaxModes + best] = u; }
      }
    }
  }
  w.sync();
  for (int j = 1 + w.lane(); j < N - 1; j += w.lanes()) {       // X <- X U, row by row (the old row in registers: indexed by constants)
    double t[kMaxModes];
IBS_MD_UNROLL
    for (int a = 0; a < kMaxModes; ++a) t[a] = (a < m && has(a)) ? w.x(a, j) : 0.0;
    for (int b = 0; b < m; ++b) {
      if (!has(b)) continue;
      double s = 0.0;
IBS_MD_UNROLL
      for (int a = 0; a < kMaxModes; ++a) if (a < m && has(a)) s = __builtin_fma(t[a], U[a * kMaxModes + b], s);
      w.x(b, j) = s;
    }
  }
  w.sync();
}

// member i scaled so that its entry of largest magnitude is +1, its derivative row, and its growth rate (returned)
template <class W>
IBS_MD_HD inline double finish(W& w, int i) {
  const int N = w.N();
  double m = 0.0, mp = -1e300;
  for (int j = 1 + w.lane(); j < N - 1; j += w.lanes()) { m = __builtin_fmax(m, __builtin_fabs(w.x(i, j))); mp = __builtin_fmax(mp, w.x(i, j)); }
  m = w.max(m); mp = w.max(mp);
  m = mp == m ? m : -m;
  const double rm = 1.0 / m;
  for (int j = w.lane(); j < N; j += w.lanes()) w.x(i, j) = (j == 0 || j == N - 1) ? 0.0 : w.x(i, j) * rm;
  w.sync();
  const double ih = 1.0 / w.h();
  const double A_in = (2.0 / 3.0) * ih, B_in = -ih / 12.0, A_e1 = 0.5 * ih, A_e0 = 2.0 * ih, B_e0 = -0.5 * ih;
  double y0 = 0.0, y1 = 0.0;
  for (int j = w.lane(); j < N; j += w.lanes()) {
    const int jm1 = j > 0 ? j - 1 : 0, jm2 = j > 1 ? j - 2 : 0;
    const int jp1 = j < N - 1 ? j + 1 : N - 1, jp2 = j < N - 2 ? j + 2 : N - 1;
    const double X = w.x(i, j);
    const double d1 = w.x(i, jp1) - w.x(i, jm1), d2 = w.x(i, jp2) - w.x(i, jm2);
    const bool end0 = (j == 0) || (j == N - 1), end1 = (j == 1) || (j == N - 2);
    const double Ac = end0 ? A_e0 : (end1 ? A_e1 : A_in), Bc = end0 ? B_e0 : (end1 ? 0.0 : B_in);
    const double dX = __builtin_fma(Ac, d1, Bc * d2);                               // utils.py:1610-1616
    const double wt = end0 ? 1.0 : ((j & 1) ? 4.0 : 2.0);                           // Simpson weights (the 1/3 cancels)
    const double X2 = wt * (X * X), dX2 = wt * (dX * dX);
    y0 += w.c(j) * X2 - w.g(j) * dX2;                                               // utils.py:1618
    y1 = __builtin_fma(w.f(j), X2, y1);                                             // utils.py:1619
    w.dx(i, j) = dX;
  }
  y0 = w.sum(y0); y1 = w.sum(y1);
  w.sync();
  return y0 / y1;                                                                   // utils.py:1621
}

}  // namespace basis

// The basis of one cluster of m members at the eigenvalues lam[0 .. m-1] (descending): returns the members found as a bit mask
// (all m bits: complete) and gam of those.  The rows x(i, .) / dx(i, .) of a member that was not found are left undefined.
template <class W>
IBS_MD_HD inline unsigned modes_cluster_basis(W& w, int m, const double* lam, double normA, double tau, double* gam) {
  unsigned found = 0;
  for (int i = 0; i < m; ++i)
    if (basis::member(w, i, lam[i], normA, tau, found)) found |= 1u << i;
  basis::ritz(w, m, found, lam[0]);
  for (int i = 0; i < m; ++i)
    if ((found >> i) & 1u) gam[i] = basis::finish(w, i);
  return found;
}

}  // namespace ibs
