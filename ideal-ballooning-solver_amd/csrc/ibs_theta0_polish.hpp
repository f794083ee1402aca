// Maximising gam over theta0 on one staged field line: the peaks of a coarse row gam[n_theta0], the bracket of a peak and a bounded
// Brent search between the coarse nodes.  ball_scan.py:248-295 has no such step: upstream reads the maximum of a line off the nodes.
// Plain C++ on both sides, no HIP: k_theta0_polish (ibs_kernels.hip) runs the state machine below in every wave, the host entry
// points ibs_theta0_polish_* / ibs_row_peaks_f64 run it on the CPU, and ibs_amd.scan.row_peaks / polish_theta0 restate it in Python.
//
// The rule:
//   beats      w beats v if w > v, or w == v and w has the smaller index; a NaN never beats anything (ibs_scan_peaks.hpp, in 1-D).
//   peak       entry j is a peak if it is not NaN and neither neighbour inside the row beats it.
//   ranking    peaks by value descending, ties by index ascending.  Slot k holds peak k; slots from n_found on repeat slot 0; a row
//              without a peak (no finite entry) has n_found = 0 and node -1 in every slot.
//   bracket    [theta0[j - 1], theta0[j + 1]], cut to the node on a side where the row ends or the neighbour is NaN.  Zero length:
//              the node is the result, nothing is evaluated.  Exactly one side cut: status bit kOneSided.
//   search     Brent's bounded search (parabolic step, golden-section fallback), derivative-free, on the absolute tolerance xtol:
//              it stops on |x - m| <= 2 xtol - (b - a) / 2 or after max_eval <= kMaxEval evaluations (status bit kMaxEvalHit).
//              Two-sided: x = the node, w / v = the better / worse end, e = d = b - a so that the first step is the parabola through
//              the three known values; nothing known is evaluated again.  One-sided: the first point is the golden point next to the
//              node, then x = that point, w = the node, v = the other end.  A non-finite value, and the value of a FAILED evaluation
//              (status bit 0 or 1, however finite), counts as -inf; the status bits are OR-ed into the slot's word.
//   incumbent  the result is the best evaluated point only if its gam is strictly greater than the node's; otherwise the node with
//              the node's gam from the table (status bit kNodeReturned).  The result is never below the coarse row.
// Reverse communication: init() and step() return true while they ask for gam at State::u.  Every statement is written so that a
// compiler may not fuse a product into a sum: the host, the device and the Python restatement request the same points.
#pragma once
#include <cmath>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define IBS_T0P_HD __host__ __device__
#else
#define IBS_T0P_HD
#endif

namespace ibs {
namespace t0p {

constexpr int kMaxSlots = 4;                      // start slots (peaks) per row
constexpr int kMaxEval = 64;                      // the loop bound of a search, whatever the data
constexpr int kNodeReturned = 1 << 10, kMaxEvalHit = 1 << 11, kOneSided = 1 << 12;      // informational status bits
constexpr double kGold = 0.3819660112501051;      // (3 - sqrt 5) / 2

IBS_T0P_HD inline bool beats(double w, int iw, double v, int iv) { return (w > v) | ((w == v) & (iw < iv)); }

IBS_T0P_HD inline bool is_peak(const double* row, int n, int j) {
  const double v = row[j];
  bool beaten = !(v == v);
  if (j > 0) beaten |= beats(row[j - 1], j - 1, v, j);
  if (j + 1 < n) beaten |= beats(row[j + 1], j + 1, v, j);
  return !beaten;
}

// the K <= kMaxSlots best peaks of one row: node [K]; returns n_found.  One pass per slot, the previous pick is the threshold
IBS_T0P_HD inline int row_peaks(const double* row, int n, int K, int* node) {
  double tv = HUGE_VAL;
  int ti = -1, nf = 0;
  for (int r = 0; r < K; ++r) {
    double bv = -HUGE_VAL;
    int bi = -1;
    for (int j = 0; j < n; ++j) {
      const double v = row[j];
      const bool after = (v < tv) | ((v == tv) & (j > ti));                  // ranks strictly after the previous pick
      if (after && is_peak(row, n, j) && (bi < 0 || beats(v, j, bv, bi))) { bv = v; bi = j; }
    }
    if (bi < 0) break;
    node[nf++] = bi; tv = bv; ti = bi;
  }
  for (int r = nf; r < K; ++r) node[r] = nf > 0 ? node[0] : -1;
  return nf;
}

struct State {
  double a, b;                 // the bracket
  double x, w, v, fx, fw, fv;  // best, second best and previous second best point with their values
  double lx;                   // the caller's tag of x (the kernel: the eigenvalue of that solve)
  double d, e;                 // last and last-but-one step
  double u;                    // the point whose value is asked for
  double xn, fn, ln;           // the node, its value from the table and its tag
  double xtol;
  int n_eval, max_eval, status;
  int phase;                   // 0 = finished, 1 = the first point of a one-sided bracket is out, 2 = Brent's loop
};

// the next point of Brent's loop into s.u; false = finished
IBS_T0P_HD inline bool propose(State& s) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  s.phase = 0;
  if (s.n_eval >= s.max_eval) { s.status |= kMaxEvalHit; return false; }
  const double tol1 = s.xtol, tol2 = 2.0 * tol1;
  const double xm = 0.5 * (s.a + s.b);
  if (std::fabs(s.x - xm) <= tol2 - 0.5 * (s.b - s.a)) return false;
  bool parab = false;
  double d = 0.0;
  if (std::fabs(s.e) > tol1) {
    const double r = (s.x - s.w) * (s.fx - s.fv);
    double q = (s.x - s.v) * (s.fx - s.fw);
    double p = (s.x - s.v) * q - (s.x - s.w) * r;
    q = 2.0 * (q - r);
    if (q > 0.0) p = -p;
    q = std::fabs(q);
    const double etemp = s.e;
    // (every test in its positive form: a NaN or a zero denominator falls through to golden section)
    if (std::fabs(p) < std::fabs(0.5 * q * etemp) && p > q * (s.a - s.x) && p < q * (s.b - s.x)) {
      d = p / q;
      const double u = s.x + d;
      if (u - s.a < tol2 || s.b - u < tol2) d = xm >= s.x ? tol1 : -tol1;
      parab = true;
      s.e = s.d;
    }
  }
  if (!parab) {
    s.e = s.x >= xm ? s.a - s.x : s.b - s.x;
    d = kGold * s.e;
  }
  s.d = d;
  s.u = std::fabs(d) >= tol1 ? s.x + d : (d > 0.0 ? s.x + tol1 : s.x - tol1);
  s.n_eval += 1;
  s.phase = 2;
  return true;
}

// lo / hi: the neighbouring nodes and their table values, has_lo / has_hi: false where the bracket is cut to the node.  tag_n: the
// caller's tag of the node.  true = gam at s.u is wanted
IBS_T0P_HD inline bool init(State& s, double lo, double flo, bool has_lo, double hi, double fhi, bool has_hi, double xn, double fn,
                            double tag_n, double xtol, int max_eval) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  s.a = has_lo ? lo : xn; s.b = has_hi ? hi : xn;
  s.xn = xn; s.fn = fn; s.ln = tag_n;
  s.x = xn; s.fx = fn; s.lx = tag_n;
  s.w = s.v = xn; s.fw = s.fv = fn;
  s.d = s.e = 0.0; s.u = xn;
  s.xtol = xtol; s.n_eval = 0; s.max_eval = max_eval; s.status = 0; s.phase = 0;
  if (!(s.b > s.a)) return false;                                  // zero length: the node
  if (has_lo && has_hi) {
    const bool lo_better = flo >= fhi;                             // (ties: the smaller index)
    s.w = lo_better ? lo : hi; s.fw = lo_better ? flo : fhi;
    s.v = lo_better ? hi : lo; s.fv = lo_better ? fhi : flo;
    s.d = s.e = s.b - s.a;
    return propose(s);
  }
  s.status |= kOneSided;
  s.v = has_hi ? hi : lo; s.fv = has_hi ? fhi : flo;               // (w = the node)
  s.u =has_hi ? s.a + kGold * (s.b - s.a) : s.b - kGold * (s.b - s.a);
  s.n_eval = 1;
  s.phase = 1;
  return true;
}

// f = gam at s.u, tag = the caller's tag of that evaluation, eval_status = its status bits 0-1.  A value that is not finite, or that
// comes with a status bit 0 or 1 (a failed evaluation), counts as -inf
IBS_T0P_HD inline bool step(State& s, double f, double tag, int eval_status) {
  if (s.phase == 0) return false;
  s.status |= eval_status & 3;
  const bool failed = (eval_status & 3) != 0;                      // (iteration cap or invalid data: its gam is not trusted)
  const double fu = (!failed && f == f && std::fabs(f) <= 1.7976931348623157e308) ? f : -HUGE_VAL;
  const double u = s.u;
  if (s.phase == 1) {
    s.x = u; s.fx = fu; s.lx = tag;                                // (w = the node, v = the other end: init)
    s.d = s.e = s.b - s.a;
    return propose(s);
  }
  if (fu >= s.fx) {
    if (u >= s.x) s.a = s.x; else s.b = s.x;
    s.v = s.w; s.fv = s.fw; s.w = s.x; s.fw = s.fx; s.x = u; s.fx = fu; s.lx = tag;
  } else {
    if (u < s.x) s.a = u; else s.b = u;
    if (fu >= s.fw || s.w == s.x) { s.v = s.w; s.fv = s.fw; s.w = u; s.fw = fu; }
    else if (fu >= s.fv || s.v == s.x || s.v == s.w) { s.v = u; s.fv = fu; }
  }
  return propose(s);
}

// the incumbent rule: (theta0*, gam*, tag*) and the status word of a finished search
IBS_T0P_HD inline void result(const State& s, double& x, double& f, double& tag, int& status) {
  const bool better = s.fx > s.fn;
  x = better ? s.x : s.xn; f = better ? s.fx : s.fn; tag = better ? s.lx : s.ln;
  status = s.status | (better ? 0 : kNodeReturned);
}

// The search of node j of a row set up from the row itself: the bracket rule above.  true = gam at s.u is wanted
IBS_T0P_HD inline bool init_row(State& s, const double* theta0, const double* row, int n, int j, double tag_n, double xtol,
                                int max_eval) {
  const bool has_lo = j > 0 && row[j - 1] == row[j - 1], has_hi = j + 1 < n && row[j + 1] == row[j + 1];
  return init(s, has_lo ? theta0[j - 1] : theta0[j], has_lo ? row[j - 1] : row[j], has_lo, has_hi ? theta0[j + 1] : theta0[j],
              has_hi ? row[j + 1] : row[j], has_hi, theta0[j], row[j], tag_n, xtol, max_eval);
}

// finite and strictly increasing
IBS_T0P_HD inline bool grid_ok(const double* theta0, int n) {
  bool ok = true;
  for (int j = 0; j < n; ++j) {
    const double t = theta0[j];
    ok &= (t == t) && std::fabs(t) <= 1.7976931348623157e308;
    if (j > 0) ok &= t > theta0[j - 1];
  }
  return ok;
}

}  // namespace t0p
}  // namespace ibs
