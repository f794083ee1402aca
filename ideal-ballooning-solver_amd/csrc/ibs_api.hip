// C-ABI layer of libibs_hip.so (declarations and reference citations: include/ibs.h).
#include <hip/hip_runtime.h>

#include <dlfcn.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <limits>
#include <string>
#include <vector>

#include "../../include/ibs.h"
#include "ibs_launch.hpp"
#include "ibs_wave.hpp"
#include "ibs_lbfgsb2.hpp"
#include "ibs_refine.hpp"
#include "ibs_certify.hpp"
#include "ibs_regrid.hpp"
#include "ibs_scan_peaks.hpp"
#include "ibs_theta0_polish.hpp"
#include "ibs_local_eq.hpp"
#include "ibs_local_eq_boundary.hpp"
#include "ibs_local_eq_boundary_polish.hpp"
#include "ibs_local_eq_grad.hpp"
#include <chrono>
#include <thread>

namespace ibs {
LaunchTable& launch_table() {
  static LaunchTable t{};
  return t;
}
LaunchNote& last_launch() {
  static thread_local LaunchNote n{};
  return n;
}
void note_launch(long blocks, int threads, const char* fmt, ...) {
  LaunchNote& n = last_launch();
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(n.name, sizeof(n.name), fmt, ap);
  va_end(ap);
  n.blocks = blocks; n.threads = threads;
}
}  // namespace ibs

static thread_local std::string g_err;
static int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}
#define HIPCHK(expr)                                                                        \
  do {                                                                                      \
    hipError_t e_ = (expr);                                                                 \
    if (e_ != hipSuccess) return fail(IBS_ERR_HIP, "%s -> %s", #expr, hipGetErrorString(e_)); \
  } while (0)

// Diagnostic overrides of the dispatch heuristics (0 = automatic).  Read ONCE from the environment when the context is
// created (IBS_FORCE_P, IBS_SCAN_CHAIN, IBS_CHAIN_W1, IBS_CHAIN_W2, IBS_GEO_LPP), changed afterwards only through
// ibs_set_option(): no getenv() on the call path, nothing process-global.
struct ibs_options : ibs::PlanOpts {     // (force_p, scan_chain, scan_resident, gcf_rows, gcf_direct, f32_lam, pack_mode, sturm_form: ibs_plan.hpp)
  int geo_lpp = 0;        // lanes per grid point of the geometry kernel: 1 | 2 | 4
  double sigma0 = std::numeric_limits<double>::quiet_NaN();   // not NaN: solves that return lam AND info flag lam_max >= sigma0 (informational status bit 4: utils.py:1597 would have taken the eigenpair nearest sigma0)
  int scan_trial_table = 1; // resident theta0 scan: 1 = the trial vector's start comes from the context's per-grid table, 0 = every wave computes it
  int reclose = 1;        // FP64 raw systems: 1 = a solve whose closing bracket fails its consistency checks is re-closed in division form, 2 = only marked, 0 = off
  int refine_tangent = -1; // refinement: alpha-tangent of a point staged in LDS (1) or read from global memory in the sums (0); -1 = by batch size
  double chain_w1 = 0.25, chain_w2 = 1.0;   // relative widths of the chain's warm starts
  long nearest_chunk_systems = 0;  // ibs_gamma_scan_nearest_f64: systems per chunk (rounded down to whole lines, at least one); 0 = by workspace budget
};

struct ibs_ctx {
  ibs_options opt, opt_created;
  int device = 0;
  hipStream_t stream = nullptr;
  // staging workspace for IBS_MEM_HOST calls (grown on demand, reused)
  void* ws = nullptr;
  size_t ws_bytes = 0;
  // page-locked mirror of the first hs_bytes of ws: small host-pointer calls pack their inputs / outputs into it and move
  // them with ONE copy each way (HostStage)
  void* hs = nullptr;
  size_t hs_bytes = 0;
  // workspace of the long-grid path (N > 2050: ibs_long.hip), grown on demand
  void* long_ws = nullptr;
  size_t long_ws_bytes = 0;
  // suspect list of the big-batch raw kernels (GcfArgs::fix_*): [count | system indices | polish values], grown on demand
  void* fix_buf = nullptr;
  long fix_cap = 0;
  ibs::Chip chip{256, 160 * 1024};   // CUs, LDS bytes a block may use
  ibs::Built built{};                // the forms of this build (ibs_create: the non-null entries of launch_table())
  // native RCCL communicator of this rank (ibs_comm_init), null = none
  void* comm = nullptr;
  int comm_rank = 0, comm_n = 1;
  // overlapped gathers (ibs_comm_allgather_start_f64): the communicator's own stream, "inputs written" marker of the
  // compute stream, one completion event per slot
  static constexpr int kCommSlots = 16;
  hipStream_t comm_stream = nullptr;
  hipEvent_t comm_ready = nullptr;
  hipEvent_t comm_done[kCommSlots] = {};
  bool comm_pending[kCommSlots] = {};
  // per-surface arrival counters of the fused scan + argmax kernel (zero between launches; the last arriver resets its
  // word).  One buffer PER STREAM the context has been used on: two plans of one context run under different streams may
  // have their fused kernels in flight at the same time, and shared counters would mix their arrivals.
  struct SurfCounters { hipStream_t stream; int* buf; int n; };
  std::vector<SurfCounters> surf_counters;
  // trial tables of the resident scan kernel (k_trial_table: the start of every lane's trial vector, a function of the grid length and
  // the rows per lane alone), built on first use and kept until ibs_destroy.  An entry belongs to the STREAM it was built on as well:
  // build and use are then ordered by the stream itself, with no synchronisation, whichever streams the context is moved between.
  // A full cache replaces the entry used longest ago, behind a device synchronisation (a launch on another stream may still read it)
  struct TrialTable { int N = 0, M = 0; hipStream_t stream = nullptr; double* buf = nullptr; unsigned long long used = 0; };
  static constexpr int kTrialTables = 16;
  TrialTable trial_tables[kTrialTables];
  unsigned long long trial_clock = 0;
  // ibs_refine_f64: per-round counts posted by the device (pinned host memory), statistics of the last call
  int* refine_hist = nullptr;
  int refine_hist_len = 0;
  long long refine_stats[4] = {0, 0, 0, 0};      // evaluations, forward sweeps, rounds, rounds enqueued
  bool refine_pending = false;                   // the last call's output kernel may still be running (device-pointer call)
  // the device-resident mode-row tables last checked by geo_rows_fit (pointers + counts) and the verdict: a few entries, oldest
  // replaced (a driver alternating between table sets does not pay the copy-back every call).  The key is addresses and sizes: a
  // caller that REUSES device memory for other rows must say so (option "forget_rows": ibs_amd does when it uploads a table set)
  struct RowsSeen { const void* r1 = nullptr; const void* r2 = nullptr; const void* xn = nullptr; const void* xnq = nullptr;
                    int n1 = 0, n2 = 0, mn = 0, mnq = 0; double d1 = 0, d2 = 0; int verdict = 0; };
  static constexpr int kRowsSeen = 4;
  RowsSeen rows_seen[kRowsSeen];
  int rows_seen_next = 0;
};

namespace {

// RCCL, bound at run time (the library carries no link-time dependency on it; in a PyTorch process the copy PyTorch has
// already loaded is used).  ncclUniqueId is a 128-byte struct passed BY VALUE to ncclCommInitRank.
struct nccl_id_t { char internal[128]; };
struct RcclApi {
  void* handle = nullptr;
  int (*GetUniqueId)(nccl_id_t*) = nullptr;
  int (*CommInitRank)(void**, int, nccl_id_t, int) = nullptr;
  int (*AllGather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
  int (*CommDestroy)(void*) = nullptr;
  const char* (*GetErrorString)(int) = nullptr;
};
RcclApi& rccl() { static RcclApi a; return a; }
constexpr int kNcclFloat64 = 8;          // ncclDataType_t (rccl.h)

// every entry point runs on the context's device and leaves the caller's current device as it found it
struct DeviceGuard {
  int prev = -1; hipError_t err = hipSuccess;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) err = hipSetDevice(dev); else prev = -1;     // (nothing to restore)
  }
  ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
  DeviceGuard(const DeviceGuard&) = delete;
  DeviceGuard& operator=(const DeviceGuard&) = delete;
};
#define ON_DEVICE(ctx_)                                                                                     \
  DeviceGuard dev_guard_((ctx_)->device);                                                                   \
  if (dev_guard_.err != hipSuccess) return fail(IBS_ERR_HIP, "hipSetDevice(%d) -> %s", (ctx_)->device, hipGetErrorString(dev_guard_.err))

using ibs::pad256; using ibs::Carve;      // (ibs_plan.hpp)

int ensure_long_ws(ibs_ctx* c, size_t bytes) {
  if (bytes <= c->long_ws_bytes) return 0;
  if (c->long_ws) { HIPCHK(hipStreamSynchronize(c->stream)); HIPCHK(hipFree(c->long_ws)); c->long_ws = nullptr; c->long_ws_bytes = 0; }
  HIPCHK(hipMalloc(&c->long_ws, bytes));
  c->long_ws_bytes = bytes;
  return 0;
}
// ctx->long_ws sized by the carve sequence that uses it (a function of a Carve&), then carved
template <typename F> int carve_long(ibs_ctx* c, F&& carve) {
  Carve sz{nullptr};
  carve(sz);
  if (int r = ensure_long_ws(c, sz.off)) return r;
  Carve cv{static_cast<char*>(c->long_ws)};
  carve(cv);
  return 0;
}
int ensure_fix(ibs_ctx* c, long n_sys) {
  if (n_sys <= c->fix_cap) return 0;
  if (c->fix_buf) { HIPCHK(hipStreamSynchronize(c->stream)); HIPCHK(hipFree(c->fix_buf)); c->fix_buf = nullptr; c->fix_cap = 0; }
  const long cap = n_sys < 4096 ? 4096 : n_sys;
  HIPCHK(hipMalloc(&c->fix_buf, 256 + (size_t)cap * 16));
  c->fix_cap = cap;
  return 0;
}
int long_waves(const ibs_ctx* c, long n_sys) { const long cap = 8L * c->chip.n_cu; return (int)(n_sys < cap ? n_sys : cap); }   // (ibs_long.hip: kLongChunk)
// the persistent grid of long_waves(n) with doubles_per_wave of ctx->long_ws each, entered into the launch arguments a of a
// one-wave-per-system kernel (a.work, a.work_doubles, a.n_waves: ibs_launch.hpp, persistent_grid)
template <class A> int with_wave_ws(ibs_ctx* c, A& a, long n, size_t doubles_per_wave) {
  const int nw = long_waves(c, n);
  if (int r = ensure_long_ws(c, (size_t)nw * doubles_per_wave * sizeof(double))) return r;
  a.work = static_cast<double*>(c->long_ws); a.work_doubles = c->long_ws_bytes / sizeof(double); a.n_waves = nw;
  return 0;
}

int ensure_ws(ibs_ctx* c, size_t bytes) {
  if (bytes <= c->ws_bytes) return 0;
  if (c->ws) { HIPCHK(hipStreamSynchronize(c->stream)); HIPCHK(hipFree(c->ws)); c->ws = nullptr; c->ws_bytes = 0; }
  HIPCHK(hipMalloc(&c->ws, bytes));
  c->ws_bytes = bytes;
  return 0;
}

// Small host-pointer calls (the drop-in gamma_ball_full: one system, ~70 KB in, ~16 KB out) spent most of their 0.17-0.22 ms
// in a dozen pageable hipMemcpyAsync of a few KB each (every one staged and waited for by the runtime).  HostStage mirrors the
// device workspace (ctx->ws) in page-locked host memory: up() copies a source into the mirror at its device offset, flush_in() moves the
// whole input span with ONE copy; down() records an output, flush_out() brings the output span back with ONE copy, waits for
// the stream and hands the pieces to the caller's buffers.  Calls whose spans exceed kMaxBytes take the direct copies.
struct HostStage {
  static constexpr size_t kMaxBytes = 4u << 20;
  ibs_ctx* c; bool on = false;
  size_t in_lo = ~size_t(0), in_hi = 0, out_lo = ~size_t(0), out_hi = 0;
  struct Piece { void* dst; size_t off, bytes; };
  std::vector<Piece> outs;
  bool in_flight = false;      // flush_in() ran and flush_out() has not: the pinned mirror / workspace are still being read by the stream
  // (an early error return between the two must not leave that copy running while the next call refills the mirror)
  ~HostStage() { if (in_flight) (void)hipStreamSynchronize(c->stream); }
  HostStage(const HostStage&) = delete;
  HostStage& operator=(const HostStage&) = delete;
  HostStage(ibs_ctx* c_, size_t need) : c(c_) {
    if (need > kMaxBytes) return;
    if (c->hs_bytes < need) {
      if (c->hs) { (void)hipStreamSynchronize(c->stream); (void)hipHostFree(c->hs); c->hs = nullptr; c->hs_bytes = 0; }
      const size_t want = need < (256u << 10) ? (256u << 10) : need;
      if (hipHostMalloc(&c->hs, want, hipHostMallocDefault) != hipSuccess) { c->hs = nullptr; (void)hipGetLastError(); return; }
      c->hs_bytes = want;
    }
    on = true;
  }
  size_t off_of(const void* dev) const { return (size_t)(static_cast<const char*>(dev) - static_cast<const char*>(c->ws)); }
  hipError_t up(const void* src, size_t bytes, void* dev) {
    if (!on) return hipMemcpyAsync(dev, src, bytes, hipMemcpyHostToDevice, c->stream);
    const size_t o = off_of(dev);
    std::memcpy(static_cast<char*>(c->hs) + o, src, bytes);
    if (o < in_lo) in_lo = o;
    if (o + bytes > in_hi) in_hi = o + bytes;
    return hipSuccess;
  }
  hipError_t flush_in() {
    if (!on || in_hi <= in_lo) return hipSuccess;
    in_flight = true;
    return hipMemcpyAsync(static_cast<char*>(c->ws) + in_lo, static_cast<char*>(c->hs) + in_lo, in_hi - in_lo, hipMemcpyHostToDevice, c->stream);
  }
  void down(void* dst, const void* dev, size_t bytes) {      // (only recorded: flush_out() moves it)
    const size_t o = off_of(dev);
    outs.push_back(Piece{dst, o, bytes});
    if (o < out_lo) out_lo = o;
    if (o + bytes > out_hi) out_hi = o + bytes;
  }
  // ends with the stream synchronised and every recorded output in the caller's memory
  hipError_t flush_out() {
    if (on && out_hi > out_lo) {
      hipError_t e = hipMemcpyAsync(static_cast<char*>(c->hs) + out_lo, static_cast<char*>(c->ws) + out_lo, out_hi - out_lo, hipMemcpyDeviceToHost, c->stream);
      if (e != hipSuccess) return e;
    }
    if (!on)
      for (const Piece& p : outs) {
        hipError_t e = hipMemcpyAsync(p.dst, static_cast<char*>(c->ws) + p.off, p.bytes, hipMemcpyDeviceToHost, c->stream);
        if (e != hipSuccess) return e;
      }
    hipError_t e = hipStreamSynchronize(c->stream);
    in_flight = false;
    if (e != hipSuccess) return e;
    if (on) for (const Piece& p : outs) std::memcpy(p.dst, static_cast<char*>(c->hs) + p.off, p.bytes);
    return hipSuccess;
  }
};

using ibs::is_long; using ibs::rows_per_lane;
// long_ok: the entry point has the generic long-grid path behind it (ibs_long.hip)
int check_grid(int32_t N, double h, bool long_ok = false) {
  const ibs::GridCheck g = ibs::check_grid_length(N, long_ok);
  if (g == ibs::GridCheck::Range) return fail(IBS_ERR_UNSUPPORTED, "N=%d outside [66, %d]", N, ibs::grid_n_max(long_ok));
  if (g == ibs::GridCheck::Even) return fail(IBS_ERR_UNSUPPORTED, "N=%d is even: the reference's Simpson rule is restated for odd N only", N);
  if (!(h > 0)) return fail(IBS_ERR_ARG, "h must be > 0");
  return 0;
}

__global__ void k_count_status(long n, const int* info, int* out) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  int bad = (i < n) && (((info[i] >> 16) & 3) != 0);      // (status bit 2 is informational: an FP32 result re-solved in FP64)
  unsigned long long m = __ballot(bad);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(out, __popcll(m));
}

// The host-pointer protocol of every entry point that takes `mem`.  The entry point declares its device buffers ONCE, in a function
// of a Stage& (in / out / scratch / status), and staged() runs that declaration twice: against no workspace to size ctx->ws, then
// against ctx->ws to carve it.  Host pointers: the inputs lie in one span of ctx->ws (moved up with one copy: HostStage), the outputs
// in the span behind it (moved back with one copy), scratch behind both.  Device pointers: in / out / status return the caller's
// pointers and only scratch is carved.
class Stage {
 public:
  const bool host;
  // input of n elements (a null source stays null)
  template <typename T> const T* in(const T* src, size_t n) {
    if (!host || !src) return src;
    T* d = in_.take<T>(n);
    if (hs_ && err_ == hipSuccess) err_ = hs_->up(src, n * sizeof(T), d);
    return d;
  }
  // output of n elements, copied back to dst; a null dst is carved too when `always` (the device code needs the buffer either way)
  template <typename T> T* out(T* dst, size_t n, bool always = false) {
    if (!host || !(dst || always)) return dst;
    T* d = out_.take<T>(n);
    if (hs_ && dst) hs_->down(dst, d, n * sizeof(T));
    return d;
  }
  // output of `rows` rows of n elements that lie ld >= n apart in dst.  Host pointers: the device buffer holds the rows packed (pitch
  // n: the launch must use rows_ld(n, ld)) and each comes back on its own, so the caller's entries n .. ld-1 of a row are never written
  template <typename T> T* out_rows(T* dst, size_t rows, size_t n, size_t ld) {
    if (!host || !dst || ld == n) return out(dst, rows * ld);
    T* d = out_.take<T>(rows * n);
    if (hs_) for (size_t r = 0; r < rows; ++r) hs_->down(dst + r * ld, d + r * n, n * sizeof(T));
    return d;
  }
  size_t rows_ld(size_t n, size_t ld) const { return host ? n : ld; }
  // workspace of the device code alone, in either mode
  template <typename T> T* scratch(size_t n, bool when = true) { return when ? scr_.take<T>(n) : nullptr; }
  // status words: host pointers always get a device buffer, whose count of bad words is what staged() returns
  int* status(int32_t* info, size_t n) {
    if (!host) return info;
    status_ = out(info, n, true);
    nbad_ = out_.take<int>(1);
    n_status_ = n;
    return status_;
  }

 private:
  template <typename D, typename L> friend int staged(ibs_ctx*, int32_t, D&&, L&&);
  Stage(bool host_, char* ws, size_t in_bytes, size_t io_bytes, HostStage* hs)
      : host(host_), in_{ws}, out_{ws ? ws + in_bytes : nullptr}, scr_{ws ? ws + io_bytes : nullptr}, hs_(hs) {}
  Carve in_, out_, scr_;
  HostStage* hs_;
  hipError_t err_ = hipSuccess;
  int *status_ = nullptr, *nbad_ = nullptr;
  size_t n_status_ = 0;
};

// decl(Stage&) declares the buffers and fills the launch arguments, launch() launches (IBS error code or 0), in either mode.
// Returns: host pointers, the count of status words with bit 0 or 1 set (0 without status()); device pointers, 0.
template <typename Decl, typename Launch>
int staged(ibs_ctx* ctx, int32_t mem, Decl&& decl, Launch&& launch) {
  const bool host = mem == IBS_MEM_HOST;
  Stage sz(host, nullptr, 0, 0, nullptr);
  decl(sz);
  const size_t in_bytes = pad256(sz.in_.off), io_bytes = in_bytes + pad256(sz.out_.off), bytes = io_bytes + sz.scr_.off;
  if (bytes) if (int r = ensure_ws(ctx, bytes)) return r;
  char* ws = static_cast<char*>(ctx->ws);
  if (!host) {
    Stage s(false, ws, 0, 0, nullptr);
    decl(s);
    return launch();
  }
  HostStage hs(ctx, io_bytes);
  Stage s(true, ws, in_bytes, io_bytes, &hs);
  decl(s);
  if (s.err_ != hipSuccess) return fail(IBS_ERR_HIP, "host -> device copy -> %s", hipGetErrorString(s.err_));
  HIPCHK(hs.flush_in());
  if (int r = launch()) return r;
  int nbad = 0;
  if (s.nbad_) {
    HIPCHK(hipMemsetAsync(s.nbad_, 0, sizeof(int), ctx->stream));
    hipLaunchKernelGGL(k_count_status, dim3((unsigned)((s.n_status_ + 255) / 256)), dim3(256), 0, ctx->stream, (long)s.n_status_, s.status_, s.nbad_);
    hs.down(&nbad, s.nbad_, sizeof(int));
  }
  HIPCHK(hs.flush_out());
  return nbad;
}

// What the geometry-fed entry points take for a batch of lines: the seven arrays [n_lines][ld], dPdrho [n_lines] and theta0 [n_theta0]
// shared by all lines -- or, per_line, n_theta0 = 1 and theta0 [n_lines] (the points forms).  Built once from the extern "C" argument
// list; the entry point checks it, declares it to its Stage and takes the views of its chunks from the staged copy.
struct GeoLines {
  const double* a[7] = {};         // bmag gradpar cvdrift cvdrift0 gds2 gds21 gds22
  int64_t ld = 0;
  const double *dPdrho = nullptr, *theta0 = nullptr;
  bool per_line = false;
  bool present() const { for (const double* p : a) if (!p) return false; return true; }
  GeoLines declare(Stage& s, size_t n_lines, size_t n_theta0) const {
    GeoLines d = *this;
    for (int k = 0; k < 7; ++k) d.a[k] = s.in(a[k], n_lines * (size_t)ld);
    d.dPdrho = s.in(dPdrho, n_lines); d.theta0 = s.in(theta0, per_line ? n_lines : n_theta0);
    return d;
  }
  GeoLines at(long l0) const {     // the lines from l0 on
    GeoLines v = *this;
    for (int k = 0; k < 7; ++k) v.a[k] = a[k] + l0 * ld;
    v.dPdrho = dPdrho + l0; v.theta0 = theta0 + (per_line ? l0 : 0);
    return v;
  }
  // into launch arguments (ibs_launch.hpp): the geo7[7] form, and the named members of ScanArgs / Theta0PolishArgs
  template <class A> void into(A& x) const { for (int k = 0; k < 7; ++k) x.geo7[k] = a[k]; x.dPdrho = dPdrho; x.theta0 = theta0; }
  template <class A> void into_named(A& x) const {
    x.bmag = a[0]; x.gradpar = a[1]; x.cvdrift = a[2]; x.cvdrift0 = a[3]; x.gds2 = a[4]; x.gds21 = a[5]; x.gds22 = a[6];
    x.dPdrho = dPdrho; x.theta0 = theta0;
  }
};

// The lines of a geometry-fed scan, chunk after chunk of whole lines (ibs::plan_line_chunks under kLineChunkBudget and option
// "nearest_chunk_systems").  carve(Carve&, L) declares ctx->long_ws of a chunk of L lines -- it runs against no buffer to size the
// chunk and LAST against ctx->long_ws, so what it sets by side effect is then real --, body(l0, Lc) launches the Lc lines from l0 on and
// returns an IBS code; the first that is not 0 ends the loop.
template <class CarveFn, class Body>
int for_line_chunks(ibs_ctx* ctx, const char* what, long n_lines, int n_theta0, int N, CarveFn&& carve, Body&& body) {
  auto bytes_of = [&](long L) { Carve sz{nullptr}; carve(sz, L); return sz.off; };
  const ibs::LineChunks ch = ibs::plan_line_chunks(n_lines, n_theta0, ctx->opt.nearest_chunk_systems, ibs::kLineChunkBudget, bytes_of);
  if (ensure_long_ws(ctx, ch.bytes) != 0) {
    (void)hipGetLastError();
    return fail(IBS_ERR_HIP, "%s: a chunk of %ld line(s) x %d theta0 at N=%d needs %zu bytes of device workspace, "
                "which could not be allocated", what, ch.lines, n_theta0, N, ch.bytes);
  }
  Carve cv{static_cast<char*>(ctx->long_ws)};
  carve(cv, ch.lines);
  for (long l0 = 0; l0 < n_lines; l0 += ch.lines)
    if (int r = body(l0, n_lines - l0 < ch.lines ? n_lines - l0 : ch.lines)) return r;
  return 0;
}

// Nearest-sigma report (option "sigma0"): the reference takes the eigenpair NEAREST sigma0 (eigs(..., sigma=sigma0), utils.py:1597;
// sigma0 = 1.0 in the coarse scan, 1.3 |gam| + 0.05 in the refinement, 0.42 in the final solve: ball_scan.py:230, 289, 337); this
// library always returns lam_max.  The two are the same eigenpair whenever lam_max < sigma0 -- true of every equilibrium seen so
// far -- and only then.  A solve with lam_max >= sigma0 carries the informational status bit 4.
template <typename T>
__global__ void k_flag_sigma(long n, const T* lam, int* info, double sigma0) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && (double)lam[i] >= sigma0) info[i] |= 16 << 16;
}
template <typename T>
static void flag_sigma(const ibs_ctx* ctx, long n, const T* lam, int* info) {
  if (!(ctx->opt.sigma0 == ctx->opt.sigma0) || !lam || !info || n <= 0) return;
  hipLaunchKernelGGL(k_flag_sigma<T>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, n, lam, info, ctx->opt.sigma0);
}

static inline int argmax_threads(int n_per) { const int t = ((n_per + 63) / 64) * 64; return t > 256 ? 256 : t; }

// first-argmax per surface (ball_scan.py:283-295 tie rule: lowest row-major index wins)
__global__ void __launch_bounds__(256) k_surface_argmax(int n_per, const double* gam, int* idx, double* val, double* pack) {
  __shared__ double sv[4];
  __shared__ int si[4];
  const double* g = gam + (size_t)blockIdx.x * n_per;
  double best = -1.7976931348623157e308;
  int bi = 0x7fffffff;
  for (int i = threadIdx.x; i < n_per; i += blockDim.x) {
    const double v = g[i];
    if (v > best || (v == best && i < bi)) { best = v; bi = i; }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const double v2 = __shfl_xor(best, d);
    const int i2 = __shfl_xor(bi, d);
    if (v2 > best || (v2 == best && i2 < bi)) { best = v2; bi = i2; }
  }
  const int w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  if (nw > 1) {                      // (one wave per surface when n_per <= 64: no LDS round trip, no barrier)
    if ((threadIdx.x & 63) == 0) { sv[w] = best; si[w] = bi; }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    for (int k = 1; k < nw; ++k)
      if (sv[k] > best || (sv[k] == best && si[k] < bi)) { best = sv[k]; bi = si[k]; }
    if (idx) idx[blockIdx.x] = bi;
    if (val) val[blockIdx.x] = best;
    if (pack) { pack[2 * blockIdx.x] = best; pack[2 * blockIdx.x + 1] = (double)bi; }   // one buffer for the all-gather
  }
}

// Hellmann-Feynman derivative of the growth rate for given tangent coefficient arrays (utils.py:1676-1680 /
// 1721-1725): one wave per system, Simpson sums with unit spacing.
__global__ void __launch_bounds__(256) k_hf_grad(long n_sys, int N, long ld, const double* __restrict__ X,
                                                 const double* __restrict__ dX, const double* __restrict__ f,
                                                 const double* __restrict__ g_p, const double* __restrict__ c_p,
                                                 const double* __restrict__ f_p, const double* __restrict__ gam,
                                                 double* __restrict__ jac) {
  const int lane = threadIdx.x & 63;
  const long sys = (long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (sys >= n_sys) return;
  const long o = sys * ld;
  double y1 = 0.0, sc = 0.0, sg = 0.0, sf = 0.0;
  for (int j = lane; j < N; j += 64) {
    const double w = (j == 0 || j == N - 1) ? 1.0 : ((j & 1) ? 4.0 : 2.0);
    const double x2 = w * X[o + j] * X[o + j], d2 = w * dX[o + j] * dX[o + j];
    y1 += f[o + j] * x2; sc += c_p[o + j] * x2; sg += g_p[o + j] * d2; sf += f_p[o + j] * x2;
  }
  y1 = ibs::wave_sum(y1); sc = ibs::wave_sum(sc); sg = ibs::wave_sum(sg); sf = ibs::wave_sum(sf);
  if (lane == 0) jac[sys] = sc / y1 - sg / y1 - gam[sys] * sf / y1;
}

// start points of the refinement from the per-surface maxima of the coarse scan (ball_scan.py:279-295)
__global__ void k_scan_starts(int n_surf, int n_alpha, int n_theta0, const double* alpha, const double* theta0,
                              const double* pack, double* start, double* sigma0, int* n_bad) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n_surf) return;
  const double m = pack[2 * s], fi = pack[2 * s + 1];
  double a = 0.0, t = 0.0, sg = 0.05;                                      // ball_scan.py:279-282: an all-zero table
  const bool ok = (m == m) && fabs(m) <= 1.7976931348623157e308 && fi >= 0.0 && fi < (double)n_alpha * n_theta0;
  if (!ok) atomicAdd(n_bad, 1);                                           // a NaN / flagged table: reported, start (0, 0)
  else if (m != 0.0) {
    const int idx = (int)fi, i = idx / n_theta0, j = idx - i * n_theta0;   // first maximum, row-major (ball_scan.py:283-288)
    // ball_scan.py:289, 295, rounded as Python rounds it (the product, then the sum: pick_start's bits, not a fused multiply-add's)
    a = alpha[i]; t = theta0[j]; sg = ibs::peaks_sigma0(m);
  }
  start[2 * s] = a; start[2 * s + 1] = t;
  if (sigma0) sigma0[s] = sg;
}

// the launcher of a planned raw solve (Long: none, launch_gcf_long) and of the second launch of the forms that list their suspects
// (k_fix_gcf, by the rows per lane of one wave per system)
template <typename T> using GcfLauncher = hipError_t (*)(const ibs::GcfArgs<T>&, hipStream_t);
template <typename T>
GcfLauncher<T> gcf_launcher(const ibs::GcfPlan& p) {
  using F = ibs::GcfForm;
  const ibs::LaunchTable& t = ibs::launch_table();
  const int M = p.M, pi = p.P == 32 ? 0 : 1;
  if constexpr (sizeof(T) == 8) {
    switch (p.form) {
      case F::Staged: return t.gcf_f64[M];      case F::Rows: return t.gcf_rows_f64[M];
      case F::Direct: return t.gcf_direct_f64[M]; case F::Group: return t.gcf_f64_g[pi][M];
      default: return nullptr;
    }
  } else {
    switch (p.form) {
      case F::F32: return t.gcf_f32[M];                     case F::F32Wide: return t.gcf_f32_wide[M];
      case F::F32WideRows: return t.gcf_f32w_rows[M];       case F::F32WideDirect: return t.gcf_direct_f32w[M];
      case F::F32LamDirect: return t.gcf_direct_f32lam[M];  case F::GroupWide: return t.gcf_f32w_g[pi][M];
      default: return nullptr;
    }
  }
}
template <typename T>
GcfLauncher<T> gcf_fix_launcher(int N) {
  if constexpr (sizeof(T) == 8) return ibs::launch_table().gcf_fix_f64[rows_per_lane(N)];
  else return ibs::launch_table().gcf_fix_f32w[rows_per_lane(N)];
}

// a planned raw solve on device rows: the solver kernel of the plan, the fix-up launch of the forms that list their suspects, or the
// long-grid kernel.  long_work: the long-grid kernel's workspace (long_waves(n_sys) * 3 N doubles) where the caller has carved it
// out of ctx->long_ws together with the rows (the geometry-fed theta scans); null = ctx->long_ws is sized here and used whole
template <typename T>
int launch_planned_gcf(ibs_ctx* ctx, const ibs::GcfPlan& plan, ibs::GcfArgs<T>& a, double* long_work = nullptr) {
  const int N = a.N;
  if (plan.form != ibs::GcfForm::Long) {
    if (plan.lists_suspects && (a.flags & 1)) {
      if (int r = ensure_fix(ctx, (long)a.n_sys)) return r;
      char* fb = static_cast<char*>(ctx->fix_buf);
      a.fix_count = reinterpret_cast<int*>(fb);
      a.fix_sys = reinterpret_cast<long*>(fb + 256);
      a.fix_center = reinterpret_cast<double*>(fb + 256 + (size_t)ctx->fix_cap * 8);
      HIPCHK(hipMemsetAsync(a.fix_count, 0, sizeof(int), ctx->stream));
    }
    HIPCHK(gcf_launcher<T>(plan)(a, ctx->stream));
    if (a.fix_count) {
      ibs::LaunchNote keep = ibs::last_launch();         // (ibs_last_launch names the solver kernel, not its fix-up pass)
      const auto fix = gcf_fix_launcher<T>(N);
      if (!fix) return fail(IBS_ERR_UNSUPPORTED, "no fix-up kernel built for N=%d", N);
      HIPCHK(fix(a, ctx->stream));
      ibs::last_launch() = keep;
    }
    return 0;
  }
  const int nw = long_waves(ctx, (long)a.n_sys);
  if (!long_work) {
    if (int r = ensure_long_ws(ctx, (size_t)nw * 3 * (size_t)N * sizeof(double))) return r;
    long_work = static_cast<double*>(ctx->long_ws);
  }
  ibs::LongGcfArgs la{};
  la.n_sys = a.n_sys; la.N = N; la.h = (double)a.h; la.g = a.g; la.c = a.c; la.f = a.f; la.gh = a.gh; la.f32 = sizeof(T) == 4;
  la.ld = a.ld; la.lam = a.lam; la.gam = a.gam; la.X = a.X; la.dX = a.dX; la.info = a.info;
  la.work = long_work; la.n_waves = nw;
  HIPCHK(ibs::launch_gcf_long(la, ctx->stream));
  return 0;
}

template <typename T>
int solve_gcf_impl(ibs_ctx* ctx, int64_t n_sys, int32_t N, T h, const T* g, const T* c, const T* f, int64_t ld,
                   T* lam, T* gam, T* X, T* dX, int32_t* info, int32_t mem, const T* gh = nullptr) {
  if (!ctx) return fail(IBS_ERR_ARG, "null context");
  if (n_sys < 0 || !g || !c || !f || ld < N) return fail(IBS_ERR_ARG, "bad arguments (n_sys=%lld ld=%lld N=%d)", (long long)n_sys, (long long)ld, N);
  if (int r = check_grid(N, (double)h, true)) return r;
  if (n_sys == 0) return 0;
  const ibs::GcfPlan plan = ibs::plan_gcf(ctx->chip, ctx->opt, ctx->built, (int)sizeof(T), (long)n_sys, N, gh != nullptr, gam != nullptr, X || dX);
  if (plan.err == ibs::PlanError::NotBuilt) return fail(IBS_ERR_UNSUPPORTED, "no kernel built for rows-per-lane M=%d (N=%d)", plan.M, N);
  ON_DEVICE(ctx);
  if (plan.err == ibs::PlanError::NoLds) return fail(IBS_ERR_UNSUPPORTED, "N=%d needs %zu B of LDS per wave", N, plan.per_wave);
  auto launch_it = [&](ibs::GcfArgs<T>& a) -> int { return launch_planned_gcf<T>(ctx, plan, a); };
  ibs::GcfArgs<T> a{};
  a.n_sys = n_sys; a.N = N; a.h = h; a.ld = ld; a.wpb = plan.wpb;
  a.flags = ctx->opt.reclose == 1 ? 1 : (ctx->opt.reclose == 2 ? 2 : 0);
  const size_t in_elems = (size_t)n_sys * ld, out_elems = (size_t)n_sys * N;
  // (host pointers: lam and info are always carved; gam not asked for stays null -- the kernels then take their eigenvalue-only
  //  exits, as they do for device-pointer calls)
  auto decl = [&](Stage& s) {
    a.g = s.in(g, in_elems); a.c = s.in(c, in_elems); a.f = s.in(f, in_elems); a.gh = s.in(gh, in_elems);
    a.lam = s.out(lam, n_sys, true); a.gam = s.out(gam, n_sys); a.X = s.out(X, out_elems); a.dX = s.out(dX, out_elems);
    a.info = s.status(info, n_sys);
  };
  return staged(ctx, mem, decl, [&]() -> int {
    if (int r = launch_it(a)) return r;
    flag_sigma<T>(ctx, (long)n_sys, a.lam, a.info);
    return 0;
  });
}


// ---------------------------------------------------------------- (alpha, theta0) maximiser (row F2): see ibs_refine.hpp
using ibs::RefineState; using ibs::RefineParams; using ibs::RefineCtrl;

__global__ void k_refine_init(int n, const int* pt_surf, const double* start, RefineState* st, RefineParams p,
                              int* idx, int* line_surf, double* line_alpha, double* th0, RefineCtrl* ctrl,
                              int N, const double* theta, int* status) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  // the theta grid must be uniform (the batched kernels take h): checked here, on the device copy; the host sees *status
  const double h = (theta[N - 1] - theta[0]) / (N - 1);
  if (k == 0) {
    ctrl->n_c = n; ctrl->n_lines = 3 * n; ctrl->done = 0; ctrl->round = 0; ctrl->h = h;
    if (!(h > 0)) *status = 2;
  }
  for (int j = 1 + k; j < N; j += gridDim.x * blockDim.x)
    if (fabs((theta[j] - theta[j - 1]) - h) > 1e-9 * fabs(h)) *status = 1;
  if (k >= n) return;
  RefineState& s = st[k];                     // (the state lives in global memory; nothing of it is kept in registers)
  const double x0[2] = {start[2 * k], start[2 * k + 1]};
  ibs::lbfgsb2::init(s.q, x0, p.lo, p.hi, p.ftol, p.gtol, p.maxiter, 20);
  s.active = 1; s.nev = 0; s.have = 0; s.sweeps = 0;
  s.lam_prev = 0.0; s.x_prev[0] = s.x_prev[1] = 0.0; s.g_prev[0] = s.g_prev[1] = 0.0; s.err_prev = 0.0;
  idx[k] = k;
  ibs::refine_emit(s.q.x, p.del_alpha, k, min(max(pt_surf[k], 0), p.n_surf - 1), line_surf, line_alpha, th0);
}

__global__ void k_refine_out(int n, const RefineState* st, double* x_opt, double* f_opt, int* n_evals, long long* stats) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  x_opt[2 * k] = st[k].q.x[0]; x_opt[2 * k + 1] = st[k].q.x[1]; f_opt[k] = st[k].q.f;
  if (n_evals) n_evals[k] = st[k].nev;
  atomicAdd_system(reinterpret_cast<unsigned long long*>(stats), (unsigned long long)st[k].nev);         // (pinned host memory)
  atomicAdd_system(reinterpret_cast<unsigned long long*>(stats + 1), (unsigned long long)st[k].sweeps);
}
}  // namespace

extern "C" {

int ibs_version(void) { return 100; }
const char* ibs_last_error(void) { return g_err.c_str(); }

int ibs_last_launch(char* name, int32_t len, int64_t* blocks, int32_t* threads) {
  const ibs::LaunchNote& n = ibs::last_launch();
  if (name && len > 0) { strncpy(name, n.name, (size_t)len - 1); name[len - 1] = 0; }
  if (blocks) *blocks = n.blocks;
  if (threads) *threads = n.threads;
  return 0;
}

int ibs_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int ibs_create(ibs_ctx** out, int device_id) {
  if (!out) return fail(IBS_ERR_ARG, "null output pointer");
  *out = nullptr;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n == 0) return fail(IBS_ERR_HIP, "no HIP device available (%s)", hipGetErrorString(e));
  if (device_id < 0 || device_id >= n) return fail(IBS_ERR_ARG, "device %d out of range (0..%d)", device_id, n - 1);
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, device_id));
  ibs_ctx* c = new ibs_ctx();
  c->device = device_id;
  c->chip.lds_per_block = (int)prop.sharedMemPerBlock > 64 * 1024 ? (int)prop.sharedMemPerBlock : 64 * 1024;
  if (prop.maxSharedMemoryPerMultiProcessor > (size_t)c->chip.lds_per_block) c->chip.lds_per_block = (int)prop.maxSharedMemoryPerMultiProcessor;
  if (c->chip.lds_per_block > 160 * 1024) c->chip.lds_per_block = 160 * 1024;
  c->chip.n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  if (const char* e = getenv("IBS_FORCE_P")) c->opt.force_p = atoi(e);
  if (const char* e = getenv("IBS_SCAN_CHAIN")) c->opt.scan_chain = atoi(e);
  if (const char* e = getenv("IBS_GEO_LPP")) c->opt.geo_lpp = atoi(e);
  if (const char* e = getenv("IBS_CHAIN_W1")) c->opt.chain_w1 = atof(e);
  if (const char* e = getenv("IBS_CHAIN_W2")) c->opt.chain_w2 = atof(e);
  c->opt_created = c->opt;
  // the forms of this build, for the planner: once per context (the registrars have run before main)
  const ibs::LaunchTable& t = ibs::launch_table();
  ibs::Built& b = c->built;
  for (int M = 0; M <= ibs::kMaxM; ++M) {
    auto mark = [M](uint64_t& mask, auto* entry) { if (entry) mask |= uint64_t(1) << M; };
    mark(b.gcf_f64, t.gcf_f64[M]); mark(b.gcf_f32, t.gcf_f32[M]); mark(b.gcf_f32_wide, t.gcf_f32_wide[M]);
    mark(b.scan, t.scan_f64[M]); mark(b.scan_chain, t.scan_chain_f64[M]);
    mark(b.gcf_rows, t.gcf_rows_f64[M]); mark(b.gcf_f32w_rows, t.gcf_f32w_rows[M]);
    mark(b.gcf_direct, t.gcf_direct_f64[M]); mark(b.gcf_f32w_direct, t.gcf_direct_f32w[M]); mark(b.gcf_f32lam_direct, t.gcf_direct_f32lam[M]);
    for (int pi = 0; pi < 2; ++pi) {
      mark(b.gcf_g[pi], t.gcf_f64_g[pi][M]); mark(b.gcf_f32w_g[pi], t.gcf_f32w_g[pi][M]);
      mark(b.scan_g[pi], t.scan_f64_g[pi][M]); mark(b.scan_chain_g[pi], t.scan_chain_f64_g[pi][M]);
    }
  }
  *out = c;
  return 0;
}

int ibs_destroy(ibs_ctx* c) {
  if (!c) return 0;
  (void)ibs_comm_destroy(c);
  DeviceGuard g(c->device);
  if (c->ws) hipFree(c->ws);
  if (c->long_ws) hipFree(c->long_ws);
  if (c->fix_buf) hipFree(c->fix_buf);
  for (auto& sc : c->surf_counters) if (sc.buf) hipFree(sc.buf);
  for (auto& tt : c->trial_tables) if (tt.buf) hipFree(tt.buf);
  if (c->refine_hist) hipHostFree(c->refine_hist);
  if (c->hs) hipHostFree(c->hs);
  delete c;
  return 0;
}

int ibs_set_stream(ibs_ctx* c, void* s) {
  if (!c) return fail(IBS_ERR_ARG, "null context");
  c->stream = reinterpret_cast<hipStream_t>(s);
  return 0;
}

int ibs_set_option(ibs_ctx* c, const char* name, double value) {
  if (!c || !name) return fail(IBS_ERR_ARG, "null context / name");
  const bool reset = !(value == value);          // NaN: back to what ibs_create() read from the environment
  const std::string n(name);
  if (n == "force_p") c->opt.force_p = reset ? c->opt_created.force_p : (int)value;
  else if (n == "scan_chain") c->opt.scan_chain = reset ? c->opt_created.scan_chain : (int)value;
  else if (n == "geo_lpp") c->opt.geo_lpp = reset ? c->opt_created.geo_lpp : (int)value;
  else if (n == "gcf_rows") c->opt.gcf_rows = reset ? c->opt_created.gcf_rows : (int)value;
  else if (n == "gcf_direct") c->opt.gcf_direct = reset ? c->opt_created.gcf_direct : (int)value;
  else if (n == "scan_resident") c->opt.scan_resident = reset ? c->opt_created.scan_resident : (int)value;
  else if (n == "scan_trial_table") c->opt.scan_trial_table = reset ? c->opt_created.scan_trial_table : (int)value;
  else if (n == "pack_mode") c->opt.pack_mode = reset ? c->opt_created.pack_mode : (int)value;
  else if (n == "f32_lam") c->opt.f32_lam = reset ? c->opt_created.f32_lam : (int)value;
  else if (n == "reclose") c->opt.reclose = reset ? c->opt_created.reclose : (int)value;
  else if (n == "sturm_form") c->opt.sturm_form = reset ? c->opt_created.sturm_form : (int)value;
  else if (n == "sigma0") c->opt.sigma0 = reset ? c->opt_created.sigma0 : value;
  else if (n == "forget_rows") { for (auto& e : c->rows_seen) e = ibs_ctx::RowsSeen{}; }      // (an action, not a setting)
  else if (n == "refine_tangent") c->opt.refine_tangent = reset ? c->opt_created.refine_tangent : (int)value;
  else if (n == "chain_w1") c->opt.chain_w1 = reset ? c->opt_created.chain_w1 : value;
  else if (n == "chain_w2") c->opt.chain_w2 = reset ? c->opt_created.chain_w2 : value;
  else if (n == "nearest_chunk_systems") c->opt.nearest_chunk_systems = reset ? c->opt_created.nearest_chunk_systems : (long)value;
  else if (n == "all" && reset) c->opt = c->opt_created;
  else return fail(IBS_ERR_ARG, "unknown option '%s'", name);
  return 0;
}

// ---- host side of the bounded quasi-Newton state machine (ibs_lbfgsb2.hpp): no GPU involved
int ibs_lbfgsb2_state_bytes(void) { return (int)sizeof(ibs::lbfgsb2::State); }

int ibs_lbfgsb2_init(void* state, const double* x0, const double* lo, const double* hi, double ftol, double gtol,
                     int32_t maxiter, int32_t maxls) {
  if (!state || !x0 || !lo || !hi) return fail(IBS_ERR_ARG, "null pointer");
  if (!(lo[0] <= hi[0]) || !(lo[1] <= hi[1]) || maxiter < 0 || maxls < 1) return fail(IBS_ERR_ARG, "bad bounds / limits");
  ibs::lbfgsb2::init(*static_cast<ibs::lbfgsb2::State*>(state), x0, lo, hi, ftol, gtol, maxiter, maxls);
  return 0;
}

int ibs_lbfgsb2_step(void* state, double f, const double* g, double* x_next) {
  if (!state || !g || !x_next) return fail(IBS_ERR_ARG, "null pointer");
  auto& s = *static_cast<ibs::lbfgsb2::State*>(state);
  const bool more = ibs::lbfgsb2::step(s, f, g);
  x_next[0] = s.x[0]; x_next[1] = s.x[1];
  return more ? 1 : 0;
}

int ibs_lbfgsb2_result(const void* state, double* x, double* f, int32_t* counters) {
  if (!state) return fail(IBS_ERR_ARG, "null pointer");
  const auto& s = *static_cast<const ibs::lbfgsb2::State*>(state);
  if (x) { x[0] = s.x[0]; x[1] = s.x[1]; }
  if (f) *f = s.f;
  if (counters) { counters[0] = s.n_iterations; counters[1] = s.nfgv; counters[2] = s.task; counters[3] = s.n_restarts; counters[4] = s.nskip; }
  return 0;
}

// ---- host side of the theta0 search and the row peaks (ibs_theta0_polish.hpp): no GPU involved
int ibs_theta0_polish_state_bytes(void) { return (int)sizeof(ibs::t0p::State); }

int ibs_theta0_polish_init(void* state, int32_t n_theta0, const double* theta0, const double* row, int32_t node, double xtol,
                           int32_t max_eval, double* x_next) {
  if (!state || !theta0 || !row || !x_next) return fail(IBS_ERR_ARG, "null pointer");
  if (n_theta0 < 1 || node < 0 || node >= n_theta0 || !(xtol > 0) || !std::isfinite(xtol) || max_eval < 1 || max_eval > ibs::t0p::kMaxEval)
    return fail(IBS_ERR_ARG, "node in [0, n_theta0), xtol > 0 and finite, max_eval in [1, %d] required", ibs::t0p::kMaxEval);
  if (!ibs::t0p::grid_ok(theta0, n_theta0)) return fail(IBS_ERR_ARG, "theta0 must be finite and strictly increasing");
  if (!(row[node] == row[node])) return fail(IBS_ERR_ARG, "the node's gam is NaN");
  auto& s = *static_cast<ibs::t0p::State*>(state);
  const bool more = ibs::t0p::init_row(s, theta0, row, n_theta0, node, 0.0, xtol, max_eval);
  *x_next = s.u;
  return more ? 1 : 0;
}

int ibs_theta0_polish_step(void* state, double gam, int32_t eval_status, double* x_next) {
  if (!state || !x_next) return fail(IBS_ERR_ARG, "null pointer");
  auto& s = *static_cast<ibs::t0p::State*>(state);
  const bool more = ibs::t0p::step(s, gam, 0.0, eval_status);
  *x_next = s.u;
  return more ? 1 : 0;
}

int ibs_theta0_polish_result(const void* state, double* theta0_star, double* gam_star, int32_t* n_eval, int32_t* status) {
  if (!state) return fail(IBS_ERR_ARG, "null pointer");
  const auto& s = *static_cast<const ibs::t0p::State*>(state);
  double x, f, tag;
  int st;
  ibs::t0p::result(s, x, f, tag, st);
  if (theta0_star) *theta0_star = x;
  if (gam_star) *gam_star = f;
  if (n_eval) *n_eval = s.n_eval;
  if (status) *status = st;
  return 0;
}

int ibs_row_peaks_f64(int32_t n_rows, int32_t n_theta0, int32_t K, const double* gam, int32_t* node, int32_t* n_found) {
  if (n_rows < 0 || n_theta0 < 1 || K < 1 || K > ibs::t0p::kMaxSlots || !gam || !node)
    return fail(IBS_ERR_ARG, "K in [1, %d], n_theta0 >= 1, gam and node required", ibs::t0p::kMaxSlots);
  for (int32_t r = 0; r < n_rows; ++r) {
    const int nf = ibs::t0p::row_peaks(gam + (size_t)r * n_theta0, n_theta0, K, node + (size_t)r * K);
    if (n_found) n_found[r] = nf;
  }
  return 0;
}

// ---- native collective: ONE ncclAllGather of the per-surface rows on the context's stream
int ibs_comm_load(const char* librccl_path) {
  RcclApi& a = rccl();
  if (a.handle) return 0;
  const char* cands[3] = {librccl_path, "librccl.so.1", "librccl.so"};
  void* h = nullptr;
  for (const char* c : cands) {
    if (!c) continue;
    h = dlopen(c, RTLD_NOW | RTLD_GLOBAL | RTLD_NOLOAD);          // the copy this process already holds, if any
    if (!h) h = dlopen(c, RTLD_NOW | RTLD_GLOBAL);
    if (h) break;
  }
  if (!h) return fail(IBS_ERR_UNSUPPORTED, "librccl not found (%s)", dlerror());
  a.GetUniqueId = reinterpret_cast<decltype(a.GetUniqueId)>(dlsym(h, "ncclGetUniqueId"));
  a.CommInitRank = reinterpret_cast<decltype(a.CommInitRank)>(dlsym(h, "ncclCommInitRank"));
  a.AllGather = reinterpret_cast<decltype(a.AllGather)>(dlsym(h, "ncclAllGather"));
  a.CommDestroy = reinterpret_cast<decltype(a.CommDestroy)>(dlsym(h, "ncclCommDestroy"));
  a.GetErrorString = reinterpret_cast<decltype(a.GetErrorString)>(dlsym(h, "ncclGetErrorString"));
  if (!a.GetUniqueId || !a.CommInitRank || !a.AllGather || !a.CommDestroy)
    return fail(IBS_ERR_UNSUPPORTED, "librccl lacks ncclGetUniqueId / ncclCommInitRank / ncclAllGather / ncclCommDestroy");
  a.handle = h;
  return 0;
}

static int nccl_fail(const char* what, int rc) {
  RcclApi& a = rccl();
  return fail(IBS_ERR_HIP, "%s -> %s", what, a.GetErrorString ? a.GetErrorString(rc) : "rccl error");
}

int ibs_comm_unique_id(void* id128) {
  if (!id128) return fail(IBS_ERR_ARG, "null pointer");
  if (!rccl().handle) { if (int r = ibs_comm_load(nullptr)) return r; }
  const int rc = rccl().GetUniqueId(static_cast<nccl_id_t*>(id128));
  return rc ? nccl_fail("ncclGetUniqueId", rc) : 0;
}

int ibs_comm_init(ibs_ctx* c, const void* id128, int32_t rank, int32_t nranks) {
  if (!c || !id128 || nranks < 1 || rank < 0 || rank >= nranks) return fail(IBS_ERR_ARG, "bad arguments");
  if (!rccl().handle) { if (int r = ibs_comm_load(nullptr)) return r; }
  if (c->comm) return fail(IBS_ERR_ARG, "the context already holds a communicator");
  ON_DEVICE(c);
  nccl_id_t id;
  memcpy(&id, id128, sizeof(id));
  void* comm = nullptr;
  const int rc = rccl().CommInitRank(&comm, nranks, id, rank);
  if (rc) return nccl_fail("ncclCommInitRank", rc);
  c->comm = comm; c->comm_rank = rank; c->comm_n = nranks;
  return 0;
}

int ibs_comm_allgather_f64(ibs_ctx* c, const double* send, double* recv, int64_t count_per_rank) {
  if (!c || !send || !recv || count_per_rank < 0) return fail(IBS_ERR_ARG, "bad arguments");
  if (!c->comm) return fail(IBS_ERR_ARG, "no communicator: call ibs_comm_init first");
  ON_DEVICE(c);
  const int rc = rccl().AllGather(send, recv, (size_t)count_per_rank, kNcclFloat64, c->comm, c->stream);
  return rc ? nccl_fail("ncclAllGather", rc) : 0;
}

// Overlapped form: the gather is ordered after everything enqueued so far on the context's stream but runs on the
// communicator's own stream, so the next scan does not wait for the ranks to meet.
int ibs_comm_allgather_start_f64(ibs_ctx* c, const double* send, double* recv, int64_t count_per_rank, int32_t slot,
                                 int32_t then_wait_slot) {
  // then_wait_slot: >= 0 device-side wait of the context's stream on that slot's gather; -1 nothing;
  //                 <= -2 HOST-side wait on slot (-2 - then_wait_slot): no stream operation at all (an event query, and a
  //                 blocking wait only if that gather has not finished) -- for callers that run several slots ahead
  const int host_slot = then_wait_slot <= -2 ? -2 - then_wait_slot : -1;
  if (!c || !send || !recv || count_per_rank < 0 || slot < 0 || slot >= ibs_ctx::kCommSlots ||
      then_wait_slot >= ibs_ctx::kCommSlots || then_wait_slot == slot || host_slot >= ibs_ctx::kCommSlots || host_slot == slot)
    return fail(IBS_ERR_ARG, "bad arguments");
  if (!c->comm) return fail(IBS_ERR_ARG, "no communicator: call ibs_comm_init first");
  ON_DEVICE(c);
  if (!c->comm_stream) {
    HIPCHK(hipStreamCreateWithFlags(&c->comm_stream, hipStreamNonBlocking));
    HIPCHK(hipEventCreateWithFlags(&c->comm_ready, hipEventDisableTiming));
    for (auto& e : c->comm_done) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  }
  HIPCHK(hipEventRecord(c->comm_ready, c->stream));
  HIPCHK(hipStreamWaitEvent(c->comm_stream, c->comm_ready, 0));
  const int rc = rccl().AllGather(send, recv, (size_t)count_per_rank, kNcclFloat64, c->comm, c->comm_stream);
  if (rc) return nccl_fail("ncclAllGather", rc);
  HIPCHK(hipEventRecord(c->comm_done[slot], c->comm_stream));
  c->comm_pending[slot] = true;
  if (then_wait_slot >= 0 && c->comm_pending[then_wait_slot]) {      // (saves the caller a second call per step)
    HIPCHK(hipStreamWaitEvent(c->stream, c->comm_done[then_wait_slot], 0));
    c->comm_pending[then_wait_slot] = false;
  }
  if (host_slot >= 0 && c->comm_pending[host_slot]) {
    if (hipEventQuery(c->comm_done[host_slot]) != hipSuccess) HIPCHK(hipEventSynchronize(c->comm_done[host_slot]));
    c->comm_pending[host_slot] = false;
  }
  return 0;
}

int ibs_comm_wait(ibs_ctx* c, int32_t slot) {
  if (!c || slot >= ibs_ctx::kCommSlots) return fail(IBS_ERR_ARG, "bad arguments");
  ON_DEVICE(c);
  for (int s = 0; s < ibs_ctx::kCommSlots; ++s) {
    if ((slot >= 0 && s != slot) || !c->comm_pending[s]) continue;
    HIPCHK(hipStreamWaitEvent(c->stream, c->comm_done[s], 0));      // (device-side ordering; the host does not block)
    c->comm_pending[s] = false;
  }
  return 0;
}

int ibs_comm_destroy(ibs_ctx* c) {
  if (!c) return fail(IBS_ERR_ARG, "null context");
  if (c->comm_stream) {
    ON_DEVICE(c);
    (void)hipStreamSynchronize(c->comm_stream);
    for (auto& e : c->comm_done) { if (e) (void)hipEventDestroy(e); e = nullptr; }
    if (c->comm_ready) (void)hipEventDestroy(c->comm_ready);
    c->comm_ready = nullptr;
    (void)hipStreamDestroy(c->comm_stream);
    c->comm_stream = nullptr;
    for (auto& b : c->comm_pending) b = false;
  }
  if (c->comm) {
    ON_DEVICE(c);
    (void)hipStreamSynchronize(c->stream);
    const int rc = rccl().CommDestroy(c->comm);
    c->comm = nullptr;
    if (rc) return nccl_fail("ncclCommDestroy", rc);
  }
  return 0;
}

int ibs_synchronize(ibs_ctx* c) {
  if (!c) return fail(IBS_ERR_ARG, "null context");
  ON_DEVICE(c);
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

int ibs_solve_gcf_f64(ibs_ctx* ctx, int64_t n_sys, int32_t N, double h, const double* g, const double* c,
                      const double* f, int64_t ld, double* lam, double* gam, double* X, double* dX,
                      int32_t* info, int32_t mem) {
  return solve_gcf_impl<double>(ctx, n_sys, N, h, g, c, f, ld, lam, gam, X, dX, info, mem);
}

int ibs_solve_gcfh_f64(ibs_ctx* ctx, int64_t n_sys, int32_t N, double h, const double* g, const double* gh,
                       const double* c, const double* f, int64_t ld, double* lam, double* gam, double* X, double* dX,
                       int32_t* info, int32_t mem) {
  if (!gh) return fail(IBS_ERR_ARG, "gh is null");
  return solve_gcf_impl<double>(ctx, n_sys, N, h, g, c, f, ld, lam, gam, X, dX, info, mem, gh);
}

int ibs_solve_gcf_f32(ibs_ctx* ctx, int64_t n_sys, int32_t N, float h, const float* g, const float* c,
                      const float* f, int64_t ld, float* lam, float* gam, float* X, float* dX,
                      int32_t* info, int32_t mem) {
  return solve_gcf_impl<float>(ctx, n_sys, N, h, g, c, f, ld, lam, gam, X, dX, info, mem);
}

// ---- the eigenpair nearest sigma (ibs_nearest.hip; utils.py:1597)
// the persistent grid of long_waves() with its workspace in ctx->long_ws (nearest_ws_doubles(N) per wave)
int ibs_solve_gcf_nearest_f64(ibs_ctx* ctx, int64_t n_sys, int32_t N, double h, const double* g, const double* gh,
                              const double* c, const double* f, int64_t ld, const double* sigma, double* lam,
                              int32_t* idx, double* gam, double* X, double* dX, int32_t* info, int32_t mem) {
  if (!ctx) return fail(IBS_ERR_ARG, "null context");
  if (n_sys < 0 || !g || !c || !f || !sigma || ld < N)
    return fail(IBS_ERR_ARG, "bad arguments (n_sys=%lld ld=%lld N=%d)", (long long)n_sys, (long long)ld, N);
  if (int r = check_grid(N, h, true)) return r;
  if (n_sys == 0) return 0;
  ON_DEVICE(ctx);
  const size_t in_elems = (size_t)n_sys * ld, out_elems = (size_t)n_sys * N;
  ibs::NearestArgs a{};
  a.n_sys = n_sys; a.N = N; a.h = h; a.ld = ld;
  auto decl = [&](Stage& s) {
    a.g = s.in(g, in_elems); a.c = s.in(c, in_elems); a.f = s.in(f, in_elems); a.gh = s.in(gh, in_elems); a.sigma = s.in(sigma, n_sys);
    a.lam = s.out(lam, n_sys); a.gam = s.out(gam, n_sys); a.idx = s.out(idx, n_sys); a.X = s.out(X, out_elems); a.dX = s.out(dX, out_elems);
    a.info = s.status(info, n_sys);
  };
  return staged(ctx, mem, decl, [&]() -> int {
    if (int r = with_wave_ws(ctx, a, a.n_sys, ibs::nearest_ws_doubles(N))) return r;
    HIPCHK(ibs::launch_gcf_nearest(a, ctx->stream));
    return 0;
  });
}

// ---- spectrum mode: the n_modes largest eigenpairs of every system (ibs_modes.hip)
// the persistent grid of long_waves() with its workspace in ctx->long_ws (modes_ws_doubles(N) per wave)
static int check_n_modes(int32_t n_modes) {
  if (n_modes < 1 || n_modes > ibs::kMaxModes) return fail(IBS_ERR_ARG, "n_modes=%d outside [1, %d]", n_modes, ibs::kMaxModes);
  return 0;
}
int ibs_solve_gcf_modes_f64(ibs_ctx* ctx, int64_t n_sys, int32_t N, double h, const double* g, const double* gh, const double* c,
                            const double* f, int64_t ld, int32_t n_modes, double* lam, double* gam, double* X, double* dX,
                            int32_t* info, int32_t mem) {
  if (!ctx) return fail(IBS_ERR_ARG, "null context");
  if (n_sys < 0 || !g || !c || !f || ld < N)
    return fail(IBS_ERR_ARG, "bad arguments (n_sys=%lld ld=%lld N=%d)", (long long)n_sys, (long long)ld, N);
  if (int r = check_n_modes(n_modes)) return r;
  if (!lam && !gam && !X && !dX && !info) return fail(IBS_ERR_ARG, "no output requested (lam, gam, X, dX and info are all null)");
  if (int r = check_grid(N, h, true)) return r;
  if (n_sys == 0) return 0;
  ON_DEVICE(ctx);
  const size_t in_elems = (size_t)n_sys * ld, n_out = (size_t)n_sys * n_modes, out_elems = n_out * N;
  ibs::ModesArgs a{};
  a.n_sys = n_sys; a.N = N; a.h = h; a.ld = ld; a.n_modes = n_modes;
  auto decl = [&](Stage& s) {
    a.g = s.in(g, in_elems); a.c = s.in(c, in_elems); a.f = s.in(f, in_elems); a.gh = s.in(gh, in_elems);
    a.lam = s.out(lam, n_out); a.gam = s.out(gam, n_out); a.X = s.out(X, out_elems); a.dX = s.out(dX, out_elems);
    a.info = s.status(info, n_out);
  };
  return staged(ctx, mem, decl, [&]() -> int {
    if (int r = with_wave_ws(ctx, a, a.n_sys, ibs::modes_ws_doubles(N))) return r;
    HIPCHK(ibs::launch_gcf_modes(a, ctx->stream));
    return 0;
  });
}

// ---- spectrum mode with an F-orthonormal Ritz basis of every cluster of modes (ibs_modes_basis.hip)
// the same persistent grid, basis_ws_doubles(N) of ctx->long_ws per wave; the members' vectors are built in the caller's X rows
int ibs_solve_gcf_modes_basis_f64(ibs_ctx* ctx, int64_t n_sys, int32_t N, double h, const double* g, const double* gh, const double* c,
                                  const double* f, int64_t ld, int32_t n_modes, double* lam, double* gam, double* X, double* dX,
                                  int32_t* cluster_first, int32_t* info, int32_t mem) {
  if (!ctx) return fail(IBS_ERR_ARG, "null context");
  if (n_sys < 0 || !g || !c || !f || ld < N)
    return fail(IBS_ERR_ARG, "bad arguments (n_sys=%lld ld=%lld N=%d)", (long long)n_sys, (long long)ld, N);
  if (int r = check_n_modes(n_modes)) return r;
  if (!X) return fail(IBS_ERR_ARG, "X is null (the basis of a cluster is built in the caller's X rows)");
  if (int r = check_grid(N, h, true)) return r;
  if (n_sys == 0) return 0;
  ON_DEVICE(ctx);
  const size_t in_elems = (size_t)n_sys * ld, n_out = (size_t)n_sys * n_modes, out_elems = n_out * N;
  ibs::ModesBasisArgs a{};
  a.n_sys = n_sys; a.N = N; a.h = h; a.ld = ld; a.n_modes = n_modes;
  auto decl = [&](Stage& s) {
    a.g = s.in(g, in_elems); a.c = s.in(c, in_elems); a.f = s.in(f, in_elems); a.gh = s.in(gh, in_elems);
    a.lam = s.out(lam, n_out); a.gam = s.out(gam, n_out); a.X = s.out(X, out_elems); a.dX = s.out(dX, out_elems);
    a.cluster_first = s.out(cluster_first, n_out); a.info = s.status(info, n_out);
  };
  return staged(ctx, mem, decl, [&]() -> int {
    if (int r = with_wave_ws(ctx, a, a.n_sys, ibs::basis_ws_doubles(N))) return r;
    HIPCHK(ibs::launch_gcf_modes_basis(a, ctx->stream));
    return 0;
  });
}

// ---- exact vector-Jacobian product of gam and lam in the (g, c, f) rows (ibs_vjp.hip)
// the persistent grid of long_waves() with its workspace in ctx->long_ws (vjp_ws_doubles(N) per wave)
int ibs_solve_gcf_vjp_f64(ibs_ctx* ctx, int64_t n_sys, int32_t N, double h, const double* g, const double* c, const double* f,
                          int64_t ld, const double* lam, const double* X, const double* gam_bar, const double* lam_bar, double* g_bar,
                          double* c_bar, double* f_bar, int32_t* info, int32_t mem) {
  if (!ctx) return fail(IBS_ERR_ARG, "null context");
  if (n_sys < 0 || !g || !c || !f || !lam || !X || !g_bar || !c_bar || !f_bar || ld < N)
    return fail(IBS_ERR_ARG, "bad arguments (n_sys=%lld ld=%lld N=%d)", (long long)n_sys, (long long)ld, N);
  if (!gam_bar && !lam_bar) return fail(IBS_ERR_ARG, "gam_bar and lam_bar are both null");
  if (int r = check_grid(N, h, true)) return r;
  if (n_sys == 0) return 0;
  ON_DEVICE(ctx);
  const size_t rows = (size_t)n_sys * ld;
  ibs::VjpArgs a{};
  a.n_sys = n_sys; a.N = N; a.h = h; a.ld = ld;
  auto decl = [&](Stage& s) {
    a.g = s.in(g, rows); a.c = s.in(c, rows); a.f = s.in(f, rows); a.X = s.in(X, rows);
    a.lam = s.in(lam, n_sys); a.gam_bar = s.in(gam_bar, n_sys); a.lam_bar = s.in(lam_bar, n_sys);
    a.g_bar = s.out(g_bar, rows); a.c_bar = s.out(c_bar, rows); a.f_bar = s.out(f_bar, rows);
    a.info = s.status(info, n_sys);
  };
  return staged(ctx, mem, decl, [&]() -> int {
    if (mem == IBS_MEM_HOST && ld > N)                  // (host pointers: the padding columns come back as zero)
      for (double* o : {a.g_bar, a.c_bar, a.f_bar}) HIPCHK(hipMemsetAsync(o, 0, rows * sizeof(double), ctx->stream));
    if (int r = with_wave_ws(ctx, a, a.n_sys, ibs::vjp_ws_doubles(N))) return r;
    HIPCHK(ibs::launch_gcf_vjp(a, ctx->stream));
    return 0;
  });
}

// ---- marginal stability: the critical scale s* of the pressure gradient at fixed rows (ibs_marginal.hip; nothing upstream corresponds:
// c is linear in dPdrho, utils.py:1560-1562, and the quantity generalises the scan of bishop_ball_s-alpha.py:90-115)
// the persistent grid of long_waves() with its workspace in ctx->long_ws (ibs::marginal_ws per wave)
int ibs_marginal_gcf_f64(ibs_ctx* ctx, int64_t n_sys, int32_t N, double h, const double* g, const double* c, int64_t ld,
                         double* scale, double* mu, double* X, double* gam0, double* g_bar, double* c_bar, int32_t* info, int32_t mem) {
  if (!ctx) return fail(IBS_ERR_ARG, "null context");
  if (!g || !c || !scale) return fail(IBS_ERR_ARG, "null argument (g, c and scale are required)");
  if (n_sys < 0 || ld < N) return fail(IBS_ERR_ARG, "bad arguments (n_sys=%lld ld=%lld N=%d)", (long long)n_sys, (long long)ld, N);
  if (int r = check_grid(N, h, true)) return r;
  if (n_sys == 0) return 0;
  ON_DEVICE(ctx);
  const size_t in_elems = (size_t)n_sys * ld, out_elems = (size_t)n_sys * N;
  ibs::MarginalArgs a{};
  a.n_sys = n_sys; a.N = N; a.h = h; a.ld = ld;
  auto decl = [&](Stage& s) {
    a.g = s.in(g, in_elems); a.c = s.in(c, in_elems);
    a.scale = s.out(scale, n_sys); a.mu = s.out(mu, n_sys); a.gam0 = s.out(gam0, n_sys);
    a.X = s.out(X, out_elems); a.g_bar = s.out(g_bar, out_elems); a.c_bar = s.out(c_bar, out_elems);
    a.info = s.status(info, n_sys);
  };
  return staged(ctx, mem, decl, [&]() -> int {
    if (int r = with_wave_ws(ctx, a, a.n_sys, ibs::marginal_ws(N, false).total)) return r;
    HIPCHK(ibs::launch_marginal_gcf(a, ctx->stream));
    return 0;
  });
}

int ibs_marginal_scan_f64(ibs_ctx* ctx, int32_t n_lines, int32_t n_theta0, int32_t N, double h, const double* bmag,
                          const double* gradpar, const double* cvdrift, const double* cvdrift0, const double* gds2,
                          const double* gds21, const double* gds22, int64_t ld, const double* dPdrho, const double* theta0,
                          double* scale, double* mu, double* dscale_dtheta0, double* dscale_ddPdrho, int32_t* info, int32_t mem) {
  const GeoLines geo{{bmag, gradpar, cvdrift, cvdrift0, gds2, gds21, gds22}, ld, dPdrho, theta0};
  if (!ctx) return fail(IBS_ERR_ARG, "null context");
  if (!geo.present() || !dPdrho || !theta0 || !scale)
    return fail(IBS_ERR_ARG, "null argument (the geometry arrays, dPdrho, theta0 and scale are required)");
  if (n_lines < 0 || n_theta0 < 0 || ld < N)
    return fail(IBS_ERR_ARG, "bad arguments (n_lines=%d n_theta0=%d ld=%lld N=%d)", n_lines, n_theta0, (long long)ld, N);
  if (int r = check_grid(N, h, true)) return r;
  if (n_lines == 0 || n_theta0 == 0) return 0;
  ON_DEVICE(ctx);
  const size_t n_sys = (size_t)n_lines * n_theta0;
  ibs::MarginalScanArgs a{};
  a.n_lines = n_lines; a.n_theta0 = n_theta0; a.N = N; a.h = h; a.ld = (long)ld;
  auto decl = [&](Stage& s) {
    geo.declare(s, n_lines, n_theta0).into(a);
    a.scale = s.out(scale, n_sys); a.mu = s.out(mu, n_sys); a.dth0 = s.out(dscale_dtheta0, n_sys); a.ddP = s.out(dscale_ddPdrho, n_sys);
    a.info = s.status(info, n_sys);
  };
  return staged(ctx, mem, decl, [&]() -> int {
    if (int r = with_wave_ws(ctx, a, (long)n_sys, ibs::marginal_ws(N, true).total)) return r;
    HIPCHK(ibs::launch_marginal_scan(a, ctx->stream));
    return 0;
  });
}

// mu = 1 / s* maximised over theta0 on every line (k_marginal_theta0_polish; the rule: ibs_theta0_polish.hpp).  The argument checks are
// those of ibs_theta0_polish_f64, before the context; the grid and the workspace those of ibs_marginal_scan_f64
int ibs_marginal_theta0_polish_f64(ibs_ctx* ctx, int32_t n_lines, int32_t n_theta0, int32_t N, double h, const double* bmag,
                                   const double* gradpar, const double* cvdrift, const double* cvdrift0, const double* gds2,
                                   const double* gds21, const double* gds22, int64_t ld, const double* dPdrho, const double* theta0,
                                   const double* mu, const int32_t* node_in, int32_t n_starts, double xtol, int32_t max_eval,
                                   double* theta0_star, double* mu_star, double* scale_star, int32_t* node, int32_t* n_eval,
                                   int32_t* info, int32_t* n_found, int32_t mem) {
  const GeoLines geo{{bmag, gradpar, cvdrift, cvdrift0, gds2, gds21, gds22}, ld, dPdrho, theta0};
  if (n_starts < 1 || n_starts > ibs::t0p::kMaxSlots || !(xtol > 0) || !std::isfinite(xtol) || max_eval < 1 ||
      max_eval > ibs::t0p::kMaxEval)
    return fail(IBS_ERR_ARG, "n_starts in [1, %d], xtol > 0 and finite, max_eval in [1, %d] required (n_starts=%d xtol=%g max_eval=%d)",
                ibs::t0p::kMaxSlots, ibs::t0p::kMaxEval, n_starts, xtol, max_eval);
  if (n_lines < 0 || n_theta0 < 1 || N < 1 || !geo.present() || !dPdrho || !theta0 || !mu || !theta0_star || !mu_star || ld < N)
    return fail(IBS_ERR_ARG, "bad arguments (n_lines=%d n_theta0=%d ld=%lld N=%d; the arrays, theta0, mu, theta0_star and mu_star are required)",
                n_lines, n_theta0, (long long)ld, N);
  if (int r = check_grid(N, h, true)) return r;
  const bool host = mem == IBS_MEM_HOST;
  if (host && !ibs::t0p::grid_ok(theta0, n_theta0)) return fail(IBS_ERR_ARG, "theta0 must be finite and strictly increasing");
  if (!ctx) return fail(IBS_ERR_ARG, "null context");
  if (n_lines == 0) return 0;
  ON_DEVICE(ctx);
  ibs::MarginalPolishArgs a{};
  a.n_lines = n_lines; a.n_theta0 = n_theta0; a.N = N; a.h = h; a.ld = (long)ld;
  a.n_starts = n_starts; a.xtol = xtol; a.max_eval = max_eval;
  const size_t n_sys = (size_t)n_lines * n_theta0, n_slots = (size_t)n_lines * n_starts;
  auto decl = [&](Stage& s) {
    geo.declare(s, n_lines, n_theta0).into(a); a.mu = s.in(mu, n_sys); a.node_in = s.in(node_in, n_slots);
    a.theta0_star = s.out(theta0_star, n_slots); a.mu_star = s.out(mu_star, n_slots); a.scale_star = s.out(scale_star, n_slots);
    a.node = s.out(node, n_slots); a.n_eval = s.out(n_eval, n_slots); a.n_found = s.out(n_found, (size_t)n_lines);
    a.info = s.status(info, n_slots);
  };
  return staged(ctx, mem, decl, [&]() -> int {
    if (int r = with_wave_ws(ctx, a, (long)n_slots, ibs::marginal_ws(N, true).total)) return r;
    HIPCHK(ibs::launch_marginal_theta0_polish(a, ctx->stream));
    return 0;
  });
}

// the objective of the margin's refinement in (alpha, theta0): val = -mu = -1 / s* and its gradient at geometry-fed points (k_marginal_points)
int ibs_marginal_obj_w_grad_f64(ibs_ctx* ctx, int32_t n_pts, int32_t N, double h, const double* geo, int64_t ld,
                                const double* theta0, double del_alpha, double* val, double* jac, double* scale, double* dscale,
                                double* dPdrho, int32_t* info, int32_t mem) {
  if (!ctx) return fail(IBS_ERR_ARG, "null context");
  if (!geo || !theta0 || !val) return fail(IBS_ERR_ARG, "null argument (geo, theta0 and val are required)");
  if (n_pts < 0 || ld < N || !(del_alpha > 0))
    return fail(IBS_ERR_ARG, "bad arguments (n_pts=%d ld=%lld N=%d del_alpha=%g)", n_pts, (long long)ld, N, del_alpha);
  if (int r = check_grid(N, h, true)) return r;
  if (n_pts == 0) return 0;
  ON_DEVICE(ctx);
  const size_t n = (size_t)n_pts, geo_elems = n * 3 * 8 * (size_t)ld;
  ibs::MarginalPointsArgs a{};
  a.n_pts = n_pts; a.N = N; a.h = h; a.ld = (long)ld; a.del_alpha = del_alpha;
  auto decl = [&](Stage& s) {
    a.geo = s.in(geo, geo_elems); a.theta0 = s.in(theta0, n);
    a.val = s.out(val, n); a.jac = s.out(jac, 2 * n); a.scale = s.out(scale, n); a.dscale = s.out(dscale, 2 * n);
    a.dPdrho = s.out(dPdrho, n);
    a.info = s.status(info, n);
  };
  return staged(ctx, mem, decl, [&]() -> int {
    if (int r = with_wave_ws(ctx, a, a.n_pts, ibs::marginal_ws(N, true).total)) return r;
    HIPCHK(ibs::launch_marginal_points(a, ctx->stream));
    return 0;
  });
}

// the same objective from ONE line per point and the alpha-tangent of its geometry: the gradient exact in alpha as well, and the
// cotangent planes of s* for the geometry's VJP (k_marginal_tangent_points)
int ibs_marginal_obj_w_grad_tangent_f64(ibs_ctx* ctx, int32_t n_pts, int32_t N, double h, const double* geo, const double* geo_da,
                                        int64_t ld, const double* theta0, double* val, double* jac, double* scale, double* dscale,
                                        double* dPdrho, double* geo_bar, int32_t* info, int32_t mem) {
  if (!ctx) return fail(IBS_ERR_ARG, "null context");
  if (!geo || !theta0 || !val) return fail(IBS_ERR_ARG, "null argument (geo, theta0 and val are required)");
  if (!geo_da && (jac || dscale)) return fail(IBS_ERR_ARG, "null geo_da (required with jac or dscale)");
  if (n_pts < 0 || ld < N) return fail(IBS_ERR_ARG, "bad arguments (n_pts=%d ld=%lld N=%d)", n_pts, (long long)ld, N);
  if (int r = check_grid(N, h, true)) return r;
  if (n_pts == 0) return 0;
  ON_DEVICE(ctx);
  const size_t n = (size_t)n_pts, geo_elems = n * 8 * (size_t)ld;
  ibs::MarginalTangentArgs a{};
  a.n_pts = n_pts; a.N = N; a.h = h; a.ld = (long)ld;
  // (host pointers: the rows of geo_bar are packed on the device and come back one by one, so the caller's entries N..ld-1 stay as they were)
  auto decl = [&](Stage& s) {
    a.geo = s.in(geo, geo_elems); a.geo_da = s.in(geo_da, geo_elems); a.theta0 = s.in(theta0, n);
    a.val = s.out(val, n); a.jac = s.out(jac, 2 * n); a.scale = s.out(scale, n); a.dscale = s.out(dscale, 2 * n);
    a.dPdrho = s.out(dPdrho, n);
    a.geo_bar = s.out_rows(geo_bar, 8 * n, N, ld); a.ld_bar = (long)s.rows_ld(N, ld);
    a.info = s.status(info, n);
  };
  return staged(ctx, mem, decl, [&]() -> int {
    if (int r = with_wave_ws(ctx, a, a.n_pts, ibs::marginal_ws(N, true).total)) return r;
    HIPCHK(ibs::launch_marginal_tangent_points(a, ctx->stream));
    return 0;
  });
}

// ---- local-equilibrium scan: shear and pressure variations of every line (ibs_local_eq.hip; the rule: ibs_local_eq.hpp).  Whole lines
// chunk after chunk (for_line_chunks, a line's n_var variations standing where the theta0 values of a scan stand); a chunk's workspace
// in ctx->long_ws = the per-wave workspace (ibs::local_eq_ws) of its persistent grid: long_waves() waves, and never more than
// kLineChunkBudget admits, so that one line with many variations on a long grid stays within the budget as well
int ibs_local_eq_scan_f64(ibs_ctx* ctx, int32_t n_lines, int32_t n_var, int32_t N, double theta_lo, double h, const double* geo,
                          int64_t ld, const double* dPdrho, const double* centre, const double* sigma, const double* ps, int64_t ps_ld,
                          const double* var, double shift, double* gam, double* lam, int32_t* count, int32_t* info, int flags) {
  if (!ctx) return fail(IBS_ERR_ARG, "null context");
  if (!geo || !dPdrho || !centre || !sigma || !var)
    return fail(IBS_ERR_ARG, "null argument (geo, dPdrho, centre, sigma and var are required)");
  if (!gam && !lam && !count) return fail(IBS_ERR_ARG, "no output requested (gam, lam and count are all null)");
  if (n_lines < 0 || n_var < 1 || ld < N || (ps && ps_ld < N))
    return fail(IBS_ERR_ARG, "bad arguments (n_lines=%d n_var=%d ld=%lld ps_ld=%lld N=%d)", n_lines, n_var, (long long)ld, (long long)ps_ld, N);
  if (flags != IBS_MEM_DEVICE && flags != IBS_MEM_HOST) return fail(IBS_ERR_ARG, "flags must be IBS_MEM_DEVICE or IBS_MEM_HOST, not %d", flags);
  if (!std::isfinite(theta_lo) || (count && !std::isfinite(shift)))
    return fail(IBS_ERR_ARG, "theta_lo and the shift of a requested count must be finite (theta_lo=%g shift=%g)", theta_lo, shift);
  if (int r = check_grid(N, h, true)) return r;
  if (n_lines == 0) return 0;
  ON_DEVICE(ctx);
  const size_t n_sys = (size_t)n_lines * n_var, plane = (size_t)n_lines * (size_t)ld;
  ibs::LocalEqArgs a{};                                    // the whole call; each chunk launches a copy with its lines
  a.n_var = n_var; a.N = N; a.theta_lo = theta_lo; a.h = h; a.ld = (long)ld; a.plane = plane; a.ps_ld = (long)ps_ld; a.shift = shift;
  auto decl = [&](Stage& s) {
    a.geo = s.in(geo, 8 * plane); a.dPdrho = s.in(dPdrho, n_lines); a.centre = s.in(centre, n_lines); a.sigma = s.in(sigma, n_lines);
    a.ps = s.in(ps, (size_t)n_lines * (size_t)ps_ld); a.var = s.in(var, 3 * (size_t)n_var);
    a.gam = s.out(gam, n_sys); a.lam = s.out(lam, n_sys); a.count = s.out(count, n_sys);
    a.info = s.status(info, n_sys);
  };
  return staged(ctx, flags, decl, [&]() -> int {
    const size_t per_wave = ibs::local_eq_ws(N).total;
    const long wave_cap = (long)(ibs::kLineChunkBudget / (per_wave * sizeof(double)));      // (>= 340: a wave's workspace is at most 3 MB)
    long nw = 0;
    double* work = nullptr;
    auto carve = [&](Carve& cv, long L) {                  // ctx->long_ws of a chunk of L lines
      nw = long_waves(ctx, L * n_var);
      if (nw > wave_cap) nw = wave_cap;
      work = cv.take<double>((size_t)nw * per_wave);
    };
    return for_line_chunks(ctx, "local_eq_scan", n_lines, n_var, N, carve, [&](long l0, long Lc) -> int {
      const long s0 = l0 * n_var;
      ibs::LocalEqArgs c = a;
      c.n_lines = (int)Lc;
      c.geo = a.geo + l0 * ld; c.dPdrho = a.dPdrho + l0; c.centre = a.centre + l0; c.sigma = a.sigma + l0;
      c.ps = a.ps ? a.ps + l0 * ps_ld : nullptr;
      c.gam = a.gam ? a.gam + s0 : nullptr; c.lam = a.lam ? a.lam + s0 : nullptr; c.count = a.count ? a.count + s0 : nullptr;
      c.info = a.info ? a.info + s0 : nullptr;
      c.work = work; c.work_doubles = (size_t)nw * per_wave; c.n_waves = nw;
      HIPCHK(ibs::launch_local_eq_scan(c, ctx->stream));
      return 0;
    });
  });
}

// ---- local-equilibrium boundaries: the crossings of the stability boundary along rays in (eps, p) of every line
// (ibs_local_eq_boundary.hip; the rule for a ray: ibs_local_eq_boundary.hpp).  Whole lines chunk after chunk exactly as the scan above, a
// line's n_ray rays standing where its variations stand; the kernel forms its rows in LDS, so a chunk carves nothing from ctx->long_ws
int ibs_local_eq_boundary_f64(ibs_ctx* ctx, int32_t n_lines, int32_t n_ray, int32_t N, double theta_lo, double h, const double* geo,
                              int64_t ld, const double* dPdrho, const double* centre, const double* sigma, const double* ps,
                              int64_t ps_ld, const double* rays, double shift, int32_t max_cross, double xtol, double* t_stable,
                              double* t_unstable, int32_t* n_cross, int32_t* lo_unstable, int32_t* node_count, int32_t* info, int flags) {
  if (!ctx) return fail(IBS_ERR_ARG, "null context");
  if (!geo || !dPdrho || !centre || !sigma || !rays || !t_stable || !t_unstable || !n_cross)
    return fail(IBS_ERR_ARG, "null argument (geo, dPdrho, centre, sigma, rays, t_stable, t_unstable and n_cross are required)");
  if (n_lines < 0 || n_ray < 1 || ld < N || (ps && ps_ld < N))
    return fail(IBS_ERR_ARG, "bad arguments (n_lines=%d n_ray=%d ld=%lld ps_ld=%lld N=%d)", n_lines, n_ray, (long long)ld, (long long)ps_ld, N);
  if (max_cross < 1 || max_cross > ibs::kMaxCross || !(xtol >= 0.0 && xtol < 1.0))
    return fail(IBS_ERR_ARG, "max_cross must lie in [1, %d] and xtol in [0, 1) (max_cross=%d xtol=%g)", ibs::kMaxCross, max_cross, xtol);
  if (flags != IBS_MEM_DEVICE && flags != IBS_MEM_HOST) return fail(IBS_ERR_ARG, "flags must be IBS_MEM_DEVICE or IBS_MEM_HOST, not %d", flags);
  if (!std::isfinite(theta_lo) || !std::isfinite(shift))
    return fail(IBS_ERR_ARG, "theta_lo and shift must be finite (theta_lo=%g shift=%g)", theta_lo, shift);
  if (int r = check_grid(N, h, true)) return r;
  if (n_lines == 0) return 0;
  ON_DEVICE(ctx);
  const size_t n_sys = (size_t)n_lines * n_ray, plane = (size_t)n_lines * (size_t)ld;
  ibs::LocalEqBoundaryArgs a{};                            // the whole call; each chunk launches a copy with its lines
  a.n_ray = n_ray; a.N = N; a.theta_lo = theta_lo; a.h = h; a.ld = (long)ld; a.plane = plane; a.ps_ld = (long)ps_ld; a.shift = shift;
  a.max_cross = max_cross; a.xtol = xtol;
  auto decl = [&](Stage& s) {
    a.geo = s.in(geo, 8 * plane); a.dPdrho = s.in(dPdrho, n_lines); a.centre = s.in(centre, n_lines); a.sigma = s.in(sigma, n_lines);
    a.ps = s.in(ps, (size_t)n_lines * (size_t)ps_ld); a.rays = s.in(rays, 7 * (size_t)n_ray);
    a.t_stable = s.out(t_stable, n_sys * max_cross); a.t_unstable = s.out(t_unstable, n_sys * max_cross); a.n_cross = s.out(n_cross, n_sys);
    a.lo_unstable = s.out(lo_unstable, n_sys); a.node_count = s.out(node_count, n_sys * 64);
    a.info = s.status(info, n_sys);
  };
  return staged(ctx, flags, decl, [&]() -> int {
    auto carve = [&](Carve&, long) {};                     // (no per-wave workspace)
    return for_line_chunks(ctx, "local_eq_boundary", n_lines, n_ray, N, carve, [&](long l0, long Lc) -> int {
      const long s0 = l0 * n_ray;
      ibs::LocalEqBoundaryArgs c = a;
      c.n_lines = (int)Lc;
      c.geo = a.geo + l0 * ld; c.dPdrho = a.dPdrho + l0; c.centre = a.centre + l0; c.sigma = a.sigma + l0;
      c.ps = a.ps ? a.ps + l0 * ps_ld : nullptr;
      c.t_stable = a.t_stable + s0 * max_cross; c.t_unstable = a.t_unstable + s0 * max_cross; c.n_cross = a.n_cross + s0;
      c.lo_unstable = a.lo_unstable ? a.lo_unstable + s0 : nullptr; c.node_count = a.node_count ? a.node_count + s0 * 64 : nullptr;
      c.info = a.info ? a.info + s0 : nullptr;
      c.n_waves = long_waves(ctx, Lc * n_ray);
      HIPCHK(ibs::launch_local_eq_boundary(c, ctx->stream));
      return 0;
    });
  });
}

// ---- local-equilibrium boundaries minimised over theta0: the first-stability parameter of every (line, ray family) between the nodes of
// its coarse row (ibs_local_eq_boundary_polish.hip; the rule: ibs_local_eq_boundary_polish.hpp).  Whole lines chunk after chunk as above, a
// line's n_ray * n_starts slots standing where its rays stand; nothing is carved from ctx->long_ws
int ibs_local_eq_boundary_polish_f64(ibs_ctx* ctx, int32_t n_lines, int32_t n_ray, int32_t N, double theta_lo, double h, const double* geo,
                                     int64_t ld, const double* dPdrho, const double* centre, const double* sigma, const double* ps,
                                     int64_t ps_ld, const double* rays, int32_t n_theta0, const double* theta0, const double* t_row,
                                     double shift, double xtol, int32_t n_starts, double xtol_theta0, int32_t max_eval,
                                     double* theta0_out, double* t_out, double* t_stable_out, double* t_unstable_out, int32_t* node,
                                     int32_t* n_eval, int32_t* lo_unstable, int32_t* info, int32_t* n_found, int flags) {
  if (!ctx) return fail(IBS_ERR_ARG, "null context");
  if (!geo || !dPdrho || !centre || !sigma || !rays || !theta0 || !t_row || !theta0_out || !t_out || !t_stable_out || !t_unstable_out)
    return fail(IBS_ERR_ARG, "null argument (geo, dPdrho, centre, sigma, rays, theta0, t_row, theta0_out, t_out, t_stable_out and "
                "t_unstable_out are required)");
  if (n_lines < 0 || n_ray < 1 || ld < N || (ps && ps_ld < N) || n_theta0 < 1 || n_theta0 > ibs::kBoundaryPolishMaxTheta0)
    return fail(IBS_ERR_ARG, "bad arguments (n_lines=%d n_ray=%d ld=%lld ps_ld=%lld N=%d; n_theta0=%d must lie in [1, %d])", n_lines, n_ray,
                (long long)ld, (long long)ps_ld, N, n_theta0, ibs::kBoundaryPolishMaxTheta0);
  if (n_starts < 1 || n_starts > ibs::t0p::kMaxSlots || !(xtol_theta0 > 0) || !std::isfinite(xtol_theta0) || max_eval < 1 ||
      max_eval > ibs::t0p::kMaxEval || !(xtol >= 0.0 && xtol < 1.0))
    return fail(IBS_ERR_ARG, "n_starts in [1, %d], xtol_theta0 > 0 and finite, max_eval in [1, %d] and xtol in [0, 1) required "
                "(n_starts=%d xtol_theta0=%g max_eval=%d xtol=%g)", ibs::t0p::kMaxSlots, ibs::t0p::kMaxEval, n_starts, xtol_theta0,
                max_eval, xtol);
  if (flags != IBS_MEM_DEVICE && flags != IBS_MEM_HOST) return fail(IBS_ERR_ARG, "flags must be IBS_MEM_DEVICE or IBS_MEM_HOST, not %d", flags);
  if (!std::isfinite(theta_lo) || !std::isfinite(shift))
    return fail(IBS_ERR_ARG, "theta_lo and shift must be finite (theta_lo=%g shift=%g)", theta_lo, shift);
  if (int r = check_grid(N, h, true)) return r;
  if (flags == IBS_MEM_HOST && !ibs::t0p::grid_ok(theta0, n_theta0)) return fail(IBS_ERR_ARG, "theta0 must be finite and strictly increasing");
  if (n_lines == 0) return 0;
  ON_DEVICE(ctx);
  const int per_line = n_ray * n_starts;
  const size_t n_fam = (size_t)n_lines * n_ray, n_sys = n_fam * n_starts, plane = (size_t)n_lines * (size_t)ld;
  ibs::LocalEqBoundaryPolishArgs a{};                      // the whole call; each chunk launches a copy with its lines
  a.n_ray = n_ray; a.N = N; a.theta_lo = theta_lo; a.h = h; a.ld = (long)ld; a.plane = plane; a.ps_ld = (long)ps_ld; a.shift = shift;
  a.xtol = xtol; a.n_theta0 = n_theta0; a.n_starts = n_starts; a.xtol_theta0 = xtol_theta0; a.max_eval = max_eval;
  auto decl = [&](Stage& s) {
    a.geo = s.in(geo, 8 * plane); a.dPdrho = s.in(dPdrho, n_lines); a.centre = s.in(centre, n_lines); a.sigma = s.in(sigma, n_lines);
    a.ps = s.in(ps, (size_t)n_lines * (size_t)ps_ld); a.rays = s.in(rays, 7 * (size_t)n_ray); a.theta0 = s.in(theta0, n_theta0);
    a.t_row = s.in(t_row, n_fam * n_theta0);
    a.theta0_out = s.out(theta0_out, n_sys); a.t_out = s.out(t_out, n_sys); a.t_stable_out = s.out(t_stable_out, n_sys);
    a.t_unstable_out = s.out(t_unstable_out, n_sys); a.node = s.out(node, n_sys); a.n_eval = s.out(n_eval, n_sys);
    a.lo_unstable = s.out(lo_unstable, n_sys); a.n_found = s.out(n_found, n_fam);
    a.info = s.status(info, n_sys);
  };
  return staged(ctx, flags, decl, [&]() -> int {
    auto carve = [&](Carve&, long) {};                     // (no per-wave workspace)
    return for_line_chunks(ctx, "local_eq_boundary_polish", n_lines, per_line, N, carve, [&](long l0, long Lc) -> int {
      const long f0 = l0 * n_ray, s0 = f0 * n_starts;
      ibs::LocalEqBoundaryPolishArgs c = a;
      c.n_lines = (int)Lc;
      c.geo = a.geo + l0 * ld; c.dPdrho = a.dPdrho + l0; c.centre = a.centre + l0; c.sigma = a.sigma + l0;
      c.ps = a.ps ? a.ps + l0 * ps_ld : nullptr;
      c.t_row = a.t_row + f0 * n_theta0;
      c.theta0_out = a.theta0_out + s0; c.t_out = a.t_out + s0; c.t_stable_out = a.t_stable_out + s0; c.t_unstable_out = a.t_unstable_out + s0;
      c.node = a.node ? a.node + s0 : nullptr; c.n_eval = a.n_eval ? a.n_eval + s0 : nullptr;
      c.lo_unstable = a.lo_unstable ? a.lo_unstable + s0 : nullptr; c.n_found = a.n_found ? a.n_found + f0 : nullptr;
      c.info = a.info ? a.info + s0 : nullptr;
      c.n_waves = long_waves(ctx, Lc * per_line);
      HIPCHK(ibs::launch_local_eq_boundary_polish(c, ctx->stream));
      return 0;
    });
  });
}

// ---- local-equilibrium gradients: lam_max, gam, d lam_max / d (theta0, eps, p, dPdrho) and the cotangent planes at points (line, theta0,
// eps, p) (ibs_local_eq_grad.hip; the formulas: ibs_local_eq_grad.hpp).  The geometry is staged once; the POINTS go chunk after chunk
// (for_line_chunks with a point standing where a line with one theta0 stands), a chunk's workspace in ctx->long_ws = the per-wave
// workspace (ibs::local_eq_grad_ws) of its persistent grid: long_waves() waves, and never more than kLineChunkBudget admits
int ibs_local_eq_grad_f64(ibs_ctx* ctx, int32_t n_lines, int32_t n_pts, int32_t N, double theta_lo, double h, const double* geo,
                          int64_t ld, const double* dPdrho, const double* centre, const double* sigma, const double* ps, int64_t ps_ld,
                          const int32_t* line_of, const double* var, double* lam, double* gam, double* dlam, double* geo_bar,
                          int64_t ld_bar, int32_t* info, int flags) {
  if (!ctx) return fail(IBS_ERR_ARG, "null context");
  if (!geo || !dPdrho || !centre || !sigma || !line_of || !var)
    return fail(IBS_ERR_ARG, "null argument (geo, dPdrho, centre, sigma, line_of and var are required)");
  if (!lam && !gam && !dlam && !geo_bar) return fail(IBS_ERR_ARG, "no output requested (lam, gam, dlam and geo_bar are all null)");
  if (n_lines < 0 || n_pts < 0 || ld < N || (ps && ps_ld < N) || (geo_bar && ld_bar < N))
    return fail(IBS_ERR_ARG, "bad arguments (n_lines=%d n_pts=%d ld=%lld ps_ld=%lld ld_bar=%lld N=%d)", n_lines, n_pts, (long long)ld,
                (long long)ps_ld, (long long)ld_bar, N);
  if (flags != IBS_MEM_DEVICE && flags != IBS_MEM_HOST) return fail(IBS_ERR_ARG, "flags must be IBS_MEM_DEVICE or IBS_MEM_HOST, not %d", flags);
  if (!std::isfinite(theta_lo)) return fail(IBS_ERR_ARG, "theta_lo must be finite (theta_lo=%g)", theta_lo);
  if (int r = check_grid(N, h, true)) return r;
  if (n_pts == 0) return 0;
  ON_DEVICE(ctx);
  const size_t n = (size_t)n_pts, plane = (size_t)n_lines * (size_t)ld;
  ibs::LocalEqGradArgs a{};                                // the whole call; each chunk launches a copy with its points
  a.n_lines = n_lines; a.N = N; a.theta_lo = theta_lo; a.h = h; a.ld = (long)ld; a.plane = plane; a.ps_ld = (long)ps_ld;
  // (host pointers: the rows of geo_bar are packed on the device and come back one by one, so the caller's entries N..ld_bar-1 stay as they were)
  auto decl = [&](Stage& s) {
    a.geo = s.in(geo, 8 * plane); a.dPdrho = s.in(dPdrho, n_lines); a.centre = s.in(centre, n_lines); a.sigma = s.in(sigma, n_lines);
    a.ps = s.in(ps, (size_t)n_lines * (size_t)ps_ld); a.line_of = s.in(line_of, n); a.var = s.in(var, 3 * n);
    a.lam = s.out(lam, n); a.gam = s.out(gam, n); a.dlam = s.out(dlam, 4 * n);
    a.geo_bar = s.out_rows(geo_bar, 8 * n, N, ld_bar); a.ld_bar = (long)s.rows_ld(N, ld_bar); a.plane_bar = n * (size_t)a.ld_bar;
    a.info = s.status(info, n);
  };
  return staged(ctx, flags, decl, [&]() -> int {
    const size_t per_wave = ibs::local_eq_grad_ws(N).total;
    const long wave_cap = (long)(ibs::kLineChunkBudget / (per_wave * sizeof(double)));      // (>= 292: a wave's workspace is at most 3.7 MB)
    long nw = 0;
    double* work = nullptr;
    auto carve = [&](Carve& cv, long P) {                  // ctx->long_ws of a chunk of P points
      nw = long_waves(ctx, P);
      if (nw > wave_cap) nw = wave_cap;
      work = cv.take<double>((size_t)nw * per_wave);
    };
    return for_line_chunks(ctx, "local_eq_grad", n_pts, 1, N, carve, [&](long p0, long Pc) -> int {
      ibs::LocalEqGradArgs c = a;
      c.n_pts = Pc;
      c.line_of = a.line_of + p0; c.var = a.var + 3 * p0;
      c.lam = a.lam ? a.lam + p0 : nullptr; c.gam = a.gam ? a.gam + p0 : nullptr; c.dlam = a.dlam ? a.dlam + 4 * p0 : nullptr;
      c.geo_bar = a.geo_bar ? a.geo_bar + p0 * a.ld_bar : nullptr;
      c.info = a.info ? a.info + p0 : nullptr;
      c.work = work; c.work_doubles = (size_t)nw * per_wave; c.n_waves = nw;
      HIPCHK(ibs::launch_local_eq_grad(c, ctx->stream));
      return 0;
    });
  });
}

// Scans that solve the assembled rows: the (g, c, f) rows of a chunk of whole lines are written out by k_assemble_gcf_long (the
// arithmetic of the scan kernels' staging: ball_scan.py:267-268 + utils.py:1560-1562) and handed to solve(first system, systems, G, C, F,
// work, work_doubles, waves) -- a one-wave-per-system kernel with ws_per_wave doubles of workspace per wave.  The chunks (rows + the
// solver's per-wave workspace) are those of for_line_chunks.
using ScanChunkSolve = std::function<int(long, long, double*, double*, double*, double*, size_t, long)>;
static int scan_rows_chunked(ibs_ctx* ctx, const char* what, int32_t n_lines, int32_t n_theta0, int32_t N, double h, const GeoLines& geo,
                             size_t ws_per_wave, const ScanChunkSolve& solve) {
  int nw = 0;
  double *work, *G, *C, *F;
  auto carve = [&](Carve& cv, long L) {          // ctx->long_ws of a chunk of L lines
    const long S = L * n_theta0;
    nw = long_waves(ctx, S);
    work = cv.take<double>((size_t)nw * ws_per_wave);
    G = cv.take<double>((size_t)S * N); C = cv.take<double>((size_t)S * N); F = cv.take<double>((size_t)S * N);
  };
  return for_line_chunks(ctx, what, n_lines, n_theta0, N, carve, [&](long l0, long Lc) -> int {
    ibs::ScanArgs<double> sa{};
    sa.n_lines = (int)Lc; sa.n_theta0 = n_theta0; sa.N = N; sa.h = h; sa.ld = geo.ld; sa.t0_stride = 0;
    geo.at(l0).into_named(sa);
    HIPCHK(ibs::launch_assemble_long(sa, G, C, F, nullptr, nullptr, nullptr, ctx->stream));
    return solve(l0 * n_theta0, Lc * n_theta0, G, C, F, work, (size_t)nw * ws_per_wave, (long)nw);
  });
}

// coarse scan with the nearest eigenpair: the chunks of scan_rows_chunked solved by k_solve_gcf_nearest
int ibs_gamma_scan_nearest_f64(ibs_ctx* ctx, int32_t n_lines, int32_t n_theta0, int32_t N, double h,
                               const double* bmag, const double* gradpar, const double* cvdrift, const double* cvdrift0,
                               const double* gds2, const double* gds21, const double* gds22, int64_t ld,
                               const double* dPdrho, const double* theta0, const double* sigma, double* gam, double* lam,
                               int32_t* idx, int32_t* info, int32_t mem) {
  const GeoLines geo{{bmag, gradpar, cvdrift, cvdrift0, gds2, gds21, gds22}, ld, dPdrho, theta0};
  if (!ctx) return fail(IBS_ERR_ARG, "null context");
  if (n_lines < 0 || n_theta0 < 0 || !geo.present() || !dPdrho || !theta0 || !sigma || ld < N)
    return fail(IBS_ERR_ARG, "bad arguments (n_lines=%d n_theta0=%d ld=%lld N=%d)", n_lines, n_theta0, (long long)ld, N);
  if (int r = check_grid(N, h, true)) return r;
  if (n_lines == 0 || n_theta0 == 0) return 0;
  ON_DEVICE(ctx);
  const size_t n_sys = (size_t)n_lines * n_theta0;
  GeoLines dgeo;
  const double* dsig;
  double *dgam, *dlam;
  int *didx, *dinfo;
  auto decl = [&](Stage& s) {
    dgeo = geo.declare(s, n_lines, n_theta0); dsig = s.in(sigma, n_sys);
    dgam = s.out(gam, n_sys); dlam = s.out(lam, n_sys); didx = s.out(idx, n_sys); dinfo = s.status(info, n_sys);
  };
  return staged(ctx, mem, decl, [&] {
    return scan_rows_chunked(ctx, "gamma_scan_nearest", n_lines, n_theta0, N, h, dgeo, ibs::nearest_ws_doubles(N),
                             [&](long s0, long S, double* G, double* C, double* F, double* work, size_t work_doubles, long nw) -> int {
      ibs::NearestArgs a{};
      a.n_sys = S; a.N = N; a.h = h; a.g = G; a.c = C; a.f = F; a.gh = nullptr; a.ld = N; a.sigma = dsig + s0;
      a.lam = dlam ? dlam + s0 : nullptr; a.idx = didx ? didx + s0 : nullptr; a.gam = dgam ? dgam + s0 : nullptr;
      a.info = dinfo ? dinfo + s0 : nullptr;
      a.work = work; a.work_doubles = work_doubles; a.n_waves = nw;
      HIPCHK(ibs::launch_gcf_nearest(a, ctx->stream));
      return 0;
    });
  });
}

// the n_modes largest eigenvalues and growth rates of every (line, theta0): the chunks of scan_rows_chunked solved by k_solve_gcf_modes
int ibs_gamma_scan_modes_f64(ibs_ctx* ctx, int32_t n_lines, int32_t n_theta0, int32_t N, double h,
                             const double* bmag, const double* gradpar, const double* cvdrift, const double* cvdrift0,
                             const double* gds2, const double* gds21, const double* gds22, int64_t ld,
                             const double* dPdrho, const double* theta0, int32_t n_modes, double* gam, double* lam,
                             int32_t* info, int32_t mem) {
  const GeoLines geo{{bmag, gradpar, cvdrift, cvdrift0, gds2, gds21, gds22}, ld, dPdrho, theta0};
  if (!ctx) return fail(IBS_ERR_ARG, "null context");
  if (n_lines < 0 || n_theta0 < 0 || !geo.present() || !dPdrho || !theta0 || ld < N)
    return fail(IBS_ERR_ARG, "bad arguments (n_lines=%d n_theta0=%d ld=%lld N=%d)", n_lines, n_theta0, (long long)ld, N);
  if (int r = check_n_modes(n_modes)) return r;
  if (!gam && !lam && !info) return fail(IBS_ERR_ARG, "no output requested (gam, lam and info are all null)");
  if (int r = check_grid(N, h, true)) return r;
  if (n_lines == 0 || n_theta0 == 0) return 0;
  ON_DEVICE(ctx);
  const size_t n_out = (size_t)n_lines * n_theta0 * n_modes;
  GeoLines dgeo;
  double *dgam, *dlam;
  int* dinfo;
  auto decl = [&](Stage& s) {
    dgeo = geo.declare(s, n_lines, n_theta0);
    dgam = s.out(gam, n_out); dlam = s.out(lam, n_out); dinfo = s.status(info, n_out);
  };
  return staged(ctx, mem, decl, [&] {
    return scan_rows_chunked(ctx, "gamma_scan_modes", n_lines, n_theta0, N, h, dgeo, ibs::modes_ws_doubles(N),
                             [&](long s0, long S, double* G, double* C, double* F, double* work, size_t work_doubles, long nw) -> int {
      const long o = s0 * n_modes;
      ibs::ModesArgs a{};
      a.n_sys = S; a.N = N; a.h = h; a.g = G; a.c = C; a.f = F; a.gh = nullptr; a.ld = N; a.n_modes = n_modes;
      a.lam = dlam ? dlam + o : nullptr; a.gam = dgam ? dgam + o : nullptr; a.info = dinfo ? dinfo + o : nullptr;
      a.work = work; a.work_doubles = work_doubles; a.n_waves = nw;
      HIPCHK(ibs::launch_gcf_modes(a, ctx->stream));
      return 0;
    });
  });
}

// ---- vector-Jacobian product of a whole (line, theta0) table of growth rates (ibs_scan_vjp.hip; nothing upstream corresponds): whole
// lines chunk after chunk (for_line_chunks); a chunk's
// workspace in ctx->long_ws = the persistent grid's per-wave workspace (ibs::exact_points_ws), three cotangent rows and a verdict per system
int ibs_gamma_scan_vjp_f64(ibs_ctx* ctx, int32_t n_lines, int32_t n_theta0, int32_t N, double h,
                           const double* bmag, const double* gradpar, const double* cvdrift, const double* cvdrift0,
                           const double* gds2, const double* gds21, const double* gds22, int64_t ld,
                           const double* dPdrho, const double* theta0, const double* sigma, const double* gam_bar,
                           double* geo_bar, double* dPdrho_bar, double* theta0_bar, double* gam, double* lam, int32_t* info,
                           int32_t mem) {
  const GeoLines geo{{bmag, gradpar, cvdrift, cvdrift0, gds2, gds21, gds22}, ld, dPdrho, theta0};
  if (!ctx) return fail(IBS_ERR_ARG, "null context");
  if (!geo.present() || !dPdrho || !theta0 || !gam_bar)
    return fail(IBS_ERR_ARG, "null argument (the geometry arrays, dPdrho, theta0 and gam_bar are required)");
  if (!geo_bar && !dPdrho_bar && !theta0_bar) return fail(IBS_ERR_ARG, "geo_bar, dPdrho_bar and theta0_bar are all null");
  if (n_lines < 0 || n_theta0 < 0 || ld < N)
    return fail(IBS_ERR_ARG, "bad arguments (n_lines=%d n_theta0=%d ld=%lld N=%d)", n_lines, n_theta0, (long long)ld, N);
  if (int r = check_grid(N, h, true)) return r;
  if (n_lines == 0 || n_theta0 == 0) return 0;
  ON_DEVICE(ctx);
  const size_t n_sys = (size_t)n_lines * n_theta0, plane = (size_t)n_lines * ld;
  const bool need_rows = geo_bar || dPdrho_bar;
  ibs::ScanVjpArgs a{};                                    // the whole call; each chunk launches a copy with its lines
  a.n_theta0 = n_theta0; a.N = N; a.h = h; a.ld = (long)ld; a.ld_bar = (long)ld;
  GeoLines dgeo;
  double* d_geo_bar = nullptr;
  auto decl = [&](Stage& s) {
    dgeo = geo.declare(s, n_lines, n_theta0); a.sigma = s.in(sigma, n_sys); a.gam_bar = s.in(gam_bar, n_sys);
    d_geo_bar = s.out(geo_bar, 7 * plane); a.dPdrho_bar = s.out(dPdrho_bar, n_lines); a.theta0_bar = s.out(theta0_bar, n_sys);
    a.gam = s.out(gam, n_sys); a.lam = s.out(lam, n_sys);
    a.info = s.status(info, n_sys);
  };
  return staged(ctx, mem, decl, [&]() -> int {
    if (mem == IBS_MEM_HOST && d_geo_bar && ld > N)      // (host pointers: the padding columns come back as zero)
      HIPCHK(hipMemsetAsync(d_geo_bar, 0, 7 * plane * sizeof(double), ctx->stream));
    const size_t per_wave = ibs::exact_points_ws(N).total;
    int nw = 0;
    double *work = nullptr, *rows = nullptr;
    int* flag = nullptr;
    auto carve = [&](Carve& cv, long L) {                  // ctx->long_ws of a chunk of L lines
      const long S = L * n_theta0;
      nw = long_waves(ctx, S);
      work = cv.take<double>((size_t)nw * per_wave);
      rows = need_rows ? cv.take<double>((size_t)S * 3 * N) : nullptr;
      flag = cv.take<int>((size_t)S);
    };
    return for_line_chunks(ctx, "gamma_scan_vjp", n_lines, n_theta0, N, carve, [&](long l0, long Lc) -> int {
      const long s0 = l0 * n_theta0;
      ibs::ScanVjpArgs c = a;
      c.n_lines = (int)Lc;
      dgeo.at(l0).into(c);
      for (int k = 0; k < 7; ++k) c.geo_bar[k] = d_geo_bar ? d_geo_bar + k * plane + l0 * ld : nullptr;
      c.gam_bar = a.gam_bar + s0;
      c.sigma = a.sigma ? a.sigma + s0 : nullptr;
      c.dPdrho_bar = a.dPdrho_bar ? a.dPdrho_bar + l0 : nullptr; c.theta0_bar = a.theta0_bar ? a.theta0_bar + s0 : nullptr;
      c.gam = a.gam ? a.gam + s0 : nullptr; c.lam = a.lam ? a.lam + s0 : nullptr; c.info = a.info ? a.info + s0 : nullptr;
      c.rows = rows; c.flag = flag;
      c.work = work; c.work_doubles = (size_t)nw * per_wave; c.n_waves = nw;
      HIPCHK(ibs::launch_scan_vjp(c, ctx->stream));
      return 0;
    });
  });
}

// ---- geometry-fed points with the eigenpair nearest sigma[p] (ibs_nearest_grad.hip): the refinement's objective + gradient and
// the final solve of ball_scan.py:305-339 in upstream's mode, one wave per point on the persistent grid of long_waves()
// the per-wave workspace (ibs::nearest_points_ws) in ctx->long_ws
int ibs_obj_w_grad_nearest_f64(ibs_ctx* ctx, int32_t n_pts, int32_t N, double h, const double* geo, int64_t ld,
                               const double* theta0, const double* sigma, double del_alpha, double* val, double* jac,
                               double* lam, int32_t* idx, int32_t* info, int32_t mem) {
  if (!ctx) return fail(IBS_ERR_ARG, "null context");
  if (n_pts < 0 || !geo || !theta0 || !sigma || !val || !jac || ld < N || !(del_alpha > 0))
    return fail(IBS_ERR_ARG, "bad arguments (n_pts=%d ld=%lld N=%d del_alpha=%g)", n_pts, (long long)ld, N, del_alpha);
  if (int r = check_grid(N, h, true)) return r;
  if (n_pts == 0) return 0;
  ON_DEVICE(ctx);
  const size_t n = (size_t)n_pts, geo_elems = n * 3 * 8 * (size_t)ld;
  ibs::NearestPointsArgs a{};
  a.n_pts = n_pts; a.N = N; a.h = h; a.ld = (long)ld; a.del_alpha = del_alpha;
  auto decl = [&](Stage& s) {
    a.geo = s.in(geo, geo_elems); a.theta0 = s.in(theta0, n); a.sigma = s.in(sigma, n);
    a.val = s.out(val, n); a.jac = s.out(jac, 2 * n); a.lam = s.out(lam, n); a.idx = s.out(idx, n); a.info = s.status(info, n);
  };
  return staged(ctx, mem, decl, [&]() -> int {
    if (int r = with_wave_ws(ctx, a, a.n_pts, ibs::nearest_points_ws(N, true).total)) return r;
    HIPCHK(ibs::launch_obj_w_grad_nearest(a, ctx->stream));
    return 0;
  });
}

int ibs_gamma_points_nearest_f64(ibs_ctx* ctx, int32_t n_pts, int32_t N, double h, const double* bmag, const double* gradpar,
                                 const double* cvdrift, const double* cvdrift0, const double* gds2, const double* gds21,
                                 const double* gds22, int64_t ld, const double* dPdrho, const double* theta0, const double* sigma,
                                 double* gam, double* lam, int32_t* idx, double* X, double* dX, int32_t* info, int32_t mem) {
  const GeoLines geo{{bmag, gradpar, cvdrift, cvdrift0, gds2, gds21, gds22}, ld, dPdrho, theta0, true};
  if (!ctx) return fail(IBS_ERR_ARG, "null context");
  if (n_pts < 0 || !geo.present() || !dPdrho || !theta0 || !sigma || !gam || ld < N)
    return fail(IBS_ERR_ARG, "bad arguments (n_pts=%d ld=%lld N=%d)", n_pts, (long long)ld, N);
  if (int r = check_grid(N, h, true)) return r;
  if (n_pts == 0) return 0;
  ON_DEVICE(ctx);
  const size_t n = (size_t)n_pts, out_elems = n * (size_t)N;
  ibs::NearestPointsArgs a{};
  a.n_pts = n_pts; a.N = N; a.h = h; a.ld = (long)ld;
  auto decl = [&](Stage& s) {
    geo.declare(s, n, 1).into(a); a.sigma = s.in(sigma, n);
    a.gam = s.out(gam, n); a.lam = s.out(lam, n); a.idx = s.out(idx, n); a.X = s.out(X, out_elems); a.dX = s.out(dX, out_elems);
    a.info = s.status(info, n);
  };
  return staged(ctx, mem, decl, [&]() -> int {
    if (int r = with_wave_ws(ctx, a, a.n_pts, ibs::nearest_points_ws(N, false).total)) return r;
    HIPCHK(ibs::launch_points_nearest(a, ctx->stream));
    return 0;
  });
}

// ---- geometry-fed points with the exact gradient of gam (ibs_exact_grad.hip): utils.py:1632-1728 with the derivative of the gam
// returned in place of the Hellmann-Feynman formulas, one wave per point on the persistent grid of long_waves()
// the per-wave workspace (ibs::exact_points_ws) in ctx->long_ws
int ibs_obj_w_grad_exact_f64(ibs_ctx* ctx, int32_t n_pts, int32_t N, double h, const double* geo, int64_t ld,
                             const double* theta0, const double* sigma, double del_alpha, double* val, double* jac,
                             double* gam, double* lam, int32_t* idx, int32_t* info, int32_t mem) {
  if (!ctx) return fail(IBS_ERR_ARG, "null context");
  if (n_pts < 0 || !geo || !theta0 || !val || !jac || ld < N || !(del_alpha > 0))
    return fail(IBS_ERR_ARG, "bad arguments (n_pts=%d ld=%lld N=%d del_alpha=%g)", n_pts, (long long)ld, N, del_alpha);
  if (int r = check_grid(N, h, true)) return r;
  if (n_pts == 0) return 0;
  ON_DEVICE(ctx);
  const size_t n = (size_t)n_pts, geo_elems = n * 3 * 8 * (size_t)ld;
  ibs::ExactPointsArgs a{};
  a.n_pts = n_pts; a.N = N; a.h = h; a.ld = (long)ld; a.del_alpha = del_alpha;
  auto decl = [&](Stage& s) {
    a.geo = s.in(geo, geo_elems); a.theta0 = s.in(theta0, n); a.sigma = s.in(sigma, n);
    a.val = s.out(val, n); a.jac = s.out(jac, 2 * n); a.gam = s.out(gam, n); a.lam = s.out(lam, n); a.idx = s.out(idx, n);
    a.info = s.status(info, n);
  };
  return staged(ctx, mem, decl, [&]() -> int {
    if (int r = with_wave_ws(ctx, a, a.n_pts, ibs::exact_points_ws(N).total)) return r;
    HIPCHK(ibs::launch_obj_w_grad_exact(a, ctx->stream));
    return 0;
  });
}

// ---- the same from ONE line per point and the alpha-tangent of its geometry (ibs_exact_tangent.hip): exact in alpha as well; the
// per-wave workspace is the same (ibs::exact_points_ws)
int ibs_obj_w_grad_exact_tangent_f64(ibs_ctx* ctx, int32_t n_pts, int32_t N, double h, const double* geo, const double* geo_da,
                                     int64_t ld, const double* theta0, const double* sigma, double* val, double* jac,
                                     double* gam, double* lam, int32_t* idx, int32_t* info, int32_t mem) {
  if (!ctx) return fail(IBS_ERR_ARG, "null context");
  if (n_pts < 0 || !geo || !geo_da || !theta0 || !val || !jac || ld < N)
    return fail(IBS_ERR_ARG, "bad arguments (n_pts=%d ld=%lld N=%d)", n_pts, (long long)ld, N);
  if (int r = check_grid(N, h, true)) return r;
  if (n_pts == 0) return 0;
  ON_DEVICE(ctx);
  const size_t n = (size_t)n_pts, geo_elems = n * 8 * (size_t)ld;
  ibs::ExactPointsArgs a{};
  a.n_pts = n_pts; a.N = N; a.h = h; a.ld = (long)ld;
  auto decl = [&](Stage& s) {
    a.geo = s.in(geo, geo_elems); a.geo_da = s.in(geo_da, geo_elems); a.theta0 = s.in(theta0, n); a.sigma = s.in(sigma, n);
    a.val = s.out(val, n); a.jac = s.out(jac, 2 * n); a.gam = s.out(gam, n); a.lam = s.out(lam, n); a.idx = s.out(idx, n);
    a.info = s.status(info, n);
  };
  return staged(ctx, mem, decl, [&]() -> int {
    if (int r = with_wave_ws(ctx, a, a.n_pts, ibs::exact_points_ws(N).total)) return r;
    HIPCHK(ibs::launch_obj_w_grad_exact_tangent(a, ctx->stream));
    return 0;
  });
}

// Geometry-fed scan on a grid beyond 2050 points: the (g, c, f) rows of every (line, theta0) system -- and their theta0 tangents when
// dgam/dtheta0 is wanted -- are written out (k_assemble_gcf_long: the arithmetic the scan kernels do while staging), solved by the
// generic long-grid kernel, and the Hellmann-Feynman sums (utils.py:1676-1680) taken by k_hf_grad.  Warm-start guesses are not
// used (they only ever steer).
static int launch_scan_long(ibs_ctx* ctx, const ibs::ScanArgs<double>& a) {
  const size_t n_sys = (size_t)a.n_lines * a.n_theta0, N = (size_t)a.N, rows = n_sys * N;
  const bool hf = a.dth0 != nullptr;
  const int nw = long_waves(ctx, (long)n_sys);
  double *work, *g, *c, *f, *gt = nullptr, *ct = nullptr, *ft = nullptr, *Xw = a.X, *dXw = a.dX, *gamw = a.gam;
  auto carve = [&](Carve& cv) {
    work = cv.take<double>((size_t)nw * 3 * N);
    g = cv.take<double>(rows); c = cv.take<double>(rows); f = cv.take<double>(rows);
    if (hf) {
      gt = cv.take<double>(rows); ct = cv.take<double>(rows); ft = cv.take<double>(rows);
      if (!a.X) Xw = cv.take<double>(rows);
      if (!a.dX) dXw = cv.take<double>(rows);
      if (!a.gam) gamw = cv.take<double>(n_sys);
    }
  };
  if (int r = carve_long(ctx, carve)) return r;
  HIPCHK(ibs::launch_assemble_long(a, g, c, f, gt, ct, ft, ctx->stream));
  ibs::LongGcfArgs la{};
  la.n_sys = (long)n_sys; la.N = a.N; la.h = a.h; la.g = g; la.c = c; la.f = f; la.gh = nullptr; la.f32 = 0; la.ld = (long)N;
  la.lam = a.lam; la.gam = gamw; la.X = Xw; la.dX = dXw; la.info = a.info; la.work = work; la.n_waves = nw;
  HIPCHK(ibs::launch_gcf_long(la, ctx->stream));
  if (hf) {
    hipLaunchKernelGGL(k_hf_grad, dim3((unsigned)((n_sys + 3) / 4)), dim3(256), 0, ctx->stream, (long)n_sys, a.N, (long)N, Xw, dXw, f, gt, ct,
                       ft, gamw, a.dth0);
    HIPCHK(hipGetLastError());
  }
  return 0;
}

// The trial table of the resident scan kernel for (N, M) on the context's current stream (ibs_ctx::trial_tables): the cached one, or
// a new one whose build is enqueued on that stream in front of the launch that reads it.  *out = null where there is none to give (the
// option is off, no builder for this M, or the stream is being captured: a captured build would run at replay, not now, and the
// entry would be taken for built) -- the kernel then computes the values itself, to the same bits.
static int trial_table_for(ibs_ctx* ctx, int N, int M, const double** out) {
  *out = nullptr;
  const ibs::LaunchTable& t = ibs::launch_table();
  if (!ctx->opt.scan_trial_table || M < 0 || M > ibs::kMaxM || !t.trial_table_f64[M]) return 0;
  ibs_ctx::TrialTable* slot = nullptr;
  for (auto& e : ctx->trial_tables) {
    if (e.buf && e.N == N && e.M == M && e.stream == ctx->stream) { e.used = ++ctx->trial_clock; *out = e.buf; return 0; }
    if (!slot || (slot->buf && (!e.buf || e.used < slot->used))) slot = &e;      // a free entry, else the one used longest ago
  }
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(ctx->stream, &cap) != hipSuccess) { (void)hipGetLastError(); return 0; }
  if (cap != hipStreamCaptureStatusNone) return 0;
  if (slot->buf) {
    HIPCHK(hipDeviceSynchronize());
    slot->N = 0;                                   // (not (N, M)'s until its build is enqueued: a failure below leaves no false entry)
  } else {
    HIPCHK(hipMalloc(reinterpret_cast<void**>(&slot->buf), (size_t)ibs::kTrialTableLen * sizeof(double)));
  }
  HIPCHK(t.trial_table_f64[M](N, slot->buf, ctx->stream));
  slot->N = N; slot->M = M; slot->stream = ctx->stream; slot->used = ++ctx->trial_clock;
  *out = slot->buf;
  return 0;
}

static int gamma_scan_impl(ibs_ctx* ctx, int32_t n_lines, int32_t n_theta0, int32_t N, double h, const GeoLines& geo, double* gam,
                           double* lam, double* X, double* dX, double* dth0, int32_t* info, int32_t mem, const double* lam_guess,
                           double guess_width, int32_t n_surf = 0, double* pack = nullptr) {
  // geo.per_line: n_theta0 = 1 and theta0[n_lines] holds one value per line (ibs_gamma_points_f64); one wave per system
  const bool t0_per_line = geo.per_line;
  const int64_t ld = geo.ld;
  if (!ctx) return fail(IBS_ERR_ARG, "null context");
  if (lam_guess && !(guess_width > 0)) return fail(IBS_ERR_ARG, "guess_width must be > 0");
  if (pack && (mem != IBS_MEM_DEVICE || n_surf <= 0 || n_lines % n_surf != 0 || !gam))
    return fail(IBS_ERR_ARG, "fused argmax: device pointers, gam output and n_lines %% n_surf == 0 required (n_lines=%d n_surf=%d)", n_lines, n_surf);
  if (n_lines < 0 || n_theta0 < 0 || !geo.present() || !geo.dPdrho || !geo.theta0 || ld < N)
    return fail(IBS_ERR_ARG, "bad arguments (n_lines=%d n_theta0=%d ld=%lld N=%d)", n_lines, n_theta0, (long long)ld, N);
  if (int r = check_grid(N, h, true)) return r;
  if (n_lines == 0 || n_theta0 == 0) return 0;
  const ibs::ScanPlan plan = ibs::plan_scan(ctx->chip, ctx->opt, ctx->built, n_lines, n_theta0, N, lam_guess != nullptr, X || dX, t0_per_line, pack != nullptr);
  if (plan.err == ibs::PlanError::NotBuilt) return fail(IBS_ERR_UNSUPPORTED, "no kernel built for rows-per-lane M=%d (N=%d)", plan.M, N);
  ON_DEVICE(ctx);
  if (plan.err == ibs::PlanError::NoLds) return fail(IBS_ERR_UNSUPPORTED, "N=%d does not fit the LDS staging", N);
  const ibs::LaunchTable& t = ibs::launch_table();
  const int pi = plan.P == 32 ? 0 : 1;
  hipError_t (*fn)(const ibs::ScanArgs<double>&, hipStream_t) = nullptr;
  switch (plan.form) {
    case ibs::ScanForm::Wave: case ibs::ScanForm::WaveLean: fn = t.scan_f64[plan.M]; break;
    case ibs::ScanForm::WaveChain: fn = t.scan_chain_f64[plan.M]; break;
    case ibs::ScanForm::Group: fn = t.scan_f64_g[pi][plan.M]; break;
    case ibs::ScanForm::GroupChain: fn = t.scan_chain_f64_g[pi][plan.M]; break;
    case ibs::ScanForm::Long: break;                   // (launch_scan_long)
  }
  ibs::ScanArgs<double> a{};
  a.n_lines = n_lines; a.n_theta0 = n_theta0; a.N = N; a.h = h; a.ld = ld;
  a.t0_stride = t0_per_line ? 1 : 0;
  a.wpb = plan.wpb; a.resident = plan.resident; a.chain = plan.chain;
  // (widths of the chain's warm starts: defaults 0.25 / 1.0 measured on the NCSX shapes (tools/bench_chain.py): 9.2 sweeps per solve instead of 15.7)
  if (plan.chain) { a.chain_w1 = ctx->opt.chain_w1; a.chain_w2 = ctx->opt.chain_w2; }
  // (the divisions of the kernel's set-up and growth-rate stage, done once here: correctly rounded on both sides)
  a.ih2 = 1.0 / (h * h); a.ih = 1.0 / h;
  const size_t n_sys = (size_t)n_lines * n_theta0, out_elems = n_sys * N;
  a.guess_width = guess_width;
  // (host pointers: gam, lam and info are always carved)
  auto decl = [&](Stage& s) {
    geo.declare(s, n_lines, n_theta0).into_named(a); a.lam_guess = s.in(lam_guess, n_sys);
    a.gam = s.out(gam, n_sys, true); a.lam = s.out(lam, n_sys, true); a.X = s.out(X, out_elems); a.dX = s.out(dX, out_elems);
    a.dth0 = s.out(dth0, n_sys); a.info = s.status(info, n_sys);
  };
  return staged(ctx, mem, decl, [&]() -> int {
    if (plan.fused_pack) {
      // one launch: the block that completes a surface reduces it (k_gamma_scan's epilogue)
      ibs_ctx::SurfCounters* sc = nullptr;
      for (auto& e : ctx->surf_counters) if (e.stream == ctx->stream) { sc = &e; break; }
      if (!sc) { ctx->surf_counters.push_back(ibs_ctx::SurfCounters{ctx->stream, nullptr, 0}); sc = &ctx->surf_counters.back(); }
      if (sc->n < n_surf) {
        if (sc->buf) { HIPCHK(hipStreamSynchronize(ctx->stream)); HIPCHK(hipFree(sc->buf)); sc->buf = nullptr; sc->n = 0; }
        const int cap_n = n_surf > 1024 ? n_surf : 1024;
        HIPCHK(hipMalloc(reinterpret_cast<void**>(&sc->buf), (size_t)cap_n * sizeof(int)));
        HIPCHK(hipMemsetAsync(sc->buf, 0, (size_t)cap_n * sizeof(int), ctx->stream));
        sc->n = cap_n;
      }
      a.lines_per_surf = n_lines / n_surf; a.surf_counter = sc->buf; a.pack = pack; a.pack_mode = plan.pack_mode;
    }
    if (plan.form == ibs::ScanForm::Wave && plan.resident) {
      if (int r = trial_table_for(ctx, N, plan.M, &a.trial_tab)) return r;
    }
    if (!fn) {
      if (int r = launch_scan_long(ctx, a)) return r;
    } else {
      HIPCHK(fn(a, ctx->stream));
    }
    flag_sigma<double>(ctx, (long)n_sys, a.lam, a.info);
    if (pack && !plan.fused_pack) {                          // chained / sub-wave / long-grid scans: the reduction is a second launch
      const int n_per = (n_lines / n_surf) * n_theta0;
      hipLaunchKernelGGL(k_surface_argmax, dim3(n_surf), dim3(argmax_threads(n_per)), 0, ctx->stream, n_per, gam, (int*)nullptr, (double*)nullptr, pack);
      HIPCHK(hipGetLastError());
    }
    return 0;
  });
}

int ibs_gamma_scan_f64(ibs_ctx* ctx, int32_t n_lines, int32_t n_theta0, int32_t N, double h,
                       const double* bmag, const double* gradpar, const double* cvdrift, const double* cvdrift0,
                       const double* gds2, const double* gds21, const double* gds22, int64_t ld,
                       const double* dPdrho, const double* theta0, double* gam, double* lam, double* X,
                       double* dX, double* dth0, int32_t* info, int32_t mem) {
  const GeoLines geo{{bmag, gradpar, cvdrift, cvdrift0, gds2, gds21, gds22}, ld, dPdrho, theta0};
  return gamma_scan_impl(ctx, n_lines, n_theta0, N, h, geo, gam, lam, X, dX, dth0, info, mem, nullptr, 0.0);
}

int ibs_gamma_scan_warm_f64(ibs_ctx* ctx, int32_t n_lines, int32_t n_theta0, int32_t N, double h,
                            const double* bmag, const double* gradpar, const double* cvdrift, const double* cvdrift0,
                            const double* gds2, const double* gds21, const double* gds22, int64_t ld,
                            const double* dPdrho, const double* theta0, const double* lam_guess, double guess_width,
                            double* gam, double* lam, double* X, double* dX, double* dth0, int32_t* info, int32_t mem) {
  if (!lam_guess) return fail(IBS_ERR_ARG, "lam_guess is null");
  const GeoLines geo{{bmag, gradpar, cvdrift, cvdrift0, gds2, gds21, gds22}, ld, dPdrho, theta0};
  return gamma_scan_impl(ctx, n_lines, n_theta0, N, h, geo, gam, lam, X, dX, dth0, info, mem, lam_guess, guess_width);
}

int ibs_gamma_scan_argmax_f64(ibs_ctx* ctx, int32_t n_lines, int32_t n_theta0, int32_t N, double h,
                              const double* bmag, const double* gradpar, const double* cvdrift, const double* cvdrift0,
                              const double* gds2, const double* gds21, const double* gds22, int64_t ld,
                              const double* dPdrho, const double* theta0, int32_t n_surf, double* gam, double* lam,
                              double* pack, int32_t* info) {
  if (!pack) return fail(IBS_ERR_ARG, "pack is null");
  const GeoLines geo{{bmag, gradpar, cvdrift, cvdrift0, gds2, gds21, gds22}, ld, dPdrho, theta0};
  return gamma_scan_impl(ctx, n_lines, n_theta0, N, h, geo, gam, lam, nullptr, nullptr, nullptr, info, IBS_MEM_DEVICE, nullptr, 0.0, n_surf, pack);
}

int ibs_gamma_points_f64(ibs_ctx* ctx, int32_t n_pts, int32_t N, double h, const double* bmag, const double* gradpar,
                         const double* cvdrift, const double* cvdrift0, const double* gds2, const double* gds21,
                         const double* gds22, int64_t ld, const double* dPdrho, const double* theta0, double* gam,
                         double* lam, double* X, double* dX, double* dgam_dtheta0, int32_t* info, int32_t mem) {
  const GeoLines geo{{bmag, gradpar, cvdrift, cvdrift0, gds2, gds21, gds22}, ld, dPdrho, theta0, true};
  return gamma_scan_impl(ctx, n_pts, 1, N, h, geo, gam, lam, X, dX, dgam_dtheta0, info, mem, nullptr, 0.0);
}

// ---- lines on a non-uniform theta grid (ibs_regrid.hip; utils.py:1565-1576): regrid onto the uniform grid of the window, then the raw
// solvers with the half-grid row gh.  The checks of the theta arguments every such entry point shares; *h = the spacing of the solve
static int check_theta_args(int32_t N, const double* theta, int64_t theta_ld, double lo, double hi, double* h) {
  if (!theta) return fail(IBS_ERR_ARG, "theta is null");
  if (theta_ld != 0 && theta_ld < N) return fail(IBS_ERR_ARG, "theta_ld=%lld is neither 0 (one shared grid) nor >= N=%d", (long long)theta_ld, N);
  if (!ibs::regrid_window_ok(lo, hi)) return fail(IBS_ERR_ARG, "theta window [%g, %g]: theta_lo and theta_hi must be finite with theta_hi > theta_lo", lo, hi);
  const ibs::GridCheck gc = ibs::check_grid_length(N, true);
  *h = gc == ibs::GridCheck::Range ? 1.0 : ibs::regrid_spacing(N, lo, hi);
  return check_grid(N, *h, true);
}

int ibs_regrid_rows_f64(ibs_ctx* ctx, int64_t n_sys, int32_t N, const double* theta, int64_t theta_ld, double theta_lo, double theta_hi,
                        const double* g, const double* c, const double* f, int64_t ld, double* g_u, double* gh, double* c_u,
                        double* f_u, int64_t ld_out, double* h_out, int32_t* info, int32_t mem) {
  if (!ctx) return fail(IBS_ERR_ARG, "null context");
  if (n_sys < 0 || !g || !g_u || !gh || ld < N || ld_out < N)
    return fail(IBS_ERR_ARG, "bad arguments (n_sys=%lld ld=%lld ld_out=%lld N=%d)", (long long)n_sys, (long long)ld, (long long)ld_out, N);
  if ((c != nullptr) != (c_u != nullptr) || (f != nullptr) != (f_u != nullptr))
    return fail(IBS_ERR_ARG, "c / c_u and f / f_u are optional as pairs");
  double h = 0.0;
  if (int r = check_theta_args(N, theta, theta_ld, theta_lo, theta_hi, &h)) return r;
  if (h_out) *h_out = h;
  if (n_sys == 0) return 0;
  ON_DEVICE(ctx);
  ibs::RegridArgs a{};
  a.n_lines = theta_ld ? n_sys : 1; a.per_line = theta_ld ? 1 : n_sys; a.N = N; a.theta_ld = theta_ld; a.lo = theta_lo; a.hi = theta_hi;
  a.ld = ld; a.n_cu = ctx->chip.n_cu;
  const size_t in_elems = (size_t)n_sys * ld;
  auto decl = [&](Stage& s) {
    a.theta = s.in(theta, theta_ld ? (size_t)n_sys * theta_ld : (size_t)N);
    a.g = s.in(g, in_elems); a.c = s.in(c, in_elems); a.f = s.in(f, in_elems);
    a.g_u = s.out_rows(g_u, n_sys, N, ld_out); a.gh = s.out_rows(gh, n_sys, N, ld_out);
    a.c_u = s.out_rows(c_u, n_sys, N, ld_out); a.f_u = s.out_rows(f_u, n_sys, N, ld_out);
    a.ld_out = (long)s.rows_ld(N, ld_out);
    a.info = s.status(info, n_sys);
  };
  return staged(ctx, mem, decl, [&]() -> int { HIPCHK(ibs::launch_regrid_rows(a, ctx->stream)); return 0; });
}

// the arguments the three geometry-fed theta entry points share, checked before the context is touched
static int check_theta_geo(ibs_ctx* ctx, int32_t n_lines, int32_t n_theta0, int32_t N, const double* theta, int64_t theta_ld, double lo,
                           double hi, const GeoLines& geo, double* h) {
  if (!ctx) return fail(IBS_ERR_ARG, "null context");
  if (n_lines < 0 || n_theta0 < 0 || !geo.present() || !geo.dPdrho || !geo.theta0 || geo.ld < N)
    return fail(IBS_ERR_ARG, "bad arguments (n_lines=%d n_theta0=%d ld=%lld N=%d)", n_lines, n_theta0, (long long)geo.ld, N);
  return check_theta_args(N, theta, theta_ld, lo, hi, h);
}

int ibs_assemble_gcf_theta_f64(ibs_ctx* ctx, int32_t n_lines, int32_t n_theta0, int32_t N, const double* theta, int64_t theta_ld,
                               double theta_lo, double theta_hi, const double* bmag, const double* gradpar, const double* cvdrift,
                               const double* cvdrift0, const double* gds2, const double* gds21, const double* gds22, int64_t ld,
                               const double* dPdrho, const double* theta0, int32_t theta0_per_line, double* g_u, double* gh,
                               double* c_u, double* f_u, double* h_out, int32_t* info, int32_t mem) {
  const GeoLines geo{{bmag, gradpar, cvdrift, cvdrift0, gds2, gds21, gds22}, ld, dPdrho, theta0, theta0_per_line != 0};
  double h = 0.0;
  if (int r = check_theta_geo(ctx, n_lines, n_theta0, N, theta, theta_ld, theta_lo, theta_hi, geo, &h)) return r;
  if (!g_u || !gh || !c_u || !f_u) return fail(IBS_ERR_ARG, "g_u, gh, c_u and f_u are required");
  if (theta0_per_line && n_theta0 != 1) return fail(IBS_ERR_ARG, "theta0_per_line needs n_theta0 = 1 (one theta0 per line), not %d", n_theta0);
  if (h_out) *h_out = h;
  if (n_lines == 0 || n_theta0 == 0) return 0;
  ON_DEVICE(ctx);
  ibs::RegridArgs a{};
  a.n_lines = n_lines; a.per_line = n_theta0; a.N = N; a.theta_ld = theta_ld; a.lo = theta_lo; a.hi = theta_hi; a.ld = ld;
  a.t0_per_line = theta0_per_line ? 1 : 0; a.ld_out = N; a.n_cu = ctx->chip.n_cu;
  const size_t n_sys = (size_t)n_lines * n_theta0, out_elems = n_sys * N;
  auto decl = [&](Stage& s) {
    a.theta = s.in(theta, theta_ld ? (size_t)n_lines * theta_ld : (size_t)N);
    geo.declare(s, n_lines, n_theta0).into(a);
    a.g_u = s.out(g_u, out_elems); a.gh = s.out(gh, out_elems); a.c_u = s.out(c_u, out_elems); a.f_u = s.out(f_u, out_elems);
    a.info = s.status(info, n_sys);
  };
  return staged(ctx, mem, decl, [&]() -> int { HIPCHK(ibs::launch_assemble_regrid(a, ctx->stream)); return 0; });
}

// Geometry-fed scan on a non-uniform grid, on the pattern of scan_rows_chunked / launch_scan_long: the four regridded rows of a chunk of
// whole lines (for_line_chunks) are written to ctx->long_ws by k_assemble_regrid and solved by the raw solver WITH gh, in the form
// plan_gcf picks for a caller-supplied half grid -- the long-grid kernel beyond 2050 points, its workspace carved out of the same allocation.  A line that is not a grid reaches the solver
// as NaN rows and comes back with status bit 1; k_regrid_poison then makes its floating-point outputs NaN.  Every system is a function of its own line: chunking changes no bit.
static int scan_theta_impl(ibs_ctx* ctx, int32_t n_lines, int32_t n_theta0, int32_t N, const double* theta, int64_t theta_ld, double lo,
                           double hi, const GeoLines& geo, double* gam, double* lam, double* X, double* dX, int32_t* info, int32_t mem) {
  double h = 0.0;
  if (int r = check_theta_geo(ctx, n_lines, n_theta0, N, theta, theta_ld, lo, hi, geo, &h)) return r;
  if (n_lines == 0 || n_theta0 == 0) return 0;
  const size_t n_sys = (size_t)n_lines * n_theta0, out_elems = n_sys * N;
  const ibs::GcfPlan plan = ibs::plan_gcf(ctx->chip, ctx->opt, ctx->built, 8, (long)n_sys, N, true, mem == IBS_MEM_HOST || gam, X || dX);
  if (plan.err == ibs::PlanError::NotBuilt) return fail(IBS_ERR_UNSUPPORTED, "no kernel built for rows-per-lane M=%d (N=%d)", plan.M, N);
  ON_DEVICE(ctx);
  if (plan.err == ibs::PlanError::NoLds) return fail(IBS_ERR_UNSUPPORTED, "N=%d needs %zu B of LDS per wave", N, plan.per_wave);
  const bool lng = plan.form == ibs::GcfForm::Long;
  const double* dth;
  GeoLines dgeo;
  double *dgam, *dlam, *dXo, *ddX;
  int* dinfo;
  auto decl = [&](Stage& s) {
    dth = s.in(theta, theta_ld ? (size_t)n_lines * theta_ld : (size_t)N);
    dgeo = geo.declare(s, n_lines, n_theta0);
    dgam = s.out(gam, n_sys, true); dlam = s.out(lam, n_sys, true); dXo = s.out(X, out_elems); ddX = s.out(dX, out_elems);
    dinfo = s.status(info, n_sys);
  };
  return staged(ctx, mem, decl, [&]() -> int {
    double *work = nullptr, *G, *GH, *C, *F;
    int* flag;                                     // the regrid's verdict on every system of the chunk
    auto carve = [&](Carve& cv, long L) {          // ctx->long_ws of a chunk of L lines
      const size_t S = (size_t)L * n_theta0;
      if (lng) work = cv.take<double>((size_t)long_waves(ctx, (long)S) * 3 * (size_t)N);
      G = cv.take<double>(S * N); GH = cv.take<double>(S * N); C = cv.take<double>(S * N); F = cv.take<double>(S * N);
      flag = cv.take<int>(S);
    };
    const int rc = for_line_chunks(ctx, geo.per_line ? "gamma_points_theta" : "gamma_scan_theta", n_lines, n_theta0, N, carve,
                                   [&](long l0, long Lc) -> int {
      const long s0 = l0 * n_theta0, S = Lc * n_theta0;
      ibs::RegridArgs ra{};
      ra.n_lines = Lc; ra.per_line = n_theta0; ra.N = N; ra.theta = dth + (theta_ld ? l0 * theta_ld : 0); ra.theta_ld = theta_ld;
      ra.lo = lo; ra.hi = hi; ra.ld = geo.ld; ra.t0_per_line = geo.per_line ? 1 : 0; ra.n_cu = ctx->chip.n_cu;
      dgeo.at(l0).into(ra);
      ra.g_u = G; ra.gh = GH; ra.c_u = C; ra.f_u = F; ra.ld_out = N; ra.info = flag;
      HIPCHK(ibs::launch_assemble_regrid(ra, ctx->stream));
      ibs::GcfArgs<double> ga{};
      ga.n_sys = S; ga.N = N; ga.h = h; ga.g = G; ga.gh = GH; ga.c = C; ga.f = F; ga.ld = N; ga.wpb = plan.wpb;
      ga.flags = ctx->opt.reclose == 1 ? 1 : (ctx->opt.reclose == 2 ? 2 : 0);
      ga.lam = dlam ? dlam + s0 : nullptr; ga.gam = dgam ? dgam + s0 : nullptr; ga.info = dinfo ? dinfo + s0 : nullptr;
      ga.X = dXo ? dXo + (size_t)s0 * N : nullptr; ga.dX = ddX ? ddX + (size_t)s0 * N : nullptr;
      if (int r = launch_planned_gcf<double>(ctx, plan, ga, work)) return r;
      HIPCHK(ibs::launch_regrid_poison(S, N, flag, ga.lam, ga.gam, ga.X, ga.dX, ctx->stream));
      return 0;
    });
    if (rc) return rc;
    flag_sigma<double>(ctx, (long)n_sys, dlam, dinfo);
    return 0;
  });
}

int ibs_gamma_scan_theta_f64(ibs_ctx* ctx, int32_t n_lines, int32_t n_theta0, int32_t N, const double* theta, int64_t theta_ld,
                             double theta_lo, double theta_hi, const double* bmag, const double* gradpar, const double* cvdrift,
                             const double* cvdrift0, const double* gds2, const double* gds21, const double* gds22, int64_t ld,
                             const double* dPdrho, const double* theta0, double* gam, double* lam, double* X, double* dX,
                             int32_t* info, int32_t mem) {
  const GeoLines geo{{bmag, gradpar, cvdrift, cvdrift0, gds2, gds21, gds22}, ld, dPdrho, theta0};
  return scan_theta_impl(ctx, n_lines, n_theta0, N, theta, theta_ld, theta_lo, theta_hi, geo, gam, lam, X, dX, info, mem);
}

int ibs_gamma_points_theta_f64(ibs_ctx* ctx, int32_t n_pts, int32_t N, const double* theta, int64_t theta_ld, double theta_lo,
                               double theta_hi, const double* bmag, const double* gradpar, const double* cvdrift, const double* cvdrift0,
                               const double* gds2, const double* gds21, const double* gds22, int64_t ld, const double* dPdrho,
                               const double* theta0, double* gam, double* lam, double* X, double* dX, int32_t* info, int32_t mem) {
  const GeoLines geo{{bmag, gradpar, cvdrift, cvdrift0, gds2, gds21, gds22}, ld, dPdrho, theta0, true};
  return scan_theta_impl(ctx, n_pts, 1, N, theta, theta_ld, theta_lo, theta_hi, geo, gam, lam, X, dX, info, mem);
}

int ibs_scan_starts_f64(ibs_ctx* ctx, int32_t n_surf, int32_t n_alpha, int32_t n_theta0, const double* alpha,
                        const double* theta0, const double* pack, double* start, double* sigma0, int32_t* n_bad) {
  if (!ctx) return fail(IBS_ERR_ARG, "null context");
  if (n_surf < 0 || n_alpha <= 0 || n_theta0 <= 0 || !alpha || !theta0 || !pack || !start || !n_bad) return fail(IBS_ERR_ARG, "bad arguments");
  if (n_surf == 0) return 0;
  ON_DEVICE(ctx);
  hipLaunchKernelGGL(k_scan_starts, dim3((unsigned)((n_surf + 127) / 128)), dim3(128), 0, ctx->stream, n_surf, n_alpha, n_theta0,
                     alpha, theta0, pack, start, sigma0, n_bad);
  HIPCHK(hipGetLastError());
  return 0;
}

// ---- objective + Hellmann-Feynman gradient on grids beyond 2050 points (utils.py:1632-1728 takes any length): composed from the
// long-grid pieces -- dPdrho of the 3 n lines (k_line_dPdrho), their (g, c, f) rows and theta0-tangents at the point's theta0
// (k_assemble_gcf_long), the centre lines' rows and the alpha-tangents (right - left) / del_alpha packed per point, ONE long-grid
// solve per point with eigenfunction (k_solve_gcf_long), two Hellmann-Feynman sums (k_hf_grad).
__global__ void k_grad_long_t0(int n_pts, const double* __restrict__ theta0, double* __restrict__ th3) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < 3 * n_pts) th3[i] = theta0[i / 3];
}
__global__ void __launch_bounds__(256) k_grad_long_pack(int n_pts, int N, double inv_del, const double* __restrict__ G, const double* __restrict__ C,
                                                        const double* __restrict__ F, const double* __restrict__ GT, const double* __restrict__ CT,
                                                        const double* __restrict__ FT, double* gC, double* cC, double* fC, double* gtC, double* ctC,
                                                        double* ftC, double* gaC, double* caC, double* faC) {
  const int p = blockIdx.y;
  const size_t l = (size_t)(3 * p) * N, m = l + N, r = m + N, o = (size_t)p * N;
  for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < N; j += gridDim.x * blockDim.x) {
    gC[o + j] = G[m + j]; cC[o + j] = C[m + j]; fC[o + j] = F[m + j];
    gtC[o + j] = GT[m + j]; ctC[o + j] = CT[m + j]; ftC[o + j] = FT[m + j];                 // utils.py:1669-1673
    gaC[o + j] = (G[r + j] - G[l + j]) * inv_del; caC[o + j] = (C[r + j] - C[l + j]) * inv_del;      // utils.py:1705-1719
    faC[o + j] = (F[r + j] - F[l + j]) * inv_del;
  }
}
__global__ void k_grad_long_out(int n_pts, const double* __restrict__ gam, const double* __restrict__ ja, const double* __restrict__ jt,
                                double* val, double* jac, double* gam_o, double* da_o, double* dt_o) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_pts) return;
  val[p] = -gam[p]; jac[2 * p] = -ja[p]; jac[2 * p + 1] = -jt[p];                            // utils.py:1728
  if (gam_o) gam_o[p] = gam[p];
  if (da_o) da_o[p] = ja[p];
  if (dt_o) dt_o[p] = jt[p];
}
static int launch_grad_long(ibs_ctx* ctx, const ibs::GradArgs<double>& a) {
  const size_t n = (size_t)a.n_pts, N = (size_t)a.N, rows = n * N;
  const int nw = long_waves(ctx, (long)n);
  double *work, *G, *C, *F, *GT, *CT, *FT, *gC, *cC, *fC, *gtC, *ctC, *ftC, *gaC, *caC, *faC, *Xw, *dXw, *dP3, *th3, *gamw, *lamw, *ja, *jt;
  auto carve = [&](Carve& cv) {
    work = cv.take<double>((size_t)nw * 3 * N);
    for (double** p : {&G, &C, &F, &GT, &CT, &FT}) *p = cv.take<double>(3 * rows);
    for (double** p : {&gC, &cC, &fC, &gtC, &ctC, &ftC, &gaC, &caC, &faC, &Xw, &dXw}) *p = cv.take<double>(rows);
    dP3 = cv.take<double>(3 * n); th3 = cv.take<double>(3 * n);
    for (double** p : {&gamw, &lamw, &ja, &jt}) *p = cv.take<double>(n);
  };
  if (int r = carve_long(ctx, carve)) return r;
  const hipStream_t st = ctx->stream;
  const long lds = a.ld;                                                  // geo: [n_pts][3][8][ld]
  HIPCHK(ibs::launch_line_dPdrho((int)(3 * n), a.N, 8 * lds, (size_t)lds, a.geo, dP3, st));
  hipLaunchKernelGGL(k_grad_long_t0, dim3((unsigned)((3 * n + 255) / 256)), dim3(256), 0, st, a.n_pts, a.theta0, th3);
  ibs::ScanArgs<double> sa{};
  sa.n_lines = (int)(3 * n); sa.n_theta0 = 1; sa.N = a.N; sa.h = a.h; sa.ld = 8 * lds;
  sa.bmag = a.geo; sa.gradpar = a.geo + lds; sa.cvdrift = a.geo + 2 * lds; sa.cvdrift0 = a.geo + 3 * lds;
  sa.gds2 = a.geo + 4 * lds; sa.gds21 = a.geo + 5 * lds; sa.gds22 = a.geo + 6 * lds;
  sa.dPdrho = dP3; sa.theta0 = th3; sa.t0_stride = 1;
  HIPCHK(ibs::launch_assemble_long(sa, G, C, F, GT, CT, FT, st));
  int bx = (a.N + 255) / 256;
  if (bx > 16) bx = 16;
  hipLaunchKernelGGL(k_grad_long_pack, dim3((unsigned)bx, (unsigned)n), dim3(256), 0, st, a.n_pts, a.N, 1.0 / a.del_alpha, G, C, F, GT, CT, FT,
                     gC, cC, fC, gtC, ctC, ftC, gaC, caC, faC);
  ibs::LongGcfArgs la{};
  la.n_sys = (long)n; la.N = a.N; la.h = a.h; la.g = gC; la.c = cC; la.f = fC; la.gh = nullptr; la.f32 = 0; la.ld = (long)N;
  la.lam = lamw; la.gam = gamw; la.X = Xw; la.dX = dXw; la.info = a.info; la.work = work; la.n_waves = nw;
  HIPCHK(ibs::launch_gcf_long(la, st));
  const unsigned hb = (unsigned)((n + 3) / 4);
  hipLaunchKernelGGL(k_hf_grad, dim3(hb), dim3(256), 0, st, (long)n, a.N, (long)N, Xw, dXw, fC, gtC, ctC, ftC, gamw, jt);
  hipLaunchKernelGGL(k_hf_grad, dim3(hb), dim3(256), 0, st, (long)n, a.N, (long)N, Xw, dXw, fC, gaC, caC, faC, gamw, ja);
  hipLaunchKernelGGL(k_grad_long_out, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a.n_pts, gamw, ja, jt, a.val, a.jac, a.gam, a.dalpha, a.dth0);
  HIPCHK(hipGetLastError());
  return 0;
}

int ibs_obj_w_grad_f64(ibs_ctx* ctx, int32_t n_pts, int32_t N, double h, const double* geo, int64_t ld,
                       const double* theta0, double del_alpha, double* val, double* jac, int32_t* info,
                       int32_t mem) {
  if (!ctx) return fail(IBS_ERR_ARG, "null context");
  if (n_pts < 0 || !geo || !theta0 || !val || !jac || ld < N || !(del_alpha > 0)) return fail(IBS_ERR_ARG, "bad arguments");
  if (int r = check_grid(N, h, true)) return r;
  if (n_pts == 0) return 0;
  const bool lng = is_long(N);                 // grids beyond 2050 points: launch_grad_long
  const int M = lng ? 1 : rows_per_lane(N);
  const auto fn = ibs::launch_table().grad_f64[M];
  if (!lng && !fn) return fail(IBS_ERR_UNSUPPORTED, "no kernel built for rows-per-lane M=%d (N=%d)", M, N);
  ON_DEVICE(ctx);
  const int wpb = ibs::plan_grad_wpb(ctx->chip, n_pts, N);
  if (wpb < 1) return fail(IBS_ERR_UNSUPPORTED, "N=%d does not fit the LDS staging", N);
  ibs::GradArgs<double> a{};
  a.n_pts = n_pts; a.N = N; a.h = h; a.ld = ld; a.del_alpha = del_alpha; a.wpb = wpb;
  const size_t n = (size_t)n_pts, geo_elems = n * 3 * 8 * ld;
  auto decl = [&](Stage& s) {
    a.gam = s.scratch<double>(n); a.dalpha = s.scratch<double>(n); a.dth0 = s.scratch<double>(n);
    a.geo = s.in(geo, geo_elems); a.theta0 = s.in(theta0, n);
    a.val = s.out(val, n); a.jac = s.out(jac, 2 * n);
    a.info = s.status(info, n);
    if (!s.host && !info) a.info = s.scratch<int>(n);        // (the kernels always write status words)
  };
  return staged(ctx, mem, decl, [&]() -> int {
    if (lng) return launch_grad_long(ctx, a);
    HIPCHK(fn(a, ctx->stream));
    return 0;
  });
}

// The mode rows a caller hands to the geometry entry points ({first mode, count} per row): 1 = every row lies inside the mode
// list and none has more pair indices about its centre than the row kernels' table image holds (ibs::kGeoMaxPairs = 64: a
// row of up to 129 modes centred on n = 0 -- VMEC's -ntor..ntor with ntor <= 64 -- or up to 65 modes otherwise; the centre
// rule is k_geo_prepare's), 0 = valid but a row is longer (the call then runs on the one-sincos-per-mode kernel, which takes
// any ordering), < 0 = a row outside the mode list (error set).  Host tables are checked on every call; device-resident
// ones are copied back ONCE per (pointers, counts, steps) -- a synchronisation the first call with a table set pays.
static int geo_rows_fit_host(const int32_t* rows, int nrows, int nmodes, const double* xn, double dn, const char* which) {
  int fit = 1;
  // (rows must not overlap: the table images of the row kernels are sized for ONE pair / group entry per mode -- 24 rows of
  //  {0, 65} over 65 modes would each be "inside the list" and together write 24 times the image)
  std::vector<char> taken((size_t)nmodes, 0);
  for (int r = 0; r < nrows; ++r) {
    const int first = rows[2 * r], cnt = rows[2 * r + 1];
    if (first < 0 || cnt < 1 || (long)first + cnt > nmodes) return fail(IBS_ERR_ARG, "%s[%d] = {%d, %d} lies outside the %d modes", which, r, first, cnt, nmodes);
    for (int k = first; k < first + cnt; ++k) {
      if (taken[k]) return fail(IBS_ERR_ARG, "%s[%d] = {%d, %d} overlaps an earlier row at mode %d: every mode may belong to one row only", which, r, first, cnt, k);
      taken[k] = 1;
    }
    if (cnt <= ibs::kGeoMaxPairs + 1) continue;
    int k0 = 0;
    if (dn != 0.0) {
      const double n0 = xn[first], kz = -n0 / dn;
      const int kr = (int)(kz + (kz >= 0 ? 0.5 : -0.5));
      if (kr >= 0 && kr < cnt && std::fabs(n0 + kr * dn) <= 1e-9 * std::fabs(dn)) k0 = kr;
    }
    if (std::max(k0, cnt - 1 - k0) > ibs::kGeoMaxPairs) fit = 0;
  }
  return fit;
}
static int geo_rows_fit(ibs_ctx* ctx, int mnmax, int mnmax_nyq, const double* xn, const double* xn_nyq, int nrows_mn,
                        const int32_t* rows_mn, int nrows_nyq, const int32_t* rows_nyq, double dn_mn, double dn_nyq, bool host) {
  if (host) {
    const int a = geo_rows_fit_host(rows_mn, nrows_mn, mnmax, xn, dn_mn, "rows_mn");
    if (a < 0) return a;
    const int b = geo_rows_fit_host(rows_nyq, nrows_nyq, mnmax_nyq, xn_nyq, dn_nyq, "rows_nyq");
    return b < 0 ? b : a;            // (only the first list feeds the (P, Q) tables; the second one's pair tables hold one entry per mode)
  }
  for (const auto& c : ctx->rows_seen)
    if (c.r1 == rows_mn && c.r2 == rows_nyq && c.xn == xn && c.xnq == xn_nyq && c.n1 == nrows_mn && c.n2 == nrows_nyq && c.mn == mnmax &&
        c.mnq == mnmax_nyq && c.d1 == dn_mn && c.d2 == dn_nyq && c.r1) return c.verdict;
  auto& c = ctx->rows_seen[ctx->rows_seen_next];
  ctx->rows_seen_next = (ctx->rows_seen_next + 1) % ibs_ctx::kRowsSeen;
  std::vector<int32_t> r1((size_t)2 * nrows_mn), r2((size_t)2 * nrows_nyq);
  std::vector<double> x1(mnmax), x2(mnmax_nyq);
  HIPCHK(hipMemcpyAsync(r1.data(), rows_mn, r1.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipMemcpyAsync(r2.data(), rows_nyq, r2.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipMemcpyAsync(x1.data(), xn, x1.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipMemcpyAsync(x2.data(), xn_nyq, x2.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  const int a = geo_rows_fit_host(r1.data(), nrows_mn, mnmax, x1.data(), dn_mn, "rows_mn");
  if (a < 0) return a;
  const int b = geo_rows_fit_host(r2.data(), nrows_nyq, mnmax_nyq, x2.data(), dn_nyq, "rows_nyq");
  if (b < 0) return b;
  c.r1 = rows_mn; c.r2 = rows_nyq; c.xn = xn; c.xnq = xn_nyq; c.n1 = nrows_mn; c.n2 = nrows_nyq; c.mn = mnmax; c.mnq = mnmax_nyq;
  c.d1 = dn_mn; c.d2 = dn_nyq; c.verdict = a;
  return c.verdict;
}

// workspace for the prepared table images of the geometry row kernels (ibs_geometry.hip): the set of the form `f`
static size_t geo_img_bytes(const ibs::GeoArgs& a, int lpp) {
  return ibs::geo_rows_usable(a, lpp) ? pad256((size_t)a.n_surf * ibs::geo_image_doubles(a, lpp) * sizeof(double)) : 0;
}

int ibs_fieldline_geometry_f64(ibs_ctx* ctx, int32_t n_surf, int32_t mnmax, int32_t mnmax_nyq, const double* xm,
                               const double* xn, const double* xm_nyq, const double* xn_nyq, const double* tab_mn,
                               const double* tab_nyq, const double* scal, int32_t n_lines, const int32_t* line_surf,
                               const double* line_alpha, int32_t N, const double* theta, int64_t ld, double* geo,
                               double* dPdrho, int32_t nrows_mn, const int32_t* rows_mn, int32_t nrows_nyq,
                               const int32_t* rows_nyq, double dn_mn, double dn_nyq, int32_t mem) {
  if (!ctx) return fail(IBS_ERR_ARG, "null context");
  if (nrows_mn < 0 || nrows_nyq < 0 || (nrows_mn > 0 && !rows_mn) || (nrows_nyq > 0 && !rows_nyq))
    return fail(IBS_ERR_ARG, "bad row tables");
  if (n_surf <= 0 || mnmax <= 0 || mnmax_nyq <= 0 || n_lines < 0 || N < 2 || ld < N || !xm || !xn || !xm_nyq || !xn_nyq ||
      !tab_mn || !tab_nyq || !scal || !line_surf || !line_alpha || !theta || !geo)
    return fail(IBS_ERR_ARG, "bad arguments");
  if (n_lines == 0) return 0;
  ON_DEVICE(ctx);
  ibs::GeoArgs a{};
  a.n_surf = n_surf; a.mnmax = mnmax; a.mnmax_nyq = mnmax_nyq; a.n_lines = n_lines; a.N = N; a.ld = ld;
  a.lpp = ctx->opt.geo_lpp;
  bool rows = nrows_mn > 0 && nrows_nyq > 0;
  if (rows) {
    const int fit = geo_rows_fit(ctx, mnmax, mnmax_nyq, xn, xn_nyq, nrows_mn, rows_mn, nrows_nyq, rows_nyq, dn_mn, dn_nyq, mem == IBS_MEM_HOST);
    if (fit < 0) return fit;
    rows = fit == 1;
  }
  if (rows) { a.nrows_mn = nrows_mn; a.nrows_nyq = nrows_nyq; a.dn_mn = dn_mn; a.dn_nyq = dn_nyq; }
  a.form = ibs::geo_pick_usable(a, n_lines, N, ctx->chip.n_cu);
  const size_t img_bytes = geo_img_bytes(a, a.form.lpp);
  const bool host = mem == IBS_MEM_HOST;
  if (host)
    for (int i = 0; i < n_lines; ++i)
      if (line_surf[i] < 0 || line_surf[i] >= n_surf) return fail(IBS_ERR_ARG, "line_surf[%d]=%d out of range", i, line_surf[i]);
  // a device-pointer call whose lines touch few of the surfaces (a large table set worked through piece by piece) builds their
  // images only
  const bool mark = !host && img_bytes && n_surf >= 32 && (long)n_lines < 8L * n_surf;
  const size_t n_mn = (size_t)n_surf * 6 * mnmax, n_nyq = (size_t)n_surf * 7 * mnmax_nyq;
  auto decl = [&](Stage& s) {
    a.xm = s.in(xm, mnmax); a.xn = s.in(xn, mnmax); a.xm_nyq = s.in(xm_nyq, mnmax_nyq); a.xn_nyq = s.in(xn_nyq, mnmax_nyq);
    a.tab_mn = s.in(tab_mn, n_mn); a.tab_nyq = s.in(tab_nyq, n_nyq); a.scal = s.in(scal, (size_t)n_surf * 6);
    a.line_surf = s.in(line_surf, n_lines); a.line_alpha = s.in(line_alpha, n_lines); a.theta = s.in(theta, N);
    if (rows) { a.rows_mn = s.in(rows_mn, (size_t)2 * nrows_mn); a.rows_nyq = s.in(rows_nyq, (size_t)2 * nrows_nyq); }
    // (host pointers with ld > N: the padding of the caller's rows stays as it was, as it does with device pointers)
    a.ld = (long)s.rows_ld(N, ld);
    a.geo = s.out_rows(geo, (size_t)8 * n_lines, N, ld); a.dPdrho = s.out(dPdrho, n_lines, true);
    if (img_bytes) a.img[ibs::geo_lpp_index(a.form.lpp)] = s.scratch<double>(img_bytes / sizeof(double));
    a.surf_used = s.scratch<int>(n_surf, mark);
  };
  return staged(ctx, mem, decl, [&]() -> int {
    HIPCHK(ibs::launch_geometry(a, ctx->stream, ctx->chip.n_cu));
    return 0;
  });
}

int ibs_fieldline_geometry_vjp_f64(ibs_ctx* ctx, int32_t n_surf, int32_t mnmax, int32_t mnmax_nyq, const double* xm,
                                   const double* xn, const double* xm_nyq, const double* xn_nyq, const double* tab_mn,
                                   const double* tab_nyq, const double* scal, int32_t n_lines, const int32_t* line_surf,
                                   const double* line_alpha, int32_t N, const double* theta, int64_t ld,
                                   const double* geo_bar, const double* dPdrho_bar, double* tab_mn_bar,
                                   double* tab_nyq_bar, double* scal_bar, double* alpha_bar, int32_t mem) {
  if (!ctx) return fail(IBS_ERR_ARG, "null context");
  if (n_lines < 0) return fail(IBS_ERR_ARG, "n_lines=%d < 0", n_lines);
  if (ld < N) return fail(IBS_ERR_ARG, "ld=%lld < N=%d", (long long)ld, N);
  if (n_surf <= 0 || mnmax <= 0 || mnmax_nyq <= 0 || N < 2 || !xm || !xn || !xm_nyq || !xn_nyq || !tab_mn || !tab_nyq ||
      !scal || !line_surf || !line_alpha || !theta || !geo_bar)
    return fail(IBS_ERR_ARG, "bad arguments");
  if (!tab_mn_bar && !tab_nyq_bar && !scal_bar && !alpha_bar) return fail(IBS_ERR_ARG, "no output requested");
  if (n_lines > 65535 || n_surf > 65535) return fail(IBS_ERR_UNSUPPORTED, "n_lines=%d, n_surf=%d: at most 65535 each", n_lines, n_surf);
  const bool host = mem == IBS_MEM_HOST;
  if (host)
    for (int i = 0; i < n_lines; ++i)
      if (line_surf[i] < 0 || line_surf[i] >= n_surf) return fail(IBS_ERR_ARG, "line_surf[%d]=%d out of range", i, line_surf[i]);
  ON_DEVICE(ctx);
  ibs::GeoVjpArgs a{};
  a.n_surf = n_surf; a.mnmax = mnmax; a.mnmax_nyq = mnmax_nyq; a.n_lines = n_lines; a.N = N; a.ld = ld;
  const size_t n_mn = (size_t)n_surf * 6 * mnmax, n_nyq = (size_t)n_surf * 7 * mnmax_nyq, n_geo = (size_t)8 * n_lines * ld;
  auto decl = [&](Stage& s) {
    a.xm = s.in(xm, mnmax); a.xn = s.in(xn, mnmax); a.xm_nyq = s.in(xm_nyq, mnmax_nyq); a.xn_nyq = s.in(xn_nyq, mnmax_nyq);
    a.tab_mn = s.in(tab_mn, n_mn); a.tab_nyq = s.in(tab_nyq, n_nyq); a.scal = s.in(scal, (size_t)n_surf * 6);
    a.line_surf = s.in(line_surf, n_lines); a.line_alpha = s.in(line_alpha, n_lines); a.theta = s.in(theta, N);
    a.geo_bar = s.in(geo_bar, n_geo); a.dPdrho_bar = s.in(dPdrho_bar, n_lines);
    a.tab_mn_bar = s.out(tab_mn_bar, n_mn); a.tab_nyq_bar = s.out(tab_nyq_bar, n_nyq);
    a.scal_bar = s.out(scal_bar, (size_t)n_surf * 6); a.alpha_bar = s.out(alpha_bar, n_lines);
    a.ws = s.scratch<double>((size_t)n_lines * ibs::kGeoVjpW * N);
  };
  // (without lines the points kernel has nothing to do; the reductions still write the zeros)
  return staged(ctx, mem, decl, [&]() -> int {
    HIPCHK(ibs::launch_geometry_vjp(a, ctx->stream));
    return 0;
  });
}

int ibs_fieldline_geometry_dalpha_f64(ibs_ctx* ctx, int32_t n_surf, int32_t mnmax, int32_t mnmax_nyq, const double* xm,
                                      const double* xn, const double* xm_nyq, const double* xn_nyq, const double* tab_mn,
                                      const double* tab_nyq, const double* scal, int32_t n_lines, const int32_t* line_surf,
                                      const double* line_alpha, int32_t N, const double* theta, int64_t ld, double* geo_da,
                                      int32_t mem) {
  if (!ctx) return fail(IBS_ERR_ARG, "null context");
  if (n_lines < 0) return fail(IBS_ERR_ARG, "n_lines=%d < 0", n_lines);
  if (ld < N) return fail(IBS_ERR_ARG, "ld=%lld < N=%d", (long long)ld, N);
  if (n_surf <= 0 || mnmax <= 0 || mnmax_nyq <= 0 || N < 2 || !xm || !xn || !xm_nyq || !xn_nyq || !tab_mn || !tab_nyq ||
      !scal || !line_surf || !line_alpha || !theta || !geo_da)
    return fail(IBS_ERR_ARG, "bad arguments");
  if (n_lines > 65535 || n_surf > 65535) return fail(IBS_ERR_UNSUPPORTED, "n_lines=%d, n_surf=%d: at most 65535 each", n_lines, n_surf);
  const bool host = mem == IBS_MEM_HOST;
  if (host)
    for (int i = 0; i < n_lines; ++i)
      if (line_surf[i] < 0 || line_surf[i] >= n_surf) return fail(IBS_ERR_ARG, "line_surf[%d]=%d out of range", i, line_surf[i]);
  if (n_lines == 0) return 0;
  ON_DEVICE(ctx);
  ibs::GeoDalphaArgs a{};
  a.n_surf = n_surf; a.mnmax = mnmax; a.mnmax_nyq = mnmax_nyq; a.n_lines = n_lines; a.N = N; a.ld = ld;
  const size_t n_mn = (size_t)n_surf * 6 * mnmax, n_nyq = (size_t)n_surf * 7 * mnmax_nyq;
  // (host pointers: the rows are packed on the device and come back one by one, so the caller's entries N..ld-1 stay as they were)
  auto decl = [&](Stage& s) {
    a.xm = s.in(xm, mnmax); a.xn = s.in(xn, mnmax); a.xm_nyq = s.in(xm_nyq, mnmax_nyq); a.xn_nyq = s.in(xn_nyq, mnmax_nyq);
    a.tab_mn = s.in(tab_mn, n_mn); a.tab_nyq = s.in(tab_nyq, n_nyq); a.scal = s.in(scal, (size_t)n_surf * 6);
    a.line_surf = s.in(line_surf, n_lines); a.line_alpha = s.in(line_alpha, n_lines); a.theta = s.in(theta, N);
    a.geo_da = s.out_rows(geo_da, (size_t)8 * n_lines, N, ld); a.ld = (long)s.rows_ld(N, ld);
  };
  return staged(ctx, mem, decl, [&]() -> int {
    HIPCHK(ibs::launch_geometry_dalpha(a, ctx->stream));
    return 0;
  });
}

int ibs_hf_grad_f64(ibs_ctx* ctx, int64_t n_sys, int32_t N, const double* X, const double* dX, const double* f,
                    const double* g_p, const double* c_p, const double* f_p, int64_t ld, const double* gam,
                    double* jac, int32_t mem) {
  if (!ctx) return fail(IBS_ERR_ARG, "null context");
  if (n_sys < 0 || !X || !dX || !f || !g_p || !c_p || !f_p || !gam || !jac || ld < N)
    return fail(IBS_ERR_ARG, "bad arguments");
  if (N < 3 || !(N & 1)) return fail(IBS_ERR_UNSUPPORTED, "N=%d: the Simpson rule of the reference needs N odd", N);
  if (n_sys == 0) return 0;
  ON_DEVICE(ctx);
  const size_t ne = (size_t)n_sys * ld;
  const double* d[7];
  double* djac;
  auto decl = [&](Stage& s) {
    const double* src[7] = {X, dX, f, g_p, c_p, f_p, gam};
    for (int k = 0; k < 7; ++k) d[k] = s.in(src[k], k < 6 ? ne : (size_t)n_sys);
    djac = s.out(jac, n_sys);
  };
  return staged(ctx, mem, decl, [&]() -> int {
    hipLaunchKernelGGL(k_hf_grad, dim3((unsigned)((n_sys + 3) / 4)), dim3(256), 0, ctx->stream, (long)n_sys, N, (long)ld, d[0], d[1], d[2],
                       d[3], d[4], d[5], d[6], djac);
    HIPCHK(hipGetLastError());
    return 0;
  });
}

int ibs_sturm_count_f64(ibs_ctx* ctx, int64_t n_sys, int32_t N, double h, const double* g, const double* c,
                        const double* f, int64_t ld, const double* shift, int32_t* count, int32_t mem) {
  if (!ctx) return fail(IBS_ERR_ARG, "null context");
  if (n_sys < 0 || !g || !c || !f || !shift || !count || ld < N) return fail(IBS_ERR_ARG, "bad arguments");
  // the Sturm count itself has no Simpson stage: even N is fine here
  if (N < 66 || N > ibs::kMaxLongN) return fail(IBS_ERR_UNSUPPORTED, "N=%d outside [66, %d]", N, ibs::kMaxLongN);
  if (!(h > 0)) return fail(IBS_ERR_ARG, "h must be > 0");
  if (n_sys == 0) return 0;
  const ibs::SturmPlan plan = ibs::plan_sturm(ctx->chip, ctx->opt, (long)n_sys, N);
  const int M = plan.M;
  auto fn = plan.form == 2 ? &ibs::launch_sturm_div : (plan.form == 3 ? &ibs::launch_sturm_long : ibs::launch_table().sturm_f64[M]);
  if (!fn) return fail(IBS_ERR_UNSUPPORTED, "no kernel built for rows-per-lane M=%d (N=%d)", M, N);
  ON_DEVICE(ctx);
  const int wpb = plan.wpb;
  if (wpb < 1) return fail(IBS_ERR_UNSUPPORTED, "N=%d needs %zu B of LDS per wave", N, plan.per_wave);
  ibs::SturmArgs<double> a{};
  a.n_sys = n_sys; a.N = N; a.h = h; a.ld = ld; a.wpb = wpb;
  const size_t in_elems = (size_t)n_sys * ld;
  auto decl = [&](Stage& s) {
    a.g = s.in(g, in_elems); a.c = s.in(c, in_elems); a.f = s.in(f, in_elems); a.shift = s.in(shift, n_sys);
    a.count = s.out(count, n_sys);
  };
  return staged(ctx, mem, decl, [&]() -> int {
    HIPCHK(fn(a, ctx->stream));
    return 0;
  });
}

// ---- geometry-fed Sturm count and the count-pair certificate of geometry-fed growth rates (ibs_certify.hip).  The argument checks
// come before any device use.
static int geo_cert_check(const ibs_ctx* ctx, int32_t n_lines, int32_t n_theta0, int32_t N, double h, const GeoLines& geo, bool even_ok) {
  if (!ctx) return fail(IBS_ERR_ARG, "null context");
  if (!geo.present()) return fail(IBS_ERR_ARG, "null argument (the seven geometry arrays are required)");
  if (!geo.dPdrho || !geo.theta0) return fail(IBS_ERR_ARG, "null argument (dPdrho and theta0 are required)");
  if (n_lines < 0 || n_theta0 < 0 || geo.ld < N)
    return fail(IBS_ERR_ARG, "bad arguments (n_lines=%d n_theta0=%d ld=%lld N=%d)", n_lines, n_theta0, (long long)geo.ld, N);
  if ((int64_t)n_lines * n_theta0 > (int64_t)std::numeric_limits<int32_t>::max())
    return fail(IBS_ERR_ARG, "n_lines * n_theta0 = %lld exceeds 2^31 - 1", (long long)((int64_t)n_lines * n_theta0));
  if (!even_ok) return check_grid(N, h, true);
  if (N < 66 || N > ibs::kMaxLongN) return fail(IBS_ERR_UNSUPPORTED, "N=%d outside [66, %d]", N, ibs::kMaxLongN);
  if (!(h > 0)) return fail(IBS_ERR_ARG, "h must be > 0");
  return 0;
}

int ibs_geo_sturm_count_f64(ibs_ctx* ctx, int32_t n_lines, int32_t n_theta0, int32_t N, double h, const double* bmag,
                            const double* gradpar, const double* cvdrift, const double* cvdrift0, const double* gds2,
                            const double* gds21, const double* gds22, int64_t ld, const double* dPdrho, const double* theta0,
                            const double* shift, int32_t* count, int32_t mem) {
  const GeoLines geo{{bmag, gradpar, cvdrift, cvdrift0, gds2, gds21, gds22}, ld, dPdrho, theta0};
  if (int r = geo_cert_check(ctx, n_lines, n_theta0, N, h, geo, true)) return r;   // (no Simpson stage: even N is fine)
  if (!shift || !count) return fail(IBS_ERR_ARG, "null argument (shift and count are required)");
  if (n_lines == 0 || n_theta0 == 0) return 0;
  ON_DEVICE(ctx);
  const size_t n_sys = (size_t)n_lines * n_theta0;
  ibs::CertifyArgs a{};
  a.n_lines = n_lines; a.n_theta0 = n_theta0; a.N = N; a.h = h; a.ld = (long)ld;
  auto decl = [&](Stage& s) {
    geo.declare(s, n_lines, n_theta0).into(a); a.shift = s.in(shift, n_sys);
    a.count = s.out(count, n_sys);
  };
  return staged(ctx, mem, decl, [&]() -> int {
    HIPCHK(ibs::launch_geo_count(a, ctx->stream));
    return 0;
  });
}

// geo.per_line: n_theta0 = 1 and theta0[n_lines] holds one value per line (the points form)
static int geo_certify_impl(ibs_ctx* ctx, int32_t n_lines, int32_t n_theta0, int32_t N, double h, const GeoLines& geo, const double* lam,
                            double tol_factor, int32_t* cert, int32_t mem) {
  if (int r = geo_cert_check(ctx, n_lines, n_theta0, N, h, geo, false)) return r;
  if (!lam || !cert) return fail(IBS_ERR_ARG, "null argument (lam and cert are required)");
  if (n_lines == 0 || n_theta0 == 0) return 0;
  ON_DEVICE(ctx);
  const size_t n_sys = (size_t)n_lines * n_theta0;
  ibs::CertifyArgs a{};
  a.n_lines = n_lines; a.n_theta0 = n_theta0; a.N = N; a.h = h; a.ld = (long)geo.ld; a.t0_stride = geo.per_line ? 1 : 0;
  a.tol_factor = tol_factor > 0 ? tol_factor : 4.0;
  auto decl = [&](Stage& s) {
    geo.declare(s, n_lines, n_theta0).into(a); a.lam = s.in(lam, n_sys);
    a.cert = s.out(cert, n_sys);
  };
  const int rc = staged(ctx, mem, decl, [&]() -> int {
    HIPCHK(ibs::launch_geo_certify(a, ctx->stream));
    return 0;
  });
  if (rc != 0 || mem != IBS_MEM_HOST) return rc;
  int n_open = 0;
  for (size_t i = 0; i < n_sys; ++i) n_open += cert[i] != 0;
  return n_open;
}

int ibs_gamma_scan_certify_f64(ibs_ctx* ctx, int32_t n_lines, int32_t n_theta0, int32_t N, double h, const double* bmag,
                               const double* gradpar, const double* cvdrift, const double* cvdrift0, const double* gds2,
                               const double* gds21, const double* gds22, int64_t ld, const double* dPdrho, const double* theta0,
                               const double* lam, double tol_factor, int32_t* cert, int32_t mem) {
  const GeoLines geo{{bmag, gradpar, cvdrift, cvdrift0, gds2, gds21, gds22}, ld, dPdrho, theta0};
  return geo_certify_impl(ctx, n_lines, n_theta0, N, h, geo, lam, tol_factor, cert, mem);
}

int ibs_gamma_points_certify_f64(ibs_ctx* ctx, int32_t n_pts, int32_t N, double h, const double* bmag, const double* gradpar,
                                 const double* cvdrift, const double* cvdrift0, const double* gds2, const double* gds21,
                                 const double* gds22, int64_t ld, const double* dPdrho, const double* theta0, const double* lam,
                                 double tol_factor, int32_t* cert, int32_t mem) {
  const GeoLines geo{{bmag, gradpar, cvdrift, cvdrift0, gds2, gds21, gds22}, ld, dPdrho, theta0, true};
  return geo_certify_impl(ctx, n_pts, 1, N, h, geo, lam, tol_factor, cert, mem);
}

// Device pointers: list, solve and second certificate are queued back to back; nothing is read back in between (the list and its
// counter stay on the device: ibs_certify.hip).  Host pointers: the in-out arrays go up with the inputs and come back as outputs.
static int geo_reclose_impl(ibs_ctx* ctx, int32_t n_lines, int32_t n_theta0, int32_t N, double h, const GeoLines& geo, double tol_factor,
                            int32_t* cert, double* lam, double* gam, double* X, double* dX, int32_t mem) {
  if (int r = geo_cert_check(ctx, n_lines, n_theta0, N, h, geo, false)) return r;
  if (!cert || !lam || !gam) return fail(IBS_ERR_ARG, "null argument (cert, lam and gam are required)");
  if (n_lines == 0 || n_theta0 == 0) return 0;
  ON_DEVICE(ctx);
  const size_t n_sys = (size_t)n_lines * n_theta0, out_elems = n_sys * (size_t)N;
  ibs::RecloseArgs a{};
  ibs::CertifyArgs& c = a.c;
  c.n_lines = n_lines; c.n_theta0 = n_theta0; c.N = N; c.h = h; c.ld = (long)geo.ld; c.t0_stride = geo.per_line ? 1 : 0;
  c.tol_factor = tol_factor > 0 ? tol_factor : 4.0;
  const int *cert_up = nullptr;
  const double *lam_up = nullptr, *gam_up = nullptr, *X_up = nullptr, *dX_up = nullptr;
  auto decl = [&](Stage& s) {
    geo.declare(s, n_lines, n_theta0).into(c);
    if (s.host) {
      cert_up = s.in((const int*)cert, n_sys); lam_up = s.in((const double*)lam, n_sys); gam_up = s.in((const double*)gam, n_sys);
      X_up = s.in((const double*)X, out_elems); dX_up = s.in((const double*)dX, out_elems);
    }
    c.cert = s.out(cert, n_sys); a.lam = s.out(lam, n_sys); a.gam = s.out(gam, n_sys); a.X = s.out(X, out_elems); a.dX = s.out(dX, out_elems);
  };
  const int rc = staged(ctx, mem, decl, [&]() -> int {
    if (mem == IBS_MEM_HOST) {
      HIPCHK(hipMemcpyAsync(c.cert, cert_up, n_sys * sizeof(int), hipMemcpyDeviceToDevice, ctx->stream));
      HIPCHK(hipMemcpyAsync(a.lam, lam_up, n_sys * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
      HIPCHK(hipMemcpyAsync(a.gam, gam_up, n_sys * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
      if (X) HIPCHK(hipMemcpyAsync(a.X, X_up, out_elems * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
      if (dX) HIPCHK(hipMemcpyAsync(a.dX, dX_up, out_elems * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    }
    // re-closing is rare: at most one wave per CU, and at most 256 MiB of row workspace
    const size_t per_wave = ibs::reclose_ws_doubles(N) * sizeof(double);
    long nw = (long)n_sys < ctx->chip.n_cu ? (long)n_sys : ctx->chip.n_cu;
    const long fit = (long)((size_t(256) << 20) / per_wave);
    if (nw > fit) nw = fit;
    if (nw < 1) nw = 1;
    if (int r = carve_long(ctx, [&](Carve& cv) {
          a.list = cv.take<int>(1 + n_sys);
          a.work = cv.take<double>((size_t)nw * ibs::reclose_ws_doubles(N));
        })) return r;
    a.n_waves = (int)nw;
    HIPCHK(ibs::launch_geo_reclose(a, ctx->stream));
    return 0;
  });
  if (rc != 0 || mem != IBS_MEM_HOST) return rc;
  int n_open = 0;
  for (size_t i = 0; i < n_sys; ++i) n_open += (cert[i] & (ibs::kCertNotMax | ibs::kCertNoEig)) != 0;
  return n_open;
}

int ibs_gamma_scan_reclose_f64(ibs_ctx* ctx, int32_t n_lines, int32_t n_theta0, int32_t N, double h, const double* bmag,
                               const double* gradpar, const double* cvdrift, const double* cvdrift0, const double* gds2,
                               const double* gds21, const double* gds22, int64_t ld, const double* dPdrho, const double* theta0,
                               double tol_factor, int32_t* cert, double* lam, double* gam, double* X, double* dX, int32_t mem) {
  const GeoLines geo{{bmag, gradpar, cvdrift, cvdrift0, gds2, gds21, gds22}, ld, dPdrho, theta0};
  return geo_reclose_impl(ctx, n_lines, n_theta0, N, h, geo, tol_factor, cert, lam, gam, X, dX, mem);
}

int ibs_gamma_points_reclose_f64(ibs_ctx* ctx, int32_t n_pts, int32_t N, double h, const double* bmag, const double* gradpar,
                                 const double* cvdrift, const double* cvdrift0, const double* gds2, const double* gds21,
                                 const double* gds22, int64_t ld, const double* dPdrho, const double* theta0, double tol_factor,
                                 int32_t* cert, double* lam, double* gam, double* X, double* dX, int32_t mem) {
  const GeoLines geo{{bmag, gradpar, cvdrift, cvdrift0, gds2, gds21, gds22}, ld, dPdrho, theta0, true};
  return geo_reclose_impl(ctx, n_pts, 1, N, h, geo, tol_factor, cert, lam, gam, X, dX, mem);
}

int ibs_surface_argmax_f64(ibs_ctx* ctx, int32_t n_surf, int32_t n_per, const double* gam, int32_t* idx,
                           double* val, int32_t mem) {
  if (!ctx) return fail(IBS_ERR_ARG, "null context");
  if (n_surf < 0 || n_per <= 0 || !gam || !idx || !val) return fail(IBS_ERR_ARG, "bad arguments");
  if (n_surf == 0) return 0;
  ON_DEVICE(ctx);
  const double* dg;
  int* di;
  double* dv;
  auto decl = [&](Stage& s) { dg = s.in(gam, (size_t)n_surf * n_per); di = s.out(idx, n_surf); dv = s.out(val, n_surf); };
  return staged(ctx, mem, decl, [&]() -> int {
    hipLaunchKernelGGL(k_surface_argmax, dim3(n_surf), dim3(argmax_threads(n_per)), 0, ctx->stream, n_per, dg, di, dv, (double*)nullptr);
    HIPCHK(hipGetLastError());
    return 0;
  });
}

int ibs_surface_argmax_pack_f64(ibs_ctx* ctx, int32_t n_surf, int32_t n_per, const double* gam, double* pack) {
  if (!ctx) return fail(IBS_ERR_ARG, "null context");
  if (n_surf < 0 || n_per <= 0 || !gam || !pack) return fail(IBS_ERR_ARG, "bad arguments");
  if (n_surf == 0) return 0;
  ON_DEVICE(ctx);
  hipLaunchKernelGGL(k_surface_argmax, dim3(n_surf), dim3(argmax_threads(n_per)), 0, ctx->stream, n_per, gam, (int*)nullptr, (double*)nullptr, pack);
  HIPCHK(hipGetLastError());
  return 0;
}

int ibs_scan_peaks_f64(ibs_ctx* ctx, int32_t n_surf, int32_t n_alpha, int32_t n_theta0, int32_t n_starts, const double* alpha,
                       const double* theta0, const double* gam, double* start, double* peak, int32_t* index, double* sigma0,
                       int32_t* n_found, int32_t* n_bad, int32_t mem) {
  if (n_surf < 0 || n_alpha < 1 || n_theta0 < 1 || n_starts < 1 || n_starts > ibs::kMaxStarts || !alpha || !theta0 || !gam || !start ||
      !peak || !n_bad)
    return fail(IBS_ERR_ARG, "bad arguments (n_starts in [1, %d], every dimension >= 1, gam, start, peak and n_bad required)", ibs::kMaxStarts);
  if (!ctx) return fail(IBS_ERR_ARG, "null context");
  if ((int64_t)n_alpha * n_theta0 > 0x7fffffff / 2) return fail(IBS_ERR_ARG, "n_alpha * n_theta0 too large");
  if (n_surf == 0) return 0;
  ON_DEVICE(ctx);
  const int n_per = n_alpha * n_theta0;
  const size_t ns = (size_t)n_surf, K = (size_t)n_starts;
  const bool host = mem == IBS_MEM_HOST;
  int added = 0;                     // host pointers: the call's own count, added to *n_bad once the outputs are back
  ibs::ScanPeaksArgs a{n_surf, n_alpha, n_theta0, n_starts};
  auto decl = [&](Stage& s) {
    a.alpha = s.in(alpha, (size_t)n_alpha); a.theta0 = s.in(theta0, (size_t)n_theta0); a.gam = s.in(gam, ns * n_per);
    a.start = s.out(start, 2 * ns * K); a.peak = s.out(peak, ns * K); a.index = s.out(index, ns * K); a.sigma0 = s.out(sigma0, ns * K);
    a.n_found = s.out(n_found, ns); a.n_bad = host ? s.out(&added, 1) : n_bad;
  };
  const int rc = staged(ctx, mem, decl, [&]() -> int {
    if (host) HIPCHK(hipMemsetAsync(a.n_bad, 0, sizeof(int), ctx->stream));
    HIPCHK(ibs::launch_scan_peaks(a, argmax_threads(n_per), ctx->stream));
    return 0;
  });
  if (rc == 0 && host) *n_bad += added;
  return rc;
}

// ---- gam maximised over theta0 on every line (k_theta0_polish; the rule: ibs_theta0_polish.hpp)
int ibs_theta0_polish_f64(ibs_ctx* ctx, int32_t n_lines, int32_t n_theta0, int32_t N, double h, const double* bmag,
                          const double* gradpar, const double* cvdrift, const double* cvdrift0, const double* gds2,
                          const double* gds21, const double* gds22, int64_t ld, const double* dPdrho, const double* theta0,
                          const double* gam, const double* lam, const int32_t* node_in, int32_t n_starts, double xtol,
                          int32_t max_eval, double* theta0_star, double* gam_star, double* lam_star, int32_t* node,
                          int32_t* n_eval, int32_t* info, int32_t* n_found, int32_t mem) {
  const GeoLines geo{{bmag, gradpar, cvdrift, cvdrift0, gds2, gds21, gds22}, ld, dPdrho, theta0};
  if (n_starts < 1 || n_starts > ibs::t0p::kMaxSlots || !(xtol > 0) || !std::isfinite(xtol) || max_eval < 1 ||
      max_eval > ibs::t0p::kMaxEval)
    return fail(IBS_ERR_ARG, "n_starts in [1, %d], xtol > 0 and finite, max_eval in [1, %d] required (n_starts=%d xtol=%g max_eval=%d)",
                ibs::t0p::kMaxSlots, ibs::t0p::kMaxEval, n_starts, xtol, max_eval);
  if (n_lines < 0 || n_theta0 < 1 || N < 1 || !geo.present() || !dPdrho || !theta0 || !gam || !theta0_star || !gam_star || ld < N)
    return fail(IBS_ERR_ARG, "bad arguments (n_lines=%d n_theta0=%d ld=%lld N=%d; the arrays, theta0, gam, theta0_star and gam_star are required)",
                n_lines, n_theta0, (long long)ld, N);
  if (int r = check_grid(N, h)) return r;
  const bool host = mem == IBS_MEM_HOST;
  if (host && !ibs::t0p::grid_ok(theta0, n_theta0)) return fail(IBS_ERR_ARG, "theta0 must be finite and strictly increasing");
  if (!ctx) return fail(IBS_ERR_ARG, "null context");
  if (n_lines == 0) return 0;
  const ibs::Theta0PolishPlan plan = ibs::plan_theta0_polish(ctx->chip, ctx->built, N, n_starts);
  auto fn = ibs::launch_table().theta0_polish_f64[plan.M];
  if (plan.err == ibs::PlanError::NotBuilt || !fn) return fail(IBS_ERR_UNSUPPORTED, "no kernel built for rows-per-lane M=%d (N=%d)", plan.M, N);
  if (plan.err == ibs::PlanError::NoLds) return fail(IBS_ERR_UNSUPPORTED, "N=%d does not fit the LDS staging", N);
  ON_DEVICE(ctx);
  ibs::Theta0PolishArgs<double> a{};
  a.n_lines = n_lines; a.n_theta0 = n_theta0; a.N = N; a.h = h; a.ld = ld;
  a.n_starts = n_starts; a.xtol = xtol; a.max_eval = max_eval; a.w1 = ctx->opt.chain_w1; a.w2 = ctx->opt.chain_w2;
  const size_t n_sys = (size_t)n_lines * n_theta0, n_slots = (size_t)n_lines * n_starts;
  auto decl = [&](Stage& s) {
    geo.declare(s, n_lines, n_theta0).into_named(a); a.gam = s.in(gam, n_sys); a.lam = s.in(lam, n_sys);
    a.node_in = s.in(node_in, n_slots);
    a.theta0_star = s.out(theta0_star, n_slots); a.gam_star = s.out(gam_star, n_slots); a.lam_star = s.out(lam_star, n_slots);
    a.node = s.out(node, n_slots); a.n_eval = s.out(n_eval, n_slots); a.n_found = s.out(n_found, (size_t)n_lines);
    a.info = s.status(info, n_slots);
  };
  return staged(ctx, mem, decl, [&]() -> int {
    HIPCHK(fn(a, ctx->stream));
    return 0;
  });
}

int ibs_refine_f64(ibs_ctx* ctx, int32_t n_surf, int32_t mnmax, int32_t mnmax_nyq, const double* xm, const double* xn,
                   const double* xm_nyq, const double* xn_nyq, const double* tab_mn, const double* tab_nyq,
                   const double* scal, int32_t nrows_mn, const int32_t* rows_mn, int32_t nrows_nyq,
                   const int32_t* rows_nyq, double dn_mn, double dn_nyq, int32_t n_pts, const int32_t* pt_surf,
                   const double* start, int32_t N, const double* theta, double del_alpha, int32_t maxiter,
                   double ftol, double gtol, double* x_opt, double* f_opt, int32_t* n_evals, int32_t mem) {
  if (!ctx) return fail(IBS_ERR_ARG, "null context");
  if (nrows_mn < 0 || nrows_nyq < 0 || (nrows_mn > 0 && !rows_mn) || (nrows_nyq > 0 && !rows_nyq))
    return fail(IBS_ERR_ARG, "bad row tables");
  if (n_surf <= 0 || mnmax <= 0 || mnmax_nyq <= 0 || n_pts < 0 || !xm || !xn || !xm_nyq || !xn_nyq || !tab_mn ||
      !tab_nyq || !scal || !theta || !(del_alpha > 0) || maxiter < 0)
    return fail(IBS_ERR_ARG, "bad arguments");
  if (n_pts == 0) return 0;                   // (an empty batch -- a rank without surfaces -- has no per-point arrays to point at)
  if (!pt_surf || !start || !x_opt || !f_opt) return fail(IBS_ERR_ARG, "bad arguments");
  ON_DEVICE(ctx);
  const bool host = (mem == IBS_MEM_HOST);
  if (N < 2) return fail(IBS_ERR_ARG, "N=%d", N);
  if (int r = check_grid(N, 1.0)) return r;
  if (host) {                                 // (device-resident grids are checked by k_refine_init)
    const double h = (theta[N - 1] - theta[0]) / (N - 1);
    if (!(h > 0)) return fail(IBS_ERR_ARG, "h must be > 0");
    for (int j = 1; j < N; ++j)
      if (fabs((theta[j] - theta[j - 1]) - h) > 1e-9 * fabs(h)) return fail(IBS_ERR_UNSUPPORTED, "theta grid is not uniform");
    for (int i = 0; i < n_pts; ++i)
      if (pt_surf[i] < 0 || pt_surf[i] >= n_surf) return fail(IBS_ERR_ARG, "pt_surf[%d]=%d out of range", i, pt_surf[i]);
  }
  const int M = rows_per_lane(N);
  auto eval = ibs::launch_table().refine_f64[M];
  if (!eval) return fail(IBS_ERR_UNSUPPORTED, "no kernel built for rows-per-lane M=%d (N=%d)", M, N);
  // LDS of the evaluation kernel: centre line (7 derived arrays) + eigenfunction + alpha-tangent (4 arrays) when they fit
  const size_t row_b = (size_t)ibs::lds_pitch(N) * sizeof(double);
  const size_t lds_extra = 32 * sizeof(double) + sizeof(RefineState) + sizeof(ibs::lbfgsb2::Work);
  // The alpha-tangent (4 more rows) in LDS saves the evaluation's sums a second trip to global memory but leaves room for ONE
  // block per CU at N = 969 (105 of 160 KB); without it two fit (70 KB each).  Batches with more points than CUs take the
  // second form: their first rounds would otherwise run in two waves of blocks.
  int lds_tangent = (12 * row_b + lds_extra <= (size_t)ctx->chip.lds_per_block) ? 1 : 0;
  if (ctx->opt.refine_tangent == 0 || (ctx->opt.refine_tangent < 0 && n_pts > ctx->chip.n_cu)) lds_tangent = 0;
  if (8 * row_b + lds_extra > (size_t)ctx->chip.lds_per_block) return fail(IBS_ERR_UNSUPPORTED, "N=%d does not fit the LDS staging", N);
  // every round = one objective/gradient evaluation of every point still in the batch.  An iteration takes at most
  // maxls = 20 line-search evaluations, and once more after a memory restart
  const int max_rounds = 2 + 42 * (maxiter > 0 ? maxiter : 1);
  const int hist_len = (max_rounds + 2 + 1) & ~1;      // then: two 64-bit statistics words, one status word
  if (ctx->refine_hist_len < hist_len) {
    if (ctx->refine_hist) { HIPCHK(hipStreamSynchronize(ctx->stream)); HIPCHK(hipHostFree(ctx->refine_hist)); ctx->refine_hist = nullptr; ctx->refine_hist_len = 0; }
    HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&ctx->refine_hist), (size_t)(hist_len + 8) * sizeof(int), hipHostMallocDefault));
    ctx->refine_hist_len = hist_len;
  } else if (ctx->refine_pending) {
    HIPCHK(hipStreamSynchronize(ctx->stream));           // (the output kernel of the previous call posts its statistics here)
  }
  ctx->refine_pending = false;
  volatile int* hist = ctx->refine_hist;
  long long* h_stats = reinterpret_cast<long long*>(ctx->refine_hist + ctx->refine_hist_len);
  volatile int* h_status = ctx->refine_hist + ctx->refine_hist_len + 4;
  for (int r = 0; r < max_rounds + 2; ++r) hist[r] = 0;
  hist[0] = n_pts + 1;
  h_stats[0] = 0; h_stats[1] = 0; *h_status = 0;
  const long ld = N;
  const int n_lines = 3 * n_pts;
  const size_t n_mn = (size_t)n_surf * 6 * mnmax, n_nyq = (size_t)n_surf * 7 * mnmax_nyq, n_geo = (size_t)8 * n_lines * ld;
  ibs::GeoArgs ga{};
  ga.n_surf = n_surf; ga.mnmax = mnmax; ga.mnmax_nyq = mnmax_nyq; ga.n_lines = n_lines; ga.N = N; ga.ld = ld;
  ga.lpp = ctx->opt.geo_lpp;
  if (nrows_mn > 0 && nrows_nyq > 0) {
    const int fit = geo_rows_fit(ctx, mnmax, mnmax_nyq, xn, xn_nyq, nrows_mn, rows_mn, nrows_nyq, rows_nyq, dn_mn, dn_nyq, host);
    if (fit < 0) return fit;
    if (fit == 1) { ga.nrows_mn = nrows_mn; ga.nrows_nyq = nrows_nyq; ga.dn_mn = dn_mn; ga.dn_nyq = dn_nyq; }
  }
  // the lanes-per-point forms the rounds can take as the batch shrinks (geo_pick_form is monotone in the batch size)
  const int lpp_first = ibs::geo_pick_usable(ga, n_lines, N, ctx->chip.n_cu).lpp;
  const int lpp_last = ibs::geo_pick_usable(ga, 3, N, ctx->chip.n_cu).lpp;
  ibs::RefineEvalArgs<double> ea{};
  const double *d_th, *d_start;
  RefineState* d_st;
  RefineCtrl* d_ctrl;
  double *d_xo, *d_fo;
  int* d_ne;
  auto decl = [&](Stage& s) {
    ga.xm = s.in(xm, mnmax); ga.xn = s.in(xn, mnmax); ga.xm_nyq = s.in(xm_nyq, mnmax_nyq); ga.xn_nyq = s.in(xn_nyq, mnmax_nyq);
    ga.tab_mn = s.in(tab_mn, n_mn); ga.tab_nyq = s.in(tab_nyq, n_nyq); ga.scal = s.in(scal, (size_t)n_surf * 6);
    if (ga.nrows_mn) { ga.rows_mn = s.in(rows_mn, (size_t)2 * nrows_mn); ga.rows_nyq = s.in(rows_nyq, (size_t)2 * nrows_nyq); }
    d_th = s.in(theta, N); ea.pt_surf = s.in(pt_surf, n_pts); d_start = s.in(start, (size_t)2 * n_pts);
    // (host pointers: n_evals is written on the device whether it is asked for or not)
    d_xo = s.out(x_opt, (size_t)2 * n_pts); d_fo = s.out(f_opt, n_pts); d_ne = s.out(n_evals, n_pts, true);
    ga.geo = s.scratch<double>(n_geo); ea.line_surf = s.scratch<int>(n_lines); ea.line_alpha = s.scratch<double>(n_lines);
    ea.th0 = s.scratch<double>(n_pts); ea.idx = s.scratch<int>(n_pts); d_st = s.scratch<RefineState>(n_pts);
    ea.gam = s.scratch<double>(n_pts); ea.dalpha = s.scratch<double>(n_pts); ea.dth0 = s.scratch<double>(n_pts);
    ea.info = s.scratch<int>(n_pts); d_ctrl = s.scratch<RefineCtrl>(1);
    for (int lpp = lpp_first; lpp <= lpp_last; lpp *= 2)
      if (geo_img_bytes(ga, lpp)) ga.img[ibs::geo_lpp_index(lpp)] = s.scratch<double>(geo_img_bytes(ga, lpp) / sizeof(double));
  };
  const hipStream_t st = ctx->stream;
  int enq = 0, rounds = -1;
  auto launch = [&]() -> int {
    ga.theta = d_th; ga.dPdrho = nullptr;
    ga.n_lines_dev = &d_ctrl->n_lines;
    ga.plane = (size_t)n_lines * ld;                                        // fixed: the batch shrinks, the planes stay

    RefineParams prm{};
    prm.lo[0] = 0.0; prm.lo[1] = 0.0; prm.hi[0] = 3.141592653589793; prm.hi[1] = 1.5707963267948966;   // ball_scan.py:311
    prm.del_alpha = del_alpha; prm.ftol = ftol; prm.gtol = gtol; prm.maxiter = maxiter; prm.n_surf = n_surf;
    ea.N = N; ea.geo = ga.geo; ea.ld = ld; ea.plane = ga.plane;
    ea.st = d_st; ea.prm = prm; ea.ctrl = d_ctrl;
    ga.line_surf = ea.line_surf; ga.line_alpha = ea.line_alpha;
    ea.hist = ctx->refine_hist; ea.hist_len = max_rounds + 2; ea.lds_tangent = lds_tangent;

    const dim3 grd((unsigned)((n_pts + 127) / 128)), blk(128);
    const dim3 gri((unsigned)((n_pts > N ? n_pts : N) + 127) / 128);
    hipLaunchKernelGGL(k_refine_init, gri, blk, 0, st, n_pts, ea.pt_surf, d_start, d_st, prm, ea.idx, ea.line_surf, ea.line_alpha, ea.th0,
                       d_ctrl, N, d_th, ctx->refine_hist + ctx->refine_hist_len + 4);
    HIPCHK(hipGetLastError());
    // Rounds are enqueued kLook ahead of the last one whose count the device has posted: the grid sizes and the geometry
    // form of round r are functions of the count after round r - 1 - kLook -- of the trajectory, not of host timing, so the
    // arithmetic (summation order of the geometry kernel's forms) is reproducible -- and the GPU never waits for the host.
    // Rounds enqueued after the last point has finished find an empty batch and return at once.
    constexpr int kLook = 1;
    while (enq < max_rounds) {
      const int need_r = enq > kLook ? enq - kLook : 0;
      int spins = 0;
      const auto t_start = std::chrono::steady_clock::now();       // (the limit is per awaited round, not per call)
      while (hist[need_r] == 0) {
        if (++spins > 2000) {
          std::this_thread::yield();
          if (std::chrono::steady_clock::now() - t_start > std::chrono::seconds(120)) {
            (void)hipStreamSynchronize(st);
            return fail(IBS_ERR_HIP, "refinement round %d did not report within 120 s", need_r);
          }
        }
      }
      const int nc = hist[need_r] - 1;
      if (nc <= 0) { rounds = need_r; break; }
      ga.n_lines = 3 * nc;
      ga.form = ibs::geo_pick_usable(ga, ga.n_lines, N, ctx->chip.n_cu);
      HIPCHK(ibs::launch_geometry(ga, st, ctx->chip.n_cu));
      ea.n_c_max = nc;
      HIPCHK(eval(ea, st));
      ++enq;
    }
    hipLaunchKernelGGL(k_refine_out, grd, blk, 0, st, n_pts, d_st, d_xo, d_fo, d_ne, h_stats);
    HIPCHK(hipGetLastError());
    ctx->refine_pending = !host;         // (host pointers: staged() waits for the stream)
    return 0;
  };
  if (int r = staged(ctx, mem, decl, launch)) return r;
  // device pointers: the results are complete once the stream reaches this point (the rounds themselves are known to be
  // over -- their counts were read above -- unless the loop ended on the round limit)
  if (rounds < 0 && ctx->refine_pending) { HIPCHK(hipStreamSynchronize(st)); ctx->refine_pending = false; }
  if (*h_status != 0) {
    HIPCHK(hipStreamSynchronize(st)); ctx->refine_pending = false;
    return *h_status == 1 ? fail(IBS_ERR_UNSUPPORTED, "theta grid is not uniform") : fail(IBS_ERR_ARG, "h must be > 0");
  }
  if (rounds < 0) {                       // (the loop ended on max_rounds, or the last rounds' counts were not looked at yet)
    rounds = enq;
    for (int r = 0; r <= enq; ++r) if (hist[r] == 1) { rounds = r; break; }
  }
  ctx->refine_stats[2] = rounds; ctx->refine_stats[3] = enq;
  return rounds;
}

/* statistics of the last ibs_refine_f64 call of this context: evaluations, forward sweeps of the eigen-solves, rounds needed, rounds enqueued */
int ibs_refine_stats(ibs_ctx* ctx, int64_t* out4) {
  if (!ctx || !out4) return fail(IBS_ERR_ARG, "null pointer");
  if (ctx->refine_pending) { ON_DEVICE(ctx); HIPCHK(hipStreamSynchronize(ctx->stream)); ctx->refine_pending = false; }
  if (ctx->refine_hist) {
    const long long* h_stats = reinterpret_cast<const long long*>(ctx->refine_hist + ctx->refine_hist_len);
    ctx->refine_stats[0] = h_stats[0]; ctx->refine_stats[1] = h_stats[1];
  }
  for (int i = 0; i < 4; ++i) out4[i] = ctx->refine_stats[i];
  return 0;
}

}  // extern "C"
