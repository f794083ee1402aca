// Launch arguments of the geometry-fed Sturm count and of the count-pair certificate of geometry-fed growth rates (ibs_certify.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace ibs {

constexpr int kCertChunk = 16;                 // grid points of every staged line per pass through LDS: one 128-byte line per row
constexpr int kCertPitch = kCertChunk + 1;     // (odd pitch in doubles: lanes on different lines read different banks)
constexpr int kCertRows = 7;                   // staged per grid point: A1, A3, C0, C1 (theta0-free factors of g, f, c) and gds2, gds21, gds22
constexpr int kCertMaxLines = 64;              // a wave's 64 systems lie on at most 64 lines (the points form)
constexpr size_t cert_lds_bytes(int lines) { return (size_t)lines * kCertRows * kCertPitch * sizeof(double); }
static_assert(cert_lds_bytes(kCertMaxLines) <= 64 * 1024, "the staged lines of one wave must fit a block's LDS");

// cert word of a system: bit 0 = an eigenvalue lies above lam + tol (lam is not lam_max), bit 1 = none lies above lam - tol (no
// eigenvalue at lam), bit 2 = not checked (lam not finite or invalid data), bit 3 = re-closed and certified (informational);
// bit 4 is the library's own mark between the steps of a re-close and never leaves it.
constexpr int kCertNotMax = 1, kCertNoEig = 2, kCertUnchecked = 4, kCertReclosed = 8, kCertPending = 16;

struct CertifyArgs {
  int n_lines, n_theta0, N; double h;
  const double* geo7[7]; long ld;              // bmag gradpar cvdrift cvdrift0 gds2 gds21 gds22, [n_lines][ld]
  const double *dPdrho, *theta0; int t0_stride;      // t0_stride: 0 = theta0[n_theta0] of every line, 1 = theta0[n_lines] (n_theta0 = 1)
  const double* shift; int* count;             // the count form: [n_lines][n_theta0]
  const double* lam; double tol_factor; int* cert;   // the certificate: tol = tol_factor N eps ||A||
  int recheck;                                 // 1 = only systems marked kCertPending: certified -> kCertReclosed alone, else the mark is taken off
};
hipError_t launch_geo_count(const CertifyArgs& a, hipStream_t st);
hipError_t launch_geo_certify(const CertifyArgs& a, hipStream_t st);

// re-close of the systems whose cert word has bit 0 or 1 (and not bit 2): listed on the device, solved again in division form by one
// wave per listed system (the long-grid pieces of ibs_long.hpp on rows written to the wave's workspace), marked kCertPending.
// Workspace: list [1 + n_sys] ints, work [n_waves][reclose_ws_doubles(N)] doubles.
constexpr size_t reclose_ws_doubles(int N) { return 6 * (size_t)N; }      // g, c, f rows + D+, D-, z of long_vector_growth
struct RecloseArgs {
  CertifyArgs c;                               // geometry, theta0 and cert as above
  double *lam, *gam, *X, *dX;                  // [n_sys] ([n_sys][N]: X, dX, optional): overwritten for the listed systems only
  int* list; double* work; int n_waves;
};
hipError_t launch_geo_reclose(const RecloseArgs& a, hipStream_t st);

}  // namespace ibs
