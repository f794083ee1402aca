// Alpha-tangent of the field-line geometry (ibs_geometry.hip): d/d alpha of the eight arrays of every line, in place of the
// reference's central difference of the rows over del_alpha (utils.py:1641-1646 / 1683-1718).  The arithmetic differentiated is the
// reference's vmec_fieldlines (utils.py:359-720) in the plain form of ibs_geometry_vjp.hpp.
//
//   k_geo_dalpha_points   one lane per grid point, grid (ceil(N / 64), n_lines) as k_geo_vjp_points: geo_dalpha_point
//                         (ibs_geometry_tangent.hpp) and eight stores.  No atomics, no cross-lane sums, nothing shared between
//                         points: a line alone gives the bits it has in a batch.
// Any mode ordering: no use of the row structure.
#include <hip/hip_runtime.h>
#include "ibs_launch.hpp"
#include "ibs_geometry_tangent.hpp"

namespace ibs {

__global__ void __launch_bounds__(64) k_geo_dalpha_points(GeoDalphaArgs a) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j < a.N) geo_dalpha_point(a, blockIdx.y, j);
}

hipError_t launch_geometry_dalpha(GeoDalphaArgs& a, hipStream_t st) {
  if (!a.plane) a.plane = (size_t)a.n_lines * a.ld;
  if (a.n_lines <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_geo_dalpha_points, dim3((a.N + 63) / 64, a.n_lines), dim3(64), 0, st, a);
  note_launch((long)((a.N + 63) / 64) * a.n_lines, 64, "ibs::k_geo_dalpha_points");
  return hipGetLastError();
}

}  // namespace ibs
