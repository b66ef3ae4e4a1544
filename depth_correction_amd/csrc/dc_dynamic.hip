// Dynamic-point probabilities of the mapper's map (gfx950): which map points belong to something that moved (launch/slam.launch
// compute_prob_dynamic; Pomerleau et al., ICRA 2014).  C ABI at the bottom; see include/dc_hip.h.  The rule, its deviations and its
// measured cost are in DESIGN "Dynamic points in the map"; the per-row arithmetic is dc_dynmath.h, which the host build shares.
//
// One update of the map against a registered reading:
//   dc_dyn_directions                   unit directions and depths of the map points (seen from the pose) and of the reading points;
//   dc_compact_rows   (dc_filters.hip)  the valid rows of both, with their row numbers;
//   dc_knn_grid_build / dc_knn_grid_query (dc_knn.hip)  every valid map direction's nearest reading direction within the beam's chord;
//   dc_dyn_update                       the visibility test and the Bayesian update of the matched map points.
// Both kernels here stream their rows once (one 24-byte gather per matched row in the update), use no LDS and no atomics and are
// bound by memory; a thread owns its rows, so the same inputs give the same bits.
#include "dc_common.h"
#include "../../include/dc_hip.h"
#include "dc_device.h"
#include "dc_hostutil.h"
#include "dc_dynmath.h"

namespace dc {

constexpr int64_t kDynBlocksMax = 1 << 16;       // the grid-stride loops take the rest

static unsigned dyn_blocks(int64_t n) {
  const int64_t b = (n + kBlock - 1) / kBlock;
  return (unsigned)(b < 1 ? 1 : (b > kDynBlocksMax ? kDynBlocksMax : b));
}

__global__ __launch_bounds__(kBlock) void dyn_directions_kernel(const double* __restrict__ points, int64_t n, const double* __restrict__ pose,
                                                                double max_range, double* __restrict__ dirs, double* __restrict__ depth,
                                                                uint8_t* __restrict__ valid) {
  double T[16];
  if (pose) {
#pragma unroll
    for (int q = 0; q < 16; ++q) T[q] = pose[q];
  }
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
    const double q[3] = {points[i * 3], points[i * 3 + 1], points[i * 3 + 2]};
    double d[3], x[3], u[3], rho;
    const bool ok = dyn_direction(pose ? T : nullptr, q, max_range, d, x, &rho, u);
    dirs[i * 3] = u[0]; dirs[i * 3 + 1] = u[1]; dirs[i * 3 + 2] = u[2];
    depth[i] = rho;
    valid[i] = ok ? 1 : 0;
  }
}

__global__ __launch_bounds__(kBlock) void dyn_update_kernel(const double* __restrict__ map_points, const double* __restrict__ map_normals,
                                                            int64_t n_map, const double* __restrict__ pose, const double* __restrict__ reading,
                                                            int64_t m, const int32_t* __restrict__ rows, const int32_t* __restrict__ match_idx,
                                                            const double* __restrict__ match_chord, int64_t n_rows, DynParams prm,
                                                            double* __restrict__ prob, uint8_t* __restrict__ seen) {
  double T[16];
#pragma unroll
  for (int q = 0; q < 16; ++q) T[q] = pose[q];
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n_rows; i += stride)
    dyn_update_entry(prm, map_points, map_normals, n_map, T, reading, m, (int64_t)rows[i], (int64_t)match_idx[i], match_chord[i], prob, seen);
}

}  // namespace dc

using namespace dc;

extern "C" {

int dc_dyn_directions(const double* points, int64_t n, const double* pose, double max_range, double* dirs_out, double* depth_out,
                      uint8_t* valid_out, hipStream_t stream) {
  if (n == 0) return DC_OK;
  if (n < 0 || !points || !dirs_out || !depth_out || !valid_out || max_range != max_range) return DC_ERR_ARG;
  hipLaunchKernelGGL(dyn_directions_kernel, dim3(dyn_blocks(n)), dim3(kBlock), 0, stream, points, n, pose, max_range, dirs_out, depth_out,
                     valid_out);
  DC_HIP(hipGetLastError());
  return DC_OK;
}

int dc_dyn_update(const double* map_points, const double* map_normals, int64_t n_map, const double* pose, const double* reading, int64_t m,
                  const int32_t* rows, const int32_t* match_idx, const double* match_chord, int64_t n_rows, double chord_max, double epsilon_a,
                  double epsilon_d, double alpha, double beta, double threshold, double max_range, double* prob, uint8_t* seen_out,
                  hipStream_t stream) {
  const DynParams prm{chord_max, epsilon_a, epsilon_d, alpha, beta, threshold, max_range};
  if (n_rows < 0 || n_map < 0 || m < 0 || !dyn_params_ok(prm)) return DC_ERR_ARG;
  if (n_rows == 0) return DC_OK;
  if (n_map > (int64_t)0x7fffffff || m > (int64_t)0x7fffffff) return DC_ERR_UNSUPPORTED;
  if (!map_points || !map_normals || !pose || !reading || !rows || !match_idx || !match_chord || !prob) return DC_ERR_ARG;
  hipLaunchKernelGGL(dyn_update_kernel, dim3(dyn_blocks(n_rows)), dim3(kBlock), 0, stream, map_points, map_normals, n_map, pose, reading, m,
                     rows, match_idx, match_chord, n_rows, prm, prob, seen_out);
  DC_HIP(hipGetLastError());
  return DC_OK;
}

}  // extern "C"
