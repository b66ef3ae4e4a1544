// Scan-to-TSDF registration (gfx950): a scan is registered against the fused sparse volume itself (DESIGN "Scan-to-TSDF registration";
// the rules: dc_tsdf_track_math.h, whose functions the kernels inline).  C ABI at the bottom; see include/dc_hip.h.
//
// One iteration on the device, with nothing returned to the host in between and no nearest-neighbour search:
//   dc_tsdf_sparse_sample     one lane per point: the point moved by the device-side estimate, the eight voxels around it found through
//                             the block table (binary search, once per block change of the lane), value, gradient, |value|, flag;
//   dc_quantile               (dc_filters.hip) the trimmed threshold over the finite distances, which are those of the valid points;
//   dc_tsdf_icp_accumulate    the pair rule, r = phi, J = [x cross grad, grad], fp64 block partials in the shape of dc_icp_accumulate;
//   dc_icp_finish             (dc_slam.hip) unchanged: the partials in block order, the 6 x 6 solve, the update, the checks.
// A registration whose status word is set turns every launch into an early exit.  No atomics, no allocation, no synchronisation;
// reductions run in a fixed order: bit-reproducible.
#include "dc_common.h"
#include "../../include/dc_hip.h"
#include "dc_device.h"
#include "dc_hostutil.h"
#include "dc_tsdf_track_math.h"

namespace dc {

__global__ __launch_bounds__(kBlock) void tsdf_sparse_sample_kernel(const uint64_t* __restrict__ keys, const int32_t* __restrict__ slots,
                                                                    const int64_t* __restrict__ n_blocks, int64_t capacity,
                                                                    const int64_t* __restrict__ sum, const int32_t* __restrict__ count,
                                                                    TsdfGrid g, double tau, int min_count,
                                                                    const double* __restrict__ points, int64_t m,
                                                                    const double* __restrict__ pose, const int32_t* __restrict__ stop,
                                                                    double* __restrict__ x_out, double* __restrict__ value_out,
                                                                    double* __restrict__ grad_out, double* __restrict__ dist_out,
                                                                    uint8_t* __restrict__ flag_out) {
  if (stop && *stop != 0) return;                     // the registration has ended: the outputs stay as they are (grid-uniform)
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= m) return;
  const double p[3] = {points[i * 3], points[i * 3 + 1], points[i * 3 + 2]};
  double x[3] = {p[0], p[1], p[2]};
  if (pose) {
    double T[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) T[q] = pose[q];
    move_point(T, p, x);
  }
  const int64_t nb0 = *n_blocks, nb = nb0 < 0 ? 0 : (nb0 > capacity ? capacity : nb0);
  const TsdfSample s = tsdf_sample_point(x, g, tau, min_count, keys, slots, nb, capacity, sum, count);
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    x_out[i * 3 + a] = x[a];
    grad_out[i * 3 + a] = s.grad[a];
  }
  value_out[i] = s.phi;
  dist_out[i] = s.dist;
  flag_out[i] = (uint8_t)s.flag;
}

// The shape of icp_accumulate_kernel (dc_slam.hip): grid stride over the points, 30 fp64 sums a lane, block_sum, one row a block.
__global__ __launch_bounds__(kBlock) void tsdf_icp_accumulate_kernel(const double* __restrict__ x, const double* __restrict__ value,
                                                                     const double* __restrict__ grad, const double* __restrict__ dist,
                                                                     const uint8_t* __restrict__ flag, int64_t m,
                                                                     const double* __restrict__ threshold, double max_residual,
                                                                     const int32_t* __restrict__ status, double* __restrict__ partials,
                                                                     uint8_t* __restrict__ kept_out) {
  using Row = IcpRow<6>;
  __shared__ double lds[kWavesPerBlock * Row::kWidth];
  if (status[0] != 0) return;                         // the registration has ended: nothing to do (block-uniform)
  const double thr = *threshold;
  double v[Row::kWidth];
#pragma unroll
  for (int q = 0; q < Row::kWidth; ++q) v[q] = 0.0;
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < m; i += stride) {
    const bool keep = tsdf_track_keep(flag[i], dist[i], thr, max_residual);
    if (kept_out) kept_out[i] = keep ? 1 : 0;
    if (!keep) continue;
    const double xi[3] = {x[i * 3], x[i * 3 + 1], x[i * 3 + 2]}, gi[3] = {grad[i * 3], grad[i * 3 + 1], grad[i * 3 + 2]};
    tsdf_track_add(xi, value[i], gi, v);
    v[Row::kUsed] += 1.0;
  }
  block_sum<Row::kWidth>(v, lds);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int q = 0; q < Row::kWidth; ++q) partials[(int64_t)blockIdx.x * Row::kWidth + q] = v[q];
  }
}

}  // namespace dc

using namespace dc;

extern "C" {

int dc_tsdf_sparse_sample(const uint64_t* keys, const int32_t* slots, const int64_t* n_blocks, int64_t capacity, const int64_t* sum,
                          const int32_t* count, double ox, double oy, double oz, double voxel, double trunc, int min_count, const double* points,
                          int64_t m, const double* pose, const int32_t* stop, double* x_out, double* value_out, double* grad_out,
                          double* dist_out, uint8_t* flag_out, hipStream_t stream) {
  const TsdfGrid g{{ox, oy, oz}, voxel, {0, 0, 0}};
  if (!tsdf_lattice_ok(g) || !(trunc > 0.0) || !isfinite(trunc) || min_count < 1 || m < 0 || capacity < 1 || capacity >= ((int64_t)1 << 22))
    return DC_ERR_ARG;
  if (m == 0) return DC_OK;
  if (!keys || !slots || !n_blocks || !sum || !count || !points || !x_out || !value_out || !grad_out || !dist_out || !flag_out) return DC_ERR_ARG;
  const int64_t blocks = (m + kBlock - 1) / kBlock;
  if (blocks > 0x7fffffff) return DC_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(tsdf_sparse_sample_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, stream, keys, slots, n_blocks, capacity, sum, count, g,
                     trunc, min_count, points, m, pose, stop, x_out, value_out, grad_out, dist_out, flag_out);
  DC_HIP(hipGetLastError());
  return DC_OK;
}

int dc_tsdf_icp_accumulate(const double* x, const double* value, const double* grad, const double* dist, const uint8_t* flag, int64_t m,
                           const double* threshold, double max_residual, const double* state, const int32_t* status, double* partials,
                           int n_blocks, uint8_t* kept_out, hipStream_t stream) {
  if (m < 0 || !threshold || !state || !status || !partials || isnan(max_residual)) return DC_ERR_ARG;
  if (m > 0 && (!x || !value || !grad || !dist || !flag)) return DC_ERR_ARG;
  if (n_blocks != dc_icp_blocks(m)) return DC_ERR_WORKSPACE;
  hipLaunchKernelGGL(tsdf_icp_accumulate_kernel, dim3((unsigned)n_blocks), dim3(kBlock), 0, stream, x, value, grad, dist, flag, m, threshold,
                     max_residual, status, partials, kept_out);
  DC_HIP(hipGetLastError());
  return DC_OK;
}

}  // extern "C"
