// Depth bias against the mesh (gfx950): binned statistics of d - t over the true incidence angle and the normal equations of the
// supervised fit, from the per-ray outputs of dc_raycast_rays.  C ABI at the bottom (include/dc_hip.h); per-ray terms in
// dc_biasmath.h; algorithm and measurements in DESIGN "Depth bias against the mesh".
//
// Reduction (the rule of dc_icp_accumulate / dc_icp_finish: per block in a fixed order, then in block order; no atomics):
//   accumulate  a bounded grid (<= kBiasBlocksMax blocks of kBlock lanes) walks the rays with a grid stride.  Per trip every lane
//               stages its ray's bin and the eight bin terms in LDS; thread b then adds the block's entries of bin b in lane order
//               (every thread reads the same LDS address: a broadcast, no bank conflict) into registers it keeps over the trips.
//               The totals and the two systems are per-lane register sums over the trips, then dc::block_sum (fixed order).
//               Block k writes row k of the partials: [n_bins x DC_BIAS_BIN_COLS] bins, then kBiasFlat padded flat values.
//   finish      one block: thread q adds value q, q + kBlock, ... of the rows in block order and writes it to its place in `out`.
// The per-block result depends on the grid size only through which rays a block takes, and the grid is a function of n alone.
#include "dc_common.h"
#include "../../include/dc_hip.h"
#include "dc_device.h"
#include "dc_hostutil.h"
#include "dc_biasmath.h"

namespace dc {

constexpr int kBiasBlocksMax = 512;

static int bias_blocks(int64_t n) {
  const int64_t b = (n + kBlock - 1) / kBlock;
  return (int)(b < 1 ? 1 : (b > kBiasBlocksMax ? kBiasBlocksMax : b));
}

static size_t bias_row(int n_bins) { return (size_t)n_bins * DC_BIAS_BIN_COLS + kBiasFlat; }

template <typename T>
__global__ __launch_bounds__(kBlock) void bias_accumulate_kernel(const T* __restrict__ depth, const T* __restrict__ inc_est,
                                                                 const uint8_t* __restrict__ mask, const int32_t* __restrict__ face,
                                                                 const double* __restrict__ t_true, const double* __restrict__ inc_true,
                                                                 int64_t n, BiasParams prm, double* __restrict__ partials) {
  __shared__ int s_bin[kBlock];
  __shared__ double s_val[kBiasBinVals * kBlock];
  __shared__ double lds[kWavesPerBlock * kBiasFlat];
  const int tid = threadIdx.x;
  double flat[kBiasFlat];
#pragma unroll
  for (int q = 0; q < kBiasFlat; ++q) flat[q] = 0.0;
  double acc[DC_BIAS_BIN_COLS];
#pragma unroll
  for (int q = 0; q < DC_BIAS_BIN_COLS; ++q) acc[q] = 0.0;
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  // block-uniform trip count: every lane reaches the barriers
  for (int64_t base = (int64_t)blockIdx.x * kBlock; base < n; base += stride) {
    const int64_t i = base + tid;
    int bin = -1;
    double v[kBiasBinVals];
#pragma unroll
    for (int q = 0; q < kBiasBinVals; ++q) v[q] = 0.0;
    if (i < n) {
      const double g = inc_true[i];
      const double ge = inc_est ? (double)inc_est[i] : NAN;
      const BiasRay o = bias_ray(prm, (double)depth[i], ge, mask ? mask[i] != 0 : true, face[i], t_true[i], g);
      bias_flat_add(prm, o, g, ge, flat);
      bin = o.bin;
      if (bin >= 0) bias_bin_terms(o, v);
    }
    s_bin[tid] = bin;
#pragma unroll
    for (int q = 0; q < kBiasBinVals; ++q) s_val[q * kBlock + tid] = v[q];
    __syncthreads();
    if (tid < prm.n_bins) {
      for (int l = 0; l < kBlock; ++l) {
        if (s_bin[l] != tid) continue;
        acc[0] += 1.0;
#pragma unroll
        for (int q = 0; q < kBiasBinVals; ++q) acc[1 + q] += s_val[q * kBlock + l];
      }
    }
    __syncthreads();
  }
  double* row = partials + (size_t)blockIdx.x * ((size_t)prm.n_bins * DC_BIAS_BIN_COLS + kBiasFlat);
  if (tid < prm.n_bins) {
#pragma unroll
    for (int q = 0; q < DC_BIAS_BIN_COLS; ++q) row[tid * DC_BIAS_BIN_COLS + q] = acc[q];
  }
  block_sum<kBiasFlat>(flat, lds);
  if (tid == 0) {
#pragma unroll
    for (int q = 0; q < kBiasFlat; ++q) row[prm.n_bins * DC_BIAS_BIN_COLS + q] = flat[q];
  }
}

__global__ __launch_bounds__(kBlock) void bias_finish_kernel(const double* __restrict__ partials, int n_blocks, int n_bins, int n_terms,
                                                             double* __restrict__ out) {
  const int binned = n_bins * DC_BIAS_BIN_COLS, width = binned + kBiasFlat;
  for (int q = threadIdx.x; q < width; q += kBlock) {
    const int dst = q < binned ? DC_BIAS_TOTALS + q : bias_flat_to_out(q - binned, n_bins, n_terms);
    if (dst < 0) continue;
    double s = 0.0;
    for (int b = 0; b < n_blocks; ++b) s += partials[(size_t)b * width + q];
    out[dst] = s;
  }
}

}  // namespace dc

extern "C" {

size_t dc_bias_workspace_bytes(int n_bins, int n_terms) {
  if (n_bins < 1 || n_bins > DC_BIAS_MAX_BINS || n_terms < 1 || n_terms > DC_BIAS_MAX_TERMS) return 0;
  return sizeof(double) * dc::bias_row(n_bins) * dc::kBiasBlocksMax + 256;
}

int dc_bias_accumulate(const void* depth, const void* inc_est, int dtype, const uint8_t* mask, const int32_t* face, const double* t_true,
                       const double* inc_true, int64_t n, int model_kind, const double* exponent, int n_terms, int n_bins,
                       double max_residual, double* out, void* ws, size_t ws_bytes, dcStream_t stream_) {
  if (n < 0 || n_bins < 1 || n_bins > DC_BIAS_MAX_BINS || n_terms < 1 || n_terms > DC_BIAS_MAX_TERMS || !exponent || !out ||
      (model_kind != DC_MODEL_POLYNOMIAL && model_kind != DC_MODEL_SCALED_POLYNOMIAL) || max_residual != max_residual)
    return DC_ERR_ARG;
  if (n > 0 && (!depth || !face || !t_true || !inc_true)) return DC_ERR_ARG;
  if (dtype != DC_F32 && dtype != DC_F64) return DC_ERR_DTYPE;
  if (!ws || ws_bytes < dc_bias_workspace_bytes(n_bins, n_terms)) return DC_ERR_WORKSPACE;
  dc::BiasParams prm;
  prm.kind = model_kind;
  prm.n_terms = n_terms;
  prm.n_bins = n_bins;
  prm.max_residual = max_residual;
  for (int k = 0; k < DC_BIAS_MAX_TERMS; ++k) {
    prm.e[k] = k < n_terms ? exponent[k] : 0.0;
    if (!(prm.e[k] - prm.e[k] == 0.0)) return DC_ERR_ARG;        // NaN or infinite
  }
  hipStream_t stream = (hipStream_t)stream_;
  double* partials = (double*)(((uintptr_t)ws + 255) & ~(uintptr_t)255);
  const int blocks = dc::bias_blocks(n);
  if (dtype == DC_F32)
    hipLaunchKernelGGL(dc::bias_accumulate_kernel<float>, dim3((unsigned)blocks), dim3(dc::kBlock), 0, stream, (const float*)depth,
                       (const float*)inc_est, mask, face, t_true, inc_true, n, prm, partials);
  else
    hipLaunchKernelGGL(dc::bias_accumulate_kernel<double>, dim3((unsigned)blocks), dim3(dc::kBlock), 0, stream, (const double*)depth,
                       (const double*)inc_est, mask, face, t_true, inc_true, n, prm, partials);
  DC_HIP(hipGetLastError());
  hipLaunchKernelGGL(dc::bias_finish_kernel, dim3(1), dim3(dc::kBlock), 0, stream, partials, blocks, n_bins, n_terms, out);
  DC_HIP(hipGetLastError());
  return DC_OK;
}

}  // extern "C"
