// Survey registration: trimmed closed-form ICP of a point cloud against a surveyed cloud, resident on the device (DESIGN "Survey
// registration"; what utils.absolute_orientation and icp_alignment of scripts/map_bias_removal do on the host).  dc_survey_align
// queues, for every iteration, on the stream:
//
//   1. dc_knn_grid_query (k = 1, r = max_dist) of the ORIGINAL query rows under the estimate in the state (a device pose), in the
//      survey's persistent grid: its bits (smallest d^2, a tie to the lower index, a non-finite row -1 / +inf).
//   2. with inlier_ratio < 1, dc_quantile of the matched distances -> the threshold in the state (+inf otherwise).
//   3. align_accumulate_kernel: a point is kept when idx >= 0 and d <= threshold; the 17 moments of the kept pairs about the two fixed
//      origins, summed per wavefront by a shuffle tree, per block through LDS, one row of partials per block; the grid is capped at
//      kAlignBlocksMax blocks and strides over the rest.
//   4. align_finish_kernel, one block: the partials in a fixed order (dc_rowsum.h), the closed-form fit (dc_align_math.h), the
//      estimate, the history row and the status word.
//
// The status word is the `stop` word of 1 and 2 and is tested by 3 and 4: once it is set every later launch returns at once, so
// the host queues all iterations and reads the result once.  No atomics, fixed summation orders, exact selections: the same
// inputs give the same bits whatever ran before.  No allocation, copy or synchronisation.
#include "dc_common.h"
#include "../../include/dc_hip.h"
#include "dc_device.h"
#include "dc_hostutil.h"
#include "dc_rowsum.h"
#include "dc_align_math.h"

namespace dc {

static int align_blocks(int64_t n) {
  const int64_t b = (n + kBlock - 1) / kBlock;
  return (int)(b < 1 ? 1 : (b > kAlignBlocksMax ? kAlignBlocksMax : b));
}

// state <- the prior as the estimate and as the prior, threshold = +inf, the rest NaN; status <- 0; history [n_rows, 5] <- NaN
__global__ void align_init_kernel(const double* __restrict__ prior, double* __restrict__ state, int32_t* __restrict__ status,
                                  double* __restrict__ history, int64_t n_hist) {
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < DC_ALIGN_STATE_COUNT) {
    double v = nan;
    if (t < 16) v = prior ? prior[t] : ((t & 3) == (t >> 2) ? 1.0 : 0.0);
    else if (t < 32) v = prior ? prior[t - 16] : (((t - 16) & 3) == ((t - 16) >> 2) ? 1.0 : 0.0);
    else if (t == DC_ALIGN_STATE_THRESHOLD) v = INFINITY;
    state[t] = v;
  }
  if (t < 4) status[t] = 0;
  for (int64_t i = t; i < n_hist; i += (int64_t)gridDim.x * blockDim.x) history[i] = nan;
}

__global__ __launch_bounds__(kBlock) void align_accumulate_kernel(const double* __restrict__ query, int64_t n,
                                                                  const double* __restrict__ map_points, int64_t n_map,
                                                                  const int32_t* __restrict__ idx, const double* __restrict__ dist,
                                                                  const double* __restrict__ threshold, const double* __restrict__ origins,
                                                                  const int32_t* __restrict__ status, double* __restrict__ partials,
                                                                  uint8_t* __restrict__ kept_out) {
  __shared__ double lds[kWavesPerBlock * DC_ALIGN_PARTIALS];
  if (status && status[0] != 0) return;             // the registration has ended: nothing to do (block-uniform)
  const double thr = *threshold;
  double o[6];
#pragma unroll
  for (int q = 0; q < 6; ++q) o[q] = origins[q];
  double v[DC_ALIGN_PARTIALS];
#pragma unroll
  for (int q = 0; q < DC_ALIGN_PARTIALS; ++q) v[q] = 0.0;
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
    const int32_t id = idx[i];
    const double d = dist[i];
    const bool keep = id >= 0 && (int64_t)id < n_map && d <= thr;      // a NaN threshold (nothing matched) keeps nothing
    if (kept_out) kept_out[i] = keep ? 1 : 0;
    if (!keep) continue;
    const double p[3] = {query[i * 3] - o[0], query[i * 3 + 1] - o[1], query[i * 3 + 2] - o[2]};
    const double* yr = map_points + (int64_t)id * 3;
    const double y[3] = {yr[0] - o[3], yr[1] - o[4], yr[2] - o[5]};
    v[0] += 1.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      v[1 + a] += p[a];
      v[4 + a] += y[a];
#pragma unroll
      for (int b = 0; b < 3; ++b) v[7 + a * 3 + b] += p[a] * y[b];
    }
    v[16] += d * d;
  }
  block_sum<DC_ALIGN_PARTIALS>(v, lds);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int q = 0; q < DC_ALIGN_PARTIALS; ++q) partials[(int64_t)blockIdx.x * DC_ALIGN_PARTIALS + q] = v[q];
  }
}

// One block: threads 8 q .. 8 q + 7 sum value q over the blocks b = l, l + 8, ... in order, thread q adds the eight sums of value
// q in order (rows_block_totals); thread 0 then solves and updates (align_finish_tail).
__global__ __launch_bounds__(kBlock) void align_finish_kernel(const double* __restrict__ partials, int n_blocks,
                                                              const double* __restrict__ origins, AlignParams prm,
                                                              double* __restrict__ state, int32_t* __restrict__ status,
                                                              double* __restrict__ history, int n_hist_rows) {
  __shared__ double s_part[DC_ALIGN_PARTIALS * kRowSumLanes];
  __shared__ double s_tot[DC_ALIGN_PARTIALS];
  if (status[0] != 0) return;
  rows_block_totals<DC_ALIGN_PARTIALS, kRowSumLanes>(partials, n_blocks, s_part, s_tot);
  if (threadIdx.x != 0) return;
  double o[6];
  for (int q = 0; q < 6; ++q) o[q] = origins[q];
  const int row = status[1];                        // iterations done so far = the row this one writes
  double* hist = (history && row >= 0 && row < n_hist_rows) ? history + (int64_t)row * DC_ALIGN_HISTORY_COLS : nullptr;
  align_finish_tail(s_tot, o, prm, state, status, hist);
}

struct AlignWs {
  void* qws; double* dist; int32_t* idx; double* partials; size_t total;
};
static AlignWs align_carve(void* ws, int64_t n) {
  Carver cv(ws);
  AlignWs c;
  c.qws = cv.take<char>(dc_quantile_workspace_bytes());
  c.dist = cv.take<double>((size_t)n);
  c.idx = cv.take<int32_t>((size_t)n);
  c.partials = cv.take<double>((size_t)kAlignBlocksMax * DC_ALIGN_PARTIALS);
  c.total = cv.off;
  return c;
}

}  // namespace dc

using namespace dc;

extern "C" {

int dc_align_blocks(int64_t n) { return n < 0 ? 0 : align_blocks(n); }

int dc_align_init(const double* prior, double* state, int32_t* status, double* history, int n_iters, hipStream_t stream) {
  if (!state || !status || n_iters < 0 || (n_iters > 0 && !history)) return DC_ERR_ARG;
  const int64_t n_hist = history ? (int64_t)n_iters * DC_ALIGN_HISTORY_COLS : 0;
  hipLaunchKernelGGL(align_init_kernel, dim3(1), dim3(kBlock), 0, stream, prior, state, status, history, n_hist);
  DC_HIP(hipGetLastError());
  return DC_OK;
}

int dc_align_accumulate(const double* query, int64_t n, const double* map_points, int64_t n_map, const int32_t* idx, const double* dist,
                        const double* threshold, const double* origins, const int32_t* status, double* partials, int n_blocks,
                        uint8_t* kept_out, hipStream_t stream) {
  if (n < 1 || n_map < 1 || !query || !map_points || !idx || !dist || !threshold || !origins || !partials) return DC_ERR_ARG;
  if (n > 0x7fffffff) return DC_ERR_UNSUPPORTED;
  if (n_blocks != align_blocks(n)) return DC_ERR_WORKSPACE;
  hipLaunchKernelGGL(align_accumulate_kernel, dim3((unsigned)n_blocks), dim3(kBlock), 0, stream, query, n, map_points, n_map, idx, dist,
                     threshold, origins, status, partials, kept_out);
  DC_HIP(hipGetLastError());
  return DC_OK;
}

int dc_align_finish(const double* partials, int n_blocks, const double* origins, double min_rot, double min_trans, int min_pairs,
                    int max_iters, double* state, int32_t* status, double* history, int n_history_rows, hipStream_t stream) {
  if (!partials || !origins || !state || !status || n_blocks < 1 || n_blocks > kAlignBlocksMax) return DC_ERR_ARG;
  if (!(min_rot >= 0.0) || !(min_trans >= 0.0) || min_pairs < 3 || max_iters < 1 || n_history_rows < 0) return DC_ERR_ARG;
  const AlignParams prm{min_rot, min_trans, min_pairs, max_iters};
  hipLaunchKernelGGL(align_finish_kernel, dim3(1), dim3(kBlock), 0, stream, partials, n_blocks, origins, prm, state, status, history,
                     history ? n_history_rows : 0);
  DC_HIP(hipGetLastError());
  return DC_OK;
}

size_t dc_survey_align_workspace_bytes(int64_t n) {
  if (n < 0) return 0;
  return align_carve(nullptr, n).total;
}

int dc_survey_align(void* grid_ws, size_t grid_ws_bytes, int64_t n_query_max, const double* map_points, int64_t n_map, const double* query,
                    int64_t n, const double* prior, double inlier_ratio, double max_dist, int n_iters, double min_rot, double min_trans,
                    int min_pairs, const double* origins, double* state, int32_t* status, double* history, void* ws, size_t ws_bytes,
                    hipStream_t stream) {
  if (!grid_ws || !map_points || n_map < 1 || !query || n < 1 || !origins || !state || !status || !history || !ws) return DC_ERR_ARG;
  if (!(max_dist > 0.0) || !(max_dist < INFINITY)) return DC_ERR_ARG;
  if (!(inlier_ratio > 0.0 && inlier_ratio <= 1.0)) return DC_ERR_ARG;
  if (n_iters < 1 || !(min_rot >= 0.0) || !(min_trans >= 0.0) || min_pairs < 3) return DC_ERR_ARG;
  if (n > n_query_max) return DC_ERR_ARG;                     // the grid's query buffer holds n_query_max rows
  if (n > 0x7fffffff) return DC_ERR_UNSUPPORTED;
  if (ws_bytes < dc_survey_align_workspace_bytes(n)) return DC_ERR_WORKSPACE;
  const AlignWs c = align_carve(ws, n);
  const int nb = align_blocks(n);
  const bool trim = inlier_ratio < 1.0;
  double* pose = state + DC_ALIGN_STATE_POSE;
  double* thr = state + DC_ALIGN_STATE_THRESHOLD;
  int rc = dc_align_init(prior, state, status, history, n_iters, stream);
  if (rc != DC_OK) return rc;
  for (int it = 0; it < n_iters; ++it) {
    rc = dc_knn_grid_query(n_map, n_query_max, query, n, pose, status, 1, max_dist, c.idx, c.dist, grid_ws, grid_ws_bytes, stream);
    if (rc != DC_OK) return rc;
    if (trim) {
      rc = dc_quantile(c.dist, n, inlier_ratio, status, thr, c.qws, dc_quantile_workspace_bytes(), stream);
      if (rc != DC_OK) return rc;
    }
    rc = dc_align_accumulate(query, n, map_points, n_map, c.idx, c.dist, thr, origins, status, c.partials, nb, nullptr, stream);
    if (rc != DC_OK) return rc;
    rc = dc_align_finish(c.partials, nb, origins, min_rot, min_trans, min_pairs, n_iters, state, status, history, n_iters, stream);
    if (rc != DC_OK) return rc;
  }
  return DC_OK;
}

}  // extern "C"
