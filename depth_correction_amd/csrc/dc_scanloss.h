// The scaffold of the supervised per-scan losses (dc_meshloss.hip, dc_cloudloss.hip): one lane per point, kLossBlock lanes per
// block, the blocks laid out per scan from scan_ptr (scan s owns ceil(n_s / 128) consecutive blocks, an empty scan none), so a
// block never straddles scans: the pose of its one scan is staged in LDS once and the block's pose sums are the sums of that scan.
// A block writes one partial row [FIXED scalar columns, dw[P], de[P], d[R|t][12]], summed in a fixed order: a shuffle tree within
// the wavefront, then wavefront 0 + wavefront 1 through LDS (scan_block_store).  The one-block finishing (scan_loss_finish) adds,
// per scan in scan order, the scan's rows on CHAINS interleaved chains (rows_lane_sum of dc_rowsum.h) and the chain sums in chain
// order; the scalar columns are then added over the scans in scan order.  No atomics anywhere.
#pragma once
#include "dc_common.h"
#include "dc_device.h"
#include "dc_points_dev.h"
#include "dc_rowsum.h"

namespace dc {

constexpr int kLossBlock = 128;
constexpr int kLossWaves = kLossBlock / kWave;
constexpr int kLossFinishBlock = 256;

// points [a, b) of scan s (scan_ptr == NULL: one scan holding every point), clipped to [0, n]
__device__ __forceinline__ void scan_range(const int64_t* __restrict__ scan_ptr, int s, int64_t n, int64_t* a, int64_t* b) {
  int64_t lo = scan_ptr ? scan_ptr[s] : 0, hi = scan_ptr ? scan_ptr[s + 1] : n;
  lo = lo < 0 ? 0 : (lo > n ? n : lo);
  hi = hi < lo ? lo : (hi > n ? n : hi);
  *a = lo;
  *b = hi;
}
__device__ __forceinline__ int64_t blocks_of(int64_t count) { return (count + kLossBlock - 1) / kLossBlock; }

// the scan of block `blk` and its points [first, last) (block-uniform); false for a block past the last scan
__device__ __forceinline__ bool block_scan(const int64_t* __restrict__ scan_ptr, int n_scans, int64_t n, int64_t blk, int* scan,
                                           int64_t* first, int64_t* last) {
  int64_t cum = 0;
  for (int s = 0; s < n_scans; ++s) {
    int64_t a, b;
    scan_range(scan_ptr, s, n, &a, &b);
    const int64_t nb = blocks_of(b - a);
    if (blk < cum + nb) {
      *scan = s;
      *first = a + (blk - cum) * kLossBlock;
      *last = b;
      return true;
    }
    cum += nb;
  }
  return false;
}

inline int64_t max_blocks(int64_t n, int n_scans) { return n / kLossBlock + n_scans; }      // >= sum_s ceil(n_s / 128)

// The block's setup, called by all its threads: the pose of `scan` staged in s_pose [12] (ends after the barrier that publishes
// it; PoseTile{in.poses ? s_pose : nullptr} reads it), `one` = the block's scan as scan 0 of a one-scan sequence, the model and
// its term count (0 without a model).
__device__ __forceinline__ void scan_block_setup(const PointInputs& in, int scan, double* s_pose, PointInputs& one, ModelParams& mp,
                                                 int& nt) {
  const int tid = threadIdx.x;
  if (in.poses && tid < 12) s_pose[tid] = in.poses[(int64_t)scan * 12 + tid];
  __syncthreads();
  one = in;
  one.scan_id = nullptr;
  one.n_scans = 1;
  load_model(in, mp);
  nt = in.model_kind == DC_MODEL_NONE ? 0 : in.n_terms;
}

__device__ __forceinline__ void zero_grads(double* gw, double* ge, double* gT) {
#pragma unroll
  for (int k = 0; k < DC_MAX_MODEL_TERMS; ++k) gw[k] = ge[k] = 0.0;
#pragma unroll
  for (int k = 0; k < 6; ++k) gT[k] = 0.0;
}

// block sums, column by column: a fixed shuffle tree per wavefront, then the wavefronts in order; row blockIdx.x of `partials`
template <int FIXED>
__device__ __forceinline__ void scan_block_store(const double* acc, const double* gw, const double* ge, const double* gT, int nt,
                                                 double (*s_red)[FIXED + 2 * DC_MAX_MODEL_TERMS + 12], double* __restrict__ partials) {
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
#pragma unroll
  for (int q = 0; q < FIXED; ++q) {
    const double s = wave_sum(acc[q]);
    if (lane == 0) s_red[wave][q] = s;
  }
#pragma unroll
  for (int k = 0; k < DC_MAX_MODEL_TERMS; ++k) {
    if (k < nt) {
      const double sw = wave_sum(gw[k]), se = wave_sum(ge[k]);
      if (lane == 0) {
        s_red[wave][FIXED + k] = sw;
        s_red[wave][FIXED + nt + k] = se;
      }
    }
  }
#pragma unroll
  for (int q = 0; q < 12; ++q) {
    // dL/d[R|t]_{a,b} = g_a [xl, 1]_b, the product rounded before it is added (no contraction into the sum)
    const double v = (q & 3) == 3 ? gT[q >> 2] : __dmul_rn(gT[q >> 2], gT[3 + (q & 3)]);
    const double s = wave_sum(v);
    if (lane == 0) s_red[wave][FIXED + 2 * nt + q] = s;
  }
  __syncthreads();
  const int ncols = FIXED + 2 * nt + 12;
  if (tid < ncols) {
    double t = s_red[0][tid];
#pragma unroll
    for (int wv = 1; wv < kLossWaves; ++wv) t += s_red[wv][tid];
    partials[(int64_t)blockIdx.x * ncols + tid] = t;
  }
}

// The body of a finishing kernel of one block of kLossFinishBlock = CHAINS x COLS threads (COLS >= the columns of a row).  out =
// [mean loss, the other FIXED - 1 scalar columns, ..., dL/dw[P] and dL/de[P] from o_term on, dL/d[R|t][12 S]], the gradients
// divided by M = used (column 1); M = 0 gives a NaN loss (the mean of nothing) and zero gradients.
template <int FIXED, int CHAINS, int COLS>
__device__ __forceinline__ void scan_loss_finish(const double* __restrict__ partials, int nt, const int64_t* __restrict__ scan_ptr,
                                                 int64_t n, int n_scans, int64_t n_rows, int o_term, double* __restrict__ out) {
  static_assert(CHAINS * COLS == kLossFinishBlock && FIXED + 2 * DC_MAX_MODEL_TERMS + 12 <= COLS, "one finishing lane per column");
  __shared__ double s_red[CHAINS][COLS];
  __shared__ double s_count;
  const int tid = threadIdx.x, col = tid & (COLS - 1), chain = tid / COLS;
  const int ncols = FIXED + 2 * nt + 12, n_scalar = FIXED + 2 * nt;
  const int o_grad = o_term + 2 * nt;                         // first pose gradient in `out`
  double total = 0.0;                                         // chain 0, scalar columns: the sum over the scans so far
  int64_t blk0 = 0;
  for (int s = 0; s < n_scans; ++s) {
    int64_t a, b;
    scan_range(scan_ptr, s, n, &a, &b);
    int64_t nb = blocks_of(b - a);
    if (blk0 + nb > n_rows) nb = n_rows - blk0;               // never past the rows the loss kernel had blocks for
    s_red[chain][col] = col < ncols ? rows_lane_sum<CHAINS>(partials + blk0 * ncols, nb, ncols, col, chain) : 0.0;
    __syncthreads();
    if (chain == 0 && col < ncols) {
      double t = s_red[0][col];
#pragma unroll
      for (int ch = 1; ch < CHAINS; ++ch) t += s_red[ch][col];
      if (col < n_scalar) total += t;
      else out[o_grad + (int64_t)s * 12 + (col - n_scalar)] = t;
    }
    __syncthreads();
    blk0 += nb;
  }
  if (tid == 1) s_count = total;                              // M = used
  __syncthreads();
  const double M = s_count;
  if (chain == 0 && col < n_scalar) {
    if (col == 0) out[0] = M > 0.0 ? total / M : __longlong_as_double(0x7ff8000000000000ll);
    else if (col < FIXED) out[col] = total;
    else out[o_term + (col - FIXED)] = M > 0.0 ? total / M : 0.0;
  }
  for (int64_t i = tid; i < 12 * (int64_t)n_scans; i += kLossFinishBlock) {
    const double v = out[o_grad + i];                         // written by this block before the barriers above
    out[o_grad + i] = M > 0.0 ? v / M : 0.0;
  }
}

// What dc_mesh_loss and dc_cloud_loss check alike, after their own pointer and count checks: the dtype, then (DC_ERR_ARG)
// `own_ok` -- the caller's conditions on its own options, which rank after the dtype -- the model kind and its term counts, inc,
// n_scans and scan_ptr, then the row limit (DC_ERR_UNSUPPORTED).  *n_terms becomes 0 without a model; `in` is filled, *rows =
// max_blocks.
inline int scan_loss_args(const void* vps, const void* dirs, const void* depth, const void* inc, const uint8_t* lmask, int dtype,
                          int64_t n, const int64_t* scan_ptr, const double* poses, int n_scans, int model_kind, int* n_terms,
                          const double* w, const double* e, bool own_ok, PointInputs* in, int64_t* rows) {
  if (dtype != DC_F32 && dtype != DC_F64) return DC_ERR_DTYPE;
  if (!own_ok) return DC_ERR_ARG;
  if (model_kind < DC_MODEL_NONE || model_kind > DC_MODEL_LAST) return DC_ERR_ARG;
  if (model_kind != DC_MODEL_NONE) {
    if (*n_terms < 1 || *n_terms > DC_MAX_MODEL_TERMS || !w || !e || (n > 0 && !inc)) return DC_ERR_ARG;
    if (model_kind == DC_MODEL_LINEAR && *n_terms != 3) return DC_ERR_ARG;
    if ((model_kind == DC_MODEL_INVCOS || model_kind == DC_MODEL_SCALED_INVCOS) && *n_terms != 1) return DC_ERR_ARG;
  } else {
    *n_terms = 0;
  }
  if (n > 0 && (n_scans < 1 || !dirs || !depth)) return DC_ERR_ARG;
  if (n_scans > 1 && !scan_ptr) return DC_ERR_ARG;
  *rows = max_blocks(n, n_scans);
  if (*rows > 0x7fffffff) return DC_ERR_UNSUPPORTED;
  in->vps = vps; in->dirs = dirs; in->depth = depth; in->inc = inc; in->lmask = lmask; in->scan_id = nullptr;
  in->poses = poses; in->w = w; in->e = e; in->model_kind = model_kind; in->n_terms = *n_terms; in->n_scans = n_scans;
  return DC_OK;
}

}  // namespace dc
