// Supervised training against a surveyed point cloud: the mean point-to-plane (or point-to-point) distance of the corrected, posed
// points of a sequence to their nearest survey points and its gradient to the model weights, the exponents and the poses, in ONE
// host call (dc_cloud_loss), all fp64 (DESIGN "Supervised training against a surveyed cloud").  The stream sees, in order:
//
//   1. cloud_points_kernel, one lane per point: x = R (vp + d' dir) + t with the statements of points_fwd_kernel (dc_points_dev.h),
//      written as fp64 rows into the workspace; a point outside `mask` becomes a NaN row, which the search answers with -1 / inf
//      without a walk.  Block 0 also writes the identity pose the search moves its queries by, and threshold = +inf.
//   2. dc_knn_grid_query (k = 1, r = max_dist) of those rows in the survey's persistent grid: the kernels of dc_knn_build, so the
//      index and the distance are its bits (smallest d^2, a tie to the lower index, d^2 < max_dist^2).
//   3. with inlier_ratio < 1, dc_quantile of the distances (+inf rows, the unmatched ones, do not count) -> threshold.
//   4. cloud_loss_kernel, one lane per point, 128 lanes per block, the blocks laid out per scan from scan_ptr (dc_scanloss.h: the
//      layout, the block's setup and partial row, the finishing).  A lane classifies its point (invalid / gated / trimmed / used),
//      forms the term and dl/dx (dc_cloudloss_math.h) and runs the point epilogue of dc_points_bwd (points_bwd_point).  The block's
//      partial row is [sum l, used, gated, trimmed, invalid, dw[P], de[P], d[R|t][12]].
//   5. cloud_loss_finish_kernel, one block: per scan, in scan order, four interleaved chains add the scan's block rows in block
//      order, the four sums are added in chain order; the scalar columns are then added over the scans in scan order.
//
// No atomics in 1, 4 and 5, and the search and the quantile are exact selections: the same inputs give the same bits whatever ran
// before.  No allocation, copy or synchronisation.
#include "dc_common.h"
#include "dc_device.h"
#include "dc_hostutil.h"
#include "dc_pointmath.h"
#include "dc_points_dev.h"
#include "dc_cloudloss_math.h"
#include "dc_scanloss.h"
#include "../../include/dc_hip.h"

namespace {

using namespace dc;

constexpr int kFixedCols = 5;                                 // sum l, used, gated, trimmed, invalid
constexpr int kMaxCols = kFixedCols + 2 * DC_MAX_MODEL_TERMS + 12;
constexpr int kFinishCols = 64;                               // one finishing lane per column, four chains
constexpr int kHeadDoubles = 32;                              // [0,16) the identity pose, [16] the threshold

template <typename T>
__global__ void __launch_bounds__(kLossBlock) cloud_points_kernel(PointInputs in, const uint8_t* __restrict__ mask,
                                                                  const int64_t* __restrict__ scan_ptr, int64_t n,
                                                                  double* __restrict__ head, double* __restrict__ x_out) {
  __shared__ double s_pose[12];
  const int tid = threadIdx.x;
  if (blockIdx.x == 0 && tid <= 16) head[tid] = tid == 16 ? INFINITY : ((tid & 3) == (tid >> 2) ? 1.0 : 0.0);
  int scan = -1;
  int64_t first = 0, last = 0;
  if (!block_scan(scan_ptr, in.n_scans, n, (int64_t)blockIdx.x, &scan, &first, &last)) return;
  if (in.poses && tid < 12) s_pose[tid] = in.poses[(int64_t)scan * 12 + tid];
  __syncthreads();
  const int64_t g = first + tid;
  if (g >= last) return;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  double x[3] = {nan, nan, nan};
  if (mask ? mask[g] != 0 : true) {
    PointInputs one = in;                                     // the block's scan as scan 0 of a one-scan sequence
    one.scan_id = nullptr;
    one.n_scans = 1;
    const PoseTile tile{in.poses ? s_pose : nullptr};
    ModelParams mp;
    load_model(in, mp);
    const PointRaw<T> raw = load_point_raw<T>(one, mp, g);
    double vp[3] = {0.0, 0.0, 0.0}, T12[12];
    if (in.vps) Row3<T, 3>::load((const T*)in.vps, g, vp, QParams{});
    load_pose(one, tile, 0, T12);
    posed_point<T>(mp, raw, vp, T12, x);
  }
  x_out[3 * g] = x[0];
  x_out[3 * g + 1] = x[1];
  x_out[3 * g + 2] = x[2];
}

template <typename T>
__global__ void __launch_bounds__(kLossBlock) cloud_loss_kernel(PointInputs in, const uint8_t* __restrict__ mask,
                                                                const int64_t* __restrict__ scan_ptr, int64_t n,
                                                                const double* __restrict__ xs, const int32_t* __restrict__ nn_idx,
                                                                const double* __restrict__ nn_dist, const double* __restrict__ map_points,
                                                                const double* __restrict__ map_normals, int64_t n_map,
                                                                const double* __restrict__ threshold, int plane, int squared, int want_e,
                                                                int32_t* __restrict__ idx_out, double* __restrict__ dist_out,
                                                                double* __restrict__ resid_out, double* __restrict__ partials) {
  __shared__ double s_pose[12];
  __shared__ double s_red[kLossWaves][kMaxCols];
  const int tid = threadIdx.x;
  int scan = -1;
  int64_t first = 0, last = 0;
  if (!block_scan(scan_ptr, in.n_scans, n, (int64_t)blockIdx.x, &scan, &first, &last)) return;   // the grid is an upper bound
  PointInputs one;
  ModelParams mp;
  int nt;
  scan_block_setup(in, scan, s_pose, one, mp, nt);
  const PoseTile tile{in.poses ? s_pose : nullptr};
  const double thr = *threshold;

  double acc[kFixedCols] = {0.0, 0.0, 0.0, 0.0, 0.0}, gw[DC_MAX_MODEL_TERMS], ge[DC_MAX_MODEL_TERMS], gT[6];
  zero_grads(gw, ge, gT);
  const int64_t g = first + tid;
  if (g < last) {
    int32_t hit = -1;
    double dist = INFINITY, resid = __longlong_as_double(0x7ff8000000000000ll);
    if (mask ? mask[g] != 0 : true) {
      const double x[3] = {xs[3 * g], xs[3 * g + 1], xs[3 * g + 2]};
      const int32_t j = nn_idx[g];
      const double d = nn_dist[g];
      if (!(isfinite(x[0]) && isfinite(x[1]) && isfinite(x[2]))) {
        acc[4] = 1.0;
      } else if (j < 0 || (int64_t)j >= n_map) {              // nothing within max_dist
        acc[2] = 1.0;
      } else if (d > thr) {                                   // beyond the inlier quantile of the matched distances
        acc[3] = 1.0;
      } else {
        const double y[3] = {map_points[3 * (int64_t)j], map_points[3 * (int64_t)j + 1], map_points[3 * (int64_t)j + 2]};
        double nv[3] = {0.0, 0.0, 0.0}, grad[3];
        if (plane) { nv[0] = map_normals[3 * (int64_t)j]; nv[1] = map_normals[3 * (int64_t)j + 1]; nv[2] = map_normals[3 * (int64_t)j + 2]; }
        acc[0] = cloud_loss_term(x, y, nv, plane != 0, squared != 0, &resid, grad);
        acc[1] = 1.0;
        hit = j;
        dist = d;
        const PointRaw<T> raw = load_point_raw<T>(one, mp, g);
        int s_unused;
        points_bwd_point<T>(one, tile, mp, g, raw, grad, gw, ge, gT, want_e != 0, true, &s_unused);
      }
    }
    if (idx_out) idx_out[g] = hit;
    if (dist_out) dist_out[g] = dist;
    if (resid_out) resid_out[g] = resid;
  }
  scan_block_store<kFixedCols>(acc, gw, ge, gT, nt, s_red, partials);
}

// out = [mean loss, used, gated, trimmed, invalid, threshold, dL/dw[P], dL/de[P], dL/d[R|t][12 S]], the gradients divided by M = used
__global__ void __launch_bounds__(kLossFinishBlock) cloud_loss_finish_kernel(const double* __restrict__ partials, int nt,
                                                                            const int64_t* __restrict__ scan_ptr, int64_t n,
                                                                            int n_scans, int64_t n_rows,
                                                                            const double* __restrict__ threshold,
                                                                            double* __restrict__ out) {
  scan_loss_finish<kFixedCols, kLossFinishBlock / kFinishCols, kFinishCols>(partials, nt, scan_ptr, n, n_scans, n_rows, 6, out);
  if (threadIdx.x == kFinishCols) out[5] = threshold ? *threshold : INFINITY;
}

struct CloudWs {
  double* head; void* qws; double* x; double* dist; int32_t* idx; double* partials; size_t total;
};
CloudWs carve(void* ws, int64_t n, int n_scans, int n_terms) {
  Carver cv(ws);
  CloudWs c;
  c.head = cv.take<double>(kHeadDoubles);
  c.qws = cv.take<char>(dc_quantile_workspace_bytes());
  c.x = cv.take<double>((size_t)n * 3);
  c.dist = cv.take<double>((size_t)n);
  c.idx = cv.take<int32_t>((size_t)n);
  c.partials = cv.take<double>((size_t)(max_blocks(n, n_scans) + 1) * (size_t)(kFixedCols + 2 * n_terms + 12));
  c.total = cv.off;
  return c;
}

}  // namespace

extern "C" {

size_t dc_cloud_loss_workspace_bytes(int64_t n, int n_scans, int n_terms) {
  if (n < 0 || n_scans < 0 || n_terms < 0 || n_terms > DC_MAX_MODEL_TERMS) return 0;
  return carve(nullptr, n, n_scans, n_terms).total;
}

int dc_cloud_loss(void* grid_ws, size_t grid_ws_bytes, int64_t n_query_max, const double* map_points, const double* map_normals,
                  int64_t n_map, const void* vps, const void* dirs, const void* depth, const void* inc, const uint8_t* lmask,
                  const uint8_t* mask, int dtype, int64_t n, const int64_t* scan_ptr, const double* poses, int n_scans, int model_kind,
                  int n_terms, const double* w, const double* e, int want_exponent, int plane, int squared, double max_dist,
                  double inlier_ratio, int32_t* idx_out, double* dist_out, double* resid_out, double* out, void* ws, size_t ws_bytes,
                  dcStream_t stream) {
  if (n_map < 1 || n < 0 || n_scans < 0 || !grid_ws || !map_points || (plane && !map_normals) || !out) return DC_ERR_ARG;
  PointInputs in;
  int64_t rows;
  const bool own_ok = max_dist > 0.0 && max_dist < INFINITY && inlier_ratio >= 0.0 && inlier_ratio <= 1.0 &&
                      n <= n_query_max;                       // the grid's query buffer holds n_query_max rows
  const int rc0 = scan_loss_args(vps, dirs, depth, inc, lmask, dtype, n, scan_ptr, poses, n_scans, model_kind, &n_terms, w, e, own_ok,
                                 &in, &rows);
  if (rc0 != DC_OK) return rc0;
  if (n > 0 && (!ws || ws_bytes < dc_cloud_loss_workspace_bytes(n, n_scans, n_terms))) return DC_ERR_WORKSPACE;
  const CloudWs c = carve(ws, n, n_scans, n_terms);
  const hipStream_t st = (hipStream_t)stream;
  const bool trim = inlier_ratio < 1.0;
  if (n > 0) {
    const dim3 grid((unsigned)rows), block(kLossBlock);
    // rows of x no scan covers (a scan_ptr that does not span [0, n]) must not reach the search or the quantile as stale memory
    DC_HIP(hipMemsetAsync(c.x, 0xff, (size_t)n * 3 * sizeof(double), st));
    if (dtype == DC_F32) cloud_points_kernel<float><<<grid, block, 0, st>>>(in, mask, scan_ptr, n, c.head, c.x);
    else cloud_points_kernel<double><<<grid, block, 0, st>>>(in, mask, scan_ptr, n, c.head, c.x);
    DC_HIP(hipGetLastError());
    int rc = dc_knn_grid_query(n_map, n_query_max, c.x, n, c.head, nullptr, 1, max_dist, c.idx, c.dist, grid_ws, grid_ws_bytes, stream);
    if (rc != DC_OK) return rc;
    if (trim) {
      rc = dc_quantile(c.dist, n, inlier_ratio, nullptr, c.head + 16, c.qws, dc_quantile_workspace_bytes(), stream);
      if (rc != DC_OK) return rc;
    }
    if (dtype == DC_F32)
      cloud_loss_kernel<float><<<grid, block, 0, st>>>(in, mask, scan_ptr, n, c.x, c.idx, c.dist, map_points, map_normals, n_map,
                                                       c.head + 16, plane, squared, want_exponent, idx_out, dist_out, resid_out,
                                                       c.partials);
    else
      cloud_loss_kernel<double><<<grid, block, 0, st>>>(in, mask, scan_ptr, n, c.x, c.idx, c.dist, map_points, map_normals, n_map,
                                                        c.head + 16, plane, squared, want_exponent, idx_out, dist_out, resid_out,
                                                        c.partials);
    DC_HIP(hipGetLastError());
  }
  cloud_loss_finish_kernel<<<1, kLossFinishBlock, 0, st>>>(c.partials, n_terms, scan_ptr, n, n_scans, rows,
                                                           (n > 0 && trim) ? c.head + 16 : nullptr, out);
  DC_HIP(hipGetLastError());
  return DC_OK;
}

}  // extern "C"
