// Scan-to-map point-to-plane ICP of the SLAM evaluation (gfx950): a restatement of the reference's mapper configuration
// (config/slam/icp.yaml, input_filters.yaml, launch/slam.launch; eval.py:214-290 runs it through ROS), not of libpointmatcher.
// C ABI at the bottom; see include/dc_hip.h.  The algorithm, its deviations and its measured cost are in DESIGN "SLAM evaluation".
//
// One ICP iteration on the device, with nothing returned to the host in between:
//   dc_knn_grid_query  (dc_knn.hip)    reading points moved by the device-side estimate, k-NN in the map's grid built earlier;
//   dc_quantile        (dc_filters.hip) the trimmed threshold: dc_nn1_corr's radix select over the matched (finite) distances of the
//                                       M x knn table;
//   dc_icp_accumulate                   both pair filters, residuals, fp64 block partials of JtJ (21), Jtr (6), pairs, sum r^2,
//                                       points with a kept pair;
//   dc_icp_finish                       one block: the partials in block order, the 6 x 6 Cholesky solve, the pose update, the
//                                       checks and the status word.
// A registration whose status word is set turns every later launch of these four into an early exit, so the host can queue
// several iterations and read the status once.  Reductions run in a fixed order and use no atomics: bit-reproducible.
//
// The sweep-aware iteration (DESIGN "Sweep-aware registration") estimates the twist of a moving sweep with the pose: dc_deskew
// (dc_sweep.hip) by the device-side twist in front, dc_icp_ct_accumulate / dc_icp_ct_finish in the places of the last two: the
// same kernel bodies and solver for 12 unknowns (icp_accumulate_body, icp_finish_totals, icp_solve), each tail its own.
#include "dc_common.h"
#include "../../include/dc_hip.h"
#include "dc_device.h"
#include "dc_hostutil.h"
#include "dc_rowsum.h"
#include "dc_slam_math.h"
#include "dc_sweepmath.h"

namespace dc {

static int icp_blocks(int64_t m) {
  const int64_t b = (m + kBlock - 1) / kBlock;
  return (int)(b < 1 ? 1 : (b > kIcpBlocksMax ? kIcpBlocksMax : b));
}

__global__ void icp_init_kernel(const double* __restrict__ prior, double* __restrict__ state, int32_t* __restrict__ status) {
  const int t = threadIdx.x;
  if (t < 16) { state[DC_ICP_STATE_POSE + t] = prior[t]; state[DC_ICP_STATE_PRIOR + t] = prior[t]; }
  else if (t < 16 + (DC_ICP_STATE_COUNT - 32)) state[32 + (t - 16)] = 0.0;
  if (t < 4) status[t] = 0;
}

// The pair kernels' body for NU = 6 or 12 unknowns: both pair filters, the residual, the Jacobian row and the block's partial row
// IcpRow<NU> (the triangle of J J^T row by row, J r, pairs, sum r^2, points with a kept pair).  `pts` / `nrm` are the points the
// pairs were matched with: the reading for NU = 6; for NU = 12 the reading de-skewed by the twist in `ct`, and `raw` / `tau` the
// reading itself with its sweep times (null and unread for NU = 6).  A lane of the 12-unknown kernel carries its 93 sums as fp64
// accumulators (186 registers): the block of four wavefronts runs one per SIMD, where a lane may use the whole 512-entry file, so
// they stay in registers (no private segment; DESIGN has the counts).
template <int NU>
__device__ __forceinline__ void icp_accumulate_body(const double* __restrict__ pts, const double* __restrict__ nrm,
                                                    const double* __restrict__ raw, const double* __restrict__ tau, int64_t m,
                                                    const double* __restrict__ map_points, const double* __restrict__ map_normals,
                                                    const int32_t* __restrict__ idx, const double* __restrict__ dist, int knn,
                                                    const double* __restrict__ threshold, double cos_min,
                                                    const double* __restrict__ state, const double* __restrict__ ct,
                                                    const int32_t* __restrict__ status, double* __restrict__ partials,
                                                    uint8_t* __restrict__ kept_out) {
  using Row = IcpRow<NU>;
  __shared__ double lds[kWavesPerBlock * Row::kWidth];
  if (status[0] != 0) return;                       // the registration has ended: nothing to do (block-uniform)
  double T[16];
#pragma unroll
  for (int q = 0; q < 16; ++q) T[q] = state[DC_ICP_STATE_POSE + q];
  double w0 = 0.0, w1 = 0.0, w2 = 0.0;
  if constexpr (NU == 12) { w0 = ct[DC_ICP_CT_STATE_TWIST + 3]; w1 = ct[DC_ICP_CT_STATE_TWIST + 4]; w2 = ct[DC_ICP_CT_STATE_TWIST + 5]; }
  const double thr = *threshold;
  double v[Row::kWidth];
#pragma unroll
  for (int q = 0; q < Row::kWidth; ++q) v[q] = 0.0;
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < m; i += stride) {
    const double p[3] = {pts[i * 3], pts[i * 3 + 1], pts[i * 3 + 2]};
    const double pn[3] = {nrm[i * 3], nrm[i * 3 + 1], nrm[i * 3 + 2]};
    double x[3];
    move_point(T, p, x);
    double nr[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) nr[r] = T[r * 4] * pn[0] + T[r * 4 + 1] * pn[1] + T[r * 4 + 2] * pn[2];
    // NU = 12: u = Exp(tau w) p_i with dc_deskew's arithmetic, and the coefficients of J_l(tau w)
    double tg = 0.0, u[3] = {0.0, 0.0, 0.0};
    SweepRot rot{};
    SweepJl jl{};
    if constexpr (NU == 12) {
      tg = tau[i];
      rot = sweep_rot(tg, w0, w1, w2);
      jl = sweep_left_jacobian(rot);
      sweep_rotate(rot, raw[i * 3], raw[i * 3 + 1], raw[i * 3 + 2], u);
    }
    bool any = false;
    for (int j = 0; j < knn; ++j) {
      const int64_t e = i * knn + j;
      const int32_t id = idx[e];
      bool keep = id >= 0 && dist[e] <= thr;        // TrimmedDistOutlierFilter (NaN threshold keeps nothing)
      double n[3] = {0.0, 0.0, 0.0}, y[3] = {0.0, 0.0, 0.0};
      if (keep) {
        n[0] = map_normals[(int64_t)id * 3]; n[1] = map_normals[(int64_t)id * 3 + 1]; n[2] = map_normals[(int64_t)id * 3 + 2];
        y[0] = map_points[(int64_t)id * 3]; y[1] = map_points[(int64_t)id * 3 + 1]; y[2] = map_points[(int64_t)id * 3 + 2];
        keep = fabs(nr[0] * n[0] + nr[1] * n[1] + nr[2] * n[2]) >= cos_min;     // SurfaceNormalOutlierFilter
      }
      if (kept_out) kept_out[e] = keep ? 1 : 0;
      if (!keep) continue;
      any = true;
      const double r = n[0] * (x[0] - y[0]) + n[1] * (x[1] - y[1]) + n[2] * (x[2] - y[2]);
      double J[NU] = {x[1] * n[2] - x[2] * n[1], x[2] * n[0] - x[0] * n[2], x[0] * n[1] - x[1] * n[0], n[0], n[1], n[2]};
      if constexpr (NU == 12) {
        const double ns0 = T[0] * n[0] + T[4] * n[1] + T[8] * n[2], ns1 = T[1] * n[0] + T[5] * n[1] + T[9] * n[2],
                     ns2 = T[2] * n[0] + T[6] * n[1] + T[10] * n[2];                 // n_s = R^T n_map
        double jw[3];
        sweep_jl_transposed(rot, jl, u[1] * ns2 - u[2] * ns1, u[2] * ns0 - u[0] * ns2, u[0] * ns1 - u[1] * ns0, jw);
        J[6] = tg * ns0; J[7] = tg * ns1; J[8] = tg * ns2; J[9] = tg * jw[0]; J[10] = tg * jw[1]; J[11] = tg * jw[2];
      }
      int q = 0;
#pragma unroll
      for (int a = 0; a < NU; ++a)
#pragma unroll
        for (int b = a; b < NU; ++b) v[q++] += J[a] * J[b];
#pragma unroll
      for (int a = 0; a < NU; ++a) v[Row::kJtr + a] += J[a] * r;
      v[Row::kPairs] += 1.0;
      v[Row::kSse] += r * r;
    }
    if (any) v[Row::kUsed] += 1.0;
  }
  block_sum<Row::kWidth>(v, lds);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int q = 0; q < Row::kWidth; ++q) partials[(int64_t)blockIdx.x * Row::kWidth + q] = v[q];
  }
}

__global__ __launch_bounds__(kBlock) void icp_accumulate_kernel(const double* __restrict__ reading, const double* __restrict__ rnormals,
                                                                int64_t m, const double* __restrict__ map_points,
                                                                const double* __restrict__ map_normals, const int32_t* __restrict__ idx,
                                                                const double* __restrict__ dist, int knn, const double* __restrict__ threshold,
                                                                double cos_min, const double* __restrict__ state,
                                                                const int32_t* __restrict__ status, double* __restrict__ partials,
                                                                uint8_t* __restrict__ kept_out) {
  icp_accumulate_body<6>(reading, rnormals, nullptr, nullptr, m, map_points, map_normals, idx, dist, knn, threshold, cos_min, state, nullptr,
                         status, partials, kept_out);
}

// The finish kernels' body (one block): threads LANES q .. LANES q + LANES - 1 sum value q of the NV-wide rows over the blocks
// b = l, l + LANES, ... in order, thread q adds the LANES sums of value q in order (rows_block_totals; 744 lane sums over the 256
// threads for NV = 93, three trips).  False for every thread but thread 0 of a registration that has not ended: it goes on to the tail.
template <int NV>
__device__ __forceinline__ bool icp_finish_totals(const double* __restrict__ partials, int n_blocks, const int32_t* __restrict__ status,
                                                  double* s_tot) {
  __shared__ double s_part[NV * kRowSumLanes];
  if (status[0] != 0) return false;
  rows_block_totals<NV, kRowSumLanes>(partials, n_blocks, s_part, s_tot);
  return threadIdx.x == 0;
}

__global__ __launch_bounds__(kBlock) void icp_finish_kernel(const double* __restrict__ partials, int n_blocks, int64_t m, IcpParams prm,
                                                            double* __restrict__ state, int32_t* __restrict__ status) {
  __shared__ double s_tot[DC_ICP_PARTIALS];
  if (icp_finish_totals<DC_ICP_PARTIALS>(partials, n_blocks, status, s_tot)) icp_finish_tail(s_tot, m, prm, state, status);
}

// ---- the sweep-aware iteration (include/dc_hip.h "sweep-aware registration") ------------------------------------------------------
__global__ void icp_ct_init_kernel(const double* __restrict__ twist, double* __restrict__ ct) {
  const int t = threadIdx.x;
  if (t < 6) { ct[DC_ICP_CT_STATE_TWIST + t] = twist[t]; ct[DC_ICP_CT_STATE_PRIOR_TWIST + t] = twist[t]; }
  else if (t >= 12 && t < DC_ICP_CT_STATE_COUNT) ct[t] = 0.0;
}

__global__ __launch_bounds__(kBlock) void icp_ct_accumulate_kernel(const double* __restrict__ reading, const double* __restrict__ dq,
                                                                   const double* __restrict__ dnq, const double* __restrict__ tau,
                                                                   int64_t m, const double* __restrict__ map_points,
                                                                   const double* __restrict__ map_normals, const int32_t* __restrict__ idx,
                                                                   const double* __restrict__ dist, int knn,
                                                                   const double* __restrict__ threshold, double cos_min,
                                                                   const double* __restrict__ state, const double* __restrict__ ct,
                                                                   const int32_t* __restrict__ status, double* __restrict__ partials,
                                                                   uint8_t* __restrict__ kept_out) {
  icp_accumulate_body<12>(dq, dnq, reading, tau, m, map_points, map_normals, idx, dist, knn, threshold, cos_min, state, ct, status, partials,
                          kept_out);
}

// The tail's workspace is in LDS (icp_solve's L takes runtime indices).
__global__ __launch_bounds__(kBlock) void icp_ct_finish_kernel(const double* __restrict__ partials, int n_blocks, int64_t m, IcpParams prm,
                                                               IcpCtParams cp, double* __restrict__ state, double* __restrict__ ct,
                                                               int32_t* __restrict__ status) {
  __shared__ double s_tot[DC_ICP_CT_PARTIALS];
  __shared__ double s_work[kIcpCtWork];
  if (icp_finish_totals<DC_ICP_CT_PARTIALS>(partials, n_blocks, status, s_tot)) icp_ct_finish_tail(s_tot, m, prm, cp, state, ct, status, s_work);
}

// Reading points the map takes: world coordinates and normals of every point, mask = nearest map point farther than min_dist
// (dist1 NULL: an empty map) and depth <= max_range.
__global__ __launch_bounds__(kBlock) void map_select_kernel(const double* __restrict__ reading, const double* __restrict__ rnormals,
                                                            const double* __restrict__ depth, int64_t m, const double* __restrict__ pose,
                                                            const double* __restrict__ dist1, double min_dist, double max_range,
                                                            uint8_t* __restrict__ mask, double* __restrict__ pts_out,
                                                            double* __restrict__ nrm_out) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= m) return;
  double T[16];
#pragma unroll
  for (int q = 0; q < 16; ++q) T[q] = pose[q];
  const double p[3] = {reading[i * 3], reading[i * 3 + 1], reading[i * 3 + 2]};
  const double pn[3] = {rnormals[i * 3], rnormals[i * 3 + 1], rnormals[i * 3 + 2]};
  double x[3];
  move_point(T, p, x);
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    pts_out[i * 3 + r] = x[r];
    nrm_out[i * 3 + r] = T[r * 4] * pn[0] + T[r * 4 + 1] * pn[1] + T[r * 4 + 2] * pn[2];
  }
  const double d = dist1 ? dist1[i] : INFINITY;
  mask[i] = (d > min_dist && depth[i] <= max_range) ? 1 : 0;
}

}  // namespace dc

using namespace dc;

// The arguments both accumulate entry points share: DC_OK or the code to return.
static int icp_accumulate_args(int64_t m, const double* map_points, const double* map_normals, const int32_t* idx, const double* dist, int knn,
                               const double* threshold, const double* state, const int32_t* status, const double* partials, int n_blocks) {
  if (m < 1 || knn < 1 || knn > 64 || !map_points || !map_normals || !idx || !dist || !threshold || !state || !status || !partials)
    return DC_ERR_ARG;
  if (m >= (int64_t)0x7fffffff / knn) return DC_ERR_UNSUPPORTED;
  if (n_blocks != icp_blocks(m)) return DC_ERR_WORKSPACE;
  return DC_OK;
}

extern "C" {

int dc_icp_blocks(int64_t m) { return m < 0 ? 0 : icp_blocks(m); }

int dc_icp_init(const double* prior, double* state, int32_t* status, hipStream_t stream) {
  if (!prior || !state || !status) return DC_ERR_ARG;
  hipLaunchKernelGGL(icp_init_kernel, dim3(1), dim3(64), 0, stream, prior, state, status);
  DC_HIP(hipGetLastError());
  return DC_OK;
}

int dc_icp_accumulate(const double* reading, const double* normals, int64_t m, const double* map_points, const double* map_normals,
                      const int32_t* idx, const double* dist, int knn, const double* threshold, double cos_min, const double* state,
                      const int32_t* status, double* partials, int n_blocks, uint8_t* kept_out, hipStream_t stream) {
  if (!reading || !normals) return DC_ERR_ARG;
  if (const int rc = icp_accumulate_args(m, map_points, map_normals, idx, dist, knn, threshold, state, status, partials, n_blocks)) return rc;
  hipLaunchKernelGGL(icp_accumulate_kernel, dim3((unsigned)n_blocks), dim3(kBlock), 0, stream, reading, normals, m, map_points, map_normals,
                     idx, dist, knn, threshold, cos_min, state, status, partials, kept_out);
  DC_HIP(hipGetLastError());
  return DC_OK;
}

int dc_icp_finish(const double* partials, int n_blocks, int64_t m, double min_rot, double min_trans, int smooth, int max_iters,
                  double max_rot, double max_trans, int min_pairs, double* state, int32_t* status, hipStream_t stream) {
  if (!icp_finish_args_ok(partials, n_blocks, m, smooth, max_iters, state, status)) return DC_ERR_ARG;
  IcpParams prm{min_rot, min_trans, max_rot, max_trans, smooth, max_iters, min_pairs};
  hipLaunchKernelGGL(icp_finish_kernel, dim3(1), dim3(kBlock), 0, stream, partials, n_blocks, m, prm, state, status);
  DC_HIP(hipGetLastError());
  return DC_OK;
}

int dc_icp_ct_init(const double* twist, double* ct_state, hipStream_t stream) {
  if (!twist || !ct_state) return DC_ERR_ARG;
  hipLaunchKernelGGL(icp_ct_init_kernel, dim3(1), dim3(64), 0, stream, twist, ct_state);
  DC_HIP(hipGetLastError());
  return DC_OK;
}

int dc_icp_ct_accumulate(const double* reading, const double* q, const double* nq, const double* tau, int64_t m, const double* map_points,
                         const double* map_normals, const int32_t* idx, const double* dist, int knn, const double* threshold,
                         double cos_min, const double* state, const double* ct_state, const int32_t* status, double* partials,
                         int n_blocks, uint8_t* kept_out, hipStream_t stream) {
  if (!reading || !q || !nq || !tau || !ct_state) return DC_ERR_ARG;
  if (const int rc = icp_accumulate_args(m, map_points, map_normals, idx, dist, knn, threshold, state, status, partials, n_blocks)) return rc;
  hipLaunchKernelGGL(icp_ct_accumulate_kernel, dim3((unsigned)n_blocks), dim3(kBlock), 0, stream, reading, q, nq, tau, m, map_points,
                     map_normals, idx, dist, knn, threshold, cos_min, state, ct_state, status, partials, kept_out);
  DC_HIP(hipGetLastError());
  return DC_OK;
}

int dc_icp_ct_finish(const double* partials, int n_blocks, int64_t m, double min_rot, double min_trans, int smooth, int max_iters,
                     double max_rot, double max_trans, int min_pairs, double beta_v, double beta_w, double max_twist_trans,
                     double max_twist_rot, double* state, double* ct_state, int32_t* status, hipStream_t stream) {
  if (!icp_finish_args_ok(partials, n_blocks, m, smooth, max_iters, state, status) || !ct_state || !(beta_v >= 0.0) || !(beta_w >= 0.0))
    return DC_ERR_ARG;
  IcpParams prm{min_rot, min_trans, max_rot, max_trans, smooth, max_iters, min_pairs};
  IcpCtParams cp{beta_v, beta_w, max_twist_trans, max_twist_rot};
  hipLaunchKernelGGL(icp_ct_finish_kernel, dim3(1), dim3(kBlock), 0, stream, partials, n_blocks, m, prm, cp, state, ct_state, status);
  DC_HIP(hipGetLastError());
  return DC_OK;
}

int dc_map_select(const double* reading, const double* normals, const double* depth, int64_t m, const double* pose, const double* dist1,
                  double min_dist, double max_range, uint8_t* mask_out, double* points_out, double* normals_out, hipStream_t stream) {
  if (m == 0) return DC_OK;
  if (m < 0 || !reading || !normals || !depth || !pose || !mask_out || !points_out || !normals_out) return DC_ERR_ARG;
  hipLaunchKernelGGL(map_select_kernel, dim3((unsigned)((m + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, reading, normals, depth, m,
                     pose, dist1, min_dist, max_range, mask_out, points_out, normals_out);
  DC_HIP(hipGetLastError());
  return DC_OK;
}

}  // extern "C"
