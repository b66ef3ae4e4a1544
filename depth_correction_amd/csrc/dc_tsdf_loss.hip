// Self-supervised training against the fused volume: the mean (squared) trilinear distance of the corrected, posed points of a
// sequence to the surface the sequence's scans were fused into, and its gradient to the model weights, the exponents and the poses,
// in ONE host call (dc_tsdf_loss), all fp64 (DESIGN "Self-supervised training against the fused volume"; the rules:
// dc_tsdf_loss_math.h).  The stream sees two launches:
//
//   1. tsdf_loss_kernel, one lane per point, 128 lanes per block, the blocks laid out per scan from scan_ptr (dc_scanloss.h: the
//      layout, the block's setup and partial row, the finishing).  A lane forms x = R (vp + d' dir) + t with the statements of
//      points_fwd_kernel (dc_points_dev.h), keeps it in registers, samples the volume at it -- eight voxel reads through the block
//      table of the total volume and, with exclusion, eight through the table segment of the block's own scan, whose bounds are
//      block-uniform -- classifies the point (invalid / unobserved / gated / used), forms the term and dl/dx and runs the point
//      epilogue of dc_points_bwd (points_bwd_point).  The block's partial row is [sum l, used, gated, unobserved, invalid, dw[P],
//      de[P], d[R|t][12]].
//   2. tsdf_loss_finish_kernel, one block: per scan, in scan order, four interleaved chains add the scan's block rows in block
//      order, the four sums are added in chain order; the scalar columns are then added over the scans in scan order.
//
// No atomics, no allocation, copy or synchronisation: the same inputs give the same bits whatever ran before.
//
// The file is built with -ffp-contract=off for the sample and the term, whose bits are compared with their numpy restatement.  The
// statements that form the point and its epilogue are those of dc_points_fwd / dc_points_bwd and are contracted as they are there, so
// that x has the bits dc_points_fwd writes: the pragma below covers the headers they live in.
#pragma clang fp contract(fast)
#include "dc_common.h"
#include "dc_device.h"
#include "dc_hostutil.h"
#include "dc_pointmath.h"
#include "dc_points_dev.h"
#include "dc_scanloss.h"
#pragma clang fp contract(off)
#include "dc_tsdf_loss_math.h"
#include "../../include/dc_hip.h"

namespace {

using namespace dc;

constexpr int kFixedCols = 5;                                 // sum l, used, gated, unobserved, invalid
constexpr int kMaxCols = kFixedCols + 2 * DC_MAX_MODEL_TERMS + 12;
constexpr int kFinishCols = 64;                               // one finishing lane per column, four chains

// the own volumes of all scans as one structure: scan s owns keys / slots [ptr[s], ptr[s + 1]), the slots index the shared pool
struct OwnTables {
  const uint64_t* keys;
  const int32_t* slots;
  const int64_t* ptr;
  int64_t n_keys, capacity;
  const int64_t* sum;
  const int32_t* count;
};

template <typename T>
__global__ void __launch_bounds__(kLossBlock) tsdf_loss_kernel(PointInputs in, const uint8_t* __restrict__ mask,
                                                               const int64_t* __restrict__ scan_ptr, int64_t n, TsdfTable total,
                                                               const int64_t* __restrict__ n_blocks, OwnTables own, TsdfGrid grid,
                                                               double tau, int min_count, double max_residual, int squared, int want_e,
                                                               double* __restrict__ value_out, uint8_t* __restrict__ flag_out,
                                                               double* __restrict__ x_out, double* __restrict__ partials) {
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
  // the tables, clamped to what the caller allocated (block-uniform)
  const int64_t nb0 = *n_blocks;
  total.nb = nb0 < 0 ? 0 : (nb0 > total.capacity ? total.capacity : nb0);
  TsdfTable mine{nullptr, nullptr, 0, own.capacity, own.sum, own.count};
  if (own.keys) {
    int64_t a = own.ptr[scan], b = own.ptr[scan + 1];
    a = a < 0 ? 0 : (a > own.n_keys ? own.n_keys : a);
    b = b < a ? a : (b > own.n_keys ? own.n_keys : b);
    mine.keys = own.keys + a;
    mine.slots = own.slots + a;
    mine.nb = b - a;
  }

  double acc[kFixedCols] = {0.0, 0.0, 0.0, 0.0, 0.0}, gw[DC_MAX_MODEL_TERMS], ge[DC_MAX_MODEL_TERMS], gT[6];
  zero_grads(gw, ge, gT);
  const int64_t g = first + tid;
  if (g < last) {
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    double x[3] = {nan, nan, nan}, value = nan;
    int cls = kTsdfLossMasked;
    if (mask ? mask[g] != 0 : true) {
      const PointRaw<T> raw = load_point_raw<T>(one, mp, g);
      double vp[3] = {0.0, 0.0, 0.0}, T12[12];
      if (in.vps) Row3<T, 3>::load((const T*)in.vps, g, vp, QParams{});
      load_pose(one, tile, 0, T12);
      posed_point<T>(mp, raw, vp, T12, x);
      const TsdfSample s = tsdf_sample_point_minus(x, grid, tau, min_count, total, mine);
      cls = tsdf_loss_class(s, max_residual);
      if (s.flag == 0) value = s.phi;
      if (cls == kTsdfLossUsed) {
        double dl_dx[3];
        acc[0] = tsdf_loss_term(s.phi, s.grad, squared != 0, dl_dx);
        acc[1] = 1.0;
        int s_unused;
        points_bwd_point<T>(one, tile, mp, g, raw, dl_dx, gw, ge, gT, want_e != 0, true, &s_unused);
      } else {
        acc[cls == kTsdfLossGated ? 2 : (cls == kTsdfLossUnobserved ? 3 : 4)] = 1.0;
      }
    }
    if (value_out) value_out[g] = value;
    if (flag_out) flag_out[g] = (uint8_t)cls;
    if (x_out) {
      x_out[3 * g] = x[0];
      x_out[3 * g + 1] = x[1];
      x_out[3 * g + 2] = x[2];
    }
  }
  scan_block_store<kFixedCols>(acc, gw, ge, gT, nt, s_red, partials);
}

// out = [mean loss, used, gated, unobserved, invalid, dL/dw[P], dL/de[P], dL/d[R|t][12 S]], the gradients divided by M = used
__global__ void __launch_bounds__(kLossFinishBlock) tsdf_loss_finish_kernel(const double* __restrict__ partials, int nt,
                                                                           const int64_t* __restrict__ scan_ptr, int64_t n, int n_scans,
                                                                           int64_t n_rows, double* __restrict__ out) {
  scan_loss_finish<kFixedCols, kLossFinishBlock / kFinishCols, kFinishCols>(partials, nt, scan_ptr, n, n_scans, n_rows, kFixedCols, out);
}

size_t partial_bytes(int64_t n, int n_scans, int n_terms) {
  return (size_t)(max_blocks(n, n_scans) + 1) * (size_t)(kFixedCols + 2 * n_terms + 12) * sizeof(double);
}

}  // namespace

extern "C" {

size_t dc_tsdf_loss_workspace_bytes(int64_t n, int n_scans, int n_terms) {
  if (n < 0 || n_scans < 0 || n_terms < 0 || n_terms > DC_MAX_MODEL_TERMS) return 0;
  return partial_bytes(n, n_scans, n_terms);
}

int dc_tsdf_loss(const uint64_t* keys, const int32_t* slots, const int64_t* n_blocks, int64_t capacity, const int64_t* sum,
                 const int32_t* count, const uint64_t* own_keys, const int32_t* own_slots, const int64_t* own_ptr, int64_t n_own_keys,
                 int64_t own_capacity, const int64_t* own_sum, const int32_t* own_count, double ox, double oy, double oz, double voxel,
                 double trunc, int min_count, const void* vps, const void* dirs, const void* depth, const void* inc, const uint8_t* lmask,
                 const uint8_t* mask, int dtype, int64_t n, const int64_t* scan_ptr, const double* poses, int n_scans, int model_kind,
                 int n_terms, const double* w, const double* e, int want_exponent, int squared, double max_residual, double* value_out,
                 uint8_t* flag_out, double* x_out, double* out, void* ws, size_t ws_bytes, dcStream_t stream) {
  const TsdfGrid grid{{ox, oy, oz}, voxel, {0, 0, 0}};
  if (n < 0 || n_scans < 0 || !out || !keys || !slots || !n_blocks || !sum || !count) return DC_ERR_ARG;
  PointInputs in;
  int64_t rows;
  const bool volume_ok = tsdf_lattice_ok(grid) && trunc > 0.0 && isfinite(trunc) && min_count >= 1 && capacity >= 1 &&
                         capacity < ((int64_t)1 << 22) && !isnan(max_residual);
  const bool exclusion_ok = !own_keys || (own_slots && own_ptr && own_sum && own_count && n_own_keys >= 0 && own_capacity >= 1);
  const int rc0 = scan_loss_args(vps, dirs, depth, inc, lmask, dtype, n, scan_ptr, poses, n_scans, model_kind, &n_terms, w, e,
                                 volume_ok && exclusion_ok, &in, &rows);
  if (rc0 != DC_OK) return rc0;
  if (n > 0 && (!ws || ws_bytes < dc_tsdf_loss_workspace_bytes(n, n_scans, n_terms))) return DC_ERR_WORKSPACE;
  double* partials = (double*)ws;
  const hipStream_t st = (hipStream_t)stream;
  if (n > 0) {
    const TsdfTable total{keys, slots, 0, capacity, sum, count};
    const OwnTables own{own_keys, own_slots, own_ptr, n_own_keys, own_capacity, own_sum, own_count};
    const dim3 grid_dim((unsigned)rows), block(kLossBlock);
    if (dtype == DC_F32)
      tsdf_loss_kernel<float><<<grid_dim, block, 0, st>>>(in, mask, scan_ptr, n, total, n_blocks, own, grid, trunc, min_count, max_residual,
                                                          squared, want_exponent, value_out, flag_out, x_out, partials);
    else
      tsdf_loss_kernel<double><<<grid_dim, block, 0, st>>>(in, mask, scan_ptr, n, total, n_blocks, own, grid, trunc, min_count, max_residual,
                                                           squared, want_exponent, value_out, flag_out, x_out, partials);
    DC_HIP(hipGetLastError());
  }
  tsdf_loss_finish_kernel<<<1, kLossFinishBlock, 0, st>>>(partials, n_terms, scan_ptr, n, n_scans, rows, out);
  DC_HIP(hipGetLastError());
  return DC_OK;
}

}  // extern "C"
