// Supervised training against the ground-truth mesh: the mean point-to-surface distance of the corrected, posed points of a
// sequence and its gradient to the model weights, the exponents and the poses, in ONE host call (dc_mesh_loss): a walk kernel and a
// finishing kernel, all fp64.  eval_map measures a map in this metric; this is the loss that trains in it (DESIGN "Supervised
// training against the mesh").
//
// Walk kernel, one lane per point, 128 lanes per block, the blocks laid out per scan from scan_ptr (dc_scanloss.h: the layout, the
// block's setup and partial row, the finishing).  A lane
//   * forms x = R (vp + d' dir) + t with the statements of points_fwd_kernel (dc_points_dev.h),
//   * finds the nearest face by dc_meshwalk.h's walk -- the one dc_mesh_closest runs, same bound, same tie rule -- after folding
//     the leaf of leaf_hint (last evaluation's winner) into the walk's state, which only prunes (dc_meshwalk.h's header),
//   * forms the term and dl/dx (dc_meshloss_math.h) and runs the point epilogue of dc_points_bwd (points_bwd_point).
// The block's partial row is [sum l, used, gated, invalid, dw[P], de[P], d[R|t][12]].  No atomics anywhere.
//
// Finishing kernel, one block: per scan, in scan order, eight interleaved chains add the scan's block rows in block order (chain c
// takes the blocks c, c + 8, ...), the eight sums are added in chain order; the scalar columns are then added over the scans in
// scan order.  out = [mean loss, used, gated, invalid, dL/dw[P], dL/de[P], dL/d[R|t][12 S]], the gradients divided by M = used; M = 0
// gives a NaN loss (the mean of nothing) and zero gradients.  The same inputs give the same bits whatever ran before.
#include "dc_common.h"
#include "dc_device.h"
#include "dc_hostutil.h"
#include "dc_pointmath.h"
#include "dc_points_dev.h"
#include "dc_trimath.h"
#include "dc_meshwalk.h"
#include "dc_meshloss_math.h"
#include "dc_scanloss.h"
#include "../../include/dc_hip.h"

namespace {

using namespace dc;

constexpr int kFixedCols = 4;                                 // sum l, used, gated, invalid
constexpr int kMaxCols = kFixedCols + 2 * DC_MAX_MODEL_TERMS + 12;

struct MeshArrays {
  const int32_t* child;
  const float* node_box;
  const double* leaf_tri;
  const int32_t* leaf_face;
  int64_t n_faces;
};

template <typename T>
__global__ void __launch_bounds__(kLossBlock) mesh_loss_kernel(MeshArrays mesh, PointInputs in, const uint8_t* __restrict__ mask,
                                                               const int64_t* __restrict__ scan_ptr, int64_t n, double limit2,
                                                               double max_dist, int squared, int want_e,
                                                               int32_t* __restrict__ leaf_hint, int32_t* __restrict__ face_out,
                                                               double* __restrict__ dist_out, double* __restrict__ closest_out,
                                                               double* __restrict__ partials) {
  __shared__ int32_t stack[kBvhStackDepth * kLossBlock];
  __shared__ double s_pose[12];
  __shared__ double s_red[kLossWaves][kMaxCols];
  const int tid = threadIdx.x;
  int scan = -1;
  int64_t first = 0, last = 0;
  block_scan(scan_ptr, in.n_scans, n, (int64_t)blockIdx.x, &scan, &first, &last);
  // the grid is an upper bound of the blocks in use (branching on `scan` rather than on block_scan's result keeps this kernel
  // at 128 VGPRs, four wavefronts per SIMD by registers)
  if (scan < 0) return;
  PointInputs one;
  ModelParams mp;
  int nt;
  scan_block_setup(in, scan, s_pose, one, mp, nt);
  const PoseTile tile{in.poses ? s_pose : nullptr};

  double acc[kFixedCols] = {0.0, 0.0, 0.0, 0.0}, gw[DC_MAX_MODEL_TERMS], ge[DC_MAX_MODEL_TERMS], gT[6];
  zero_grads(gw, ge, gT);
  const int64_t g = first + tid;
  const bool active = g < last;
  if (active) {
    int32_t face = -1, leaf_w = -1;
    double dist = INFINITY, c[3] = {NAN, NAN, NAN};
    if (mask ? mask[g] != 0 : true) {
      const PointRaw<T> raw = load_point_raw<T>(one, mp, g);
      double vp[3] = {0.0, 0.0, 0.0}, T12[12], x[3];
      if (in.vps) Row3<T, 3>::load((const T*)in.vps, g, vp, QParams{});
      load_pose(one, tile, 0, T12);
      posed_point<T>(mp, raw, vp, T12, x);
      if (isfinite(x[0]) && isfinite(x[1]) && isfinite(x[2])) {
        double best = limit2;                                 // d^2 of the best face so far (the max_dist bound before the first)
        int32_t best_face = -1;
        int64_t best_leaf = -1;
        if (leaf_hint) {
          const int32_t h = leaf_hint[g];
          if (h >= 0 && (int64_t)h < mesh.n_faces) mesh_walk_leaf(mesh.leaf_tri, mesh.leaf_face, h, x, best, best_face, best_leaf);
        }
        const Query32 q = mesh_query(x);
        mesh_walk<kLossBlock>(mesh.child, mesh.node_box, mesh.leaf_tri, mesh.leaf_face, mesh.n_faces, x, q, stack, tid, best, best_face,
                              best_leaf);
        if (best_face >= 0) {
          const double d = __dsqrt_rn(best);
          if (max_dist > 0.0 && !(d <= max_dist)) {
            acc[2] = 1.0;
          } else {
            double tri[9], r, grad[3];
#pragma unroll
            for (int k = 0; k < 9; ++k) tri[k] = mesh.leaf_tri[9 * best_leaf + k];
            closest_on_triangle(tri, x, c, nullptr);          // the winning face again: the same operations, the same point
            acc[0] = mesh_loss_term(x, c, squared != 0, &r, grad);
            acc[1] = 1.0;
            face = best_face;
            leaf_w = (int32_t)best_leaf;
            dist = d;
            int s_unused;
            points_bwd_point<T>(one, tile, mp, g, raw, grad, gw, ge, gT, want_e != 0, true, &s_unused);
          }
        } else {
          if (max_dist > 0.0) acc[2] = 1.0;                   // nothing within the bound
          else acc[3] = 1.0;                                  // without a bound: every d^2 was a NaN
        }
      } else {
        acc[3] = 1.0;
      }
    }
    if (leaf_hint) leaf_hint[g] = leaf_w;
    if (face_out) face_out[g] = face;
    if (dist_out) dist_out[g] = dist;
    if (closest_out) {
      closest_out[3 * g] = c[0];
      closest_out[3 * g + 1] = c[1];
      closest_out[3 * g + 2] = c[2];
    }
  }
  scan_block_store<kFixedCols>(acc, gw, ge, gT, nt, s_red, partials);
}

__global__ void __launch_bounds__(kLossFinishBlock) mesh_loss_finish_kernel(const double* __restrict__ partials, int nt,
                                                                           const int64_t* __restrict__ scan_ptr, int64_t n,
                                                                           int n_scans, int64_t n_rows, double* __restrict__ out) {
  scan_loss_finish<kFixedCols, 8, 32>(partials, nt, scan_ptr, n, n_scans, n_rows, 4, out);
}

}  // namespace

extern "C" {

size_t dc_mesh_loss_workspace_bytes(int64_t n, int n_scans, int n_terms) {
  if (n < 0 || n_scans < 0 || n_terms < 0 || n_terms > DC_MAX_MODEL_TERMS) return 0;
  return (size_t)(max_blocks(n, n_scans) + 1) * (size_t)(kFixedCols + 2 * n_terms + 12) * sizeof(double);
}

int dc_mesh_loss(const int32_t* child, const float* node_box, const double* leaf_tri, const int32_t* leaf_face, int64_t n_faces,
                 const void* vps, const void* dirs, const void* depth, const void* inc, const uint8_t* lmask, const uint8_t* mask,
                 int dtype, int64_t n, const int64_t* scan_ptr, const double* poses, int n_scans, int model_kind, int n_terms,
                 const double* w, const double* e, int want_exponent, int squared, double max_dist, int32_t* leaf_hint,
                 int32_t* face_out, double* dist_out, double* closest_out, double* out, void* ws, size_t ws_bytes, dcStream_t stream) {
  if (n_faces < 1 || n < 0 || n_scans < 0 || !node_box || !leaf_tri || !leaf_face || (n_faces > 1 && !child) || !out) return DC_ERR_ARG;
  PointInputs in;
  int64_t rows;
  const int rc = scan_loss_args(vps, dirs, depth, inc, lmask, dtype, n, scan_ptr, poses, n_scans, model_kind, &n_terms, w, e,
                                max_dist == max_dist, &in, &rows);
  if (rc != DC_OK) return rc;
  if (n > 0 && (!ws || ws_bytes < dc_mesh_loss_workspace_bytes(n, n_scans, n_terms))) return DC_ERR_WORKSPACE;
  double* partials = (double*)ws;
  if (n > 0) {
    // the walk prunes with d^2: the bound squared, one part in 2^50 up so that its rounding cannot cut a face at exactly max_dist
    // (sqrt(d^2) <= max_dist decides in the end), as in dc_mesh_closest
    const bool bounded = max_dist > 0.0 && max_dist < INFINITY;
    const double limit2 = bounded ? max_dist * max_dist * (1.0 + 0x1p-50) : INFINITY;
    const double md = bounded ? max_dist : 0.0;
    const MeshArrays mesh{child, node_box, leaf_tri, leaf_face, n_faces};
    const dim3 grid((unsigned)rows), block(kLossBlock);
    if (dtype == DC_F32)
      mesh_loss_kernel<float><<<grid, block, 0, (hipStream_t)stream>>>(mesh, in, mask, scan_ptr, n, limit2, md, squared, want_exponent,
                                                                      leaf_hint, face_out, dist_out, closest_out, partials);
    else
      mesh_loss_kernel<double><<<grid, block, 0, (hipStream_t)stream>>>(mesh, in, mask, scan_ptr, n, limit2, md, squared, want_exponent,
                                                                       leaf_hint, face_out, dist_out, closest_out, partials);
    DC_HIP(hipGetLastError());
  }
  mesh_loss_finish_kernel<<<1, kLossFinishBlock, 0, (hipStream_t)stream>>>(partials, n_terms, scan_ptr, n, n_scans, rows, out);
  DC_HIP(hipGetLastError());
  return DC_OK;
}

}  // extern "C"
