// Supervised training against the ground-truth mesh: the mean point-to-surface distance of the corrected, posed points of a
// sequence and its gradient to the model weights, the exponents and the poses, in ONE host call (dc_mesh_loss): a walk kernel and a
// finishing kernel, all fp64.  eval_map measures a map in this metric; this is the loss that trains in it (DESIGN "Supervised
// training against the mesh").
//
// Walk kernel, one lane per point, 128 lanes per block.  The blocks are laid out per scan from scan_ptr (scan s owns
// ceil(n_s / 128) consecutive blocks, an empty scan none), so a block never straddles scans: the pose of its one scan is staged in
// LDS once and the block's pose sums are the sums of that scan.  A lane
//   * forms x = R (vp + d' dir) + t with the statements of points_fwd_kernel (dc_points_dev.h),
//   * finds the nearest face by dc_meshwalk.h's walk -- the one dc_mesh_closest runs, same bound, same tie rule -- after folding
//     the leaf of leaf_hint (last evaluation's winner) into the walk's state, which only prunes (dc_meshwalk.h's header),
//   * forms the term and dl/dx (dc_meshloss_math.h) and runs the point epilogue of dc_points_bwd (points_bwd_point).
// The block's partial row [sum l, used, gated, invalid, dw[P], de[P], d[R|t][12]] is summed in a fixed order: a shuffle tree within
// the wavefront, then wavefront 0 + wavefront 1 through LDS.  No atomics anywhere.
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
#include "../../include/dc_hip.h"

namespace {

using namespace dc;

constexpr int kLossBlock = 128;
constexpr int kLossWaves = kLossBlock / kWave;
constexpr int kFixedCols = 4;                                 // sum l, used, gated, invalid
constexpr int kMaxCols = kFixedCols + 2 * DC_MAX_MODEL_TERMS + 12;
constexpr int kFinishBlock = 256;
constexpr int kChains = kFinishBlock / 32;                    // kMaxCols == 32 columns x 8 chains

struct MeshArrays {
  const int32_t* child;
  const float* node_box;
  const double* leaf_tri;
  const int32_t* leaf_face;
  int64_t n_faces;
};

// points [a, b) of scan s (scan_ptr == NULL: one scan holding every point), clipped to [0, n]
__device__ __forceinline__ void scan_range(const int64_t* __restrict__ scan_ptr, int s, int64_t n, int64_t* a, int64_t* b) {
  int64_t lo = scan_ptr ? scan_ptr[s] : 0, hi = scan_ptr ? scan_ptr[s + 1] : n;
  lo = lo < 0 ? 0 : (lo > n ? n : lo);
  hi = hi < lo ? lo : (hi > n ? n : hi);
  *a = lo;
  *b = hi;
}
__device__ __forceinline__ int64_t blocks_of(int64_t count) { return (count + kLossBlock - 1) / kLossBlock; }

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
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  // the scan of this block and its first point (block-uniform)
  int scan = -1;
  int64_t first = 0, last = 0, cum = 0;
  for (int s = 0; s < in.n_scans; ++s) {
    int64_t a, b;
    scan_range(scan_ptr, s, n, &a, &b);
    const int64_t nb = blocks_of(b - a);
    if ((int64_t)blockIdx.x < cum + nb) {
      scan = s;
      first = a + ((int64_t)blockIdx.x - cum) * kLossBlock;
      last = b;
      break;
    }
    cum += nb;
  }
  if (scan < 0) return;                                       // the grid is an upper bound of the blocks in use
  if (in.poses && tid < 12) s_pose[tid] = in.poses[(int64_t)scan * 12 + tid];
  __syncthreads();
  PointInputs one = in;                                       // the block's scan as scan 0 of a one-scan sequence
  one.scan_id = nullptr;
  one.n_scans = 1;
  const PoseTile tile{in.poses ? s_pose : nullptr};
  ModelParams mp;
  load_model(in, mp);
  const int nt = in.model_kind == DC_MODEL_NONE ? 0 : in.n_terms;

  double acc[kFixedCols] = {0.0, 0.0, 0.0, 0.0}, gw[DC_MAX_MODEL_TERMS], ge[DC_MAX_MODEL_TERMS], gT[6];
#pragma unroll
  for (int k = 0; k < DC_MAX_MODEL_TERMS; ++k) gw[k] = ge[k] = 0.0;
#pragma unroll
  for (int k = 0; k < 6; ++k) gT[k] = 0.0;
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
  // block sums, column by column: a fixed shuffle tree per wavefront, then the wavefronts in order
#pragma unroll
  for (int q = 0; q < kFixedCols; ++q) {
    const double s = wave_sum(acc[q]);
    if (lane == 0) s_red[wave][q] = s;
  }
#pragma unroll
  for (int k = 0; k < DC_MAX_MODEL_TERMS; ++k) {
    if (k < nt) {
      const double sw = wave_sum(gw[k]), se = wave_sum(ge[k]);
      if (lane == 0) {
        s_red[wave][kFixedCols + k] = sw;
        s_red[wave][kFixedCols + nt + k] = se;
      }
    }
  }
#pragma unroll
  for (int q = 0; q < 12; ++q) {
    // dL/d[R|t]_{a,b} = g_a [xl, 1]_b, the product rounded before it is added (no contraction into the sum)
    const double v = (q & 3) == 3 ? gT[q >> 2] : __dmul_rn(gT[q >> 2], gT[3 + (q & 3)]);
    const double s = wave_sum(v);
    if (lane == 0) s_red[wave][kFixedCols + 2 * nt + q] = s;
  }
  __syncthreads();
  const int ncols = kFixedCols + 2 * nt + 12;
  if (tid < ncols) {
    double t = s_red[0][tid];
#pragma unroll
    for (int wv = 1; wv < kLossWaves; ++wv) t += s_red[wv][tid];
    partials[(int64_t)blockIdx.x * ncols + tid] = t;
  }
}

__global__ void __launch_bounds__(kFinishBlock) mesh_loss_finish_kernel(const double* __restrict__ partials, int nt,
                                                                       const int64_t* __restrict__ scan_ptr, int64_t n, int n_scans,
                                                                       int64_t n_rows, double* __restrict__ out) {
  __shared__ double s_red[kChains][32];
  __shared__ double s_count;
  const int tid = threadIdx.x, col = tid & 31, chain = tid >> 5;
  const int ncols = kFixedCols + 2 * nt + 12, n_scalar = kFixedCols + 2 * nt;
  double total = 0.0;                                         // chain 0, scalar columns: the sum over the scans so far
  int64_t blk0 = 0;
  for (int s = 0; s < n_scans; ++s) {
    int64_t a, b;
    scan_range(scan_ptr, s, n, &a, &b);
    int64_t nb = blocks_of(b - a);
    if (blk0 + nb > n_rows) nb = n_rows - blk0;               // never past the rows the walk kernel had blocks for
    double sum = 0.0;
    if (col < ncols)
      for (int64_t r = chain; r < nb; r += kChains) sum += partials[(blk0 + r) * ncols + col];
    s_red[chain][col] = sum;
    __syncthreads();
    if (chain == 0 && col < ncols) {
      double t = s_red[0][col];
#pragma unroll
      for (int ch = 1; ch < kChains; ++ch) t += s_red[ch][col];
      if (col < n_scalar) total += t;
      else out[n_scalar + (int64_t)s * 12 + (col - n_scalar)] = t;
    }
    __syncthreads();
    blk0 += nb;
  }
  if (tid == 1) s_count = total;                              // M = used
  __syncthreads();
  const double M = s_count;
  if (chain == 0 && col < n_scalar) {
    if (col == 0) out[0] = M > 0.0 ? total / M : __longlong_as_double(0x7ff8000000000000ll);
    else if (col < kFixedCols) out[col] = total;
    else out[col] = M > 0.0 ? total / M : 0.0;
  }
  for (int64_t i = tid; i < 12 * (int64_t)n_scans; i += kFinishBlock) {
    const double v = out[n_scalar + i];                       // written by this block before the barriers above
    out[n_scalar + i] = M > 0.0 ? v / M : 0.0;
  }
}

inline int64_t max_blocks(int64_t n, int n_scans) { return n / kLossBlock + n_scans; }      // >= sum_s ceil(n_s / 128)

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
  if (dtype != DC_F32 && dtype != DC_F64) return DC_ERR_DTYPE;
  if (max_dist != max_dist) return DC_ERR_ARG;
  if (model_kind < DC_MODEL_NONE || model_kind > DC_MODEL_LAST) return DC_ERR_ARG;
  if (model_kind != DC_MODEL_NONE) {
    if (n_terms < 1 || n_terms > DC_MAX_MODEL_TERMS || !w || !e || (n > 0 && !inc)) return DC_ERR_ARG;
    if (model_kind == DC_MODEL_LINEAR && n_terms != 3) return DC_ERR_ARG;
    if ((model_kind == DC_MODEL_INVCOS || model_kind == DC_MODEL_SCALED_INVCOS) && n_terms != 1) return DC_ERR_ARG;
  } else {
    n_terms = 0;
  }
  if (n > 0 && (n_scans < 1 || !dirs || !depth)) return DC_ERR_ARG;
  if (n_scans > 1 && !scan_ptr) return DC_ERR_ARG;
  const int64_t rows = max_blocks(n, n_scans);
  if (rows > 0x7fffffff) return DC_ERR_UNSUPPORTED;
  if (n > 0 && (!ws || ws_bytes < dc_mesh_loss_workspace_bytes(n, n_scans, n_terms))) return DC_ERR_WORKSPACE;
  double* partials = (double*)ws;
  if (n > 0) {
    // the walk prunes with d^2: the bound squared, one part in 2^50 up so that its rounding cannot cut a face at exactly max_dist
    // (sqrt(d^2) <= max_dist decides in the end), as in dc_mesh_closest
    const bool bounded = max_dist > 0.0 && max_dist < INFINITY;
    const double limit2 = bounded ? max_dist * max_dist * (1.0 + 0x1p-50) : INFINITY;
    const double md = bounded ? max_dist : 0.0;
    PointInputs in;
    in.vps = vps; in.dirs = dirs; in.depth = depth; in.inc = inc; in.lmask = lmask; in.scan_id = nullptr;
    in.poses = poses; in.w = w; in.e = e; in.model_kind = model_kind; in.n_terms = n_terms; in.n_scans = n_scans;
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
  mesh_loss_finish_kernel<<<1, kFinishBlock, 0, (hipStream_t)stream>>>(partials, n_terms, scan_ptr, n, n_scans, rows, out);
  DC_HIP(hipGetLastError());
  return DC_OK;
}

}  // extern "C"
