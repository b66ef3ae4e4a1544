// Map accuracy against a triangle mesh: the exact distance from every query point to the nearest triangle (dc_mesh_closest), over the
// LBVH of dc_raycast.hip, and area-weighted sampling of points from a mesh (dc_mesh_sample).  The reference holds a map against a
// surveyed ground-truth cloud (scripts/mapping_accuracy:82-118); with rendered-mesh datasets the ground truth is the mesh itself.
//
// dc_mesh_closest: one lane per query, one launch, no workspace.  Depth-first walk with the nearer child first and the other on a
// per-lane stack in LDS (depth 64, lane-minor: the layout of raycast_kernel); the walk itself is dc_meshwalk.h's, which dc_mesh_loss
// shares.  A node is visited only while a LOWER BOUND of the squared distance from the query to its box is not above the best
// squared distance so far.  Triangles are tested in fp64
// (dc_trimath.h); the smallest d^2 wins, equal d^2 the lower face index, so the result does not depend on the traversal order.
//
// The box bound, in fp32 (next to the ray rule in dc_raycast.hip's header: no box a ray touches is rejected; here: no box that holds
// the nearest triangle is skipped).  u = 2^-24 is the unit roundoff.  The boxes are exact fp32 numbers that contain their faces.
// The query p (fp64) is rounded to pf, |pf_a - p_a| <= u |p_a| (a query beyond the fp32 range is clamped to +-FLT_MAX, which only
// moves it toward every box).  Per axis the true gap is g = max(lo - p, p - hi, 0) and the computed one
//     gc = max(fl(lo - pf), fl(pf - hi), 0) <= (g + u |p_a|) (1 + u).
// With m = 2^-23 max_a |pf_a| >= u |p_a| (1 + u) (twice what is needed; m is a power-of-two multiple of a float: exact) the reduced gap
//     h = max(fl(gc - m), 0) <= g (1 + u)^2:
// gc - m <= (g + u|p_a|)(1 + u) - m <= g (1 + u), and the subtraction rounds once more.  The bound is
//     b = fl(fl(fl(fl(h0 h0) + fl(h1 h1)) + fl(h2 h2)) (1 - 2^-20)):
// three squarings, two additions and the final product contribute (1 + u)^4 on top of the (1 + u)^4 of the squared gaps, so
// b <= |g|^2 (1 + u)^8 (1 - 2^-20) < |g|^2, because (1 + u)^8 < 1 + 2^-20 (8 u = 2^-21: a factor two of headroom).  |g|^2 is the exact
// squared distance to the box, which is not above the squared distance to any triangle inside it.  b is compared with the best d^2
// rounded UP to fp32 (__double2float_ru, as the cast does with best.t), and a box whose bound EQUALS it is still visited: a face at
// exactly the best distance with a lower index has to be seen for the tie rule.
//
// dc_mesh_sample: sample i is a pure function of (mesh, seed, i) -- three splitmix64 uniforms, a binary search in the inclusive
// prefix sum of the face areas, the square-root parametrisation of the triangle (dc_trimath.h) -- bit-equal to the numpy
// restatement in tests/mesh_reference.py whatever the launch shape.
#include "dc_common.h"
#include "dc_hostutil.h"
#include "dc_trimath.h"
#include "dc_meshwalk.h"
#include "../../include/dc_hip.h"

namespace {

constexpr int kClosestBlock = 128;
constexpr int kSampleBlock = 256;

template <typename T>
__global__ void __launch_bounds__(kClosestBlock) mesh_closest_kernel(const int32_t* __restrict__ child, const float* __restrict__ node_box,
                                                                    const double* __restrict__ leaf_tri, const int32_t* __restrict__ leaf_face,
                                                                    int64_t n, const T* __restrict__ points, int64_t n_points, double limit2,
                                                                    double max_dist, int32_t* __restrict__ face_out,
                                                                    double* __restrict__ dist_out, double* __restrict__ closest_out) {
  __shared__ int32_t stack[dc::kBvhStackDepth * kClosestBlock];
  const int lane = threadIdx.x;
  const int64_t g = (int64_t)blockIdx.x * kClosestBlock + lane;
  if (g >= n_points) return;
  const double p[3] = {(double)points[3 * g], (double)points[3 * g + 1], (double)points[3 * g + 2]};
  double best = limit2;                            // d^2 of the best face so far (the max_dist bound before the first)
  int32_t best_face = -1;
  int64_t best_leaf = -1;
  if (isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2])) {
    const dc::Query32 q = dc::mesh_query(p);
    dc::mesh_walk<kClosestBlock>(child, node_box, leaf_tri, leaf_face, n, p, q, stack, lane, best, best_face, best_leaf);
  }
  double dist = INFINITY, c[3] = {NAN, NAN, NAN};
  if (best_face >= 0) {
    dist = __dsqrt_rn(best);
    if (max_dist > 0.0 && !(dist <= max_dist)) {
      best_face = -1;
      dist = INFINITY;
    } else if (closest_out) {
      double tri[9];
#pragma unroll
      for (int k = 0; k < 9; ++k) tri[k] = leaf_tri[9 * best_leaf + k];
      dc::closest_on_triangle(tri, p, c, nullptr);   // the winning face again: the same operations, the same point
    }
  }
  face_out[g] = best_face;
  dist_out[g] = dist;
  if (closest_out) {
    closest_out[3 * g] = c[0];
    closest_out[3 * g + 1] = c[1];
    closest_out[3 * g + 2] = c[2];
  }
}

__global__ void __launch_bounds__(kSampleBlock) mesh_sample_kernel(const double* __restrict__ verts, const int32_t* __restrict__ faces,
                                                                   int64_t n_faces, const double* __restrict__ area_cdf, int64_t n_samples,
                                                                   int64_t seed, int32_t* __restrict__ face_out, double* __restrict__ points_out) {
  const int64_t i = (int64_t)blockIdx.x * kSampleBlock + threadIdx.x;
  if (i >= n_samples) return;
  double u[3], tri[9], p[3];
  dc::mesh_sample_uniforms(seed, i, u);
  const int64_t f = dc::mesh_sample_face(area_cdf, n_faces, u[0]);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int64_t v = faces[3 * f + c];
#pragma unroll
    for (int a = 0; a < 3; ++a) tri[3 * c + a] = verts[3 * v + a];
  }
  dc::mesh_sample_point(tri, u[1], u[2], p);
  face_out[i] = (int32_t)f;
  points_out[3 * i] = p[0];
  points_out[3 * i + 1] = p[1];
  points_out[3 * i + 2] = p[2];
}

inline unsigned grid_of(int64_t n, int block) { return (unsigned)((n + block - 1) / block); }

}  // namespace

extern "C" {

int dc_mesh_closest(const int32_t* child, const float* node_box, const double* leaf_tri, const int32_t* leaf_face, int64_t n_faces,
                    const void* points, int dtype, int64_t n_points, double max_dist, int32_t* face_out, double* dist_out,
                    double* closest_out, dcStream_t stream) {
  if (n_faces < 1 || n_points < 0 || !node_box || !leaf_tri || !leaf_face || (n_faces > 1 && !child)) return DC_ERR_ARG;
  if (dtype != DC_F32 && dtype != DC_F64) return DC_ERR_DTYPE;
  if (max_dist != max_dist) return DC_ERR_ARG;
  if (n_points == 0) return DC_OK;
  if (!points || !face_out || !dist_out) return DC_ERR_ARG;
  if (n_points > (int64_t)kClosestBlock * 0x7fffffff) return DC_ERR_UNSUPPORTED;
  // the walk prunes with d^2: the bound squared, one part in 2^50 up so that its rounding cannot cut a face at exactly max_dist
  // (sqrt(d^2) <= max_dist decides in the end)
  const bool bounded = max_dist > 0.0 && max_dist < INFINITY;
  const double limit2 = bounded ? max_dist * max_dist * (1.0 + 0x1p-50) : INFINITY;
  const double md = bounded ? max_dist : 0.0;
  const unsigned grid = grid_of(n_points, kClosestBlock);
  if (dtype == DC_F32)
    mesh_closest_kernel<float><<<grid, kClosestBlock, 0, (hipStream_t)stream>>>(child, node_box, leaf_tri, leaf_face, n_faces,
                                                                                (const float*)points, n_points, limit2, md, face_out,
                                                                                dist_out, closest_out);
  else
    mesh_closest_kernel<double><<<grid, kClosestBlock, 0, (hipStream_t)stream>>>(child, node_box, leaf_tri, leaf_face, n_faces,
                                                                                 (const double*)points, n_points, limit2, md, face_out,
                                                                                 dist_out, closest_out);
  DC_HIP(hipGetLastError());
  return DC_OK;
}

int dc_mesh_sample(const double* verts, const int32_t* faces, int64_t n_faces, const double* area_cdf, int64_t n_samples, int64_t seed,
                   int32_t* face_out, double* points_out, dcStream_t stream) {
  if (n_faces < 1 || n_samples < 0 || !verts || !faces || !area_cdf) return DC_ERR_ARG;
  if (n_samples == 0) return DC_OK;
  if (!face_out || !points_out) return DC_ERR_ARG;
  if (n_samples > (int64_t)kSampleBlock * 0x7fffffff) return DC_ERR_UNSUPPORTED;
  mesh_sample_kernel<<<grid_of(n_samples, kSampleBlock), kSampleBlock, 0, (hipStream_t)stream>>>(verts, faces, n_faces, area_cdf, n_samples,
                                                                                                seed, face_out, points_out);
  DC_HIP(hipGetLastError());
  return DC_OK;
}

}  // extern "C"
