// The nearest-triangle walk over the LBVH of dc_raycast.hip, shared by dc_mesh_closest (dc_meshdist.hip) and dc_mesh_loss
// (dc_meshloss.hip): ONE copy of the box bound and of the leaf test with its tie rule, so the two entry points cannot drift apart; the
// depth-first loop is dc::bvh_walk (dc_bvh.h), the ray casts' too.  The rule and the derivation of the fp32 box bound are in dc_meshdist.hip's header comment.
//
// State of a walk: best (d^2 of the best face so far, or the caller's bound before the first), best_face (mesh numbering, -1 = none)
// and best_leaf (its leaf, what closest_on_triangle is run on again for the closest point).  mesh_walk_leaf folds one leaf into the
// state -- the smallest d^2 wins, equal d^2 the lower face index, a NaN never -- and mesh_walk visits every node whose bound is not
// above the state's best.  The result is the lexicographic minimum of (d^2, face) over the faces with d^2 <= the initial best and
// does not depend on the order of the visits: a state that some leaves were folded into BEFORE the walk (dc_mesh_loss's hint)
// only prunes more, it never changes the answer -- a box whose bound EQUALS best is still visited, so a face at exactly the best
// distance with a lower index is still seen.
#pragma once
#include "dc_common.h"
#include "dc_bvh.h"
#include "dc_trimath.h"
#include <float.h>

namespace dc {

struct Query32 {
  float p[3], margin;
};

// the query rounded to fp32 (clamped to the fp32 range) and the margin of the box bound
__device__ __forceinline__ Query32 mesh_query(const double* p) {
  Query32 q;
  float pmax = 0.0f;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    q.p[a] = fminf(fmaxf((float)p[a], -FLT_MAX), FLT_MAX);
    pmax = fmaxf(pmax, fabsf(q.p[a]));
  }
  q.margin = fmaxf(pmax * 0x1p-23f, 1e-30f);
  return q;
}

// lower bound of the squared distance from the query to the box of `node` (derivation: dc_meshdist.hip's header)
__device__ __forceinline__ float box_bound(const float* __restrict__ node_box, int64_t node, const Query32& q) {
  const float* b = node_box + 6 * node;
  float s = 0.0f;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float g = fmaxf(fmaxf(b[a] - q.p[a], q.p[a] - b[3 + a]), 0.0f);
    const float h = fmaxf(g - q.margin, 0.0f);
    s = __fadd_rn(s, __fmul_rn(h, h));             // explicit roundings: the derivation counts them (no contraction)
  }
  return __fmul_rn(s, 1.0f - 0x1p-20f);
}

// one leaf folded into the state
__device__ __forceinline__ void mesh_walk_leaf(const double* __restrict__ leaf_tri, const int32_t* __restrict__ leaf_face, int64_t leaf,
                                               const double* p, double& best, int32_t& best_face, int64_t& best_leaf) {
  double tri[9], c[3];
#pragma unroll
  for (int k = 0; k < 9; ++k) tri[k] = leaf_tri[9 * leaf + k];
  const double d2 = closest_on_triangle(tri, p, c, nullptr);
  const int32_t face = leaf_face[leaf];
  if (d2 < best || (d2 == best && (best_face < 0 || face < best_face))) {      // a NaN never wins
    best = d2;
    best_face = face;
    best_leaf = leaf;
  }
}

// The walk as a visitor of bvh_walk (dc_bvh.h): a box is admitted when its bound is not above the best d^2 (rounded up to fp32), the
// bound orders the children, a leaf is mesh_walk_leaf.
struct MeshVisitor {
  const float* __restrict__ node_box;
  const double* __restrict__ leaf_tri;
  const int32_t* __restrict__ leaf_face;
  const double* p; const Query32& q;
  double& best;                 // best, best_face, best_leaf: the state of the header comment
  int32_t& best_face;
  int64_t& best_leaf;

  __device__ __forceinline__ bool enter(int64_t node, float& key) const {
    key = box_bound(node_box, node, q);
    return key <= __double2float_ru(best);
  }
  __device__ __forceinline__ void leaf(int64_t leaf) { mesh_walk_leaf(leaf_tri, leaf_face, leaf, p, best, best_face, best_leaf); }
};

// n = number of faces; stack: int32 [kBvhStackDepth * BLOCK] in LDS.  No barrier inside: lanes of a block may call it or not.
template <int BLOCK>
__device__ __forceinline__ void mesh_walk(const int32_t* __restrict__ child, const float* __restrict__ node_box,
                                          const double* __restrict__ leaf_tri, const int32_t* __restrict__ leaf_face, int64_t n,
                                          const double* p, const Query32& q, int32_t* stack, int lane, double& best, int32_t& best_face,
                                          int64_t& best_leaf) {
  MeshVisitor vis = {node_box, leaf_tri, leaf_face, p, q, best, best_face, best_leaf};
  bvh_walk<BLOCK>(child, n, stack, lane, vis);
}

}  // namespace dc
