// The nearest-triangle walk over the LBVH of dc_raycast.hip, shared by dc_mesh_closest (dc_meshdist.hip) and dc_mesh_loss
// (dc_meshloss.hip): ONE copy of the box bound, of the leaf test with its tie rule and of the depth-first loop, so the two entry
// points cannot drift apart.  The rule and the derivation of the fp32 box bound are in dc_meshdist.hip's header comment.
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
#include "dc_trimath.h"
#include <float.h>

namespace dc {

constexpr int kWalkStackDepth = 64;      // per-lane stack in LDS, lane-minor: int32 [kWalkStackDepth * BLOCK]

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

// Depth-first from the root with the nearer child first and the other on this lane's stack (stack[sp * BLOCK + lane]); n = number of
// faces (leaves are the nodes n - 1 .. 2 n - 2).  No barrier inside: lanes of a block may call it or not.
template <int BLOCK>
__device__ __forceinline__ void mesh_walk(const int32_t* __restrict__ child, const float* __restrict__ node_box,
                                          const double* __restrict__ leaf_tri, const int32_t* __restrict__ leaf_face, int64_t n,
                                          const double* p, const Query32& q, int32_t* stack, int lane, double& best, int32_t& best_face,
                                          int64_t& best_leaf) {
  int sp = 0;
  int64_t node = 0;
  bool live = box_bound(node_box, 0, q) <= __double2float_ru(best);
  while (live) {
    if (node >= n - 1) {
      mesh_walk_leaf(leaf_tri, leaf_face, node - (n - 1), p, best, best_face, best_leaf);
    } else {
      const float lim = __double2float_ru(best);
      const int64_t ca = child[2 * node], cb = child[2 * node + 1];
      const float ba = box_bound(node_box, ca, q), bb = box_bound(node_box, cb, q);
      const bool go_a = ba <= lim, go_b = bb <= lim;
      if (go_a || go_b) {
        if (go_a && go_b) {
          const bool a_first = ba <= bb;
          if (sp < kWalkStackDepth) stack[sp * BLOCK + lane] = (int32_t)(a_first ? cb : ca);     // sp < 64 always (depth <= 63)
          ++sp;
          node = a_first ? ca : cb;
        } else {
          node = go_a ? ca : cb;
        }
        continue;
      }
    }
    // next postponed node whose box may still hold a face as near as the best one
    live = false;
    while (sp > 0) {
      --sp;
      node = sp < kWalkStackDepth ? stack[sp * BLOCK + lane] : 0;
      if (box_bound(node_box, node, q) <= __double2float_ru(best)) { live = true; break; }
    }
  }
}

}  // namespace dc
