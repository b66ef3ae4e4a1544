// What every user of the LBVH of dc_raycast.hip shares, ONE copy each: the depth-first walk (bvh_walk), the bottom-up box fit of the
// build (bvh_fit_climb) and the scan lookup of the per-scan kernels (scan_of).  Node numbering: internal nodes 0 .. n-2 (root 0), leaf i
// is node n-1+i; with one primitive the root is leaf 0 and `child` has no rows.
//
// The visitor of bvh_walk holds the query and the state of the search (the best hit so far, say) and supplies
//     bool enter(int64_t node, float& key)   is the box of `node` admitted under the visitor's CURRENT bound?  `key` orders an admitted
//                                            node against its sibling (the smaller key first, the first child on a tie);
//     void leaf(int64_t leaf)                folds primitive `leaf` (a row of the leaf arrays) into the state.
// enter is asked for the root, for both children of a visited inner node, and again for a postponed node when it is popped.  It answers
// with a bool, not a sentinel key: the nearest-triangle walk admits a box whose bound is +inf while its best is +inf.  When enter never
// rejects a box that holds a primitive leaf would still accept, the state after the walk is the state after leaf over EVERY primitive,
// whatever the tree and the order of the visits.
#pragma once
#include "dc_common.h"

namespace dc {

// Per-lane stack: int32 [kBvhStackDepth * BLOCK] in LDS, lane-minor (a wavefront's pushes hit 64 distinct banks).  The build's trees
// are at most 63 deep, so a walk never holds more than 63 postponed nodes.
constexpr int kBvhStackDepth = 64;

// Depth-first from the root, the child with the smaller key first and the other on this lane's stack (stack[sp * BLOCK + lane]).
// n = number of primitives (leaves are the nodes n - 1 .. 2 n - 2).  No barrier inside: lanes of a block may call it or not.
// Precondition: depth <= 63 (past it a push is dropped and its pop reads node 0: no access outside the stack, no other promise).
// The descent is a loop of its own on purpose: as one loop with a `continue` the walk compiles 2 - 5 % slower (DESIGN "One tree walk").
template <int BLOCK, typename Visitor>
DC_HD void bvh_walk(const int32_t* __restrict__ child, int64_t n, int32_t* stack, int lane, Visitor& vis) {
  int sp = 0;
  int64_t node = 0;
  float key;
  bool live = vis.enter(0, key);
  while (live) {
    while (live && node < n - 1) {                       // down to a leaf, or to a node neither child of which is admitted
      const int64_t ca = child[2 * node], cb = child[2 * node + 1];
      float ka, kb;
      const bool go_a = vis.enter(ca, ka), go_b = vis.enter(cb, kb);
      if (go_a && go_b) {
        const bool a_first = ka <= kb;
        if (sp < kBvhStackDepth) stack[sp * BLOCK + lane] = (int32_t)(a_first ? cb : ca);
        ++sp;
        node = a_first ? ca : cb;
      } else {
        node = go_a ? ca : cb;
        live = go_a || go_b;
      }
    }
    if (live) vis.leaf(node - (n - 1));
    // next postponed node that the bound of now still admits
    live = false;
    while (sp > 0) {
      --sp;
      node = sp < kBvhStackDepth ? stack[sp * BLOCK + lane] : 0;
      if (vis.enter(node, key)) { live = true; break; }
    }
  }
}

// The scan of row g: the last s in [0, n_scans) with scan_offset[s] <= g, scan 0 when there is none; clamped to [0, n_scans), so
// offsets that do not span [0, n] cannot move a read outside a per-scan array.
DC_HD int scan_of(const int64_t* __restrict__ scan_offset, int n_scans, int64_t g) {
  int lo = 0, hi = n_scans;
  while (hi - lo > 1) {
    const int mid = lo + (hi - lo) / 2;
    if (scan_offset[mid] <= g) lo = mid; else hi = mid;
  }
  return lo;
}

#if defined(__HIPCC__)
__device__ __forceinline__ float load_box(const float* p) {
  return __uint_as_float(__hip_atomic_load((const uint32_t*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}

// Bottom-up fit of the build: the lane that wrote the box of `node` (a leaf) climbs; one counter per internal node lets the second
// child that arrives form the parent's box, the exact min / max of its children's -- bit-identical for any arrival order.
__device__ __forceinline__ void bvh_fit_climb(int64_t node, const int32_t* __restrict__ child, const int32_t* __restrict__ parent,
                                              int32_t* __restrict__ counter, float* node_box) {
  node = parent[node];
  while (node >= 0) {
    __threadfence();                                        // this child's box is visible before the counter says so
    if (atomicAdd(&counter[node], 1) == 0) return;          // the sibling is still on its way: it fits the parent
    __threadfence();
    const int64_t a0 = child[2 * node], b0 = child[2 * node + 1];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      node_box[6 * node + a] = fminf(load_box(node_box + 6 * a0 + a), load_box(node_box + 6 * b0 + a));
      node_box[6 * node + 3 + a] = fmaxf(load_box(node_box + 6 * a0 + 3 + a), load_box(node_box + 6 * b0 + 3 + a));
    }
    node = parent[node];
  }
}
#endif

}  // namespace dc
