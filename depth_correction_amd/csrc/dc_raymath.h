// Per-ray arithmetic of the BVH ray caster (dc_raycast.hip), host and device: the outward-rounded leaf boxes, the ray set-up, the
// fp32 slab test with its pruning rule and the fp64 watertight triangle test.  The kernels and the host build (dc_hostcheck.cpp)
// perform the same rounded operations and give the same bits: no fused multiply-adds in the triangle test, and the two directed
// roundings fp64 -> fp32 have a host twin built from round-to-nearest and one step of nextafterf.
//
// What the pieces promise together (pinned by tests/test_raycast_host.py and tests/test_gpu_raycast_edge.py):
//   1. box_entry never rejects a box that holds a face test_triangle reports a hit on, neither with t_far = +inf nor with
//      t_far = prune_far(t) for the t of that hit, for the face's own leaf box and for every box around it;
//   2. so the traversal returns what test_triangle applied to every face in index order returns (the smallest t, on equal t the
//      lower face index), whatever the tree looks like and whatever order it is walked in;
//   3. a ray through a shared edge or vertex hits at least one of the faces around it.
#pragma once
#include "dc_common.h"
#include <math.h>

namespace dc {

// fp64 -> fp32 rounded towards -inf / +inf (inf and NaN pass through)
DC_HD float f32_rd(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __double2float_rd(x);
#else
  const float f = (float)x;
  return (double)f > x ? nextafterf(f, -INFINITY) : f;
#endif
}

DC_HD float f32_ru(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __double2float_ru(x);
#else
  const float f = (float)x;
  return (double)f < x ? nextafterf(f, INFINITY) : f;
#endif
}

// leaf box of the triangle v [9]: box[a] <= every vertex's coordinate a <= box[3 + a], the tightest fp32 numbers that do
DC_HD void leaf_box(const double* v, float* box) {
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    box[a] = f32_rd(fmin(fmin(v[a], v[3 + a]), v[6 + a]));
    box[3 + a] = f32_ru(fmax(fmax(v[a], v[3 + a]), v[6 + a]));
  }
}

struct Ray32 {
  float o[3], inv[3], margin;
};

struct Hit {
  double t, u, v;
  int32_t face;
  int32_t leaf;                 // the winning leaf (row of leaf_tri), -1 without a hit
};

// A ray in the frame of the watertight test: axes permuted to (kx, ky, kz), kz the dominant one.  Scalars only: the compiler turns
// a select between elements of a private array into a runtime index, and a runtime-indexed private array lives in scratch memory.
struct Ray64 {
  double d0, d1, d2;            // direction (world frame), for the culling test
  double ox, oy, oz;            // origin, permuted
  double sx, sy, sz;            // shear constants
  int kx, ky, kz;
};

DC_HD double pick(int k, double a, double b, double c) { return k == 0 ? a : (k == 1 ? b : c); }

// A direction component below kRayMinDir counts as +-kRayMinDir in the slab test, and the boxes grow by at least kRayMinMargin.  A
// ray that runs parallel to a slab exactly on its boundary (an axis-parallel ray from the world origin along a tessellation line, or
// in the plane of a flat box) then leaves the slab at t = kRayMinMargin / kRayMinDir = 1e10 at the earliest, farther than any hit;
// inside the slab by more than that margin the exit is later still, outside it the entry lies beyond 1e10 as well.
constexpr float kRayMinDir = 1e-30f;
constexpr float kRayMinMargin = 1e-20f;

// the two forms of the ray (origin o, direction d, fp64 world frame) the tests below take
DC_HD void ray_setup(double d0, double d1, double d2, double o0, double o1, double o2, Ray64& ray64, Ray32& ray) {
  ray64.d0 = d0;
  ray64.d1 = d1;
  ray64.d2 = d2;
  // watertight test set-up: kz = dominant axis, (kx, ky) keep the winding
  const double ad0 = fabs(ray64.d0), ad1 = fabs(ray64.d1), ad2 = fabs(ray64.d2);
  const int kz = ad0 >= ad1 ? (ad0 >= ad2 ? 0 : 2) : (ad1 >= ad2 ? 1 : 2);
  int kx = kz == 2 ? 0 : kz + 1, ky = kx == 2 ? 0 : kx + 1;
  const double dz = pick(kz, ray64.d0, ray64.d1, ray64.d2);
  if (dz < 0.0) { const int s = kx; kx = ky; ky = s; }
  ray64.kx = kx;
  ray64.ky = ky;
  ray64.kz = kz;
  ray64.sz = 1.0 / dz;
  ray64.sx = pick(kx, ray64.d0, ray64.d1, ray64.d2) * ray64.sz;
  ray64.sy = pick(ky, ray64.d0, ray64.d1, ray64.d2) * ray64.sz;
  ray64.ox = pick(kx, o0, o1, o2);
  ray64.oy = pick(ky, o0, o1, o2);
  ray64.oz = pick(kz, o0, o1, o2);
  const double oo[3] = {o0, o1, o2}, dd[3] = {ray64.d0, ray64.d1, ray64.d2};
  float omax = 0.0f;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    ray.o[a] = (float)oo[a];
    omax = fmaxf(omax, fabsf(ray.o[a]));
    float da = (float)dd[a];
    if (fabsf(da) < kRayMinDir) da = copysignf(kRayMinDir, da);
    ray.inv[a] = 1.0f / da;
  }
  ray.margin = fmaxf(omax * 0x1p-22f, kRayMinMargin);
}

// The t_far with which the traversal prunes once the best hit so far lies at t (+inf: nothing found yet).  box_entry's entry distance
// is an fp32 product of a rounded difference and a rounded reciprocal: for a box of no thickness met face-on it exceeds the exact
// hit distance by up to a few 2^-24 relative, so the bound gets the slack the exit distance has.  Without it a face whose own t is
// <= the best t can be pruned: the tie rule breaks, and closest hit itself for two hits within 1e-7 relative.
DC_HD float prune_far(double t) { return f32_ru(t) * (1.0f + 0x1p-20f); }

// entry distance of the box b [6] (>= 0), or +inf when the ray misses it before t_far
DC_HD float box_entry(const float* __restrict__ b, const Ray32& r, float t_far) {
  float tn = 0.0f, tf = t_far;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float t0 = (b[a] - r.margin - r.o[a]) * r.inv[a];
    const float t1 = (b[3 + a] + r.margin - r.o[a]) * r.inv[a];
    tn = fmaxf(tn, fminf(t0, t1));
    tf = fminf(tf, fmaxf(t0, t1) * (1.0f + 0x1p-20f));
  }
  return tn <= tf ? tn : INFINITY;
}

// Woop, Benthin, Wald 2013 in fp64; t, u (weight of v1), v (weight of v2) of a hit with t > t_min that beats `best`
DC_HD void test_triangle(const double* __restrict__ tri, int32_t face, int32_t leaf, const Ray64& r, double t_min, bool cull, Hit& best) {
  // no fused multiply-adds here: watertightness needs the edge function of a shared edge to be computed as the exact negation
  // of the neighbour's (fl(a b) - fl(c d) = -(fl(c d) - fl(a b)); fma(a, b, -fl(c d)) is not -fma(c, d, -fl(a b)))
#pragma clang fp contract(off)
  const double t0 = tri[0], t1 = tri[1], t2 = tri[2], t3 = tri[3], t4 = tri[4], t5 = tri[5], t6 = tri[6], t7 = tri[7], t8 = tri[8];
  const double Az = pick(r.kz, t0, t1, t2) - r.oz, Bz = pick(r.kz, t3, t4, t5) - r.oz, Cz = pick(r.kz, t6, t7, t8) - r.oz;
  const double Ax = (pick(r.kx, t0, t1, t2) - r.ox) - r.sx * Az, Ay = (pick(r.ky, t0, t1, t2) - r.oy) - r.sy * Az;
  const double Bx = (pick(r.kx, t3, t4, t5) - r.ox) - r.sx * Bz, By = (pick(r.ky, t3, t4, t5) - r.oy) - r.sy * Bz;
  const double Cx = (pick(r.kx, t6, t7, t8) - r.ox) - r.sx * Cz, Cy = (pick(r.ky, t6, t7, t8) - r.oy) - r.sy * Cz;
  const double U = Cx * By - Cy * Bx, V = Ax * Cy - Ay * Cx, W = Bx * Ay - By * Ax;
  if ((U < 0.0 || V < 0.0 || W < 0.0) && (U > 0.0 || V > 0.0 || W > 0.0)) return;
  const double det = U + V + W;
  if (det == 0.0) return;
  const double T = U * (r.sz * Az) + V * (r.sz * Bz) + W * (r.sz * Cz);
  const double t = T / det;
  if (!(t > t_min) || t > best.t || (t == best.t && face >= best.face)) return;
  if (cull) {
    const double e10 = t3 - t0, e11 = t4 - t1, e12 = t5 - t2, e20 = t6 - t0, e21 = t7 - t1, e22 = t8 - t2;
    const double nd = (e11 * e22 - e12 * e21) * r.d0 + (e12 * e20 - e10 * e22) * r.d1 + (e10 * e21 - e11 * e20) * r.d2;
    if (!(nd < 0.0)) return;
  }
  best.t = t;
  best.u = V / det;
  best.v = W / det;
  best.face = face;
  best.leaf = leaf;
}

// The closest-hit search as a visitor of bvh_walk (dc_bvh.h): a box is admitted when the ray enters it before prune_far of the best
// hit so far, the entry distance orders the children, a leaf is test_triangle.  Set the rays with ray_setup and best to a miss.
struct TriVisitor {
  const float* __restrict__ node_box;
  const double* __restrict__ leaf_tri;
  const int32_t* __restrict__ leaf_face;
  double t_min; bool cull;
  Ray64 ray64;                  // the three below: set by the caller (ray_setup, no_hit) before the walk
  Ray32 ray;
  Hit best;

  DC_HD bool enter(int64_t node, float& key) const {
    key = box_entry(node_box + 6 * node, ray, prune_far(best.t));
    return key < INFINITY;
  }
  DC_HD void leaf(int64_t leaf) { test_triangle(leaf_tri + 9 * leaf, leaf_face[leaf], (int32_t)leaf, ray64, t_min, cull, best); }
};

DC_HD Hit no_hit() { return Hit{INFINITY, 0.0, 0.0, -1, -1}; }

}  // namespace dc
