// The scan-shadow test of one ray against the rays it meets (filters.py:257-309), shared by the two kernels that find a ray's
// direction neighbours themselves: shadow_group_kernel (dc_knn.hip, a walk over the direction grid) and image_shadow_kernel
// (dc_rangeimage.hip, a walk over an image window).  Device only.
//   membership   sqdist of the fp64 copies of the two directions <= r^2 (cKDTree's squared distance: products and sums
//                individually rounded, in axis order) -- radius_kernel's inclusion test
//   pair test    the cosine of the angle between the ray back to the viewpoint (o - x) and the vector to the neighbour (x_j - x), in
//                the cloud's dtype and in torch's operation order (see shadow_mask_kernel, dc_filters.hip).  The extreme ANGLES are
//                the arc cosines of the extreme COSINES: the walk keeps the largest and the smallest cosine; a cosine an ulp outside
//                [-1, 1] or a NaN -- whose arc cosine is NaN in the reference's row -- removes the ray.  The ray itself is met like
//                any other: its vector is zero, its cosine 0.
#pragma once
#include "dc_common.h"

namespace dc {

// cKDTree's squared distance: products and sums individually rounded, in axis order.
__device__ __forceinline__ double sqdist(const double* a, const double* b) {
  const double d0 = a[0] - b[0], d1 = a[1] - b[1], d2 = a[2] - b[2];
  double s = __dmul_rn(d0, d0);
  s = __dadd_rn(s, __dmul_rn(d1, d1));
  s = __dadd_rn(s, __dmul_rn(d2, d2));
  return s;
}

template <typename T>
struct ShadowRay {
  T xi0, xi1, xi2;      // the ray's end point
  T a0, a1, a2;         // unit vector back to its viewpoint
  T cmax, cmin;         // extreme cosines met so far
  bool bad;
};

template <typename T>
__device__ __forceinline__ void shadow_ray_init(ShadowRay<T>& s, const T* __restrict__ x, const T* __restrict__ vps, int vps_rows, int64_t i) {
#pragma clang fp contract(off)
  const T eps = (T)1e-8;
  s.xi0 = x[i * 3]; s.xi1 = x[i * 3 + 1]; s.xi2 = x[i * 3 + 2];
  const T* o = vps + (vps_rows == 1 ? 0 : i * 3);
  T a0 = o[0] - s.xi0, a1 = o[1] - s.xi1, a2 = o[2] - s.xi2;
  const T na = sqrt(fma(a2, a2, fma(a1, a1, a0 * a0)));       // torch's norm: an fma chain (see shadow_mask_kernel)
  const T da = na > eps ? na : eps;
  s.a0 = a0 / da; s.a1 = a1 / da; s.a2 = a2 / da;
  s.cmax = -(T)INFINITY; s.cmin = (T)INFINITY;
  s.bad = false;
}

// the ray meets its direction neighbour jn
template <typename T>
__device__ __forceinline__ void shadow_ray_meet(ShadowRay<T>& s, const T* __restrict__ x, int64_t jn) {
#pragma clang fp contract(off)
  const T eps = (T)1e-8;
  T b0 = x[jn * 3] - s.xi0, b1 = x[jn * 3 + 1] - s.xi1, b2 = x[jn * 3 + 2] - s.xi2;
  const T nb = sqrt(fma(b2, b2, fma(b1, b1, b0 * b0)));
  const T db = nb > eps ? nb : eps;
  b0 /= db; b1 /= db; b2 /= db;
  const T cs = s.a0 * b0 + s.a1 * b1 + s.a2 * b2;
  s.bad = s.bad || !(cs >= (T)-1 && cs <= (T)1);
  s.cmax = cs > s.cmax ? cs : s.cmax;
  s.cmin = cs < s.cmin ? cs : s.cmin;
}

// kept: every angle within [lo, hi].  A ray that met no neighbour at all (not even itself: non-finite direction) has an all-fill
// row in the reference: kept.
template <typename T>
__device__ __forceinline__ bool shadow_ray_kept(T cmin, T cmax, bool bad, T lo, T hi) {
  const bool none = cmin > cmax;
  const T amin = none ? (T)INFINITY : (T)acos(cmax), amax = none ? -(T)INFINITY : (T)acos(cmin);
  return !bad && (amin > amax ? lo <= hi : (amin >= lo && amax <= hi));
}

}  // namespace dc
