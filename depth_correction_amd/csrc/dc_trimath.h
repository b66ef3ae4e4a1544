// Per-triangle arithmetic of the map-accuracy kernels (dc_meshdist.hip), host and device: the closest point of a triangle to a
// query point and one area-weighted sample of a mesh.  Everything here is fp64 with contraction switched off, so that the kernel
// and the host build (dc_hostcheck.cpp) perform the same rounded operations and give the same bits.
//
// closest_on_triangle: the Voronoi-region method of Ericson, "Real-Time Collision Detection" 5.1.5 -- the three vertex regions,
// the three edge regions, then the interior (the foot of the perpendicular on the plane).  A query exactly over an edge or a
// vertex gets the same point whichever branch takes it (the edge parameter is then exactly 0 or 1 times the edge).  Thin
// triangles: with s = |ab x ac| / (|ab| |ac|) the region tests (differences of products of dot products) carry a relative error
// of about 2^-52 / s^2, so below s = 2^-30 they say nothing; such a triangle (collinear or coincident vertices included) is
// treated as its three edges, the closest of the three point-segment answers (first of ab, bc, ca on equal distance).  That is
// exact for a degenerate triangle and off by at most the triangle's width, s times its longest edge, otherwise.  The same path
// takes over when the region tests contradict each other (no edge or vertex region, yet not all of va, vb, vc positive): the
// closest point is then on the boundary, which the three segments cover.  Every result is finite for finite input: no division
// by a zero length is made.
#pragma once
#include "dc_common.h"
#include "dc_rng.h"
#include <math.h>

namespace dc {

// region codes of closest_on_triangle (tests; the kernel ignores them)
enum { kTriVertexA = 0, kTriVertexB = 1, kTriVertexC = 2, kTriEdgeAB = 3, kTriEdgeCA = 4, kTriEdgeBC = 5, kTriInterior = 6, kTriThin = 7 };

// closest point of the segment [a, b] to p -> q, returns |p - q|^2
DC_HD double closest_on_segment(const double* a, const double* b, const double* p, double* q) {
#pragma clang fp contract(off)
  const double e0 = b[0] - a[0], e1 = b[1] - a[1], e2 = b[2] - a[2];
  const double ee = (e0 * e0 + e1 * e1) + e2 * e2;
  double t = 0.0;
  if (ee > 0.0) {
    t = (((p[0] - a[0]) * e0 + (p[1] - a[1]) * e1) + (p[2] - a[2]) * e2) / ee;
    t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
  }
  q[0] = a[0] + t * e0;
  q[1] = a[1] + t * e1;
  q[2] = a[2] + t * e2;
  const double d0 = p[0] - q[0], d1 = p[1] - q[1], d2 = p[2] - q[2];
  return (d0 * d0 + d1 * d1) + d2 * d2;
}

// closest point of the triangle tri = (a, b, c) [9] to p -> q, returns |p - q|^2; *region (optional) <- the branch taken
DC_HD double closest_on_triangle(const double* tri, const double* p, double* q, int* region) {
#pragma clang fp contract(off)
  const double* a = tri;
  const double* b = tri + 3;
  const double* c = tri + 6;
  const double ab0 = b[0] - a[0], ab1 = b[1] - a[1], ab2 = b[2] - a[2];
  const double ac0 = c[0] - a[0], ac1 = c[1] - a[1], ac2 = c[2] - a[2];
  const double n0 = ab1 * ac2 - ab2 * ac1, n1 = ab2 * ac0 - ab0 * ac2, n2 = ab0 * ac1 - ab1 * ac0;
  const double nn = (n0 * n0 + n1 * n1) + n2 * n2;
  const double abab = (ab0 * ab0 + ab1 * ab1) + ab2 * ab2, acac = (ac0 * ac0 + ac1 * ac1) + ac2 * ac2;
  int reg = kTriThin;
  bool done = false;
  if (nn > 0x1p-60 * (abab * acac)) {            // s > 2^-30 (false for NaN and for a zero edge)
    done = true;
    const double ap0 = p[0] - a[0], ap1 = p[1] - a[1], ap2 = p[2] - a[2];
    const double d1 = (ab0 * ap0 + ab1 * ap1) + ab2 * ap2, d2 = (ac0 * ap0 + ac1 * ap1) + ac2 * ap2;
    const double bp0 = p[0] - b[0], bp1 = p[1] - b[1], bp2 = p[2] - b[2];
    const double d3 = (ab0 * bp0 + ab1 * bp1) + ab2 * bp2, d4 = (ac0 * bp0 + ac1 * bp1) + ac2 * bp2;
    const double cp0 = p[0] - c[0], cp1 = p[1] - c[1], cp2 = p[2] - c[2];
    const double d5 = (ab0 * cp0 + ab1 * cp1) + ab2 * cp2, d6 = (ac0 * cp0 + ac1 * cp1) + ac2 * cp2;
    const double vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    if (d1 <= 0.0 && d2 <= 0.0) {
      reg = kTriVertexA;
      q[0] = a[0]; q[1] = a[1]; q[2] = a[2];
    } else if (d3 >= 0.0 && d4 <= d3) {
      reg = kTriVertexB;
      q[0] = b[0]; q[1] = b[1]; q[2] = b[2];
    } else if (d6 >= 0.0 && d5 <= d6) {
      reg = kTriVertexC;
      q[0] = c[0]; q[1] = c[1]; q[2] = c[2];
    } else if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {
      reg = kTriEdgeAB;
      const double v = d1 / (d1 - d3);             // d1 > 0 or d3 < 0 here (else a vertex region took it): no 0 / 0
      q[0] = a[0] + v * ab0; q[1] = a[1] + v * ab1; q[2] = a[2] + v * ab2;
    } else if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {
      reg = kTriEdgeCA;
      const double w = d2 / (d2 - d6);
      q[0] = a[0] + w * ac0; q[1] = a[1] + w * ac1; q[2] = a[2] + w * ac2;
    } else if (va <= 0.0 && (d4 - d3) >= 0.0 && (d5 - d6) >= 0.0) {
      reg = kTriEdgeBC;
      const double w = (d4 - d3) / ((d4 - d3) + (d5 - d6));
      q[0] = b[0] + w * (c[0] - b[0]); q[1] = b[1] + w * (c[1] - b[1]); q[2] = b[2] + w * (c[2] - b[2]);
    } else {
      const double sum = (va + vb) + vc;
      if (sum > 0.0 && va >= 0.0 && vb >= 0.0 && vc >= 0.0) {
        reg = kTriInterior;
        // the foot of the perpendicular, p - n (n . ap) / |n|^2, rather than a + v ab + w ac with v = vb / sum, w = vc / sum: on a thin
        // triangle the barycentrics lose 2^-52 / s^2 to cancellation and move the point ALONG the triangle by that share of its
        // length, whatever the height of p; the foot is off by the normal's angular error (2^-52 / s) times the height only
        const double t = ((n0 * ap0 + n1 * ap1) + n2 * ap2) / nn;
        q[0] = p[0] - t * n0; q[1] = p[1] - t * n1; q[2] = p[2] - t * n2;
      } else {
        done = false;                              // the tests contradict each other: rounding on a triangle near the limit
      }
    }
  }
  double dd;
  if (done) {
    const double e0 = p[0] - q[0], e1 = p[1] - q[1], e2 = p[2] - q[2];
    dd = (e0 * e0 + e1 * e1) + e2 * e2;
  } else {
    reg = kTriThin;
    double r[3];
    dd = closest_on_segment(a, b, p, q);
    double d = closest_on_segment(b, c, p, r);
    if (d < dd) { dd = d; q[0] = r[0]; q[1] = r[1]; q[2] = r[2]; }
    d = closest_on_segment(c, a, p, r);
    if (d < dd) { dd = d; q[0] = r[0]; q[1] = r[1]; q[2] = r[2]; }
  }
  if (region) *region = reg;
  return dd;
}

// ---- area-weighted sampling (dc_mesh_sample) ---------------------------------------------------------------------------------
// u_t = (splitmix64(splitmix64(seed) + 4 i + t) >> 11) 2^-53, t = 0, 1, 2: in [0, 1), exact in fp64
DC_HD void mesh_sample_uniforms(int64_t seed, int64_t i, double* u) {
  const uint64_t base = splitmix64((uint64_t)seed) + 4ull * (uint64_t)i;
  for (int t = 0; t < 3; ++t) u[t] = (double)(splitmix64(base + (uint64_t)t) >> 11) * 0x1p-53;
}

// the first face f with u0 * total < area_cdf[f] (total = area_cdf[n - 1] > 0); past the end: the last face of non-zero area
DC_HD int64_t mesh_sample_face(const double* area_cdf, int64_t n, double u0) {
#pragma clang fp contract(off)
  const double total = area_cdf[n - 1];
  const double x = u0 * total;
  int64_t lo = 0, hi = n;                          // first f in [0, n] with x < cdf[f]
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (x < area_cdf[mid]) hi = mid; else lo = mid + 1;
  }
  if (lo < n) return lo;
  lo = 0;
  hi = n - 1;                                      // first f with cdf[f] >= total: the last face that added area
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (area_cdf[mid] >= total) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// p = (1 - sqrt(u1)) v0 + sqrt(u1) (1 - u2) v1 + sqrt(u1) u2 v2, in this order of operations
DC_HD void mesh_sample_point(const double* tri, double u1, double u2, double* p) {
#pragma clang fp contract(off)
  const double s = sqrt(u1);                       // correctly rounded on the host and on gfx950 (fp64 v_sqrt + the library's fix-up)
  const double w0 = 1.0 - s, w1 = s * (1.0 - u2), w2 = s * u2;
  for (int a = 0; a < 3; ++a) p[a] = (w0 * tri[a] + w1 * tri[3 + a]) + w2 * tri[6 + a];
}

}  // namespace dc
