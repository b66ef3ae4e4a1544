// Global registration: the rules of the coarse stage (dc_globalreg.hip; DESIGN "Global registration"), host and device.  Scalars
// only, fp64 unless said otherwise, no fused multiply-adds; every dot product is (x0 y0 + x1 y1) + x2 y2.
//
// Pair feature of the points x_i, x_j with normals n_i, n_j (any sign, any non-zero length): d = x_j - x_i, L = sqrt(d.d), e = d / L,
// n^ = n / |n|, a1 = |n^_i.e|, a2 = |n^_j.e|, a3 = |n^_i.n^_j|, bin(a) = min(B - 1, (int)floor(B a)), B = 11.  The pair is valid iff
// L is finite and > 0, both |n| are finite and > 0 and none of a1, a2, a3 is NaN.  These rules are this package's, not PCL's: they are
// invariant to a rigid motion and to the sign of either normal, and continuous at a = 0 (the oriented FPFH angles are neither on
// coplanar pairs).
//
// Bin edges in designed scenes: a sits on an edge where B a is an integer.  Coplanar pairs give a1 = a2 = 0 (bin 0) and a3 = 1 (bin
// B - 1, by the min), pairs across two perpendicular walls whose offset is axis-aligned give 0 or 1 as well.  Both are safe: 0 and 1
// are not edges (a >= 0 by the absolute value, the min keeps a >= 1 in the last bin), so a value a rounding error away from them
// (1 - ulp on a rotated coplanar pair) lands in the same bin.  The ten inner edges k / B are hit only by a cosine that is exactly
// k / B, e.g. a wall pair with d along (k, sqrt(B^2 - k^2), 0): the tests' oracle asserts that no input they use comes within 1e-9 of one.
#pragma once
#include <math.h>
#include "dc_common.h"
#include "dc_rng.h"
#include "dc_align_math.h"

namespace dc {

constexpr int kGregBins = 11;                   // B
constexpr int kGregFeat = 3 * kGregBins;        // 33 values per descriptor
constexpr int kGregMaxK = 64;                   // most neighbour slots per point

DC_HD double greg_dot(double x0, double x1, double x2, double y0, double y1, double y2) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return (x0 * y0 + x1 * y1) + x2 * y2;
}

DC_HD int greg_bin(double a) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const int b = (int)floor((double)kGregBins * a);
  return b < kGregBins - 1 ? b : kGregBins - 1;
}

// The pair (x_i, n_i), (x_j, n_j): returns 1 and a [3], *L when it is valid, 0 otherwise (a and *L are then not meaningful).
DC_HD int greg_pair_feature(const double* xi, const double* ni, const double* xj, const double* nj, double* a, double* L) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double d0 = xj[0] - xi[0], d1 = xj[1] - xi[1], d2 = xj[2] - xi[2];
  const double len = sqrt(greg_dot(d0, d1, d2, d0, d1, d2));
  const double li = sqrt(greg_dot(ni[0], ni[1], ni[2], ni[0], ni[1], ni[2]));
  const double lj = sqrt(greg_dot(nj[0], nj[1], nj[2], nj[0], nj[1], nj[2]));
  *L = len;
  if (!(len > 0.0) || !(len < INFINITY) || !(li > 0.0) || !(li < INFINITY) || !(lj > 0.0) || !(lj < INFINITY)) return 0;
  const double e0 = d0 / len, e1 = d1 / len, e2 = d2 / len;
  const double u0 = ni[0] / li, u1 = ni[1] / li, u2 = ni[2] / li;
  const double v0 = nj[0] / lj, v1 = nj[1] / lj, v2 = nj[2] / lj;
  a[0] = fabs(greg_dot(u0, u1, u2, e0, e1, e2));
  a[1] = fabs(greg_dot(v0, v1, v2, e0, e1, e2));
  a[2] = fabs(greg_dot(u0, u1, u2, v0, v1, v2));
  if (a[0] != a[0] || a[1] != a[1] || a[2] != a[2]) return 0;
  return 1;
}

// One value of the descriptor before its block is scaled: F = SPFH_i + (1 / m_i) acc, acc the sum of (1 / L_ij) SPFH_j over the valid
// slots in ascending slot order, one term at a time (greg_fpfh_term).
DC_HD double greg_fpfh_term(double acc, double L, double spfh_j) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double w = 1.0 / L;
  return acc + w * spfh_j;
}

DC_HD double greg_fpfh_value(double spfh_i, int m, double acc) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double inv = 1.0 / (double)m;
  return spfh_i + inv * acc;
}

// A block of 11 scaled to sum 100: v * (100 / sum), sum taken in ascending bin order; a sum of 0 (or a sum that is not > 0) leaves zeros.
DC_HD double greg_block_scale(double sum) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return sum > 0.0 ? 100.0 / sum : 0.0;
}

// Descriptor distance in fp32: s = 0; s = s + t t for t = fq[b] - fs[b], b ascending; the product is rounded, then the sum.
DC_HD float greg_feature_dist(const float* fq, const float* fs) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  float s = 0.0f;
  for (int b = 0; b < kGregFeat; ++b) {
    const float t = fq[b] - fs[b];
    const float tt = t * t;
    s = s + tt;
  }
  return s;
}

// Draw t (0, 1, 2) of hypothesis h among C correspondences.
DC_HD int64_t greg_draw(uint64_t seed, uint64_t h, int t, int64_t C) {
  return (int64_t)(splitmix64(seed ^ (h << 2) ^ (uint64_t)t) % (uint64_t)C);
}

DC_HD double greg_edge(const double* a, const double* b) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double d0 = a[0] - b[0], d1 = a[1] - b[1], d2 = a[2] - b[2];
  return sqrt(greg_dot(d0, d1, d2, d0, d1, d2));
}

// The edge check of one point pair: lp = |p_a - p_b|, ly = |y_a - y_b|; lp >= min_edge, lp >= rho ly and ly >= rho lp.
DC_HD int greg_edge_ok(double lp, double ly, double min_edge, double rho) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return (lp >= min_edge && lp >= rho * ly && ly >= rho * lp) ? 1 : 0;
}

// Edge check and fit of the three pairs (p [9], y [9], row-major, in draw order; the draws are distinct by the caller) about the
// origins o [6]: the 17 moments summed in draw order (E, which the solve does not read, is 0), align_solve.  Returns 1 and T [16]
// when the edges pass, align_solve does not call the pairs degenerate and T is finite; 0 otherwise (T is then not meaningful).
DC_HD int greg_check_fit(const double* p, const double* y, const double* o, double min_edge, double rho, double* T, double* lam) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  for (int a = 0; a < 3; ++a) {
    const int b = a == 2 ? 0 : a + 1;               // pairs (0,1) (1,2) (2,0)
    if (!greg_edge_ok(greg_edge(p + 3 * a, p + 3 * b), greg_edge(y + 3 * a, y + 3 * b), min_edge, rho)) return 0;
  }
  double tot[DC_ALIGN_PARTIALS];
  for (int q = 0; q < DC_ALIGN_PARTIALS; ++q) tot[q] = 0.0;
  for (int t = 0; t < 3; ++t) {
    const double pc[3] = {p[3 * t] - o[0], p[3 * t + 1] - o[1], p[3 * t + 2] - o[2]};
    const double yc[3] = {y[3 * t] - o[3], y[3 * t + 1] - o[4], y[3 * t + 2] - o[5]};
    tot[0] += 1.0;
    for (int a = 0; a < 3; ++a) {
      tot[1 + a] += pc[a];
      tot[4 + a] += yc[a];
      for (int b = 0; b < 3; ++b) tot[7 + a * 3 + b] += pc[a] * yc[b];
    }
  }
  bool finite = true;
  for (int q = 0; q < DC_ALIGN_PARTIALS; ++q) finite = finite && isfinite(tot[q]);
  if (!finite) return 0;
  if (align_solve(tot, o, T, lam)) return 0;
  for (int q = 0; q < 12; ++q) finite = finite && isfinite(T[q]);
  return finite ? 1 : 0;
}

// |T p - y|^2 with T p = ((T00 p0 + T01 p1) + T02 p2) + T03, dc_knn_grid_query's order
DC_HD double greg_residual2(const double* T, const double* p, const double* y) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double r0 = (((T[0] * p[0] + T[1] * p[1]) + T[2] * p[2]) + T[3]) - y[0];
  const double r1 = (((T[4] * p[0] + T[5] * p[1]) + T[6] * p[2]) + T[7]) - y[1];
  const double r2 = (((T[8] * p[0] + T[9] * p[1]) + T[10] * p[2]) + T[11]) - y[2];
  return greg_dot(r0, r1, r2, r0, r1, r2);
}

}  // namespace dc
