// Per-ray arithmetic of the surfel ray caster (dc_raycast.hip: dc_surfel_bvh_build, dc_surfel_cast_rays; compiled for the host by
// dc_hostcheck.cpp, so that the CPU tests pin it).  Definitions: include/dc_hip.h, DESIGN "Depth bias against a surveyed cloud".
//
// A surfel is a survey point with its normal and a radius: the disk (p, n, rho), two-sided (survey normals have no orientation: no
// culling).  n is used as given; |n| is divided out wherever unit length matters.  A disk travels as one 64-byte row of 8 doubles
// (p0 p1 p2 n0 n1 n2 rho^2 0), rho^2 = fl(rho rho).
//
// No fused multiply-adds in this header (#pragma clang fp contract(off) in every function; the host build has -ffp-contract=off), and
// every sum of products is written in ONE order,
//     x . y = (x0 y0 + x1 y1) + x2 y2,
// so the kernels and the host build perform the same correctly rounded operations and give the same bits.  The arc cosine is
// acos01 below, built from +, *, / and sqrt alone, for the same reason: the device library's acos and the host's differ in the
// last place.
//
// test_disk (ray o + t d, fp64 world frame):
//     q = p - o,  den = n . d,  t = (n . q) / den,  h = t d - q,  r^2 = h . h,
// a hit iff den != 0, t_min < t < inf and r^2 <= rho^2 (the rim counts; anything NaN compares false: a miss).  Closest hit: the
// smallest t, on equal t the lower survey index -- test_triangle's rule, independent of the tree.
//
// disk_box.  The exact disk spans p_a +- rho sqrt(n_b^2 + n_c^2) / |n| on axis a (not rho sqrt(1 - n_a^2), which cancels for an
// axis-aligned normal: a wall-aligned disk gets a half-extent of exactly 0).  The box is that span grown by the margin
//     m = 2^-48 (|p0| + |p1| + |p2| + rho)
// and rounded outward to fp32 (f32_rd / f32_ru).  Why m: property 1 (below) needs the point x = o + t d of an ACCEPTED hit, for the
// rounded t and the exact ray, inside the box up to what box_entry's own margin max(2^-22 |o|, 1e-20) absorbs.  With u = 2^-53:
//   * q_a, t d_a and h_a are one rounding each, so the exact h' = x - p has |h'_a - h_a| <= u (|q_a| + |t d_a| + |h_a|);
//   * r^2 <= fl(rho^2) for the computed h gives |h| <= rho (1 + 3 u);
//   * x is not exactly in the disk's plane: n . q and n . d carry 3 u sum|n_a q_a| and 3 u sum|n_a d_a|, the quotient u, so x
//     stands off the plane by at most 3 u |q| + 4 u t |d|;
//   so on every axis |x_a - p_a| <= (exact half-extent) + 3 u rho + 8 u R with R = max(|q|, t |d|) <= |p| + |o| + rho the range of
//   the ray: about 2^-52 of the RANGE, not of rho.  The half-extent itself is computed with 4 roundings (<= 4 u rho).  The part
//   8 u (|p| + rho) + 7 u rho <= 2^-49 (|p|_1 + rho) is m with a factor 2 to spare; the part 8 u |o| <= 2^-49 sqrt 3 max|o_a| lies
//   27 binary orders below box_entry's margin 2^-22 max|o_a|.
//   A wall-aligned disk's box is 2 m thick plus at most one fp32 ulp per side.
// Property 1 (pinned by tests/test_surfel_host.py): for every (ray, disk) pair test_disk accepts at t, box_entry(disk_box) is finite
// with t_far = +inf and with t_far = prune_far(t).  Every ancestor's box holds the leaf's (exact min / max), so the traversal returns
// what test_disk over every disk in index order returns.
//
// Blend, given the first hit (t1, n1) and the parameters window >= 0 (along the ray, in units of |d|) and min_cos in [0, 1).
// Members: the disks with a hit, t <= fl(t1 + window) and |n_i . n1| / (|n_i| |n1|) >= min_cos; the first hit is a member whatever
// its own quotient rounds to.  With w_i = 1 - r_i^2 / rho_i^2 (0 for rho_i^2 = 0), a_i = t_i - t1, g_i = w_i / |n_i|,
// s_i = -1 when n_i . n1 < 0 else +1:
//     W = sum w_i,   S = sum w_i a_i,   N = sum (s_i g_i) n_i,
//     t = t1 + S / W,   cos(inc) = min(1, |N . d| / (|N| |d|)),   inc = acos01(cos(inc)),   count = the number of members.
// W = 0 (every member exactly on its rim) or N = 0: the first hit's t and / or normal instead.  window = 0: no second pass,
// t = t1, inc from n1, count = 1.  The sums are taken in the order the members are met (the host build: index order; the kernel: the
// order of its walk over the deterministic tree), so each is reproducible and they differ from each other by rounding only.
//
// Rounding-error count, to first order, in units of 2^-52 (a correctly rounded +, *, / or sqrt contributes 1/2 relative), against
// the exact sums of the same doubles w_i, a_i, n_i, for k members:
//   S: 1/2 per product, (k - 1) / 2 for the additions of non-negative terms: k / 2 relative;  W: (k - 1) / 2;  S / W: k;
//   t = t1 + S / W:                    |dt| <= k (t - t1) + t / 2                                       [surfel_t_err(k)]
//   g_i: |n_i|^2 3/2, its root 5/4, the quotient 7/4; g_i n_ia 9/4; the k - 1 additions per component (k - 1) / 2 of
//   sum w_i |n_ia| / |n_i|; over the three components (the vector of the |n_ia| / |n_i| has length 1):
//                                      |dN| <= (k / 2 + 7/4) W
//   so the unit vector N / |N| turns by at most (k / 2 + 7/4) kappa with kappa = W / |N| (>= 1, and <= 1 / min_cos because
//   N . n1 / |n1| = sum w_i |cos_i| >= min_cos W), and cos(inc) moves by as much; N . d: 3/2 |N| |d|; |N|, |d|: 5/4 each,
//   their product and the quotient 1/2 each: 5 more.  acos01 is within one unit of its result, and a test that takes the cosine
//   of the returned angle adds that and the cosine's own rounding, 5/2 together:
//                                      |d cos(inc)| <= (k / 2 + 7/4) kappa + 15/2                       [surfel_cos_err(k, kappa)]
#pragma once
#include <math.h>
#include "dc_common.h"
#include "dc_raymath.h"

namespace dc {

// Scalars only: a runtime-indexed private array would live in scratch memory on the device (see Ray64).
struct SurfelRay {
  double o0, o1, o2;
  double d0, d1, d2;
};

struct SurfelHit {
  double t, r2;
  int32_t index;                // survey index, -1 without a hit
  int32_t leaf;                 // the winning leaf (row of leaf_disk), -1 without a hit
};

struct SurfelBlend {
  double W, S, N0, N1, N2;
  int32_t count;
};

constexpr int kDiskRow = 8;     // doubles per disk: p, n, rho^2, 0

// the error counts of the header comment, in units of 2^-52
DC_HD double surfel_t_err(int k, double t, double t1) { return (double)k * (t - t1) + 0.5 * t; }
DC_HD double surfel_cos_err(int k, double kappa) { return (0.5 * (double)k + 1.75) * kappa + 7.5; }

DC_HD double surfel_dot(double x0, double x1, double x2, double y0, double y1, double y2) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return (x0 * y0 + x1 * y1) + x2 * y2;
}

// arc cosine on [0, 1] (NaN stays NaN; the callers clamp to 1): the rational approximation of fdlibm's e_acos.c (Sun Microsystems,
// 1993, freely distributable), which uses +, *, / and sqrt only, so that host and device agree to the bit.  Within one unit in the
// last place of the result.
DC_HD double acos01(double x) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double pio2_hi = 1.57079632679489655800e+00, pio2_lo = 6.12323399573676603587e-17;
  const double pS0 = 1.66666666666666657415e-01, pS1 = -3.25565818622400915405e-01, pS2 = 2.01212532134862925881e-01,
               pS3 = -4.00555345006794114027e-02, pS4 = 7.91534994289814532176e-04, pS5 = 3.47933107596021167570e-05;
  const double qS1 = -2.40339491173441421878e+00, qS2 = 2.02094576023350569471e+00, qS3 = -6.88283971605453293030e-01,
               qS4 = 7.70381505559019352791e-02;
  if (!(x == x)) return x;
  if (x >= 1.0) return 0.0;
  if (x < 0.5) {
    if (x < 0x1p-57) return pio2_hi + pio2_lo;
    const double z = x * x;
    const double p = z * (pS0 + z * (pS1 + z * (pS2 + z * (pS3 + z * (pS4 + z * pS5)))));
    const double q = 1.0 + z * (qS1 + z * (qS2 + z * (qS3 + z * qS4)));
    const double r = p / q;
    return pio2_hi - (x - (pio2_lo - r * x));
  }
  const double z = (1.0 - x) * 0.5;
  const double s = sqrt(z);
  uint64_t bits;
  __builtin_memcpy(&bits, &s, 8);
  bits &= 0xffffffff00000000ull;
  double df;
  __builtin_memcpy(&df, &bits, 8);
  const double c = (z - df * df) / (s + df);
  const double p = z * (pS0 + z * (pS1 + z * (pS2 + z * (pS3 + z * (pS4 + z * pS5)))));
  const double q = 1.0 + z * (qS1 + z * (qS2 + z * (qS3 + z * qS4)));
  const double r = p / q;
  const double w = r * s + c;
  return 2.0 * (df + w);
}

// box [6] (lo xyz, hi xyz) of the disk (p [3], n [3], rho): the exact span grown by m and rounded outward (header comment)
DC_HD void disk_box(const double* p, const double* n, double rho, float* box) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double n0 = n[0], n1 = n[1], n2 = n[2];
  const double s0 = n0 * n0, s1 = n1 * n1, s2 = n2 * n2;
  const double len = sqrt((s0 + s1) + s2);
  const double m = 0x1p-48 * (((fabs(p[0]) + fabs(p[1])) + fabs(p[2])) + rho);
  const double e0 = rho * sqrt(s1 + s2) / len + m;
  const double e1 = rho * sqrt(s0 + s2) / len + m;
  const double e2 = rho * sqrt(s0 + s1) / len + m;
  box[0] = f32_rd(p[0] - e0);
  box[1] = f32_rd(p[1] - e1);
  box[2] = f32_rd(p[2] - e2);
  box[3] = f32_ru(p[0] + e0);
  box[4] = f32_ru(p[1] + e1);
  box[5] = f32_ru(p[2] + e2);
}

// t and r^2 of the ray on the disk's row; true for a hit beyond t_min
DC_HD bool disk_hit(const double* __restrict__ disk, const SurfelRay& r, double t_min, double& t, double& r2) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double q0 = disk[0] - r.o0, q1 = disk[1] - r.o1, q2 = disk[2] - r.o2;
  const double den = surfel_dot(disk[3], disk[4], disk[5], r.d0, r.d1, r.d2);
  const double nq = surfel_dot(disk[3], disk[4], disk[5], q0, q1, q2);
  t = nq / den;
  const double h0 = t * r.d0 - q0, h1 = t * r.d1 - q1, h2 = t * r.d2 - q2;
  r2 = surfel_dot(h0, h1, h2, h0, h1, h2);
  return den != 0.0 && t > t_min && t < INFINITY && r2 <= disk[6];
}

// a hit beyond t_min that beats `best`: smaller t, on equal t the lower survey index
DC_HD void test_disk(const double* __restrict__ disk, int32_t index, int32_t leaf, const SurfelRay& r, double t_min, SurfelHit& best) {
  double t, r2;
  if (!disk_hit(disk, r, t_min, t, r2)) return;
  if (t > best.t || (t == best.t && index >= best.index)) return;
  best.t = t;
  best.r2 = r2;
  best.index = index;
  best.leaf = leaf;
}

// |n . d| / (|n| |d|)
DC_HD double surfel_cos(double n0, double n1, double n2, const SurfelRay& r) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double nd = surfel_dot(n0, n1, n2, r.d0, r.d1, r.d2);
  const double nn = surfel_dot(n0, n1, n2, n0, n1, n2);
  const double dd = surfel_dot(r.d0, r.d1, r.d2, r.d0, r.d1, r.d2);
  return fabs(nd) / (sqrt(nn) * sqrt(dd));
}

DC_HD void blend_init(SurfelBlend& b) {
  b.W = b.S = b.N0 = b.N1 = b.N2 = 0.0;
  b.count = 0;
}

// Second pass on one disk: adds it to the sums when it is a member.  `first` is the first hit's row, t1 its t, t_end = fl(t1 + window).
DC_HD void blend_disk(const double* __restrict__ disk, bool is_first, const double* __restrict__ first, const SurfelRay& r, double t_min,
                      double t1, double t_end, double min_cos, SurfelBlend& b) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  double t, r2;
  if (!disk_hit(disk, r, t_min, t, r2) || !(t <= t_end)) return;
  const double n0 = disk[3], n1 = disk[4], n2 = disk[5];
  const double dot = surfel_dot(n0, n1, n2, first[3], first[4], first[5]);
  const double len = sqrt(surfel_dot(n0, n1, n2, n0, n1, n2));
  if (!is_first) {
    const double len1 = sqrt(surfel_dot(first[3], first[4], first[5], first[3], first[4], first[5]));
    if (!(fabs(dot) / (len * len1) >= min_cos)) return;
  }
  const double w = disk[6] > 0.0 ? 1.0 - r2 / disk[6] : 0.0;
  const double g = w / len;
  const double sg = dot < 0.0 ? -g : g;
  b.W = b.W + w;
  b.S = b.S + w * (t - t1);
  b.N0 = b.N0 + sg * n0;
  b.N1 = b.N1 + sg * n1;
  b.N2 = b.N2 + sg * n2;
  b.count += 1;
}

DC_HD SurfelHit no_surfel_hit() { return SurfelHit{INFINITY, 0.0, -1, -1}; }

// The two passes as visitors of bvh_walk (dc_bvh.h) over a tree of disks.  Pass 1 (kBlend false) keeps the closest hit in `best` and
// prunes with it, as TriVisitor does.  Pass 2 (kBlend true) adds every member of the blend to `blend` under the fixed bound
// prune_far(t_end): prune_far does not decrease, and a member's t is at most t_end, so property 1 keeps every member's boxes.  The
// order of the walk depends on the tree and the ray alone.  t_end and min_cos are read by pass 2 only.
template <bool kBlend>
struct DiskVisitor {
  const float* __restrict__ node_box;
  const double* __restrict__ leaf_disk;
  const int32_t* __restrict__ leaf_index;
  const SurfelRay& sr; const Ray32& ray;
  double t_min, t_end, min_cos;
  SurfelHit& best; SurfelBlend& blend;

  DC_HD bool enter(int64_t node, float& key) const {
    key = box_entry(node_box + 6 * node, ray, prune_far(kBlend ? t_end : best.t));
    return key < INFINITY;
  }
  DC_HD void leaf(int64_t leaf) {
    const double* disk = leaf_disk + kDiskRow * leaf;
    if (kBlend) blend_disk(disk, leaf == best.leaf, leaf_disk + kDiskRow * (int64_t)best.leaf, sr, t_min, best.t, t_end, min_cos, blend);
    else test_disk(disk, leaf_index[leaf], (int32_t)leaf, sr, t_min, best);
  }
};

// the return of one ray: t, inc and count from the first hit (its row `first`) and the blend sums (count = 0: window = 0, no second pass)
DC_HD void surfel_finish(const SurfelHit& best, const double* __restrict__ first, const SurfelBlend& b, const SurfelRay& r, double& t,
                         double& inc, int32_t& count) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (best.leaf < 0) {
    t = INFINITY;
    inc = NAN;
    count = 0;
    return;
  }
  t = best.t;
  count = 1;
  double n0 = first[3], n1 = first[4], n2 = first[5];
  if (b.count > 0) {
    count = b.count;
    if (b.W > 0.0) {
      t = best.t + b.S / b.W;
      if (surfel_dot(b.N0, b.N1, b.N2, b.N0, b.N1, b.N2) > 0.0) { n0 = b.N0; n1 = b.N1; n2 = b.N2; }
    }
  }
  inc = acos01(fmin(1.0, surfel_cos(n0, n1, n2, r)));
}

}  // namespace dc
