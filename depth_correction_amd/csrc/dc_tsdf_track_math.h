// Scan-to-TSDF registration: the rules of sampling a sparse volume at a point and of the point-to-surface row built from the sample
// (DESIGN "Scan-to-TSDF registration"), shared by the kernels (dc_tsdf_track.hip), the host build (dc_hostcheck.cpp) and, restated in
// numpy, tests/tsdf_track_reference.py.  Built with -ffp-contract=off like dc_tsdf_sparse_math.h, whose lattice, table and pool these are:
// every product and sum below is rounded on its own, in the order written.
//
// Sampling    For a world point x: q = (x - og) / a - 0.5 per axis.  RANGE unless x is finite and -2^23 <= q < 2^23 - 1 on every axis.
//             i0 = floor(q), f = q - (double)i0 in [0, 1).  Corner c = bx + 2 by + 4 bz (the surface-nets numbering) is the voxel
//             i0 + (bx, by, bz); it is observed iff its block is in the table and count >= min_count, and has the value tsdf_value (units
//             of tau).  UNOBSERVED unless all eight are observed.  Otherwise, with lerp(p, q, t) = p + t (q - p):
//               phi  = tau lerp(lerp(lerp(v0, v1, fx), lerp(v2, v3, fx), fy), lerp(lerp(v4, v5, fx), lerp(v6, v7, fx), fy), fz)
//               gx   = lerp(lerp(v1 - v0, v3 - v2, fy), lerp(v5 - v4, v7 - v6, fy), fz)
//               gy   = lerp(lerp(v2 - v0, v3 - v1, fx), lerp(v6 - v4, v7 - v5, fx), fz)
//               gz   = lerp(lerp(v4 - v0, v5 - v1, fx), lerp(v6 - v2, v7 - v3, fx), fy)
//               grad = (tau / a) (gx, gy, gz), the quotient formed once.
//             An invalid point has phi = NaN, grad = 0, dist = +inf (dist = |phi| otherwise), so that a quantile over the finite
//             distances ranks the valid points only.
// Pair        kept iff flag == 0, dist <= threshold (a NaN threshold keeps nothing) and dist < max_residual: strict, so that a fully
//             clamped sample (|phi| == tau, zero gradient) is no pair at max_residual = tau.
// Row         r = phi, J = [x cross grad, grad] with x the moved point; the 30 sums of IcpRow<6> (dc_slam_math.h) as they are:
//             minimising sum phi(T p)^2 with the left-multiplied increment is what icp_finish_tail solves.
#pragma once
#include "dc_slam_math.h"
#include "dc_tsdf_sparse_math.h"

namespace dc {

constexpr int kTsdfSampleRange = 1;                      // flag: x not finite or q outside [-2^23, 2^23 - 1)
constexpr int kTsdfSampleUnobserved = 2;                 // flag: one of the eight corners is unobserved

struct TsdfSample {
  double phi, grad[3], dist;
  int flag;
};

DC_HD double tsdf_lerp(double p, double q, double t) { return p + t * (q - p); }

// phi / tau and the gradient in units of tau per voxel from the eight corner values v (corner c = bx + 2 by + 4 bz) and f [3]
DC_HD void tsdf_trilinear(const double* v, const double* f, double* value, double* g) {
  const double fx = f[0], fy = f[1], fz = f[2];
  *value = tsdf_lerp(tsdf_lerp(tsdf_lerp(v[0], v[1], fx), tsdf_lerp(v[2], v[3], fx), fy),
                     tsdf_lerp(tsdf_lerp(v[4], v[5], fx), tsdf_lerp(v[6], v[7], fx), fy), fz);
  g[0] = tsdf_lerp(tsdf_lerp(v[1] - v[0], v[3] - v[2], fy), tsdf_lerp(v[5] - v[4], v[7] - v[6], fy), fz);
  g[1] = tsdf_lerp(tsdf_lerp(v[2] - v[0], v[3] - v[1], fx), tsdf_lerp(v[6] - v[4], v[7] - v[5], fx), fz);
  g[2] = tsdf_lerp(tsdf_lerp(v[4] - v[0], v[5] - v[1], fx), tsdf_lerp(v[6] - v[2], v[7] - v[3], fx), fy);
}

// The sample at the world point x.  keys [nb] / slots are the table, sum / count the pool of `capacity` blocks; a slot outside the pool
// counts as a missing block.  The corners are visited z fastest, so that the lane's cache searches once per block change.
DC_HD TsdfSample tsdf_sample_point(const double* x, const TsdfGrid& g, double tau, int min_count, const uint64_t* keys, const int32_t* slots,
                                   int64_t nb, int64_t capacity, const int64_t* sum, const int32_t* count) {
  TsdfSample s{NAN, {0.0, 0.0, 0.0}, INFINITY, kTsdfSampleRange};
  double q[3];
  bool in = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    q[a] = (x[a] - g.og[a]) / g.a - 0.5;
    in = in && isfinite(x[a]) && q[a] >= -kTsdfVoxelRange && q[a] < kTsdfVoxelRange - 1.0;
  }
  if (!in) return s;
  int i0[3];
  double f[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double fl = floor(q[a]);
    i0[a] = (int)fl;
    f[a] = q[a] - (double)i0[a];
  }
  double v[8];
  bool all = true;
  TsdfBlockCache cache{kTsdfNoKey, -1};
#pragma unroll
  for (int bx = 0; bx < 2; ++bx)
#pragma unroll
    for (int by = 0; by < 2; ++by)
#pragma unroll
      for (int bz = 0; bz < 2; ++bz) {
        const int i[3] = {i0[0] + bx, i0[1] + by, i0[2] + bz};
        const int64_t pos = tsdf_cached_find(keys, nb, tsdf_voxel_key(i), &cache);
        const int64_t slot = pos < 0 ? -1 : (int64_t)slots[pos];
        double val = 0.0;
        bool obs = slot >= 0 && slot < capacity;
        if (obs) {
          const int64_t at = slot * kTsdfBlockVoxels + tsdf_voxel_local(i);
          obs = tsdf_observed(count, at, min_count);
          if (obs) val = tsdf_value(sum, count, at);
        }
        all = all && obs;
        v[bx + 2 * by + 4 * bz] = val;
      }
  if (!all) {
    s.flag = kTsdfSampleUnobserved;
    return s;
  }
  double value, gr[3];
  tsdf_trilinear(v, f, &value, gr);
  const double scale = tau / g.a;
  s.phi = tau * value;
  s.grad[0] = scale * gr[0]; s.grad[1] = scale * gr[1]; s.grad[2] = scale * gr[2];
  s.dist = fabs(s.phi);
  s.flag = 0;
  return s;
}

// Is the sample of a point a pair?
DC_HD bool tsdf_track_keep(int flag, double dist, double threshold, double max_residual) {
  return flag == 0 && dist <= threshold && dist < max_residual;
}

// Adds the pair (moved point x, r = phi, gradient g) to the 30 sums v of IcpRow<6>; kUsed is the caller's.
DC_HD void tsdf_track_add(const double* x, double r, const double* g, double* v) {
  const double J[6] = {x[1] * g[2] - x[2] * g[1], x[2] * g[0] - x[0] * g[2], x[0] * g[1] - x[1] * g[0], g[0], g[1], g[2]};
  int q = 0;
#pragma unroll
  for (int a = 0; a < 6; ++a)
#pragma unroll
    for (int b = a; b < 6; ++b) v[q++] += J[a] * J[b];
#pragma unroll
  for (int a = 0; a < 6; ++a) v[IcpRow<6>::kJtr + a] += J[a] * r;
  v[IcpRow<6>::kPairs] += 1.0;
  v[IcpRow<6>::kSse] += r * r;
}

}  // namespace dc
