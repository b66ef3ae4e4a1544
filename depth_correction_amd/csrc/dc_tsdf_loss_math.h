// Self-supervised training against the fused volume: the rules of sampling a sparse volume with one scan's own contribution taken
// out, and of the loss term built from the sample (DESIGN "Self-supervised training against the fused volume"), shared by the kernels
// (dc_tsdf_loss.hip), the host build (dc_hostcheck.cpp) and, restated in numpy, tests/tsdf_loss_reference.py.  Built with
// -ffp-contract=off like dc_tsdf_track_math.h, whose sample this extends: every product and sum below is rounded on its own.
//
// Exclusion   The volume's sums are integers, so the volume of "all scans but s" is, bit for bit, the total minus the volume of scan s
//             alone.  Corner voxel i has sum = sum_total(i) - sum_own(i) and count = count_total(i) - count_own(i); a voxel whose block
//             a table lacks contributes 0 from that table (a slot outside its pool counts as a missing block).  The corner is observed
//             iff its block is in the TOTAL table and count >= min_count; its value is (double)sum / ((double)count 2^20), as tsdf_value
//             forms it.  The range test, i0, f, the corner order (z fastest), tsdf_trilinear, phi = tau value and grad = (tau / a) g are
//             those of tsdf_sample_point; without an own table (NULL) the result is bit-equal to tsdf_sample_point.
// Term        squared: l = phi^2, dl/dx = (2 phi) grad.  Otherwise l = |phi|, dl/dx = sign(phi) grad, zero at phi = 0.
// Class       a point of the mask is INVALID (x not finite, or the sample's flag RANGE), UNOBSERVED (flag UNOBSERVED), GATED (|phi| >=
//             max_residual: strict as tsdf_track_keep is, so a fully clamped sample is never used) or USED.  The volume is a constant of
//             the gradient.
#pragma once
#include "dc_tsdf_track_math.h"

namespace dc {

constexpr int kTsdfLossUsed = 0, kTsdfLossInvalid = 1, kTsdfLossUnobserved = 2, kTsdfLossGated = 3, kTsdfLossMasked = 255;

// One table with its pool: keys [nb] ascending / slots, sum / count of `capacity` blocks.  keys == NULL: no table.
struct TsdfTable {
  const uint64_t* keys;
  const int32_t* slots;
  int64_t nb, capacity;
  const int64_t* sum;
  const int32_t* count;
};

// index into sum / count of voxel i in table t (one search per block change through the lane's cache), -1 where its block is missing
DC_HD int64_t tsdf_table_voxel(const TsdfTable& t, const int* i, TsdfBlockCache* cache) {
  const int64_t pos = tsdf_cached_find(t.keys, t.nb, tsdf_voxel_key(i), cache);
  const int64_t slot = pos < 0 ? -1 : (int64_t)t.slots[pos];
  return slot >= 0 && slot < t.capacity ? slot * kTsdfBlockVoxels + tsdf_voxel_local(i) : -1;
}

// The sample at the world point x of the volume `total` minus the volume `own` (own.keys == NULL: nothing is taken out).  The caches
// are the lane's, one per table: a caller that samples along a line (dc_tsdf_cast_math.h) keeps them from sample to sample.
DC_HD TsdfSample tsdf_sample_point_minus(const double* x, const TsdfGrid& g, double tau, int min_count, const TsdfTable& total,
                                         const TsdfTable& own, TsdfBlockCache* cache_total, TsdfBlockCache* cache_own) {
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
#pragma unroll
  for (int bx = 0; bx < 2; ++bx)
#pragma unroll
    for (int by = 0; by < 2; ++by)
#pragma unroll
      for (int bz = 0; bz < 2; ++bz) {
        const int i[3] = {i0[0] + bx, i0[1] + by, i0[2] + bz};
        const int64_t at = tsdf_table_voxel(total, i, cache_total);
        double val = 0.0;
        bool obs = at >= 0;
        if (obs) {
          int64_t sum = total.sum[at];
          int32_t count = total.count[at];
          if (own.keys) {
            const int64_t mine = tsdf_table_voxel(own, i, cache_own);
            if (mine >= 0) {
              sum -= own.sum[mine];
              count -= own.count[mine];
            }
          }
          obs = count >= min_count;
          if (obs) val = (double)sum / ((double)count * kTsdfOne);
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

// the same for a lane that takes one sample
DC_HD TsdfSample tsdf_sample_point_minus(const double* x, const TsdfGrid& g, double tau, int min_count, const TsdfTable& total,
                                         const TsdfTable& own) {
  TsdfBlockCache cache_total{kTsdfNoKey, -1}, cache_own{kTsdfNoKey, -1};
  return tsdf_sample_point_minus(x, g, tau, min_count, total, own, &cache_total, &cache_own);
}

// l and dl/dx [3] of a used point from its sample
DC_HD double tsdf_loss_term(double phi, const double* grad, bool squared, double* dl_dx) {
  const double c = squared ? 2.0 * phi : (phi > 0.0 ? 1.0 : (phi < 0.0 ? -1.0 : 0.0));
#pragma unroll
  for (int a = 0; a < 3; ++a) dl_dx[a] = c * grad[a];
  return squared ? phi * phi : fabs(phi);
}

// the class of a point of the mask from its sample
DC_HD int tsdf_loss_class(const TsdfSample& s, double max_residual) {
  if (s.flag == kTsdfSampleRange) return kTsdfLossInvalid;    // a point that is not finite is out of range
  if (s.flag != 0) return kTsdfLossUnobserved;
  return s.dist < max_residual ? kTsdfLossUsed : kTsdfLossGated;
}

}  // namespace dc
