// Ray casting the fused volume: the rule of marching a ray through a sparse TSDF volume to the zero crossing of its trilinear
// interpolant (DESIGN "Ray casting the fused volume"), shared by the kernel (dc_tsdf_cast.hip), the host build (dc_hostcheck.cpp) and,
// restated in numpy, tests/tsdf_cast_reference.py.  Built with -ffp-contract=off like dc_tsdf_loss_math.h, whose sample this takes:
// every product and sum below is rounded on its own, in the order written.
//
// Ray         o = R vp + t and u = R dir for the scan's pose, the row sums as tsdf_ray_walk forms them (((R0 v0 + R1 v1) + R2 v2) + t).
//             SKIPPED when the mask is 0, o or u is not finite, or u is zero.  The parameter t is in units of |dir|.
// Samples     t_j = t_min + (double)j step for j = 0 .. J, J = floor((t_max - t_min) / step); p_j = o + t_j u per axis; the sample is
//             tsdf_sample_point_minus(p_j): the volume `total` minus the scan's own volume (none: tsdf_sample_point to the bit).
// March       in ascending j.  A sample with flag != 0 is invalid and breaks a bracket; a valid one with phi > 0 opens the bracket or
//             moves its near end; the march stops at the first valid sample with phi <= 0: a crossing iff sample j - 1 was valid with
//             phi > 0, BEHIND otherwise (the ray entered observed solid from unobserved space, or started inside).  No stop: MISS.
// Refinement  (t0, phi0) = sample j - 1, (t1, phi1) = sample j, t* = t0 + (t1 - t0) (phi0 / (phi0 - phi1)).  `refine` rounds of
//             bracketed regula falsi: sample at t*; invalid: LOST; phi* > 0 replaces the near end, otherwise the far end; t* again.  A last
//             sample at t* gives the residual phi and the gradient g; invalid, or g all zero: LOST.
// Hit         t = t*, normal = g / |g| with |g| = sqrt((g0 g0 + g1 g1) + g2 g2) (to the free side, as the faces of the extraction),
//             inc = acos01(min(1, surfel_cos(normal, u))) (dc_surfelmath.h: the cosine |n . u| / (|n| |u|) of the casts, in the one
//             form the host and the device give the same bits for), face = the table position of the block of the last sample's base
//             voxel i0.  Not a hit: face -1, t +inf, inc, normal and phi NaN -- the miss of dc_raycast_rays.
// Skipping    A sample whose base voxel i0 lies in a block the table lacks (or whose slot lies outside the pool) has corner 0
//             unobserved: it is invalid whatever the other corners hold, and is decided by one look-up without a voxel read.  Per axis
//             the computed i0 does not decrease (u_a > 0), does not increase (u_a < 0) or stays (u_a = 0) as j grows: t_j, the product
//             t u_a, the sum with o_a, the quotient and the floor are each monotone in their argument, and rounding to nearest keeps
//             that.  So if samples j and j' > j have their base voxels in the same absent block, so has every sample between them, and
//             the lane may go on at j' + 1.  j' is an estimate from the block's exit (tsdf_cast_jump), and the lane lands there and
//             looks: where the estimate is too far, the base block differs and the lane steps to j + 1 instead.  The result is that of
//             the march over every j whatever the estimate gives.
// Samples     the count of calls of the sample function: every j reached and every refinement sample without skipping; with it, only
//             those that are in range and whose base block is in the table (the others read no voxel).
#pragma once
#include "dc_surfelmath.h"
#include "dc_tsdf_loss_math.h"

namespace dc {

constexpr int kTsdfCastHit = 0, kTsdfCastSkipped = 1, kTsdfCastMiss = 2, kTsdfCastBehind = 3, kTsdfCastLost = 4;
constexpr int kTsdfCastMaxSteps = 1 << 24;

struct TsdfCastRule {
  double t_min, step, tau;
  int J, refine, min_count;
  bool skip;
};

// a lane's ray and what it keeps from sample to sample
struct TsdfCastLane {
  double o[3], u[3];
  TsdfBlockCache cache_total, cache_own;
  int samples;
};

struct TsdfCastResult {
  int32_t face;
  double t, inc, normal[3], phi;
  int status, samples;
};

// J of the rule, or -1 where the arguments are not 0 <= t_min < t_max, both finite, 0 < step <= tau, J <= 2^24
DC_HD int tsdf_cast_steps(double t_min, double t_max, double step, double tau) {
  if (!(t_min >= 0.0) || !(t_max > t_min) || !isfinite(t_max) || !(step > 0.0) || !(step <= tau)) return -1;
  const double J = floor((t_max - t_min) / step);
  return J <= (double)kTsdfCastMaxSteps ? (int)J : -1;
}

// o and u of the rule from the widened vp, dir [3] and the pose, row-major [16]; false: the ray is SKIPPED
DC_HD bool tsdf_cast_setup(const double* vp, const double* dir, const double* pose, bool masked_in, TsdfCastLane* L) {
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double* R = pose + 4 * a;
    L->o[a] = ((R[0] * vp[0] + R[1] * vp[1]) + R[2] * vp[2]) + R[3];
    L->u[a] = (R[0] * dir[0] + R[1] * dir[1]) + R[2] * dir[2];
  }
  L->cache_total = TsdfBlockCache{kTsdfNoKey, -1};
  L->cache_own = TsdfBlockCache{kTsdfNoKey, -1};
  L->samples = 0;
  const bool finite = isfinite(L->o[0]) && isfinite(L->o[1]) && isfinite(L->o[2]) && isfinite(L->u[0]) && isfinite(L->u[1]) && isfinite(L->u[2]);
  const bool zero = L->u[0] == 0.0 && L->u[1] == 0.0 && L->u[2] == 0.0;
  return masked_in && finite && !zero;
}

// the range test and the base voxel i0 of tsdf_sample_point at the world point x; false: the sample's flag is RANGE
DC_HD bool tsdf_cast_base(const double* x, const TsdfGrid& g, int* i0) {
  double q[3];
  bool in = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    q[a] = (x[a] - g.og[a]) / g.a - 0.5;
    in = in && isfinite(x[a]) && q[a] >= -kTsdfVoxelRange && q[a] < kTsdfVoxelRange - 1.0;
  }
  if (!in) return false;
#pragma unroll
  for (int a = 0; a < 3; ++a) i0[a] = (int)floor(q[a]);
  return true;
}

DC_HD void tsdf_cast_point(const TsdfCastLane& L, double t, double* p) {
#pragma unroll
  for (int a = 0; a < 3; ++a) p[a] = L.o[a] + t * L.u[a];
}

// The sample at the parameter t.  With skipping, *absent <- the base block is missing (i0 then holds the base voxel) and no voxel is read.
DC_HD TsdfSample tsdf_cast_sample(TsdfCastLane& L, double t, const TsdfGrid& g, const TsdfCastRule& r, const TsdfTable& total,
                                  const TsdfTable& own, int* i0, bool* absent) {
  TsdfSample s{NAN, {0.0, 0.0, 0.0}, INFINITY, kTsdfSampleRange};
  double p[3];
  tsdf_cast_point(L, t, p);
  *absent = false;
  if (r.skip) {
    if (!tsdf_cast_base(p, g, i0)) return s;
    if (tsdf_table_voxel(total, i0, &L.cache_total) < 0) {
      *absent = true;
      s.flag = kTsdfSampleUnobserved;
      return s;
    }
  }
  L.samples += 1;
  return tsdf_sample_point_minus(p, g, r.tau, r.min_count, total, own, &L.cache_total, &L.cache_own);
}

// An estimate of the last j' in [j, J] whose base voxel still lies in the block of i0, one sample short of the block's exit: the
// exit of axis a is where q_a reaches the block's far face, x_a = og_a + (8 b_a + (u_a > 0 ? 8 : 0) + 0.5) a.  Only an estimate:
// the caller lands on j' and compares the blocks.
DC_HD int tsdf_cast_jump(const TsdfCastLane& L, const int* i0, const TsdfGrid& g, const TsdfCastRule& r, int j) {
  double t_exit = INFINITY;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    if (L.u[a] == 0.0) continue;
    const double edge = (double)((i0[a] >> 3) * 8 + (L.u[a] > 0.0 ? 8 : 0));
    const double te = ((g.og[a] + (edge + 0.5) * g.a) - L.o[a]) / L.u[a];
    t_exit = te < t_exit ? te : t_exit;
  }
  const double c = floor((t_exit - r.t_min) / r.step) - 1.0;
  return c >= (double)r.J ? r.J : (c > (double)j ? (int)c : j);
}

DC_HD double tsdf_cast_secant(double t0, double phi0, double t1, double phi1) { return t0 + (t1 - t0) * (phi0 / (phi0 - phi1)); }

// One ray that is not SKIPPED, from the march to the hit.
DC_HD TsdfCastResult tsdf_cast_ray(TsdfCastLane& L, const TsdfGrid& g, const TsdfCastRule& r, const TsdfTable& total, const TsdfTable& own) {
  TsdfCastResult out{-1, INFINITY, NAN, {NAN, NAN, NAN}, NAN, kTsdfCastMiss, 0};
  double t0 = 0.0, phi0 = 0.0, t1 = 0.0, phi1 = 0.0;
  bool open = false, crossing = false;
  int i0[3] = {0, 0, 0};
  bool absent;
  for (int j = 0; j <= r.J; ++j) {
    const double t = r.t_min + (double)j * r.step;
    const TsdfSample s = tsdf_cast_sample(L, t, g, r, total, own, i0, &absent);
    if (s.flag != 0) {
      open = false;
      if (absent) {
        const int jn = tsdf_cast_jump(L, i0, g, r, j);
        if (jn > j + 1) {
          double pn[3];
          int in[3];
          tsdf_cast_point(L, r.t_min + (double)jn * r.step, pn);
          if (tsdf_cast_base(pn, g, in) && (in[0] >> 3) == (i0[0] >> 3) && (in[1] >> 3) == (i0[1] >> 3) && (in[2] >> 3) == (i0[2] >> 3)) j = jn;
        }
      }
      continue;
    }
    if (s.phi > 0.0) {
      open = true;
      t0 = t;
      phi0 = s.phi;
      continue;
    }
    t1 = t;
    phi1 = s.phi;
    crossing = open;
    out.status = open ? kTsdfCastLost : kTsdfCastBehind;       // a crossing is LOST until its last sample stands
    break;
  }
  if (crossing) {
    double ts = tsdf_cast_secant(t0, phi0, t1, phi1);
    bool valid = true;
    for (int k = 0; k < r.refine && valid; ++k) {
      const TsdfSample s = tsdf_cast_sample(L, ts, g, r, total, own, i0, &absent);
      valid = s.flag == 0;
      if (!valid) break;
      if (s.phi > 0.0) { t0 = ts; phi0 = s.phi; } else { t1 = ts; phi1 = s.phi; }
      ts = tsdf_cast_secant(t0, phi0, t1, phi1);
    }
    if (valid) {
      const TsdfSample s = tsdf_cast_sample(L, ts, g, r, total, own, i0, &absent);
      const bool flat = s.grad[0] == 0.0 && s.grad[1] == 0.0 && s.grad[2] == 0.0;
      if (s.flag == 0 && !flat) {
        const double len = sqrt(surfel_dot(s.grad[0], s.grad[1], s.grad[2], s.grad[0], s.grad[1], s.grad[2]));
        const double n0 = s.grad[0] / len, n1 = s.grad[1] / len, n2 = s.grad[2] / len;
        double p[3];
        tsdf_cast_point(L, ts, p);
        tsdf_cast_base(p, g, i0);                                  // a valid sample is in range
        const SurfelRay ray{L.o[0], L.o[1], L.o[2], L.u[0], L.u[1], L.u[2]};
        out.face = (int32_t)tsdf_cached_find(total.keys, total.nb, tsdf_voxel_key(i0), &L.cache_total);
        out.t = ts;
        out.inc = acos01(fmin(1.0, surfel_cos(n0, n1, n2, ray)));
        out.normal[0] = n0; out.normal[1] = n1; out.normal[2] = n2;
        out.phi = s.phi;
        out.status = kTsdfCastHit;
      }
    }
  }
  out.samples = L.samples;
  return out;
}

}  // namespace dc
