// Per-beam arithmetic of the finite-beam renderer (dc_raycast.hip: dc_beam_subrays, dc_raycast_beams; compiled for the host by
// dc_hostcheck.cpp, so that the CPU tests pin it): the beam's frame, the sub-rays of a footprint sample, and the rules that reduce a
// bundle of sub-ray returns to one return.  The kernel evaluates the rules across lanes; the predicates it uses are the ones below,
// and beam_select states the whole reduction over arrays.  Definitions: include/dc_hip.h, DESIGN "Finite-beam rendering".
//
// No fused multiply-adds in this header: dc_beam_subrays and dc_raycast_beams inline the same functions into different kernels and
// must form bit-identical sub-rays, and a contraction the compiler chooses per call site would break that.
#pragma once
#include <math.h>
#include "dc_common.h"

#ifndef DC_BEAM_MAX_SAMPLES
#define DC_BEAM_MAX_SAMPLES 64
#define DC_BEAM_MEAN 0
#define DC_BEAM_QUANTILE 1
#define DC_BEAM_UNIFORM 0
#define DC_BEAM_LAMBERT 1
#endif

namespace dc {

// Scalars only: a runtime-indexed private array would live in scratch memory on the device.
struct BeamFrame {
  double d0, d1, d2;              // unit axis d = s / |s|
  double a0, a1, a2;              // e1 = (a x d) / |a x d|, a = the unit axis of the smallest |d_k| (ties: the lower k)
  double b0, b1, b2;              // e2 = d x e1
  bool ok;                        // false: the direction is zero or not finite, the beam is a miss
};

DC_HD BeamFrame beam_frame(double s0, double s1, double s2) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  BeamFrame f;
  const double len = sqrt(s0 * s0 + s1 * s1 + s2 * s2);
  f.d0 = s0 / len;
  f.d1 = s1 / len;
  f.d2 = s2 / len;
  f.ok = isfinite(f.d0) && isfinite(f.d1) && isfinite(f.d2) && len > 0.0;
  const double m0 = fabs(f.d0), m1 = fabs(f.d1), m2 = fabs(f.d2);
  const int k = (m0 <= m1 && m0 <= m2) ? 0 : (m1 <= m2 ? 1 : 2);
  // a x d for a = unit axis k
  const double c0 = k == 0 ? 0.0 : (k == 1 ? f.d2 : -f.d1);
  const double c1 = k == 0 ? -f.d2 : (k == 1 ? 0.0 : f.d0);
  const double c2 = k == 0 ? f.d1 : (k == 1 ? -f.d0 : 0.0);
  const double cl = sqrt(c0 * c0 + c1 * c1 + c2 * c2);
  f.a0 = c0 / cl;
  f.a1 = c1 / cl;
  f.a2 = c2 / cl;
  f.b0 = f.d1 * f.a2 - f.d2 * f.a1;
  f.b1 = f.d2 * f.a0 - f.d0 * f.a2;
  f.b2 = f.d0 * f.a1 - f.d1 * f.a0;
  return f;
}

// Sub-ray of the pattern row (px, py) of a beam from the view point v: origin o = v + r0 q, direction D = d + spread q with
// q = px e1 + py e2.  D is not normalised: D . d = 1, so the cast's t is the axial depth.  NaN for a beam without a frame.
DC_HD void beam_subray(const BeamFrame& f, double v0, double v1, double v2, double px, double py, double r0, double spread, double* o,
                       double* D) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (!f.ok) {
    o[0] = o[1] = o[2] = D[0] = D[1] = D[2] = NAN;
    return;
  }
  const double q0 = px * f.a0 + py * f.b0, q1 = px * f.a1 + py * f.b1, q2 = px * f.a2 + py * f.b2;
  o[0] = v0 + r0 * q0;
  o[1] = v1 + r0 * q1;
  o[2] = v2 + r0 * q2;
  D[0] = f.d0 + spread * q0;
  D[1] = f.d1 + spread * q1;
  D[2] = f.d2 + spread * q2;
}

// ---- the rules of the reduction ----
// a sample is a hit when its sub-ray found a face and its weight is finite
DC_HD bool beam_is_hit(int32_t face, double w) { return face >= 0 && isfinite(w); }
// the order of the hits: by (t, j) ascending
DC_HD bool beam_before(double ta, int ja, double tb, int jb) { return ta < tb || (ta == tb && ja < jb); }
// the quantile's threshold on the running weight c of the ordered hits (c_last: the last one)
DC_HD bool beam_reached(double c, double tau, double c_last) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return c >= tau * c_last;
}
// the sample whose face the beam reports: the smallest |t - depth|, ties to the lower j (callers walk j ascending)
DC_HD bool beam_closer(double dist, double best) { return dist < best; }
// a beam without enough hits, or without weight, is a miss
DC_HD bool beam_is_miss(int n_hits, int min_hits, double total) { return n_hits < min_hits || !(total > 0.0); }

// The whole reduction of one bundle of n_samples <= DC_BEAM_MAX_SAMPLES returns (sub_face / sub_t / sub_w as dc_raycast_beams
// writes them): what the kernel computes across the lanes of a beam, written over arrays.
DC_HD void beam_select(const int32_t* sub_face, const double* sub_t, const double* sub_w, int n_samples, int detection, double tau,
                       int min_hits, int32_t* face_out, double* depth_out, int32_t* n_hits_out) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  int n_hits = 0;
  for (int j = 0; j < n_samples; ++j) n_hits += beam_is_hit(sub_face[j], sub_w[j]) ? 1 : 0;
  double total = 0.0, depth = INFINITY;
  if (detection == DC_BEAM_MEAN) {
    double swt = 0.0;
    for (int j = 0; j < n_samples; ++j) {
      if (!beam_is_hit(sub_face[j], sub_w[j])) continue;
      total += sub_w[j];
      swt += sub_w[j] * sub_t[j];
    }
    depth = swt / total;
  } else {
    int order[DC_BEAM_MAX_SAMPLES];                             // order[m] = the sample at place m of the hits ordered by (t, j)
    for (int j = 0; j < n_samples; ++j) {
      if (!beam_is_hit(sub_face[j], sub_w[j])) continue;
      int rank = 0;
      for (int i = 0; i < n_samples; ++i)
        rank += (beam_is_hit(sub_face[i], sub_w[i]) && beam_before(sub_t[i], i, sub_t[j], j)) ? 1 : 0;
      order[rank] = j;
    }
    for (int m = 0; m < n_hits; ++m) total += sub_w[order[m]];   // one at a time, in that order
    double c = 0.0;
    for (int m = 0; m < n_hits; ++m) {
      c += sub_w[order[m]];
      if (beam_reached(c, tau, total)) { depth = sub_t[order[m]]; break; }
    }
  }
  *n_hits_out = n_hits;
  if (beam_is_miss(n_hits, min_hits, total)) {
    *face_out = -1;
    *depth_out = INFINITY;
    return;
  }
  int best = -1;
  double best_dist = INFINITY;
  for (int j = 0; j < n_samples; ++j) {
    if (!beam_is_hit(sub_face[j], sub_w[j])) continue;
    const double dist = fabs(sub_t[j] - depth);
    if (beam_closer(dist, best_dist)) { best_dist = dist; best = j; }
  }
  *face_out = best >= 0 ? sub_face[best] : -1;
  *depth_out = best >= 0 ? depth : INFINITY;
}

}  // namespace dc
