// The per-row arithmetic of the map's dynamic-point probabilities (dc_dynamic.hip), shared by the kernels and the test-only host
// build (dc_hostcheck.cpp): the direction and depth of a point as the sensor sees it, and the Bayesian update of one map point that a
// beam of the reading passed by or ended on.  The rule follows Pomerleau et al., "Long-term 3D map maintenance in dynamic
// environments" (ICRA 2014), the method behind norlab_icp_mapper's compute_prob_dynamic (launch/slam.launch); DESIGN "Dynamic points
// in the map" states it and its deviations.  Everything is fp64; sums and products are unfused and in the order written, so the
// host build, the kernels and the numpy oracle (tests/dynamic_reference.py) agree bit for bit.
#pragma once
#include <math.h>
#include "dc_common.h"

namespace dc {

constexpr double kDynEps = 1e-4;       // the floor of every weight, and the probabilities a dynamic point is pinned to

constexpr int kDynSeenOccluded = 1;    // seen_out codes of dc_dyn_update
constexpr int kDynSeenUpdated = 2;

struct DynParams {
  double chord_max, epsilon_a, epsilon_d, alpha, beta, threshold, max_range;
};

// The argument checks of dc_dyn_update (chord_max = 2 sin(beam_half_angle) with 0 < beam_half_angle < pi / 2).
DC_HD bool dyn_params_ok(const DynParams& p) {
  return p.chord_max > 0.0 && p.chord_max < 2.0 && p.epsilon_a >= 0.0 && isfinite(p.epsilon_a) && p.epsilon_d >= 0.0 &&
         isfinite(p.epsilon_d) && p.alpha > 0.0 && p.alpha < 1.0 && p.beta > 0.0 && p.beta < 1.0 && p.threshold > 0.0 &&
         p.threshold <= 1.0 && p.max_range == p.max_range;
}

// Point q as the sensor at T (row-major 4 x 4, world from sensor; NULL: q is in the sensor frame already) sees it: d = q - t,
// x = R^T d with x_r = (R[0][r] d0 + R[1][r] d1) + R[2][r] d2, rho = sqrt((x0^2 + x1^2) + x2^2), u = x / rho.  Returns whether the
// row is valid: rho finite, > 0 and <= max_range (max_range <= 0 or inf: no bound); u is zero otherwise.
DC_HD bool dyn_direction(const double* T, const double* q, double max_range, double* d, double* x, double* rho, double* u) {
#pragma clang fp contract(off)
  if (T) {
    d[0] = q[0] - T[3]; d[1] = q[1] - T[7]; d[2] = q[2] - T[11];
    for (int r = 0; r < 3; ++r) x[r] = (T[r] * d[0] + T[4 + r] * d[1]) + T[8 + r] * d[2];
  } else {
    for (int r = 0; r < 3; ++r) { d[r] = q[r]; x[r] = q[r]; }
  }
  const double rr = sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]);
  *rho = rr;
  bool ok = isfinite(rr) && rr > 0.0;
  if (ok && max_range > 0.0 && isfinite(max_range)) ok = rr <= max_range;
  for (int r = 0; r < 3; ++r) u[r] = ok ? x[r] / rr : 0.0;
  return ok;
}

// One map point (x, rho, d of dyn_direction; normal n, world frame; probability *P) against the reading point p (sensor frame) whose
// direction is its nearest one, at the chord c < chord_max.  Returns 0 (an invalid reading point: nothing done), kDynSeenOccluded
// (the map point lies behind what the beam hit: *P left as it is) or kDynSeenUpdated (*P updated).
DC_HD int dyn_update_row(const DynParams& prm, const double* x, double rho, const double* d, const double* n, const double* p, double c,
                         double* P) {
#pragma clang fp contract(off)
  const double eps = kDynEps, one = 1.0 - kDynEps;
  const double r = sqrt((p[0] * p[0] + p[1] * p[1]) + p[2] * p[2]);
  if (!(isfinite(r) && r > 0.0)) return 0;
  const double e0 = p[0] - x[0], e1 = p[1] - x[1], e2 = p[2] - x[2];
  const double delta = sqrt((e0 * e0 + e1 * e1) + e2 * e2);
  const double d_max = prm.epsilon_a * r;
  if (!((r + prm.epsilon_d) + d_max >= rho)) return kDynSeenOccluded;
  const double w_v = eps + one * fabs((n[0] * d[0] + n[1] * d[1]) + n[2] * d[2]) / rho;
  const double w_d1 = eps + one * (1.0 - c / prm.chord_max);
  const double offset = delta - prm.epsilon_d;
  double w_d2, w_p2;
  if (delta < prm.epsilon_d || rho > r) w_d2 = eps;
  else if (offset < d_max) w_d2 = eps + one * offset / d_max;
  else w_d2 = 1.0;
  if (delta < prm.epsilon_d) w_p2 = 1.0;
  else if (offset < d_max) w_p2 = eps + one * (1.0 - offset / d_max);
  else w_p2 = eps;
  const double c2 = w_v * w_d1, c1 = 1.0 - c2;
  const double P0 = *P;
  double pd, ps;
  if (P0 < prm.threshold) {
    pd = c1 * P0 + (c2 * w_d2) * ((1.0 - prm.alpha) * (1.0 - P0) + prm.beta * P0);
    ps = c1 * (1.0 - P0) + (c2 * w_p2) * (prm.alpha * (1.0 - P0) + (1.0 - prm.beta) * P0);
  } else {                                      // a point once dynamic stays dynamic
    pd = one;
    ps = eps;
  }
  *P = pd / (pd + ps);
  return kDynSeenUpdated;
}

// Entry i of dc_dyn_update's tables, with nothing taken on trust: the map row, the match and the ranges are checked here.
DC_HD void dyn_update_entry(const DynParams& prm, const double* map_points, const double* map_normals, int64_t n_map, const double* T,
                            const double* reading, int64_t m, int64_t row, int64_t j, double c, double* prob, uint8_t* seen) {
  if (row < 0 || row >= n_map || j < 0 || j >= m || !(c < prm.chord_max)) return;
  const double q[3] = {map_points[row * 3], map_points[row * 3 + 1], map_points[row * 3 + 2]};
  double d[3], x[3], u[3], rho;
  if (!dyn_direction(T, q, prm.max_range, d, x, &rho, u)) return;
  const double n[3] = {map_normals[row * 3], map_normals[row * 3 + 1], map_normals[row * 3 + 2]};
  const double p[3] = {reading[j * 3], reading[j * 3 + 1], reading[j * 3 + 2]};
  double P = prob[row];
  const int code = dyn_update_row(prm, x, rho, d, n, p, c, &P);
  if (code == kDynSeenUpdated) prob[row] = P;
  if (seen && code != 0) seen[row] = (uint8_t)code;
}

}  // namespace dc
