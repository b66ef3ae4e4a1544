// Per-ray arithmetic of the depth-bias evaluation (dc_bias.hip; compiled for the host by dc_hostcheck.cpp, so that the CPU tests pin
// it): residual, relative residual, angle error, the used-ray rule, the bin rule and the terms of the two least-squares systems.
// Definitions and the layout of `out`: include/dc_hip.h, DESIGN "Depth bias against the mesh".
#pragma once
#include <math.h>
#include "dc_common.h"
#include "dc_pointmath.h"

#ifndef DC_BIAS_MAX_BINS
#define DC_BIAS_MAX_BINS 256
#define DC_BIAS_MAX_TERMS 4
#define DC_BIAS_TOTALS 5
#define DC_BIAS_BIN_COLS 9
#define DC_BIAS_SYSTEM(p) (2 + (p) + (p) * ((p) + 1) / 2)
#define DC_BIAS_OUT_COUNT(b, p) (DC_BIAS_TOTALS + DC_BIAS_BIN_COLS * (b) + 2 * DC_BIAS_SYSTEM(p))
#endif

namespace dc {

constexpr int kBiasBinVals = DC_BIAS_BIN_COLS - 1;                     // staged per ray: every column but the count
constexpr int kBiasSysFull = DC_BIAS_SYSTEM(DC_BIAS_MAX_TERMS);        // a system padded to DC_BIAS_MAX_TERMS terms
constexpr int kBiasFlat = DC_BIAS_TOTALS + 2 * kBiasSysFull;           // values that are not binned: the totals and both systems
constexpr double kBiasHalfPi = 1.57079632679489661923;

struct BiasParams {
  int kind;                       // DC_MODEL_POLYNOMIAL (y = r) | DC_MODEL_SCALED_POLYNOMIAL (y = rho)
  int n_terms, n_bins;
  double max_residual;            // <= 0: no gate
  double e[DC_BIAS_MAX_TERMS];
};

struct BiasRay {
  int bin;                        // bin of a used ray, -1 otherwise
  bool in_mask, hit, gated, has_est;
  double r, rho, delta, y;
};

// bin of a true incidence angle in [0, pi / 2]
DC_HD int bias_bin(double g, int n_bins) {
  const double q = floor(g * (double)n_bins / kBiasHalfPi);
  const int b = q < 0.0 ? 0 : (q >= (double)n_bins ? n_bins - 1 : (int)q);
  return b;
}

DC_HD BiasRay bias_ray(const BiasParams& prm, double d, double g_est, bool in_mask, int face, double t, double g) {
  BiasRay o;
  o.bin = -1;
  o.in_mask = in_mask;
  o.hit = in_mask && face >= 0 && isfinite(t) && isfinite(g);
  o.gated = false;
  o.has_est = false;
  o.r = o.rho = o.delta = o.y = 0.0;
  if (!o.hit || !(d > 0.0) || !isfinite(d)) return o;
  const double r = d - t;
  if (prm.max_residual > 0.0 && !(fabs(r) <= prm.max_residual)) { o.gated = true; return o; }
  o.r = r;
  o.rho = r / d;
  o.y = prm.kind == DC_MODEL_SCALED_POLYNOMIAL ? o.rho : r;
  o.has_est = isfinite(g_est);
  o.delta = o.has_est ? g_est - g : 0.0;
  o.bin = bias_bin(g, prm.n_bins);
  return o;
}

// v[0 .. kBiasBinVals): the columns 1 .. 8 of a used ray's bin row
DC_HD void bias_bin_terms(const BiasRay& o, double* v) {
  v[0] = o.r;
  v[1] = o.r * o.r;
  v[2] = fabs(o.r);
  v[3] = o.rho;
  v[4] = o.rho * o.rho;
  v[5] = o.delta;
  v[6] = o.delta * o.delta;
  v[7] = o.has_est ? 1.0 : 0.0;
}

// v[0 .. kBiasSysFull) += the terms of one ray of a system padded to DC_BIAS_MAX_TERMS terms (phi_k = 0 for k >= n_terms): count, the
// upper triangle of phi phi^T row by row, phi y, y^2.  Fixed trip counts: v stays in registers.
DC_HD void bias_system_add(const BiasParams& prm, double x, double y, double* v) {
  double phi[DC_BIAS_MAX_TERMS];
#pragma unroll
  for (int k = 0; k < DC_BIAS_MAX_TERMS; ++k) phi[k] = k < prm.n_terms ? pow_term(x, prm.e[k]) : 0.0;
  v[0] += 1.0;
  int q = 1;
#pragma unroll
  for (int a = 0; a < DC_BIAS_MAX_TERMS; ++a)
#pragma unroll
    for (int b = a; b < DC_BIAS_MAX_TERMS; ++b) v[q++] += phi[a] * phi[b];
#pragma unroll
  for (int a = 0; a < DC_BIAS_MAX_TERMS; ++a) v[q++] += phi[a] * y;
  v[q] += y * y;
}

// flat[0 .. kBiasFlat) += one ray's totals and system terms
DC_HD void bias_flat_add(const BiasParams& prm, const BiasRay& o, double g, double g_est, double* flat) {
  flat[0] += 1.0;
  if (o.in_mask) flat[1] += 1.0;
  if (o.hit) flat[2] += 1.0;
  if (o.gated) flat[4] += 1.0;
  if (o.bin < 0) return;
  flat[3] += 1.0;
  bias_system_add(prm, g, o.y, flat + DC_BIAS_TOTALS);
  if (o.has_est) bias_system_add(prm, g_est, o.y, flat + DC_BIAS_TOTALS + kBiasSysFull);
}

// position in `out` of entry j of the padded flat vector, or -1 for an entry of the padding
DC_HD int bias_flat_to_out(int j, int n_bins, int P) {
  if (j < DC_BIAS_TOTALS) return j;
  j -= DC_BIAS_TOTALS;
  const int s = j / kBiasSysFull, q = j - s * kBiasSysFull;
  const int base = DC_BIAS_TOTALS + DC_BIAS_BIN_COLS * n_bins + s * DC_BIAS_SYSTEM(P);
  if (q == 0) return base;
  constexpr int M = DC_BIAS_MAX_TERMS, T = M * (M + 1) / 2;
  if (q < 1 + T) {
    int a = 0, rem = q - 1;
    while (rem >= M - a) { rem -= M - a; ++a; }
    const int b = a + rem;
    if (a >= P || b >= P) return -1;
    return base + 1 + (a * P - a * (a - 1) / 2) + (b - a);
  }
  if (q < 1 + T + M) {
    const int a = q - 1 - T;
    return a < P ? base + 1 + P * (P + 1) / 2 + a : -1;
  }
  return base + 1 + P * (P + 1) / 2 + P;
}

}  // namespace dc
