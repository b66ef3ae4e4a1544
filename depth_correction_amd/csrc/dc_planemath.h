// Per-element arithmetic of the plane neighbourhoods (dc_planes.hip), host and device: the RANSAC hypothesis with its degeneracy
// rule, the inlier predicate, the best key, the refit from the ten summed moments, and the plane features (model value and
// derivatives, plane point, Bessel covariance, per-point backward).  dc_hostcheck.cpp compiles it for the host, so that the CPU
// tests pin it against a high-precision reference (tests/planes_reference.py) and the GPU tests compare the kernels with it.
//
// Everything up to and including plane_refit gives the same bits on the host and on the device: only IEEE +, -, *, /, sqrt and
// fma, each function under `fp contract(off)` with the fused operations spelled out.  (The model functions call cos / sin / pow,
// whose last bits depend on the maths library: they are pinned by error bounds.)  The stated operation orders:
//   residual of x against the plane (n, d):   r = fma(n2, x2, fma(n1, x1, n0 * x0)) + d,   inlier when |r| <= thresh
//   cross product:                            c0 = fma(u1, v2, -(u2 * v1)), and cyclically
//   squared norm:                             fma(a2, a2, fma(a1, a1, a0 * a0))
//   moments:                                  S_ab = fma(da, db, S_ab), s_a += da, count += 1
#pragma once
#include <math.h>
#include "dc_common.h"
#include "dc_pointmath.h"
#include "dc_rng.h"

namespace dc {

constexpr int kPlaneBlock = 256;             // threads of every plane kernel: the width of the reduction tree
constexpr int kRefitBlocksMax = 1024;        // blocks of the refit's moments kernel (grid stride beyond)

template <typename T>
DC_HD void load3(const T* p, int64_t i, double* x) {
  x[0] = (double)p[i * 3]; x[1] = (double)p[i * 3 + 1]; x[2] = (double)p[i * 3 + 2];
}

// ---- RANSAC -------------------------------------------------------------------------------------------------------
// positions in the remaining-point list that hypothesis h of round `round` draws
DC_HD void ransac_draw(uint64_t seed, int64_t round, int h, int64_t n_rem, int64_t* j) {
  for (int t = 0; t < 3; ++t)
    j[t] = (int64_t)(splitmix64(seed ^ ((uint64_t)round << 40) ^ ((uint64_t)h << 2) ^ (uint64_t)t) % (uint64_t)n_rem);
}

DC_HD double dot3_fma(const double* a, const double* b) { return fma(a[2], b[2], fma(a[1], b[1], a[0] * b[0])); }

// pl [4] <- the plane (n, d) through p0, p1, p2, or (0, 0, 0, +inf) for a degenerate hypothesis (positions not distinct, or
// |u x v| <= 1e-12 |u| |v|): a plane with d = +inf has no inlier.  Returns whether the hypothesis is valid.
DC_HD bool plane_from_points(const double* p0, const double* p1, const double* p2, bool distinct, double* pl) {
#pragma clang fp contract(off)
  const double u[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]};
  const double v[3] = {p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]};
  const double c[3] = {fma(u[1], v[2], -(u[2] * v[1])), fma(u[2], v[0], -(u[0] * v[2])), fma(u[0], v[1], -(u[1] * v[0]))};
  const double nc = sqrt(dot3_fma(c, c)), nu = sqrt(dot3_fma(u, u)), nv = sqrt(dot3_fma(v, v));
  const bool ok = distinct && nc > 1e-12 * nu * nv;
  pl[0] = pl[1] = pl[2] = 0.0;
  pl[3] = (double)INFINITY;
  if (ok) {
    pl[0] = c[0] / nc; pl[1] = c[1] / nc; pl[2] = c[2] / nc;
    pl[3] = -dot3_fma(pl, p0);
  }
  return ok;
}

// |n . x + d| <= thresh in the stated order; NaN and inf coordinates, and the plane of a degenerate hypothesis, give false
DC_HD bool plane_inlier(const double* pl, const double* x, double thresh) {
#pragma clang fp contract(off)
  const double r = fma(pl[2], x[2], fma(pl[1], x[1], pl[0] * x[0])) + pl[3];
  return fabs(r) <= thresh;
}

// the larger key wins: the larger count, then the lower h; a degenerate hypothesis counts -1
DC_HD int64_t ransac_best_key(int32_t count, bool valid, int H, int h) {
  const int32_t c = valid ? count : -1;
  return (int64_t)((uint64_t)(int64_t)c << 32) | (int64_t)(uint32_t)(H - 1 - h);
}

DC_HD void ransac_best_decode(int64_t key, int H, int32_t* best) {
  best[0] = H - 1 - (int32_t)(uint32_t)(key & 0xffffffffll);
  best[1] = (int32_t)(key >> 32);
}

// v [10] += one inlier's moments about the anchor a: count, s (3), S (6: xx xy xz yy yz zz)
DC_HD void refit_moments_add(const double* x, const double* a, double* v) {
#pragma clang fp contract(off)
  const double dx = x[0] - a[0], dy = x[1] - a[1], dz = x[2] - a[2];
  v[0] += 1.0; v[1] += dx; v[2] += dy; v[3] += dz;
  v[4] = fma(dx, dx, v[4]); v[5] = fma(dx, dy, v[5]); v[6] = fma(dx, dz, v[6]);
  v[7] = fma(dy, dy, v[7]); v[8] = fma(dy, dz, v[8]); v[9] = fma(dz, dz, v[9]);
}

// One Jacobi rotation of the symmetric 3 x 3 matrix in the (p, q) plane (r the third index): app, aqq, apq its entries there,
// arp / arq the other two, vp / vq the columns p and q of the eigenvector matrix.
DC_HD void jacobi_rotate(double& app, double& aqq, double& apq, double& arp, double& arq, double* vp, double* vq) {
#pragma clang fp contract(off)
  if (apq == 0.0) return;
  const double theta = (aqq - app) / (2.0 * apq);
  const double t = copysign(1.0, theta) / (fabs(theta) + sqrt(theta * theta + 1.0));
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
  app = app - t * apq;
  aqq = aqq + t * apq;
  apq = 0.0;
  const double rp = c * arp - s * arq, rq = s * arp + c * arq;
  arp = rp; arq = rq;
  for (int k = 0; k < 3; ++k) {
    const double a = c * vp[k] - s * vq[k], b = s * vp[k] + c * vq[k];
    vp[k] = a; vq[k] = b;
  }
}

// Unit eigenvector of the smallest eigenvalue of the symmetric matrix C (xx xy xz yy yz zz): cyclic Jacobi, a fixed number of
// sweeps (it converges quadratically; 8 sweeps leave the off-diagonal far below one rounding of the diagonal).  On equal
// eigenvalues the lowest column wins.  Unlike eig3_sym (hardware reciprocal square root and the maths library's acos / cos on the
// device) this gives the same bits on the host and on the device.
DC_HD void smallest_eigvec_jacobi(const double* C, double* nv) {
  double a00 = C[0], a01 = C[1], a02 = C[2], a11 = C[3], a12 = C[4], a22 = C[5];
  double v0[3] = {1.0, 0.0, 0.0}, v1[3] = {0.0, 1.0, 0.0}, v2[3] = {0.0, 0.0, 1.0};
  for (int sweep = 0; sweep < 8; ++sweep) {
    jacobi_rotate(a00, a11, a01, a02, a12, v0, v1);
    jacobi_rotate(a00, a22, a02, a01, a12, v0, v2);
    jacobi_rotate(a11, a22, a12, a01, a02, v1, v2);
  }
  const double* best = v0;
  double lam = a00;
  if (a11 < lam) { lam = a11; best = v1; }
  if (a22 < lam) { lam = a22; best = v2; }
  nv[0] = best[0]; nv[1] = best[1]; nv[2] = best[2];
}

// params [4] <- the least-squares plane of the inliers from their ten summed moments v about the anchor: covariance, the
// eigenvector of its smallest eigenvalue, its largest-magnitude component made positive, d = -n . centroid
DC_HD void plane_refit(const double* v, const double* anchor, double* params) {
#pragma clang fp contract(off)
  const double n = v[0];
  const double m[3] = {v[1] / n, v[2] / n, v[3] / n};
  const double C[6] = {fma(-m[0], m[0], v[4] / n), fma(-m[0], m[1], v[5] / n), fma(-m[0], m[2], v[6] / n),
                       fma(-m[1], m[1], v[7] / n), fma(-m[1], m[2], v[8] / n), fma(-m[2], m[2], v[9] / n)};
  double nv[3];
  smallest_eigvec_jacobi(C, nv);
  const double inv = 1.0 / sqrt(dot3_fma(nv, nv));
  int kmax = 0;
  if (fabs(nv[1]) > fabs(nv[kmax])) kmax = 1;
  if (fabs(nv[2]) > fabs(nv[kmax])) kmax = 2;
  const double sg = (kmax == 0 ? nv[0] : (kmax == 1 ? nv[1] : nv[2])) < 0.0 ? -inv : inv;
  for (int k = 0; k < 3; ++k) nv[k] *= sg;
  const double c[3] = {anchor[0] + m[0], anchor[1] + m[1], anchor[2] + m[2]};
  params[0] = nv[0]; params[1] = nv[1]; params[2] = nv[2];
  params[3] = -dot3_fma(nv, c);
}

// ---- plane features -----------------------------------------------------------------------------------------------
DC_HD void load_model_params(int kind, int n_terms, const double* w, const double* e, ModelParams& mp) {
  mp.kind = kind;
  mp.n_terms = n_terms;
#pragma unroll
  for (int k = 0; k < DC_MAX_MODEL_TERMS; ++k) {
    mp.w[k] = (k < n_terms && w) ? w[k] : 0.0;
    mp.e[k] = (k < n_terms && e) ? e[k] : 0.0;
  }
}

// d'(d, gamma) and its partial derivatives (the polynomial kinds: model.py:181-199, 243-261; the others: model_depth)
DC_HD double model_eval(const ModelParams& mp, double d, double g, double* dd, double* dg) {
  const int kind = mp.kind;
  if (kind == DC_MODEL_NONE) { *dd = 1.0; *dg = 0.0; return d; }
  if (kind == DC_MODEL_LINEAR) { *dd = mp.w[0]; *dg = mp.w[1]; return mp.w[0] * d + mp.w[1] * g + mp.w[2]; }
  if (kind == DC_MODEL_INVCOS || kind == DC_MODEL_SCALED_INVCOS) {
    const double c = cos(g), s = sin(g);
    const double t = mp.w[0] * s / (c * c);                  // d/dg (w0 / cos g); |cos g| = cos g on [0, pi/2]
    if (kind == DC_MODEL_INVCOS) { *dd = 1.0; *dg = -t; return d - mp.w[0] / c; }
    const double f = 1.0 - mp.w[0] / fabs(c);
    *dd = f; *dg = -d * t;
    return d * f;
  }
  double b = 0.0, db = 0.0;
#pragma unroll
  for (int k = 0; k < DC_MAX_MODEL_TERMS; ++k)
    if (k < mp.n_terms) {
      b += pow_term(g, mp.e[k]) * mp.w[k];
      if (mp.e[k] != 0.0) db += mp.w[k] * mp.e[k] * pow_term(g, mp.e[k] - 1.0);
    }
  if (kind == DC_MODEL_SCALED_POLYNOMIAL) { *dd = 1.0 - b; *dg = -d * db; return d * (1.0 - b); }
  *dd = 1.0; *dg = -db;
  return d - b;
}

// dd'/dw_k
DC_HD double model_dw(const ModelParams& mp, int k, double d, double g) {
  if (mp.kind == DC_MODEL_POLYNOMIAL) return -pow_term(g, mp.e[k]);
  if (mp.kind == DC_MODEL_SCALED_POLYNOMIAL) return -d * pow_term(g, mp.e[k]);
  return model_dw_other(mp, k, d, g);
}

struct PlanePoint {
  double vp[3], dir[3], d, c, g, dp, ddp_dd, ddp_dg, x[3];
};

// the corrected point x = vp + d'(d, gamma) dir of cloud row i on a plane of normal n, gamma = arccos |dir . n|
template <typename T>
DC_HD void plane_point(const T* vps, const T* dirs, const T* depth, int64_t i, const double* n, const ModelParams& mp, PlanePoint& q) {
  load3(vps, i, q.vp);
  load3(dirs, i, q.dir);
  q.d = (double)depth[i];
  q.c = q.dir[0] * n[0] + q.dir[1] * n[1] + q.dir[2] * n[2];
  const double a = fabs(q.c);
  q.g = acos(a > 1.0 ? 1.0 : a);
  q.dp = model_eval(mp, q.d, q.g, &q.ddp_dd, &q.ddp_dg);
  for (int k = 0; k < 3; ++k) q.x[k] = q.vp[k] + q.dp * q.dir[k];
}

// v [9] += one plane point's moments about the anchor a: s (3), S (6)
DC_HD void plane_moments_add(const double* x, const double* a, double* v) {
  const double dx = x[0] - a[0], dy = x[1] - a[1], dz = x[2] - a[2];
  v[0] += dx; v[1] += dy; v[2] += dz;
  v[3] = fma(dx, dx, v[3]); v[4] = fma(dx, dy, v[4]); v[5] = fma(dx, dz, v[5]);
  v[6] = fma(dy, dy, v[6]); v[7] = fma(dy, dz, v[7]); v[8] = fma(dz, dz, v[8]);
}

// cov [9] (row-major 3 x 3, Bessel) and mean [3] from the nine moments v of n points about the anchor a.
// n = 1: inf * 0 = NaN, like torch.cov of one observation
DC_HD void plane_cov_finish(const double* v, double n, const double* a, double* cov, double* mean) {
  const double s[3] = {v[0], v[1], v[2]};
  const double f = 1.0 / (n - 1.0);
  const double C[6] = {(v[3] - s[0] * s[0] / n) * f, (v[4] - s[0] * s[1] / n) * f, (v[5] - s[0] * s[2] / n) * f,
                       (v[6] - s[1] * s[1] / n) * f, (v[7] - s[1] * s[2] / n) * f, (v[8] - s[2] * s[2] / n) * f};
  cov[0] = C[0]; cov[1] = C[1]; cov[2] = C[2];
  cov[3] = C[1]; cov[4] = C[3]; cov[5] = C[4];
  cov[6] = C[2]; cov[7] = C[4]; cov[8] = C[5];
  for (int k = 0; k < 3; ++k) mean[k] = a[k] + s[k] / n;
}

// M = (G + G^T) / (n - 1) of the upstream gradient G [9] of a plane's covariance
DC_HD void plane_bwd_matrix(const double* G, double n_minus_1, double (*M)[3]) {
  const double f = 1.0 / n_minus_1;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) M[r][c] = (G[r * 3 + c] + G[c * 3 + r]) * f;
}

// One point's backward: dL/dx = M (x - mean), chained through x = vp + d'(d, gamma) dir.  gx [3] is the gradient to the viewpoint,
// gdir [3] to the direction, *gdepth to the depth; returns dL/dd', which the weight gradients multiply by model_dw.
// d gamma / d dir = -sign(c) / sqrt(1 - c^2) n, and zero where the arccos has no derivative (c = +-1) and without a model.
DC_HD double plane_bwd_point(const PlanePoint& q, const double* n, const double (*M)[3], const double* mu, int kind, double* gx,
                             double* gdir, double* gdepth) {
  const double dx[3] = {q.x[0] - mu[0], q.x[1] - mu[1], q.x[2] - mu[2]};
  for (int k = 0; k < 3; ++k) gx[k] = M[k][0] * dx[0] + M[k][1] * dx[1] + M[k][2] * dx[2];
  const double gdp = gx[0] * q.dir[0] + gx[1] * q.dir[1] + gx[2] * q.dir[2];
  const double s2 = 1.0 - q.c * q.c;
  const double sgn = q.c > 0.0 ? 1.0 : (q.c < 0.0 ? -1.0 : 0.0);
  const double gg = (s2 > 0.0 && kind != DC_MODEL_NONE) ? gdp * q.ddp_dg * (-sgn / sqrt(s2)) : 0.0;
  for (int k = 0; k < 3; ++k) gdir[k] = gx[k] * q.dp + gg * n[k];
  *gdepth = gdp * q.ddp_dd;
  return gdp;
}

}  // namespace dc
