// Symmetric 3x3 eigen-decomposition for per-neighbourhood covariance matrices.
//
// Replaces torch.linalg.eigh (LAPACK syevd) at reference depth_cloud.py:376-399.  Requirements taken
// from the reference's only known-answer test (loss.py:714-735: eigenvalues atol 1e-6, eigenvectors
// atol 1e-5 up to sign) and from BASELINE.json (eigenvalues within 1e-5 relative): the absolute error
// must stay O(eps * |C|) for EVERY eigenvalue, including clustered small ones (collinear lidar rings
// give l0 ~ l1 << l2), where the plain trigonometric closed form loses half the digits.
//
// Method: scale by max|c_ij|; trigonometric roots of the characteristic cubic pick the ISOLATED
// eigenvalue (largest if det(B) >= 0, else smallest), whose value and eigenvector (largest cross
// product of two rows of C - l*I) are well conditioned; the remaining pair comes from the exact 2x2
// problem in the orthogonal complement, so a cluster is resolved at its own scale.  No iteration, no
// data-dependent loop: one wavefront's lanes stay converged except for two short selects.
#pragma once
#include "dc_common.h"
#include <math.h>

namespace dc {

#if defined(__HIPCC__) && defined(__HIP_DEVICE_COMPILE__)
template <typename R> DC_HD R rsqrt_(R x) { return (R)rsqrt((double)x); }       // v_rsq_f64 + refinement, no division
// 1 / x for a normal, finite, non-zero x (counts, traces, clamped denominators): v_rcp_f64 and two Newton steps instead of the IEEE
// division sequence (div_scale x2, rcp, fma x5, div_fmas, div_fixup); <= 1 ulp.
// Measured on an MI355X over 2^20 arguments: v_rcp_f64 is within 4.6e-8 (2^-24.4) and v_rsq_f64 within 5.2e-8 (2^-24.2) of the
// exact value; one Newton step leaves 2.1e-15 and 4.1e-15, two leave the rounding of the last operation (1.4e-16 for the root).
DC_HD double recip_(double x) {
  double r = __builtin_amdgcn_rcp(x);
  r = fma(fma(-x, r, 1.0), r, r);
  return fma(fma(-x, r, 1.0), r, r);
}
// the same with ONE Newton step (a few 1e-15 relative: for a factor that scales its result as a whole, like the reciprocal of a
// trace, or that normalises a vector of which the direction is used, or whose length error is budgeted: see rsqrt2_) and the raw instruction (a correction term that is itself
// ~1e-6 of its sum needs no more); rsqrt likewise
DC_HD double recip1_(double x) {
  const double r = __builtin_amdgcn_rcp(x);
  return fma(fma(-x, r, 1.0), r, r);
}
DC_HD double rcp_raw_(double x) { return __builtin_amdgcn_rcp(x); }
DC_HD double rsq_raw_(double x) { return __builtin_amdgcn_rsq(x); }              // v_rsq_f64 as it stands (~2^-24)
DC_HD double rsqrt1_(double x) {
  const double y = __builtin_amdgcn_rsq(x);
  const double e = fma(-x * y, y, 1.0);          // 1 - x y^2
  return fma(0.5 * y, e, y);
}
// TWO Newton steps: for a factor whose error reaches an eigenvalue at first order (the basis of eig3_sym_v2's 2x2 problem).  A vector
// normalised with rsqrt1_ is off unit length by up to 4e-15, which is harmless where only its direction or a Rayleigh CORRECTION uses
// it, but u . A u of such a vector is off by twice that times the eigenvalue: with one step eig3_sym_v2 reached 1.0e-14 lam_max on
// isotropic neighbourhoods of 16 points, where eig3_sym is at 5e-15 (tests/test_gpu_eig_spectra.py).
// (The deflation branch of eig3_smallest_unit keeps one step for iso: there w = iso x u inherits iso's length error, so m11 = w . A w
// and m01 carry it at first order too -- up to 2 * 4e-15 lam1, 3.5e-15 lam_max where lam1 / lam_max ~ 0.44 (cos 3 ang ~ 0.999);
// 2.4e-15 measured, inside the 1e-14 contract, and needles, lam1 << lam_max, do not feel it.)
DC_HD double rsqrt2_(double x) {
  double y = __builtin_amdgcn_rsq(x);
  y = fma(0.5 * y, fma(-x * y, y, 1.0), y);
  return fma(0.5 * y, fma(-x * y, y, 1.0), y);
}
// cos for the root estimate (argument in [0, pi], result only seeds a Newton step): the hardware cosine.  cosf() would
// drag in the large-argument range reduction (~250 instructions, computed for every lane because it is select-based).
DC_HD float cos_est_(float x) { return __cosf(x); }
// raw v_sqrt_f32 / v_rcp_f32 (1 ulp, no denormal / exactness fix-up sequences): the estimate only seeds a Newton step
DC_HD float sqrt_est_(float x) { return __builtin_amdgcn_sqrtf(x); }
DC_HD float rcp_est_(float x) { return __builtin_amdgcn_rcpf(x); }
#else
template <typename R> DC_HD R rsqrt_(R x) { return R(1) / sqrt(x); }
DC_HD double recip_(double x) { return 1.0 / x; }
DC_HD double recip1_(double x) { return 1.0 / x; }
DC_HD double rcp_raw_(double x) { return 1.0 / x; }
DC_HD double rsq_raw_(double x) { return 1.0 / sqrt(x); }
DC_HD double rsqrt1_(double x) { return 1.0 / sqrt(x); }
DC_HD double rsqrt2_(double x) { return 1.0 / sqrt(x); }
DC_HD float cos_est_(float x) { return cosf(x); }
DC_HD float sqrt_est_(float x) { return sqrtf(x); }
DC_HD float rcp_est_(float x) { return 1.0f / x; }
#endif

// Which eigenvalue eig3_smallest isolates first.  With half = det(B) / (2 p^3) = cos(3 ang) the gaps of the scaled
// spectrum are  beta1 - beta0 = 2 sqrt(3) sin(ang)  and  beta2 - beta1 = 2 sqrt(3) sin(pi/3 - ang).  The SMALLEST
// eigenvalue is taken directly whenever its gap to the middle one is comfortable (half < 0.9: gap >= 0.52 p, so the
// fp32 estimate + one Newton step lands within ~1e-11 and the eigenvector's cross products are well conditioned);
// only nearly prolate spectra (half >= 0.9: lam0 ~ lam1 << lam2, collinear neighbourhoods such as a single lidar ring)
// isolate the LARGEST one (gap >= 2.7 p there) and resolve the small pair by the exact 2x2 problem in its complement.
// Planar and generic neighbourhoods therefore never execute the deflation code (it used to run for every wavefront
// holding one lane with det(B) >= 0).
constexpr float kDeflateHalf = 0.9f;
// the slimmer core (eig3_smallest_unit) takes the smallest eigenvalue directly up to here (gap >= 0.05 p), with a second Newton
// step from kNewton2Half on (gap < 0.52 p): wavefronts holding a few edge-like neighbourhoods then pay ~20 instructions instead of
// the ~100 of the deflation path, which is left to nearly exact needles
constexpr float kDeflateHalfUnit = 0.999f, kNewton2Half = 0.9f;

template <typename R>
DC_HD void cross3(const R* a, const R* b, R* c) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}

// Unit eigenvector of the symmetric matrix for a well separated eigenvalue `lam`.
template <typename R>
DC_HD void eigvec_isolated(R a00, R a01, R a02, R a11, R a12, R a22, R lam, R* v) {
  R r0[3] = {a00 - lam, a01, a02};
  R r1[3] = {a01, a11 - lam, a12};
  R r2[3] = {a02, a12, a22 - lam};
  R c0[3], c1[3], c2[3];
  cross3(r0, r1, c0);
  cross3(r0, r2, c1);
  cross3(r1, r2, c2);
  R d0 = c0[0] * c0[0] + c0[1] * c0[1] + c0[2] * c0[2];
  R d1 = c1[0] * c1[0] + c1[1] * c1[1] + c1[2] * c1[2];
  R d2 = c2[0] * c2[0] + c2[1] * c2[1] + c2[2] * c2[2];
  R dm = d0;
  R s0 = c0[0], s1 = c0[1], s2 = c0[2];
  if (d1 > dm) { dm = d1; s0 = c1[0]; s1 = c1[1]; s2 = c1[2]; }
  if (d2 > dm) { dm = d2; s0 = c2[0]; s1 = c2[1]; s2 = c2[2]; }
  if (dm > R(0)) {
    R inv = rsqrt_(dm);
    v[0] = s0 * inv; v[1] = s1 * inv; v[2] = s2 * inv;
  } else {
    v[0] = R(1); v[1] = R(0); v[2] = R(0);
  }
}

// lam[0] <= lam[1] <= lam[2]; V[k][0..2] = unit eigenvector of lam[k] (sign arbitrary).
template <typename R>
DC_HD void eig3_sym(R a00, R a01, R a02, R a11, R a12, R a22, R* lam, R (*V)[3]) {
  R m = fmax(fmax(fabs(a00), fabs(a11)), fabs(a22));
  m = fmax(m, fmax(fabs(a01), fmax(fabs(a02), fabs(a12))));
  if (!(m > R(0)) || !(m < R(INFINITY))) {   // zero matrix, or NaN/inf input: propagate like LAPACK would not throw
    R z = (m == R(0)) ? R(0) : R(NAN);
    lam[0] = lam[1] = lam[2] = z;
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) V[i][j] = (i == j) ? R(1) : R(0);
    return;
  }
  const R inv_m = R(1) / m;
  a00 *= inv_m; a01 *= inv_m; a02 *= inv_m; a11 *= inv_m; a12 *= inv_m; a22 *= inv_m;

  const R off = a01 * a01 + a02 * a02 + a12 * a12;
  const R q = (a00 + a11 + a22) * R(1.0 / 3.0);
  const R b00 = a00 - q, b11 = a11 - q, b22 = a22 - q;
  const R p2 = (b00 * b00 + b11 * b11 + b22 * b22 + R(2) * off) * R(1.0 / 6.0);
  R iso[3], u[3], w[3];
  R l_iso, l_lo, l_hi, ca, cb;
  bool iso_is_max;
  if (!(p2 > R(0))) {
    // multiple of the identity
    lam[0] = lam[1] = lam[2] = q * m;
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) V[i][j] = (i == j) ? R(1) : R(0);
    return;
  }
  {
    const R p = sqrt(p2);
    const R c00 = b11 * b22 - a12 * a12;
    const R c01 = a01 * b22 - a12 * a02;
    const R c02 = a01 * a12 - b11 * a02;
    const R det = (b00 * c00 - a01 * c01 + a02 * c02) / (p * p2);
    R half = fmin(fmax(det * R(0.5), R(-1)), R(1));
    const R ang = acos(half) * R(1.0 / 3.0);
    iso_is_max = half >= R(0);
    // beta2 = 2cos(ang) (largest), beta0 = 2cos(ang + 2pi/3) (smallest)
    const R beta = iso_is_max ? R(2) * cos(ang) : R(2) * cos(ang + R(2.0943951023931954923));
    l_iso = q + p * beta;
  }
  eigvec_isolated(a00, a01, a02, a11, a12, a22, l_iso, iso);
  // orthonormal basis (u, w) of the complement of iso
  if (fabs(iso[0]) > fabs(iso[1])) {
    R inv = rsqrt_(iso[0] * iso[0] + iso[2] * iso[2]);
    u[0] = -iso[2] * inv; u[1] = R(0); u[2] = iso[0] * inv;
  } else {
    R inv = rsqrt_(iso[1] * iso[1] + iso[2] * iso[2]);
    u[0] = R(0); u[1] = iso[2] * inv; u[2] = -iso[1] * inv;
  }
  cross3(iso, u, w);
  // A u, A w, A iso
  const R au0 = a00 * u[0] + a01 * u[1] + a02 * u[2];
  const R au1 = a01 * u[0] + a11 * u[1] + a12 * u[2];
  const R au2 = a02 * u[0] + a12 * u[1] + a22 * u[2];
  const R aw0 = a00 * w[0] + a01 * w[1] + a02 * w[2];
  const R aw1 = a01 * w[0] + a11 * w[1] + a12 * w[2];
  const R aw2 = a02 * w[0] + a12 * w[1] + a22 * w[2];
  const R ai0 = a00 * iso[0] + a01 * iso[1] + a02 * iso[2];
  const R ai1 = a01 * iso[0] + a11 * iso[1] + a12 * iso[2];
  const R ai2 = a02 * iso[0] + a12 * iso[1] + a22 * iso[2];
  l_iso = iso[0] * ai0 + iso[1] * ai1 + iso[2] * ai2;          // Rayleigh quotient
  const R m00 = u[0] * au0 + u[1] * au1 + u[2] * au2;
  const R m01 = u[0] * aw0 + u[1] * aw1 + u[2] * aw2;
  const R m11 = w[0] * aw0 + w[1] * aw1 + w[2] * aw2;
  // 2x2 symmetric eigenproblem
  const R h = (m00 - m11) * R(0.5);
  const R mean = (m00 + m11) * R(0.5);
  const R rad = sqrt(h * h + m01 * m01);
  l_hi = mean + rad;
  l_lo = mean - rad;
  // eigenvector of l_hi in (u, w) coordinates: the better conditioned of the two row null vectors
  {
    R x1 = m01, y1 = l_hi - m00;      // from row 0: (m00 - l) x + m01 y = 0
    R x2 = l_hi - m11, y2 = m01;      // from row 1
    R n1 = x1 * x1 + y1 * y1, n2 = x2 * x2 + y2 * y2;
    R x = n1 >= n2 ? x1 : x2, y = n1 >= n2 ? y1 : y2, n = n1 >= n2 ? n1 : n2;
    if (n > R(0)) { R inv = rsqrt_(n); ca = x * inv; cb = y * inv; } else { ca = R(1); cb = R(0); }
  }
  R vhi[3] = {ca * u[0] + cb * w[0], ca * u[1] + cb * w[1], ca * u[2] + cb * w[2]};
  R vlo[3] = {-cb * u[0] + ca * w[0], -cb * u[1] + ca * w[1], -cb * u[2] + ca * w[2]};
  if (iso_is_max) {
    lam[0] = l_lo; lam[1] = l_hi; lam[2] = l_iso;
    for (int j = 0; j < 3; ++j) { V[0][j] = vlo[j]; V[1][j] = vhi[j]; V[2][j] = iso[j]; }
  } else {
    lam[0] = l_iso; lam[1] = l_lo; lam[2] = l_hi;
    for (int j = 0; j < 3; ++j) { V[0][j] = iso[j]; V[1][j] = vlo[j]; V[2][j] = vhi[j]; }
  }
  // round-off can leave neighbours out of order by an ulp; restore ascending order
  for (int pass = 0; pass < 2; ++pass) {
    for (int k = 0; k < 2; ++k) {
      if (lam[k] > lam[k + 1]) {
        R t = lam[k]; lam[k] = lam[k + 1]; lam[k + 1] = t;
        for (int j = 0; j < 3; ++j) { R s = V[k][j]; V[k][j] = V[k + 1][j]; V[k + 1][j] = s; }
      }
    }
  }
  lam[0] *= m; lam[1] *= m; lam[2] *= m;
}

// Core of the hot path: smallest eigenpair of a symmetric positive semi-definite matrix of TRACE 1 (what a covariance
// divided by its trace is).  fp32 trigonometric estimate of the isolated root -> one fp64 Newton step on
// det(A - l I) -> eigenvector = the column of adj(A - l I) with the largest diagonal entry (adj = c v v^T for an
// eigenvalue, c > 0 for the smallest and for the largest one, so the diagonal is c v_k^2: its largest entry names the
// best conditioned column and the three columns share their off-diagonal cofactors: 6 products instead of 9 cross-product
// terms + 3 norms) -> Rayleigh quotient.  The Newton step reuses the adjugate: det = d0 M00 + a01 M01 + a02 M02,
// d det / dl = -(M00 + M11 + M22).
// RAYLEIGH = false leaves the eigenvalue at the Newton iterate (error <= ~1e-12 of the spread: below what 32-bit fixed-point
// coordinates resolve by orders of magnitude; the float32 / q32 kernels take it).
template <bool RAYLEIGH = true>
DC_HD void eig3_smallest_unit(double a00, double a01, double a02, double a11, double a12, double a22, double* lam, double* v0) {
  const double q = 1.0 / 3.0;
  const double b00 = a00 - q, b11 = a11 - q, b22 = a22 - q;
  const double k01 = a01 * a01, k02 = a02 * a02, k12 = a12 * a12;
  const double p2 = (b00 * b00 + b11 * b11 + b22 * b22 + 2.0 * (k01 + k02 + k12)) * (1.0 / 6.0);
  if (!(p2 > 0.0)) {                      // multiple of the identity
    *lam = q;
    v0[0] = 1.0; v0[1] = 0.0; v0[2] = 0.0;
    return;
  }
  // ---- fp32 estimate of the isolated root of det(B - x I) = 0, x in units of p ----
  const float pf = sqrt_est_((float)p2);
  const float f00 = (float)b00, f11 = (float)b11, f22 = (float)b22, f01 = (float)a01, f02 = (float)a02, f12 = (float)a12;
  const float detf = f00 * (f11 * f22 - f12 * f12) - f01 * (f01 * f22 - f12 * f02) + f02 * (f01 * f12 - f11 * f02);
  float half = 0.5f * detf * rcp_est_(pf * pf * pf);
  half = fminf(fmaxf(half, -1.0f), 1.0f);
  const bool iso_is_max = half >= kDeflateHalfUnit;
  // smallest root beta0 = 2 cos(acos(half) / 3 + 2 pi / 3) without the inverse cosine: in s = sqrt(1 - half) it is analytic on
  // [0, sqrt 2] (acos(1 - s^2) = 2 asin(s / sqrt 2), and the end half = -1 is even in its own square root), a degree-7 minimax
  // polynomial is within 5e-8 of it (2.5e-7 evaluated in float32: what the trigonometric form reaches)
  float beta;
  {
    const float sq = sqrt_est_(1.0f - half);
    float pl = -1.993398076e-04f;
    pl = fmaf(pl, sq, 1.522336419e-03f); pl = fmaf(pl, sq, -5.673570384e-03f); pl = fmaf(pl, sq, 1.511769878e-02f);
    pl = fmaf(pl, sq, -3.736451873e-02f); pl = fmaf(pl, sq, 1.110385112e-01f); pl = fmaf(pl, sq, -8.164918407e-01f);
    beta = fmaf(pl, sq, -1.000000052e+00f);
  }
  if (iso_is_max) beta = 2.0f * cos_est_(acosf(half) * (1.0f / 3.0f));          // needles: the largest root starts the deflation
  double l = q + (double)(pf * beta);
  const double pa = a02 * a12, pb = a01 * a12, pc = a01 * a02;        // independent of l
  double d0 = a00 - l, d1 = a11 - l, d2 = a22 - l;
  double M00 = fma(d1, d2, -k12), M11 = fma(d0, d2, -k02), M22 = fma(d0, d1, -k01);
  double M01 = fma(-a01, d2, pa), M02 = fma(-a02, d1, pb), M12;
  {
    // ---- one Newton step in fp64 ----
    const double f = fma(a02, M02, fma(a01, M01, d0 * M00));
    const double s = (M00 + M11) + M22;                                // = -f'(l)
    if (fabs(s) > 1e-200) l = fma(f, rcp_raw_(s), l);
  }
  d0 = a00 - l; d1 = a11 - l; d2 = a22 - l;
  if (half >= kNewton2Half && !iso_is_max) {
    // the middle eigenvalue is close (edge-like neighbourhood): a second step
    M00 = fma(d1, d2, -k12); M11 = fma(d0, d2, -k02); M22 = fma(d0, d1, -k01);
    M01 = fma(-a01, d2, pa); M02 = fma(-a02, d1, pb);
    const double f = fma(a02, M02, fma(a01, M01, d0 * M00));
    const double s = (M00 + M11) + M22;
    if (fabs(s) > 1e-200) l = fma(f, rcp_raw_(s), l);
    d0 = a00 - l; d1 = a11 - l; d2 = a22 - l;
  }
  M00 = fma(d1, d2, -k12); M11 = fma(d0, d2, -k02); M22 = fma(d0, d1, -k01);
  M01 = fma(-a01, d2, pa); M02 = fma(-a02, d1, pb); M12 = fma(-a12, d0, pc);
  const bool s0 = M00 >= M11 && M00 >= M22;
  const bool s1 = !s0 && M11 >= M22;
  double iso[3];
  iso[0] = s0 ? M00 : (s1 ? M01 : M02);
  iso[1] = s0 ? M01 : (s1 ? M11 : M12);
  iso[2] = s0 ? M02 : (s1 ? M12 : M22);
  const double n2 = iso[0] * iso[0] + iso[1] * iso[1] + iso[2] * iso[2];
  if (n2 > 0.0) {
    const double inv = rsqrt1_(n2);
    iso[0] *= inv; iso[1] *= inv; iso[2] *= inv;
  } else {
    iso[0] = 1.0; iso[1] = 0.0; iso[2] = 0.0;
  }
  double l_iso = l;
  if (RAYLEIGH || iso_is_max) {
    // Rayleigh quotient as a correction of l: l + v . (A - l I) v
    const double w0 = d0 * iso[0] + a01 * iso[1] + a02 * iso[2];
    const double w1 = a01 * iso[0] + d1 * iso[1] + a12 * iso[2];
    const double w2 = a02 * iso[0] + a12 * iso[1] + d2 * iso[2];
    l_iso = l + (iso[0] * w0 + iso[1] * w1 + iso[2] * w2);
  }
  if (!iso_is_max) {
    *lam = l_iso;
    v0[0] = iso[0]; v0[1] = iso[1]; v0[2] = iso[2];
    return;
  }
  // nearly prolate spectrum: smallest eigenpair of the 2x2 problem in the complement of the (largest) isolated eigenvector
  double u[3], w[3];
  if (fabs(iso[0]) > fabs(iso[1])) {
    const double inv = rsqrt_(iso[0] * iso[0] + iso[2] * iso[2]);
    u[0] = -iso[2] * inv; u[1] = 0.0; u[2] = iso[0] * inv;
  } else {
    const double inv = rsqrt_(iso[1] * iso[1] + iso[2] * iso[2]);
    u[0] = 0.0; u[1] = iso[2] * inv; u[2] = -iso[1] * inv;
  }
  cross3(iso, u, w);
  const double au0 = a00 * u[0] + a01 * u[1] + a02 * u[2];
  const double au1 = a01 * u[0] + a11 * u[1] + a12 * u[2];
  const double au2 = a02 * u[0] + a12 * u[1] + a22 * u[2];
  const double aw0 = a00 * w[0] + a01 * w[1] + a02 * w[2];
  const double aw1 = a01 * w[0] + a11 * w[1] + a12 * w[2];
  const double aw2 = a02 * w[0] + a12 * w[1] + a22 * w[2];
  const double m00 = u[0] * au0 + u[1] * au1 + u[2] * au2;
  const double m01 = u[0] * aw0 + u[1] * aw1 + u[2] * aw2;
  const double m11 = w[0] * aw0 + w[1] * aw1 + w[2] * aw2;
  const double h = (m00 - m11) * 0.5, mean = (m00 + m11) * 0.5;
  const double rad = sqrt(h * h + m01 * m01);
  const double l_lo = mean - rad;
  const double x1 = m01, y1 = l_lo - m00, x2 = l_lo - m11, y2 = m01;
  const double n1 = x1 * x1 + y1 * y1, nn2 = x2 * x2 + y2 * y2;
  double x = n1 >= nn2 ? x1 : x2, y = n1 >= nn2 ? y1 : y2;
  const double n = n1 >= nn2 ? n1 : nn2;
  if (n > 0.0) { const double inv = rsqrt_(n); x *= inv; y *= inv; } else { x = 0.0; y = 1.0; }
  v0[0] = x * u[0] + y * w[0]; v0[1] = x * u[1] + y * w[1]; v0[2] = x * u[2] + y * w[2];
  *lam = l_lo;
}

// The full decomposition at the cost of the hot path's solver (round 4; what features_fwd_tile_kernel calls).  eig3_sym above
// spends ~700 instructions per matrix, two thirds of them in fp64 acos / cos, IEEE divisions and square roots.  Same scheme --
// isolate the eigenvalue on the side of the sign of det(B), deflate, solve the exact 2x2 problem in the complement -- built
// from the pieces of eig3_smallest_unit: exact power-of-two scaling (frexp / ldexp: no reciprocal, no rounding), the root
// estimate in float32 on B / p (the degree-7 polynomial in sqrt(1 - |half|): the isolated root always sits on the
// well-conditioned side, and the largest root of B is minus the smallest root of -B), one fp64 Halley step on det(A - l I)
// from the adjugate, the adjugate's best column as eigenvector, a Rayleigh correction, v_rsq_f64 + Newton steps for every
// normalisation (two where the factor's error would reach an eigenvalue, one for the last pair's coordinates).  ~280 instructions;
// pinned against LAPACK by the same host families as eig3_sym (tests/test_hostcheck.py) and, on the device, against an exact
// reference by tests/test_gpu_eig_spectra.py.
DC_HD void eig3_sym_v2(double a00, double a01, double a02, double a11, double a12, double a22, double* lam, double (*V)[3]) {
  double m = fmax(fmax(fabs(a00), fabs(a11)), fabs(a22));
  m = fmax(m, fmax(fabs(a01), fmax(fabs(a02), fabs(a12))));
  if (!(m > 0.0) || !(m < (double)INFINITY)) {   // zero matrix, or NaN/inf input
    const double z = (m == 0.0) ? 0.0 : (double)NAN;
    lam[0] = lam[1] = lam[2] = z;
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) V[i][j] = (i == j) ? 1.0 : 0.0;
    return;
  }
  int ex;
  (void)frexp(m, &ex);                           // m = f 2^ex, f in [0.5, 1): the scaling below is exact
  a00 = ldexp(a00, -ex); a01 = ldexp(a01, -ex); a02 = ldexp(a02, -ex);
  a11 = ldexp(a11, -ex); a12 = ldexp(a12, -ex); a22 = ldexp(a22, -ex);
  const double q = ((a00 + a11) + a22) * (1.0 / 3.0);
  const double b00 = a00 - q, b11 = a11 - q, b22 = a22 - q;
  const double k01 = a01 * a01, k02 = a02 * a02, k12 = a12 * a12;
  const double p2 = (b00 * b00 + b11 * b11 + b22 * b22 + 2.0 * (k01 + k02 + k12)) * (1.0 / 6.0);
  if (!(p2 > 0.0)) {                             // multiple of the identity
    lam[0] = lam[1] = lam[2] = ldexp(q, ex);
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) V[i][j] = (i == j) ? 1.0 : 0.0;
    return;
  }
  // ---- float32 estimate of the isolated root of det(B - x I) = 0 on B / p (entries of order one whatever p is) ----
  const double rp = rsq_raw_(p2);
  const float rpf = (float)rp;
  const float f00 = (float)b00 * rpf, f11 = (float)b11 * rpf, f22 = (float)b22 * rpf;
  const float f01 = (float)a01 * rpf, f02 = (float)a02 * rpf, f12 = (float)a12 * rpf;
  const float detf = f00 * (f11 * f22 - f12 * f12) - f01 * (f01 * f22 - f12 * f02) + f02 * (f01 * f12 - f11 * f02);
  float half = fminf(fmaxf(0.5f * detf, -1.0f), 1.0f);
  if (!(half == half)) half = 0.0f;              // (an overflowing p2 / rp pair: any start inside the spectrum will do)
  const bool iso_is_max = half >= 0.0f;          // det(B) >= 0: the largest eigenvalue is the isolated one (gap >= sqrt(3) p)
  float beta;
  {
    const float sq = sqrt_est_(1.0f + fabsf(half));       // smallest root of B for -|half|: in [1, sqrt 2]
    float pl = -1.993398076e-04f;
    pl = fmaf(pl, sq, 1.522336419e-03f); pl = fmaf(pl, sq, -5.673570384e-03f); pl = fmaf(pl, sq, 1.511769878e-02f);
    pl = fmaf(pl, sq, -3.736451873e-02f); pl = fmaf(pl, sq, 1.110385112e-01f); pl = fmaf(pl, sq, -8.164918407e-01f);
    beta = fmaf(pl, sq, -1.000000052e+00f);
    beta = iso_is_max ? -beta : beta;
  }
  double l = fma(p2 * rp, (double)beta, q);      // q + p beta
  const double pa = a02 * a12, pb = a01 * a12, pc = a01 * a02;
  double d0 = a00 - l, d1 = a11 - l, d2 = a22 - l;
  double M00 = fma(d1, d2, -k12), M11 = fma(d0, d2, -k02), M22 = fma(d0, d1, -k01);
  double M01 = fma(-a01, d2, pa), M02 = fma(-a02, d1, pb), M12;
  {
    // ---- one Halley step in fp64 on f(l) = det(A - l I): f' = -(M00 + M11 + M22), f'' = 2 (d0 + d1 + d2).  Cubic
    // convergence from the 2.5e-7 p estimate lands at the rounding level (a Newton step leaves ~1e-13 p, which shows as an
    // eigenvector residual of 1e-14: five instructions more buy LAPACK's accuracy) ----
    const double f = fma(a02, M02, fma(a01, M01, d0 * M00));
    const double s = (M00 + M11) + M22;
    const double den = fma(2.0 * s, s, -f * (2.0 * ((d0 + d1) + d2)));
    if (fabs(den) > 1e-300) l = fma(2.0 * f * s, rcp_raw_(den), l);
  }
  d0 = a00 - l; d1 = a11 - l; d2 = a22 - l;
  M00 = fma(d1, d2, -k12); M11 = fma(d0, d2, -k02); M22 = fma(d0, d1, -k01);
  M01 = fma(-a01, d2, pa); M02 = fma(-a02, d1, pb); M12 = fma(-a12, d0, pc);
  // adj(A - l I) = c v v^T with c > 0 for the smallest and for the largest eigenvalue: the largest diagonal entry names the
  // best conditioned column
  const bool s0 = M00 >= M11 && M00 >= M22;
  const bool s1 = !s0 && M11 >= M22;
  double iso[3];
  iso[0] = s0 ? M00 : (s1 ? M01 : M02);
  iso[1] = s0 ? M01 : (s1 ? M11 : M12);
  iso[2] = s0 ? M02 : (s1 ? M12 : M22);
  const double n2 = iso[0] * iso[0] + iso[1] * iso[1] + iso[2] * iso[2];
  if (n2 > 0.0) {
    const double inv = rsqrt2_(n2);               // (iso, u and w = iso x u carry the 2x2 problem: unit to the last bit, see rsqrt2_)
    iso[0] *= inv; iso[1] *= inv; iso[2] *= inv;
  } else {
    iso[0] = 1.0; iso[1] = 0.0; iso[2] = 0.0;
  }
  // Rayleigh quotient as a correction of l: l + v . (A - l I) v
  double l_iso;
  {
    const double w0 = d0 * iso[0] + a01 * iso[1] + a02 * iso[2];
    const double w1 = a01 * iso[0] + d1 * iso[1] + a12 * iso[2];
    const double w2 = a02 * iso[0] + a12 * iso[1] + d2 * iso[2];
    l_iso = l + (iso[0] * w0 + iso[1] * w1 + iso[2] * w2);
  }
  // orthonormal basis (u, w) of the complement, the exact 2x2 problem there
  double u[3], w[3];
  if (fabs(iso[0]) > fabs(iso[1])) {
    const double inv = rsqrt2_(iso[0] * iso[0] + iso[2] * iso[2]);
    u[0] = -iso[2] * inv; u[1] = 0.0; u[2] = iso[0] * inv;
  } else {
    const double inv = rsqrt2_(iso[1] * iso[1] + iso[2] * iso[2]);
    u[0] = 0.0; u[1] = iso[2] * inv; u[2] = -iso[1] * inv;
  }
  cross3(iso, u, w);
  const double au0 = a00 * u[0] + a01 * u[1] + a02 * u[2];
  const double au1 = a01 * u[0] + a11 * u[1] + a12 * u[2];
  const double au2 = a02 * u[0] + a12 * u[1] + a22 * u[2];
  const double aw0 = a00 * w[0] + a01 * w[1] + a02 * w[2];
  const double aw1 = a01 * w[0] + a11 * w[1] + a12 * w[2];
  const double aw2 = a02 * w[0] + a12 * w[1] + a22 * w[2];
  const double m00 = u[0] * au0 + u[1] * au1 + u[2] * au2;
  const double m01 = u[0] * aw0 + u[1] * aw1 + u[2] * aw2;
  const double m11 = w[0] * aw0 + w[1] * aw1 + w[2] * aw2;
  const double h = (m00 - m11) * 0.5, mean = (m00 + m11) * 0.5;
  const double r2 = h * h + m01 * m01;
  const double rad = r2 > 0.0 ? r2 * rsqrt2_(r2) : 0.0;
  double l_hi = mean + rad, l_lo = mean - rad;
  double ca, cb;
  {
    // eigenvector of l_hi in (u, w) coordinates: the better conditioned of the two row null vectors
    const double x1 = m01, y1 = l_hi - m00, x2 = l_hi - m11, y2 = m01;
    const double n1 = x1 * x1 + y1 * y1, nn2 = x2 * x2 + y2 * y2;
    const double x = n1 >= nn2 ? x1 : x2, y = n1 >= nn2 ? y1 : y2, n = n1 >= nn2 ? n1 : nn2;
    if (n > 0.0) { const double inv = rsqrt1_(n); ca = x * inv; cb = y * inv; } else { ca = 1.0; cb = 0.0; }
  }
  const double vhi[3] = {ca * u[0] + cb * w[0], ca * u[1] + cb * w[1], ca * u[2] + cb * w[2]};
  const double vlo[3] = {ca * w[0] - cb * u[0], ca * w[1] - cb * u[1], ca * w[2] - cb * u[2]};
  // ascending order: the pair is ordered by construction; the isolated eigenvalue can only cross it by round-off
  // (spectra isotropic to machine precision), where moving it onto its neighbour changes nothing that can be resolved
  if (iso_is_max) {
    l_iso = fmax(l_iso, l_hi);
    lam[0] = ldexp(l_lo, ex); lam[1] = ldexp(l_hi, ex); lam[2] = ldexp(l_iso, ex);
    for (int j = 0; j < 3; ++j) { V[0][j] = vlo[j]; V[1][j] = vhi[j]; V[2][j] = iso[j]; }
  } else {
    l_iso = fmin(l_iso, l_lo);
    lam[0] = ldexp(l_iso, ex); lam[1] = ldexp(l_lo, ex); lam[2] = ldexp(l_hi, ex);
    for (int j = 0; j < 3; ++j) { V[0][j] = iso[j]; V[1][j] = vlo[j]; V[2][j] = vhi[j]; }
  }
}

// Smallest eigenpair and trace of any symmetric positive semi-definite matrix through the core above (one reciprocal of
// the trace, one Newton step on it).
DC_HD void eig3_smallest_v2(double a00, double a01, double a02, double a11, double a12, double a22, double* lam0,
                            double* v0, double* tr_out) {
  const double m = a00 + a11 + a22;
  *tr_out = m;
  if (!(m > 0.0) || !(m < (double)INFINITY)) {
    const bool zero = (m == 0.0) && a01 == 0.0 && a02 == 0.0 && a12 == 0.0;
    *lam0 = zero ? 0.0 : (double)NAN;
    v0[0] = 1.0; v0[1] = 0.0; v0[2] = 0.0;
    return;
  }
  const double inv_m = recip1_(m);
  double lr;
  eig3_smallest_unit<true>(a00 * inv_m, a01 * inv_m, a02 * inv_m, a11 * inv_m, a12 * inv_m, a22 * inv_m, &lr, v0);
  *lam0 = lr * m;
}

// Hot-path variant: only the smallest eigenpair (lam0, v0) and the trace, which is all the min-eigenvalue /
// trace losses and their backward consume.  Same isolate-then-deflate scheme as eig3_sym; the isolated
// eigenvalue starts from an fp32 trigonometric estimate (native acos / cos, ~1e-6 relative to the spread)
// and is polished by one fp64 Newton step on the characteristic polynomial (isolated root: quadratic
// convergence to ~1e-12), then by the Rayleigh quotient of its fp64 eigenvector.  Roughly half the fp64
// instructions of the full solver; accuracy identical (checked against LAPACK in tests/test_hostcheck.py).
DC_HD void eig3_smallest_r2(double a00, double a01, double a02, double a11, double a12, double a22, double* lam0,
                            double* v0, double* tr_out) {
  // covariance matrices are positive semi-definite: the trace bounds every entry, one add instead of a max tree
  const double m = a00 + a11 + a22;
  *tr_out = m;
  if (!(m > 0.0) || !(m < (double)INFINITY)) {
    const bool zero = (m == 0.0) && a01 == 0.0 && a02 == 0.0 && a12 == 0.0;
    *lam0 = zero ? 0.0 : (double)NAN;
    v0[0] = 1.0; v0[1] = 0.0; v0[2] = 0.0;
    return;
  }
  const double inv_m = recip_(m);       // 0 < m < inf
  a00 *= inv_m; a01 *= inv_m; a02 *= inv_m; a11 *= inv_m; a12 *= inv_m; a22 *= inv_m;
  const double q = 1.0 / 3.0;             // trace of the scaled matrix is 1
  const double b00 = a00 - q, b11 = a11 - q, b22 = a22 - q;
  const double off = a01 * a01 + a02 * a02 + a12 * a12;
  const double p2 = (b00 * b00 + b11 * b11 + b22 * b22 + 2.0 * off) * (1.0 / 6.0);
  if (!(p2 > 0.0)) {                      // multiple of the identity
    *lam0 = q * m;
    v0[0] = 1.0; v0[1] = 0.0; v0[2] = 0.0;
    return;
  }
  // ---- fp32 estimate of the isolated root of det(B - x I) = 0, x in units of p ----
  const float pf = sqrt_est_((float)p2);
  const float f00 = (float)b00, f11 = (float)b11, f22 = (float)b22, f01 = (float)a01, f02 = (float)a02, f12 = (float)a12;
  const float detf = f00 * (f11 * f22 - f12 * f12) - f01 * (f01 * f22 - f12 * f02) + f02 * (f01 * f12 - f11 * f02);
  float half = 0.5f * detf * rcp_est_(pf * pf * pf);
  half = fminf(fmaxf(half, -1.0f), 1.0f);
  const bool iso_is_max = half >= kDeflateHalf;
  const float ang = acosf(half) * (1.0f / 3.0f);
  const float beta = 2.0f * cos_est_(iso_is_max ? ang : ang + 2.0943951f);
  double l = q + (double)(pf * beta);
  // ---- one Newton step on f(l) = det(A - l I) in fp64 ----
  {
    const double d0 = a00 - l, d1 = a11 - l, d2 = a22 - l;
    const double m0 = d1 * d2 - a12 * a12, m1 = d0 * d2 - a02 * a02, m2 = d0 * d1 - a01 * a01;
    const double f = d0 * m0 - a01 * (a01 * d2 - a12 * a02) + a02 * (a01 * a12 - d1 * a02);
    const double fp = -(m0 + m1 + m2);
    if (fabs(fp) > 1e-200) l -= f * recip_(fp);
  }
  double iso[3];
  eigvec_isolated(a00, a01, a02, a11, a12, a22, l, iso);
  const double ai0 = a00 * iso[0] + a01 * iso[1] + a02 * iso[2];
  const double ai1 = a01 * iso[0] + a11 * iso[1] + a12 * iso[2];
  const double ai2 = a02 * iso[0] + a12 * iso[1] + a22 * iso[2];
  const double l_iso = iso[0] * ai0 + iso[1] * ai1 + iso[2] * ai2;
  if (!iso_is_max) {
    *lam0 = l_iso * m;
    v0[0] = iso[0]; v0[1] = iso[1]; v0[2] = iso[2];
    return;
  }
  // smallest eigenpair of the 2x2 problem in the complement of the (largest) isolated eigenvector
  double u[3], w[3];
  if (fabs(iso[0]) > fabs(iso[1])) {
    const double inv = rsqrt_(iso[0] * iso[0] + iso[2] * iso[2]);
    u[0] = -iso[2] * inv; u[1] = 0.0; u[2] = iso[0] * inv;
  } else {
    const double inv = rsqrt_(iso[1] * iso[1] + iso[2] * iso[2]);
    u[0] = 0.0; u[1] = iso[2] * inv; u[2] = -iso[1] * inv;
  }
  cross3(iso, u, w);
  const double au0 = a00 * u[0] + a01 * u[1] + a02 * u[2];
  const double au1 = a01 * u[0] + a11 * u[1] + a12 * u[2];
  const double au2 = a02 * u[0] + a12 * u[1] + a22 * u[2];
  const double aw0 = a00 * w[0] + a01 * w[1] + a02 * w[2];
  const double aw1 = a01 * w[0] + a11 * w[1] + a12 * w[2];
  const double aw2 = a02 * w[0] + a12 * w[1] + a22 * w[2];
  const double m00 = u[0] * au0 + u[1] * au1 + u[2] * au2;
  const double m01 = u[0] * aw0 + u[1] * aw1 + u[2] * aw2;
  const double m11 = w[0] * aw0 + w[1] * aw1 + w[2] * aw2;
  const double h = (m00 - m11) * 0.5, mean = (m00 + m11) * 0.5;
  const double rad = sqrt(h * h + m01 * m01);
  const double l_lo = mean - rad;
  // eigenvector of l_lo in (u, w) coordinates
  const double x1 = m01, y1 = l_lo - m00, x2 = l_lo - m11, y2 = m01;
  const double n1 = x1 * x1 + y1 * y1, n2 = x2 * x2 + y2 * y2;
  double x = n1 >= n2 ? x1 : x2, y = n1 >= n2 ? y1 : y2;
  const double n = n1 >= n2 ? n1 : n2;
  if (n > 0.0) { const double inv = rsqrt_(n); x *= inv; y *= inv; } else { x = 0.0; y = 1.0; }
  v0[0] = x * u[0] + y * w[0]; v0[1] = x * u[1] + y * w[1]; v0[2] = x * u[2] + y * w[2];
  *lam0 = l_lo * m;
}

}  // namespace dc

namespace dc {
// What the kernels call: the round-3 solver (eig3_smallest_v2: trace-1 core, adjugate eigenvector, polynomial root estimate);
// eig3_smallest_r2 above is round 2's, kept for the A-B baseline form of the step kernel and pinned by the same host checks.
DC_HD void eig3_smallest(double a00, double a01, double a02, double a11, double a12, double a22, double* lam0, double* v0,
                         double* tr_out) {
  eig3_smallest_v2(a00, a01, a02, a11, a12, a22, lam0, v0, tr_out);
}
}  // namespace dc
