// Per-point arithmetic of the moving-sweep model (dc_raycast.hip: dc_sweep_rays, dc_raycast_sweep; dc_sweep.hip: dc_deskew; compiled
// for the host by dc_hostcheck.cpp, so that the CPU tests pin it).  Definitions: include/dc_hip.h, DESIGN "Moving-sweep rendering and
// de-skew".
//
// A scan has a twist (v, w) over the whole sweep, expressed in the frame at sweep time 0.  At sweep time tau the sensor stands at
//   D(tau) = [Exp(tau w) | tau v]
// in that frame: rotation and translation interpolated separately (not the SE(3) exponential).  With a = tau w, th = |a|, h = th / 2:
//   D(tau) x = ((x + A (a x x)) + B (a x (a x x))) + tau v,   A = sin th / th = (sin h / h) cos h,   B = (sin h / h)^2 / 2,
//   th < 2^-26:  A = 1, B = 1/2  (their error there, th^2 / 6, is below 2^-54).
// B is not (1 - cos th) / th^2, which cancels for small th.  One sincos, at h, serves both.  Directions and normals take the
// rotation only.  tau is any double: negative values are times before the reference, and a tau that is not finite gives NaN.
// tau = 0 and w = v = 0 return x itself (a = 0: every added term is a zero).  |w| <= pi is the caller's duty.
//
// No fused multiply-adds in this header: dc_sweep_rays, dc_raycast_sweep and dc_deskew inline the same functions into different
// kernels and must form bit-identical rays, and a contraction the compiler chooses per call site would break that.
//
// Error of a component of D(tau) x against the exact value for the same doubles, for th <= pi, in units of u = 2^-52 (so a
// correctly rounded product, sum, quotient or root contributes at most 1/2 relative; sincos at most 2, the device library's bound),
// every error taken with the same sign.  Worst case th = pi, h = pi / 2:
//   a = tau w: 1/2 per component; th = sqrt(a . a): (1/2 + 1/2 + 1/2) * 2 for a square, + 1/2 + 1/2 for the sums, halved by the
//     root, + 1/2:                                                                                 |dth| <= 1.75 th
//   q = sin h / h: the argument moves it by |h cot h - 1| * 1.75 (1.75 at pi / 2), sincos 2, the quotient 1/2:       4.25 relative
//   B = q q / 2 = 0.2026: 2 * 4.25 + 1/2 = 9 relative, 1.83 absolute; A = q cos h: cos h moves by sin h * h * 1.75 + 2 cos h = 2.75
//     absolute, times q = 0.637: 1.75 absolute (A itself is 0 there)
//   c = a x x: per component (1/2 + 1/2) (|a_j x_k| + |a_k x_j|) + 1/2 |c_i| <= 1.5 th |x|
//   e = a x c: sqrt 2 * 1.5 th^2 |x| from c, + 1 th^2 |x| + 1/2 th^2 |x| like c:                    <= 3.63 th^2 |x|
//   A c:  1.75 * pi |x|                                                                                              =  5.5 |x|
//   B e:  1.83 * pi^2 |x| + 0.2026 * 3.63 pi^2 |x| + 1/2 * 0.2026 pi^2 |x|                                           = 26.3 |x|
//   the two sums of the rotation 1/2 |x| each, the product tau v 1/2 |tau v|, the last sum 1/2 (|x| + |tau v|):        1.5 |x| + |tau v|
// together below 33.3 |x| + |tau v| at th = pi; at th = 2.5 the same count gives 31, at pi / 2 21.  The tests hold every component
// to 34 u (|x| + |tau v|).
#pragma once
#include <math.h>
#include "dc_common.h"

namespace dc {

// Scalars only: a runtime-indexed private array would live in scratch memory on the device.
struct SweepRot {
  double a0, a1, a2;              // a = tau w
  double A, B;
};

DC_HD SweepRot sweep_rot(double tau, double w0, double w1, double w2) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  SweepRot r;
  r.a0 = tau * w0;
  r.a1 = tau * w1;
  r.a2 = tau * w2;
  const double th = sqrt(r.a0 * r.a0 + r.a1 * r.a1 + r.a2 * r.a2);
  if (th < 0x1p-26) {
    r.A = 1.0;
    r.B = 0.5;
  } else {                        // NaN comes here and stays NaN
    const double h = 0.5 * th;
    double s, c;
    sincos(h, &s, &c);
    const double q = s / h;
    r.A = q * c;
    r.B = 0.5 * (q * q);
  }
  return r;
}

// y = Exp(a) x
DC_HD void sweep_rotate(const SweepRot& r, double x0, double x1, double x2, double* y) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double c0 = r.a1 * x2 - r.a2 * x1, c1 = r.a2 * x0 - r.a0 * x2, c2 = r.a0 * x1 - r.a1 * x0;
  const double e0 = r.a1 * c2 - r.a2 * c1, e1 = r.a2 * c0 - r.a0 * c2, e2 = r.a0 * c1 - r.a1 * c0;
  y[0] = (x0 + r.A * c0) + r.B * e0;
  y[1] = (x1 + r.A * c1) + r.B * e1;
  y[2] = (x2 + r.A * c2) + r.B * e2;
}

// y = D(tau) x = Exp(a) x + tau v
DC_HD void sweep_point(const SweepRot& r, double tau, double v0, double v1, double v2, double x0, double x1, double x2, double* y) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  sweep_rotate(r, x0, x1, x2, y);
  y[0] = y[0] + tau * v0;
  y[1] = y[1] + tau * v1;
  y[2] = y[2] + tau * v2;
}

// The left Jacobian of SO(3) at a = tau w (dc_icp_ct_accumulate: the derivative of Exp(tau w) x by w; DESIGN "Sweep-aware
// registration"):  Exp(a + da) = Exp(J_l(a) da) Exp(a) to first order,
//   J_l(a) = I + C1 [a]x + C2 [a]x^2,   C1 = (1 - cos th) / th^2 = (sin h / h)^2 / 2 = B of sweep_rot (no cancellation),
//   C2 = (th - sin th) / th^3.
// th - sin th cancels for small th (its rounding error is about u th against th^3 / 6), so below th = 1 C2 is its series
//   1/6 - x/120 + x^2/5040 - ... + x^8 / 19!,  x = th^2,
// nine terms in Horner's form: the first one left out, x^9 / 21!, is below 2e-20 at th = 1, a thousandth of a rounding of 1/6.  At
// th >= 1 the difference is at least 0.158 and is formed directly.  th < 2^-26: J_l = I + [a]x / 2 (C1 = 1/2, C2 = 0; what is left
// out, th^2 / 6, is below 2^-54).  NaN stays NaN.
//
// Error of an entry of J_l against the exact matrix of the same doubles a, th <= pi, counted as above in units of u = 2^-52:
//   th: the squares 1/2 each and two sums 1/2 each, halved by the root, + 1/2:                                 |dth| <= 1.25 th
//   q = sin h / h: argument |h cot h - 1| * 1.25 <= 1.25, sincos 2, quotient 1/2: 3.75;  C1 = q q / 2: 2 * 3.75 + 1/2 = 8 relative
//   d = th - sin th with the same rounded th on both sides: (1 - cos th) th 1.25 + 2 sin th + d / 2; relative to d this is largest
//     at th = 1: (0.575 + 1.683) / 0.1585 + 1/2 = 14.8;  th^3 = (th th) th: 3 * 1.25 + 1 = 4.75;  quotient 1/2:  C2 <= 20 relative
//     (the series: x carries 3, which moves C2 by less than 1; Horner's roundings add less than 1 1/2: below 3)
//   C1 [a]x: 8 + 1/2 on |C1 a_k| <= th / 2:                                                                           4.25 th
//   [a]x^2 entries a_i a_j (1/2) or -(a_j^2 + a_k^2) (1): with C2 <= 1/6, (20 + 1 + 1/2) th^2 / 6:                     3.6 th^2
//   the two sums: 1/2 (1 + th / 2) + 1/2 (1 + th / 2 + th^2 / 6)
// together below 1 + 4.75 th + 3.7 th^2 (52.5 at th = pi).  The tests hold every entry to that count.
struct SweepJl {
  double C1, C2;
};

DC_HD SweepJl sweep_left_jacobian(const SweepRot& r) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  SweepJl j;
  const double x = r.a0 * r.a0 + r.a1 * r.a1 + r.a2 * r.a2;
  const double th = sqrt(x);
  j.C1 = r.B;
  if (th < 0x1p-26) {
    j.C2 = 0.0;
  } else if (th < 1.0) {
    double s = 1.0 / 121645100408832000.0;                   // 1 / 19!
    s = 1.0 / 355687428096000.0 - x * s;                     // 1 / 17!
    s = 1.0 / 1307674368000.0 - x * s;                       // 1 / 15!
    s = 1.0 / 6227020800.0 - x * s;                          // 1 / 13!
    s = 1.0 / 39916800.0 - x * s;                            // 1 / 11!
    s = 1.0 / 362880.0 - x * s;                              // 1 / 9!
    s = 1.0 / 5040.0 - x * s;                                // 1 / 7!
    s = 1.0 / 120.0 - x * s;                                 // 1 / 5!
    j.C2 = 1.0 / 6.0 - x * s;
  } else {                        // NaN comes here and stays NaN
    j.C2 = (th - sin(th)) / ((th * th) * th);
  }
  return j;
}

// y = J_l(a)^T u = (u - C1 (a x u)) + C2 (a x (a x u))     ([a]x is skew, its square symmetric)
DC_HD void sweep_jl_transposed(const SweepRot& r, const SweepJl& j, double u0, double u1, double u2, double* y) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double c0 = r.a1 * u2 - r.a2 * u1, c1 = r.a2 * u0 - r.a0 * u2, c2 = r.a0 * u1 - r.a1 * u0;
  const double e0 = r.a1 * c2 - r.a2 * c1, e1 = r.a2 * c0 - r.a0 * c2, e2 = r.a0 * c1 - r.a1 * c0;
  y[0] = (u0 - j.C1 * c0) + j.C2 * e0;
  y[1] = (u1 - j.C1 * c1) + j.C2 * e1;
  y[2] = (u2 - j.C1 * c2) + j.C2 * e2;
}

// J = J_l(a), row-major 3 x 3: (I + C1 [a]x) + C2 [a]x^2 entry by entry
DC_HD void sweep_jl_matrix(const SweepRot& r, const SweepJl& j, double* J) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double a0 = r.a0, a1 = r.a1, a2 = r.a2;
  J[0] = 1.0 + j.C2 * -(a1 * a1 + a2 * a2);
  J[1] = -(j.C1 * a2) + j.C2 * (a0 * a1);
  J[2] = j.C1 * a1 + j.C2 * (a0 * a2);
  J[3] = j.C1 * a2 + j.C2 * (a0 * a1);
  J[4] = 1.0 + j.C2 * -(a0 * a0 + a2 * a2);
  J[5] = -(j.C1 * a0) + j.C2 * (a1 * a2);
  J[6] = -(j.C1 * a1) + j.C2 * (a0 * a2);
  J[7] = j.C1 * a0 + j.C2 * (a1 * a2);
  J[8] = 1.0 + j.C2 * -(a0 * a0 + a1 * a1);
}

}  // namespace dc
