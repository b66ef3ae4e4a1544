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

}  // namespace dc
