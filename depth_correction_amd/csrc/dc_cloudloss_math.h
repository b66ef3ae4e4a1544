// Per-point term of the supervised cloud loss (dc_cloudloss.hip), host and device: for a corrected point x, its nearest survey point
// y and that point's unit normal n,
//   plane form:  r = n . (x - y) (signed),  l = |r|  (r^2 with `squared`),  dl/dx = sign(r) n  (2 r n)
//   point form:  r = |x - y|,               l = r    (r^2 with `squared`),  dl/dx = (x - y) / r  (2 (x - y))
// The correspondence is a constant: y and n do not move with x.  l = 0 has no direction: the gradient is zero there (squared or
// not); a NaN stays visible.  fp64 with contraction switched off: every product and sum is rounded on its own, left to right, so
// the host build and the device give the same bits, and the point form's r is sqrt of dc_knn.hip's sqdist of the pair.
#pragma once
#include "dc_common.h"
#include <math.h>

namespace dc {

// x [3], y [3], n [3] (read with `plane` only) -> *r, grad [3] = dl/dx; returns l
DC_HD double cloud_loss_term(const double* x, const double* y, const double* n, bool plane, bool squared, double* r, double* grad) {
#pragma clang fp contract(off)
  const double e0 = x[0] - y[0], e1 = x[1] - y[1], e2 = x[2] - y[2];
  if (plane) {
    const double p = (n[0] * e0 + n[1] * e1) + n[2] * e2;
    *r = p;
    if (squared) {
      const double t = 2.0 * p;
      grad[0] = t * n[0]; grad[1] = t * n[1]; grad[2] = t * n[2];
      return p * p;
    }
    if (p > 0.0) {
      grad[0] = n[0]; grad[1] = n[1]; grad[2] = n[2];
    } else if (p < 0.0) {
      grad[0] = -n[0]; grad[1] = -n[1]; grad[2] = -n[2];
    } else {
      grad[0] = grad[1] = grad[2] = p != p ? p : 0.0;   // r = 0: no direction; a NaN stays visible
    }
    return fabs(p);
  }
  const double d2 = (e0 * e0 + e1 * e1) + e2 * e2;
  const double d = sqrt(d2);                            // correctly rounded on the host and on gfx950
  *r = d;
  if (squared) {
    grad[0] = 2.0 * e0; grad[1] = 2.0 * e1; grad[2] = 2.0 * e2;
    return d2;
  }
  if (d > 0.0) {
    grad[0] = e0 / d; grad[1] = e1 / d; grad[2] = e2 / d;
  } else {
    grad[0] = grad[1] = grad[2] = d != d ? d : 0.0;
  }
  return d;
}

}  // namespace dc
