// Per-point term of the supervised mesh loss (dc_meshloss.hip), host and device: for a corrected point x and the closest point c of
// the mesh, the residual r = |x - c|, the term l = r (or r^2 with `squared`) and its gradient dl/dx.  c minimises the distance, so
// dr/dx = (x - c) / r: the closest point's own motion does not enter (envelope theorem).  r = 0 has no direction: the gradient is
// zero there (squared or not).  fp64 with contraction switched off: r is formed from x - c by the operations closest_on_triangle
// ends with (dc_trimath.h), so sqrt of the walk's best d^2 and this r are the same bits, on the host build as on the device.
#pragma once
#include "dc_common.h"
#include <math.h>

namespace dc {

// x [3], c [3] -> *r = |x - c|, grad [3] = dl/dx; returns l
DC_HD double mesh_loss_term(const double* x, const double* c, bool squared, double* r, double* grad) {
#pragma clang fp contract(off)
  const double e0 = x[0] - c[0], e1 = x[1] - c[1], e2 = x[2] - c[2];
  const double d2 = (e0 * e0 + e1 * e1) + e2 * e2;
  const double d = sqrt(d2);                       // correctly rounded on the host and on gfx950
  *r = d;
  if (squared) {
    grad[0] = 2.0 * e0; grad[1] = 2.0 * e1; grad[2] = 2.0 * e2;
    return d2;
  }
  if (d > 0.0) {
    grad[0] = e0 / d; grad[1] = e1 / d; grad[2] = e2 / d;
  } else {
    grad[0] = grad[1] = grad[2] = d != d ? d : 0.0;   // r = 0: no direction; a NaN stays visible
  }
  return d;
}

}  // namespace dc
