// Range-image arithmetic shared by the kernels of dc_rangeimage.hip and the host build (csrc/dc_hostcheck.cpp):
//   * the pixel of a sensor-frame point on a spherical H x W grid -- the reference's range_projection
//     (scripts/depth_denoising:44-91; compare_to_ddd uses the same), restated in fp64 in its operation order;
//   * the slots of an image window around a pixel (rows clip, columns wrap or clip);
//   * the membership predicate of a window slot (occupied + 3-D radius gate);
//   * the order-preserving key of a depth for the nearest-point-wins rule.
// Every product and sum is rounded on its own (no contraction): the host build and the device give the same bits wherever
// their atan2 / asin agree, and tests/rangeimage_reference.py restates the same expression tree in numpy.
#pragma once
#include <math.h>
#include "dc_common.h"

namespace dc {

struct RangeGrid {
  int rows, cols;            // H, W
  double fov_up, fov_down;   // degrees, as the reference's proj_fov_up / proj_fov_down (fov_down usually negative)
  int wrap;                  // columns span the full turn: != 0 a window wraps over the seam, 0 it clips.  Rows never wrap.
};

DC_HD bool range_grid_ok(const RangeGrid& g) {
  const double fov = fabs(g.fov_down) + fabs(g.fov_up);
  return g.rows >= 1 && g.cols >= 1 && (int64_t)g.rows * g.cols <= (int64_t)0x7fffffff && fov > 0.0 && fov < INFINITY;
}

// |p| as numpy's norm over the last axis of an [n,3] array sums it: (x x + y y) + z z, one rounding per operation
DC_HD double range_depth(double x, double y, double z) {
#if defined(__HIPCC__)
#pragma clang fp contract(off)
#endif
  const double xx = x * x, yy = y * y, zz = z * z;
  const double s = xx + yy;
  return sqrt(s + zz);
}

// Pixel r * W + c of the sensor-frame point (x, y, z), or -1 when it is rejected: a NaN or an infinity among the coordinates,
// a depth that is not > min_depth (so zero depth never projects), or -- with clamp == 0 -- a row outside the image (the point
// is outside the vertical field of view; the columns span the full turn, so a column is always clamped: yaw = +pi lands on
// column W and is brought back to W - 1 as the reference does).  *depth_out receives |p| whenever it is given.
DC_HD int32_t range_pixel(const RangeGrid& g, double x, double y, double z, int clamp, double min_depth, double* depth_out) {
#if defined(__HIPCC__)
#pragma clang fp contract(off)
#endif
  const double kPi = 3.141592653589793;
  const double depth = range_depth(x, y, z);
  if (depth_out) *depth_out = depth;
  if (!(fabs(x) < INFINITY && fabs(y) < INFINITY && fabs(z) < INFINITY)) return -1;
  if (!(depth > min_depth) || !(depth < INFINITY)) return -1;
  const double fov_up = g.fov_up / 180.0 * kPi, fov_down = g.fov_down / 180.0 * kPi;
  const double fov = fabs(fov_down) + fabs(fov_up);
  const double yaw = -atan2(y, x);
  const double pitch = asin(z / (depth + 1e-8));
  double px = 0.5 * (yaw / kPi + 1.0);
  double py = 1.0 - (pitch + fabs(fov_down)) / fov;
  px *= (double)g.cols;
  py *= (double)g.rows;
  px = floor(px);
  py = floor(py);
  if (!clamp && (py < 0.0 || py > (double)(g.rows - 1))) return -1;
  px = px < (double)(g.cols - 1) ? px : (double)(g.cols - 1);
  px = px > 0.0 ? px : 0.0;
  py = py < (double)(g.rows - 1) ? py : (double)(g.rows - 1);
  py = py > 0.0 ? py : 0.0;
  return (int32_t)py * g.cols + (int32_t)px;
}

// A window of half extents (ah, aw) fits the grid when no pixel can appear in it twice and it has at most 121 slots.
DC_HD bool image_window_ok(const RangeGrid& g, int ah, int aw) {
  if (ah < 0 || aw < 0 || ah > DC_IMAGE_MAX_WINDOW || aw > DC_IMAGE_MAX_WINDOW) return false;
  return 2 * ah + 1 <= g.rows && 2 * aw + 1 <= g.cols && (2 * ah + 1) * (2 * aw + 1) <= DC_IMAGE_MAX_WINDOW;
}

// Pixel of the window slot (dr, dc) of the centre pixel (r, c), or -1 outside the image.
DC_HD int32_t image_window_pixel(const RangeGrid& g, int r, int c, int dr, int dc) {
  const int rr = r + dr;
  int cc = c + dc;
  if (rr < 0 || rr >= g.rows) return -1;
  if (cc < 0 || cc >= g.cols) {
    if (!g.wrap) return -1;
    cc = cc < 0 ? cc + g.cols : cc - g.cols;     // |dc| <= aw < W: one turn is enough
  }
  return rr * g.cols + cc;
}

// the gate of a window: r <= 0, an infinity or a NaN means none
DC_HD bool image_gate_on(double r) { return r > 0.0 && r < INFINITY; }

// |xj - xi|^2 <= r^2, each product and sum rounded on its own, in axis order
DC_HD bool image_within(const double* xi, const double* xj, double r) {
#if defined(__HIPCC__)
#pragma clang fp contract(off)
#endif
  const double d0 = xj[0] - xi[0], d1 = xj[1] - xi[1], d2 = xj[2] - xi[2];
  const double p0 = d0 * d0, p1 = d1 * d1, p2 = d2 * d2;
  const double s = (p0 + p1) + p2;
  return s <= r * r;
}

// Slot membership: the slot's pixel is occupied and its point passes the gate; the centre is always a member.
DC_HD bool image_member(bool occupied, bool centre, const double* xi, const double* xj, double r) {
  if (!occupied) return false;
  if (centre || !image_gate_on(r)) return true;
  return image_within(xi, xj, r);
}

// Depths that project are positive and finite: their bit patterns order as they do.
DC_HD uint64_t range_depth_key(double depth) {
  union { double d; uint64_t u; } v;
  v.d = depth;
  return v.u;
}
DC_HD double range_key_depth(uint64_t key) {
  union { double d; uint64_t u; } v;
  v.u = key;
  return v.d;
}
#define DC_RANGE_EMPTY_KEY 0xffffffffffffffffull

}  // namespace dc
