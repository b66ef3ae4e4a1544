// De-skew of moving-sweep scans (gfx950): every point of every scan goes from the sensor frame at its own sweep time tau into the
// frame at sweep time 0 of its scan, x' = D(tau) x (dc_sweepmath.h: the arithmetic dc_sweep_rays and dc_raycast_sweep render with).
// C ABI at the bottom (include/dc_hip.h); DESIGN "Moving-sweep rendering and de-skew".
//
// One lane per point, one launch for every scan: the scan is found by dc::scan_of (dc_bvh.h), the clamped bisection of dc_raycast_rays
// (the index stays in [0, n_scans), so offsets that do not span [0, n] cannot move a read outside twists).  A lane reads everything it needs before it
// writes, and no lane touches another's rows, so the outputs may be the inputs (DC_F64); the pointers are not __restrict__ for that.
#include "dc_common.h"
#include "dc_bvh.h"
#include "dc_sweepmath.h"
#include "dc_hostutil.h"
#include "../../include/dc_hip.h"

namespace {

constexpr int kSweepBlock = 256;

template <typename T>
__global__ void __launch_bounds__(kSweepBlock) deskew_kernel(const T* points, const T* vps, const T* normals, const double* __restrict__ tau,
                                                             int64_t total, const int64_t* __restrict__ scan_offset,
                                                             const double* __restrict__ twists, int n_scans, double* points_out,
                                                             double* vps_out, double* normals_out) {
  const int64_t g = (int64_t)blockIdx.x * kSweepBlock + threadIdx.x;
  if (g >= total) return;
  const double* tw = twists + 6 * (int64_t)dc::scan_of(scan_offset, n_scans, g);
  const double tg = tau[g];
  const double t0 = tw[0], t1 = tw[1], t2 = tw[2];
  const dc::SweepRot r = dc::sweep_rot(tg, tw[3], tw[4], tw[5]);
  double x[3], v[3] = {0.0, 0.0, 0.0}, m[3] = {0.0, 0.0, 0.0};
  dc::sweep_point(r, tg, t0, t1, t2, (double)points[3 * g], (double)points[3 * g + 1], (double)points[3 * g + 2], x);
  if (vps) dc::sweep_point(r, tg, t0, t1, t2, (double)vps[3 * g], (double)vps[3 * g + 1], (double)vps[3 * g + 2], v);
  if (normals) dc::sweep_rotate(r, (double)normals[3 * g], (double)normals[3 * g + 1], (double)normals[3 * g + 2], m);
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    points_out[3 * g + a] = x[a];
    if (vps) vps_out[3 * g + a] = v[a];
    if (normals) normals_out[3 * g + a] = m[a];
  }
}

}  // namespace

extern "C" {

int dc_deskew(const void* points, const void* vps, const void* normals, int dtype, const double* tau, int64_t n, const int64_t* scan_offset,
              const double* twists, int n_scans, double* points_out, double* vps_out, double* normals_out, dcStream_t stream) {
  if (n < 0 || n_scans < 0) return DC_ERR_ARG;
  if (dtype != DC_F32 && dtype != DC_F64) return DC_ERR_DTYPE;
  if (n == 0) return DC_OK;
  if (n_scans < 1 || !points || !tau || !scan_offset || !twists || !points_out || (vps != nullptr) != (vps_out != nullptr) ||
      (normals != nullptr) != (normals_out != nullptr))
    return DC_ERR_ARG;
  const unsigned grid = (unsigned)((n + kSweepBlock - 1) / kSweepBlock);
  if (dtype == DC_F32)
    deskew_kernel<float><<<grid, kSweepBlock, 0, (hipStream_t)stream>>>((const float*)points, (const float*)vps, (const float*)normals, tau, n,
                                                                      scan_offset, twists, n_scans, points_out, vps_out, normals_out);
  else
    deskew_kernel<double><<<grid, kSweepBlock, 0, (hipStream_t)stream>>>((const double*)points, (const double*)vps, (const double*)normals, tau,
                                                                       n, scan_offset, twists, n_scans, points_out, vps_out, normals_out);
  DC_HIP(hipGetLastError());
  return DC_OK;
}

}  // extern "C"
