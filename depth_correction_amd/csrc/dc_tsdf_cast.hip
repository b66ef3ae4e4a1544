// Ray casting the fused volume (gfx950): rays of measured clouds marched through a sparse TSDF volume to the zero crossing of its
// trilinear interpolant, with the field's own normal and the incidence angle at the hit (DESIGN "Ray casting the fused volume"; the
// rule: dc_tsdf_cast_math.h, whose functions the kernel inlines).  C ABI at the bottom; see include/dc_hip.h.
//
// One launch, one lane per ray, 64 lanes per block: the rays are scan-major, so the lanes of a wavefront are neighbouring rays of one
// scan and walk neighbouring voxels, and a block retires as soon as its one wavefront's longest ray ends.  A lane keeps its ray, the
// bracket and one block cache per table (total, own) in registers; the march is tsdf_cast_ray as the host build runs it, so the
// outputs are its bits.  A sample whose base block the table lacks is decided by the look-up alone, and the lane jumps to the
// block's exit (the proof that nothing is skipped wrongly: dc_tsdf_cast_math.h "Skipping").  No atomics, no allocation, no host read,
// no LDS: the same inputs give the same bits whatever ran before.
#include "dc_common.h"
#include "../../include/dc_hip.h"
#include "dc_device.h"
#include "dc_hostutil.h"
#include "dc_bvh.h"
#include "dc_tsdf_cast_math.h"

namespace dc {

constexpr int kTsdfCastBlock = 64;

// the own volumes of all scans as one structure (dc_tsdf_loss.hip): scan s owns keys / slots [ptr[s], ptr[s + 1])
struct TsdfCastOwn {
  const uint64_t* keys;
  const int32_t* slots;
  const int64_t* ptr;
  int64_t n_keys, capacity;
  const int64_t* sum;
  const int32_t* count;
};

struct TsdfCastOut {
  int32_t* face;
  double* t;
  double* inc;
  double* normal;
  double* phi;
  uint8_t* status;
  int32_t* samples;
};

template <typename T>
__global__ __launch_bounds__(kTsdfCastBlock) void tsdf_cast_kernel(TsdfTable total, const int64_t* __restrict__ n_blocks, TsdfCastOwn own,
                                                                   TsdfGrid grid, TsdfCastRule rule, const T* __restrict__ vps,
                                                                   const T* __restrict__ dirs, const uint8_t* __restrict__ mask, int64_t n,
                                                                   const int64_t* __restrict__ scan_offset,
                                                                   const double* __restrict__ poses, int n_scans, TsdfCastOut out) {
  const int64_t g = (int64_t)blockIdx.x * kTsdfCastBlock + threadIdx.x;
  if (g >= n) return;
  // the tables, clamped to what the caller allocated
  const int64_t nb0 = *n_blocks;
  total.nb = nb0 < 0 ? 0 : (nb0 > total.capacity ? total.capacity : nb0);
  const int scan = scan_of(scan_offset, n_scans, g);
  TsdfTable mine{nullptr, nullptr, 0, own.capacity, own.sum, own.count};
  if (own.keys) {
    int64_t a = own.ptr[scan], b = own.ptr[scan + 1];
    a = a < 0 ? 0 : (a > own.n_keys ? own.n_keys : a);
    b = b < a ? a : (b > own.n_keys ? own.n_keys : b);
    mine.keys = own.keys + a;
    mine.slots = own.slots + a;
    mine.nb = b - a;
  }
  const double vp[3] = {(double)vps[3 * g], (double)vps[3 * g + 1], (double)vps[3 * g + 2]};
  const double dir[3] = {(double)dirs[3 * g], (double)dirs[3 * g + 1], (double)dirs[3 * g + 2]};
  double M[12];
#pragma unroll
  for (int q = 0; q < 12; ++q) M[q] = poses[16 * (int64_t)scan + q];
  TsdfCastLane lane;
  TsdfCastResult r{-1, INFINITY, NAN, {NAN, NAN, NAN}, NAN, kTsdfCastSkipped, 0};
  if (tsdf_cast_setup(vp, dir, M, mask ? mask[g] != 0 : true, &lane)) r = tsdf_cast_ray(lane, grid, rule, total, mine);
  out.face[g] = r.face;
  out.t[g] = r.t;
  out.inc[g] = r.inc;
  out.normal[3 * g] = r.normal[0];
  out.normal[3 * g + 1] = r.normal[1];
  out.normal[3 * g + 2] = r.normal[2];
  out.phi[g] = r.phi;
  out.status[g] = (uint8_t)r.status;
  out.samples[g] = r.samples;
}

}  // namespace dc

using namespace dc;

extern "C" {

int dc_tsdf_sparse_cast_rays(const uint64_t* keys, const int32_t* slots, const int64_t* n_blocks, int64_t capacity, const int64_t* sum,
                             const int32_t* count, const uint64_t* own_keys, const int32_t* own_slots, const int64_t* own_ptr,
                             int64_t n_own_keys, int64_t own_capacity, const int64_t* own_sum, const int32_t* own_count, double ox, double oy,
                             double oz, double voxel, double trunc, int min_count, const void* vps, const void* dirs, const uint8_t* mask,
                             int dtype, int64_t n, const int64_t* scan_offset, const double* poses, int n_scans, double t_min, double t_max,
                             double step, int refine, int skip, int32_t* face_out, double* t_out, double* inc_out, double* normal_out,
                             double* phi_out, uint8_t* status_out, int32_t* samples_out, hipStream_t stream) {
  const TsdfGrid grid{{ox, oy, oz}, voxel, {0, 0, 0}};
  if (dtype != DC_F32 && dtype != DC_F64) return DC_ERR_DTYPE;
  if (!tsdf_lattice_ok(grid) || !(trunc > 0.0) || !isfinite(trunc) || min_count < 1 || n < 0 || capacity < 1 || capacity >= ((int64_t)1 << 22) ||
      refine < 0)
    return DC_ERR_ARG;
  const int J = tsdf_cast_steps(t_min, t_max, step, trunc);
  if (J < 0) return DC_ERR_ARG;
  if (own_keys && (!own_slots || !own_ptr || !own_sum || !own_count || n_own_keys < 0 || own_capacity < 1)) return DC_ERR_ARG;
  if (n == 0) return DC_OK;
  if (!keys || !slots || !n_blocks || !sum || !count || !vps || !dirs || !scan_offset || !poses || n_scans < 1 || !face_out || !t_out ||
      !inc_out || !normal_out || !phi_out || !status_out || !samples_out)
    return DC_ERR_ARG;
  const int64_t blocks = (n + kTsdfCastBlock - 1) / kTsdfCastBlock;
  if (blocks > 0x7fffffff) return DC_ERR_UNSUPPORTED;
  const TsdfTable total{keys, slots, 0, capacity, sum, count};
  const TsdfCastOwn own{own_keys, own_slots, own_ptr, n_own_keys, own_capacity, own_sum, own_count};
  const TsdfCastRule rule{t_min, step, trunc, J, refine, min_count, skip != 0};
  const TsdfCastOut out{face_out, t_out, inc_out, normal_out, phi_out, status_out, samples_out};
  if (dtype == DC_F32)
    hipLaunchKernelGGL(tsdf_cast_kernel<float>, dim3((unsigned)blocks), dim3(kTsdfCastBlock), 0, stream, total, n_blocks, own, grid, rule,
                       (const float*)vps, (const float*)dirs, mask, n, scan_offset, poses, n_scans, out);
  else
    hipLaunchKernelGGL(tsdf_cast_kernel<double>, dim3((unsigned)blocks), dim3(kTsdfCastBlock), 0, stream, total, n_blocks, own, grid, rule,
                       (const double*)vps, (const double*)dirs, mask, n, scan_offset, poses, n_scans, out);
  DC_HIP(hipGetLastError());
  return DC_OK;
}

}  // extern "C"
