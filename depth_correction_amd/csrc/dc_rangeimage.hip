// Range-image neighbourhoods (gfx950): a scan as an organised H x W cloud.  The reference flattens its Ouster's H x W clouds
// (`if cloud.ndim == 2: cloud = cloud.reshape((-1,))`) and projects them back onto the sphere where it needs an image
// (scripts/depth_denoising:44-91 range_projection / :94-116 depth_to_points, scripts/compare_to_ddd); here the image IS the
// neighbourhood structure: the neighbours of a pixel are the pixels around it -- no grid, no sort, no search.
//   dc_range_project        pixel of every point, nearest point per pixel (ties: lower index), range image
//   dc_range_organize       the same + the winners compacted in pixel order as DepthCloud source fields
//   dc_range_from_grid      the same outputs for a sensor that delivers the H x W array itself (no projection)
//   dc_range_index_image    index image of a cloud that carries its pixels (after rows were dropped)
//   dc_image_features_fwd   dc_features_fwd's outputs on window neighbourhoods with a 3-D radius gate, ONE launch
//   dc_image_shadow_mask    dc_shadow_filter's mask with the candidates taken from the window
// The pixel rule, the window arithmetic and the membership predicate live in dc_rangeimage_math.h (host build: dc_hostcheck.cpp);
// the moments, the eigen-decomposition and the normal are dc_features_fwd's own functions (dc_pointmath.h, dc_eig3.h), the shadow
// pair test is dc_shadow_filter's (dc_shadow_pair.h).  DESIGN "Range-image neighbourhoods".
#include <cstring>
#include "dc_common.h"
#include "../../include/dc_hip.h"
#include "dc_device.h"
#include "dc_hostutil.h"
#include "dc_sort.h"
#include "dc_pointmath.h"
#include "dc_rangeimage_math.h"
#include "dc_shadow_pair.h"

namespace dc {

// ray of raw row i in the sensor frame, fp64: the widened coordinates minus the widened viewpoint
template <typename TI>
__device__ __forceinline__ void sensor_ray(const TI* __restrict__ pts, int stride, const TI* __restrict__ vps, int vps_rows, int64_t i,
                                           double* ray) {
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double vp = vps ? (double)vps[(vps_rows == 1 ? 0 : i * 3) + a] : 0.0;
    ray[a] = (double)pts[i * stride + a] - vp;
  }
}

// ---- the winner of every pixel, two passes (a 64-bit key cannot hold an fp64 depth AND the index) ---------------------------------
// pass 1: pixel[i]; keys[pixel] = min over the pixel's points of the order-preserving bits of the depth
template <typename TI>
__global__ __launch_bounds__(kBlock) void range_depth_pass_kernel(const TI* __restrict__ pts, int stride, const TI* __restrict__ vps,
                                                                  int vps_rows, int64_t n, RangeGrid g, int clamp, double min_depth,
                                                                  int32_t* __restrict__ pixel, unsigned long long* __restrict__ keys) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  double ray[3], depth;
  sensor_ray(pts, stride, vps, vps_rows, i, ray);
  const int32_t p = range_pixel(g, ray[0], ray[1], ray[2], clamp, min_depth, &depth);
  pixel[i] = p;
  if (p >= 0) atomicMin(&keys[p], (unsigned long long)range_depth_key(depth));
}

// pass 2: among the points whose depth IS the pixel's minimum the lowest index wins (index_image starts above every index)
template <typename TI>
__global__ __launch_bounds__(kBlock) void range_index_pass_kernel(const TI* __restrict__ pts, int stride, const TI* __restrict__ vps,
                                                                  int vps_rows, int64_t n, const int32_t* __restrict__ pixel,
                                                                  const unsigned long long* __restrict__ keys,
                                                                  int32_t* __restrict__ index_image) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const int32_t p = pixel[i];
  if (p < 0) return;
  double ray[3];
  sensor_ray(pts, stride, vps, vps_rows, i, ray);
  const double depth = range_depth(ray[0], ray[1], ray[2]);       // (the very function range_pixel calls: the same bits)
  if ((unsigned long long)range_depth_key(depth) == keys[p]) atomicMin(&index_image[p], (int32_t)i);
}

// per pixel: -1 where nothing landed, the range image (-1 for an empty pixel, as the reference writes), the occupancy flag
template <typename TO>
__global__ __launch_bounds__(kBlock) void range_finalize_kernel(const unsigned long long* __restrict__ keys, int64_t hw,
                                                                int32_t* __restrict__ index_image, TO* __restrict__ range_image,
                                                                int32_t* __restrict__ flags) {
  const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (p >= hw) return;
  const unsigned long long k = keys[p];
  const bool empty = k == DC_RANGE_EMPTY_KEY;
  if (empty) index_image[p] = -1;
  if (range_image) range_image[p] = empty ? (TO)-1 : (TO)range_key_depth((uint64_t)k);
  if (flags) flags[p] = empty ? 0 : 1;
}

// an H x W array of points: row-major order is the pixel order, a pixel is occupied when its ray is finite and deeper than min_depth
template <typename TI, typename TO>
__global__ __launch_bounds__(kBlock) void range_grid_flags_kernel(const TI* __restrict__ pts, int stride, const TI* __restrict__ vps,
                                                                  int vps_rows, int64_t hw, double min_depth,
                                                                  int32_t* __restrict__ index_image, TO* __restrict__ range_image,
                                                                  int32_t* __restrict__ flags) {
  const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (p >= hw) return;
  double ray[3];
  sensor_ray(pts, stride, vps, vps_rows, p, ray);
  const double depth = range_depth(ray[0], ray[1], ray[2]);
  const bool ok = fabs(ray[0]) < INFINITY && fabs(ray[1]) < INFINITY && fabs(ray[2]) < INFINITY && depth > min_depth && depth < INFINITY;
  index_image[p] = ok ? (int32_t)p : -1;
  if (range_image) range_image[p] = ok ? (TO)depth : (TO)-1;
  flags[p] = ok ? 1 : 0;
}

// The winners in pixel order: pos = exclusive prefix sums of the flags.  The source fields are DepthCloud.from_points' (depth_cloud.py:592-638,
// scan_compact_kernel of dc_scanio.hip: the raw row converted to the cloud's dtype, then the viewpoint subtracted; zero-depth rays cannot
// occur here), points = vps + depth * dirs with the product and the sum rounded separately (dc_to_points).  index_image is rewritten to
// point at the compact rows.
template <typename TI, typename TO>
__global__ __launch_bounds__(kBlock) void range_gather_kernel(const TI* __restrict__ pts, int stride, const TI* __restrict__ vps, int vps_rows,
                                                              int64_t hw, int32_t* __restrict__ index_image, const int32_t* __restrict__ flags,
                                                              const int32_t* __restrict__ pos, TO* __restrict__ vps_out, TO* __restrict__ dirs_out,
                                                              TO* __restrict__ depth_out, TO* __restrict__ points_out,
                                                              int32_t* __restrict__ pixel_out, int32_t* __restrict__ index_out,
                                                              int64_t* __restrict__ count_out) {
#pragma clang fp contract(off)
  const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (p >= hw) return;
  if (p == hw - 1) *count_out = (int64_t)pos[p] + flags[p];
  if (!flags[p]) return;
  const int64_t i = index_image[p], o = pos[p];
  TO ray[3], vp[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    vp[a] = vps ? (TO)vps[(vps_rows == 1 ? 0 : i * 3) + a] : (TO)0;
    ray[a] = (TO)pts[i * stride + a] - vp[a];
  }
  const TO d = sqrt(ray[0] * ray[0] + ray[1] * ray[1] + ray[2] * ray[2]);
  depth_out[o] = d;
  const bool unit = d > (TO)0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const TO dir = unit ? ray[a] / d : ray[a];
    dirs_out[o * 3 + a] = dir;
    vps_out[o * 3 + a] = vp[a];
    if (points_out) { const TO prod = d * dir; points_out[o * 3 + a] = vp[a] + prod; }
  }
  pixel_out[o] = (int32_t)p;
  if (index_out) index_out[o] = (int32_t)i;
  index_image[p] = (int32_t)o;
}

__global__ __launch_bounds__(kBlock) void range_scatter_index_kernel(const int32_t* __restrict__ pixel, int64_t m, const int64_t* __restrict__ count,
                                                                     int64_t hw, int32_t* __restrict__ index_image) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int64_t mm = count ? (*count < m ? *count : m) : m;
  if (i >= mm) return;
  const int32_t p = pixel[i];
  if (p >= 0 && p < hw) index_image[p] = (int32_t)i;
}

// ------------------------------------------------------------------------------------------------------------------------------------
// Window features of a whole organised scan in one launch.
// STAGED: a workgroup owns a tile of kTileH x kTileW = 8 x 32 pixels (a wavefront: two image rows of 32) and stages the tile plus its halo
// of (ah, aw) pixels ONCE into LDS -- the index image first (consecutive lanes read consecutive pixels of an image row; column wrap,
// clipped columns and rows outside the image become -1 here), then the xyz of the occupied pixels (rows of an organised cloud are in pixel
// order: the rows of one image row are a near-contiguous run) -- as four planes {index, x, y, z}: the lanes of a wavefront walk their
// windows in step, so a slot is read by 32 consecutive lanes at 32 consecutive words (no bank conflict; 8-B words for float64).  One lane
// per centre pixel then walks its (2 ah + 1)(2 aw + 1) slots out of LDS in window order.  At window (3,3) and float64 the staged tile is
// 14 x 38 x 28 B = 14.9 KB; the staged form is taken up to 20 KB, where eight workgroups (the CU's 32 wavefronts) still fit the 160 KB of
// LDS -- occupancy is never LDS-bound.  Larger windows (and that is all it is for) take the DIRECT form: one lane per cloud row reads the
// index image and the rows from global memory.  Both forms accumulate the slots in window order with cov_add and finish with cov_finish /
// eig3_sym / normal_and_incidence exactly as features_fwd_kernel does on a table holding the same members in the same order.
// No atomics, no host round trip; tile and launch bounds are fixed here.
constexpr int kTileH = 8, kTileW = 32;
constexpr size_t kImageStageMax = 20 * 1024;
static inline size_t image_stage_bytes(int ah, int aw, int es) {
  const size_t nh = (size_t)(kTileH + 2 * ah) * (size_t)(kTileW + 2 * aw), nh4 = (nh + 3) & ~(size_t)3;
  return nh4 * (4 + 3 * (size_t)es);
}

template <typename T, bool STAGED>
__global__ __launch_bounds__(kBlock) void image_features_kernel(
    const T* __restrict__ x, const T* __restrict__ dirs, const int32_t* __restrict__ pixel, const int32_t* __restrict__ index_image, int64_t m,
    const int64_t* __restrict__ count, RangeGrid g, int ah, int aw, double rad, T* __restrict__ mean, T* __restrict__ cov,
    T* __restrict__ eigvals, T* __restrict__ eigvecs, T* __restrict__ normals, T* __restrict__ inc, int32_t* __restrict__ nvalid,
    int32_t* __restrict__ nbr_out) {
  extern __shared__ int4 image_lds[];
  const int hw_ = kTileW + 2 * aw, hh = kTileH + 2 * ah, nh = hw_ * hh, nh4 = (nh + 3) & ~3;
  int32_t* s_idx = reinterpret_cast<int32_t*>(image_lds);
  T* s_x = reinterpret_cast<T*>(s_idx + nh4);
  T* s_y = s_x + nh4;
  T* s_z = s_y + nh4;
  const QParams qp{};
  int64_t i;
  int r, c, e0 = 0;
  if (STAGED) {
    const int tiles_c = (g.cols + kTileW - 1) / kTileW;
    const int r0 = ((int)blockIdx.x / tiles_c) * kTileH, c0 = ((int)blockIdx.x % tiles_c) * kTileW;
    for (int e = threadIdx.x; e < nh; e += kBlock) {
      const int hr = e / hw_, hc = e - hr * hw_;
      const int rr = r0 - ah + hr;
      int cc = c0 - aw + hc;
      bool in = rr >= 0 && rr < g.rows;
      if (cc < 0 || cc >= g.cols) {
        if (g.wrap) { cc %= g.cols; cc = cc < 0 ? cc + g.cols : cc; }
        else in = false;
      }
      s_idx[e] = in ? index_image[(int64_t)rr * g.cols + cc] : -1;
    }
    for (int e = threadIdx.x; e < nh; e += kBlock) {          // (each thread reads back the slots it wrote: no barrier in between)
      const int32_t j = s_idx[e];
      if (j >= 0 && j < m) {
        s_x[e] = x[(int64_t)j * 3]; s_y[e] = x[(int64_t)j * 3 + 1]; s_z[e] = x[(int64_t)j * 3 + 2];
      } else s_idx[e] = -1;
    }
    __syncthreads();
    const int tr = threadIdx.x / kTileW, tc = threadIdx.x % kTileW;
    r = r0 + tr; c = c0 + tc;
    if (r >= g.rows || c >= g.cols) return;
    e0 = (tr + ah) * hw_ + tc + aw;
    i = s_idx[e0];
    if (i < 0) return;
  } else {
    i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t mm = count ? (*count < m ? *count : m) : m;
    if (i >= mm) return;
    const int32_t p = pixel[i];
    if (p < 0 || (int64_t)p >= (int64_t)g.rows * g.cols) return;
    r = p / g.cols; c = p - r * g.cols;
  }
  double xi[3];
  if (STAGED) { xi[0] = (double)s_x[e0]; xi[1] = (double)s_y[e0]; xi[2] = (double)s_z[e0]; }
  else Row3<T, 3>::load(x, i, xi, qp);
  const int kw = 2 * aw + 1, K = (2 * ah + 1) * kw;
  CovAcc acc;
  cov_init(acc);
  int32_t* row = nbr_out ? nbr_out + i * K : nullptr;
  int slot = 0;
  for (int dr = -ah; dr <= ah; ++dr) {
    for (int dc = -aw; dc <= aw; ++dc, ++slot) {
      int32_t j;
      double xj[3] = {0.0, 0.0, 0.0};
      if (STAGED) {
        const int e = e0 + dr * hw_ + dc;
        j = s_idx[e];
        if (j >= 0) { xj[0] = (double)s_x[e]; xj[1] = (double)s_y[e]; xj[2] = (double)s_z[e]; }
      } else {
        const int32_t pj = image_window_pixel(g, r, c, dr, dc);
        j = pj < 0 ? -1 : index_image[pj];
        if (j >= m) j = -1;
        if (j >= 0) Row3<T, 3>::load(x, j, xj, qp);
      }
      const bool member = image_member(j >= 0, dr == 0 && dc == 0, xi, xj, rad);
      if (member) cov_add(acc, xj[0] - xi[0], xj[1] - xi[1], xj[2] - xi[2], 1.0);
      if (row) row[slot] = member ? j : -1;
    }
  }
  double moff[3], cm[3], C[6], D, omega;
  cov_finish(acc, 0.0, moff, cm, C, &D, &omega);
  if (mean) { mean[i * 3] = (T)(xi[0] + moff[0]); mean[i * 3 + 1] = (T)(xi[1] + moff[1]); mean[i * 3 + 2] = (T)(xi[2] + moff[2]); }
  if (cov) {
    T* o = cov + i * 9;
    o[0] = (T)C[0]; o[1] = (T)C[1]; o[2] = (T)C[2];
    o[3] = (T)C[1]; o[4] = (T)C[3]; o[5] = (T)C[4];
    o[6] = (T)C[2]; o[7] = (T)C[4]; o[8] = (T)C[5];
  }
  if (nvalid) nvalid[i] = (int32_t)acc.W;
  if (eigvals || eigvecs || normals || inc) {
    double lam[3], V[3][3];
    eig3_sym<double>(C[0], C[1], C[2], C[3], C[4], C[5], lam, V);
    if (eigvals) { eigvals[i * 3] = (T)lam[0]; eigvals[i * 3 + 1] = (T)lam[1]; eigvals[i * 3 + 2] = (T)lam[2]; }
    if (eigvecs) {   // torch layout: eigvecs[i, :, k] = k-th eigenvector
      T* e = eigvecs + i * 9;
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) e[a * 3 + b] = (T)V[b][a];
    }
    if (normals || inc) {
      double dr3[3], nrm[3], a;
      Row3<T, 3>::load(dirs, i, dr3, qp);
      normal_and_incidence(dr3, V[0], nrm, &a);
      if (normals) Row3<T, 3>::store(normals, i, nrm, qp);
      if (inc) inc[i] = (T)a;
    }
  }
}

// Scan-shadow mask with the candidates taken from the image window: one lane per row walks the window of its pixel; a candidate is a
// direction neighbour by dc_shadow_filter's own inclusion test and meets the ray through its own pair test (dc_shadow_pair.h).  The mask
// depends on the SET of direction neighbours only, so it is dc_shadow_filter's whenever the window holds them all.  Rows at and beyond
// *count (when given) get 0.
template <typename T>
__global__ __launch_bounds__(kBlock) void image_shadow_kernel(const T* __restrict__ x, const T* __restrict__ vps, int vps_rows,
                                                              const T* __restrict__ dirs, const int32_t* __restrict__ pixel,
                                                              const int32_t* __restrict__ index_image, int64_t m,
                                                              const int64_t* __restrict__ count, RangeGrid g, int ah, int aw, double rad, T lo,
                                                              T hi, uint8_t* __restrict__ mask) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= m) return;
  const int32_t p = pixel[i];
  if ((count && i >= *count) || p < 0 || (int64_t)p >= (int64_t)g.rows * g.cols) { mask[i] = 0; return; }
  const int r = p / g.cols, c = p - r * g.cols;
  const double q[3] = {(double)dirs[i * 3], (double)dirs[i * 3 + 1], (double)dirs[i * 3 + 2]};
  const double r2 = rad * rad;
  ShadowRay<T> ray;
  shadow_ray_init(ray, x, vps, vps_rows, i);
  for (int dr = -ah; dr <= ah; ++dr)
    for (int dc = -aw; dc <= aw; ++dc) {
      const int32_t pj = image_window_pixel(g, r, c, dr, dc);
      const int64_t j = pj < 0 ? -1 : index_image[pj];
      if (j < 0 || j >= m) continue;
      const double pp[3] = {(double)dirs[j * 3], (double)dirs[j * 3 + 1], (double)dirs[j * 3 + 2]};
      if (sqdist(pp, q) <= r2) shadow_ray_meet(ray, x, j);
    }
  mask[i] = shadow_ray_kept(ray.cmin, ray.cmax, ray.bad, lo, hi) ? 1 : 0;
}

struct RangeWs {
  unsigned long long* keys;
  int32_t *pixel, *flags, *pos;
  void* scan;
  size_t scan_bytes, total;
};
static RangeWs carve_range(void* ws, int64_t n, int64_t hw) {
  Carver c(ws);
  RangeWs w;
  const size_t ne = (size_t)(n > 0 ? n : 1), np = (size_t)(hw > 0 ? hw : 1);
  w.keys = c.take<unsigned long long>(np);
  w.pixel = c.take<int32_t>(ne);
  w.flags = c.take<int32_t>(np);
  w.pos = c.take<int32_t>(np);
  w.scan_bytes = scan_bytes(np);
  w.scan = c.take<char>(w.scan_bytes);
  w.total = c.off + 256;
  return w;
}

static inline unsigned blocks_of(int64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

// keys, pixel and the provisional index image of n raw rows (the finalize pass is the caller's)
template <typename TI>
static int launch_winner_passes(const TI* pts, int stride, const TI* vps, int vps_rows, int64_t n, const RangeGrid& g, int clamp,
                                double min_depth, int32_t* pixel, unsigned long long* keys, int32_t* index_image, hipStream_t stream) {
  const int64_t hw = (int64_t)g.rows * g.cols;
  DC_HIP(hipMemsetAsync(keys, 0xff, (size_t)hw * sizeof(unsigned long long), stream));      // DC_RANGE_EMPTY_KEY
  DC_HIP(hipMemsetAsync(index_image, 0x7f, (size_t)hw * sizeof(int32_t), stream));          // 0x7f7f7f7f: above every index
  if (n == 0) return DC_OK;
  hipLaunchKernelGGL((range_depth_pass_kernel<TI>), dim3(blocks_of(n)), dim3(kBlock), 0, stream, pts, stride, vps, vps_rows, n, g, clamp,
                     min_depth, pixel, keys);
  hipLaunchKernelGGL((range_index_pass_kernel<TI>), dim3(blocks_of(n)), dim3(kBlock), 0, stream, pts, stride, vps, vps_rows, n,
                     (const int32_t*)pixel, (const unsigned long long*)keys, index_image);
  return DC_OK;
}

}  // namespace dc

using namespace dc;

static bool range_args_ok(int64_t n, int stride, const void* points, const void* vps, int vps_rows, const RangeGrid& g) {
  if (n < 0 || stride < 3 || !range_grid_ok(g) || (n > 0 && !points)) return false;
  if (vps && vps_rows != 1 && vps_rows != n) return false;
  return true;
}

extern "C" {

size_t dc_range_project_workspace_bytes(int64_t n, int rows, int cols) {
  if (n < 0 || rows < 1 || cols < 1) return 0;
  return carve_range(nullptr, 0, (int64_t)rows * cols).total;
}

int dc_range_project(const void* points, int stride, int dtype, const void* vps, int vps_rows, int64_t n, int rows, int cols, double fov_up,
                     double fov_down, int wrap, int clamp, double min_depth, int32_t* pixel, int32_t* index_image, void* range_image, void* ws,
                     size_t ws_bytes, hipStream_t stream) {
  const RangeGrid g{rows, cols, fov_up, fov_down, wrap};
  if (!range_args_ok(n, stride, points, vps, vps_rows, g) || !index_image || !ws || (n > 0 && !pixel) || min_depth != min_depth) return DC_ERR_ARG;
  if (dtype != DC_F32 && dtype != DC_F64) return DC_ERR_DTYPE;
  if (n >= (int64_t)0x7f000000) return DC_ERR_UNSUPPORTED;
  const int64_t hw = (int64_t)rows * cols;
  RangeWs w = carve_range(ws, 0, hw);
  if (ws_bytes < w.total) return DC_ERR_WORKSPACE;
  int rc;
  if (dtype == DC_F32) {
    rc = launch_winner_passes((const float*)points, stride, (const float*)vps, vps_rows, n, g, clamp, min_depth, pixel, w.keys, index_image, stream);
    if (rc) return rc;
    hipLaunchKernelGGL((range_finalize_kernel<float>), dim3(blocks_of(hw)), dim3(kBlock), 0, stream, (const unsigned long long*)w.keys, hw,
                       index_image, (float*)range_image, (int32_t*)nullptr);
  } else {
    rc = launch_winner_passes((const double*)points, stride, (const double*)vps, vps_rows, n, g, clamp, min_depth, pixel, w.keys, index_image, stream);
    if (rc) return rc;
    hipLaunchKernelGGL((range_finalize_kernel<double>), dim3(blocks_of(hw)), dim3(kBlock), 0, stream, (const unsigned long long*)w.keys, hw,
                       index_image, (double*)range_image, (int32_t*)nullptr);
  }
  DC_HIP(hipGetLastError());
  return DC_OK;
}

size_t dc_range_organize_workspace_bytes(int64_t n, int rows, int cols) {
  if (n < 0 || rows < 1 || cols < 1) return 0;
  return carve_range(nullptr, n, (int64_t)rows * cols).total;
}

int dc_range_organize(const void* points, int stride, int in_dtype, const void* vps, int vps_rows, int64_t n, int rows, int cols, double fov_up,
                      double fov_down, int wrap, int clamp, double min_depth, int out_dtype, void* vps_out, void* dirs_out, void* depth_out,
                      void* points_out, int32_t* pixel_out, int32_t* index_out, int32_t* index_image, void* range_image, int64_t* count_out,
                      void* ws, size_t ws_bytes, hipStream_t stream) {
  const RangeGrid g{rows, cols, fov_up, fov_down, wrap};
  if (!range_args_ok(n, stride, points, vps, vps_rows, g) || !index_image || !count_out || !ws || min_depth != min_depth) return DC_ERR_ARG;
  if (n > 0 && (!vps_out || !dirs_out || !depth_out || !pixel_out)) return DC_ERR_ARG;
  if ((in_dtype != DC_F32 && in_dtype != DC_F64) || (out_dtype != DC_F32 && out_dtype != DC_F64)) return DC_ERR_DTYPE;
  if (n >= (int64_t)0x7f000000) return DC_ERR_UNSUPPORTED;
  const int64_t hw = (int64_t)rows * cols;
  RangeWs w = carve_range(ws, n, hw);
  if (ws_bytes < w.total) return DC_ERR_WORKSPACE;
#define RUN(TI, TO)                                                                                                                        \
  do {                                                                                                                                     \
    const int rc = launch_winner_passes((const TI*)points, stride, (const TI*)vps, vps_rows, n, g, clamp, min_depth, w.pixel, w.keys,       \
                                        index_image, stream);                                                                              \
    if (rc) return rc;                                                                                                                     \
    hipLaunchKernelGGL((range_finalize_kernel<TO>), dim3(blocks_of(hw)), dim3(kBlock), 0, stream, (const unsigned long long*)w.keys, hw,    \
                       index_image, (TO*)range_image, w.flags);                                                                            \
    if (n == 0) break;                                                                                                                     \
    DC_HIP(exclusive_scan_32(w.scan, w.scan_bytes, w.flags, w.pos, (size_t)hw, stream));                                                   \
    hipLaunchKernelGGL((range_gather_kernel<TI, TO>), dim3(blocks_of(hw)), dim3(kBlock), 0, stream, (const TI*)points, stride,              \
                       (const TI*)vps, vps_rows, hw, index_image, (const int32_t*)w.flags, (const int32_t*)w.pos, (TO*)vps_out,            \
                       (TO*)dirs_out, (TO*)depth_out, (TO*)points_out, pixel_out, index_out, count_out);                                   \
  } while (0)
  if (in_dtype == DC_F32 && out_dtype == DC_F32) RUN(float, float);
  else if (in_dtype == DC_F32) RUN(float, double);
  else if (out_dtype == DC_F32) RUN(double, float);
  else RUN(double, double);
#undef RUN
  if (n == 0) DC_HIP(hipMemsetAsync(count_out, 0, sizeof(int64_t), stream));
  DC_HIP(hipGetLastError());
  return DC_OK;
}

int dc_range_from_grid(const void* points, int stride, int in_dtype, const void* vps, int vps_rows, int rows, int cols, double min_depth,
                       int out_dtype, void* vps_out, void* dirs_out, void* depth_out, void* points_out, int32_t* pixel_out, int32_t* index_out,
                       int32_t* index_image, void* range_image, int64_t* count_out, void* ws, size_t ws_bytes, hipStream_t stream) {
  const RangeGrid g{rows, cols, 1.0, -1.0, 1};          // (only the size matters here)
  const int64_t hw = (int64_t)rows * cols;
  if (!range_grid_ok(g) || stride < 3 || !points || !index_image || !count_out || !ws || min_depth != min_depth) return DC_ERR_ARG;
  if (vps && vps_rows != 1 && vps_rows != hw) return DC_ERR_ARG;
  if (!vps_out || !dirs_out || !depth_out || !pixel_out) return DC_ERR_ARG;
  if ((in_dtype != DC_F32 && in_dtype != DC_F64) || (out_dtype != DC_F32 && out_dtype != DC_F64)) return DC_ERR_DTYPE;
  RangeWs w = carve_range(ws, 0, hw);
  if (ws_bytes < w.total) return DC_ERR_WORKSPACE;
#define RUN(TI, TO)                                                                                                                        \
  do {                                                                                                                                     \
    hipLaunchKernelGGL((range_grid_flags_kernel<TI, TO>), dim3(blocks_of(hw)), dim3(kBlock), 0, stream, (const TI*)points, stride,          \
                       (const TI*)vps, vps_rows, hw, min_depth, index_image, (TO*)range_image, w.flags);                                   \
    DC_HIP(exclusive_scan_32(w.scan, w.scan_bytes, w.flags, w.pos, (size_t)hw, stream));                                                   \
    hipLaunchKernelGGL((range_gather_kernel<TI, TO>), dim3(blocks_of(hw)), dim3(kBlock), 0, stream, (const TI*)points, stride,              \
                       (const TI*)vps, vps_rows, hw, index_image, (const int32_t*)w.flags, (const int32_t*)w.pos, (TO*)vps_out,            \
                       (TO*)dirs_out, (TO*)depth_out, (TO*)points_out, pixel_out, index_out, count_out);                                   \
  } while (0)
  if (in_dtype == DC_F32 && out_dtype == DC_F32) RUN(float, float);
  else if (in_dtype == DC_F32) RUN(float, double);
  else if (out_dtype == DC_F32) RUN(double, float);
  else RUN(double, double);
#undef RUN
  DC_HIP(hipGetLastError());
  return DC_OK;
}

int dc_range_index_image(const int32_t* pixel, int64_t m, const int64_t* count, int rows, int cols, int32_t* index_image, hipStream_t stream) {
  const int64_t hw = (int64_t)rows * cols;
  if (m < 0 || rows < 1 || cols < 1 || hw > (int64_t)0x7fffffff || !index_image || (m > 0 && !pixel) || m > (int64_t)0x7fffffff) return DC_ERR_ARG;
  DC_HIP(hipMemsetAsync(index_image, 0xff, (size_t)hw * sizeof(int32_t), stream));
  if (m == 0) return DC_OK;
  hipLaunchKernelGGL(range_scatter_index_kernel, dim3(blocks_of(m)), dim3(kBlock), 0, stream, pixel, m, count, hw, index_image);
  DC_HIP(hipGetLastError());
  return DC_OK;
}

int dc_image_features_fwd(const void* points, const void* dirs, int dtype, const int32_t* pixel, const int32_t* index_image, int64_t m,
                          const int64_t* count, int rows, int cols, int wrap, int ah, int aw, double r, void* mean, void* cov, void* eigvals,
                          void* eigvecs, void* normals, void* inc_angles, int32_t* nvalid, int32_t* nbr_out, hipStream_t stream) {
  const RangeGrid g{rows, cols, 1.0, -1.0, wrap};
  if (m < 0 || !range_grid_ok(g) || !image_window_ok(g, ah, aw) || r != r) return DC_ERR_ARG;
  if (dtype != DC_F32 && dtype != DC_F64) return DC_ERR_DTYPE;
  if (m == 0) return DC_OK;
  if (!points || !pixel || !index_image || ((normals || inc_angles) && !dirs) || m > (int64_t)0x7fffffff) return DC_ERR_ARG;
  const size_t lds = image_stage_bytes(ah, aw, dtype == DC_F32 ? 4 : 8);
  const bool staged = lds <= kImageStageMax;
  const unsigned tiles = (unsigned)(((rows + kTileH - 1) / kTileH) * ((cols + kTileW - 1) / kTileW));
#define LAUNCH(T, ST, GRID, LDS)                                                                                                           \
  hipLaunchKernelGGL((image_features_kernel<T, ST>), dim3(GRID), dim3(kBlock), LDS, stream, (const T*)points, (const T*)dirs, pixel,        \
                     index_image, m, count, g, ah, aw, r, (T*)mean, (T*)cov, (T*)eigvals, (T*)eigvecs, (T*)normals, (T*)inc_angles, nvalid, \
                     nbr_out)
  if (dtype == DC_F32) { if (staged) LAUNCH(float, true, tiles, lds); else LAUNCH(float, false, blocks_of(m), 0); }
  else { if (staged) LAUNCH(double, true, tiles, lds); else LAUNCH(double, false, blocks_of(m), 0); }
#undef LAUNCH
  DC_HIP(hipGetLastError());
  return DC_OK;
}

int dc_image_shadow_mask(const void* points, const void* vps, int vps_rows, const void* dirs, int dtype, const int32_t* pixel,
                         const int32_t* index_image, int64_t m, const int64_t* count, int rows, int cols, int wrap, int ah, int aw, double r,
                         double lo, double hi, uint8_t* mask_out, hipStream_t stream) {
  const RangeGrid g{rows, cols, 1.0, -1.0, wrap};
  if (m < 0 || !range_grid_ok(g) || !image_window_ok(g, ah, aw) || !(r > 0.0)) return DC_ERR_ARG;
  if (dtype != DC_F32 && dtype != DC_F64) return DC_ERR_DTYPE;
  if (m == 0) return DC_OK;
  if (!points || !vps || !dirs || !pixel || !index_image || !mask_out || (vps_rows != 1 && vps_rows != m) || m > (int64_t)0x7fffffff)
    return DC_ERR_ARG;
  if (dtype == DC_F32)
    hipLaunchKernelGGL((image_shadow_kernel<float>), dim3(blocks_of(m)), dim3(kBlock), 0, stream, (const float*)points, (const float*)vps,
                       vps_rows, (const float*)dirs, pixel, index_image, m, count, g, ah, aw, r, (float)lo, (float)hi, mask_out);
  else
    hipLaunchKernelGGL((image_shadow_kernel<double>), dim3(blocks_of(m)), dim3(kBlock), 0, stream, (const double*)points, (const double*)vps,
                       vps_rows, (const double*)dirs, pixel, index_image, m, count, g, ah, aw, r, lo, hi, mask_out);
  DC_HIP(hipGetLastError());
  return DC_OK;
}

}  // extern "C"
