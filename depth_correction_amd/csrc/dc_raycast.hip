// Triangle-mesh ray casting for the rendered-mesh datasets (render.py; the reference rasterises with pytorch3d, dataset.py:1073-1130).
//
// LBVH build (dc_bvh_build), Karras 2012 "Maximizing parallelism in the construction of BVHs, octrees and k-d trees":
//   1. key[f] = (morton30(centroid_f in the scene box) << 32) | f -- unique keys, so the tree does not depend on scheduling;
//   2. dc::sort_pairs_u64 (dc_sort.h) orders the faces by key -> leaf_face;
//   3. internal node i of the n - 1 covers the leaf range found from the common-prefix lengths of its neighbours' keys;
//   4. bottom-up fitting: every leaf writes its box and climbs; one atomic counter per internal node lets the second child that
//      arrives form the parent's box.  Boxes are float32, rounded outward from the fp64 vertex bounds (round-down for the
//      minimum, round-up for the maximum), and an internal box is the exact min / max of its children's: bit-identical for any
//      arrival order, and every face lies inside each box on its path to the root.
// Node numbering: internal nodes 0 .. n-2 (root 0), leaf i is node n-1+i; with one face the root is leaf 0.  The tree's depth is
// at most 63: a child's keys share a strictly longer prefix than its parent's, and the 64-bit keys start with two zero bits.
//
// Closest-hit cast (dc_raycast): one lane per ray, every (pose, ray) pair in one launch.  The per-ray arithmetic is dc_raymath.h (host
// and device).  The boxes are tested in fp32 (slab test; the exit distance is scaled by 1 + 2^-20, Ize 2013's 1 + 2 gamma_3 with
// headroom for the fp32 rounding of the direction; the boxes grow by 2^-22 |origin|, at least 1e-20, for the rounding of the
// origin; a direction component below 1e-30 counts as 1e-30, so that a ray running exactly on a slab's boundary stays in it up
// to t = 1e10; and the best hit's t prunes with the same 1 + 2^-20, because the fp32 entry distance of a flat box met face-on can
// exceed the exact hit distance by a few 2^-24).  The walk is dc::bvh_walk (dc_bvh.h: the nearer child first, the other on a per-lane
// stack in LDS) with dc::TriVisitor (dc_raymath.h) deciding which boxes to enter.  Triangles are tested in fp64 with the watertight
// test of Woop, Benthin and Wald (JCGT 2013), no FMA contraction there (see test_triangle).  A hit counts when t > t_min (and
// dot(n, d) < 0 with culling).  Guaranteed, and pinned by tests/test_raycast_host.py and tests/test_gpu_raycast_edge.py:
//   1. no box is rejected that holds a face test_triangle reports a hit on, before the first hit and under the pruning rule;
//   2. so the cast returns what test_triangle over every face in index order returns: the smallest t, on equal t the lower face
//      index, independent of the tree and of the traversal order, bitwise reproducible and equal to the host build's answer;
//   3. a ray through a shared edge or vertex hits at least one of the faces around it.
//
// dc_raycast_rays casts the rays of measured clouds (per-ray view point and direction, per-scan pose) through the same device
// function (cast_ray) and adds the true incidence angle on the winning triangle: the ground truth of eval_bias.
//
// dc_raycast_beams renders finite beams: a bundle of S sub-rays per beam (dc_beammath.h) goes through cast_ray, one lane per sub-ray,
// and the S consecutive lanes of a beam reduce their returns to one return with cross-lane reads only (rules: dc_beammath.h).  S is
// a power of two <= 64, so a wavefront holds 64 / S whole beams; the lanes past the last beam stay in the kernel as misses until
// the reduction is done, because a cross-lane read from a lane that has left returns garbage.
//
// dc_raycast_sweep renders a moving sweep: every lane first forms its ray at its own sweep time (dc_sweepmath.h) in the start frame
// of its scan, then is one of raycast_rays_kernel's lanes; dc_sweep_rays writes those rays out instead of casting them.
//
// dc_surfel_bvh_build / dc_surfel_cast_rays cast the same measured rays against a surveyed cloud, every survey point an oriented disk
// (dc_surfelmath.h): the same build over the disks' boxes (build_tree; only the Morton keys and the leaves differ) and the same walk
// with dc::DiskVisitor -- the disk test at the leaves, then a second walk that blends the disks within a depth window behind the first
// hit.  The nearest-triangle queries (dc_meshwalk.h) are a third visitor of that one walk.
#include "dc_common.h"
#include "dc_bvh.h"
#include "dc_beammath.h"
#include "dc_raymath.h"
#include "dc_sweepmath.h"
#include "dc_surfelmath.h"
#include "dc_hostutil.h"
#include "dc_sort.h"
#include "../../include/dc_hip.h"

namespace {

constexpr int kBuildBlock = 256;
constexpr int kCastBlock = 128;
using dc::kBvhStackDepth;

__device__ __forceinline__ uint32_t expand_bits10(uint32_t v) {
  v &= 0x3ffu;
  v = (v | (v << 16)) & 0x030000ffu;
  v = (v | (v << 8)) & 0x0300f00fu;
  v = (v | (v << 4)) & 0x030c30c3u;
  v = (v | (v << 2)) & 0x09249249u;
  return v;
}

__device__ __forceinline__ uint32_t quantise10(double c, double lo, double scale) {
  double q = (c - lo) * scale;
  q = q < 0.0 ? 0.0 : (q > 1023.0 ? 1023.0 : q);
  return (uint32_t)q;
}

struct SceneBox {
  double lo[3];
  double scale[3];        // 1024 / extent (0 for a flat axis)
};

// key and value of primitive i with the centre c [3]: (morton30(c in the scene box) << 32) | i
__device__ __forceinline__ void morton_key(const double* c, const SceneBox& box, int64_t i, uint64_t* __restrict__ keys,
                                           uint32_t* __restrict__ vals) {
  uint32_t code = 0;
#pragma unroll
  for (int a = 0; a < 3; ++a) code |= expand_bits10(quantise10(c[a], box.lo[a], box.scale[a])) << (2 - a);
  keys[i] = ((uint64_t)code << 32) | (uint64_t)(uint32_t)i;
  vals[i] = (uint32_t)i;
}

__global__ void __launch_bounds__(kBuildBlock) morton_kernel(const double* __restrict__ verts, const int32_t* __restrict__ faces,
                                                             int64_t n, SceneBox box, uint64_t* __restrict__ keys,
                                                             uint32_t* __restrict__ vals) {
  const int64_t f = (int64_t)blockIdx.x * kBuildBlock + threadIdx.x;
  if (f >= n) return;
  double c[3];
#pragma unroll
  for (int a = 0; a < 3; ++a)
    c[a] = (verts[3 * (int64_t)faces[3 * f] + a] + verts[3 * (int64_t)faces[3 * f + 1] + a] + verts[3 * (int64_t)faces[3 * f + 2] + a]) *
           (1.0 / 3.0);
  morton_key(c, box, f, keys, vals);
}

// length of the common prefix of keys i and j, -1 outside [0, n)
__device__ __forceinline__ int delta(const uint64_t* __restrict__ keys, int64_t n, int64_t i, int64_t j) {
  if (j < 0 || j >= n) return -1;
  return __clzll((long long)(keys[i] ^ keys[j]));
}

__global__ void __launch_bounds__(kBuildBlock) karras_kernel(const uint64_t* __restrict__ keys, int64_t n, int32_t* __restrict__ child,
                                                             int32_t* __restrict__ parent) {
  const int64_t i = (int64_t)blockIdx.x * kBuildBlock + threadIdx.x;
  if (i >= n - 1) return;
  const int d = delta(keys, n, i, i + 1) > delta(keys, n, i, i - 1) ? 1 : -1;
  const int dmin = delta(keys, n, i, i - d);
  int64_t lmax = 2;
  while (delta(keys, n, i, i + lmax * d) > dmin) lmax *= 2;
  int64_t l = 0;
  for (int64_t t = lmax / 2; t >= 1; t /= 2)
    if (delta(keys, n, i, i + (l + t) * d) > dmin) l += t;
  const int64_t j = i + l * d;
  const int dnode = delta(keys, n, i, j);
  int64_t s = 0;
  for (int64_t t = (l + 1) / 2;; t = (t + 1) / 2) {       // ceil(l / 2), ceil(l / 4), ... down to 1
    if (delta(keys, n, i, i + (s + t) * d) > dnode) s += t;
    if (t == 1) break;
  }
  const int64_t gamma = i + s * d + (d < 0 ? -1 : 0);
  const int64_t lo = i < j ? i : j, hi = i < j ? j : i;
  const int32_t left = (int32_t)(lo == gamma ? (n - 1) + gamma : gamma);
  const int32_t right = (int32_t)(hi == gamma + 1 ? (n - 1) + gamma + 1 : gamma + 1);
  child[2 * i] = left;
  child[2 * i + 1] = right;
  parent[left] = (int32_t)i;
  parent[right] = (int32_t)i;
}

__global__ void __launch_bounds__(kBuildBlock) fit_kernel(const double* __restrict__ verts, const int32_t* __restrict__ faces, int64_t n,
                                                          const int32_t* __restrict__ leaf_face, const int32_t* __restrict__ child,
                                                          const int32_t* __restrict__ parent, int32_t* __restrict__ counter,
                                                          float* node_box, double* __restrict__ leaf_tri) {
  const int64_t i = (int64_t)blockIdx.x * kBuildBlock + threadIdx.x;
  if (i >= n) return;
  const int64_t f = leaf_face[i];
  double v[9];
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int a = 0; a < 3; ++a) v[3 * c + a] = verts[3 * (int64_t)faces[3 * f + c] + a];
#pragma unroll
  for (int k = 0; k < 9; ++k) leaf_tri[9 * i + k] = v[k];
  dc::leaf_box(v, node_box + 6 * ((n - 1) + i));
  dc::bvh_fit_climb((n - 1) + i, child, parent, counter, node_box);
}

using dc::Hit;
using dc::Ray32;
using dc::Ray64;

// A sensor-frame ray in the world: direction R s and origin R v + t of the pose M (4 x 4, row-major).  Every cast kernel forms its ray
// here, with the multiply-adds written out, so that kernels given the same ray cast the same bits: left to the compiler, the
// contraction of M[0] * s0 + M[1] * s1 + M[2] * s2 is chosen per call site (it depends on where s comes from -- a load, a conversion
// from fp32, the sweep arithmetic).  The order is the one the fp64 thin casts were built with.
__device__ __forceinline__ void pose_dir(const double* __restrict__ M, double s0, double s1, double s2, double& d0, double& d1, double& d2) {
#pragma clang fp contract(off)
  d0 = fma(M[2], s2, fma(M[0], s0, M[1] * s1));
  d1 = fma(M[6], s2, fma(M[4], s0, M[5] * s1));
  d2 = fma(M[10], s2, fma(M[9], s1, M[8] * s0));
}

__device__ __forceinline__ void pose_point(const double* __restrict__ M, double v0, double v1, double v2, double& o0, double& o1, double& o2) {
#pragma clang fp contract(off)
  o0 = fma(M[2], v2, fma(M[0], v0, M[1] * v1)) + M[3];
  o1 = fma(M[6], v2, fma(M[4], v0, M[5] * v1)) + M[7];
  o2 = fma(M[10], v2, fma(M[8], v0, M[9] * v1)) + M[11];
}

// |n . d| / (|n| |d|) on the triangle tri [9] with n = (v1 - v0) x (v2 - v0): the cosine of the incidence angle of the world-frame
// direction d (0 / 0 on a face of zero area: NaN).  Written out for the same reason as pose_dir, in the order raycast_rays_kernel<double>
// was built with; dc_raycast_rays and dc_raycast_sweep take its arccos, dc_raycast_beams weights a sub-ray with it.
__device__ __forceinline__ double incidence_cos(const double* __restrict__ tri, double d0, double d1, double d2) {
#pragma clang fp contract(off)
  const double e10 = tri[3] - tri[0], e11 = tri[4] - tri[1], e12 = tri[5] - tri[2];
  const double e20 = tri[6] - tri[0], e21 = tri[7] - tri[1], e22 = tri[8] - tri[2];
  const double n0 = fma(e11, e22, -(e12 * e21)), n1 = fma(e12, e20, -(e10 * e22)), n2 = fma(e10, e21, -(e11 * e20));
  const double nd = fma(n2, d2, fma(n0, d0, n1 * d1));
  const double nn = fma(n2, n2, fma(n0, n0, n1 * n1));
  const double dd = fma(d2, d2, fma(d0, d0, d1 * d1));
  return fabs(nd) / (sqrt(nn) * sqrt(dd));
}

// The ray of a measured point in the world: view point vps[g] and direction dirs[g] (sensor frame, fp32 or fp64) under the pose M.
// The beam and sweep kernels pass their own fp64 sub-ray (g = 0) and so cast the ray raycast_rays_kernel would.
template <typename T>
__device__ __forceinline__ void measured_ray(const T* __restrict__ vps, const T* __restrict__ dirs, int64_t g, const double* __restrict__ M,
                                             double& d0, double& d1, double& d2, double& o0, double& o1, double& o2) {
  const double s0 = (double)dirs[3 * g], s1 = (double)dirs[3 * g + 1], s2 = (double)dirs[3 * g + 2];
  const double v0 = (double)vps[3 * g], v1 = (double)vps[3 * g + 1], v2 = (double)vps[3 * g + 2];
  pose_dir(M, s0, s1, s2, d0, d1, d2);
  pose_point(M, v0, v1, v2, o0, o1, o2);
}

// Closest hit of one ray (origin o, direction d, both fp64 world frame) over the tree: the traversal every cast kernel shares.
// `stack` is the block's LDS stack (kBvhStackDepth x kCastBlock, lane-minor); best.leaf is the winning leaf's row of leaf_tri.
__device__ __forceinline__ Hit cast_ray(const int32_t* __restrict__ child, const float* __restrict__ node_box,
                                        const double* __restrict__ leaf_tri, const int32_t* __restrict__ leaf_face, int64_t n, double d0,
                                        double d1, double d2, double o0, double o1, double o2, double tmin, int cull, int32_t* stack,
                                        int lane) {
  dc::TriVisitor vis = {node_box, leaf_tri, leaf_face, tmin, cull != 0};
  dc::ray_setup(d0, d1, d2, o0, o1, o2, vis.ray64, vis.ray);
  vis.best = dc::no_hit();
  dc::bvh_walk<kCastBlock>(child, n, stack, lane, vis);
  return vis.best;
}

__global__ void __launch_bounds__(kCastBlock) raycast_kernel(const int32_t* __restrict__ child, const float* __restrict__ node_box,
                                                             const double* __restrict__ leaf_tri, const int32_t* __restrict__ leaf_face,
                                                             int64_t n, const double* __restrict__ dirs, const double* __restrict__ t_min,
                                                             int64_t n_rays, const double* __restrict__ poses, int64_t total, int cull,
                                                             int32_t* __restrict__ face_out, double* __restrict__ t_out,
                                                             double* __restrict__ bary_out) {
  __shared__ int32_t stack[kBvhStackDepth * kCastBlock];
  const int lane = threadIdx.x;
  const int64_t g = (int64_t)blockIdx.x * kCastBlock + lane;
  if (g >= total) return;
  const int64_t p = g / n_rays, r = g - p * n_rays;
  const double* M = poses + 16 * p;
  const double s0 = dirs[3 * r], s1 = dirs[3 * r + 1], s2 = dirs[3 * r + 2];
  double d0, d1, d2;
  pose_dir(M, s0, s1, s2, d0, d1, d2);
  const Hit best = cast_ray(child, node_box, leaf_tri, leaf_face, n, d0, d1, d2, M[3], M[7], M[11], t_min[r], cull, stack, lane);
  face_out[g] = best.face;
  t_out[g] = best.t;
  bary_out[2 * g] = best.u;
  bary_out[2 * g + 1] = best.v;
}

// The rays of measured clouds (dc_raycast_rays): per-ray view point and direction in the sensor frame of the ray's scan (dc::scan_of).
template <typename T>
__global__ void __launch_bounds__(kCastBlock) raycast_rays_kernel(const int32_t* __restrict__ child, const float* __restrict__ node_box,
                                                                  const double* __restrict__ leaf_tri, const int32_t* __restrict__ leaf_face,
                                                                  int64_t n, const T* __restrict__ vps, const T* __restrict__ dirs,
                                                                  int64_t total, const int64_t* __restrict__ scan_offset,
                                                                  const double* __restrict__ poses, int n_scans, double t_min, int cull,
                                                                  int32_t* __restrict__ face_out, double* __restrict__ t_out,
                                                                  double* __restrict__ inc_out) {
  __shared__ int32_t stack[kBvhStackDepth * kCastBlock];
  const int lane = threadIdx.x;
  const int64_t g = (int64_t)blockIdx.x * kCastBlock + lane;
  if (g >= total) return;
  double d0, d1, d2, o0, o1, o2;
  measured_ray(vps, dirs, g, poses + 16 * (int64_t)dc::scan_of(scan_offset, n_scans, g), d0, d1, d2, o0, o1, o2);
  const Hit best = cast_ray(child, node_box, leaf_tri, leaf_face, n, d0, d1, d2, o0, o1, o2, t_min, cull, stack, lane);
  face_out[g] = best.face;
  t_out[g] = best.t;
  double inc = NAN;
  if (best.leaf >= 0) inc = acos(fmin(1.0, incidence_cos(leaf_tri + 9 * (int64_t)best.leaf, d0, d1, d2)));   // zero area: NaN
  inc_out[g] = inc;
}

// The footprint pattern travels in the kernel's arguments (HOST array at the C ABI): no copy, no workspace.
struct BeamPattern {
  double v[3 * DC_BEAM_MAX_SAMPLES];          // rows (px, py, weight)
};

template <typename T>
__global__ void __launch_bounds__(kBuildBlock) beam_subrays_kernel(const T* __restrict__ vps, const T* __restrict__ dirs, int64_t total,
                                                                   BeamPattern pat, int n_samples, double r0, double spread,
                                                                   double* __restrict__ origins_out, double* __restrict__ dirs_out) {
  const int64_t g = (int64_t)blockIdx.x * kBuildBlock + threadIdx.x;
  if (g >= total) return;
  const int64_t i = g / n_samples;
  const int j = (int)(g - i * n_samples);
  const dc::BeamFrame f = dc::beam_frame((double)dirs[3 * i], (double)dirs[3 * i + 1], (double)dirs[3 * i + 2]);
  double o[3], D[3];
  dc::beam_subray(f, (double)vps[3 * i], (double)vps[3 * i + 1], (double)vps[3 * i + 2], pat.v[3 * j], pat.v[3 * j + 1], r0, spread, o, D);
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    origins_out[3 * g + a] = o[a];
    dirs_out[3 * g + a] = D[a];
  }
}

// One lane per sub-ray; sub-ray g = beam (g >> log2s), sample (g & (S - 1)).  kCastBlock is a multiple of 64 and S divides 64, so
// the S lanes of a beam are consecutive lanes of one wavefront, starting at a multiple of S.
template <typename T>
__global__ void __launch_bounds__(kCastBlock) raycast_beams_kernel(
    const int32_t* __restrict__ child, const float* __restrict__ node_box, const double* __restrict__ leaf_tri,
    const int32_t* __restrict__ leaf_face, int64_t n, const T* __restrict__ vps, const T* __restrict__ dirs, int64_t n_beams,
    const int64_t* __restrict__ scan_offset, const double* __restrict__ poses, int n_scans, BeamPattern pat, int log2s, double r0,
    double spread, const double* __restrict__ t_min_beam, double t_min, int cull, int weight_kind, int detection, double tau, int min_hits,
    int32_t* __restrict__ face_out, double* __restrict__ depth_out, int32_t* __restrict__ n_hits_out, int32_t* __restrict__ sub_face,
    double* __restrict__ sub_t, double* __restrict__ sub_w) {
  __shared__ int32_t stack[kBvhStackDepth * kCastBlock];
  const int lane = threadIdx.x;
  const int64_t g = (int64_t)blockIdx.x * kCastBlock + lane;
  const int S = 1 << log2s;
  const int64_t i = g >> log2s;
  const int j = (int)(g & (S - 1));
  const bool live = i < n_beams;                  // the other lanes are misses; they stay for the cross-lane part
  int32_t face = -1;
  double t = INFINITY, w = 0.0;
  if (live) {
    const double* M = poses + 16 * (int64_t)dc::scan_of(scan_offset, n_scans, i);
    const dc::BeamFrame f = dc::beam_frame((double)dirs[3 * i], (double)dirs[3 * i + 1], (double)dirs[3 * i + 2]);
    if (f.ok) {
      double o[3], D[3];
      dc::beam_subray(f, (double)vps[3 * i], (double)vps[3 * i + 1], (double)vps[3 * i + 2], pat.v[3 * j], pat.v[3 * j + 1], r0, spread, o,
                      D);
      double d0, d1, d2, o0, o1, o2;
      measured_ray(o, D, 0, M, d0, d1, d2, o0, o1, o2);
      const Hit best = cast_ray(child, node_box, leaf_tri, leaf_face, n, d0, d1, d2, o0, o1, o2, t_min_beam ? t_min_beam[i] : t_min, cull,
                                stack, lane);
      if (best.leaf >= 0) {
        w = pat.v[3 * j + 2];
        if (weight_kind == DC_BEAM_LAMBERT)           // 0 / 0 on a face of zero area: NaN, not a hit
          w *= fmin(1.0, incidence_cos(leaf_tri + 9 * (int64_t)best.leaf, d0, d1, d2));
        if (dc::beam_is_hit(best.face, w)) {
          face = best.face;
          t = best.t;
        } else {
          w = 0.0;
        }
      }
    }
    if (sub_face) {
      sub_face[g] = face;
      sub_t[g] = t;
      sub_w[g] = w;
    }
  }

  // ---- the bundle's reduction: every lane of the wavefront is here ----
  const int wl = lane & 63, base = wl & ~(S - 1);
  const uint64_t group = S == 64 ? ~0ull : ((1ull << S) - 1ull);
  const uint64_t hits = (__ballot(face >= 0) >> base) & group;
  const int n_hits = __popcll(hits);
  double total = 0.0, depth = INFINITY;
  if (detection == DC_BEAM_MEAN) {
    double swt = 0.0;
    for (int k = 0; k < S; ++k) {                     // ascending j, one term at a time
      const double tk = __shfl(t, base + k), wk = __shfl(w, base + k);
      if ((hits >> k) & 1ull) {
        total += wk;
        swt += wk * tk;
      }
    }
    depth = swt / total;
  } else {
    int rank = 0;                                     // place of this lane's hit in the order by (t, j)
    for (int k = 0; k < S; ++k) {
      const double tk = __shfl(t, base + k);
      rank += (((hits >> k) & 1ull) && dc::beam_before(tk, k, t, j)) ? 1 : 0;
    }
    int src = j;                                      // the sample at place j of that order
    for (int k = 0; k < S; ++k) {
      const int rk = __shfl(rank, base + k);
      if (((hits >> k) & 1ull) && rk == j) src = k;
    }
    const double ts = __shfl(t, base + src), ws = __shfl(w, base + src);
    double c = 0.0, cj = 0.0;                         // the running weight, added one at a time in that order: every lane of the beam
    for (int m = 0; m < S; ++m) {                     // forms the same sequence, lane j keeps c_j
      const double wm = __shfl(ws, base + m);
      if (m < n_hits) c += wm;
      if (m == j) cj = c;
    }
    total = c;
    const uint64_t reached = (__ballot(j < n_hits && dc::beam_reached(cj, tau, total)) >> base) & group;
    const int first = reached ? __ffsll((unsigned long long)reached) - 1 : 0;
    const double tq = __shfl(ts, base + first);
    if (reached) depth = tq;
  }
  const bool miss = dc::beam_is_miss(n_hits, min_hits, total);
  int best_k = -1;
  double best_dist = INFINITY;
  for (int k = 0; k < S; ++k) {
    const double tk = __shfl(t, base + k);
    if ((hits >> k) & 1ull) {
      const double dist = fabs(tk - depth);
      if (dc::beam_closer(dist, best_dist)) { best_dist = dist; best_k = k; }
    }
  }
  const int32_t fk = __shfl(face, base + (best_k >= 0 ? best_k : 0));
  if (live && j == 0) {
    const bool ok = !miss && best_k >= 0;
    face_out[i] = ok ? fk : -1;
    depth_out[i] = ok ? depth : INFINITY;
    n_hits_out[i] = n_hits;
  }
}

// The ray of a moving sweep in the start frame of its scan (dc_sweepmath.h): origin D(tau) vp, direction Exp(tau w) dir.  The scan is
// found as in raycast_rays_kernel; tw is its row of twists (v, w), tg the ray's sweep time.
template <typename T>
__device__ __forceinline__ int sweep_ray(const T* __restrict__ vps, const T* __restrict__ dirs, double tg, int64_t g,
                                         const int64_t* __restrict__ scan_offset, const double* __restrict__ twists, int n_scans, double* o,
                                         double* D) {
  const int lo = dc::scan_of(scan_offset, n_scans, g);
  const double* tw = twists + 6 * (int64_t)lo;
  const dc::SweepRot r = dc::sweep_rot(tg, tw[3], tw[4], tw[5]);
  dc::sweep_point(r, tg, tw[0], tw[1], tw[2], (double)vps[3 * g], (double)vps[3 * g + 1], (double)vps[3 * g + 2], o);
  dc::sweep_rotate(r, (double)dirs[3 * g], (double)dirs[3 * g + 1], (double)dirs[3 * g + 2], D);
  return lo;
}

template <typename T>
__global__ void __launch_bounds__(kBuildBlock) sweep_rays_kernel(const T* __restrict__ vps, const T* __restrict__ dirs,
                                                                 const double* __restrict__ tau, int64_t total,
                                                                 const int64_t* __restrict__ scan_offset, const double* __restrict__ twists,
                                                                 int n_scans, double* __restrict__ origins_out, double* __restrict__ dirs_out) {
  const int64_t g = (int64_t)blockIdx.x * kBuildBlock + threadIdx.x;
  if (g >= total) return;
  double o[3], D[3];
  sweep_ray(vps, dirs, tau[g], g, scan_offset, twists, n_scans, o, D);
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    origins_out[3 * g + a] = o[a];
    dirs_out[3 * g + a] = D[a];
  }
}

// dc_raycast_sweep: sweep_ray, then raycast_rays_kernel's body on that ray.  A ray whose tau is not finite is a miss without a cast
// (its ray is NaN, which cast_ray would carry through every box of the tree to the same miss).
template <typename T>
__global__ void __launch_bounds__(kCastBlock) raycast_sweep_kernel(const int32_t* __restrict__ child, const float* __restrict__ node_box,
                                                                   const double* __restrict__ leaf_tri, const int32_t* __restrict__ leaf_face,
                                                                   int64_t n, const T* __restrict__ vps, const T* __restrict__ dirs,
                                                                   const double* __restrict__ tau, int64_t total,
                                                                   const int64_t* __restrict__ scan_offset, const double* __restrict__ poses,
                                                                   const double* __restrict__ twists, int n_scans,
                                                                   const double* __restrict__ t_min_ray, double t_min, int cull,
                                                                   int32_t* __restrict__ face_out, double* __restrict__ t_out,
                                                                   double* __restrict__ inc_out) {
  __shared__ int32_t stack[kBvhStackDepth * kCastBlock];
  const int lane = threadIdx.x;
  const int64_t g = (int64_t)blockIdx.x * kCastBlock + lane;
  if (g >= total) return;
  int32_t face = -1;
  double t = INFINITY, inc = NAN;
  const double tg = tau[g];
  if (isfinite(tg)) {
    double o[3], D[3];
    const int s = sweep_ray(vps, dirs, tg, g, scan_offset, twists, n_scans, o, D);
    double d0, d1, d2, o0, o1, o2;
    measured_ray(o, D, 0, poses + 16 * (int64_t)s, d0, d1, d2, o0, o1, o2);
    const Hit best = cast_ray(child, node_box, leaf_tri, leaf_face, n, d0, d1, d2, o0, o1, o2, t_min_ray ? t_min_ray[g] : t_min, cull, stack,
                              lane);
    face = best.face;
    t = best.t;
    if (best.leaf >= 0) inc = acos(fmin(1.0, incidence_cos(leaf_tri + 9 * (int64_t)best.leaf, d0, d1, d2)));   // zero area: NaN
  }
  face_out[g] = face;
  t_out[g] = t;
  inc_out[g] = inc;
}

// ---- surfels: a surveyed cloud as oriented disks (dc_surfelmath.h) ------------------------------------------------------------------
using dc::SurfelBlend;
using dc::SurfelHit;
using dc::SurfelRay;
using dc::kDiskRow;

__global__ void __launch_bounds__(kBuildBlock) surfel_morton_kernel(const double* __restrict__ points, int64_t n, SceneBox box,
                                                                    uint64_t* __restrict__ keys, uint32_t* __restrict__ vals) {
  const int64_t i = (int64_t)blockIdx.x * kBuildBlock + threadIdx.x;
  if (i >= n) return;
  morton_key(points + 3 * i, box, i, keys, vals);
}

// fit_kernel with disk_box at the leaves; leaf i also writes its disk's row of leaf_disk
__global__ void __launch_bounds__(kBuildBlock) surfel_fit_kernel(const double* __restrict__ points, const double* __restrict__ normals,
                                                                 const double* __restrict__ radii, int64_t n,
                                                                 const int32_t* __restrict__ leaf_index, const int32_t* __restrict__ child,
                                                                 const int32_t* __restrict__ parent, int32_t* __restrict__ counter,
                                                                 float* node_box, double* __restrict__ leaf_disk) {
  const int64_t i = (int64_t)blockIdx.x * kBuildBlock + threadIdx.x;
  if (i >= n) return;
  const int64_t s = leaf_index[i];
  double p[3], nv[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    p[a] = points[3 * s + a];
    nv[a] = normals[3 * s + a];
  }
  const double rho = radii[s];
  double* row = leaf_disk + kDiskRow * i;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    row[a] = p[a];
    row[3 + a] = nv[a];
  }
  row[6] = rho * rho;
  row[7] = 0.0;
  dc::disk_box(p, nv, rho, node_box + 6 * ((n - 1) + i));
  dc::bvh_fit_climb((n - 1) + i, child, parent, counter, node_box);
}

// One pass of dc_surfel_cast_rays over the tree of disks (dc::DiskVisitor: the closest hit, or the blend behind it up to t_end)
template <bool kBlend>
__device__ __forceinline__ void surfel_walk(const int32_t* __restrict__ child, const float* __restrict__ node_box,
                                            const double* __restrict__ leaf_disk, const int32_t* __restrict__ leaf_index, int64_t n,
                                            const SurfelRay& sr, const Ray32& ray, double tmin, SurfelHit& best, double t_end, double min_cos,
                                            SurfelBlend& blend, int32_t* stack, int lane) {
  dc::DiskVisitor<kBlend> vis = {node_box, leaf_disk, leaf_index, sr, ray, tmin, t_end, min_cos, best, blend};
  dc::bvh_walk<kCastBlock>(child, n, stack, lane, vis);
}

// dc_surfel_cast_rays: the ray of raycast_rays_kernel, the closest disk, then (window > 0) the blend over the disks behind it
template <typename T>
__global__ void __launch_bounds__(kCastBlock) surfel_cast_kernel(const int32_t* __restrict__ child, const float* __restrict__ node_box,
                                                                 const double* __restrict__ leaf_disk, const int32_t* __restrict__ leaf_index,
                                                                 int64_t n, const T* __restrict__ vps, const T* __restrict__ dirs,
                                                                 int64_t total, const int64_t* __restrict__ scan_offset,
                                                                 const double* __restrict__ poses, int n_scans, double t_min, double window,
                                                                 double min_cos, int32_t* __restrict__ index_out,
                                                                 double* __restrict__ t_first_out, double* __restrict__ t_out,
                                                                 double* __restrict__ inc_out, int32_t* __restrict__ count_out) {
  __shared__ int32_t stack[kBvhStackDepth * kCastBlock];
  const int lane = threadIdx.x;
  const int64_t g = (int64_t)blockIdx.x * kCastBlock + lane;
  if (g >= total) return;
  SurfelRay sr;
  measured_ray(vps, dirs, g, poses + 16 * (int64_t)dc::scan_of(scan_offset, n_scans, g), sr.d0, sr.d1, sr.d2, sr.o0, sr.o1, sr.o2);
  Ray64 ray64;
  Ray32 ray;
  dc::ray_setup(sr.d0, sr.d1, sr.d2, sr.o0, sr.o1, sr.o2, ray64, ray);
  SurfelHit best = dc::no_surfel_hit();
  SurfelBlend blend;
  dc::blend_init(blend);
  surfel_walk<false>(child, node_box, leaf_disk, leaf_index, n, sr, ray, t_min, best, 0.0, 0.0, blend, stack, lane);
  if (best.leaf >= 0 && window > 0.0)
    surfel_walk<true>(child, node_box, leaf_disk, leaf_index, n, sr, ray, t_min, best, best.t + window, min_cos, blend, stack, lane);
  double t, inc;
  int32_t count;
  dc::surfel_finish(best, leaf_disk + kDiskRow * (int64_t)(best.leaf >= 0 ? best.leaf : 0), blend, sr, t, inc, count);
  index_out[g] = best.index;
  t_first_out[g] = best.t;
  t_out[g] = t;
  inc_out[g] = inc;
  count_out[g] = count;
}

// the checks dc_beam_subrays and dc_raycast_beams share; fills `pat`
inline bool beam_pattern_ok(const double* pattern, int n_samples, double r0, double spread, BeamPattern* pat) {
  if (!pattern || n_samples < 1 || n_samples > DC_BEAM_MAX_SAMPLES) return false;
  if (!(r0 >= 0.0) || !(spread >= 0.0) || !std::isfinite(r0) || !std::isfinite(spread)) return false;
  for (int k = 0; k < 3 * DC_BEAM_MAX_SAMPLES; ++k) pat->v[k] = 0.0;
  for (int k = 0; k < 3 * n_samples; ++k) {
    if (!std::isfinite(pattern[k]) || (k % 3 == 2 && pattern[k] < 0.0)) return false;
    pat->v[k] = pattern[k];
  }
  return true;
}

inline unsigned grid_of(int64_t n, int block) { return (unsigned)((n + block - 1) / block); }

// What dc_bvh_build and dc_surfel_bvh_build share between argument check and fit kernel: scene box, workspace, the Morton keys
// (`morton` launches the kernel that writes them), the sort into leaf_prim and the Karras tree.  *counter: the fit's zeroed counters.
template <typename Morton>
int build_tree(int64_t n, const double* scene_box, int32_t* leaf_prim, int32_t* child, int32_t* parent, void* ws, hipStream_t stream,
               int32_t** counter, Morton morton) {
  SceneBox box;
  for (int a = 0; a < 3; ++a) {
    const double ext = scene_box[3 + a] - scene_box[a];
    if (!(ext >= 0.0)) return DC_ERR_ARG;
    box.lo[a] = scene_box[a];
    box.scale[a] = ext > 0.0 ? 1024.0 / ext : 0.0;
  }
  dc::Carver c(ws);
  uint64_t* keys_in = c.take<uint64_t>(n);
  uint64_t* keys_out = c.take<uint64_t>(n);
  uint32_t* vals_in = c.take<uint32_t>(n);
  *counter = c.take<int32_t>(n);
  const size_t sort_bytes = dc::sort_pairs_bytes((size_t)n, 64);
  void* sort_tmp = c.take<char>(sort_bytes);
  DC_HIP(hipMemsetAsync(parent, 0xff, sizeof(int32_t), stream));                    // the root has no parent
  DC_HIP(hipMemsetAsync(*counter, 0, sizeof(int32_t) * n, stream));
  morton(box, keys_in, vals_in);
  DC_HIP(hipGetLastError());
  DC_HIP(dc::sort_pairs_u64(sort_tmp, sort_bytes, keys_in, keys_out, vals_in, leaf_prim, (size_t)n, 0, 62, stream));
  if (n > 1) {
    karras_kernel<<<grid_of(n - 1, kBuildBlock), kBuildBlock, 0, stream>>>(keys_out, n, child, parent);
    DC_HIP(hipGetLastError());
  }
  return DC_OK;
}

}  // namespace

extern "C" {

size_t dc_bvh_workspace_bytes(int64_t n_faces) {
  if (n_faces < 1) return 0;
  dc::Carver c(nullptr);
  c.take<uint64_t>(n_faces);
  c.take<uint64_t>(n_faces);
  c.take<uint32_t>(n_faces);
  c.take<int32_t>(n_faces);
  c.take<char>(dc::sort_pairs_bytes((size_t)n_faces, 64));
  return c.off + 256;
}

int dc_bvh_build(const double* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, const double* scene_box, int32_t* leaf_face,
                 int32_t* child, int32_t* parent, float* node_box, double* leaf_tri, void* ws, size_t ws_bytes, dcStream_t stream_) {
  if (n_faces < 1 || n_faces > (int64_t)INT32_MAX / 2 || n_verts < 1 || !verts || !faces || !scene_box || !leaf_face ||
      (n_faces > 1 && !child) || !parent || !node_box || !leaf_tri)       // one face: the root is a leaf and child has no rows
    return DC_ERR_ARG;
  if (!ws || ws_bytes < dc_bvh_workspace_bytes(n_faces)) return DC_ERR_WORKSPACE;
  hipStream_t stream = (hipStream_t)stream_;
  int32_t* counter;
  const int rc = build_tree(n_faces, scene_box, leaf_face, child, parent, ws, stream, &counter,
                            [&](const SceneBox& box, uint64_t* keys, uint32_t* vals) {
                              morton_kernel<<<grid_of(n_faces, kBuildBlock), kBuildBlock, 0, stream>>>(verts, faces, n_faces, box, keys, vals);
                            });
  if (rc != DC_OK) return rc;
  fit_kernel<<<grid_of(n_faces, kBuildBlock), kBuildBlock, 0, stream>>>(verts, faces, n_faces, leaf_face, child, parent, counter, node_box,
                                                                       leaf_tri);
  DC_HIP(hipGetLastError());
  return DC_OK;
}

int dc_raycast(const int32_t* child, const float* node_box, const double* leaf_tri, const int32_t* leaf_face, int64_t n_faces,
               const double* dirs, const double* t_min, int64_t n_rays, const double* poses, int n_poses, int cull, int32_t* face_out,
               double* t_out, double* bary_out, dcStream_t stream) {
  if (n_faces < 1 || n_rays < 0 || n_poses < 0 || !node_box || !leaf_tri || !leaf_face || (n_faces > 1 && !child)) return DC_ERR_ARG;
  const int64_t total = n_rays * (int64_t)n_poses;
  if (total == 0) return DC_OK;
  if (!dirs || !t_min || !poses || !face_out || !t_out || !bary_out) return DC_ERR_ARG;
  raycast_kernel<<<grid_of(total, kCastBlock), kCastBlock, 0, (hipStream_t)stream>>>(child, node_box, leaf_tri, leaf_face, n_faces, dirs, t_min,
                                                                                    n_rays, poses, total, cull, face_out, t_out, bary_out);
  DC_HIP(hipGetLastError());
  return DC_OK;
}

int dc_raycast_rays(const int32_t* child, const float* node_box, const double* leaf_tri, const int32_t* leaf_face, int64_t n_faces,
                    const void* vps, const void* dirs, int dtype, int64_t n, const int64_t* scan_offset, const double* poses, int n_scans,
                    double t_min, int cull, int32_t* face_out, double* t_out, double* inc_out, dcStream_t stream) {
  if (n_faces < 1 || n < 0 || n_scans < 0 || !node_box || !leaf_tri || !leaf_face || (n_faces > 1 && !child) || !(t_min == t_min))
    return DC_ERR_ARG;
  if (dtype != DC_F32 && dtype != DC_F64) return DC_ERR_DTYPE;
  if (n == 0) return DC_OK;
  if (n_scans < 1 || !vps || !dirs || !scan_offset || !poses || !face_out || !t_out || !inc_out) return DC_ERR_ARG;
  if (dtype == DC_F32)
    raycast_rays_kernel<float><<<grid_of(n, kCastBlock), kCastBlock, 0, (hipStream_t)stream>>>(
        child, node_box, leaf_tri, leaf_face, n_faces, (const float*)vps, (const float*)dirs, n, scan_offset, poses, n_scans, t_min, cull,
        face_out, t_out, inc_out);
  else
    raycast_rays_kernel<double><<<grid_of(n, kCastBlock), kCastBlock, 0, (hipStream_t)stream>>>(
        child, node_box, leaf_tri, leaf_face, n_faces, (const double*)vps, (const double*)dirs, n, scan_offset, poses, n_scans, t_min, cull,
        face_out, t_out, inc_out);
  DC_HIP(hipGetLastError());
  return DC_OK;
}

int dc_beam_subrays(const void* vps, const void* dirs, int dtype, int64_t n, const double* pattern, int n_samples, double r0, double spread,
                    double* origins_out, double* dirs_out, dcStream_t stream) {
  BeamPattern pat;
  if (n < 0 || !beam_pattern_ok(pattern, n_samples, r0, spread, &pat)) return DC_ERR_ARG;
  if (dtype != DC_F32 && dtype != DC_F64) return DC_ERR_DTYPE;
  if (n == 0) return DC_OK;
  if (!vps || !dirs || !origins_out || !dirs_out || n > (int64_t)1 << 55) return DC_ERR_ARG;
  const int64_t total = n * n_samples;
  if (dtype == DC_F32)
    beam_subrays_kernel<float><<<grid_of(total, kBuildBlock), kBuildBlock, 0, (hipStream_t)stream>>>(
        (const float*)vps, (const float*)dirs, total, pat, n_samples, r0, spread, origins_out, dirs_out);
  else
    beam_subrays_kernel<double><<<grid_of(total, kBuildBlock), kBuildBlock, 0, (hipStream_t)stream>>>(
        (const double*)vps, (const double*)dirs, total, pat, n_samples, r0, spread, origins_out, dirs_out);
  DC_HIP(hipGetLastError());
  return DC_OK;
}

int dc_raycast_beams(const int32_t* child, const float* node_box, const double* leaf_tri, const int32_t* leaf_face, int64_t n_faces,
                     const void* vps, const void* dirs, int dtype, int64_t n, const int64_t* scan_offset, const double* poses, int n_scans,
                     const double* pattern, int n_samples, double r0, double spread, const double* t_min_beam, double t_min, int cull,
                     int weight_kind, int detection, double tau, int min_hits, int32_t* face_out, double* depth_out, int32_t* n_hits_out,
                     int32_t* sub_face, double* sub_t, double* sub_w, dcStream_t stream) {
  if (n_faces < 1 || n < 0 || n_scans < 0 || !node_box || !leaf_tri || !leaf_face || (n_faces > 1 && !child) || !(t_min == t_min))
    return DC_ERR_ARG;
  BeamPattern pat;
  if (!beam_pattern_ok(pattern, n_samples, r0, spread, &pat) || (n_samples & (n_samples - 1)) != 0) return DC_ERR_ARG;
  if (!(tau > 0.0) || !(tau <= 1.0) || min_hits < 1 || min_hits > n_samples) return DC_ERR_ARG;
  if ((weight_kind != DC_BEAM_UNIFORM && weight_kind != DC_BEAM_LAMBERT) || (detection != DC_BEAM_MEAN && detection != DC_BEAM_QUANTILE))
    return DC_ERR_ARG;
  if (dtype != DC_F32 && dtype != DC_F64) return DC_ERR_DTYPE;
  if (n == 0) return DC_OK;
  if (n_scans < 1 || !vps || !dirs || !scan_offset || !poses || !face_out || !depth_out || !n_hits_out || n > (int64_t)1 << 55)
    return DC_ERR_ARG;
  if (sub_face && (!sub_t || !sub_w)) return DC_ERR_ARG;
  int log2s = 0;
  while ((1 << log2s) < n_samples) ++log2s;
  const int64_t total = n * n_samples;
  if (dtype == DC_F32)
    raycast_beams_kernel<float><<<grid_of(total, kCastBlock), kCastBlock, 0, (hipStream_t)stream>>>(
        child, node_box, leaf_tri, leaf_face, n_faces, (const float*)vps, (const float*)dirs, n, scan_offset, poses, n_scans, pat, log2s, r0,
        spread, t_min_beam, t_min, cull, weight_kind, detection, tau, min_hits, face_out, depth_out, n_hits_out, sub_face, sub_t, sub_w);
  else
    raycast_beams_kernel<double><<<grid_of(total, kCastBlock), kCastBlock, 0, (hipStream_t)stream>>>(
        child, node_box, leaf_tri, leaf_face, n_faces, (const double*)vps, (const double*)dirs, n, scan_offset, poses, n_scans, pat, log2s,
        r0, spread, t_min_beam, t_min, cull, weight_kind, detection, tau, min_hits, face_out, depth_out, n_hits_out, sub_face, sub_t, sub_w);
  DC_HIP(hipGetLastError());
  return DC_OK;
}

int dc_sweep_rays(const void* vps, const void* dirs, int dtype, const double* tau, int64_t n, const int64_t* scan_offset, const double* twists,
                  int n_scans, double* origins_out, double* dirs_out, dcStream_t stream) {
  if (n < 0 || n_scans < 0) return DC_ERR_ARG;
  if (dtype != DC_F32 && dtype != DC_F64) return DC_ERR_DTYPE;
  if (n == 0) return DC_OK;
  if (n_scans < 1 || !vps || !dirs || !tau || !scan_offset || !twists || !origins_out || !dirs_out) return DC_ERR_ARG;
  if (dtype == DC_F32)
    sweep_rays_kernel<float><<<grid_of(n, kBuildBlock), kBuildBlock, 0, (hipStream_t)stream>>>(
        (const float*)vps, (const float*)dirs, tau, n, scan_offset, twists, n_scans, origins_out, dirs_out);
  else
    sweep_rays_kernel<double><<<grid_of(n, kBuildBlock), kBuildBlock, 0, (hipStream_t)stream>>>(
        (const double*)vps, (const double*)dirs, tau, n, scan_offset, twists, n_scans, origins_out, dirs_out);
  DC_HIP(hipGetLastError());
  return DC_OK;
}

int dc_raycast_sweep(const int32_t* child, const float* node_box, const double* leaf_tri, const int32_t* leaf_face, int64_t n_faces,
                     const void* vps, const void* dirs, int dtype, const double* tau, int64_t n, const int64_t* scan_offset,
                     const double* poses, const double* twists, int n_scans, const double* t_min_ray, double t_min, int cull,
                     int32_t* face_out, double* t_out, double* inc_out, dcStream_t stream) {
  if (n_faces < 1 || n < 0 || n_scans < 0 || !node_box || !leaf_tri || !leaf_face || (n_faces > 1 && !child) || !(t_min == t_min))
    return DC_ERR_ARG;
  if (dtype != DC_F32 && dtype != DC_F64) return DC_ERR_DTYPE;
  if (n == 0) return DC_OK;
  if (n_scans < 1 || !vps || !dirs || !tau || !scan_offset || !poses || !twists || !face_out || !t_out || !inc_out) return DC_ERR_ARG;
  if (dtype == DC_F32)
    raycast_sweep_kernel<float><<<grid_of(n, kCastBlock), kCastBlock, 0, (hipStream_t)stream>>>(
        child, node_box, leaf_tri, leaf_face, n_faces, (const float*)vps, (const float*)dirs, tau, n, scan_offset, poses, twists, n_scans,
        t_min_ray, t_min, cull, face_out, t_out, inc_out);
  else
    raycast_sweep_kernel<double><<<grid_of(n, kCastBlock), kCastBlock, 0, (hipStream_t)stream>>>(
        child, node_box, leaf_tri, leaf_face, n_faces, (const double*)vps, (const double*)dirs, tau, n, scan_offset, poses, twists, n_scans,
        t_min_ray, t_min, cull, face_out, t_out, inc_out);
  DC_HIP(hipGetLastError());
  return DC_OK;
}

size_t dc_surfel_bvh_workspace_bytes(int64_t n) { return dc_bvh_workspace_bytes(n); }

int dc_surfel_bvh_build(const double* points, const double* normals, const double* radii, int64_t n, const double* scene_box,
                        int32_t* leaf_index, int32_t* child, int32_t* parent, float* node_box, double* leaf_disk, void* ws, size_t ws_bytes,
                        dcStream_t stream_) {
  if (n < 1 || n > (int64_t)INT32_MAX / 2 || !points || !normals || !radii || !scene_box || !leaf_index || (n > 1 && !child) || !parent ||
      !node_box || !leaf_disk)                                              // one disk: the root is a leaf and child has no rows
    return DC_ERR_ARG;
  if (!ws || ws_bytes < dc_surfel_bvh_workspace_bytes(n)) return DC_ERR_WORKSPACE;
  hipStream_t stream = (hipStream_t)stream_;
  int32_t* counter;
  const int rc = build_tree(n, scene_box, leaf_index, child, parent, ws, stream, &counter,
                            [&](const SceneBox& box, uint64_t* keys, uint32_t* vals) {
                              surfel_morton_kernel<<<grid_of(n, kBuildBlock), kBuildBlock, 0, stream>>>(points, n, box, keys, vals);
                            });
  if (rc != DC_OK) return rc;
  surfel_fit_kernel<<<grid_of(n, kBuildBlock), kBuildBlock, 0, stream>>>(points, normals, radii, n, leaf_index, child, parent, counter,
                                                                        node_box, leaf_disk);
  DC_HIP(hipGetLastError());
  return DC_OK;
}

int dc_surfel_cast_rays(const int32_t* child, const float* node_box, const double* leaf_disk, const int32_t* leaf_index, int64_t n_disks,
                        const void* vps, const void* dirs, int dtype, int64_t n, const int64_t* scan_offset, const double* poses, int n_scans,
                        double t_min, double window, double min_cos, int32_t* index_out, double* t_first_out, double* t_out, double* inc_out,
                        int32_t* count_out, dcStream_t stream) {
  if (n_disks < 1 || n < 0 || n_scans < 0 || !node_box || !leaf_disk || !leaf_index || (n_disks > 1 && !child) || !(t_min == t_min) ||
      !(window >= 0.0) || !(min_cos >= 0.0) || !(min_cos < 1.0))
    return DC_ERR_ARG;
  if (dtype != DC_F32 && dtype != DC_F64) return DC_ERR_DTYPE;
  if (n == 0) return DC_OK;
  if (n_scans < 1 || !vps || !dirs || !scan_offset || !poses || !index_out || !t_first_out || !t_out || !inc_out || !count_out)
    return DC_ERR_ARG;
  if (dtype == DC_F32)
    surfel_cast_kernel<float><<<grid_of(n, kCastBlock), kCastBlock, 0, (hipStream_t)stream>>>(
        child, node_box, leaf_disk, leaf_index, n_disks, (const float*)vps, (const float*)dirs, n, scan_offset, poses, n_scans, t_min, window,
        min_cos, index_out, t_first_out, t_out, inc_out, count_out);
  else
    surfel_cast_kernel<double><<<grid_of(n, kCastBlock), kCastBlock, 0, (hipStream_t)stream>>>(
        child, node_box, leaf_disk, leaf_index, n_disks, (const double*)vps, (const double*)dirs, n, scan_offset, poses, n_scans, t_min,
        window, min_cos, index_out, t_first_out, t_out, inc_out, count_out);
  DC_HIP(hipGetLastError());
  return DC_OK;
}

}  // extern "C"
