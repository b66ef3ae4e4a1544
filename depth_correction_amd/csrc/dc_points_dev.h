// Device-side view of the per-point inputs of a sequence (local scans + poses + model) shared by the
// point, consistency and ICP kernels.
#pragma once
#include "dc_common.h"
#include "dc_device.h"
#include "dc_pointmath.h"

namespace dc {

struct PointInputs {
  const void* vps;        // [N,3]
  const void* dirs;       // [N,3]
  const void* depth;      // [N]
  const void* inc;        // [N]   (may be null when model kind is NONE)
  const uint8_t* lmask;   // [N]   (null = all true)
  const int32_t* scan_id; // [N]   (null = scan 0)
  const double* poses;    // [S,12] device, row-major [R|t] (null = identity)
  const double* w;        // [P] device
  const double* e;        // [P] device
  int model_kind, n_terms, n_scans;
  // [blocks, 2 n_scans + 1] or null: the points of every 256-point block are grouped -- those inside the loss mask first, by scan
  // id, then those outside it, by scan id (the plan ordered them so) -- and segment v of block b (v < S: inside, scan v; v >= S:
  // outside, scan v - S) is its lanes seg_start[b (2 S + 1) + v] .. seg_start[b (2 S + 1) + v + 1]  (reduce_pose_grads_grouped)
  const uint16_t* seg_start = nullptr;
};

__device__ __forceinline__ void load_model(const PointInputs& in, ModelParams& mp) {
  mp.kind = in.model_kind;
  mp.n_terms = in.n_terms;
#pragma unroll
  for (int k = 0; k < DC_MAX_MODEL_TERMS; ++k) {
    const bool on = k < in.n_terms && in.model_kind != DC_MODEL_NONE;
    mp.w[k] = on ? in.w[k] : 0.0;
    mp.e[k] = on ? in.e[k] : 0.0;
  }
}

// Poses of a sequence are read per LANE (a block of Morton-ordered points holds points of most scans).  Every block
// copies the (few) poses into LDS once, coalesced, and the lanes read them from there instead of gathering 12 doubles
// each from global memory (6 x 64 L1 tag lookups per wavefront).
constexpr int kLdsScans = 32;              // 3 KB; sequences with more scans read their poses from global memory

struct PoseTile {
  const double* lds;                       // staged poses, or nullptr: read from global memory
};

// Call from all threads of the block; the caller's next __syncthreads() publishes the tile.
__device__ __forceinline__ PoseTile stage_poses(const PointInputs& in, double* s_pose) {
  if (!in.poses || in.n_scans > kLdsScans) return PoseTile{nullptr};
  for (int t = threadIdx.x; t < in.n_scans * 12; t += blockDim.x) s_pose[t] = in.poses[t];
  return PoseTile{s_pose};
}

__device__ __forceinline__ void load_pose(const PointInputs& in, const PoseTile& tile, int s, double* T) {
  if (in.poses) {
    const double* p = (tile.lds ? tile.lds : in.poses) + (int64_t)s * 12;
#pragma unroll
    for (int q = 0; q < 12; ++q) T[q] = p[q];
  } else {
#pragma unroll
    for (int q = 0; q < 12; ++q) T[q] = (q == 0 || q == 5 || q == 10) ? 1.0 : 0.0;
  }
}

__device__ __forceinline__ void load_pose(const PointInputs& in, int s, double* T) { load_pose(in, PoseTile{nullptr}, s, T); }

// ------------------------------------------------------------------------------------------------
// Backward epilogue per point: dL/dx_j -> dL/dw, dL/dexponent, dL/d[R|t] of the point's scan.
// acc layout: [0,P) grad w, [P,2P) grad exponent, then 12 per-scan slots handled by the caller.
// ------------------------------------------------------------------------------------------------
// the per-point inputs of the epilogue in their storage type, so they can be requested early (before a gather loop)
template <typename T>
struct PointRaw {
  T dr[3], d, inc;
  bool lm;
  int s;
};
template <typename T>
__device__ __forceinline__ PointRaw<T> load_point_raw(const PointInputs& in, const ModelParams& mp, int64_t j) {
  PointRaw<T> r;
  const T* dirs = (const T*)in.dirs;
  r.dr[0] = dirs[j * 3]; r.dr[1] = dirs[j * 3 + 1]; r.dr[2] = dirs[j * 3 + 2];
  r.d = ((const T*)in.depth)[j];
  r.lm = in.lmask ? in.lmask[j] != 0 : true;
  r.s = in.scan_id ? in.scan_id[j] : 0;
  r.inc = (mp.kind != DC_MODEL_NONE) ? ((const T*)in.inc)[j] : (T)0;
  return r;
}

template <typename T>
__device__ __forceinline__ void points_bwd_point(const PointInputs& in, const PoseTile& poses, const ModelParams& mp, int64_t j,
                                                 const PointRaw<T>& raw, const double* g, double* gw, double* ge, double* gT,
                                                 bool want_e, bool want_pose, int* scan) {
  double vp[3], dr[3], T12[12];
  const QParams qp0{};
  if (in.vps) Row3<T, 3>::load((const T*)in.vps, j, vp, qp0);
  else { vp[0] = vp[1] = vp[2] = 0.0; }
  dr[0] = (double)raw.dr[0]; dr[1] = (double)raw.dr[1]; dr[2] = (double)raw.dr[2];
  const double d = (double)raw.d;
  const bool lm = raw.lm;
  const int s = raw.s;
  *scan = s;
  load_pose(in, poses, s, T12);
  // dL/dd' = (R dir) . g = dir . (R^T g)
  const double rg0 = T12[0] * g[0] + T12[4] * g[1] + T12[8] * g[2];
  const double rg1 = T12[1] * g[0] + T12[5] * g[1] + T12[9] * g[2];
  const double rg2 = T12[2] * g[0] + T12[6] * g[1] + T12[10] * g[2];
  const double gd = dr[0] * rg0 + dr[1] * rg1 + dr[2] * rg2;
  double dcorr = d;
  if (mp.kind > DC_MODEL_SCALED_POLYNOMIAL && lm) {          // Linear / InvCos / ScaledInvCos: no exponents
    const double inc = (double)raw.inc;
#pragma unroll
    for (int k = 0; k < 3; ++k)
      if (k < mp.n_terms) gw[k] += gd * model_dw_other(mp, k, d, inc);
    dcorr = model_depth(mp, d, inc, true);
  } else if (mp.kind != DC_MODEL_NONE && lm) {
    const double inc = (double)raw.inc;
    const double base = mp.kind == DC_MODEL_SCALED_POLYNOMIAL ? -d * gd : -gd;
    double bias = 0.0;
#pragma unroll
    for (int k = 0; k < DC_MAX_MODEL_TERMS; ++k) {
      if (k < mp.n_terms) {
        const double pk = pow_term(inc, mp.e[k]);
        bias += pk * mp.w[k];
        gw[k] += base * pk;
        if (want_e) ge[k] += (inc > 0.0) ? base * mp.w[k] * pk * log(inc) : 0.0;
      }
    }
    dcorr = mp.kind == DC_MODEL_SCALED_POLYNOMIAL ? d * (1.0 - bias) : d - bias;
  }
  if (want_pose) {
    // x = R xl + t, xl = vps + d' dirs:  dL/dR = g xl^T, dL/dt = g
    const double xl0 = vp[0] + dcorr * dr[0], xl1 = vp[1] + dcorr * dr[1], xl2 = vp[2] + dcorr * dr[2];
    // kept factored (6 values, not 12) until the block reduction: gT = [g, xl], dL/d[R|t]_{a,b} = g_a * [xl, 1]_b
    gT[0] = g[0]; gT[1] = g[1]; gT[2] = g[2]; gT[3] = xl0; gT[4] = xl1; gT[5] = xl2;
  }
}

template <typename T>
__device__ __forceinline__ void points_bwd_point(const PointInputs& in, const PoseTile& poses, const ModelParams& mp, int64_t j,
                                                 const double* g, double* gw, double* ge, double* gT, bool want_e,
                                                 bool want_pose, int* scan) {
  points_bwd_point<T>(in, poses, mp, j, load_point_raw<T>(in, mp, j), g, gw, ge, gT, want_e, want_pose, scan);
}

// x = R (vp + d' dir) + t of one point from its raw inputs, vp [3] and the pose T12 of its scan: the statements of
// points_fwd_kernel, so that a kernel that forms the point itself (dc_mesh_loss) gets the point dc_points_fwd writes in fp64
template <typename T>
__device__ __forceinline__ void posed_point(const ModelParams& mp, const PointRaw<T>& raw, const double* vp, const double* T12, double* x) {
  double dr[3] = {(double)raw.dr[0], (double)raw.dr[1], (double)raw.dr[2]};
  const double dc_ = model_depth(mp, (double)raw.d, raw.lm ? (double)raw.inc : 0.0, raw.lm);
  double vr[3], drr[3];
  rot3(T12, vp, vr);
  vr[0] += T12[3]; vr[1] += T12[7]; vr[2] += T12[11];
  rot3(T12, dr, drr);
  x[0] = vr[0] + dc_ * drr[0]; x[1] = vr[1] + dc_ * drr[1]; x[2] = vr[2] + dc_ * drr[2];
}

}  // namespace dc
