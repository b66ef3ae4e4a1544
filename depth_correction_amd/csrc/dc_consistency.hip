// Map-consistency hot path kernels (gfx950): corrected points, neighbourhood features + loss forward,
// hand-derived backward.  C ABI at the bottom; declarations and reference citations in include/dc_hip.h.
//
// Data layout in HBM (all arrays owned by the caller, i.e. torch's allocator):
//   per point (SoA): vps[N,3], dirs[N,3], depth[N], inc[N] (T = f32|f64), lmask u8[N], scan_id i32[N]
//   points          x[N,S]  S = 3 (API layout) or 4 (padded: one 16-B gather per neighbour for f32 / q32);
//                   point format PT = f32 | f64 | q32 (DC_Q32: int32 fixed point, x = origin + q * scale)
//   neighbours      nbr i32[N,K] row major, -1 = missing
//   backward record rec[N,8] = {cmean.xyz, c1, v0.xyz, c2} in the point format (32 B: two 16-B loads per edge)
//   incoming edges  csr_ptr i32[N+1], csr_src i32[E]  (transpose of nbr, built once per neighbourhood set)
//   block tables    per 256-row block the distinct rows it references + u16 block-local positions, slot-major
//                   (dc_blocktab.hip): what the hot ("staged") kernels read instead of nbr / csr_*
// Arithmetic on chip is fp64 (differences against the centre point are exact, covariances and the eigen-solve
// keep LAPACK-level accuracy; the backward's per-edge term for q32 records is formed in fp32 from fp32-exact
// inputs); only storage is T.  No atomics: block partial sums are
// written to a workspace and reduced in a fixed order, so every result is bitwise reproducible.
#include <type_traits>
#include <atomic>
#include <mutex>
#include <cstdio>
#include <hip/hip_ext.h>
#include "dc_common.h"
#include "dc_device.h"
#include "dc_pointmath.h"
#include "dc_prof.h"
#include "dc_points_dev.h"
#include "dc_cons_route.h"
#include "../../include/dc_hip.h"

namespace dc {

// ------------------------------------------------------------------------------------------------
// K1+K2+K3: d' = model(d, inc) on masked points, (vps, dirs) -> pose frame, x = vps' + d' dirs'.
// ------------------------------------------------------------------------------------------------
template <typename T, typename PT, int STRIDE>
__global__ __launch_bounds__(kBlock) void points_fwd_kernel(PointInputs in, int64_t n, QParams qp, PT* __restrict__ x_out,
                                                            T* __restrict__ vps_out, T* __restrict__ dirs_out,
                                                            T* __restrict__ depth_out) {
  __shared__ double s_pose[kLdsScans * 12];
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int64_t ic = i < n ? i : n - 1;                                // lanes past the end read the last point, store nothing
  ModelParams mp;
  load_model(in, mp);
  // the point's own loads are issued (raw, unconverted: no wait yet) BEFORE the poses are staged, so the two global
  // round trips overlap
  T vp_r[3] = {T(0), T(0), T(0)}, dr_r[3];
  if (in.vps) { const T* q = (const T*)in.vps + ic * 3; vp_r[0] = q[0]; vp_r[1] = q[1]; vp_r[2] = q[2]; }   // NULL: sensor origin
  { const T* q = (const T*)in.dirs + ic * 3; dr_r[0] = q[0]; dr_r[1] = q[1]; dr_r[2] = q[2]; }
  const T d_r = ((const T*)in.depth)[ic];
  const bool lm = in.lmask ? in.lmask[ic] != 0 : true;
  const T inc_r = (mp.kind != DC_MODEL_NONE) ? ((const T*)in.inc)[ic] : T(0);
  const int sid = in.scan_id ? in.scan_id[ic] : 0;
  const PoseTile poses = stage_poses(in, s_pose);
  __syncthreads();
  if (i >= n) return;
  double vp[3] = {(double)vp_r[0], (double)vp_r[1], (double)vp_r[2]}, dr[3] = {(double)dr_r[0], (double)dr_r[1], (double)dr_r[2]};
  double T12[12];
  const double dc_ = model_depth(mp, (double)d_r, lm ? (double)inc_r : 0.0, lm);
  load_pose(in, poses, sid, T12);
  double vr[3], drr[3], x[3];
  rot3(T12, vp, vr);
  vr[0] += T12[3]; vr[1] += T12[7]; vr[2] += T12[11];
  rot3(T12, dr, drr);
  x[0] = vr[0] + dc_ * drr[0]; x[1] = vr[1] + dc_ * drr[1]; x[2] = vr[2] + dc_ * drr[2];
  Row3<PT, STRIDE>::store(x_out, i, x, qp);
  if (vps_out) Row3<T, 3>::store(vps_out, i, vr, qp);
  if (dirs_out) Row3<T, 3>::store(dirs_out, i, drr, qp);
  if (depth_out) depth_out[i] = (T)dc_;
}

// Everything of the forward after the neighbourhood moments are gathered: covariance -> smallest eigenpair -> loss,
// backward record, masked loss / count of this lane (acc2).  Shared by the gather and the LDS-staged kernel.
template <typename T, typename PT, bool FULL_EIG>
__device__ __forceinline__ void consistency_point(CovAcc& acc, const typename Pt<PT>::Raw& ci, int64_t i,
                                                  const uint8_t* __restrict__ mask, const T* __restrict__ offset,
                                                  const LossParams& lp, const QParams& qp, PT* __restrict__ rec,
                                                  T* __restrict__ pointwise, T* __restrict__ eigvals, double* acc2) {
  cov_same_weights(acc);
  // moments are in raw units (q32: multiples of the resolution); scale once
  const double u = Pt<PT>::unit(qp), u2 = u * u;
  double moff[3], cm[3], C[6], D, omega;
  cov_finish(acc, 0.0, moff, cm, C, &D, &omega, u2);
  const bool m = mask ? mask[i] != 0 : true;
  const double off = offset ? (double)offset[i] : 0.0;
  double lam0, v0[3], tr, c1, c2, l;
  if (FULL_EIG) {
    double lam[3], V[3][3];
    eig3_sym<double>(C[0], C[1], C[2], C[3], C[4], C[5], lam, V);
    lam0 = lam[0]; v0[0] = V[0][0]; v0[1] = V[0][1]; v0[2] = V[0][2];
    tr = lam[0] + lam[1] + lam[2];
    eigvals[i * 3] = (T)lam[0]; eigvals[i * 3 + 1] = (T)lam[1]; eigvals[i * 3 + 2] = (T)lam[2];
  } else {
    eig3_smallest(C[0], C[1], C[2], C[3], C[4], C[5], &lam0, v0, &tr);
  }
  double raw;
  l = loss_and_coeffs(lp, lam0, tr, D, off, m, &c1, &c2, &raw);
  const bool drop = loss_dropped(lp, l);
  if (drop) c1 = c2 = 0.0;
  if (m && !drop) { acc2[0] = l; acc2[1] = 1.0; }
  // record: covariance mean in the point format; coefficients act on differences in metres
  if (rec) RecRaw<PT>::store(rec, i, Pt<PT>::offset(ci, cm), c1, v0, c2);
  if (pointwise) pointwise[i] = (T)(lp.raw_pointwise ? raw : l);
}

// ------------------------------------------------------------------------------------------------
// Hot-path forward: neighbourhood covariance -> smallest eigenpair -> pointwise loss + backward
// record; block partial sums of (masked loss, mask count).
// ------------------------------------------------------------------------------------------------
template <typename T, typename PT, int STRIDE, bool FULL_EIG>
__global__ __launch_bounds__(kBlock) void consistency_fwd_kernel(
    const PT* __restrict__ x, const int32_t* __restrict__ nbr, const int32_t* __restrict__ centre_idx, int64_t n, int k,
    const uint8_t* __restrict__ mask,
    const T* __restrict__ offset, LossParams lp, QParams qp, PT* __restrict__ rec, T* __restrict__ pointwise,
    T* __restrict__ eigvals, double* __restrict__ partials) {
  const int64_t nblocks = (n + kBlock - 1) / kBlock;
  const int64_t blk = xcd_block(nblocks);
  double acc2[2] = {0.0, 0.0};
  if (blk >= 0) {
    const int64_t i = blk * kBlock + threadIdx.x;          // row of nbr / rec / pointwise
    if (i < n) {
      // with a centre list only the listed points are centres (e.g. the masked ones); rows stay compact
      const int64_t ip = centre_idx ? (int64_t)centre_idx[i] : i;
      const typename Pt<PT>::Raw ci = Pt<PT>::template load<STRIDE>(x, ip, qp);
      CovAcc acc;
      cov_init(acc);
      const int32_t* row = nbr + i * k;
      for (int q0 = 0; q0 < k; q0 += 4) {
        // four independent gathers in flight per trip (a missing neighbour re-reads the centre row: always valid)
        int32_t j[4];
        typename Pt<PT>::Raw cj[4];
#pragma unroll
        for (int u_ = 0; u_ < 4; ++u_) j[u_] = (q0 + u_ < k) ? row[q0 + u_] : -1;
#pragma unroll
        for (int u_ = 0; u_ < 4; ++u_) cj[u_] = Pt<PT>::template load<STRIDE>(x, j[u_] >= 0 ? (int64_t)j[u_] : ip, qp);
#pragma unroll
        for (int u_ = 0; u_ < 4; ++u_) {
          // a missing neighbour re-read the centre row: its difference is exactly zero, only the count is masked
          double d[3];
          Pt<PT>::delta(cj[u_], ci, d);
          cov_add1(acc, d[0], d[1], d[2]);
          acc.W -= (j[u_] >= 0) ? 0.0 : 1.0;
        }
      }
      consistency_point<T, PT, FULL_EIG>(acc, ci, i, mask, offset, lp, qp, rec, pointwise, eigvals, acc2);
    }
  }
  wave_partials<2>(acc2, partials);
}

// (the backward epilogue per point, points_bwd_point, lives in dc_points_dev.h: dc_meshloss.hip runs it too)

// Per-scan sums of the 12 pose-gradient values g_a * [xl, 1]_b of the 256 points of a block (gx = [g, xl] of this
// lane; pcol0 = first pose slot of this block's partial column).  The lanes are counting-sorted by scan id (wave ballots + a tiny prefix), staged in LDS in that
// order (14 KB) and every (scan, value) pair is summed by one thread over its contiguous segment: ~25 additions per pair
// instead of a 256-lane tree per scan, and a fixed order (wave, lane) => bitwise reproducible.  Scans absent from the
// block keep the zeros the caller put into the workspace.
constexpr int kPoseRow = 7;              // doubles per staged point: the factors [g, xl] + 1 pad (conflict-free 8-B LDS stores)
constexpr int kMaxBlockScans = 64;       // more distinct scans in one block: per-scan tree reduction instead

__device__ __forceinline__ void reduce_pose_grads(const PointInputs& in, bool active, const double* gx, int scan,
                                                  double* lds, double* __restrict__ pcol0, double* s_val) {
  constexpr int NW = kBlock / kWave;
  __shared__ int s_cnt[NW][kMaxBlockScans];
  __shared__ int s_start[kMaxBlockScans + 1];
  __shared__ int s_range[2];
  const int64_t rs = (int64_t)gridDim.x * kWavesPerBlock;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  if (tid == 0) { s_range[0] = 0x7fffffff; s_range[1] = -1; }
  __syncthreads();
  const bool ok = active && scan >= 0 && scan < in.n_scans;
  {
    // range of the scans present: wave-level min / max first, one LDS atomic per wavefront
    int lo = ok ? scan : 0x7fffffff, hi = ok ? scan : -1;
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) {
      lo = min(lo, __shfl_xor(lo, off, kWave));
      hi = max(hi, __shfl_xor(hi, off, kWave));
    }
    if (lane == 0 && hi >= 0) { atomicMin(&s_range[0], lo); atomicMax(&s_range[1], hi); }
  }
  __syncthreads();
  const int s_lo = s_range[0], s_hi = s_range[1];
  if (s_hi < s_lo) return;                                  // block-uniform: nothing to add
  const int ns = s_hi - s_lo + 1;
  if (ns > kMaxBlockScans) {
    for (int s = s_lo; s <= s_hi; ++s) {
      double t[12];
      const bool mine = ok && scan == s;
#pragma unroll
      for (int q = 0; q < 12; ++q) t[q] = mine ? gx[q >> 2] * ((q & 3) == 3 ? 1.0 : gx[3 + (q & 3)]) : 0.0;
      block_sum<12>(t, lds);
      if (tid == 0) {
#pragma unroll
        for (int q = 0; q < 12; ++q) pcol0[(s * 12 + q) * rs] = t[q];
      }
    }
    return;
  }
  const int r = ok ? scan - s_lo : -1;
  int rank_in_wave = 0;
  for (int q = 0; q < ns; ++q) {
    const unsigned long long m = __ballot(r == q);
    if (lane == 0) s_cnt[wave][q] = __popcll(m);
    if (r == q) rank_in_wave = __popcll(m & ((1ull << lane) - 1ull));
  }
  __syncthreads();
  if (wave == 0) {
    // exclusive prefix of the per-scan totals over the (at most 64) scans of the range, inside one wavefront
    int tot = 0;
    if (lane < ns) {
#pragma unroll
      for (int w = 0; w < NW; ++w) tot += s_cnt[w][lane];
    }
    int incl = tot;
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
      const int up = __shfl_up(incl, off, kWave);
      if (lane >= off) incl += up;
    }
    if (lane < ns) s_start[lane] = incl - tot;
    if (lane == ns - 1) s_start[ns] = incl;                 // number of contributing lanes
  }
  __syncthreads();
  if (ok) {
    int pos = s_start[r] + rank_in_wave;
    for (int w = 0; w < wave; ++w) pos += s_cnt[w][r];
#pragma unroll
    for (int q = 0; q < 6; ++q) s_val[pos * kPoseRow + q] = gx[q];
  }
  __syncthreads();
  // the 12 products g_a * [xl, 1]_b are formed while summing (each rounded, then added: no contraction, so the sums do
  // not depend on how many factors were staged)
  // Two lanes per (scan, entry): even / odd elements of the segment, four independent partial sums each so that the LDS
  // reads pipeline (a single running sum made this loop a chain of ~100 dependent LDS round trips per block).
  for (int item = tid; item < ns * 24; item += kBlock) {
    const int pair = item >> 1, part = item & 1;
    const int rr = pair / 12, q = pair - rr * 12, a = q >> 2, b = q & 3;
    const int beg = s_start[rr] + part, end = s_start[rr + 1];
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    int p = beg;
    for (; p + 6 < end; p += 8) {
#pragma unroll
      for (int u_ = 0; u_ < 4; ++u_) {
        const double ga = s_val[(p + 2 * u_) * kPoseRow + a];
        acc[u_] = __dadd_rn(acc[u_], b == 3 ? ga : __dmul_rn(ga, s_val[(p + 2 * u_) * kPoseRow + 3 + b]));
      }
    }
    for (; p < end; p += 2) {
      const double ga = s_val[p * kPoseRow + a];
      acc[0] = __dadd_rn(acc[0], b == 3 ? ga : __dmul_rn(ga, s_val[p * kPoseRow + 3 + b]));
    }
    double sum = __dadd_rn(__dadd_rn(acc[0], acc[1]), __dadd_rn(acc[2], acc[3]));
    sum = __dadd_rn(sum, __shfl_xor(sum, 1, kWave));         // even + odd half (the two lanes are neighbours)
    if (part == 0) pcol0[((s_lo + rr) * 12 + q) * rs] = sum;
  }
}

// The same sums when the plan has grouped the points of every block by scan id (PointInputs.seg_start; round 4): the segments
// are contiguous lane ranges known since set-up, so nothing is counted, ranked or sorted at run time, and NO BARRIER is left
// at the block's tail.  Every wavefront sums its own 64 lanes: the six factors go to its part of an LDS array where they stand,
// (scan, entry, half) items of the two to four scans its lanes belong to walk their stretch of the segment, and the sums go to
// the wavefront's row of s_part.  A ticket in LDS tells the wavefront that finishes last to add the four rows in fixed order
// (bitwise reproducible) and to store the block's 12 S sums as ONE contiguous row of the row-major pose partials
// [blocks][12 S]; the others have long retired.  Before: a counting sort of the block's lanes by scan -- three more barriers,
// a ballot loop over the scans, a prefix pass -- one running block-wide barrier before the sums, 12 S pieces of 32 B stored to
// as many pages per block, and a 30 MB memset of the pose columns per evaluation (113 us at C2, 65 % of the wave cycles
// waiting).
constexpr int kTicketScans = 16;          // the four partial rows cost 96 B of LDS per scan: sequences of up to 16 scans take the ticket form
// (module-scope LDS word: the backward kernels zero it before their staging barrier, pose_ticket_init)
__shared__ int s_pose_ticket;
__device__ __forceinline__ void pose_ticket_init() { if (threadIdx.x == 0) s_pose_ticket = 0; }
__device__ __forceinline__ void reduce_pose_grads_grouped(const PointInputs& in, int64_t blk, bool active, const double* gx,
                                                          int scan, double* __restrict__ prow, double* s_val) {
  constexpr int NW = kBlock / kWave;
  __shared__ double s_part[NW][12 * kTicketScans];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int S = in.n_scans, V = 2 * S;                      // V segments per block: (inside the loss mask, scan) then (outside, scan)
  if (blk < 0) {                                            // padding block of the last round: its row holds zeros
    for (int item = tid; item < S * 12; item += kBlock) prow[item] = 0.0;
    return;
  }
  const uint16_t* seg = in.seg_start + blk * (V + 1);
  // the segments that reach into this wavefront's 64 lanes: lane v < V looks at segment v
  const int w_beg = wave * kWave, w_end = w_beg + kWave;
  int sb_l = 0, se_l = 0;
  if (lane < V) { sb_l = seg[lane]; se_l = seg[lane + 1]; }
  const unsigned long long present = __ballot(lane < V && sb_l < w_end && se_l > w_beg && se_l > sb_l);
  const int v_lo = present ? __builtin_ctzll(present) : 0, v_hi = present ? 63 - __builtin_clzll(present) : -1;
  const int n_items = (v_hi - v_lo + 1) * 24;
  for (int item = lane; item < S * 12; item += kWave) s_part[wave][item] = 0.0;
#pragma unroll
  for (int q = 0; q < 6; ++q) s_val[tid * kPoseRow + q] = active ? gx[q] : 0.0;
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");     // own lanes' values: the wavefront's LDS operations are in order
  __builtin_amdgcn_wave_barrier();
  for (int item0 = 0; item0 < n_items; item0 += kWave) {
    const int item = item0 + lane;
    const int pair = item >> 1, part = item & 1;
    const int rs_ = pair / 12, q = pair - rs_ * 12, a = q >> 2, b = q & 3;
    const int v = min(v_lo + rs_, V - 1);
    // (the shuffles run with every lane active: a masked-off source lane would hand back zero)
    const int sb = __shfl(sb_l, v, kWave), se = __shfl(se_l, v, kWave);
    if (item >= n_items) continue;
    const int beg = max(sb, w_beg) + part, end = min(se, w_end);
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    int p = beg;
    for (; p + 6 < end; p += 8) {
#pragma unroll
      for (int u_ = 0; u_ < 4; ++u_) {
        const double ga = s_val[(p + 2 * u_) * kPoseRow + a];
        acc[u_] = __dadd_rn(acc[u_], b == 3 ? ga : __dmul_rn(ga, s_val[(p + 2 * u_) * kPoseRow + 3 + b]));
      }
    }
    for (; p < end; p += 2) {
      const double ga = s_val[p * kPoseRow + a];
      acc[0] = __dadd_rn(acc[0], b == 3 ? ga : __dmul_rn(ga, s_val[p * kPoseRow + 3 + b]));
    }
    double sum = __dadd_rn(__dadd_rn(acc[0], acc[1]), __dadd_rn(acc[2], acc[3]));
    sum = __dadd_rn(sum, __shfl_xor(sum, 1, kWave));         // even + odd half (the two lanes are neighbours)
    // the two segments of a scan (inside / outside the mask) can both reach into one wavefront: an add, not a store (two
    // addends on a zeroed slot: the same sum in either order)
    if (part == 0) atomicAdd(&s_part[wave][(v >= S ? v - S : v) * 12 + q], sum);
  }
  // ticket: the wavefront that arrives last adds the rows up and stores the block's row
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  int old = 0;
  if (lane == 0) old = atomicAdd(&s_pose_ticket, 1);
  old = __builtin_amdgcn_readfirstlane(old);
  if (old != NW - 1) return;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  for (int item = lane; item < S * 12; item += kWave) {
    double t = s_part[0][item];
#pragma unroll
    for (int w = 1; w < NW; ++w) t = __dadd_rn(t, s_part[w][item]);
    prow[item] = t;
  }
}

// Sequences of 17 .. 64 scans: the same static segments, summed by the whole block behind one barrier (the partial rows of the
// ticket form would take 24 KB of LDS).
__device__ __forceinline__ void reduce_pose_grads_grouped_wide(const PointInputs& in, int64_t blk, bool active, const double* gx,
                                                               double* __restrict__ prow, double* s_val) {
  const int tid = threadIdx.x;
  const int S = in.n_scans, V = 2 * S;
  if (blk < 0) {
    for (int item = tid; item < S * 12; item += kBlock) prow[item] = 0.0;
    return;
  }
  const uint16_t* seg = in.seg_start + blk * (V + 1);
#pragma unroll
  for (int q = 0; q < 6; ++q) s_val[tid * kPoseRow + q] = active ? gx[q] : 0.0;
  __syncthreads();
  for (int item = tid; item < S * 24; item += kBlock) {
    const int pair = item >> 1, part = item & 1;
    const int rr = pair / 12, q = pair - rr * 12, a = q >> 2, b = q & 3;
    double sum = 0.0;
    for (int half = 0; half < 2; ++half) {                  // the scan's points inside the loss mask, then those outside
      const int beg = (int)seg[rr + half * S] + part, end = (int)seg[rr + half * S + 1];
      double acc[4] = {0.0, 0.0, 0.0, 0.0};
      int p = beg;
      for (; p + 6 < end; p += 8) {
#pragma unroll
        for (int u_ = 0; u_ < 4; ++u_) {
          const double ga = s_val[(p + 2 * u_) * kPoseRow + a];
          acc[u_] = __dadd_rn(acc[u_], b == 3 ? ga : __dmul_rn(ga, s_val[(p + 2 * u_) * kPoseRow + 3 + b]));
        }
      }
      for (; p < end; p += 2) {
        const double ga = s_val[p * kPoseRow + a];
        acc[0] = __dadd_rn(acc[0], b == 3 ? ga : __dmul_rn(ga, s_val[p * kPoseRow + 3 + b]));
      }
      sum = __dadd_rn(sum, __dadd_rn(__dadd_rn(acc[0], acc[1]), __dadd_rn(acc[2], acc[3])));
    }
    sum = __dadd_rn(sum, __shfl_xor(sum, 1, kWave));
    if (part == 0) prow[pair] = sum;
  }
}

// Parameter gradients of one block into the partial rows of its wavefronts (row = 4 * block + wave; no LDS, no barrier:
// every wavefront leaves as soon as its lane 0 has written its sums):
//   [0,P) w, [P,2P) exponent, [2P, 2P + 12 S) poses.  Only the slots in use are reduced.  The pose slots are summed per
// block (counting sort by scan in LDS) into the row of the block's first wavefront; the others keep the caller's zeros.
template <typename T>
__device__ __forceinline__ void reduce_param_grads(const PointInputs& in, bool active, bool want_e, bool want_pose,
                                                   double* gw, double* ge, double* gT, int scan, double* lds,
                                                   double* __restrict__ partials, int64_t blk = -2) {
  const int64_t rs = (int64_t)gridDim.x * kWavesPerBlock;              // slot a lives at partials[a * rs + row]
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  double* prow = partials + (int64_t)blockIdx.x * kWavesPerBlock + wave;
  const int P = in.n_terms;
#pragma unroll
  for (int k = 0; k < DC_MAX_MODEL_TERMS; ++k) {
    if (k < P) {
      const double sw = wave_sum(gw[k]);
      const double se = want_e ? wave_sum(ge[k]) : 0.0;
      if (lane == 0) { prow[k * rs] = sw; prow[(P + k) * rs] = se; }
    }
  }
  // blk: the block's logical index where the caller's lanes are the plan's points in order (the grouped layout applies), -2 otherwise
  if (!want_pose) return;
  __shared__ double s_val[kBlock * kPoseRow];      // ONE staging array for whichever form runs (each function's own would add up: 14 KB apiece)
  if (in.seg_start && blk != -2) {
    double* prow = partials + 2 * P * rs + (int64_t)blockIdx.x * 12 * in.n_scans;
    if (in.n_scans <= kTicketScans) reduce_pose_grads_grouped(in, blk, active, gT, scan, prow, s_val);
    else reduce_pose_grads_grouped_wide(in, blk, active, gT, prow, s_val);
  }
  else reduce_pose_grads(in, active, gT, scan, lds, partials + (int64_t)blockIdx.x * kWavesPerBlock + 2 * P * rs, s_val);
}

// ------------------------------------------------------------------------------------------------
// Hot-path backward: dL/dx_j = sum over incoming edges (i -> j) of c1_i (v0_i . d) v0_i - c2_i d,
// d = x_j - cmean_i, gathered through the transposed neighbour list; fused with the point epilogue.
// ------------------------------------------------------------------------------------------------
#ifndef DC_BWD_F32
#define DC_BWD_F32 1
#endif
template <typename PT> constexpr bool kEdgeF32 = DC_BWD_F32 && std::is_same<PT, q32>::value;

// g += sum over four incoming edges of c1 (v0 . d) v0 - c2 d, d = x_j - cmean_i, from the raw 16-B pieces of the four
// records (an all-zero record contributes exactly nothing).  Shared by the gather and the LDS-staged kernel.
//   q32: the records hold c1, v0, c2 in fp32 and the integer differences of neighbouring points are exact in fp32
//   (< 2^24 grid steps), so the terms are formed in fp32 and the trip's partial sum is folded into the fp64
//   accumulators (error ~1e-7 of the largest term of the trip);
//   float / double points: fp64 throughout, separate multiplies and adds (measured faster than the dependent FMA
//   chains contraction produces: 90 vs 98 us at N = 2 M).
template <typename PT>
__device__ __forceinline__ void edge_terms4(const typename Pt<PT>::Raw& cj, const int4 (*q)[RecRaw<PT>::kRow16], double* g) {
  if constexpr (kEdgeF32<PT>) {
#pragma clang fp contract(fast)
    float gf[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int u_ = 0; u_ < 4; ++u_) {
      const int4 ra = q[u_][0], rb = q[u_][1];
      const float d0 = (float)(cj.v[0] - ra.x), d1 = (float)(cj.v[1] - ra.y), d2 = (float)(cj.v[2] - ra.z);
      const float c1 = __int_as_float(ra.w), c2 = __int_as_float(rb.w);
      const float v0 = __int_as_float(rb.x), v1 = __int_as_float(rb.y), v2 = __int_as_float(rb.z);
      const float t = c1 * (v0 * d0 + v1 * d1 + v2 * d2);
      gf[0] += t * v0 - c2 * d0;
      gf[1] += t * v1 - c2 * d1;
      gf[2] += t * v2 - c2 * d2;
    }
    g[0] += (double)gf[0]; g[1] += (double)gf[1]; g[2] += (double)gf[2];
  } else {
#pragma clang fp contract(off)
#pragma unroll
    for (int u_ = 0; u_ < 4; ++u_) {
      typename Pt<PT>::Raw m;
      double v[3], c1, c2, d[3];
      RecRaw<PT>::from_row(q[u_], m, &c1, v, &c2);
      Pt<PT>::delta(cj, m, d);
      const double t = c1 * (v[0] * d[0] + v[1] * d[1] + v[2] * d[2]);
      g[0] += t * v[0] - c2 * d[0];
      g[1] += t * v[1] - c2 * d[1];
      g[2] += t * v[2] - c2 * d[2];
    }
  }
}

template <typename T, typename PT, int STRIDE, bool WANT_E, bool WANT_POSE>
__global__ __launch_bounds__(kBlock) void consistency_bwd_kernel(
    const PT* __restrict__ x, const PT* __restrict__ rec, const int32_t* __restrict__ csr_ptr,
    const int32_t* __restrict__ csr_src, const uint8_t* __restrict__ lane_perm, int64_t n, PointInputs in, QParams qp,
    T* __restrict__ grad_points, double* __restrict__ partials, int n_acc, uint32_t rec_bytes) {
  // measured: the edge loop is faster with separate multiplies and adds (more independent work per trip) than with
  // the dependent FMA chains contraction produces (90 vs 98 us at N = 2 M)
#pragma clang fp contract(off)
  constexpr int want_e = WANT_E, want_pose = WANT_POSE;
  __shared__ double lds[(kBlock / kWave) * 2 * DC_MAX_MODEL_TERMS];
  __shared__ double s_pose[kLdsScans * 12];
  const PoseTile poses = in.dirs ? stage_poses(in, s_pose) : PoseTile{nullptr};
  if (WANT_POSE) pose_ticket_init();
  __syncthreads();
  const int64_t nblocks = (n + kBlock - 1) / kBlock;
  const int64_t blk = xcd_block(nblocks);
  ModelParams mp;
  load_model(in, mp);
  double gw[DC_MAX_MODEL_TERMS], ge[DC_MAX_MODEL_TERMS], gT[6];
#pragma unroll
  for (int k = 0; k < DC_MAX_MODEL_TERMS; ++k) gw[k] = ge[k] = 0.0;
#pragma unroll
  for (int k = 0; k < 6; ++k) gT[k] = 0.0;
  int scan = -1;
  bool active = false;
  if (blk >= 0) {
    // lane_perm orders the 256 points of a block by in-degree, so the lanes of a wavefront run similar trip counts
    const int64_t base = blk * kBlock;
    const int64_t j = base + (lane_perm ? (int64_t)lane_perm[base + threadIdx.x] : (int64_t)threadIdx.x);
    if (j < n) {
      active = true;
      double g[3] = {0.0, 0.0, 0.0};
      const typename Pt<PT>::Raw cj = Pt<PT>::template load<STRIDE>(x, j, qp);
      const double u = Pt<PT>::unit(qp);
      const int32_t beg = csr_ptr[j], end = csr_ptr[j + 1];
      // four edges per trip; the indices of the NEXT trip are requested before the records of this one are used,
      // so each trip exposes one memory latency instead of two.  Records come through a buffer resource: 32-bit
      // offsets, and an empty slot (index -1) is out of range and reads an all-zero record (c1 = c2 = 0).
      const BufRsrc rrec = make_rsrc(rec, rec_bytes);
      int32_t nxt[4];
#pragma unroll
      for (int u_ = 0; u_ < 4; ++u_) nxt[u_] = (beg + u_ < end) ? csr_src[beg + u_] : -1;
      for (int32_t e0 = beg; e0 < end; e0 += 4) {
        int32_t src[4];
        int4 q[4][RecRaw<PT>::kRow16];
#pragma unroll
        for (int u_ = 0; u_ < 4; ++u_) src[u_] = nxt[u_];
#pragma unroll
        for (int u_ = 0; u_ < 4; ++u_) {
#pragma unroll
          for (int a = 0; a < RecRaw<PT>::kRow16; ++a) q[u_][a] = buf_load16(rrec, (uint32_t)src[u_] * RowBytes<PT>::rec + 16u * a);
        }
#pragma unroll
        for (int u_ = 0; u_ < 4; ++u_) nxt[u_] = (e0 + 4 + u_ < end) ? csr_src[e0 + 4 + u_] : -1;
        edge_terms4<PT>(cj, q, g);
      }
      g[0] *= u; g[1] *= u; g[2] *= u;
      if (grad_points) Row3<T, STRIDE>::store(grad_points, j, g, QParams{});
      if (in.dirs) points_bwd_point<T>(in, poses, mp, j, g, gw, ge, gT, want_e != 0, want_pose != 0, &scan);
    }
  }
  if (in.dirs) reduce_param_grads<T>(in, active, want_e, want_pose, gw, ge, gT, scan, lds, partials, lane_perm ? -2 : blk);
}

// ------------------------------------------------------------------------------------------------
// LDS-staged gathers through a block table (dc_blocktab.hip).  A per-lane gather from global memory costs one L1 tag
// lookup per reference and the L1 serves one lookup per cycle: at K = 10 the 2560 references of a 256-point block kept
// the L1 of its CU busy for ~2560 cycles, which bounded both hot kernels (rocprofv3 TCP_TOTAL_CACHE_ACCESSES ~ 1.06 per
// CU cycle).  In Morton order those references hit only ~375 distinct rows, so every block first copies its distinct
// rows into LDS (one lookup each), then gathers from LDS through 16-bit block-local positions that are stored
// slot-major (a wavefront reads one slot with a single coalesced 128-B load).  Same arithmetic in the same order as the
// gather kernels => bit-identical results.
// ------------------------------------------------------------------------------------------------
struct BlockTab {
  const int32_t* __restrict__ blk_ptr;
  const int32_t* __restrict__ blk_ids;
  const int32_t* __restrict__ slot_ptr;
  const uint16_t* __restrict__ loc;
};
constexpr uint32_t kNoLoc = 0xFFFFu;

// Copy the distinct rows of block `blk` (ROW16 16-B pieces each) into `tile`; returns their number.  Piece a of row t
// lives at tile[a * cap + t]: a ds_read_b128 serves 16 lanes per cycle from 16 four-bank groups, and with whole rows
// back to back (32-B records) the group would be (2 t + a) mod 16 -- only 8 of the 16 for each piece, measured as 2/3
// of all LDS cycles lost to bank conflicts.  Piece-major, the group is t mod 16.
template <int ROW16>
__device__ __forceinline__ int stage_rows(const int32_t* __restrict__ blk_ptr, const int32_t* __restrict__ blk_ids, int64_t blk,
                                          const int4* __restrict__ src, int4* tile, int cap) {
  const int32_t base = blk_ptr[blk], nd = blk_ptr[blk + 1] - base;
  for (int t = threadIdx.x; t < nd; t += kBlock) {
    const int64_t id = blk_ids[base + t];
#pragma unroll
    for (int a = 0; a < ROW16; ++a) tile[a * cap + t] = src[id * ROW16 + a];
  }
  return nd;
}

// `off` = 16 x (row in the block's distinct list), exactly what the table stores: the LDS byte address needs no shift
template <int ROW16>
__device__ __forceinline__ void read_row(const int4* tile, int cap, uint32_t off, int4* q) {
  const char* p = reinterpret_cast<const char*>(tile) + off;
#pragma unroll
  for (int a = 0; a < ROW16; ++a) q[a] = *reinterpret_cast<const int4*>(p + (size_t)a * cap * 16);
}

// A staged q32 row is one 16-byte piece {x0, x1, x2, u0}.  A sweep that uses the point alone lets the compiler narrow its read to
// ds_read_b96, which the LDS serves in eight groups of 8 lanes on 32 banks where ds_read_b128 takes four groups of 16 on 64
// (MI355X: twice the array cycles before any conflict).  Naming the fourth word as the input of an empty statement keeps the read
// whole at no instruction.  The statement stands where the row is consumed, so the wait for the read stays where it was.
__device__ __forceinline__ void keep_row_word(int w) { asm volatile("" ::"v"(w)); }

constexpr int kPreSlots = 16;

// one slot from LDS; returns 1 if it held a neighbour.  MISS = false: the caller knows the slot is filled.
template <typename PT, bool MISS, bool WIDE = false>
__device__ __forceinline__ int slot_add(const int4* tile, int cap, const typename Pt<PT>::Raw& ci, uint32_t l, CovAcc& acc) {
  constexpr int XR = Pt<PT>::kRow16;
  const bool have = !MISS || l != kNoLoc;
  int4 piece[XR];
  read_row<XR>(tile, cap, have ? l : 0u, piece);
  const typename Pt<PT>::Raw cj = Pt<PT>::from_row(piece);
  if constexpr (WIDE) keep_row_word(piece[0].w);
  double d[3];
  Pt<PT>::delta(have ? cj : ci, ci, d);
  cov_add_d(acc, d[0], d[1], d[2]);
  return have ? 1 : 0;
}

// the first min(nslots, 16) slots from registers: whole trips of four with the LDS reads batched, then the remainder
// (WIDE: as gather_fixed)
template <typename PT, bool MISS, bool WIDE = false>
__device__ __forceinline__ int gather_slots(const int4* tile, int cap, const typename Pt<PT>::Raw& ci, const uint32_t* pre,
                                            int nslots, CovAcc& acc) {
  constexpr int XR = Pt<PT>::kRow16;
  int n_have = 0;
#pragma unroll
  for (int t = 0; t < kPreSlots / 4; ++t) {
    if (4 * t + 4 <= nslots) {
      typename Pt<PT>::Raw cj[4];
      bool have[4];
      int w4[4];
#pragma unroll
      for (int u_ = 0; u_ < 4; ++u_) {
        have[u_] = !MISS || pre[4 * t + u_] != kNoLoc;
        int4 piece[XR];
        read_row<XR>(tile, cap, have[u_] ? pre[4 * t + u_] : 0u, piece);
        cj[u_] = Pt<PT>::from_row(piece);
        w4[u_] = piece[0].w;
      }
#pragma unroll
      for (int u_ = 0; u_ < 4; ++u_) {
        if constexpr (WIDE) keep_row_word(w4[u_]);
        double d[3];
        Pt<PT>::delta(have[u_] ? cj[u_] : ci, ci, d);
        cov_add_d(acc, d[0], d[1], d[2]);
        n_have += have[u_] ? 1 : 0;
      }
    } else {
#pragma unroll
      for (int u_ = 0; u_ < 4; ++u_)
        if (4 * t + u_ < nslots) n_have += slot_add<PT, MISS, WIDE>(tile, cap, ci, pre[4 * t + u_], acc);
    }
  }
  return n_have;
}

// The slots beyond the first 16 (radius neighbourhoods: a hundred or two per point), in trips of eight: the positions of the
// NEXT trip are requested before the rows of this one are read, and the eight row reads of a trip are in flight together.  One
// slot per iteration -- a dependent {position load, LDS read} pair each -- left the kernel waiting on memory for most of a
// 200-slot row.  `packed` (dcBlockTable.packed): rows fill their slots from 0 upwards, so a wavefront stops at the first trip
// that is empty for all its lanes -- its own longest row, not the block's.
constexpr int kTrip = 8;
template <typename PT, bool WIDE = false>
__device__ __forceinline__ int gather_tail(const int4* tile, int cap, const typename Pt<PT>::Raw& ci, const uint16_t* lrow,
                                           int nslots, bool packed, CovAcc& acc) {
  constexpr int XR = Pt<PT>::kRow16;
  int n_have = 0;
  uint32_t nxt[kTrip];
#pragma unroll
  for (int u_ = 0; u_ < kTrip; ++u_) nxt[u_] = (kPreSlots + u_ < nslots) ? (uint32_t)lrow[(kPreSlots + u_) * kBlock] : kNoLoc;
  for (int q0 = kPreSlots; q0 < nslots; q0 += kTrip) {
    uint32_t l[kTrip];
#pragma unroll
    for (int u_ = 0; u_ < kTrip; ++u_) l[u_] = nxt[u_];
    if (packed && __all((int)(l[0] == kNoLoc))) break;
#pragma unroll
    for (int u_ = 0; u_ < kTrip; ++u_) nxt[u_] = (q0 + kTrip + u_ < nslots) ? (uint32_t)lrow[(q0 + kTrip + u_) * kBlock] : kNoLoc;
    typename Pt<PT>::Raw cj[kTrip];
    int w4[kTrip];
#pragma unroll
    for (int u_ = 0; u_ < kTrip; ++u_) {
      int4 piece[XR];
      read_row<XR>(tile, cap, l[u_] != kNoLoc ? l[u_] : 0u, piece);
      cj[u_] = Pt<PT>::from_row(piece);
      w4[u_] = piece[0].w;
    }
#pragma unroll
    for (int u_ = 0; u_ < kTrip; ++u_) {
      if constexpr (WIDE) keep_row_word(w4[u_]);
      const bool have = l[u_] != kNoLoc;
      double d[3];
      Pt<PT>::delta(have ? cj[u_] : ci, ci, d);
      cov_add_d(acc, d[0], d[1], d[2]);
      n_have += have ? 1 : 0;
    }
  }
  return n_have;
}

template <typename T, typename PT, bool FULL_EIG>
__global__ __launch_bounds__(kBlock) void consistency_fwd_staged_kernel(
    const PT* __restrict__ x, BlockTab tab, int cap, const int32_t* __restrict__ centre_idx, int64_t n,
    const uint8_t* __restrict__ mask, const T* __restrict__ offset, LossParams lp, QParams qp, PT* __restrict__ rec,
    T* __restrict__ pointwise, T* __restrict__ eigvals, double* __restrict__ partials) {
  constexpr int XR = Pt<PT>::kRow16;
  extern __shared__ int4 tile[];
  const int64_t nblocks = (n + kBlock - 1) / kBlock;
  const int64_t blk = xcd_block(nblocks);
  double acc2[2] = {0.0, 0.0};
  const int4* xg = reinterpret_cast<const int4*>(x);
  const int64_t i = blk * kBlock + threadIdx.x;
  const bool live = blk >= 0 && i < n;
  typename Pt<PT>::Raw ci;
  int32_t nslots = 0;
  const uint16_t* lrow = tab.loc;
  uint32_t pre[kPreSlots];                 // the lane's first 16 block-local positions
  if (blk >= 0) {
    // the lane's own requests go out before the staging loop, so their latency hides behind it
    const int32_t s0 = tab.slot_ptr[blk];
    nslots = tab.slot_ptr[blk + 1] - s0;
    lrow = tab.loc + (int64_t)s0 * kBlock + threadIdx.x;
    if (live) ci = Pt<PT>::from_row(xg + (centre_idx ? (int64_t)centre_idx[i] : i) * XR);
#pragma unroll
    for (int q = 0; q < kPreSlots; ++q) pre[q] = (live && q < nslots) ? (uint32_t)lrow[q * kBlock] : kNoLoc;
    stage_rows<XR>(tab.blk_ptr, tab.blk_ids, blk, xg, tile, cap);
  }
  __syncthreads();
  if (live) {
    CovAcc acc;
    cov_init(acc);
    // a missing neighbour (empty slot) contributes a zero difference and is not counted; only wavefronts that hold one
    // pay for the selects
    bool miss = false;
#pragma unroll
    for (int q = 0; q < kPreSlots; ++q) miss |= (q < nslots) && pre[q] == kNoLoc;
    int n_have = 0;
    if (__any((int)miss)) n_have = gather_slots<PT, true>(tile, cap, ci, pre, nslots, acc);
    else n_have = gather_slots<PT, false>(tile, cap, ci, pre, nslots, acc);
    for (int q = kPreSlots; q < nslots; ++q) {             // K > 16: one slot at a time
      const uint32_t l = lrow[q * kBlock];
      n_have += slot_add<PT, true>(tile, cap, ci, l, acc);
    }
    acc.W = (double)n_have;
    consistency_point<T, PT, FULL_EIG>(acc, ci, i, mask, offset, lp, qp, rec, pointwise, eigvals, acc2);
  }
  wave_partials<2>(acc2, partials);
}

// Fixed slot count: a forward table built from a neighbour table [rows, K] has exactly K slots in every block, so the
// slot loop, the position loads and the validity handling are resolved at compile time (the run-time variant above
// spends ~60 VALU instructions per point on them).  Same arithmetic in the same order => bit-identical results.
// WIDE (the one-pass step kernels' q32 rows): the 16-byte row is read whole (keep_row_word)
template <typename PT, int NS, bool MISS, bool WIDE = false>
__device__ __forceinline__ int gather_fixed(const int4* tile, int cap, const typename Pt<PT>::Raw& ci, const uint32_t* pre,
                                            CovAcc& acc) {
  constexpr int XR = Pt<PT>::kRow16;
  static_assert(!WIDE || XR == 1, "a row of one 16-byte piece");
  int n_have = 0;
#pragma unroll
  for (int q0 = 0; q0 < NS; q0 += 4) {
    typename Pt<PT>::Raw cj[4];
    bool have[4];
    int w4[4];
#pragma unroll
    for (int u_ = 0; u_ < 4; ++u_) {
      if (q0 + u_ < NS) {
        have[u_] = !MISS || pre[q0 + u_] != kNoLoc;
        int4 piece[XR];
        read_row<XR>(tile, cap, have[u_] ? pre[q0 + u_] : 0u, piece);
        cj[u_] = Pt<PT>::from_row(piece);
        w4[u_] = piece[0].w;
      }
    }
#pragma unroll
    for (int u_ = 0; u_ < 4; ++u_) {
      if (q0 + u_ < NS) {
        if constexpr (WIDE) keep_row_word(w4[u_]);
        double d[3];
        Pt<PT>::delta(have[u_] ? cj[u_] : ci, ci, d);
        cov_add_d(acc, d[0], d[1], d[2]);
        n_have += have[u_] ? 1 : 0;
      }
    }
  }
  return n_have;
}

template <typename T, typename PT, bool FULL_EIG, int NS>
__global__ __launch_bounds__(kBlock) void consistency_fwd_fixed_kernel(
    const PT* __restrict__ x, BlockTab tab, int cap, const int32_t* __restrict__ centre_idx, int64_t n,
    const uint8_t* __restrict__ mask, const T* __restrict__ offset, LossParams lp, QParams qp, PT* __restrict__ rec,
    T* __restrict__ pointwise, T* __restrict__ eigvals, double* __restrict__ partials) {
  constexpr int XR = Pt<PT>::kRow16;
  extern __shared__ int4 tile[];
  const int64_t nblocks = (n + kBlock - 1) / kBlock;
  const int64_t blk = xcd_block(nblocks);
  double acc2[2] = {0.0, 0.0};
  const int32_t s0 = blk >= 0 ? tab.slot_ptr[blk] : 0;
  // a table with another slot count than the launch was specialised for (not a table of [rows, NS]): fail loudly
  const bool bad = blk >= 0 && tab.slot_ptr[blk + 1] - s0 != NS;
  if (blk >= 0 && !bad) {
    const int4* xg = reinterpret_cast<const int4*>(x);
    const int64_t i = blk * kBlock + threadIdx.x;
    const bool live = i < n;
    // the table holds all 256 lanes of every block (0xFFFF beyond the last row): unconditional, immediate-offset loads
    const uint16_t* lrow = tab.loc + (int64_t)s0 * kBlock + threadIdx.x;
    uint32_t pre[NS];
#pragma unroll
    for (int q = 0; q < NS; ++q) pre[q] = (uint32_t)lrow[q * kBlock];
    typename Pt<PT>::Raw ci = Pt<PT>::from_row(xg + (live ? (centre_idx ? (int64_t)centre_idx[i] : i) : 0) * XR);
    stage_rows<XR>(tab.blk_ptr, tab.blk_ids, blk, xg, tile, cap);
    __syncthreads();
    if (live) {
      CovAcc acc;
      cov_init(acc);
      uint32_t mx = pre[0];
#pragma unroll
      for (int q = 1; q < NS; ++q) mx = max(mx, pre[q]);
      int n_have;
      if (__any((int)(mx == kNoLoc))) n_have = gather_fixed<PT, NS, true>(tile, cap, ci, pre, acc);
      else n_have = gather_fixed<PT, NS, false>(tile, cap, ci, pre, acc);
      acc.W = (double)n_have;
      consistency_point<T, PT, FULL_EIG>(acc, ci, i, mask, offset, lp, qp, rec, pointwise, eigvals, acc2);
    }
  } else {
    __syncthreads();
  }
  if (bad) acc2[0] = acc2[1] = __longlong_as_double(0x7ff8000000000000ll);
  wave_partials<2>(acc2, partials);
}

template <typename T, typename PT, bool WANT_E, bool WANT_POSE>
__global__ __launch_bounds__(kBlock) void consistency_bwd_staged_kernel(
    const PT* __restrict__ x, const PT* __restrict__ rec, BlockTab tab, int cap, int64_t n, PointInputs in, QParams qp,
    T* __restrict__ grad_points, double* __restrict__ partials, int n_acc) {
  constexpr int want_e = WANT_E, want_pose = WANT_POSE;
  constexpr int RR = RecRaw<PT>::kRow16, XR = Pt<PT>::kRow16;
  extern __shared__ int4 tile[];
  __shared__ double lds[(kBlock / kWave) * 2 * DC_MAX_MODEL_TERMS];
  __shared__ double s_pose[kLdsScans * 12];
  const PoseTile poses = in.dirs ? stage_poses(in, s_pose) : PoseTile{nullptr};      // published by the staging barrier
  const int64_t nblocks = (n + kBlock - 1) / kBlock;
  const int64_t blk = xcd_block(nblocks);
  ModelParams mp;
  load_model(in, mp);
  double gw[DC_MAX_MODEL_TERMS], ge[DC_MAX_MODEL_TERMS], gT[6];
#pragma unroll
  for (int k = 0; k < DC_MAX_MODEL_TERMS; ++k) gw[k] = ge[k] = 0.0;
#pragma unroll
  for (int k = 0; k < 6; ++k) gT[k] = 0.0;
  int scan = -1;
  const int64_t j = blk * kBlock + threadIdx.x;
  const bool active = blk >= 0 && j < n;
  typename Pt<PT>::Raw cj;
  PointRaw<T> raw;
  uint32_t pre[kPreSlots];
  int32_t nslots = 0;
  uint32_t nd = 0;
  const uint16_t* lrow = tab.loc;
  if (blk >= 0) {
    const int32_t s0 = tab.slot_ptr[blk];
    nslots = tab.slot_ptr[blk + 1] - s0;
    lrow = tab.loc + (int64_t)s0 * kBlock + threadIdx.x;
    if (active) {
      // everything this lane needs later is requested before the staging loop: its latency hides behind it
      cj = Pt<PT>::from_row(reinterpret_cast<const int4*>(x) + j * XR);
      if (in.dirs) raw = load_point_raw<T>(in, mp, j);
    }
#pragma unroll
    for (int q = 0; q < kPreSlots; ++q) pre[q] = (active && q < nslots) ? (uint32_t)lrow[q * kBlock] : kNoLoc;
    nd = (uint32_t)stage_rows<RR>(tab.blk_ptr, tab.blk_ids, blk, reinterpret_cast<const int4*>(rec), tile, cap);
    // row nd is an all-zero record: empty slots point there and contribute exactly nothing
    if (threadIdx.x < RR) tile[threadIdx.x * cap + nd] = make_int4(0, 0, 0, 0);
  }
  const uint32_t nd16 = nd * 16u;                           // positions are byte offsets; 0xFFFF (empty) clamps to the zero record
  if (WANT_POSE) pose_ticket_init();
  __syncthreads();
  if (active) {
    double g[3] = {0.0, 0.0, 0.0};
    const double u = Pt<PT>::unit(qp);
    // a lane's slots fill from 0 upwards: once a whole trip is empty for every lane of the wavefront, so are the rest
    bool more = true;
#pragma unroll
    for (int t = 0; t < kPreSlots / 4; ++t) {
      if (more && 4 * t < nslots) {
        if (__all((int)(pre[4 * t] == kNoLoc))) {
          more = false;
        } else {
          int4 q[4][RR];
#pragma unroll
          for (int u_ = 0; u_ < 4; ++u_) read_row<RR>(tile, cap, min(pre[4 * t + u_], nd16), q[u_]);
          edge_terms4<PT>(cj, q, g);
        }
      }
    }
    if (more && nslots > kPreSlots) {                       // in-degrees above 16: positions fetched trip by trip
      uint32_t nxt[4];
#pragma unroll
      for (int u_ = 0; u_ < 4; ++u_) nxt[u_] = (kPreSlots + u_ < nslots) ? (uint32_t)lrow[(kPreSlots + u_) * kBlock] : kNoLoc;
      for (int q0 = kPreSlots; q0 < nslots; q0 += 4) {
        uint32_t l[4];
        int4 q[4][RR];
#pragma unroll
        for (int u_ = 0; u_ < 4; ++u_) l[u_] = nxt[u_];
        if (__all((int)(l[0] == kNoLoc))) break;
#pragma unroll
        for (int u_ = 0; u_ < 4; ++u_) nxt[u_] = (q0 + 4 + u_ < nslots) ? (uint32_t)lrow[(q0 + 4 + u_) * kBlock] : kNoLoc;
#pragma unroll
        for (int u_ = 0; u_ < 4; ++u_) read_row<RR>(tile, cap, min(l[u_], nd16), q[u_]);
        edge_terms4<PT>(cj, q, g);
      }
    }
    g[0] *= u; g[1] *= u; g[2] *= u;
    if (grad_points) Row3<T, 4>::store(grad_points, j, g, QParams{});
    if (in.dirs) points_bwd_point<T>(in, poses, mp, j, raw, g, gw, ge, gT, want_e != 0, want_pose != 0, &scan);
  }
  if (in.dirs) reduce_param_grads<T>(in, active, want_e, want_pose, gw, ge, gT, scan, lds, partials, blk);
}

// Backward over a "lane run" table (dc_block_table_build_runs): the positions of a point's incoming edges are stored
// per point, contiguous and padded to a multiple of four (one 8-B load = one trip of four edges) instead of slot-major
// padded to the block's largest in-degree -- at K = 10 that is 12 instead of 16.2 stored positions per point (48 + 8 MB
// of run pointers instead of 105 MB at C2), and every lane stops at its own in-degree.  Same edge order and the same
// trips of four as the other backward kernels => bit-identical gradients.
struct RunTab {
  const int32_t* __restrict__ blk_ptr;
  const int32_t* __restrict__ blk_ids;
  const int32_t* __restrict__ run_ptr;     // [n + 1] in units of runs (4 positions = 8 B)
  const uint16_t* __restrict__ loc;        // 16 x position, 0xFFFF = padding
};
constexpr int kPreRuns = 4;

template <typename PT>
__device__ __forceinline__ void run_edges(const int4* tile, int cap, uint2 r, uint32_t nd16, const typename Pt<PT>::Raw& cj, double* g) {
  constexpr int RR = RecRaw<PT>::kRow16;
  int4 q[4][RR];
  read_row<RR>(tile, cap, min(r.x & 0xFFFFu, nd16), q[0]);
  read_row<RR>(tile, cap, min(r.x >> 16, nd16), q[1]);
  read_row<RR>(tile, cap, min(r.y & 0xFFFFu, nd16), q[2]);
  read_row<RR>(tile, cap, min(r.y >> 16, nd16), q[3]);
  edge_terms4<PT>(cj, q, g);
}

template <typename T, typename PT, bool WANT_E, bool WANT_POSE>
__global__ __launch_bounds__(kBlock) void consistency_bwd_runs_kernel(
    const PT* __restrict__ x, const PT* __restrict__ rec, RunTab tab, int cap, int64_t n, PointInputs in, QParams qp,
    T* __restrict__ grad_points, double* __restrict__ partials, int n_acc) {
  constexpr int want_e = WANT_E, want_pose = WANT_POSE;
  constexpr int RR = RecRaw<PT>::kRow16, XR = Pt<PT>::kRow16;
  extern __shared__ int4 tile[];
  __shared__ double lds[(kBlock / kWave) * 2 * DC_MAX_MODEL_TERMS];
  __shared__ double s_pose[kLdsScans * 12];
  const PoseTile poses = in.dirs ? stage_poses(in, s_pose) : PoseTile{nullptr};      // published by the staging barrier
  const int64_t nblocks = (n + kBlock - 1) / kBlock;
  const int64_t blk = xcd_block(nblocks);
  ModelParams mp;
  load_model(in, mp);
  double gw[DC_MAX_MODEL_TERMS], ge[DC_MAX_MODEL_TERMS], gT[6];
#pragma unroll
  for (int k = 0; k < DC_MAX_MODEL_TERMS; ++k) gw[k] = ge[k] = 0.0;
#pragma unroll
  for (int k = 0; k < 6; ++k) gT[k] = 0.0;
  int scan = -1;
  const int64_t j = blk * kBlock + threadIdx.x;
  const bool active = blk >= 0 && j < n;
  typename Pt<PT>::Raw cj;
  PointRaw<T> raw;
  uint2 pre[kPreRuns];
  int32_t nruns = 0;
  uint32_t nd = 0;
  const uint2* runs = reinterpret_cast<const uint2*>(tab.loc);
  if (blk >= 0) {
    if (active) {
      // everything this lane needs later is requested before the staging loop: its latency hides behind it
      const int32_t r0 = tab.run_ptr[j];
      nruns = tab.run_ptr[j + 1] - r0;
      runs += r0;
      cj = Pt<PT>::from_row(reinterpret_cast<const int4*>(x) + j * XR);
      if (in.dirs) raw = load_point_raw<T>(in, mp, j);
    }
#pragma unroll
    for (int t = 0; t < kPreRuns; ++t) pre[t] = t < nruns ? runs[t] : make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu);
    nd = (uint32_t)stage_rows<RR>(tab.blk_ptr, tab.blk_ids, blk, reinterpret_cast<const int4*>(rec), tile, cap);
    // row nd is an all-zero record: padding positions clamp to it and contribute exactly nothing
    if (threadIdx.x < RR) tile[threadIdx.x * cap + nd] = make_int4(0, 0, 0, 0);
  }
  const uint32_t nd16 = nd * 16u;
  if (WANT_POSE) pose_ticket_init();
  __syncthreads();
  if (active) {
    double g[3] = {0.0, 0.0, 0.0};
    const double u = Pt<PT>::unit(qp);
#pragma unroll
    for (int t = 0; t < kPreRuns; ++t)
      if (__any((int)(t < nruns))) run_edges<PT>(tile, cap, pre[t], nd16, cj, g);
    if (__any((int)(nruns > kPreRuns))) {                   // in-degrees above 16: runs fetched trip by trip, one ahead
      uint2 nxt = kPreRuns < nruns ? runs[kPreRuns] : make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu);
      for (int t = kPreRuns; __any((int)(t < nruns)); ++t) {
        const uint2 r = nxt;
        nxt = t + 1 < nruns ? runs[t + 1] : make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu);
        run_edges<PT>(tile, cap, r, nd16, cj, g);
      }
    }
    g[0] *= u; g[1] *= u; g[2] *= u;
    if (grad_points) Row3<T, 4>::store(grad_points, j, g, QParams{});
    if (in.dirs) points_bwd_point<T>(in, poses, mp, j, raw, g, gw, ge, gT, want_e != 0, want_pose != 0, &scan);
  }
  if (in.dirs) reduce_param_grads<T>(in, active, want_e, want_pose, gw, ge, gT, scan, lds, partials, blk);
}

}  // namespace dc

// The basis form, the chained steps, the one-pass step kernels and the one-pass pose kernel live in headers of their own; they are
// parts of this translation unit (they use the tables and gather helpers above) and are included in the order they build on each other.
#include "dc_cons_basis.h"
#include "dc_cons_chain.h"
#include "dc_cons_step.h"
#include "dc_cons_pose.h"

namespace dc {

// Quantile-inlier gating of the pointwise loss (loss.py:256-277) for the fused path: `raw` is the forward's raw loss
// (DC_LOSS_RAW_POINTWISE), *threshold the bound the caller derived from it (quantile x multiplier, or the given maximum).
// A masked centre with raw loss above the bound (or NaN: `<=` fails as in torch) is dropped: its record's coefficients
// are zeroed, so the backward passes nothing through it; the sums become {sum of relu / sqrt loss, count} of the inliers.
template <typename PT> struct RecWord { using type = PT; };
template <> struct RecWord<q32> { using type = int32_t; };          // c1 / c2 are float bits: all-zero bits = 0.0f
template <typename T, typename PT>
__global__ __launch_bounds__(kBlock) void consistency_gate_kernel(const T* __restrict__ raw, const uint8_t* __restrict__ mask, int64_t n,
                                                                  const double* __restrict__ threshold, int sqrt_,
                                                                  PT* __restrict__ rec, double* __restrict__ partials) {
  const int64_t nblocks = (n + kBlock - 1) / kBlock;
  const int64_t blk = xcd_block(nblocks);
  double acc2[2] = {0.0, 0.0};
  const int64_t i = blk * kBlock + threadIdx.x;
  if (blk >= 0 && i < n) {
    const bool m = mask ? mask[i] != 0 : true;
    const T r = raw[i];
    const bool in = m && (r <= (T)*threshold);        // compared in the cloud dtype, like the reference's tensors
    if (in) {
      double l = (double)r;
      l = l > 0.0 ? l : 0.0;
      if (sqrt_) l = sqrt(l);
      acc2[0] = l; acc2[1] = 1.0;
    } else if (m) {
      using W = typename RecWord<PT>::type;
      W* row = reinterpret_cast<W*>(rec) + i * 8;
      row[3] = W(0); row[7] = W(0);
    }
  }
  wave_partials<2>(acc2, partials);
}

// Stand-alone point epilogue for the un-fused API path (grad of points given).
template <typename T, int STRIDE>
__global__ __launch_bounds__(kBlock) void points_bwd_kernel(const T* __restrict__ grad_x, const int32_t* __restrict__ perm,
                                                            int64_t n, PointInputs in, int want_e, int want_pose,
                                                            double* __restrict__ partials, int n_acc) {
  __shared__ double lds[(kBlock / kWave) * 2 * DC_MAX_MODEL_TERMS];
  __shared__ double s_pose[kLdsScans * 12];
  const PoseTile poses = stage_poses(in, s_pose);
  __syncthreads();
  ModelParams mp;
  load_model(in, mp);
  double gw[DC_MAX_MODEL_TERMS], ge[DC_MAX_MODEL_TERMS], gT[6];
#pragma unroll
  for (int k = 0; k < DC_MAX_MODEL_TERMS; ++k) gw[k] = ge[k] = 0.0;
#pragma unroll
  for (int k = 0; k < 6; ++k) gT[k] = 0.0;
  int scan = -1;
  const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const bool active = j < n;
  if (active) {
    double g[3];
    Row3<T, STRIDE>::load(grad_x, perm ? (int64_t)perm[j] : j, g, QParams{});      // perm: grad rows live in another point order
    points_bwd_point<T>(in, poses, mp, j, g, gw, ge, gT, want_e != 0, want_pose != 0, &scan);
  }
  reduce_param_grads<T>(in, active, want_e, want_pose, gw, ge, gT, scan, lds, partials);
}

// Sum the block partials [n_acc][n_rows] in a fixed order into out[n_acc]: one 1024-lane block per accumulator,
// contiguous (coalesced) reads.
constexpr int kRedBlock = 1024;
// Sum of p[threadIdx.x], p[threadIdx.x + 1024], ... in a fixed order with 32 loads in flight per lane: the rows were
// written by blocks on every XCD, so each read is a trip to the fabric, and with four in flight the ~31 rows per lane
// (N = 2 M) took eight dependent round trips.
constexpr int kPoseRedCols = 8;          // columns of the row-major pose partials a block of reduce_eval_kernel sums: one 64-byte line
__device__ __forceinline__ double strided_sum(const double* __restrict__ p, int64_t n_rows, int64_t stride = 1, int first = -1,
                                              int step = kRedBlock) {
  constexpr int U = 32;                  // 32 k rows (N = 2 M: one row per wavefront) in ONE round trip per lane
  double acc[U];
#pragma unroll
  for (int u_ = 0; u_ < U; ++u_) acc[u_] = 0.0;
  int64_t r = first < 0 ? (int)threadIdx.x : first;        // this lane's rows: r, r + step, ...
  for (; r + (int64_t)(U - 1) * step < n_rows; r += (int64_t)U * step) {
#pragma unroll
    for (int u_ = 0; u_ < U; ++u_) acc[u_] += p[(r + (int64_t)u_ * step) * stride];
  }
  {
    double last[U];                      // the tail's loads are issued together, too
#pragma unroll
    for (int u_ = 0; u_ < U; ++u_) last[u_] = (r + (int64_t)u_ * step < n_rows) ? p[(r + (int64_t)u_ * step) * stride] : 0.0;
#pragma unroll
    for (int u_ = 0; u_ < U; ++u_) acc[u_] += last[u_];
  }
#pragma unroll
  for (int w = U / 2; w > 0; w >>= 1) {
#pragma unroll
    for (int u_ = 0; u_ < w; ++u_) acc[u_] += acc[u_ + w];
  }
  return acc[0];
}
__global__ __launch_bounds__(kRedBlock) void reduce_partials_kernel(const double* __restrict__ partials, int64_t n_rows,
                                                                    double* __restrict__ out) {
  __shared__ double lds[kRedBlock / kWave];
  const double* p = partials + (int64_t)blockIdx.x * n_rows;
  const double s = wave_sum(strided_sum(p, n_rows));
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  if (lane == 0) lds[wave] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int wv = 0; wv < kRedBlock / kWave; ++wv) t += lds[wv];
    out[blockIdx.x] = t;
  }
}

// One launch for a whole evaluation: out[0..2) <- forward partials, out[2..2+n_red) <- backward partials,
// out[2+n_red..2+n_acc) <- 0 (gradient slots that were not requested).  With `adam.p` the block that finishes
// dL/dw_i also takes the Adam step of w_i (dc_sequence_step: the kernels of the next evaluation come after it on
// the stream).
__global__ __launch_bounds__(kRedBlock) void reduce_eval_kernel(const double* __restrict__ p_fwd, const double* __restrict__ p_bwd,
                                                                int64_t rows_fwd, int64_t rows_bwd, int n_red, int n_out,
                                                                double* __restrict__ out, AdamArgs adam,
                                                                const int32_t* __restrict__ status, int pose_first = -1,
                                                                int pose_cols = 0) {
  // pose_first >= 0: the accumulators from 2 + pose_first on (the pose slots) were written ROW-major [rows_bwd / 4][pose_cols]
  // behind the column-major ones (one row per block of the backward / pose kernel).  A block of this kernel then sums EIGHT
  // neighbouring columns -- one 64-byte line of every row: lane & 7 is the column, the other lane bits the row -- so every line is
  // fetched once, by one XCD (a block per column fetched each line eight times: 16 us at N = 2 M, 20 scans, against 4).
  __shared__ double lds[kRedBlock / kWave * kPoseRedCols];
  const int a = blockIdx.x;                // grid = red_grid(): only the sums that were asked for get a block
  if (a == 0)                              // block 0 also clears the slots of gradients that were not requested
    for (int z = 2 + n_red + threadIdx.x; z < n_out; z += kRedBlock) out[z] = 0.0;
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  if (pose_first >= 0 && a >= 2 + pose_first) {
    const int col = (a - 2 - pose_first) * kPoseRedCols + (threadIdx.x & (kPoseRedCols - 1));
    const bool have = col < pose_cols;
    const double* p = p_bwd + (int64_t)pose_first * rows_bwd + (have ? col : 0);
    double s = strided_sum(p, have ? rows_bwd / kWavesPerBlock : 0, pose_cols, threadIdx.x / kPoseRedCols, kRedBlock / kPoseRedCols);
#pragma unroll
    for (int o = kPoseRedCols; o < kWave; o <<= 1) s += __shfl_xor(s, o, kWave);
    if (lane < kPoseRedCols) lds[wave * kPoseRedCols + lane] = s;
    __syncthreads();
    if (threadIdx.x < kPoseRedCols && have) {
      double t = 0.0;
      for (int wv = 0; wv < kRedBlock / kWave; ++wv) t += lds[wv * kPoseRedCols + threadIdx.x];
      out[2 + pose_first + col] = t;
    }
    return;
  }
  const bool flagged = a == 0 && threadIdx.x == 0 && status && *status != 0;      // requested before the rows, not after
  const int64_t n_rows = a < 2 ? rows_fwd : rows_bwd;
  const double* p = a < 2 ? p_fwd + (int64_t)a * rows_fwd : p_bwd + (int64_t)(a - 2) * rows_bwd;
  const bool step = adam.p && a >= 2 && a - 2 < adam.n && threadIdx.x == 0;
  double p0 = 0.0, m0 = 0.0, v0 = 0.0;
  if (step) { p0 = adam.p[a - 2]; m0 = adam.m[a - 2]; v0 = adam.v[a - 2]; }      // in flight together with the partial rows
  const double s = wave_sum(strided_sum(p, n_rows));
  if (lane == 0) lds[wave] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int wv = 0; wv < kRedBlock / kWave; ++wv) t += lds[wv];
    // points that did not fit the fixed-point extent (or were NaN) make the evaluation meaningless: say so in the loss
    if (flagged) t = __longlong_as_double(0x7ff8000000000000ll);
    out[a] = t;
    if (step) adam_apply(adam, a - 2, t, p0, m0, v0);
  }
}

// blocks of reduce_eval_kernel: one per column-major sum, one per kPoseRedCols columns of row-major pose partials
static inline unsigned red_grid(int n_red, int pose_first, int pose_cols) {
  if (pose_first < 0 || n_red <= pose_first) return 2u + (unsigned)n_red;
  return 2u + (unsigned)pose_first + (unsigned)((pose_cols + kPoseRedCols - 1) / kPoseRedCols);
}

__global__ void adam_kernel(const double* __restrict__ grad, AdamArgs adam) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i < adam.n) adam_update(adam, i, grad[i]);
}

// The same with the step counter on the device (one block): t = *step + 1 enters the bias corrections and is written back,
// so the launch can be captured into a hipGraph and replayed -- a host-side counter would be frozen into the graph.
__global__ __launch_bounds__(256) void adam_device_step_kernel(const double* __restrict__ grad, AdamArgs adam, int64_t* __restrict__ step) {
  const double t = (double)(*step + 1);
  adam.bias1 = 1.0 - pow(adam.b1, t);
  adam.bias2_sqrt = sqrt(1.0 - pow(adam.b2, t));
  for (int i = threadIdx.x; i < adam.n; i += blockDim.x) adam_update(adam, i, grad[i]);
  __syncthreads();                                   // every lane has read the counter
  if (threadIdx.x == 0) *step = (int64_t)t;
}

}  // namespace dc

// ================================================================================================
// C ABI
// ================================================================================================
using namespace dc;

#define DC_CHECK_LAUNCH()                                  \
  do {                                                     \
    hipError_t err__ = hipGetLastError();                  \
    if (err__ != hipSuccess) return (int)err__;            \
  } while (0)

static inline int64_t n_blocks(int64_t n) { return (n + kBlock - 1) / kBlock; }
// The A-B switches of dc_set_option: process-wide, read once per launch
// dc_set_option(0, 1): ignore block tables, gather from global memory
static std::atomic<bool> g_no_tab{false};
// dc_set_option(1, 1): run-time slot loop instead of the fixed-K forward kernels
static std::atomic<int> g_fwd_generic{0};
// dc_set_option(3, 1): ignore a sequence's basis rows (general path)
static std::atomic<bool> g_no_basis{false};
// dc_set_option(4, 1): basis form with separate forward and backward kernels
static std::atomic<bool> g_two_pass{false};
// dc_set_option(5, n): polls of a chained launch's wait for its weights (tests force 0)
static std::atomic<int> g_chain_spin{1 << 22};
// dc_set_option(6, v): 1 = consistency_step_q32_kernel for float32 clouds with a [rows, K] table (default), 7 =
// consistency_step_basis_kernel<.., kStepVar> for them too, 0 = its round-2 form (K = 10, P = 2 only: A-B baseline)
static std::atomic<int> g_step_var{1};
// dc_set_option(7, 1): pose gradients through the three-kernel general path (A-B, tests)
static std::atomic<bool> g_pose_three_pass{false};
// dc_set_option(8, 1): every launch of a chain walks the blocks forwards (A-B, chain_block_of)
static std::atomic<bool> g_no_reverse{false};
// dc_set_option(9, 1): consistency_step_q32_kernel built for six blocks per CU where the default is built for seven (the 512-row tile,
// one or two weights): the same body under __launch_bounds__(kBlock, 6) (A-B, tests); the other instantiations are not affected
static std::atomic<bool> g_step_six{false};
// dc_set_option(10, 1): consistency_step_q32_kernel ignores dcSequenceDesc.step_rows and stages through blk_ids (A-B, tests)
static std::atomic<bool> g_no_step_rows{false};
// dc_set_option(11, 1): consistency_step_q32_kernel ignores dcSequenceDesc.step_loc and reads its tile positions from the table's loc (A-B, tests)
static std::atomic<bool> g_no_step_loc{false};

// consistency_step_ragged_q32_kernel with a tile of CAP rows: more than 64 KB of LDS per block needs the attribute (once per
// instantiation, process and device).  Capacities up to the table's own limit (4095 rows), so every ball-neighbourhood table that can be
// built runs fused -- at one block per CU for the densest (voxel grid 0.1 m, r = 0.25 m: 2 000 distinct rows per block).
template <int P, int CAP>
static int ragged_launch(dim3 grid, hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1, const PointBasis& pb, const BlockTab& tab,
                         const dcBlockTable* t, int64_t n_rows, const uint8_t* mask, const LossParams& lp, const QParams& qp, double* p_fwd,
                         double* p_bwd, const StepChain& ch) {
  constexpr size_t bytes = (size_t)StepRow<q32, P>::kPieces * CAP * 16;
  static_assert(bytes >= step_hand_bytes<P>(), "the hand-over of step_block_row lives in the tile");
  // function attributes are per device: one bit per device of the process (a second GPU of the same process sets its own)
  static std::atomic<uint64_t> attr_set{0};
  if (bytes > 60 * 1024) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    const uint64_t bit = 1ull << (dev & 63);
    if (!(attr_set.fetch_or(bit) & bit)) {
      hipError_t err = hipFuncSetAttribute((const void*)consistency_step_ragged_q32_kernel<P, CAP>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
      if (err != hipSuccess) { attr_set.fetch_and(~bit); return (int)err; }
    }
  }
  hipExtLaunchKernelGGL((consistency_step_ragged_q32_kernel<P, CAP>), grid, dim3(kBlock), bytes, stream, ev0, ev1, 0, pb, tab, t->own_base, t->row_ptr, n_rows,
                        mask, lp, qp, p_fwd, p_bwd, ch);
  return DC_OK;
}

// dc_cons_route.h restates what the device headers own: every constant and row size it uses is held against the definition here
static_assert(kRouteBlock == kBlock && kRouteXcds == kXcds && kRouteWavesPerBlock == kWavesPerBlock && kRouteLdsScans == kLdsScans &&
              kRouteMaxBlockScans == kMaxBlockScans && kRouteStepQ32Cap == kStepQ32Cap && kRouteChainFront == kChainFront, "dc_cons_route.h");
static_assert(route_xcd_grid(1) == xcd_grid(1) && route_xcd_grid(8) == xcd_grid(8) && route_xcd_grid(7813) == xcd_grid(7813), "dc_cons_route.h");
static_assert(route_step_row_bytes(false, 1) == StepRow<q32, 1>::kPieces * 16 && route_step_row_bytes(false, 2) == StepRow<q32, 2>::kPieces * 16 &&
              route_step_row_bytes(false, 3) == StepRow<q32, 3>::kPieces * 16 && route_step_row_bytes(true, 1) == StepRow<double, 1>::kPieces * 16 &&
              route_step_row_bytes(true, 2) == StepRow<double, 2>::kPieces * 16 && route_step_row_bytes(true, 3) == StepRow<double, 3>::kPieces * 16, "dc_cons_route.h");
static_assert(route_x_row_bytes(false) == RowBytes<q32>::x && route_x_row_bytes(true) == RowBytes<double>::x &&
              route_rec_row_bytes(false) == RowBytes<q32>::rec && route_rec_row_bytes(true) == RowBytes<double>::rec, "dc_cons_route.h");

// the switches the route reads, once per call
static inline RouteOptions route_options() {
  RouteOptions o;
  o.no_tab = g_no_tab.load(); o.fwd_generic = g_fwd_generic.load(); o.no_basis = g_no_basis.load(); o.two_pass = g_two_pass.load();
  o.step_var = g_step_var.load(); o.pose_three_pass = g_pose_three_pass.load(); o.step_six = g_step_six.load();
  return o;
}

// The instantiation ladders, written once: M(value, ...) for K = 10 / 4 / 8 / 16 and for one or two weights; OTHER (a statement, may be
// empty) is what any other value runs -- the slot-loop kernel, the instantiations for three weights where a kernel has them.
#define DC_SWITCH_K(k, OTHER, M, ...) \
  do { switch (k) { case 10: M(10, __VA_ARGS__); break; case 4: M(4, __VA_ARGS__); break; case 8: M(8, __VA_ARGS__); break; \
                    case 16: M(16, __VA_ARGS__); break; default: { OTHER; } } } while (0)
#define DC_SWITCH_P(p, OTHER, M, ...) \
  do { if ((p) == 2) M(2, __VA_ARGS__); else if ((p) == 1) M(1, __VA_ARGS__); else { OTHER; } } while (0)

extern "C" {

int dc_version(void) { return 100; }

int64_t dc_partial_rows(int64_t n) { return route_xcd_grid(route_blocks(n)) * kRouteWavesPerBlock; }

int dc_param_grad_count(int n_terms, int n_scans) { return 2 * n_terms + 12 * n_scans; }

// ordinary evaluations: rows x (2 + 2 P + 12 S) columns; chained steps: two buffers of (2 + P) columns behind them (chain_buffer)
int64_t dc_sequence_partials_count(int64_t n, int n_terms, int n_scans) { return route_partials_count(n, n_terms, n_scans); }

static PointInputs make_inputs(const void* vps, const void* dirs, const void* depth, const void* inc,
                               const uint8_t* lmask, const int32_t* scan_id, const double* poses, int n_scans,
                               int model_kind, int n_terms, const double* w, const double* e) {
  PointInputs in;
  in.vps = vps; in.dirs = dirs; in.depth = depth; in.inc = inc; in.lmask = lmask; in.scan_id = scan_id;
  in.poses = poses; in.w = w; in.e = e; in.model_kind = model_kind; in.n_terms = n_terms; in.n_scans = n_scans;
  return in;
}

static int check_model(int model_kind, int n_terms, const void* inc, const double* w, const double* e) {
  if (model_kind < DC_MODEL_NONE || model_kind > DC_MODEL_LAST) return DC_ERR_ARG;
  if (model_kind != DC_MODEL_NONE) {
    if (n_terms < 1 || n_terms > DC_MAX_MODEL_TERMS || !inc || !w || !e) return DC_ERR_ARG;
    if (model_kind == DC_MODEL_LINEAR && n_terms != 3) return DC_ERR_ARG;
    if ((model_kind == DC_MODEL_INVCOS || model_kind == DC_MODEL_SCALED_INVCOS) && n_terms != 1) return DC_ERR_ARG;
  }
  return DC_OK;
}

static int make_qparams(int point_fmt, int dtype, int stride, const double* qparams, QParams* qp, int32_t* flag = nullptr) {
  *qp = QParams{};
  qp->flag = flag;
  if (point_fmt == DC_Q32) {
    if (!qparams || stride != 4 || dtype != DC_F32 || !(qparams[3] > 0.0)) return DC_ERR_ARG;
    qp->origin[0] = qparams[0]; qp->origin[1] = qparams[1]; qp->origin[2] = qparams[2];
    qp->scale = qparams[3];
    qp->inv_scale = 1.0 / qparams[3];
    return DC_OK;
  }
  return point_fmt == dtype ? DC_OK : DC_ERR_DTYPE;      // float / double points share the inputs' dtype
}

// Dispatch over (input dtype, point format, row stride).
#define DC_DISPATCH_FMT(dtype, fmt, stride, LAUNCH)                       \
  do {                                                                    \
    if ((fmt) == DC_Q32) { LAUNCH(float, q32, 4); }                       \
    else if ((dtype) == DC_F32) { if ((stride) == 3) { LAUNCH(float, float, 3); } else { LAUNCH(float, float, 4); } } \
    else if ((dtype) == DC_F64) { if ((stride) == 3) { LAUNCH(double, double, 3); } else { LAUNCH(double, double, 4); } } \
    else return DC_ERR_DTYPE;                                             \
  } while (0)

int dc_points_fwd(const void* vps, const void* dirs, const void* depth, const void* inc, const uint8_t* lmask,
                  const int32_t* scan_id, const double* poses, int n_scans, int model_kind, int n_terms,
                  const double* w, const double* e, int64_t n, int dtype, int point_fmt, const double* qparams,
                  int out_stride, void* points_out, void* vps_out, void* dirs_out, void* depth_out, int32_t* status,
                  hipStream_t stream) {
  if (n == 0) return DC_OK;
  if (n < 0 || !dirs || !depth || !points_out || (out_stride != 3 && out_stride != 4)) return DC_ERR_ARG;
  if (scan_id && (!poses || n_scans < 1)) return DC_ERR_ARG;
  int rc = check_model(model_kind, n_terms, inc, w, e);
  if (rc) return rc;
  QParams qp;
  rc = make_qparams(point_fmt, dtype, out_stride, qparams, &qp, status);
  if (rc) return rc;
  if (n == 0) return DC_OK;
  if (model_kind == DC_MODEL_NONE) n_terms = 0;
  PointInputs in = make_inputs(vps, dirs, depth, inc, lmask, scan_id, poses, n_scans, model_kind, n_terms, w, e);
  dim3 grid((unsigned)n_blocks(n)), block(kBlock);
#define LAUNCH(T, PT, S) \
  DC_TIMED_LAUNCH((points_fwd_kernel<T, PT, S>), grid, block, 0, stream, in, n, qp, (PT*)points_out, (T*)vps_out, (T*)dirs_out, (T*)depth_out)
  { ProfScope prof(0); DC_DISPATCH_FMT(dtype, point_fmt, out_stride, LAUNCH); }
#undef LAUNCH
  DC_CHECK_LAUNCH();
  return DC_OK;
}

int dc_points_basis(const void* vps, const void* dirs, const void* depth, const void* inc, const uint8_t* lmask,
                    const int32_t* scan_id, const double* poses, int n_scans, int model_kind, int n_terms, const double* e,
                    int64_t n, int dtype, const double* qparams, void* rows_out, int32_t* status, hipStream_t stream) {
  if (n == 0) return DC_OK;
  if (n < 0 || !dirs || !depth || !rows_out) return DC_ERR_ARG;
  if (scan_id && (!poses || n_scans < 1)) return DC_ERR_ARG;
  if (dtype != DC_F32 && dtype != DC_F64) return DC_ERR_DTYPE;
  if (dtype == DC_F32 && !qparams) return DC_ERR_ARG;         // float32 clouds: rows on the q32 grid
  // the weights do not enter the basis rows: a dummy non-null pointer satisfies the model check, load_model reads e only... and w
  int rc = check_model(model_kind, n_terms, inc, e, e);
  if (rc || model_kind == DC_MODEL_NONE) return rc ? rc : DC_ERR_ARG;
  QParams qp;
  rc = make_qparams(dtype == DC_F32 ? DC_Q32 : DC_F64, dtype, 4, qparams, &qp, status);
  if (rc) return rc;
  PointInputs in = make_inputs(vps, dirs, depth, inc, lmask, scan_id, poses, n_scans, model_kind, n_terms, e, e);
  if (dtype == DC_F32)
    hipLaunchKernelGGL((points_basis_kernel<q32>), dim3((unsigned)n_blocks(n)), dim3(kBlock), 0, stream, in, n, qp, rows_out);
  else
    hipLaunchKernelGGL((points_basis_kernel<double>), dim3((unsigned)n_blocks(n)), dim3(kBlock), 0, stream, in, n, qp, rows_out);
  DC_CHECK_LAUNCH();
  return DC_OK;
}

int dc_step_rows_build(const dcBlockTable* table, int64_t n_rows, const void* basis, int row_words, void* rows_out, hipStream_t stream) {
  if (!table || n_rows < 0 || table->layout != DC_TABLE_SLOTS || !table->blk_ptr || row_words < 7 || row_words > 6 + 3) return DC_ERR_ARG;
  if (n_rows == 0) return DC_OK;
  if (!table->blk_ids || !basis || !rows_out || ((uintptr_t)rows_out & 15)) return DC_ERR_ARG;
  hipLaunchKernelGGL(step_rows_kernel, dim3((unsigned)n_blocks(n_rows)), dim3(kBlock), 0, stream, table->blk_ptr, table->blk_ids,
                     static_cast<const int32_t*>(basis), row_words, static_cast<int32_t*>(rows_out));
  DC_CHECK_LAUNCH();
  return DC_OK;
}

int dc_step_loc_build(const dcBlockTable* table, int64_t n_rows, void* loc_out, hipStream_t stream) {
  if (!table || n_rows < 0 || table->layout != DC_TABLE_SLOTS || !table->slot_ptr) return DC_ERR_ARG;
  if (n_rows == 0) return DC_OK;
  if (!table->loc || !loc_out || ((uintptr_t)loc_out & 15)) return DC_ERR_ARG;
  hipLaunchKernelGGL(step_loc_kernel, dim3((unsigned)n_blocks(n_rows)), dim3(kBlock), 0, stream, table->slot_ptr, table->loc,
                     static_cast<uint32_t*>(loc_out));
  DC_CHECK_LAUNCH();
  return DC_OK;
}

int dc_points_local_basis(const void* dirs, const void* depth, const void* inc, const uint8_t* lmask, const int32_t* scan_id,
                          int model_kind, int n_terms, const double* e, int64_t n, int dtype, const dcPoseTable* table, void* rows_out,
                          hipStream_t stream) {
  if (n == 0) return DC_OK;
  if (n < 0 || !dirs || !depth || !rows_out || n_terms < 1 || n_terms > 2 || !table || !table->blk_ptr || !table->ids) return DC_ERR_ARG;
  if (dtype != DC_F32) return DC_ERR_DTYPE;                  // float32 clouds (q32 points): what the pose kernel takes
  int rc = check_model(model_kind, n_terms, inc, e, e);
  if (rc || model_kind == DC_MODEL_NONE) return rc ? rc : DC_ERR_ARG;
  PointInputs in = make_inputs(nullptr, dirs, depth, inc, lmask, scan_id, nullptr, 1, model_kind, n_terms, e, e);
  PoseTab tab{table->blk_ptr, table->ids, table->loc, table->own_pos, table->row_seg, table->row_scan};
  hipLaunchKernelGGL((points_local_basis_kernel<float>), dim3((unsigned)n_blocks(n)), dim3(kBlock), 0, stream, in, tab, (int32_t*)rows_out);
  DC_CHECK_LAUNCH();
  return DC_OK;
}

int dc_pose_table_build(const dcBlockTable* fwd, const int32_t* scan_id, int64_t n, int n_scans, int k, int32_t* ids_out,
                        uint16_t* loc_out, uint16_t* own_pos, uint16_t* row_seg, uint8_t* row_scan, int32_t* info, hipStream_t stream) {
  if (!fwd || fwd->layout != DC_TABLE_SLOTS || !fwd->blk_ptr || !fwd->blk_ids || !fwd->slot_ptr || !fwd->loc || !fwd->own_base) return DC_ERR_ARG;
  if (n < 1 || n_scans < 1 || n_scans > kMaxBlockScans || !ids_out || !loc_out || !own_pos || !row_seg || !row_scan || !info) return DC_ERR_ARG;
  if (k != 4 && k != 8 && k != 10 && k != 16) return DC_ERR_UNSUPPORTED;
  hipError_t err = hipMemsetAsync(info, 0, sizeof(int32_t), stream);
  if (err != hipSuccess) return (int)err;
  BlockTab tab{fwd->blk_ptr, fwd->blk_ids, fwd->slot_ptr, fwd->loc};
  const dim3 grid((unsigned)n_blocks(n)), block(kBlock);
#define PT_K(KK) hipLaunchKernelGGL((pose_table_kernel<KK>), grid, block, 0, stream, tab, fwd->own_base, scan_id, n, n_scans, ids_out, loc_out, own_pos, \
                                    row_seg, row_scan, info)
  if (k == 10) PT_K(10); else if (k == 4) PT_K(4); else if (k == 8) PT_K(8); else PT_K(16);
#undef PT_K
  DC_CHECK_LAUNCH();
  return DC_OK;
}

// `reduce` = false leaves the block partials in partials_ws for a later combined reduction (dc_sequence_eval).
static int consistency_fwd_impl(const void* points, int stride, int dtype, int point_fmt, const double* qparams,
                                const int32_t* nbr, const int32_t* centre_idx, const dcBlockTable* table, int64_t n, int k,
                                const uint8_t* mask,
                                const void* offset, int loss_kind,
                                int normalization, int sqrt_, void* rec, void* pointwise, void* eigvals, double* partials_ws,
                                double* sums_out, hipStream_t stream, bool reduce) {
  if (n == 0 && sums_out) return (int)hipMemsetAsync(sums_out, 0, 2 * sizeof(double), stream);
  if (n < 0 || k < 1 || !points || !partials_ws || !sums_out || (stride != 3 && stride != 4)) return DC_ERR_ARG;
  if ((loss_kind & 0xFF) != DC_LOSS_MIN_EIGVAL && (loss_kind & 0xFF) != DC_LOSS_TRACE) return DC_ERR_ARG;
  if (loss_kind & ~(0xFF | DC_LOSS_RAW_POINTWISE | DC_LOSS_SKIP_NANS | DC_LOSS_ONLY_FINITE)) return DC_ERR_ARG;
  BlockTab tab{};
  size_t lds_bytes = 0;
  int lds_rows = 0;
  const bool staged = use_table(table, g_no_tab.load(), DC_TABLE_SLOTS, stride, point_fmt == DC_F64 ? 32u : 16u, 0, 60 * 1024, &lds_bytes, &lds_rows);
  if (staged) tab = BlockTab{table->blk_ptr, table->blk_ids, table->slot_ptr, table->loc};
  const int fixed_k = g_fwd_generic.load() ? 0 : k;        // a table of [rows, k] has k slots in every block
  if (!staged && !nbr) return table ? DC_ERR_UNSUPPORTED : DC_ERR_ARG;
  QParams qp;
  int rc = make_qparams(point_fmt, dtype, stride, qparams, &qp);
  if (rc) return rc;
  if (n == 0) return (int)hipMemsetAsync(sums_out, 0, 2 * sizeof(double), stream);
  const LossParams lp = make_loss_params(loss_kind, normalization, sqrt_);
  const int64_t rows = xcd_grid(n_blocks(n));
  dim3 grid((unsigned)rows), block(kBlock);
#define FWD_ARGS(T, PT) (const PT*)points, nbr, centre_idx, n, k, mask, (const T*)offset, lp, qp, (PT*)rec, (T*)pointwise, (T*)eigvals, partials_ws
#define FWD_STAGED_ARGS(T, PT) (const PT*)points, tab, lds_rows, centre_idx, n, mask, (const T*)offset, lp, qp, (PT*)rec, (T*)pointwise, (T*)eigvals, partials_ws
#define DC_SWITCH_EIG(M, ...) do { if (eigvals) M(true, __VA_ARGS__); else M(false, __VA_ARGS__); } while (0)
#define FWD_FIXED(EIG, T, PT, NS) DC_TIMED_LAUNCH((consistency_fwd_fixed_kernel<T, PT, EIG, NS>), grid, block, lds_bytes, stream, FWD_STAGED_ARGS(T, PT))
#define FWD_STAGED(EIG, T, PT) DC_TIMED_LAUNCH((consistency_fwd_staged_kernel<T, PT, EIG>), grid, block, lds_bytes, stream, FWD_STAGED_ARGS(T, PT))
#define FWD_GATHER(EIG, T, PT, S) DC_TIMED_LAUNCH((consistency_fwd_kernel<T, PT, S, EIG>), grid, block, 0, stream, FWD_ARGS(T, PT))
#define FWD_FIXED_K(NS, T, PT) DC_SWITCH_EIG(FWD_FIXED, T, PT, NS)
#define LAUNCH(T, PT, S) \
  do { \
    if (S == 4 && staged) DC_SWITCH_K(fixed_k, DC_SWITCH_EIG(FWD_STAGED, T, PT), FWD_FIXED_K, T, PT);   /* padded rows + block table: gathers served from LDS */ \
    else DC_SWITCH_EIG(FWD_GATHER, T, PT, S); \
  } while (0)
  { ProfScope prof(1); DC_DISPATCH_FMT(dtype, point_fmt, stride, LAUNCH); }
#undef LAUNCH
#undef FWD_FIXED_K
#undef FWD_GATHER
#undef FWD_STAGED
#undef FWD_FIXED
#undef DC_SWITCH_EIG
  DC_CHECK_LAUNCH();
  if (!reduce) return DC_OK;
  hipLaunchKernelGGL(reduce_partials_kernel, dim3(2), dim3(kRedBlock), 0, stream, partials_ws, rows * kWavesPerBlock, sums_out);
  DC_CHECK_LAUNCH();
  return DC_OK;
}

int dc_consistency_fwd(const void* points, int stride, int dtype, int point_fmt, const double* qparams,
                       const int32_t* nbr, const int32_t* centre_idx, const dcBlockTable* table, int64_t n, int k,
                       const uint8_t* mask, const void* offset, int loss_kind, int normalization, int sqrt_, void* rec,
                       void* pointwise, void* eigvals, double* partials_ws, double* sums_out, hipStream_t stream) {
  return consistency_fwd_impl(points, stride, dtype, point_fmt, qparams, nbr, centre_idx, table, n, k, mask, offset, loss_kind, normalization,
                              sqrt_, rec, pointwise, eigvals, partials_ws, sums_out, stream, true);
}

static int consistency_bwd_impl(const void* points, int stride, int dtype, int point_fmt, const double* qparams, const void* rec,
                                const int32_t* csr_ptr, const int32_t* csr_src, const uint8_t* lane_perm,
                                const dcBlockTable* table, int64_t n,
                                const void* vps, const void* dirs, const void* depth, const void* inc, const uint8_t* lmask,
                                const int32_t* scan_id, const double* poses, int n_scans, int model_kind, int n_terms,
                                const double* w, const double* e, int want_exponent_grad, int want_pose_grad,
                                void* grad_points, double* partials_ws, double* grads_out, hipStream_t stream, bool reduce,
                                int64_t rec_rows, const uint16_t* scan_seg = nullptr) {
  if (n < 0 || !points || !rec || (stride != 3 && stride != 4)) return DC_ERR_ARG;
  BlockTab tab{};
  RunTab rtab{};
  size_t lds_bytes = 0;
  int lds_rows = 0;
  // the pose variants hold up to 16 KB of static LDS for the per-scan sums: staged records within 44 KB fit the default 64 KB of a
  // workgroup; longer lists (ball neighbourhoods: 1 500 centres reference a block at r = 0.4 m) take the run kernel with a larger
  // dynamic allocation (hipFuncSetAttribute below) -- one or two blocks per CU, but gathers from LDS: un-staged, the backward of the
  // r = 0.4 m table took 535 us
  const uint32_t rec_row = point_fmt == DC_F64 ? 64u : 32u;
  const bool no_tab = g_no_tab.load();
  const bool by_runs = !lane_perm && use_table(table, no_tab, DC_TABLE_RUNS, stride, rec_row, 1, 128 * 1024, &lds_bytes, &lds_rows);
  const bool staged = by_runs || (!lane_perm && use_table(table, no_tab, DC_TABLE_SLOTS, stride, rec_row, 1, 44 * 1024, &lds_bytes, &lds_rows));
  if (by_runs) rtab = RunTab{table->blk_ptr, table->blk_ids, table->run_ptr, table->loc};
  else if (staged) tab = BlockTab{table->blk_ptr, table->blk_ids, table->slot_ptr, table->loc};
  if (!staged && (!csr_ptr || !csr_src)) return table ? DC_ERR_UNSUPPORTED : DC_ERR_ARG;
  const bool params = dirs != nullptr;
  if (!params && !grad_points) return DC_ERR_ARG;
  if (params) {
    if (!depth || !partials_ws || !grads_out) return DC_ERR_ARG;
    if (scan_id && (!poses || n_scans < 1)) return DC_ERR_ARG;
    if (want_pose_grad && n_scans < 1) return DC_ERR_ARG;
    int rc = check_model(model_kind, n_terms, inc, w, e);
    if (rc) return rc;
  }
  QParams qp;
  int rc = make_qparams(point_fmt, dtype, stride, qparams, &qp);
  if (rc) return rc;
  if (model_kind == DC_MODEL_NONE) n_terms = 0;
  const int n_acc = 2 * n_terms + 12 * n_scans;
  if (n == 0) return params ? (int)hipMemsetAsync(grads_out, 0, n_acc * sizeof(double), stream) : DC_OK;
  PointInputs in = make_inputs(vps, dirs, depth, inc, lmask, scan_id, poses, n_scans, model_kind, n_terms, w, e);
  // points grouped by scan inside every block (the plan's layout): per-scan pose sums over static lane ranges -- for the
  // kernels whose lanes are the plan's points in order (not with a lane map), and while a block's scans fit the item loop
  const bool grouped = scan_seg && want_pose_grad && !lane_perm && n_scans <= kMaxBlockScans && !reduce && params;   // (the caller's reduction knows the row-major pose rows)
  in.seg_start = grouped ? scan_seg : nullptr;
  const int64_t rows = xcd_grid(n_blocks(n));
  const int64_t prows = rows * kWavesPerBlock;               // partial rows: one per wavefront
  dim3 grid((unsigned)rows), block(kBlock);
  // byte size of the record array for the buffer resource (rows <= n; a compact centre list has fewer)
  const uint64_t rec_total = (uint64_t)(rec_rows > 0 ? rec_rows : n) * (point_fmt == DC_F64 ? 64u : 32u);
  if (rec_total >= (1ull << 32)) return DC_ERR_UNSUPPORTED;
  const uint32_t rec_bytes = (uint32_t)rec_total;
  const int n_red = want_pose_grad ? n_acc : 2 * n_terms;       // slots the kernel produces
  if (params && want_pose_grad && !grouped) {               // (the grouped reduction writes every pose slot of every row itself)
    hipError_t err = hipMemsetAsync(partials_ws + (size_t)prows * 2 * n_terms, 0, (size_t)prows * 12 * n_scans * sizeof(double), stream);
    if (err != hipSuccess) return (int)err;
  }
  if (params && n_red < n_acc && reduce) {
    hipError_t err = hipMemsetAsync(grads_out + n_red, 0, (size_t)(n_acc - n_red) * sizeof(double), stream);
    if (err != hipSuccess) return (int)err;
  }
#define BWD_ARGS(T, PT) (const PT*)points, (const PT*)rec, csr_ptr, csr_src, lane_perm, n, in, qp, (T*)grad_points, partials_ws, n_acc, rec_bytes
#define BWD_STAGED_ARGS(T, PT) (const PT*)points, (const PT*)rec, tab, lds_rows, n, in, qp, (T*)grad_points, partials_ws, n_acc
#define BWD_RUNS_ARGS(T, PT) (const PT*)points, (const PT*)rec, rtab, lds_rows, n, in, qp, (T*)grad_points, partials_ws, n_acc
  // the four (WANT_E, WANT_POSE) instantiations of a backward kernel
#define DC_SWITCH_EP(M, ...) \
  do { if (want_pose_grad && want_exponent_grad) M(true, true, __VA_ARGS__); else if (want_pose_grad) M(false, true, __VA_ARGS__); \
       else if (want_exponent_grad) M(true, false, __VA_ARGS__); else M(false, false, __VA_ARGS__); } while (0)
#define BWD_RUNS(E, PO, T, PT) DC_TIMED_LAUNCH((consistency_bwd_runs_kernel<T, PT, E, PO>), grid, block, lds_bytes, stream, BWD_RUNS_ARGS(T, PT))
#define BWD_STAGED(E, PO, T, PT) DC_TIMED_LAUNCH((consistency_bwd_staged_kernel<T, PT, E, PO>), grid, block, lds_bytes, stream, BWD_STAGED_ARGS(T, PT))
#define BWD_GATHER(E, PO, T, PT, S) DC_TIMED_LAUNCH((consistency_bwd_kernel<T, PT, S, E, PO>), grid, block, 0, stream, BWD_ARGS(T, PT))
#define BWD_RUNS_LDS(E, PO, T, PT) e_ = hipFuncSetAttribute((const void*)consistency_bwd_runs_kernel<T, PT, E, PO>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes)
#define LAUNCH(T, PT, S) \
  do { \
    if (S == 4 && by_runs) DC_SWITCH_EP(BWD_RUNS, T, PT); \
    else if (S == 4 && staged) DC_SWITCH_EP(BWD_STAGED, T, PT); \
    else DC_SWITCH_EP(BWD_GATHER, T, PT, S); \
  } while (0)
  if (by_runs && lds_bytes > 44 * 1024) {
    int attr_rc = DC_OK;
#define BIG_LDS(T, PT, S) \
  do { \
    if (S == 4) { \
      hipError_t e_; \
      DC_SWITCH_EP(BWD_RUNS_LDS, T, PT); \
      if (e_ != hipSuccess) attr_rc = (int)e_; \
    } \
  } while (0)
    DC_DISPATCH_FMT(dtype, point_fmt, stride, BIG_LDS);
#undef BIG_LDS
    if (attr_rc) return attr_rc;
  }
  { ProfScope prof(2); DC_DISPATCH_FMT(dtype, point_fmt, stride, LAUNCH); }
#undef LAUNCH
#undef BWD_RUNS_LDS
#undef BWD_GATHER
#undef BWD_STAGED
#undef BWD_RUNS
#undef DC_SWITCH_EP
  DC_CHECK_LAUNCH();
  if (params && n_red > 0 && reduce) {
    hipLaunchKernelGGL(reduce_partials_kernel, dim3(n_red), dim3(kRedBlock), 0, stream, partials_ws, prows, grads_out);
    DC_CHECK_LAUNCH();
  }
  return DC_OK;
}

int dc_consistency_bwd(const void* points, int stride, int dtype, int point_fmt, const double* qparams, const void* rec,
                       const int32_t* csr_ptr, const int32_t* csr_src, const uint8_t* lane_perm, const dcBlockTable* table,
                       int64_t n, const void* vps, const void* dirs, const void* depth, const void* inc, const uint8_t* lmask,
                       const int32_t* scan_id, const double* poses, int n_scans, int model_kind, int n_terms, const double* w,
                       const double* e, int want_exponent_grad, int want_pose_grad, void* grad_points, double* partials_ws,
                       double* grads_out, hipStream_t stream) {
  return consistency_bwd_impl(points, stride, dtype, point_fmt, qparams, rec, csr_ptr, csr_src, lane_perm, table, n, vps, dirs, depth,
                              inc, lmask, scan_id, poses, n_scans, model_kind, n_terms, w, e, want_exponent_grad,
                              want_pose_grad, grad_points, partials_ws, grads_out, stream, true, 0);
}

int dc_points_bwd(const void* grad_points, const int32_t* perm, int stride, int dtype, int64_t n, const void* vps,
                  const void* dirs, const void* depth, const void* inc, const uint8_t* lmask, const int32_t* scan_id,
                  const double* poses, int n_scans, int model_kind, int n_terms, const double* w, const double* e,
                  int want_exponent_grad, int want_pose_grad, double* partials_ws, double* grads_out,
                  hipStream_t stream) {
  if (n < 0 || !grad_points || !dirs || !depth || !partials_ws || !grads_out || (stride != 3 && stride != 4))
    return DC_ERR_ARG;
  if (scan_id && (!poses || n_scans < 1)) return DC_ERR_ARG;
  int rc = check_model(model_kind, n_terms, inc, w, e);
  if (rc) return rc;
  if (model_kind == DC_MODEL_NONE) n_terms = 0;
  const int n_acc = 2 * n_terms + 12 * n_scans;
  if (n_acc == 0) return DC_OK;
  if (n == 0) return (int)hipMemsetAsync(grads_out, 0, n_acc * sizeof(double), stream);
  PointInputs in = make_inputs(vps, dirs, depth, inc, lmask, scan_id, poses, n_scans, model_kind, n_terms, w, e);
  const int64_t rows = n_blocks(n);
  const int64_t prows = rows * kWavesPerBlock;
  dim3 grid((unsigned)rows), block(kBlock);
  const int n_red = want_pose_grad ? n_acc : 2 * n_terms;
  if (n_red < n_acc) {
    hipError_t err = hipMemsetAsync(grads_out + n_red, 0, (size_t)(n_acc - n_red) * sizeof(double), stream);
    if (err != hipSuccess) return (int)err;
  }
  if (n_red == 0) return DC_OK;
  if (want_pose_grad) {      // blocks only write the pose slots of the scans they contain
    hipError_t err = hipMemsetAsync(partials_ws + (size_t)prows * 2 * n_terms, 0, (size_t)prows * 12 * n_scans * sizeof(double), stream);
    if (err != hipSuccess) return (int)err;
  }
#define LAUNCH(T, S) \
  hipLaunchKernelGGL((points_bwd_kernel<T, S>), grid, block, 0, stream, (const T*)grad_points, perm, n, in, \
                     want_exponent_grad, want_pose_grad, partials_ws, n_acc)
  if (dtype == DC_F32) { if (stride == 3) LAUNCH(float, 3); else LAUNCH(float, 4); }
  else if (dtype == DC_F64) { if (stride == 3) LAUNCH(double, 3); else LAUNCH(double, 4); }
  else return DC_ERR_DTYPE;
#undef LAUNCH
  DC_CHECK_LAUNCH();
  hipLaunchKernelGGL(reduce_partials_kernel, dim3(n_red), dim3(kRedBlock), 0, stream, partials_ws, prows, grads_out);
  DC_CHECK_LAUNCH();
  return DC_OK;
}

#ifdef DC_BLOCK_TRACE
int dc_debug_block_trace(void* buf) {        // diagnostic build only: [4 x grid] uint64 (or null to stop recording)
  unsigned long long* p = (unsigned long long*)buf;
  return (int)hipMemcpyToSymbol(HIP_SYMBOL(dc::g_block_trace), &p, sizeof(p));
}
#endif
// option 0: 1 = ignore block tables and gather from global memory (ablation / A-B measurements), 0 = default; the other options are
// listed at the switches above route_options and in dc_hip.h.
// The switches exist for A-B measurements and for the tests that hold one path against another; a process that has not asked for them
// (DC_ENABLE_ABLATIONS=1 in its environment when the library is first used) cannot change them: the product has no mutable
// process-wide state.
int dc_set_option(int option, int value) {
  static const bool enabled = [] { const char* e = getenv("DC_ENABLE_ABLATIONS"); return e && atoi(e) != 0; }();
  if (!enabled) return DC_ERR_UNSUPPORTED;
  if (option == 0) { g_no_tab.store(value != 0); return DC_OK; }
  if (option == 1) { g_fwd_generic.store(value); return DC_OK; }
  if (option == 3) { g_no_basis.store(value != 0); return DC_OK; }
  if (option == 4) { g_two_pass.store(value != 0); return DC_OK; }
  if (option == 5) { g_chain_spin.store(value < 0 ? (1 << 22) : value); return DC_OK; }
  if (option == 6) { g_step_var.store(value); return DC_OK; }
  if (option == 7) { g_pose_three_pass.store(value != 0); return DC_OK; }
  if (option == 8) { g_no_reverse.store(value != 0); return DC_OK; }
  if (option == 9) { g_step_six.store(value != 0); return DC_OK; }
  if (option == 10) { g_no_step_rows.store(value != 0); return DC_OK; }
  if (option == 11) { g_no_step_loc.store(value != 0); return DC_OK; }
  return DC_ERR_ARG;
}

// ---- profiler control ---------------------------------------------------------------------------------------
int dc_profiler_enable(int every) {
  std::lock_guard<std::mutex> lock(g_prof.mu);
  g_prof.every = every < 0 ? 0 : every;
  return DC_OK;
}
int dc_profiler_reset(void) {
  std::lock_guard<std::mutex> lock(g_prof.mu);
  for (int k = 0; k < kProfKinds; ++k) { g_prof.count[k] = 0; g_prof.seen[k] = 0; }
  return DC_OK;
}
// Source-level name of the kernel instantiation the last launch of `kind` used, e.g.
// "(consistency_fwd_fixed_kernel<float, q32, false, 10>)"; empty before the first launch.
int dc_profiler_kernel(int kind, char* buf, int len) {
  if (kind < 0 || kind >= kProfKinds || !buf || len < 1) return DC_ERR_ARG;
  const char* nm = g_prof.last_kernel[kind];
  snprintf(buf, (size_t)len, "%s", nm ? nm : "");
  return DC_OK;
}
// kind: 0 points_fwd, 1 consistency_fwd, 2 consistency_bwd, 3 features_fwd.  Waits for the recorded launches to finish.
int dc_profiler_read(int kind, double* total_ms, int64_t* launches) {
  if (kind < 0 || kind >= kProfKinds || !total_ms || !launches) return DC_ERR_ARG;
  double tot = 0.0;
  int n;
  { std::lock_guard<std::mutex> lock(g_prof.mu); n = g_prof.count[kind]; }
  for (int i = 0; i < n; ++i) {
    hipError_t err = hipEventSynchronize(g_prof.stop[kind][i]);
    if (err != hipSuccess) return (int)err;
    float ms = 0.f;
    err = hipEventElapsedTime(&ms, g_prof.start[kind][i], g_prof.stop[kind][i]);
    if (err != hipSuccess) return (int)err;
    tot += ms;
  }
  *total_ms = tot;
  *launches = n;
  return DC_OK;
}

static int make_adam(double* param, double* exp_avg, double* exp_avg_sq, int64_t n, int64_t step, double grad_scale, double lr,
                     double beta1, double beta2, double eps, double weight_decay, AdamArgs* a) {
  if (!param || !exp_avg || !exp_avg_sq || n < 0 || n > 0x7fffffff || step < 1) return DC_ERR_ARG;
  *a = AdamArgs{param, exp_avg, exp_avg_sq, (int)n, grad_scale, lr, beta1, beta2, eps, weight_decay,
                1.0 - pow(beta1, (double)step), sqrt(1.0 - pow(beta2, (double)step))};
  return DC_OK;
}

int dc_adam_step(double* param, const double* grad, double* exp_avg, double* exp_avg_sq, int64_t n, int64_t step,
                 double grad_scale, double lr, double beta1, double beta2, double eps, double weight_decay,
                 hipStream_t stream) {
  AdamArgs a;
  int rc = make_adam(param, exp_avg, exp_avg_sq, n, step, grad_scale, lr, beta1, beta2, eps, weight_decay, &a);
  if (rc || !grad) return rc ? rc : DC_ERR_ARG;
  if (n == 0) return DC_OK;
  hipLaunchKernelGGL(adam_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, stream, grad, a);
  DC_CHECK_LAUNCH();
  return DC_OK;
}

int dc_adam_step_device(double* param, const double* grad, double* exp_avg, double* exp_avg_sq, int64_t n, int64_t* step,
                        double grad_scale, double lr, double beta1, double beta2, double eps, double weight_decay,
                        hipStream_t stream) {
  AdamArgs a;
  int rc = make_adam(param, exp_avg, exp_avg_sq, n, 1, grad_scale, lr, beta1, beta2, eps, weight_decay, &a);
  if (rc || !grad || !step) return rc ? rc : DC_ERR_ARG;
  hipLaunchKernelGGL(adam_device_step_kernel, dim3(1), dim3(256), 0, stream, grad, a, step);
  DC_CHECK_LAUNCH();
  return DC_OK;
}

// One evaluation of a whole sequence (eval.py:85-112 + backward) from a caller-filled descriptor: dc_choose_route (dc_cons_route.h)
// decides which kernels run, the launch functions below run them.  out fp64 [2 + 2 P + 12 S] = {sum loss over mask, mask count, grads
// of the sum}.
// a chained step (dc_sequence_step_chained): this launch also finishes the previous evaluation (StepChain)
struct ChainCall {
  int32_t* ready;
  int parity, has_prev;
  double* out_prev;
  AdamArgs adam_prev;
  const double* grad_sum;    // nullptr: the previous evaluation's rows are summed by this launch
  bool reduce_now;           // also launch the ordinary reduction of THIS evaluation's rows into `out` (no Adam)
  double* w_prev_out = nullptr;
  uint32_t stamp = 0;        // the launch's number (its step): marks the weights it publishes
  const double* prev_rows = nullptr;   // linked chains: the PREVIOUS launch's partial rows when that was another sequence's (else this
  int64_t prev_count = 0;              // sequence's other buffer), how many there are, and the running sums they are added to
  const double* acc_in = nullptr;
  const int32_t* prev_status = nullptr;
};
// the two partial-row buffers of a chain: behind the columns ordinary evaluations use, so that an evaluation of the same
// sequence between two chained steps (a validation pass, a lazily produced loss cloud) cannot overwrite a pending step
static inline double* chain_buffer(const dcSequenceDesc* d, int n_terms, int parity) {
  const int64_t rows = route_seq_rows(d).rows;
  const int n_acc = 2 * n_terms + 12 * d->n_scans;
  return d->partials + (int64_t)(2 + n_acc) * rows + (int64_t)parity * (2 + n_terms) * rows;
}
// what the leading blocks of a chained launch (or of the flush of a linked chain) need; the previous launch's rows are the call's
// own (linked chains) or `own_prev`
static StepChain make_chain(const ChainCall& c, int n_out, const double* own_prev, int64_t own_rows, int32_t* status, int spin_limit,
                            const double* w_now, int reverse) {
  StepChain ch{};
  ch.ready = c.ready; ch.stamp = c.stamp; ch.parity = c.parity; ch.has_prev = c.has_prev; ch.n_front = kChainFront; ch.n_out = n_out;
  ch.reverse = reverse;
  ch.prev = c.prev_rows ? c.prev_rows : own_prev; ch.prev_rows = c.prev_rows ? c.prev_count : own_rows;
  ch.grad_sum = c.grad_sum; ch.out_prev = c.out_prev; ch.w_prev_out = c.w_prev_out; ch.status = status; ch.spin_limit = spin_limit;
  ch.w_now = w_now; ch.prev_status = c.prev_status; ch.acc_in = c.acc_in; ch.adam = c.adam_prev;
  return ch;
}

// ---- the one-pass step kernels: what every launch takes, and one launch function per route kind ----------------------------------
struct StepLaunch {
  const dcSequenceDesc* d; hipStream_t stream; dim3 grid; PointBasis pb; BlockTab tab; LossParams lp; QParams qp; double *p_fwd, *p_bwd; StepChain ch;
};

// ball neighbourhoods on float32 clouds: the tile may take up to 128 KB of LDS (ragged_launch)
static int launch_step_ragged(const SeqRoute& r, const StepLaunch& a) {
  ProfScope prof(1);
#define RAGGED(P, CAP) (prof.name("(consistency_step_ragged_q32_kernel<" #P ", " #CAP ">)"), \
                        ragged_launch<P, CAP>(a.grid, a.stream, prof.start(), prof.stop(), a.pb, a.tab, r.table, r.n_rows, a.d->mask, a.lp, a.qp, a.p_fwd, a.p_bwd, a.ch))
#define RAGGED_CAPS(P, X) do { switch (r.cap) { case 1024: return RAGGED(P, 1024); case 1280: return RAGGED(P, 1280); case 1600: return RAGGED(P, 1600); \
                                                case 2048: return RAGGED(P, 2048); case 2560: return RAGGED(P, 2560); default: return RAGGED(P, 4096); } } while (0)
  DC_SWITCH_P(r.P, switch (r.cap) { case 1024: return RAGGED(3, 1024); case 1600: return RAGGED(3, 1600); default: return RAGGED(3, 2560); }, RAGGED_CAPS, 0);
#undef RAGGED_CAPS
#undef RAGGED
  return DC_OK;
}

// float32 clouds with a [rows, K] table and block headers: fp64 row differences in a static LDS tile
static int launch_step_q32(const SeqRoute& r, const StepLaunch& a) {
  ProfScope prof(1);
  const StepHdr* hdr = static_cast<const StepHdr*>(a.d->step_hdr);
  // the per-block row copy belongs to the same table as the headers (the route is here because of them): staged from when the caller
  // passes one, unless dc_set_option(10, 1) asks for the trip through blk_ids
  const int32_t* step_rows = g_no_step_rows.load() ? nullptr : static_cast<const int32_t*>(a.d->step_rows);
  // so do the packed tile positions (dc_set_option(11, 1): the table's loc)
  const uint32_t* step_loc = g_no_step_loc.load() ? nullptr : static_cast<const uint32_t*>(a.d->step_loc);
  const dim3 block(kBlock);
  static_assert(kStepQ32Cap == 512, "the profiler names the instantiation by its literal arguments");
  static_assert(step_q32_blocks<1, 512>() == 7 && step_q32_blocks<2, 512>() == 7 && step_q32_blocks<3, 512>() == 6 && step_q32_blocks<2, 768>() == 6,
                "which instantiations dc_set_option(9, 1) has a six-block build of");
#define STEPQ_TAIL a.pb, a.tab, hdr, step_rows, step_loc, a.d->centre_idx, r.n_rows, a.lp, a.qp, a.p_fwd, a.p_bwd, a.ch
#define STEPQ(P, NS, CAP) DC_TIMED_LAUNCH((consistency_step_q32_kernel<NS, P, CAP>), a.grid, block, 0, a.stream, STEPQ_TAIL)
#define STEPQ_SIX(P, NS, X) DC_TIMED_LAUNCH((consistency_step_q32_kernel<NS, P, 512, 6>), a.grid, block, 0, a.stream, STEPQ_TAIL)
#define STEPQ_P(NS, CAP) DC_SWITCH_P(r.P, STEPQ(3, NS, CAP), STEPQ, NS, CAP)
#define STEPQ_SIX_P(NS, X) DC_SWITCH_P(r.P, , STEPQ_SIX, NS, X)
  if (r.six) DC_SWITCH_K(r.k, , STEPQ_SIX_P, 0);             // (dc_set_option(9, 1): the six-blocks-per-CU build of the instantiations whose default is seven)
  else if (r.cap == 512) DC_SWITCH_K(r.k, , STEPQ_P, 512);
  else DC_SWITCH_K(r.k, , STEPQ_P, 768);
#undef STEPQ_SIX_P
#undef STEPQ_P
#undef STEPQ_SIX
#undef STEPQ
#undef STEPQ_TAIL
  return DC_OK;
}

// any [rows, K] table (float64 clouds; float32 ones without headers, with longer lists or under dc_set_option(6, ..)): the tables themselves
#define STEP_TAIL a.pb, a.tab, r.table->own_base, r.rows_fwd, a.d->centre_idx, r.n_rows, a.d->mask, a.lp, a.qp, a.p_fwd, a.p_bwd, a.ch
// the dynamic LDS of a launch: the tile, which in a chain also carries the hand-over of step_block_row (a tile of a few rows is smaller)
static size_t step_lds(const SeqRoute& r, const StepLaunch& a, size_t hand_bytes) {
  return a.ch.ready && r.lds_fwd < hand_bytes ? hand_bytes : r.lds_fwd;
}
static int launch_step_basis(const SeqRoute& r, const StepLaunch& a) {
  ProfScope prof(1);
  const dim3 block(kBlock);
#define STEPB(P, NS, PT) DC_TIMED_LAUNCH((consistency_step_basis_kernel<PT, NS, P, kStepVar>), a.grid, block, step_lds(r, a, step_hand_bytes<P>()), a.stream, STEP_TAIL)
#define STEPB_P(NS, PT) DC_SWITCH_P(r.P, STEPB(3, NS, PT), STEPB, NS, PT)
  if (r.round2 && r.f64) DC_TIMED_LAUNCH((consistency_step_basis_kernel<double, 10, 2, 0>), a.grid, block, step_lds(r, a, step_hand_bytes<2>()), a.stream, STEP_TAIL);
  else if (r.round2) DC_TIMED_LAUNCH((consistency_step_basis_kernel<q32, 10, 2, 0>), a.grid, block, step_lds(r, a, step_hand_bytes<2>()), a.stream, STEP_TAIL);
  else if (r.f64) DC_SWITCH_K(r.k, , STEPB_P, double);
  else DC_SWITCH_K(r.k, , STEPB_P, q32);
#undef STEPB_P
#undef STEPB
  return DC_OK;
}

// any other slot count: the run-time slot loop
static int launch_step_slots(const SeqRoute& r, const StepLaunch& a) {
  ProfScope prof(1);
  const dim3 block(kBlock);
#define STEPS(P, PT, X) DC_TIMED_LAUNCH((consistency_step_basis_slots_kernel<PT, P>), a.grid, block, step_lds(r, a, step_hand_bytes<P>()), a.stream, STEP_TAIL, r.table->packed)
  if (r.f64) DC_SWITCH_P(r.P, STEPS(3, double, 0), STEPS, double, 0);
  else DC_SWITCH_P(r.P, STEPS(3, q32, 0), STEPS, q32, 0);
#undef STEPS
  return DC_OK;
}
#undef STEP_TAIL

// loss and dL/dw in ONE pass (forward-mode) for up to three weights: no record, no backward launch, no transposed table; a chained
// launch first finishes the evaluation before it
static int run_one_pass(const SeqRoute& r, const dcSequenceDesc* d, const double* w, double* out, hipStream_t stream, const AdamArgs& adam,
                        const ChainCall* chain) {
  StepLaunch a{};
  int rc = make_qparams(d->point_fmt, d->dtype, 4, d->qparams, &a.qp);
  if (rc) return rc;
  a.d = d; a.stream = stream; a.grid = dim3((unsigned)r.grid);
  a.pb = PointBasis{d->basis, w, r.n_terms, r.f64 ? 1.0 : a.qp.inv_scale};
  a.lp = make_loss_params(d->loss_kind & ~DC_LOSS_RAW_POINTWISE, d->normalization, d->sqrt_);
  a.tab = BlockTab{r.table->blk_ptr, r.table->blk_ids, r.table->slot_ptr, r.table->loc};
  a.p_fwd = chain ? chain_buffer(d, r.n_terms, chain->parity) : d->partials;
  a.p_bwd = chain ? a.p_fwd + 2 * r.g_blocks : d->partials + 2 * r.rows;
  if (chain) a.ch = make_chain(*chain, 2 + r.n_acc, chain_buffer(d, r.n_terms, chain->parity ^ 1), r.g_blocks, d->status, g_chain_spin.load(), w,
                               (chain->parity && !g_no_reverse.load()) ? 1 : 0);
  a.ch.blk_skip = (d->mask && !d->centre_idx) ? d->blk_skip : nullptr;
  switch (r.kind) {
    case ROUTE_STEP_RAGGED: rc = launch_step_ragged(r, a); break;
    case ROUTE_STEP_Q32: rc = launch_step_q32(r, a); break;
    case ROUTE_STEP_BASIS: rc = launch_step_basis(r, a); break;
    default: rc = launch_step_slots(r, a); break;
  }
  if (rc) return rc;
  DC_CHECK_LAUNCH();
  // a chain's sums are taken by its next launch, or by the flush; with several ranks this evaluation's sums are wanted now as well
  // (they go through an all-reduce next)
  if (chain && !chain->reduce_now) return DC_OK;
  const int64_t rows_g = chain ? r.g_blocks : r.grid * kWavesPerBlock;
  hipLaunchKernelGGL(reduce_eval_kernel, dim3(2 + r.n_terms), dim3(kRedBlock), 0, stream, a.p_fwd, a.p_bwd, rows_g, rows_g, r.n_terms, 2 + r.n_acc, out,
                     chain ? AdamArgs{} : adam, (const int32_t*)d->status);
  DC_CHECK_LAUNCH();
  return DC_OK;
}

// the basis form with separate forward and backward kernels (forward only: a loss without gradients)
static int run_two_pass(const SeqRoute& r, const dcSequenceDesc* d, const double* w, int want_grad, double* out, hipStream_t stream,
                        const AdamArgs& adam) {
  QParams qp;
  int rc = make_qparams(d->point_fmt, d->dtype, 4, d->qparams, &qp);
  if (rc) return rc;
  const PointBasis pb{d->basis, w, r.n_terms, r.f64 ? 1.0 : qp.inv_scale};
  const LossParams lp = make_loss_params(d->loss_kind & ~DC_LOSS_RAW_POINTWISE, d->normalization, d->sqrt_);
  const BlockTab tab{r.table->blk_ptr, r.table->blk_ids, r.table->slot_ptr, r.table->loc};
  const dim3 block(kBlock);
  double *p_fwd = d->partials, *p_bwd = d->partials + 2 * r.rows;
  {
    ProfScope prof(1);
    const dim3 grid((unsigned)r.g_blocks);
#define FWDB_TAIL(PT, T) pb, tab, r.table->own_base, r.rows_fwd, d->centre_idx, r.n_rows, d->mask, (const T*)nullptr, lp, qp, \
                         (PT*)(want_grad ? d->rec : nullptr), (T*)nullptr, (T*)nullptr, p_fwd
#define FWDB(P, NS, PT, T) DC_TIMED_LAUNCH((consistency_fwd_basis_kernel<PT, false, NS, P>), grid, block, r.lds_fwd, stream, FWDB_TAIL(PT, T))
#define FWDB_SLOTS(P, PT, T) DC_TIMED_LAUNCH((consistency_fwd_basis_slots_kernel<PT, false, P>), grid, block, r.lds_fwd, stream, FWDB_TAIL(PT, T))
#define FWDB_P(NS, PT, T) DC_SWITCH_P(r.P, if (r.P == 3) FWDB(3, NS, PT, T); else FWDB(0, NS, PT, T), FWDB, NS, PT, T)
#define FWDB_SLOTS_P(PT, T) DC_SWITCH_P(r.P, if (r.P == 3) FWDB_SLOTS(3, PT, T); else FWDB_SLOTS(0, PT, T), FWDB_SLOTS, PT, T)
    if (r.f64) DC_SWITCH_K(r.k, FWDB_SLOTS_P(double, double), FWDB_P, double, double);
    else DC_SWITCH_K(r.k, FWDB_SLOTS_P(q32, float), FWDB_P, q32, float);
#undef FWDB_SLOTS_P
#undef FWDB_P
#undef FWDB_SLOTS
#undef FWDB
#undef FWDB_TAIL
  }
  DC_CHECK_LAUNCH();
  if (want_grad) {
    const RunTab rtab{d->bwd_table->blk_ptr, d->bwd_table->blk_ids, d->bwd_table->run_ptr, d->bwd_table->loc};
    const dim3 grid((unsigned)(r.rows / kWavesPerBlock));
    ProfScope prof(2);
#define BWDB(P, PT, X) DC_TIMED_LAUNCH((consistency_bwd_basis_kernel<PT, P>), grid, block, r.lds_bwd, stream, pb, (const PT*)d->rec, rtab, r.rows_bwd, d->n, qp, p_bwd)
    if (r.f64) DC_SWITCH_P(r.P, if (r.P == 3) BWDB(3, double, 0); else BWDB(0, double, 0), BWDB, double, 0);
    else DC_SWITCH_P(r.P, if (r.P == 3) BWDB(3, q32, 0); else BWDB(0, q32, 0), BWDB, q32, 0);
#undef BWDB
    DC_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(reduce_eval_kernel, dim3(2 + r.n_red), dim3(kRedBlock), 0, stream, p_fwd, p_bwd, r.g_blocks * kWavesPerBlock, r.rows, r.n_red,
                     2 + r.n_acc, out, adam, (const int32_t*)d->status);
  DC_CHECK_LAUNCH();
  return DC_OK;
}

// pose gradients (no exponent gradients) of a float32 sequence with a [rows, K] table: everything in ONE launch
// (consistency_step_pose_kernel) when the plan has built the pose tables and the local basis rows for these exponents
static int run_pose(const SeqRoute& r, const dcSequenceDesc* d, const double* w, const double* poses, double* out, hipStream_t stream,
                    const AdamArgs& adam) {
  QParams qp;
  int rc = make_qparams(d->point_fmt, d->dtype, 4, d->qparams, &qp, d->status);
  if (rc) return rc;
  const dcPoseTable* pt = d->pose_table;
  const PoseTab tab{pt->blk_ptr, pt->ids, pt->loc, pt->own_pos, pt->row_seg, pt->row_scan};
  const LossParams lp = make_loss_params(d->loss_kind & ~DC_LOSS_RAW_POINTWISE, d->normalization, d->sqrt_);
  const int64_t rows_b = r.rows / kWavesPerBlock;            // one row per block, every column contiguous
  const dim3 grid((unsigned)rows_b), block(kBlock);
  double *p_fwd = d->partials, *p_bwd = d->partials + 2 * r.rows;
  {
    ProfScope prof(1);
#define POSE(P, NS, X) DC_TIMED_LAUNCH((consistency_step_pose_kernel<NS, P>), grid, block, 0, stream, (const int32_t*)d->local_basis, tab, poses, d->n_scans, \
                                       w, d->n, d->mask, lp, qp, p_fwd, p_bwd)
#define POSE_P(NS, X) DC_SWITCH_P(r.P, , POSE, NS, X)
    DC_SWITCH_K(r.k, , POSE_P, 0);
#undef POSE_P
#undef POSE
  }
  DC_CHECK_LAUNCH();
  hipLaunchKernelGGL(reduce_eval_kernel, dim3(2 + r.n_acc), dim3(kRedBlock), 0, stream, p_fwd, p_bwd, rows_b, rows_b, r.n_acc, 2 + r.n_acc, out, adam,
                     (const int32_t*)d->status, -1, 0);
  DC_CHECK_LAUNCH();
  return DC_OK;
}

// points, forward, backward: three kernels (+ the fixed-order reduction)
// (measured in round 4 and dropped: a forward that FORMS the rows it stages from the raw inputs -- model, pose, ray end point per
// staged row, the owning block writing x for the backward -- instead of dc_points_fwd + a forward over x.  It removes a 22 us launch
// and 48 B per point of traffic, but a block stages 1.47 rows per point and each costs five scattered loads and ~80 fp64
// instructions in front of the staging barrier: 106 us against 22 + 46.)
static int run_general(const SeqRoute& r, const dcSequenceDesc* d, const double* w, const double* e, const double* poses, int want_grad,
                       int want_exponent_grad, int want_pose_grad, double* out, hipStream_t stream, const AdamArgs& adam) {
  const int stride = 4;
  double *p_fwd = d->partials, *p_bwd = d->partials + 2 * r.rows;
  int rc = dc_points_fwd(d->vps, d->dirs, d->depth, d->inc, d->lmask, d->scan_id, poses, d->n_scans, d->model_kind,
                         d->n_terms, w, e, d->n, d->dtype, d->point_fmt, d->qparams, stride, d->x, nullptr, nullptr,
                         nullptr, d->status, stream);
  if (rc) return rc;
  rc = consistency_fwd_impl(d->x, stride, d->dtype, d->point_fmt, d->qparams, d->nbr, d->centre_idx, d->fwd_table, r.n_rows, d->k, d->mask,
                            nullptr, d->loss_kind, d->normalization, d->sqrt_, want_grad ? d->rec : nullptr, nullptr, nullptr, p_fwd, out, stream,
                            false);
  if (!rc && want_grad)
    rc = consistency_bwd_impl(d->x, stride, d->dtype, d->point_fmt, d->qparams, d->rec, d->csr_ptr, d->csr_src, d->lane_perm,
                              d->bwd_table, d->n, d->vps, d->dirs, d->depth, d->inc, d->lmask, d->scan_id, poses, d->n_scans, d->model_kind,
                              d->n_terms, w, e, want_exponent_grad, want_pose_grad, nullptr, p_bwd, out + 2, stream, false,
                              r.n_rows, d->scan_seg);
  if (rc) return rc;
  const int pose_first = r.grouped ? 2 * r.n_terms : -1;     // the grouped backward leaves the pose slots row-major, one row per block
  hipLaunchKernelGGL(reduce_eval_kernel, dim3(red_grid(r.n_red, pose_first, 12 * d->n_scans)), dim3(kRedBlock), 0, stream, p_fwd, p_bwd,
                     r.g_blocks * kWavesPerBlock, r.rows, r.n_red, 2 + r.n_acc, out, adam, (const int32_t*)d->status, pose_first, 12 * d->n_scans);
  DC_CHECK_LAUNCH();
  return DC_OK;
}

static int sequence_eval_impl(const dcSequenceDesc* d, const double* w, const double* e, const double* poses, int want_grad,
                              int want_exponent_grad, int want_pose_grad, double* out, hipStream_t stream,
                              const AdamArgs& adam, const ChainCall* chain = nullptr) {
  SeqRoute r;
  const int rc = dc_choose_route_call(d, w, poses, out, want_grad, want_exponent_grad, want_pose_grad, chain != nullptr, route_options(), &r);
  if (rc) return rc;
  switch (r.kind) {
    case ROUTE_EMPTY: return (int)hipMemsetAsync(out, 0, (size_t)(2 + r.n_acc) * sizeof(double), stream);
    case ROUTE_STEP_RAGGED: case ROUTE_STEP_Q32: case ROUTE_STEP_BASIS: case ROUTE_STEP_SLOTS: return run_one_pass(r, d, w, out, stream, adam, chain);
    case ROUTE_TWO_PASS: return run_two_pass(r, d, w, want_grad, out, stream, adam);
    case ROUTE_POSE: return run_pose(r, d, w, poses, out, stream, adam);
    default: return run_general(r, d, w, e, poses, want_grad, want_exponent_grad, want_pose_grad, out, stream, adam);
  }
}

int dc_consistency_gate(const void* raw_pointwise, int dtype, int point_fmt, const uint8_t* mask, int64_t n,
                        const double* threshold, int sqrt_, void* rec, double* partials_ws, double* sums_out,
                        hipStream_t stream) {
  if (n < 0 || !partials_ws || !sums_out || !threshold) return DC_ERR_ARG;
  if (n == 0) return (int)hipMemsetAsync(sums_out, 0, 2 * sizeof(double), stream);
  if (!raw_pointwise || !rec) return DC_ERR_ARG;
  const int64_t rows = xcd_grid(n_blocks(n));
  const dim3 grid((unsigned)rows), block(kBlock);
  if (point_fmt == DC_Q32 && dtype == DC_F32)
    hipLaunchKernelGGL((consistency_gate_kernel<float, q32>), grid, block, 0, stream, (const float*)raw_pointwise, mask, n, threshold, sqrt_, (q32*)rec, partials_ws);
  else if (point_fmt == DC_F32 && dtype == DC_F32)
    hipLaunchKernelGGL((consistency_gate_kernel<float, float>), grid, block, 0, stream, (const float*)raw_pointwise, mask, n, threshold, sqrt_, (float*)rec, partials_ws);
  else if (point_fmt == DC_F64 && dtype == DC_F64)
    hipLaunchKernelGGL((consistency_gate_kernel<double, double>), grid, block, 0, stream, (const double*)raw_pointwise, mask, n, threshold, sqrt_, (double*)rec, partials_ws);
  else
    return DC_ERR_DTYPE;
  DC_CHECK_LAUNCH();
  hipLaunchKernelGGL(reduce_partials_kernel, dim3(2), dim3(kRedBlock), 0, stream, partials_ws, rows * kWavesPerBlock, sums_out);
  DC_CHECK_LAUNCH();
  return DC_OK;
}

int dc_sequence_eval(const dcSequenceDesc* d, const double* w, const double* e, const double* poses, int want_grad,
                     int want_exponent_grad, int want_pose_grad, double* out, hipStream_t stream) {
  return sequence_eval_impl(d, w, e, poses, want_grad, want_exponent_grad, want_pose_grad, out, stream, AdamArgs{});
}

// Evaluation + optimiser step of the model weights in one host call (train.py:220-312 for a single sequence on this
// rank): the block of the final reduction that finishes dL/dw_i also applies torch.optim.Adam's update to w_i.
int dc_sequence_step(const dcSequenceDesc* d, double* w, const double* e, const double* poses, double* exp_avg,
                     double* exp_avg_sq, int64_t step, double grad_scale, double lr, double beta1, double beta2, double eps,
                     double weight_decay, double* out, hipStream_t stream) {
  if (!d || d->model_kind == DC_MODEL_NONE || d->n_terms < 1 || d->n == 0) return DC_ERR_ARG;
  AdamArgs a;
  int rc = make_adam(w, exp_avg, exp_avg_sq, d->n_terms, step, grad_scale, lr, beta1, beta2, eps, weight_decay, &a);
  if (rc) return rc;
  return sequence_eval_impl(d, w, e, poses, 1, 0, 0, out, stream, a);
}

// What the chained entry points share: the argument check, the ChainCall of launch `step` that finishes `has_prev` ? the launch before
// it : nothing, the previous launch's rows where they are another sequence's (linked_call) and -- `update` -- the Adam step `step - 1`
// its leading blocks take.
static int linked_call(const dcSequenceDesc* d_prev, int prev_parity, int finish, const double* acc_in, int n_terms, ChainCall* c);
static int chain_call(const dcSequenceDesc* d, double* w, double* exp_avg, double* exp_avg_sq, int64_t step, bool has_prev, bool update,
                      double grad_scale, double lr, double beta1, double beta2, double eps, double weight_decay, int32_t* ready, double* out_prev,
                      ChainCall* c, const dcSequenceDesc* d_prev = nullptr, int prev_parity = 0, int finish = 0, const double* acc_in = nullptr) {
  if (!d || d->model_kind == DC_MODEL_NONE || d->n_terms < 1 || d->n == 0 || !ready || !out_prev || step < 1) return DC_ERR_ARG;
  if (update && step < 2) return DC_ERR_ARG;
  *c = ChainCall{ready, (int)(step & 1), has_prev ? 1 : 0, out_prev, AdamArgs{}, nullptr, false};
  c->stamp = (uint32_t)step;
  const int rc = linked_call(d_prev, prev_parity, finish, acc_in, d->n_terms, c);
  if (rc || !update) return rc;
  return make_adam(w, exp_avg, exp_avg_sq, d->n_terms, step - 1, grad_scale, lr, beta1, beta2, eps, weight_decay, &c->adam_prev);
}

int dc_sequence_step_chained_rec(const dcSequenceDesc* d, double* w, const double* e, const double* poses, double* exp_avg,
                                 double* exp_avg_sq, int64_t step, int has_prev, double grad_scale, double lr, double beta1, double beta2,
                                 double eps, double weight_decay, int32_t* ready, double* out_prev, double* w_used_prev,
                                 hipStream_t stream) {
  ChainCall c;
  const int rc = chain_call(d, w, exp_avg, exp_avg_sq, step, has_prev != 0, has_prev != 0, grad_scale, lr, beta1, beta2, eps, weight_decay, ready,
                            out_prev, &c);
  if (rc) return rc;
  c.w_prev_out = has_prev ? w_used_prev : nullptr;
  return sequence_eval_impl(d, w, e, poses, 1, 0, 0, out_prev, stream, AdamArgs{}, &c);
}

int dc_sequence_step_chained(const dcSequenceDesc* d, double* w, const double* e, const double* poses, double* exp_avg,
                             double* exp_avg_sq, int64_t step, int has_prev, double grad_scale, double lr, double beta1, double beta2,
                             double eps, double weight_decay, int32_t* ready, double* out_prev, hipStream_t stream) {
  return dc_sequence_step_chained_rec(d, w, e, poses, exp_avg, exp_avg_sq, step, has_prev, grad_scale, lr, beta1, beta2, eps, weight_decay, ready,
                                      out_prev, nullptr, stream);
}

// ---- a chain over the SEVERAL sequences of one loss (train.py:172-175; eval.py:85-112 pools their sums) ---------------------------
// Launch (step, i) evaluates sequence i and first finishes the launch before it -- sequence i - 1 of this step, or the last sequence
// of the previous step -- by summing ITS rows (d_prev, parity prev_parity) onto the running sums of the step (acc_in, NULL for the
// step's second launch).  finish: 0 nothing is pending (the very first launch), 1 sum into out_prev (the running sums; may be
// acc_in itself), 2 the sums complete a step: Adam update `step - 1` on w, out_prev <- the step's totals, w_used_prev.
static int linked_call(const dcSequenceDesc* d_prev, int prev_parity, int finish, const double* acc_in, int n_terms, ChainCall* c) {
  if (finish == 0) return DC_OK;
  if (!d_prev || !d_prev->partials || d_prev->n_terms != n_terms || d_prev->n < 1) return DC_ERR_ARG;
  if (d_prev->partials_count < dc_sequence_partials_count(d_prev->n, n_terms, d_prev->n_scans)) return DC_ERR_WORKSPACE;
  c->prev_rows = chain_buffer(d_prev, n_terms, prev_parity & 1);
  c->prev_count = route_seq_rows(d_prev).g_blocks;
  c->acc_in = acc_in;
  c->prev_status = d_prev->status;
  return DC_OK;
}

int dc_sequence_step_linked(const dcSequenceDesc* d, const dcSequenceDesc* d_prev, int prev_parity, int finish, const double* acc_in,
                            double* w, const double* e, const double* poses, double* exp_avg, double* exp_avg_sq, int64_t step,
                            int64_t stamp, double grad_scale, double lr, double beta1, double beta2, double eps, double weight_decay,
                            int32_t* ready, double* out_prev, double* w_used_prev, hipStream_t stream) {
  if (stamp < 1 || finish < 0 || finish > 2) return DC_ERR_ARG;
  ChainCall c;
  const int rc = chain_call(d, w, exp_avg, exp_avg_sq, step, finish != 0, finish == 2, grad_scale, lr, beta1, beta2, eps, weight_decay, ready, out_prev,
                            &c, d_prev, prev_parity, finish, acc_in);
  if (rc) return rc;
  c.stamp = (uint32_t)stamp;
  c.w_prev_out = finish == 2 ? w_used_prev : nullptr;
  return sequence_eval_impl(d, w, e, poses, 1, 0, 0, out_prev, stream, AdamArgs{}, &c);
}

// the last launch of a linked chain finished on its own: d_prev's rows (+ acc_in) -> out, Adam update `step` (one small launch)
int dc_sequence_chain_flush_linked(const dcSequenceDesc* d_prev, int prev_parity, const double* acc_in, double* w, double* exp_avg,
                                   double* exp_avg_sq, int64_t step, int64_t stamp, double grad_scale, double lr, double beta1, double beta2,
                                   double eps, double weight_decay, int32_t* ready, double* out, hipStream_t stream) {
  if (!d_prev || d_prev->model_kind == DC_MODEL_NONE || d_prev->n_terms < 1 || d_prev->n_terms > 3 || !ready || !out || step < 1) return DC_ERR_ARG;
  ChainCall c{ready, 0, 1, out, AdamArgs{}, nullptr, false, nullptr};
  c.stamp = (uint32_t)stamp;
  int rc = linked_call(d_prev, prev_parity, 2, acc_in, d_prev->n_terms, &c);
  if (rc) return rc;
  rc = make_adam(w, exp_avg, exp_avg_sq, d_prev->n_terms, step, grad_scale, lr, beta1, beta2, eps, weight_decay, &c.adam_prev);
  if (rc) return rc;
  const StepChain ch = make_chain(c, 2 + 2 * d_prev->n_terms + 12 * d_prev->n_scans, nullptr, 0, d_prev->status, 0, w, 0);
  const int P = d_prev->n_terms;
  if (P == 1) hipLaunchKernelGGL(chain_front_only_kernel<1>, dim3(kChainFront), dim3(kBlock), 0, stream, ch);
  else if (P == 2) hipLaunchKernelGGL(chain_front_only_kernel<2>, dim3(kChainFront), dim3(kBlock), 0, stream, ch);
  else hipLaunchKernelGGL(chain_front_only_kernel<3>, dim3(kChainFront), dim3(kBlock), 0, stream, ch);
  DC_CHECK_LAUNCH();
  return DC_OK;
}

int dc_sequence_chain_flush(const dcSequenceDesc* d, double* w, double* exp_avg, double* exp_avg_sq, int64_t step, double grad_scale,
                            double lr, double beta1, double beta2, double eps, double weight_decay, double* out, hipStream_t stream) {
  if (!d || d->model_kind == DC_MODEL_NONE || d->n_terms < 1 || d->n == 0 || !out || step < 1) return DC_ERR_ARG;
  AdamArgs a;
  int rc = make_adam(w, exp_avg, exp_avg_sq, d->n_terms, step, grad_scale, lr, beta1, beta2, eps, weight_decay, &a);
  if (rc) return rc;
  const int n_terms = d->n_terms, n_acc = 2 * n_terms + 12 * d->n_scans;
  if (!d->partials || d->partials_count < dc_sequence_partials_count(d->n, n_terms, d->n_scans)) return DC_ERR_WORKSPACE;
  const int64_t g_blocks = route_seq_rows(d).g_blocks;
  const double* buf = chain_buffer(d, n_terms, (int)(step & 1));
  hipLaunchKernelGGL(reduce_eval_kernel, dim3(2 + n_terms), dim3(kRedBlock), 0, stream, buf, buf + 2 * g_blocks, g_blocks, g_blocks,
                     n_terms, 2 + n_acc, out, a, (const int32_t*)d->status);
  DC_CHECK_LAUNCH();
  return DC_OK;
}

int dc_sequence_eval_after_update(const dcSequenceDesc* d, double* w, const double* e, const double* poses, double* exp_avg,
                                  double* exp_avg_sq, int64_t step, const double* grad_sum, double grad_scale, double lr, double beta1,
                                  double beta2, double eps, double weight_decay, int32_t* ready, double* out, double* w_used,
                                  hipStream_t stream) {
  ChainCall c;
  const int rc = chain_call(d, w, exp_avg, exp_avg_sq, step, grad_sum != nullptr, grad_sum != nullptr, grad_scale, lr, beta1, beta2, eps, weight_decay,
                            ready, out, &c);
  if (rc) return rc;
  c.grad_sum = grad_sum ? grad_sum : w; c.reduce_now = true; c.w_prev_out = w_used;
  return sequence_eval_impl(d, w, e, poses, 1, 0, 0, out, stream, AdamArgs{}, &c);
}

}  // extern "C"
