// Pose mode in one pass: the pose table, the local basis rows and the one-pass pose kernel.  A part of dc_consistency.hip, included
// after dc_cons_step.h (it shares the step kernels' sweeps and partial sums).
#pragma once

namespace dc {

// ================================================================================================
// Pose mode in ONE pass (round 4): loss, dL/dw AND dL/d[R|t] of every scan from one launch
// ================================================================================================
// train() with pose corrections (train.py:300-312, eval.py:68-82; scripts/model_poses_learning:71) moves the poses every
// iteration, so the basis rows of the model-only step (X0 = R x + t) are stale after every step and the general path ran three
// full passes: dc_points_fwd (22 us) -> forward writing a record per centre (46) -> backward over the transposed table with
// per-scan sums (86; 113 in round 3).  Here one kernel does it:
//   * LOCAL basis rows (dc_points_local_basis, once per exponent set): {d0, dir, c_k, scan} in the SENSOR frame -- 32 B, nothing
//     in them depends on a pose.  Staging forms a row's world point with the CURRENT pose and weights: d' = d0 + sum w_k c_k,
//     x = R_s (d' dir) + t_s on the q32 grid, u = R_s dir; the sweeps then run as in consistency_step_q32_kernel.
//     The rows are stored PER BLOCK in the order of its list (24 B each, 1.75 x the points at C2; the scan of a row is a byte of
//     dcPoseTable.row_scan): staging reads them as one contiguous, coalesced stream -- as gathers through the id list they cost
//     two dependent memory latencies and ~2.3 cycles of the CU's address pipeline per row.
//   * reverse mode INSIDE the block for the poses: in the second sweep every centre ADDS its edges' gradients
//     g_ij = c1_i (v0_i . e) v0_i - c2_i e, e = x_j - mean_i, to the staged rows' sums in LDS (chain_term_pose: 64-bit integer
//     atomics under a per-block power-of-two scale, so the order they land in does not matter).  Rows shared by several blocks
//     get a partial sum in each; the sums over blocks are the reduction's.
//   * the block's distinct rows are listed BY SCAN (dcPoseTable.ids: (scan, id) order, row_seg = where each scan starts), so
//     dL/d[R|t]_s = (sum_j g_j (x_j - t_s)^T) R_s | sum_j g_j runs over a contiguous row range of the tile: eight lanes per scan,
//     fixed order, one row of the row-major pose partials per block.  Bitwise reproducible like everything else.
// 154 us of kernels in three launches -> one launch; see DESIGN 4 for the measured time.
struct PoseTab {
  const int32_t* __restrict__ blk_ptr;     // [blocks + 1], the forward table's
  const int32_t* __restrict__ ids;         // distinct rows of every block in (scan, id) order
  const uint16_t* __restrict__ loc;        // [blocks * K][256]: 16 x position in that order, 0xFFFF = empty slot
  const uint16_t* __restrict__ own_pos;    // [N]: 16 x position of the point's own row in its block's list
  const uint16_t* __restrict__ row_seg;    // [blocks][S + 1]: first row of every scan in the block's list; [S] = the row count
  const uint8_t* __restrict__ row_scan;    // the scan of every listed row (parallel to ids)
};
constexpr int kPoseCap = 512;              // rows of the static tile (the table builder refuses blocks with longer lists)

// Per block: (scan, id) order of its distinct rows, remapped positions, own positions.  info[0] <- 1 when a
// block cannot take the pose kernel (more than kPoseCap rows, or a block whose list misses one of its own rows).
template <int K>
__global__ __launch_bounds__(kBlock) void pose_table_kernel(BlockTab tab, const int32_t* __restrict__ own_base,
                                                            const int32_t* __restrict__ scan_id, int64_t n, int n_scans,
                                                            int32_t* __restrict__ ids_out, uint16_t* __restrict__ loc_out,
                                                            uint16_t* __restrict__ own_pos, uint16_t* __restrict__ row_seg,
                                                            uint8_t* __restrict__ row_scan, int32_t* __restrict__ info) {
  __shared__ int32_t s_id[kPoseCap];
  __shared__ uint8_t s_scan[kPoseCap];
  __shared__ uint16_t s_new[kPoseCap];
  __shared__ int s_start[kMaxBlockScans + 1];
  const int64_t b = blockIdx.x;
  const int tid = threadIdx.x;
  const int32_t base = tab.blk_ptr[b], nd = tab.blk_ptr[b + 1] - base;
  const int32_t own = own_base[b];
  if (nd > kPoseCap || own < 0 || tab.slot_ptr[b + 1] - tab.slot_ptr[b] != K) {        // block-uniform
    if (tid == 0) atomicMax(info, 1);
    return;
  }
  if (tid <= n_scans) s_start[tid] = 0;
  __syncthreads();
  for (int t = tid; t < nd; t += kBlock) {
    const int32_t id = tab.blk_ids[base + t];
    const int sc = scan_id ? scan_id[id] : 0;
    s_id[t] = id;
    s_scan[t] = (uint8_t)sc;
    atomicAdd(&s_start[sc + 1], 1);                      // histogram, shifted by one for the prefix
  }
  __syncthreads();
  if (tid == 0) for (int q = 0; q < n_scans; ++q) s_start[q + 1] += s_start[q];
  __syncthreads();
  for (int t = tid; t < nd; t += kBlock) {
    const int sc = s_scan[t];
    int rank = 0;
    for (int t2 = 0; t2 < t; ++t2) rank += s_scan[t2] == sc ? 1 : 0;      // stable: ascending id inside a scan
    const int p = s_start[sc] + rank;
    s_new[t] = (uint16_t)p;
    ids_out[base + p] = s_id[t];
    row_scan[base + p] = (uint8_t)sc;
  }
  if (tid <= n_scans) row_seg[b * (n_scans + 1) + tid] = (uint16_t)s_start[tid];
  __syncthreads();
  const int64_t i = b * kBlock + tid;
  if (i < n) own_pos[i] = (uint16_t)(s_new[own + tid] << 4);
  const uint16_t* lrow = tab.loc + (int64_t)tab.slot_ptr[b] * kBlock + tid;
#pragma unroll
  for (int q = 0; q < K; ++q) {
    const uint16_t l = lrow[q * kBlock];
    loc_out[((int64_t)b * K + q) * kBlock + tid] = l == 0xFFFF ? (uint16_t)0xFFFF : (uint16_t)(s_new[l >> 4] << 4);
  }
}

// {d0, dir, c_0, c_1}: the pose-independent part of a ray (sensor frame; viewpoints at the sensor origin), 6 words.  One workgroup
// per block of the pose table writes the rows of the block's list, in its order, at rows [blk_ptr[b], blk_ptr[b + 1]).
template <typename T>
__global__ __launch_bounds__(kBlock) void points_local_basis_kernel(PointInputs in, PoseTab tab, int32_t* __restrict__ rows) {
  const int64_t b = blockIdx.x;
  const int32_t base = tab.blk_ptr[b], nd = tab.blk_ptr[b + 1] - base;
  ModelParams mp;
  load_model(in, mp);
  for (int t = threadIdx.x; t < nd; t += kBlock) {
    const int64_t i = tab.ids[base + t];
    const T* dp = (const T*)in.dirs + i * 3;
    const double d = (double)((const T*)in.depth)[i];
    const bool lm = in.lmask ? in.lmask[i] != 0 : true;
    const bool on = mp.kind != DC_MODEL_NONE && lm;
    const double inc = on ? (double)((const T*)in.inc)[i] : 0.0;
    const double d0 = (on && mp.kind == DC_MODEL_LINEAR) ? 0.0 : d;
    float c[2] = {0.0f, 0.0f};
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      if (k < mp.n_terms && on) {
        const double dk = mp.kind > DC_MODEL_SCALED_POLYNOMIAL ? model_dw_other(mp, k, d, inc)
                                                               : (mp.kind == DC_MODEL_SCALED_POLYNOMIAL ? -d : -1.0) * pow_term(inc, mp.e[k]);
        c[k] = (float)dk;
      }
    }
    int2* r = reinterpret_cast<int2*>(rows) + 3 * (int64_t)(base + t);
    r[0] = make_int2(__float_as_int((float)d0), __float_as_int((float)dp[0]));
    r[1] = make_int2(__float_as_int((float)dp[1]), __float_as_int((float)dp[2]));
    r[2] = make_int2(__float_as_int(c[0]), __float_as_int(c[1]));
  }
}

// second sweep of the pose kernel, one neighbour: chain_term_q32 plus the edge's gradient g_ij = al v0 - c2 e_j ADDED to the
// neighbour's row of the block's gradient planes.  The sums are 64-bit integers, so the order the wavefronts' LDS atomics land in
// does not matter (bit-reproducible); the coefficients arrive scaled by the block's power of two S with |g_ij| S < 2^50, and
// double(g) + 1.5 2^52 holds round(g) in its mantissa: the bit pattern minus that of 1.5 2^52 (low word zero) IS the integer.
template <int P, int CAP>
__device__ __forceinline__ void chain_term_pose(const int4* tile, unsigned long long* s_g, uint32_t off, bool have, const Pt<q32>::Raw& ci,
                                                const float* cmf, const float* vs, const float* vu, float c2f, float* gw) {
  const char* row = reinterpret_cast<const char*>(tile) + (have ? off : 0u);
  const int4 p0 = *reinterpret_cast<const int4*>(row);
  const int4 p1 = *reinterpret_cast<const int4*>(row + (size_t)CAP * 16);
  const float2v e01 = float2v{(float)(p0.x - ci.v[0]), (float)(p0.y - ci.v[1])} - float2v{cmf[0], cmf[1]};
  const float e0 = e01.x, e1 = e01.y, e2 = (float)(p0.z - ci.v[2]) - cmf[2];
  const float u0 = __int_as_float(p0.w), u1 = __int_as_float(p1.x), u2 = __int_as_float(p1.y);
  const float al = fmaf(vs[2], e2, fmaf(vs[1], e1, vs[0] * e0));                       // c1 (v . e_j)
  const float g0 = fmaf(al, vu[0], -(c2f * e0)), g1 = fmaf(al, vu[1], -(c2f * e1)), g2 = fmaf(al, vu[2], -(c2f * e2));
  float tj = fmaf(g2, u2, fmaf(g1, u1, g0 * u0));                                      // g_ij . u_j
  if (!have) tj = 0.0f;
  if constexpr (P == 2) {
    float2v g = float2v{gw[0], gw[1]};
    g = __builtin_elementwise_fma(float2v{tj, tj}, float2v{__int_as_float(p1.z), __int_as_float(p1.w)}, g);
    gw[0] = g.x; gw[1] = g.y;
  } else {
    gw[0] = fmaf(tj, __int_as_float(p1.z), gw[0]);
  }
  if (have) {
    constexpr double kMagic = 6755399441055744.0;                                      // 1.5 2^52
    unsigned long long* cell = reinterpret_cast<unsigned long long*>(reinterpret_cast<char*>(s_g) + (off >> 1));
    const float gg[3] = {g0, g1, g2};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const unsigned long long bits = (unsigned long long)__double_as_longlong((double)gg[a] + kMagic) - 0x4338000000000000ull;
      atomicAdd(cell + a * CAP, bits);
    }
  }
}

// Pose-mode evaluation in ONE launch (float32 sequences, [rows, K] tables, no exponent gradients).  A block stages its distinct
// rows from the pose-independent local basis rows {d0, dir, c0, c1, scan} with the CURRENT poses and weights, runs the step kernel's
// two sweeps, and in the second sweep every centre adds its edges' gradients to the block's per-row gradient planes in LDS
// (chain_term_pose); the rows of one scan are contiguous in the block's list (dc_pose_table_build), so dL/d[R|t]_s of the block
// is a sum over a row range: one row [12 S] of the row-major pose partials per block, summed by reduce_eval_kernel.
template <int NS, int P>
__global__ __launch_bounds__(kBlock, 4) void consistency_step_pose_kernel(
    const int32_t* __restrict__ lrows, PoseTab tab, const double* __restrict__ poses, int n_scans, const double* __restrict__ w,
    int64_t n, const uint8_t* __restrict__ mask, LossParams lp, QParams qp, double* __restrict__ p_fwd, double* __restrict__ p_bwd) {
  constexpr int CAP = kPoseCap;
  __shared__ int4 tile[2 * CAP];                            // piece 0 {X, u0} | piece 1 {u1, u2, c0, c1}
  __shared__ unsigned long long s_g[3 * CAP];               // three planes: the rows' gradient sums (64-bit integers)
  __shared__ double s_pose[kLdsScans * 12];
  __shared__ float s_bound[kWavesPerBlock];
  const int tid = threadIdx.x;
  const int64_t nblocks = (n + kBlock - 1) / kBlock;
  const int64_t blk = xcd_block(nblocks);
  // one partial row per block in every column: {sum loss, count} at p_fwd, dL/dw, zeros for dL/de, the 12 S pose sums at p_bwd.  The
  // eight rows of a 64-byte line are blocks of ONE XCD (blockIdx & 7), so the line is completed in that XCD's L2, and the
  // reduction reads every column as one contiguous run.
  const int64_t rs = (int64_t)gridDim.x;
  double* pcol = p_bwd + 2 * P * rs + (int64_t)(blockIdx.x & 7) * (gridDim.x >> 3) + (blockIdx.x >> 3);
  double acc2[2] = {0.0, 0.0}, gw[P];
#pragma unroll
  for (int k = 0; k < P; ++k) gw[k] = 0.0;
  if (blk < 0) {                                            // padding block of the last round (block-uniform): zero rows
    for (int item = tid; item < 12 * n_scans; item += kBlock) pcol[item * rs] = 0.0;
  } else {
    for (int t = tid; t < n_scans * 12; t += kBlock) s_pose[t] = poses[t];
    double wq[P];
#pragma unroll
    for (int k = 0; k < P; ++k) wq[k] = w[k];
    const int64_t i = blk * kBlock + tid;
    const bool live = i < n;
    const bool in_mask = live && (mask ? mask[i] != 0 : true);
    const uint16_t* lrow = tab.loc + (blk * NS) * kBlock + tid;
    uint32_t pre[NS];
#pragma unroll
    for (int q = 0; q < NS; ++q) pre[q] = live ? (uint32_t)lrow[q * kBlock] : kNoLoc;
    const uint32_t own = live ? (uint32_t)tab.own_pos[i] : 0u;
    const int32_t base = tab.blk_ptr[blk], nd = tab.blk_ptr[blk + 1] - base;
    // the (at most two) rows this thread stages, in flight before anything else: the block's rows are one contiguous stream
    static_assert(CAP == 2 * kBlock, "two staged rows per thread");
    int2 rw[2][3];
    int rsc[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int t = tid + j * kBlock < nd ? tid + j * kBlock : 0;
      const int2* src = reinterpret_cast<const int2*>(lrows) + 3 * (int64_t)(base + t);
      rw[j][0] = src[0]; rw[j][1] = src[1]; rw[j][2] = src[2];
      rsc[j] = tab.row_scan[base + t];
    }
    for (int t = tid; t < 3 * CAP; t += kBlock) s_g[t] = 0ull;
    __syncthreads();                                        // the poses are in LDS
    // ---- staging: the world point of every distinct row from its local basis row, the current pose and weights ----
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int t = tid + j * kBlock;
      if (t >= nd) continue;
      const float c0 = __int_as_float(rw[j][2].x), c1f = __int_as_float(rw[j][2].y);
      const int sc = rsc[j];
      double dp = (double)__int_as_float(rw[j][0].x) + wq[0] * (double)c0;
      if constexpr (P > 1) dp += wq[1] * (double)c1f;
      const double dl[3] = {(double)__int_as_float(rw[j][0].y), (double)__int_as_float(rw[j][1].x), (double)__int_as_float(rw[j][1].y)};
      const double* Tp = s_pose + sc * 12;
      double u[3], x[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        u[a] = Tp[4 * a] * dl[0] + Tp[4 * a + 1] * dl[1] + Tp[4 * a + 2] * dl[2];
        x[a] = Tp[4 * a + 3] + dp * u[a];
      }
      tile[t] = make_int4(quantize(x[0], qp.origin[0], qp.inv_scale, qp.flag), quantize(x[1], qp.origin[1], qp.inv_scale, qp.flag),
                          quantize(x[2], qp.origin[2], qp.inv_scale, qp.flag), __float_as_int((float)u[0]));
      tile[CAP + t] = make_int4(__float_as_int((float)u[1]), __float_as_int((float)u[2]), rw[j][2].x, rw[j][2].y);
    }
    __syncthreads();
    // ---- the centre: moments, smallest eigenpair, loss (as consistency_step_q32_kernel) and a bound of its edges' gradients ----
    const bool work = live && (!mask || __any((int)in_mask));
    Pt<q32>::Raw ci;
    double cm[3] = {0.0, 0.0, 0.0}, v0[3] = {0.0, 0.0, 0.0}, c1 = 0.0, c2 = 0.0;
    float bound = 0.0f;
    if (work) {
      const char* tb = reinterpret_cast<const char*>(tile);
      ci = Pt<q32>::from_row(reinterpret_cast<const int4*>(tb + own));
      CovAcc acc;
      cov_init(acc);
      uint32_t mo = pre[0];
#pragma unroll
      for (int q = 1; q < NS; ++q) mo |= pre[q];
      const bool any_miss = __any((int)(mo & 1u)) != 0;
      int n_have;
      if (any_miss) n_have = gather_fixed<q32, NS, true, true>(tile, CAP, ci, pre, acc);      // (16-byte reads: keep_row_word)
      else n_have = gather_fixed<q32, NS, false, true>(tile, CAP, ci, pre, acc);
      acc.W = (double)n_have;
      double se2;
      step_point2<q32, NS>(acc, n_have, !any_miss, in_mask, lp, qp, acc2, cm, v0, &c1, &c2, &se2);
      // |g_ij| <= (|c1| + |c2|) |e_j| and |e_j|^2 <= sum_j |e_j|^2 (at least one grid unit, so that c S stays finite)
      const float r = sqrtf((float)se2);
      bound = (float)(fabs(c1) + fabs(c2)) * (r > 1.0f ? r : 1.0f);
    }
    bound = bound == bound ? bound : INFINITY;              // a NaN coefficient poisons the block's sums like an infinite one
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) bound = fmaxf(bound, __shfl_xor(bound, o, kWave));
    if ((tid & (kWave - 1)) == 0) s_bound[tid / kWave] = bound;
    __syncthreads();
    bound = s_bound[0];
#pragma unroll
    for (int q = 1; q < kWavesPerBlock; ++q) bound = fmaxf(bound, s_bound[q]);
    const bool poisoned = !(bound < INFINITY);              // block-uniform
    int sh = 0;
    if (bound > 0.0f && !poisoned) {
      int ex;
      (void)frexpf(bound, &ex);                             // bound < 2^ex
      sh = 50 - ex;
      sh = sh > 100 ? 100 : sh;
    }
    const double S = ldexp(1.0, sh), invS = ldexp(1.0, -sh);
    // ---- second sweep: dL/dw of the centre, and its edges' gradients into the rows' planes ----
    if (work && !poisoned) {
      float cmf[3], vs[3], vu[3], gwf[P];
      const double c1s = c1 * S;
#pragma unroll
      for (int a = 0; a < 3; ++a) { cmf[a] = (float)cm[a]; vs[a] = (float)(c1s * v0[a]); vu[a] = (float)v0[a]; }
      const float c2f = (float)(c2 * S);
#pragma unroll
      for (int k = 0; k < P; ++k) gwf[k] = 0.0f;
      if (__any((int)(c1 != 0.0 || c2 != 0.0))) {
#pragma unroll
        for (int q = 0; q < NS; ++q) {
          if (q % 4 == 0 && q > 0) __builtin_amdgcn_sched_barrier(0);
          chain_term_pose<P, CAP>(tile, s_g, pre[q], pre[q] != kNoLoc && (c1 != 0.0 || c2 != 0.0), ci, cmf, vs, vu, c2f, gwf);
        }
      }
#pragma unroll
      for (int k = 0; k < P; ++k) gw[k] = (double)gwf[k] * (qp.scale * invS);
    }
    __syncthreads();                                        // every edge has been added
    // ---- dL/d[R|t]_s = sum_j g_j (x) [x_local_j, 1] over the rows of scan s, contiguous in the block's list.  With
    //      x_local = R^T (x - t) the sum is (sum_j g_j (x_j - t)^T) R: eight lanes per scan (n_scans <= 32) take every eighth row
    //      each and sum g (x) q and g over them -- q the row's grid coordinates, g its three integer sums, all in LDS -- the eight
    //      lanes' twelve sums are added by DPP quad / row operations that also halve what a lane carries (as wave_sum4_dpp), and
    //      lanes 0..2 of the eight finish row a of [dL/dR | dL/dt] with the scan's pose ----
    {
      const uint16_t* seg = tab.row_seg + blk * (n_scans + 1);
      const int sc = tid >> 3, part = tid & 7;
      const bool mine = sc < n_scans;
      const int end = mine ? (int)seg[sc + 1] : 0;
      // slot (p & 1) 6 + (p >> 1) 3 + c ends on lane p of the eight: lanes 0..2 get {sum g_a q_c}, a = p; lane 3 {sum g_a}
      double sacc[12];
#pragma unroll
      for (int q = 0; q < 12; ++q) sacc[q] = 0.0;
      for (int p = mine ? (int)seg[sc] + part : 0; p < end; p += 8) {
        const int4 xr = tile[p];
        const double qd[3] = {(double)xr.x, (double)xr.y, (double)xr.z};
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          const unsigned long long bits = s_g[a * CAP + p];
          const double g = fma((double)(int)(uint32_t)(bits >> 32), 4294967296.0, (double)(uint32_t)bits);
#pragma unroll
          for (int c = 0; c < 3; ++c) sacc[(a & 1) * 6 + (a >> 1) * 3 + c] = fma(g, qd[c], sacc[(a & 1) * 6 + (a >> 1) * 3 + c]);
          sacc[9 + a] += g;                                 // lane 3: (3 & 1) 6 + (3 >> 1) 3 = 9
        }
      }
      const bool up1 = (part & 1) != 0, up2 = (part & 2) != 0;
      double h[6], r3[3], gs[3];
#pragma unroll
      for (int q = 0; q < 6; ++q) h[q] = (up1 ? sacc[6 + q] : sacc[q]) + dpp_f64<kDppXor1>(up1 ? sacc[q] : sacc[6 + q]);
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        r3[q] = (up2 ? h[3 + q] : h[q]) + dpp_f64<kDppXor2>(up2 ? h[q] : h[3 + q]);
        r3[q] += dpp_f64<kDppShl4>(r3[q]);                  // lanes 0..3 of the eight: + lanes 4..7
        gs[q] = dpp_f64<kDppQuad3>(r3[q]);                  // {sum g_a} from lane 3 of the quad
      }
      if (mine && part < 3) {
        const double unscale = qp.scale * invS;             // the block's gradient unit
        const double* Tp = s_pose + sc * 12;
        const double ga = (part == 0 ? gs[0] : (part == 1 ? gs[1] : gs[2])) * unscale;
        double m[3];                                        // row a of sum_j g_j (x_j - t)^T
#pragma unroll
        for (int c = 0; c < 3; ++c) m[c] = fma(r3[c] * unscale, qp.scale, ga * (qp.origin[c] - Tp[4 * c + 3]));
        double* dst = pcol + (sc * 12 + part * 4) * rs;
#pragma unroll
        for (int b2 = 0; b2 < 3; ++b2) {
          const double v = fma(m[2], Tp[8 + b2], fma(m[1], Tp[4 + b2], m[0] * Tp[b2]));
          dst[b2 * rs] = poisoned ? (double)NAN : v;
        }
        dst[3 * rs] = poisoned ? (double)NAN : ga;
      }
    }
  }
  // {sum loss, count, dL/dw} of the wavefront; the exponent-gradient columns [P, 2P) of this evaluation are zero
  if (tid < P) p_bwd[(P + tid) * rs + blockIdx.x] = 0.0;
  step_partials<P, true>(acc2, gw, p_fwd, p_bwd, true, 0);
}

}  // namespace dc
