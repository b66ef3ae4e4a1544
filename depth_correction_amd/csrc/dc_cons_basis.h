// Basis form of the consistency iteration: the basis rows, the kernels that form points from them on the fly (forward, fixed and
// run-time slot counts) and the backward over a run table.  A part of dc_consistency.hip, which includes it after its block
// tables and gather helpers (BlockTab, RunTab, gather_fixed, gather_slots, run_edges): one translation unit.
#pragma once

namespace dc {

// ================================================================================================
// Basis form of the iteration (fixed poses, fixed exponents): every model of the reference is affine in its weights
// (Polynomial d' = d - sum w_k g^e_k, ScaledPolynomial d' = d (1 - sum w_k g^e_k), Linear, InvCos, ScaledInvCos:
// model.py:113-349), so the world point of ray j is
//     x_j(w) = X0_j + (sum_k w_k c_kj) u_j,     X0_j = R (vp + d0 dir) + t,   u_j = R dir,   c_kj = dd'/dw_k   (zero outside the local mask)
// with X0, u and c constant while the poses do not move.  They are computed once (points_basis_kernel); an iteration then
// needs no pass over the points to refresh x: the forward forms the rows it stages (and its centre) from the basis rows on
// the fly, the backward its own point, and the chain to the weights is dL/dw_k = sum_j (g_j . u_j) c_kj -- no model, no
// pose, no incidence angles in the loop.  X0 lives on the q32 grid, u and c in float32 (the correction sum w c is
// centimetres, so its fp32 rounding is ~1e-9 m, far below the grid).  A coordinate is the grid value
// X0 + rint((sum w_k c_k) u / step): the same integer for every block that forms it, rounded twice (X0 and the increment)
// instead of once.  A row is 24 + 4 P bytes: 32 for the two-term models, one aligned sector per gathered point.
// ================================================================================================
struct PointBasis {
  const void* __restrict__ rows;       // [n, 6 + P] words: X0, u, c_0 .. c_{P-1} (Basis<PT>: int32 / float32 bits for q32, fp64 for double)
  const double* __restrict__ w;        // [P] device weights of this evaluation
  int n_terms;
  double w_scale;                      // weights are staged as w_k * w_scale: 1 / grid step for q32, 1 for fp64 points
};

// ---- the per-block row copy of the one-pass step kernel of float32 clouds (dcSequenceDesc.step_rows, dc_step_rows_build) ------------
// For every entry e of a slot table's blk_ids the basis row blk_ids[e], W = 6 + P words as they stand, stored where the block stages
// it from: block b's nd = blk_ptr[b + 1] - blk_ptr[b] entries fill the words [W blk_ptr[b], W blk_ptr[b + 1]) of the copy -- the `base`
// of the block's header addresses it, nothing else is needed.  Inside that stretch the rows lie PIECE-MAJOR: piece g is the words
// [4 g, 4 g + step_rows_piece_words(W, g)) of a row, all nd entries of piece 0 first, then all of piece 1, ...:
//     word c of entry t  at  W blk_ptr[b] + 4 (c / 4) nd + step_rows_piece_words(W, c / 4) t + c % 4.
// Lane t of a wavefront therefore reads a piece right beside lane t + 1's: one contiguous stream per piece instead of a gather by id.
// The 8-word row (two weights) is two 16-byte pieces, 16-byte aligned.  A row of 7 or 9 words keeps its words and no padding: its
// LAST piece is short (3 words for one weight, 1 word for three), stored at that stride, and its pieces are only 4-byte aligned
// (W blk_ptr[b] words is no multiple of four) -- as the 28- and 36-byte basis rows themselves are.
__host__ __device__ constexpr int step_rows_piece_words(int row_words, int piece) {
  return row_words - 4 * piece < 4 ? row_words - 4 * piece : 4;
}

// s_w[k] = w_k * w_scale for the lanes of the block (call before a barrier); coherent: the weights were written by other
// blocks of this very launch (chained steps), so the load must not be served by this XCD's L2
__device__ __forceinline__ void stage_weights(const PointBasis& pb, double* s_w, bool coherent = false) {
  if ((int)threadIdx.x < pb.n_terms) {
    const double w = coherent ? __hip_atomic_load(pb.w + threadIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : pb.w[threadIdx.x];
    s_w[threadIdx.x] = w * pb.w_scale;
  }
}

// Row layout and arithmetic of the basis per point format.  q32 (float32 clouds): X0 on the fixed-point grid, u and c in
// float32 (the correction sum w c is centimetres, so its fp32 rounding is ~1e-9 m, far below the grid); a coordinate is
// X0 + rint((sum w_k c_k) u / step).  double (float64 clouds, the reference's default float_type): everything fp64,
// x = X0 + (sum w_k c_k) u -- the same point as R (vp + d' dir) + t up to the order of the fp64 operations.
template <typename PT> struct Basis;
template <> struct Basis<q32> {
  using T = float;                                       // dtype of the cloud's arrays
  // P > 0: term count known at compile time (one contiguous row, loads issued together), P = 0: run-time count
  template <int P>
  static __device__ __forceinline__ Pt<q32>::Raw point(const PointBasis& pb, const double* wq, int64_t row) {
    const int np = P > 0 ? P : pb.n_terms;
    const int32_t* r = static_cast<const int32_t*>(pb.rows) + row * (6 + np);
    int32_t q[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) q[c] = r[c];
    // float32 throughout (one formula for every kernel that forms a point from its basis row, so that all of them form the
    // same integer): the correction sum is < 2^20 grid steps, its float32 rounding a few hundredths of a step
    float sc = 0.0f;
    if constexpr (P > 0) {
      float c[P];
#pragma unroll
      for (int k = 0; k < P; ++k) c[k] = __int_as_float(r[6 + k]);
#pragma unroll
      for (int k = 0; k < P; ++k) sc = fmaf((float)wq[k], c[k], sc);
    } else {
      for (int k = 0; k < np; ++k) sc = fmaf((float)wq[k], __int_as_float(r[6 + k]), sc);
    }
    Pt<q32>::Raw o;
#pragma unroll
    for (int a = 0; a < 3; ++a) o.v[a] = q[a] + (int32_t)rintf(sc * __int_as_float(q[3 + a]));
    return o;
  }
  static __device__ __forceinline__ void stage(int4* tile, int, int t, const Pt<q32>::Raw& r) { tile[t] = make_int4(r.v[0], r.v[1], r.v[2], 0); }
  // gw[k] += (g . u_j) c_kj for the point's own row (g in metres^-1 units of the loss)
  template <int NP>
  static __device__ __forceinline__ void chain(const PointBasis& pb, int np, int64_t j, const double* g, double* gw) {
    const int32_t* r = static_cast<const int32_t*>(pb.rows) + j * (6 + np);
    const double gu = g[0] * (double)__int_as_float(r[3]) + g[1] * (double)__int_as_float(r[4]) + g[2] * (double)__int_as_float(r[5]);
#pragma unroll
    for (int k = 0; k < NP; ++k)
      if (k < np) gw[k] = gu * (double)__int_as_float(r[6 + k]);
  }
  static __device__ __forceinline__ void write(void* rows, int64_t i, int nt, const double* x0, const double* u, const QParams& qp) {
    int32_t* r = static_cast<int32_t*>(rows) + i * (6 + nt);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      r[a] = quantize(x0[a], qp.origin[a], qp.inv_scale, qp.flag);
      r[3 + a] = __float_as_int((float)u[a]);
    }
  }
  static __device__ __forceinline__ void write_term(void* rows, int64_t i, int nt, int k, double c) {
    static_cast<int32_t*>(rows)[i * (6 + nt) + 6 + k] = __float_as_int((float)c);
  }
};
template <> struct Basis<double> {
  using T = double;
  template <int P>
  static __device__ __forceinline__ Pt<double>::Raw point(const PointBasis& pb, const double* wq, int64_t row) {
    const int np = P > 0 ? P : pb.n_terms;
    const double* r = static_cast<const double*>(pb.rows) + row * (6 + np);
    double q[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) q[c] = r[c];
    double sc = 0.0;
    if constexpr (P > 0) {
      double c[P];
#pragma unroll
      for (int k = 0; k < P; ++k) c[k] = r[6 + k];
#pragma unroll
      for (int k = 0; k < P; ++k) sc += wq[k] * c[k];
    } else {
      for (int k = 0; k < np; ++k) sc += wq[k] * r[6 + k];
    }
    Pt<double>::Raw o;
#pragma unroll
    for (int a = 0; a < 3; ++a) o.v[a] = q[a] + sc * q[3 + a];
    return o;
  }
  // 32-B rows, piece-major like stage_rows<2>: (x, y) at tile[t], (z, -) at tile[cap + t]
  static __device__ __forceinline__ void stage(int4* tile, int cap, int t, const Pt<double>::Raw& r) {
    tile[t] = make_int4(__double2loint(r.v[0]), __double2hiint(r.v[0]), __double2loint(r.v[1]), __double2hiint(r.v[1]));
    tile[cap + t] = make_int4(__double2loint(r.v[2]), __double2hiint(r.v[2]), 0, 0);
  }
  template <int NP>
  static __device__ __forceinline__ void chain(const PointBasis& pb, int np, int64_t j, const double* g, double* gw) {
    const double* r = static_cast<const double*>(pb.rows) + j * (6 + np);
    const double gu = g[0] * r[3] + g[1] * r[4] + g[2] * r[5];
#pragma unroll
    for (int k = 0; k < NP; ++k)
      if (k < np) gw[k] = gu * r[6 + k];
  }
  static __device__ __forceinline__ void write(void* rows, int64_t i, int nt, const double* x0, const double* u, const QParams&) {
    double* r = static_cast<double*>(rows) + i * (6 + nt);
#pragma unroll
    for (int a = 0; a < 3; ++a) { r[a] = x0[a]; r[3 + a] = u[a]; }
  }
  static __device__ __forceinline__ void write_term(void* rows, int64_t i, int nt, int k, double c) {
    static_cast<double*>(rows)[i * (6 + nt) + 6 + k] = c;
  }
};

// the lane's centre from the staged rows (row `t` of the block's distinct list)
template <typename PT>
__device__ __forceinline__ typename Pt<PT>::Raw staged_point(const int4* tile, int cap, int t) {
  int4 piece[Pt<PT>::kRow16];
  read_row<Pt<PT>::kRow16>(tile, cap, (uint32_t)t * 16u, piece);
  return Pt<PT>::from_row(piece);
}

// X0, u and c of every point (once per pose set): the same inputs and arithmetic as points_fwd_kernel.
template <typename PT>
__global__ __launch_bounds__(kBlock) void points_basis_kernel(PointInputs in, int64_t n, QParams qp, void* __restrict__ rows) {
  using T = typename Basis<PT>::T;
  __shared__ double s_pose[kLdsScans * 12];
  const PoseTile poses = stage_poses(in, s_pose);
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  ModelParams mp;
  load_model(in, mp);
  double vp[3], dr[3], T12[12];
  if (in.vps) Row3<T, 3>::load((const T*)in.vps, i, vp, qp);
  else { vp[0] = vp[1] = vp[2] = 0.0; }
  Row3<T, 3>::load((const T*)in.dirs, i, dr, qp);
  const double d = (double)((const T*)in.depth)[i];
  const bool lm = in.lmask ? in.lmask[i] != 0 : true;
  const double inc = (mp.kind != DC_MODEL_NONE && lm) ? (double)((const T*)in.inc)[i] : 0.0;
  load_pose(in, poses, in.scan_id ? in.scan_id[i] : 0, T12);
  double vr[3], drr[3], x0[3];
  rot3(T12, vp, vr);
  vr[0] += T12[3]; vr[1] += T12[7]; vr[2] += T12[11];
  rot3(T12, dr, drr);
  const bool on = mp.kind != DC_MODEL_NONE && lm;
  const double d0 = (on && mp.kind == DC_MODEL_LINEAR) ? 0.0 : d;      // d' at w = 0
#pragma unroll
  for (int a = 0; a < 3; ++a) x0[a] = vr[a] + d0 * drr[a];
  Basis<PT>::write(rows, i, mp.n_terms, x0, drr, qp);
#pragma unroll
  for (int k = 0; k < DC_MAX_MODEL_TERMS; ++k) {
    if (k < mp.n_terms) {
      double dk = 0.0;                                                  // dd'/dw_k
      if (on) {
        if (mp.kind > DC_MODEL_SCALED_POLYNOMIAL) dk = model_dw_other(mp, k, d, inc);
        else dk = (mp.kind == DC_MODEL_SCALED_POLYNOMIAL ? -d : -1.0) * pow_term(inc, mp.e[k]);
      }
      Basis<PT>::write_term(rows, i, mp.n_terms, k, dk);
    }
  }
}

// The per-block row copy (layout: step_rows_piece_words): one workgroup per 256-point block walks the W nd words of its stretch in
// the order they are stored -- contiguous stores -- and gathers each from the basis row its entry names.  Every listed entry is
// written, those of blocks the step kernel skips included; blk_ptr and blk_ids bound everything that is read or written.
__global__ __launch_bounds__(kBlock) void step_rows_kernel(const int32_t* __restrict__ blk_ptr, const int32_t* __restrict__ blk_ids,
                                                           const int32_t* __restrict__ basis, int W, int32_t* __restrict__ out) {
  const int32_t base = blk_ptr[blockIdx.x], nd = blk_ptr[blockIdx.x + 1] - base;
  const int32_t* ids = blk_ids + base;
  int32_t* stretch = out + (int64_t)base * W;
  const int full = (W / 4) * 4 * nd;                                    // words of the whole pieces; the short last piece follows
  for (int j = threadIdx.x; j < W * nd; j += kBlock) {
    const int g = j < full ? j / (4 * nd) : W / 4;
    const int gw = step_rows_piece_words(W, g);
    const int r = j - 4 * g * nd, t = r / gw, c = r - t * gw;
    stretch[j] = basis[(int64_t)ids[t] * W + 4 * g + c];
  }
}

// ---- the packed tile positions of the one-pass step kernel of float32 clouds (dcSequenceDesc.step_loc, dc_step_loc_build) ----------
// A lane of consistency_step_q32_kernel holds its NS 16-bit positions two to a register (pk[]: slot 2 j in the low half of word j).
// They depend on the table alone, so they are stored in that form: block b's 256 NW words (NW = NS / 2) fill the byte range its NS
// rows of `loc` occupy -- from byte 512 slot_ptr[b], word 128 slot_ptr[b], onward: the header's s0 addresses them -- PIECE-MAJOR like
// the row copy: a piece is four consecutive words of a lane (the last piece of NW = 5 the one that remains), all 256 lanes of piece 0
// first, then all of piece 1:   word j of lane t  at  128 slot_ptr[b] + 1024 (j / 4) + step_loc_piece_words(NW, j / 4) t + j % 4.
// A lane fetches a piece with one load of 16 (8, 4) bytes right beside its neighbour's, 16-byte aligned where it is 16 bytes long.
__host__ __device__ constexpr int step_loc_piece_words(int nw, int piece) { return nw - 4 * piece < 4 ? nw - 4 * piece : 4; }

// One workgroup per 256-point block walks the 256 NW words of its range in the order they are stored.  slot_ptr bounds everything:
// the words written are [128 s0, 128 s0 + 256 NW), inside the block's own rows of `loc`, which are what is read.
__global__ __launch_bounds__(kBlock) void step_loc_kernel(const int32_t* __restrict__ slot_ptr, const uint16_t* __restrict__ loc,
                                                          uint32_t* __restrict__ out) {
  const int32_t s0 = slot_ptr[blockIdx.x];
  const int nw = (slot_ptr[blockIdx.x + 1] - s0) / 2;
  const uint16_t* lrow = loc + (int64_t)s0 * kBlock;
  uint32_t* range = out + (int64_t)s0 * (kBlock / 2);
  const int full = (nw / 4) * 4 * kBlock;                               // words of the whole pieces; the short last piece follows
  for (int j = threadIdx.x; j < nw * kBlock; j += kBlock) {
    const int g = j < full ? j / (4 * kBlock) : nw / 4;
    const int gw = step_loc_piece_words(nw, g);
    const int r = j - 4 * g * kBlock, t = r / gw, w = 4 * g + (r - t * gw);
    range[j] = (uint32_t)lrow[2 * w * kBlock + t] | ((uint32_t)lrow[(2 * w + 1) * kBlock + t] << 16);
  }
}

template <typename PT, bool FULL_EIG, int NS, int P>
__global__ __launch_bounds__(kBlock) void consistency_fwd_basis_kernel(
    PointBasis pb, BlockTab tab, const int32_t* __restrict__ own_base, int cap, const int32_t* __restrict__ centre_idx, int64_t n,
    const uint8_t* __restrict__ mask, const typename Basis<PT>::T* __restrict__ offset, LossParams lp, QParams qp, PT* __restrict__ rec,
    typename Basis<PT>::T* __restrict__ pointwise, typename Basis<PT>::T* __restrict__ eigvals, double* __restrict__ partials) {
  using T = typename Basis<PT>::T;
  extern __shared__ int4 tile[];
  __shared__ double s_w[DC_MAX_MODEL_TERMS];
  const int64_t nblocks = (n + kBlock - 1) / kBlock;
  const int64_t blk = xcd_block(nblocks);
  double acc2[2] = {0.0, 0.0};
  const int32_t s0 = blk >= 0 ? tab.slot_ptr[blk] : 0;
  // a table with another slot count than the launch was specialised for (not a table of [rows, NS]): fail loudly
  const bool bad = blk >= 0 && tab.slot_ptr[blk + 1] - s0 != NS;
  if (blk >= 0 && !bad) {
    const int64_t i = blk * kBlock + threadIdx.x;
    const bool live = i < n;
    const uint16_t* lrow = tab.loc + (int64_t)s0 * kBlock + threadIdx.x;
    uint32_t pre[NS];
#pragma unroll
    for (int q = 0; q < NS; ++q) pre[q] = (uint32_t)lrow[q * kBlock];
    stage_weights(pb, s_w);
    const int32_t base = tab.blk_ptr[blk], nd = tab.blk_ptr[blk + 1] - base;
    // the block's own rows sit contiguously in its list (k-NN: every point is its own neighbour): the centre comes from LDS
    const int32_t own = (own_base && !centre_idx) ? own_base[blk] : -1;
    __syncthreads();
    double wq[P > 0 ? P : DC_MAX_MODEL_TERMS];
#pragma unroll
    for (int k = 0; k < (P > 0 ? P : DC_MAX_MODEL_TERMS); ++k) wq[k] = (P > 0 || k < pb.n_terms) ? s_w[k] : 0.0;
    for (int t = threadIdx.x; t < nd; t += kBlock)
      Basis<PT>::stage(tile, cap, t, Basis<PT>::template point<P>(pb, wq, tab.blk_ids[base + t]));
    typename Pt<PT>::Raw ci;
    if (own < 0) ci = Basis<PT>::template point<P>(pb, wq, live ? (centre_idx ? (int64_t)centre_idx[i] : i) : 0);
    __syncthreads();
    if (own >= 0) ci = staged_point<PT>(tile, cap, own + (live ? (int)threadIdx.x : 0));
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
    __syncthreads();
  }
  if (bad) acc2[0] = acc2[1] = __longlong_as_double(0x7ff8000000000000ll);
  wave_partials<2>(acc2, partials);
}

// The same for any slot count (radius neighbourhoods: the reference's default nn_r = 0.25, K = the largest count; or the
// run-time-slot ablation): the slot loop of consistency_fwd_staged_kernel over rows formed from the basis.
template <typename PT, bool FULL_EIG, int P>
__global__ __launch_bounds__(kBlock) void consistency_fwd_basis_slots_kernel(
    PointBasis pb, BlockTab tab, const int32_t* __restrict__ own_base, int cap, const int32_t* __restrict__ centre_idx, int64_t n,
    const uint8_t* __restrict__ mask, const typename Basis<PT>::T* __restrict__ offset, LossParams lp, QParams qp, PT* __restrict__ rec,
    typename Basis<PT>::T* __restrict__ pointwise, typename Basis<PT>::T* __restrict__ eigvals, double* __restrict__ partials) {
  using T = typename Basis<PT>::T;
  extern __shared__ int4 tile[];
  __shared__ double s_w[DC_MAX_MODEL_TERMS];
  const int64_t nblocks = (n + kBlock - 1) / kBlock;
  const int64_t blk = xcd_block(nblocks);
  double acc2[2] = {0.0, 0.0};
  const int64_t i = blk * kBlock + threadIdx.x;
  const bool live = blk >= 0 && i < n;
  int32_t nslots = 0, own = -1;
  const uint16_t* lrow = tab.loc;
  uint32_t pre[kPreSlots];
  stage_weights(pb, s_w);
  if (blk >= 0) {
    const int32_t s0 = tab.slot_ptr[blk];
    nslots = tab.slot_ptr[blk + 1] - s0;
    lrow = tab.loc + (int64_t)s0 * kBlock + threadIdx.x;
#pragma unroll
    for (int q = 0; q < kPreSlots; ++q) pre[q] = (live && q < nslots) ? (uint32_t)lrow[q * kBlock] : kNoLoc;
    own = (own_base && !centre_idx) ? own_base[blk] : -1;
  }
  __syncthreads();
  double wq[P > 0 ? P : DC_MAX_MODEL_TERMS];
#pragma unroll
  for (int k = 0; k < (P > 0 ? P : DC_MAX_MODEL_TERMS); ++k) wq[k] = (P > 0 || k < pb.n_terms) ? s_w[k] : 0.0;
  typename Pt<PT>::Raw ci;
  if (blk >= 0) {
    const int32_t base = tab.blk_ptr[blk], nd = tab.blk_ptr[blk + 1] - base;
    for (int t = threadIdx.x; t < nd; t += kBlock)
      Basis<PT>::stage(tile, cap, t, Basis<PT>::template point<P>(pb, wq, tab.blk_ids[base + t]));
    if (own < 0) ci = Basis<PT>::template point<P>(pb, wq, live ? (centre_idx ? (int64_t)centre_idx[i] : i) : 0);
  }
  __syncthreads();
  if (live) {
    if (own >= 0) ci = staged_point<PT>(tile, cap, own + (int)threadIdx.x);
    CovAcc acc;
    cov_init(acc);
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

// Backward in basis form over a run table: the point itself and the chain to the weights come from the basis rows.
// partial rows: [0, P) dL/dw (the exponent slots [P, 2P) are written as zeros).
template <typename PT, int P>
__global__ __launch_bounds__(kBlock) void consistency_bwd_basis_kernel(
    PointBasis pb, const PT* __restrict__ rec, RunTab tab, int cap, int64_t n, QParams qp, double* __restrict__ partials) {
  constexpr int RR = RecRaw<PT>::kRow16;
  constexpr int NP = P > 0 ? P : DC_MAX_MODEL_TERMS;
  extern __shared__ int4 tile[];
  __shared__ double s_w[DC_MAX_MODEL_TERMS];
  const int64_t nblocks = (n + kBlock - 1) / kBlock;
  const int64_t blk = xcd_block(nblocks);
  double gw[NP];
#pragma unroll
  for (int k = 0; k < NP; ++k) gw[k] = 0.0;
  const int64_t j = blk * kBlock + threadIdx.x;
  const bool active = blk >= 0 && j < n;
  uint2 pre[kPreRuns];
  int32_t nruns = 0;
  uint32_t nd = 0;
  const uint2* runs = reinterpret_cast<const uint2*>(tab.loc);
  if (blk >= 0) {
    if (active) {
      const int32_t r0 = tab.run_ptr[j];
      nruns = tab.run_ptr[j + 1] - r0;
      runs += r0;
    }
#pragma unroll
    for (int t = 0; t < kPreRuns; ++t) pre[t] = t < nruns ? runs[t] : make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu);
    stage_weights(pb, s_w);
    nd = (uint32_t)stage_rows<RR>(tab.blk_ptr, tab.blk_ids, blk, reinterpret_cast<const int4*>(rec), tile, cap);
    if (threadIdx.x < RR) tile[threadIdx.x * cap + nd] = make_int4(0, 0, 0, 0);
  }
  const uint32_t nd16 = nd * 16u;
  __syncthreads();
  if (active) {
    double wq[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) wq[k] = (P > 0 || k < pb.n_terms) ? s_w[k] : 0.0;
    const typename Pt<PT>::Raw cj = Basis<PT>::template point<P>(pb, wq, j);
    double g[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int t = 0; t < kPreRuns; ++t)
      if (__any((int)(t < nruns))) run_edges<PT>(tile, cap, pre[t], nd16, cj, g);
    if (__any((int)(nruns > kPreRuns))) {
      uint2 nxt = kPreRuns < nruns ? runs[kPreRuns] : make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu);
      for (int t = kPreRuns; __any((int)(t < nruns)); ++t) {
        const uint2 r = nxt;
        nxt = t + 1 < nruns ? runs[t + 1] : make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu);
        run_edges<PT>(tile, cap, r, nd16, cj, g);
      }
    }
    const double u = Pt<PT>::unit(qp);
    g[0] *= u; g[1] *= u; g[2] *= u;
    // u_j and c_j again (the row is still in the cache): holding them across the edge loop costs a wavefront of occupancy
    Basis<PT>::template chain<NP>(pb, P > 0 ? P : pb.n_terms, j, g, gw);
  }
  // per-wavefront partial rows, as reduce_param_grads writes them
  const int64_t rs = (int64_t)gridDim.x * kWavesPerBlock;
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  double* prow = partials + (int64_t)blockIdx.x * kWavesPerBlock + wave;
#pragma unroll
  for (int k = 0; k < NP; ++k) {
    if (k < pb.n_terms) {
      const double sw = wave_sum(gw[k]);
      if (lane == 0) { prow[k * rs] = sw; prow[(pb.n_terms + k) * rs] = 0.0; }
    }
  }
}

}  // namespace dc
