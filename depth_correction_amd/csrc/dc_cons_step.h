// Loss AND dL/dw in one pass: the staged rows, the per-centre tail, the second sweep, the partial sums and the four one-pass step
// kernels.  A part of dc_consistency.hip, included after dc_cons_basis.h and dc_cons_chain.h.
#pragma once

namespace dc {

// ---- loss AND dL/dw in one pass (forward-mode accumulation) -------------------------------------------------------------
// With only the P model weights to differentiate, the reverse pass over the transposed table is not needed:
//     dL/dw_k = sum_i sum_{j in N(i)} (dl_i/dx_j) . (dx_j/dw_k),   dl_i/dx_j = c1_i (v0_i . d) v0_i - c2_i d,  d = x_j - cmean_i,
//     dx_j/dw_k = c_kj u_j
// is a second sweep of centre i over its OWN neighbours, whose rows (x_j and now also u_j, c_kj) already sit in LDS.  No
// backward record is written or read (64 + 64 MB per iteration at C2), no transposed table, no second launch; the terms
// are the ones the backward kernel adds up, grouped by centre instead of by point, with c1 / c2 / cmean in fp64.
// Staged row (piece-major, 16-B pieces; piece 0 starts with the point in its usual row format, so the first sweep and the
// centre read it as before):  q32: {x0, x1, x2, u0 | u1, u2, c0, c1 | c2}, x on the grid, u / c float32 bits;
// double: {x0, x1 | x2, u0' u1' | u2', c0', c1', c2'} (u', c': float32 copies for the second sweep).
template <typename PT, int P> struct StepRow;
template <int P> struct StepRow<q32, P> {
  static constexpr int kPieces = (6 + P + 3) / 4;
  struct Raw { int32_t q[6 + P]; };                       // a basis row as fetched (before the weights are known)
  static __device__ __forceinline__ Raw fetch(const PointBasis& pb, int64_t row) {
    const int32_t* r = static_cast<const int32_t*>(pb.rows) + row * (6 + P);
    Raw o;
#pragma unroll
    for (int c = 0; c < 6 + P; ++c) o.q[c] = r[c];
    return o;
  }
  static __device__ __forceinline__ void stage(const PointBasis& pb, const double* wq, int64_t row, int4* tile, int cap, int t) {
    place(fetch(pb, row), wq, tile, cap, t);
  }
  // Entry t of a block's list of `nd` rows, from one of two sources (the same for the whole launch): `crow`, the block's stretch of the
  // per-block row copy (dcSequenceDesc.step_rows, layout: step_rows_piece_words) -- one trip, lane t beside lane t + 1 -- or, when it
  // is null, the basis row ids[t]: the id first, then a gather.  The same words either way.
  static __device__ __forceinline__ Raw fetch_copy(const int32_t* crow, int nd, int t) {
    constexpr int W = 6 + P;
    Raw o;
#pragma unroll
    for (int g = 0; g < kPieces; ++g) {
      const int gw = step_rows_piece_words(W, g);
      const int32_t* r = crow + (uint32_t)(4 * g * nd + gw * t);
#pragma unroll
      for (int c = 0; c < gw; ++c) o.q[4 * g + c] = r[c];
    }
    return o;
  }
  static __device__ __forceinline__ void place(const Raw& raw, const double* wq, int4* tile, int cap, int t) {
    const int32_t* q = raw.q;
    float sc = 0.0f;                                      // exactly Basis<q32>::point's arithmetic
#pragma unroll
    for (int k = 0; k < P; ++k) sc = fmaf((float)wq[k], __int_as_float(q[6 + k]), sc);
    int32_t x[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) x[a] = q[a] + (int32_t)rintf(sc * __int_as_float(q[3 + a]));
    tile[t] = make_int4(x[0], x[1], x[2], q[3]);
    tile[cap + t] = make_int4(q[4], q[5], q[6], P > 1 ? q[P > 1 ? 7 : 6] : 0);
    if constexpr (P > 2) tile[2 * cap + t] = make_int4(q[8], 0, 0, 0);
  }
  // the neighbourhood mean in the staged rows' units: x_i + cm (grid steps; exact in fp64)
  static __device__ __forceinline__ void mean_of(const Pt<q32>::Raw& ci, const double* cm, double* mean) {
#pragma unroll
    for (int a = 0; a < 3; ++a) mean[a] = (double)ci.v[a] + cm[a];
  }
  // e = x_j - mean (grid steps), u_j, c_kj of the staged row at byte offset `off`
  static __device__ __forceinline__ void load(const int4* tile, int cap, uint32_t off, const double* mean, double* e, double* u, double* c) {
    const char* row = reinterpret_cast<const char*>(tile) + off;
    const int4 p0 = *reinterpret_cast<const int4*>(row);
    const int4 p1 = *reinterpret_cast<const int4*>(row + (size_t)cap * 16);
    e[0] = (double)p0.x - mean[0]; e[1] = (double)p0.y - mean[1]; e[2] = (double)p0.z - mean[2];
    u[0] = (double)__int_as_float(p0.w); u[1] = (double)__int_as_float(p1.x); u[2] = (double)__int_as_float(p1.y);
    c[0] = (double)__int_as_float(p1.z);
    if constexpr (P > 1) c[1] = (double)__int_as_float(p1.w);
    if constexpr (P > 2) c[2] = (double)__int_as_float(reinterpret_cast<const int4*>(row + (size_t)cap * 32)->x);
  }
};
template <int P> struct StepRow<double, P> {
  // Staged row of a float64 cloud (round 5): {x0, x1 | x2, u0' u1' | u2', c0', c1', c2'} -- the point in fp64 as before (the first
  // sweep and the centre read pieces 0 and 1: the loss is what it was, bit for bit), u and c as float32 COPIES for the second sweep:
  // 48 B instead of 64, three LDS reads per neighbour there instead of four.  The kernel is bound by LDS reads at random rows
  // (SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE = 0.62, LDS busy two thirds of the launch).  The point itself is formed from the
  // fp64 basis row; the float32 copies enter dL/dw only: a relative rounding of 6e-8 per term, of random sign over 2e7 terms.
  static constexpr int kPieces = 3;
  static_assert(P <= 3, "three float32 weights' terms fit the third piece");
  static __device__ __forceinline__ int4 pack(double a, double b) {
    return make_int4(__double2loint(a), __double2hiint(a), __double2loint(b), __double2hiint(b));
  }
  struct Raw { double q[6 + P]; };
  static __device__ __forceinline__ Raw fetch(const PointBasis& pb, int64_t row) {
    const double* r = static_cast<const double*>(pb.rows) + row * (6 + P);
    Raw o;
#pragma unroll
    for (int c = 0; c < 6 + P; ++c) o.q[c] = r[c];
    return o;
  }
  static __device__ __forceinline__ void stage(const PointBasis& pb, const double* wq, int64_t row, int4* tile, int cap, int t) {
    place(fetch(pb, row), wq, tile, cap, t);
  }
  static __device__ __forceinline__ void place(const Raw& raw, const double* wq, int4* tile, int cap, int t) {
    double q[9];
#pragma unroll
    for (int c = 0; c < 9; ++c) q[c] = c < 6 + P ? raw.q[c] : 0.0;
    double sc = 0.0;
#pragma unroll
    for (int k = 0; k < P; ++k) sc += wq[k] * q[6 + k];
#pragma unroll
    for (int a = 0; a < 3; ++a) q[a] += sc * q[3 + a];
    tile[t] = pack(q[0], q[1]);
    tile[cap + t] = make_int4(__double2loint(q[2]), __double2hiint(q[2]), __float_as_int((float)q[3]), __float_as_int((float)q[4]));
    tile[2 * cap + t] = make_int4(__float_as_int((float)q[5]), __float_as_int((float)q[6]), __float_as_int((float)q[7]), __float_as_int((float)q[8]));
  }
  static __device__ __forceinline__ void mean_of(const Pt<double>::Raw& ci, const double* cm, double* mean) {
#pragma unroll
    for (int a = 0; a < 3; ++a) mean[a] = ci.v[a] + cm[a];
  }
  static __device__ __forceinline__ void load(const int4* tile, int cap, uint32_t off, const double* mean, double* e, double* u, double* c) {
    const char* row = reinterpret_cast<const char*>(tile) + off;
    const int4 p0 = *reinterpret_cast<const int4*>(row);
    const int4 p1 = *reinterpret_cast<const int4*>(row + (size_t)cap * 16);
    const int4 p2 = *reinterpret_cast<const int4*>(row + (size_t)cap * 32);
    e[0] = __hiloint2double(p0.y, p0.x) - mean[0]; e[1] = __hiloint2double(p0.w, p0.z) - mean[1]; e[2] = __hiloint2double(p1.y, p1.x) - mean[2];
    u[0] = (double)__int_as_float(p1.z); u[1] = (double)__int_as_float(p1.w); u[2] = (double)__int_as_float(p2.x);
    c[0] = (double)__int_as_float(p2.y);
    if constexpr (P > 1) c[1] = (double)__int_as_float(p2.z);
    if constexpr (P > 2) c[2] = (double)__int_as_float(p2.w);
  }
};

// one neighbour's share of dL/dw: gw[k] += t c_kj, t = c1 (v . e)(v . u_j) - c2 (e . u_j); have = false: nothing
template <typename PT, int P>
__device__ __forceinline__ void chain_term(const int4* tile, int cap, uint32_t off, bool have, const double* mean, const double* v,
                                           double c1, double c2, double* gw) {
  double e[3], u[3], c[P];
  StepRow<PT, P>::load(tile, cap, have ? off : 0u, mean, e, u, c);
  const double al = v[0] * e[0] + v[1] * e[1] + v[2] * e[2];
  const double be = v[0] * u[0] + v[1] * u[1] + v[2] * u[2];
  const double ga = e[0] * u[0] + e[1] * u[1] + e[2] * u[2];
  double tj = c1 * al * be - c2 * ga;
  if (!have) tj = 0.0;
#pragma unroll
  for (int k = 0; k < P; ++k) gw[k] = fma(tj, c[k], gw[k]);
}

// everything of a centre after its moments are gathered: covariance -> smallest eigenpair -> loss (acc2) and the
// coefficients of its neighbours' terms; an empty neighbourhood (NaN mean, zero coefficients) contributes exactly nothing
template <typename PT>
__device__ __forceinline__ void step_point(CovAcc& acc, bool m, const LossParams& lp, const QParams& qp, double* acc2, double* cm,
                                           double* v0, double* c1, double* c2) {
  cov_same_weights(acc);
  const double u = Pt<PT>::unit(qp);
  double moff[3], C[6], D, omega, lam0, tr;
  cov_finish(acc, 0.0, moff, cm, C, &D, &omega, u * u);
  eig3_smallest_r2(C[0], C[1], C[2], C[3], C[4], C[5], &lam0, v0, &tr);      // (the A-B baseline form, dc_set_option(6, 0))
  const double l = loss_and_coeffs(lp, lam0, tr, D, 0.0, m, c1, c2);
  const bool drop = loss_dropped(lp, l);
  if (drop) *c1 = *c2 = 0.0;
  if (m && !drop) { acc2[0] = l; acc2[1] = 1.0; }
  if (!(*c1 != 0.0 || *c2 != 0.0)) { cm[0] = cm[1] = cm[2] = 0.0; v0[0] = v0[1] = v0[2] = 0.0; }
}

// ---- the slimmer forms of the one-pass kernel's per-centre work (VAR bits of consistency_step_basis_kernel) ----------------
constexpr int kVarF32Sweep = 1;     // second sweep in float32 (q32 points: differences, u and c are float32-exact already)
constexpr int kVarSlimTail = 2;     // covariance -> eigenpair -> loss without the intermediate normalisations (eig3_smallest_unit)
constexpr int kVarDppSums = 4;      // wavefront sums through DPP row operations instead of ds_bpermute shuffles
constexpr int kStepVar = kVarF32Sweep | kVarSlimTail | kVarDppSums;     // what every instantiation but the A-B baseline (0) uses

// Covariance, smallest eigenpair, loss and the coefficients c1, c2 of a centre from its moments about the centre point.
// The covariance is only ever needed divided by its trace (eig3_smallest_unit), so the Bessel / unit factor f = unit^2 / D
// multiplies the trace alone; `full` (wave-uniform): every lane of the wavefront has all `ns` neighbours, W and D are constants (ns: the
// slot count, NS unless the kernel learns it at run time; 1 / ns and 1 / (ns - 1) are correctly rounded divisions either way, so a
// run-time count gives the bits of the compile-time one).
template <typename PT, int NS>
__device__ __forceinline__ void step_point2(const CovAcc& acc, int n_have, bool full, bool m, const LossParams& lp, const QParams& qp,
                                            double* acc2, double* cm, double* v0, double* c1, double* c2, double* sum_e2 = nullptr,
                                            int ns = NS) {
  const double u = Pt<PT>::unit(qp);
  double invW, D, invD;
  if (full) {
    invW = 1.0 / ns; D = ns - 1.0; invD = 1.0 / (ns - 1.0);
  } else {
    const double W = (double)n_have;
    invW = recip1_(W);                                  // W = 0: inf * 0 -> NaN mean, like the reference's 0 / 0
    D = W - 1.0;
    D = D < 1e-6 ? 1e-6 : D;
    invD = recip1_(D);
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) cm[a] = acc.s[a] * invW;
  double Cp[6];
  Cp[0] = fma(-acc.s[0], cm[0], acc.S[0]); Cp[1] = fma(-acc.s[0], cm[1], acc.S[1]); Cp[2] = fma(-acc.s[0], cm[2], acc.S[2]);
  Cp[3] = fma(-acc.s[1], cm[1], acc.S[3]); Cp[4] = fma(-acc.s[1], cm[2], acc.S[4]); Cp[5] = fma(-acc.s[2], cm[2], acc.S[5]);
  const double mp = (Cp[0] + Cp[3]) + Cp[5];            // trace in the units of the differences
  if (sum_e2) *sum_e2 = mp;                             // = sum_j |x_j - mean|^2
  const double f = (u * u) * invD;
  const double tr = mp * f;
  double lam_rel, inv_tr;
  if (!(mp > 0.0) || !(mp < (double)INFINITY)) {
    const bool zero = (mp == 0.0) && Cp[1] == 0.0 && Cp[2] == 0.0 && Cp[4] == 0.0;
    lam_rel = zero ? 0.0 : (double)NAN;
    inv_tr = 1e6;                                       // tr is 0 (or NaN): the clamp of loss.py:253 applies
    v0[0] = 1.0; v0[1] = 0.0; v0[2] = 0.0;
  } else {
    const double inv_m = recip1_(mp);
    eig3_smallest_unit<!std::is_same<PT, q32>::value>(Cp[0] * inv_m, Cp[1] * inv_m, Cp[2] * inv_m, Cp[3] * inv_m, Cp[4] * inv_m, Cp[5] * inv_m,
                                                       &lam_rel, v0);
    const double inv_u2 = std::is_same<PT, q32>::value ? qp.inv_scale * qp.inv_scale : 1.0;
    inv_tr = inv_m * (D * inv_u2);                      // 1 / tr = 1 / (mp f)
  }
  const double lam0 = lam_rel * tr;
  // loss_and_coeffs with the reciprocals at hand
  double raw, g_vv = 0.0, g_eye = 0.0;
  if (lp.kind == DC_LOSS_MIN_EIGVAL) {
    if (lp.normalization) {
      const double inv = tr < 1e-6 ? 1e6 : inv_tr;      // 1 / clamp(tr, 1e-6); NaN compares false
      raw = lam0 * inv;
      g_vv = inv;
      g_eye = (tr > 1e-6) ? -raw * inv : 0.0;
    } else {
      raw = lam0;
      g_vv = 1.0;
    }
  } else {
    raw = tr;
    g_eye = 1.0;
  }
  double l = raw;
  double a = (m && l > 0.0) ? 1.0 : 0.0;
  l = l > 0.0 ? l : (l != l ? l : 0.0);
  if (lp.sqrt_) {
    const double sq = sqrt(l);
    a = (l > 0.0) ? a * 0.5 / sq : 0.0;
    l = sq;
  }
  const bool drop = loss_dropped(lp, l);                    // (skip_nans / only_finite: not part of the reduction at all)
  const double fd = drop ? 0.0 : 2.0 * a * invD;
  *c1 = fd * g_vv;
  *c2 = -fd * g_eye;
  if (m && !drop) { acc2[0] = l; acc2[1] = 1.0; }
  // an empty neighbourhood (NaN mean) must contribute nothing to the second sweep: only possible when slots are missing
  if (!full && !(*c1 != 0.0 || *c2 != 0.0)) { cm[0] = cm[1] = cm[2] = 0.0; v0[0] = v0[1] = v0[2] = 0.0; }
}

// One neighbour's share of dL/dw in float32 (q32 rows): the difference to the centre is an exact int32, u and c are float32
// words already, and the per-centre factors are rounded once; the lane's sums stay float32 over its K neighbours and join the
// fp64 reduction afterwards.  vs = c1 v0, vu = v0, both float32.
template <int P>
__device__ __forceinline__ void chain_term_f32(const int4* tile, int cap, uint32_t off, bool have, const Pt<q32>::Raw& ci, const float* cmf,
                                               const float* vs, const float* vu, float c2f, float* gw) {
  const char* row = reinterpret_cast<const char*>(tile) + (have ? off : 0u);
  const int4 p0 = *reinterpret_cast<const int4*>(row);
  const int4 p1 = *reinterpret_cast<const int4*>(row + (size_t)cap * 16);
  const float e0 = (float)(p0.x - ci.v[0]) - cmf[0], e1 = (float)(p0.y - ci.v[1]) - cmf[1], e2 = (float)(p0.z - ci.v[2]) - cmf[2];
  const float u0 = __int_as_float(p0.w), u1 = __int_as_float(p1.x), u2 = __int_as_float(p1.y);
  const float al = fmaf(vs[2], e2, fmaf(vs[1], e1, vs[0] * e0));
  const float be = fmaf(vu[2], u2, fmaf(vu[1], u1, vu[0] * u0));
  const float ga = fmaf(e2, u2, fmaf(e1, u1, e0 * u0));
  float tj = fmaf(al, be, -(c2f * ga));
  if (!have) tj = 0.0f;
  gw[0] = fmaf(tj, __int_as_float(p1.z), gw[0]);
  if constexpr (P > 1) gw[1] = fmaf(tj, __int_as_float(p1.w), gw[1]);
  if constexpr (P > 2) gw[2] = fmaf(tj, __int_as_float(reinterpret_cast<const int4*>(row + (size_t)cap * 32)->x), gw[2]);
}

// the second sweep over the slots beyond the first 16, in the same trips of eight; a trip's float32 sums join the fp64 sums trip by
// trip (a row of two hundred neighbours is too long for one float32 running sum)
template <int P>
__device__ __forceinline__ void chain_tail_f32(const int4* tile, int cap, const uint16_t* lrow, int nslots, bool packed, const Pt<q32>::Raw& ci,
                                               const float* cmf, const float* vs, const float* vu, float c2f, double* gw) {
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
    float g[P];
#pragma unroll
    for (int k = 0; k < P; ++k) g[k] = 0.0f;
#pragma unroll
    for (int u_ = 0; u_ < kTrip; ++u_) chain_term_f32<P>(tile, cap, l[u_], l[u_] != kNoLoc, ci, cmf, vs, vu, c2f, g);
#pragma unroll
    for (int k = 0; k < P; ++k) gw[k] += (double)g[k];
  }
}
template <typename PT, int P>
__device__ __forceinline__ void chain_tail(const int4* tile, int cap, const uint16_t* lrow, int nslots, bool packed, const double* mean,
                                           const double* v0, double c1, double c2, double* gw) {
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
#pragma unroll
    for (int u_ = 0; u_ < kTrip; ++u_) chain_term<PT, P>(tile, cap, l[u_], l[u_] != kNoLoc, mean, v0, c1, c2, gw);
  }
}

// (Round 5, measured and dropped for float64 rows: loss AND dL/dw from ONE sweep.  t_j is bilinear in (1, cm) x d_j, so with
//  A_k = sum c_kj u_j, B_k = sum c_kj (d_j . u_j), M_k = sum c_kj u_j d_j^T the second sweep collapses to
//  c1 (v^T M_k v - (v . cm)(v . A_k)) - c2 (B_k - cm . A_k): every staged row read once, 64 B per neighbour instead of 96.  But the 26
//  fp64 accumulators beside the moments cost the occupancy the LDS saving was meant to buy: 246 registers = two wavefronts per SIMD and
//  101 us; held to 168 registers (three per SIMD) 117 us, against 69 us for the two sweeps at 126 registers.)
// ---- wavefront sums through DPP -------------------------------------------------------------------------------------------
// One 32-bit half of a double moved by a DPP row operation (quad permutes, rotations inside a row of 16 lanes)
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v) {
  // (every lane has a source under these controls; bound_ctrl only spares the `old` operand its initialisation)
  const int lo = __builtin_amdgcn_mov_dpp(__double2loint(v), CTRL, 0xF, 0xF, true);
  const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(v), CTRL, 0xF, 0xF, true);
  return __hiloint2double(hi, lo);
}
constexpr int kDppXor1 = 0xB1;      // quad_perm:[1,0,3,2]
constexpr int kDppXor2 = 0x4E;      // quad_perm:[2,3,0,1]
constexpr int kDppRor4 = 0x124;     // row_ror:4
constexpr int kDppRor8 = 0x128;     // row_ror:8
constexpr int kDppShl4 = 0x104;     // row_shl:4 (lane l reads lane l + 4 of its row)
constexpr int kDppQuad3 = 0xFF;     // quad_perm:[3,3,3,3]
// Lane l < W of every 2 W lanes: the value of lane l + W (W = 16: the next row, W = 32: the other half), through gfx950's row / half
// swaps -- VALU moves, where a shuffle is an LDS round trip.  (The other lanes get nothing they can use.)
template <int W>
__device__ __forceinline__ double upper_lanes_f64(double v) {
  const unsigned lo = (unsigned)__double2loint(v), hi = (unsigned)__double2hiint(v);
  // {vdst, vsrc} after the swap of vdst's odd rows (upper half) with vsrc's even rows (lower half): vsrc's lower lanes hold vdst's upper
  if constexpr (W == 16)
    return __hiloint2double((int)__builtin_amdgcn_permlane16_swap(hi, hi, false, false)[1], (int)__builtin_amdgcn_permlane16_swap(lo, lo, false, false)[1]);
  else
    return __hiloint2double((int)__builtin_amdgcn_permlane32_swap(hi, hi, false, false)[1], (int)__builtin_amdgcn_permlane32_swap(lo, lo, false, false)[1]);
}
// Four values per lane -> lane l < 4 of the wavefront holds the total of value bitrev2(l) (as wave_sum_packed<4>): two quad
// steps that also halve what a lane carries, two rotations inside the rows, two cross-row exchanges.  SWAP: the cross-row exchanges as
// swaps, which serve lanes < 16 only (the same additions in the same order there: step_block_row, whose wavefront 0 alone stands
// between the block and its end).
template <bool SWAP = false>
__device__ __forceinline__ double wave_sum4_dpp(double* v) {
  const int lane = threadIdx.x & (kWave - 1);
  const bool up1 = (lane & 1) != 0, up2 = (lane & 2) != 0;
  // bit 0: this lane keeps values {0, 1} (bit clear) or {2, 3} (bit set), the partner the others
  const double k0 = up1 ? v[2] : v[0], g0 = up1 ? v[0] : v[2];
  const double k1 = up1 ? v[3] : v[1], g1 = up1 ? v[1] : v[3];
  const double a0 = k0 + dpp_f64<kDppXor1>(g0);
  const double a1 = k1 + dpp_f64<kDppXor1>(g1);
  // bit 1: keeps the first of its two (bit clear) or the second
  const double kk = up2 ? a1 : a0, gg = up2 ? a0 : a1;
  double r = kk + dpp_f64<kDppXor2>(gg);
  r += dpp_f64<kDppRor4>(r);
  r += dpp_f64<kDppRor8>(r);
  if constexpr (SWAP) {
    r += upper_lanes_f64<16>(r);
    r += upper_lanes_f64<32>(r);
  } else {
    r += __shfl_xor(r, 16, kWave);
    r += __shfl_xor(r, 32, kWave);
  }
  return r;
}

// wave_sum_packed<8> with every level in registers of its own (the in-place form indexes its array by a lane-dependent address: 80 B
// of scratch in the three-weight step kernels): the same selects, exchanges and additions in the same order
__device__ __forceinline__ double wave_sum8_regs(const double* v) {
  const int lane = threadIdx.x & (kWave - 1);
  const bool up1 = (lane & 1) != 0, up2 = (lane & 2) != 0, up4 = (lane & 4) != 0;
  double a[4], b[2];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double keep = up1 ? v[k + 4] : v[k], give = up1 ? v[k] : v[k + 4];
    a[k] = keep + __shfl_xor(give, 1, kWave);
  }
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const double keep = up2 ? a[k + 2] : a[k], give = up2 ? a[k] : a[k + 2];
    b[k] = keep + __shfl_xor(give, 2, kWave);
  }
  const double keep = up4 ? b[1] : b[0], give = up4 ? b[0] : b[1];
  double r = keep + __shfl_xor(give, 4, kWave);
#pragma unroll
  for (int off = 8; off < kWave; off <<= 1) r += __shfl_xor(r, off, kWave);
  return r;
}

// {sum loss, count} -> p_fwd columns, dL/dw -> p_bwd columns (same row stride: one row per wavefront), through one packed
// wavefront reduction of the 2 + P values: the ordinary (unchained) form of the step kernels.  (per_block: the pose kernel's one row
// per block; the chained step kernels have step_block_row below.)
template <int P, bool DPP = false>
__device__ __forceinline__ void step_partials(const double* acc2, const double* gw, double* __restrict__ p_fwd, double* __restrict__ p_bwd,
                                              bool per_block = false, int n_front = 0) {
  constexpr int NV = 2 + P, NP2 = NV <= 4 ? 4 : 8;
  __shared__ double s_comb[kWavesPerBlock][NP2];
  double v[NP2];
  v[0] = acc2[0]; v[1] = acc2[1];
#pragma unroll
  for (int k = 0; k < NP2 - 2; ++k) v[2 + k] = k < P ? gw[k] : 0.0;
  double tot;
  if constexpr (DPP && NP2 == 4) tot = wave_sum4_dpp(v);
  else tot = wave_sum_packed<NP2>(v);
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  int64_t rs = (int64_t)gridDim.x * kWavesPerBlock, row = (int64_t)blockIdx.x * kWavesPerBlock + wave;
  if (per_block) {
    // chained steps: one row per block (a quarter of the rows for the next launch's leading blocks to sum)
    if (lane < NP2) s_comb[wave][lane] = tot;
    __syncthreads();
    if (wave != 0) return;
    if (lane < NP2) tot = (s_comb[0][lane] + s_comb[1][lane]) + (s_comb[2][lane] + s_comb[3][lane]);
    rs = (int64_t)gridDim.x - n_front;
    row = (int64_t)blockIdx.x - n_front;
  }
  if (lane < NP2) {
    const int q = packed_value_of_lane<NP2>(lane);
    if (q < 2) p_fwd[q * rs + row] = tot;
    else if (q < NV) p_bwd[(q - 2) * rs + row] = tot;
  }
}

// ---- a chained launch's row of partials {sum loss, count, dL/dw_0..P-1}: ONE row per block, summed ONCE -----------------------
// Every one-pass step kernel ends its chained form here, so that the same lane values give the same row whichever kernel formed
// them (the tests compare the kernels' chained sums byte for byte).  The order of the additions is fixed:
//  (a) every lane holds its fp64 values: the loss and dL/dw_k, already converted and scaled (1 + P values; an idle lane's are +0.0);
//  (b) wavefronts 1..3 hand their lanes' values to wavefront 0 through LDS -- `hand`, laid out [value][wavefront - 1][lane] -- and
//      lane l of wavefront 0 forms (v0 + v1) + (v2 + v3) per value, v_w being lane l's value in wavefront w;
//  (c) wavefront 0 runs the packed wavefront reduction once over {loss, 0, dL/dw..}: wave_sum4_dpp for 2 + P <= 4 (its cross-row
//      exchanges as swaps: the same additions), wave_sum8_regs for three weights (DPP = false, the A-B baseline: wave_sum_packed, the
//      same selects, exchanges and additions through shuffles);
//  (d) the count is the number of lanes that count, wavefront by wavefront (popcount of the ballot), added as (c0 + c1) + (c2 + c3):
//      small integers, so the same double as the sum of the lanes' 0 / 1 in any order; it takes the place of column 1's total;
//  (e) lanes < NP2 of wavefront 0 store the row: row blockIdx.x - n_front of gridDim.x - n_front, columns {loss, count} at p_fwd and
//      dL/dw at p_bwd.
// `bad` (a slot count the kernel is not built for, a wait for the weights that ran out) poisons loss and count with NaN; `nothing` (a
// padding block, a block none of whose centres is inside the mask) stores +0.0 in every column -- what the sums of its zeros were --
// without a barrier.  Both are the same for the whole block, and every thread of the block makes the call.
// `hand` is the block's tile: it is dead once every wavefront has left its second sweep, which the first barrier below waits for (no LDS
// of its own: the q32 kernel's seven or six tiles per CU stay what they were).  The launch gives the tile at least step_hand_bytes<P>().
// The row's address is the same for the whole block but for the lane's column: the bases stay in scalar registers and a lane adds a
// 32-bit byte offset ((2 + P) * 8 * rows < 2^32: a hundred million blocks).
template <int P> constexpr size_t step_hand_bytes() { return (size_t)((kWavesPerBlock - 1) * kWave * (1 + P) + kWavesPerBlock) * sizeof(double); }
template <int P, bool DPP = true>
__device__ __forceinline__ void step_block_row(double loss, bool cnt_lane, const double* gw, bool bad, bool nothing, double* hand,
                                               double* __restrict__ p_fwd, double* __restrict__ p_bwd, int n_front) {
  constexpr int NV = 2 + P, NP2 = NV <= 4 ? 4 : 8, NL = 1 + P, kOthers = kWavesPerBlock - 1;
  static_assert(kWavesPerBlock == 4, "(v0 + v1) + (v2 + v3)");
  const uint32_t lane = threadIdx.x & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
  const uint32_t rs = gridDim.x - (uint32_t)n_front, row = blockIdx.x - (uint32_t)n_front;
  const int q = packed_value_of_lane<NP2>((int)(lane & (NP2 - 1)));
  char* const fwd = reinterpret_cast<char*>(p_fwd);
  char* const bwd = reinterpret_cast<char*>(p_bwd);
  const uint32_t off_f = ((uint32_t)q * rs + row) * 8u, off_b = ((uint32_t)(q - 2) * rs + row) * 8u;
  if (nothing && !bad) {
    if (wave == 0 && lane < NP2) {
      if (q < 2) *reinterpret_cast<double*>(fwd + off_f) = 0.0;
      else if (q < NV) *reinterpret_cast<double*>(bwd + off_b) = 0.0;
    }
    return;
  }
  const double nan_ = __longlong_as_double(0x7ff8000000000000ll);
  double cnt = bad ? nan_ : (double)(int)__popcll(__ballot((int)cnt_lane));
  double v[NP2];
  v[0] = bad ? nan_ : loss; v[1] = 0.0;
#pragma unroll
  for (int k = 0; k < NP2 - 2; ++k) v[2 + k] = k < P ? gw[k] : 0.0;
  __syncthreads();                                      // every wavefront has read the last of its staged rows
  if (wave != 0) {
    double* h = hand + (wave - 1) * kWave + lane;
    h[0] = v[0];
#pragma unroll
    for (int k = 0; k < P; ++k) h[(1 + k) * kOthers * kWave] = v[2 + k];
    if (lane == 0) hand[NL * kOthers * kWave + wave] = cnt;
  }
  __syncthreads();
  if (wave != 0) return;
  {
    const double* h = hand + lane;
    v[0] = (v[0] + h[0]) + (h[kWave] + h[2 * kWave]);
#pragma unroll
    for (int k = 0; k < P; ++k) {
      const double* hk = h + (1 + k) * kOthers * kWave;
      v[2 + k] = (v[2 + k] + hk[0]) + (hk[kWave] + hk[2 * kWave]);
    }
    const double* hc = hand + NL * kOthers * kWave;
    cnt = (cnt + hc[1]) + (hc[2] + hc[3]);
  }
  double tot;
  if constexpr (NP2 == 4) tot = DPP ? wave_sum4_dpp<true>(v) : wave_sum_packed<4>(v);
  else tot = DPP ? wave_sum8_regs(v) : wave_sum_packed<8>(v);
  if (q == 1) tot = cnt;
  if (lane < NP2) {
    if (q < 2) *reinterpret_cast<double*>(fwd + off_f) = tot;
    else if (q < NV) *reinterpret_cast<double*>(bwd + off_b) = tot;
  }
}

// partial rows: columns {sum loss, count} at p_fwd (stride gridDim * 4) and [0, P) dL/dw at p_bwd (same stride)
template <typename PT, int NS, int P, int VAR = 0>
__global__ __launch_bounds__(kBlock) void consistency_step_basis_kernel(
    PointBasis pb, BlockTab tab, const int32_t* __restrict__ own_base, int cap, const int32_t* __restrict__ centre_idx, int64_t n,
    const uint8_t* __restrict__ mask, LossParams lp, QParams qp, double* __restrict__ p_fwd, double* __restrict__ p_bwd,
    StepChain ch) {
  extern __shared__ int4 tile[];
  __shared__ double s_w[DC_MAX_MODEL_TERMS];
  __shared__ int s_ok;
  __shared__ double s_front[kBlock / kWave];
  const bool chained = ch.ready != nullptr;
  if (chained && (int)blockIdx.x < ch.n_front) { chain_front_block<P>(ch, s_front); return; }
  const int64_t nblocks = (n + kBlock - 1) / kBlock;
  int64_t blk = chain_block_of(ch, chained, nblocks);
  if (blk >= 0 && ch.blk_skip && ch.blk_skip[blk]) blk = -1;            // no centre of this block is inside the loss mask
  double acc2[2] = {0.0, 0.0}, gw[P];
#pragma unroll
  for (int k = 0; k < P; ++k) gw[k] = 0.0;
  const int32_t s0 = blk >= 0 ? tab.slot_ptr[blk] : 0;
  bool bad = blk >= 0 && tab.slot_ptr[blk + 1] - s0 != NS;
  if (blk >= 0 && !bad) {
    const int64_t i = blk * kBlock + threadIdx.x;
    const bool live = i < n;
    const bool in_mask = live && (mask ? mask[i] != 0 : true);
    const uint16_t* lrow = tab.loc + (int64_t)s0 * kBlock + threadIdx.x;
    uint32_t pre[NS];
#pragma unroll
    for (int q = 0; q < NS; ++q) pre[q] = (uint32_t)lrow[q * kBlock];
    const int32_t base = tab.blk_ptr[blk], nd = tab.blk_ptr[blk + 1] - base;
    const int32_t own = (own_base && !centre_idx) ? own_base[blk] : -1;
    double wq[P];
    if (chained) {
      // the weights of this launch come from its leading blocks: fetch the rows this lane stages (the first two: a block
      // lists ~1.5 distinct rows per lane) BEFORE waiting for them, so that the wait hides behind the fetch or vice versa
      // (a wait that never ends poisons the sums instead of hanging)
      typename StepRow<PT, P>::Raw r0, r1;
      const int t0 = threadIdx.x, t1 = threadIdx.x + kBlock;
      if (t0 < nd) r0 = StepRow<PT, P>::fetch(pb, tab.blk_ids[base + t0]);
      if (t1 < nd) r1 = StepRow<PT, P>::fetch(pb, tab.blk_ids[base + t1]);
      chain_weights<P>(ch, pb.w_scale, s_w, &s_ok);
      __syncthreads();
      if (!s_ok) bad = true;
#pragma unroll
      for (int k = 0; k < P; ++k) wq[k] = s_w[k];
      if (t0 < nd) StepRow<PT, P>::place(r0, wq, tile, cap, t0);
      if (t1 < nd) StepRow<PT, P>::place(r1, wq, tile, cap, t1);
      for (int t = threadIdx.x + 2 * kBlock; t < nd; t += kBlock) StepRow<PT, P>::stage(pb, wq, tab.blk_ids[base + t], tile, cap, t);
    } else {
      stage_weights(pb, s_w);
      __syncthreads();
#pragma unroll
      for (int k = 0; k < P; ++k) wq[k] = s_w[k];
      for (int t = threadIdx.x; t < nd; t += kBlock) StepRow<PT, P>::stage(pb, wq, tab.blk_ids[base + t], tile, cap, t);
    }
    typename Pt<PT>::Raw ci;
    if (own < 0) ci = Basis<PT>::template point<P>(pb, wq, live ? (centre_idx ? (int64_t)centre_idx[i] : i) : 0);
    __syncthreads();
    if (own >= 0) ci = staged_point<PT>(tile, cap, own + (live ? (int)threadIdx.x : 0));
    if (live && (!mask || __any((int)in_mask))) {        // (a wavefront of masked-out centres only: nothing to add, see consistency_step_q32_kernel)
      CovAcc acc;
      cov_init(acc);
      uint32_t mx = pre[0];
#pragma unroll
      for (int q = 1; q < NS; ++q) mx = max(mx, pre[q]);
      const bool any_miss = __any((int)(mx == kNoLoc)) != 0;
      int n_have;
      constexpr bool kWide = std::is_same<PT, q32>::value;            // (16-byte reads of the 16-byte rows: keep_row_word)
      if (any_miss) n_have = gather_fixed<PT, NS, true, kWide>(tile, cap, ci, pre, acc);
      else n_have = gather_fixed<PT, NS, false, kWide>(tile, cap, ci, pre, acc);
      acc.W = (double)n_have;
      double cm[3], v0[3], c1, c2;
      if constexpr ((VAR & kVarSlimTail) != 0) step_point2<PT, NS>(acc, n_have, !any_miss, in_mask, lp, qp, acc2, cm, v0, &c1, &c2);
      else step_point<PT>(acc, in_mask, lp, qp, acc2, cm, v0, &c1, &c2);
      const double u = Pt<PT>::unit(qp);
      if constexpr ((VAR & kVarF32Sweep) != 0 && std::is_same<PT, q32>::value) {
        // second sweep in float32 (see chain_term_f32); the lane's sums join the fp64 reduction
        float cmf[3], vs[3], vu[3], gwf[P];
#pragma unroll
        for (int a = 0; a < 3; ++a) { cmf[a] = (float)cm[a]; vs[a] = (float)(c1 * v0[a]); vu[a] = (float)v0[a]; }
        const float c2f = (float)c2;
#pragma unroll
        for (int k = 0; k < P; ++k) gwf[k] = 0.0f;
        // (groups of four with a scheduling fence between them: left alone, the compiler requests all 2 NS row pieces up
        // front -- 80 registers -- and the kernel drops from 6 to 4 wavefronts per SIMD)
        if (any_miss) {
#pragma unroll
          for (int q = 0; q < NS; ++q) {
            if (q % 4 == 0 && q > 0) __builtin_amdgcn_sched_barrier(0);
            chain_term_f32<P>(tile, cap, pre[q], pre[q] != kNoLoc, ci, cmf, vs, vu, c2f, gwf);
          }
        } else {
#pragma unroll
          for (int q = 0; q < NS; ++q) {
            if (q % 4 == 0 && q > 0) __builtin_amdgcn_sched_barrier(0);
            chain_term_f32<P>(tile, cap, pre[q], true, ci, cmf, vs, vu, c2f, gwf);
          }
        }
#pragma unroll
        for (int k = 0; k < P; ++k) gw[k] = (double)gwf[k] * u;
      } else {
        double mean[3];
        StepRow<PT, P>::mean_of(ci, cm, mean);
        // second sweep over the same slots (full wavefronts skip the validity selects)
        if (any_miss) {
#pragma unroll
          for (int q = 0; q < NS; ++q) chain_term<PT, P>(tile, cap, pre[q], pre[q] != kNoLoc, mean, v0, c1, c2, gw);
        } else {
#pragma unroll
          for (int q = 0; q < NS; ++q) chain_term<PT, P>(tile, cap, pre[q], true, mean, v0, c1, c2, gw);
        }
#pragma unroll
        for (int k = 0; k < P; ++k) gw[k] *= u;            // differences were in grid steps
      }
    }
  }
  if (chained) {                                         // one row per block (step_block_row)
    step_block_row<P, (VAR & kVarDppSums) != 0>(acc2[0], acc2[1] != 0.0, gw, bad, blk < 0, reinterpret_cast<double*>(tile), p_fwd, p_bwd, ch.n_front);
    return;
  }
  if (bad) acc2[0] = acc2[1] = __longlong_as_double(0x7ff8000000000000ll);
  step_partials<P, (VAR & kVarDppSums) != 0>(acc2, gw, p_fwd, p_bwd);
}

// ---- the one-pass kernel for q32 points and a fixed slot count: what a C2 step runs ----------------------------------------
// Same table, same basis rows, same staged rows {x0 x1 x2 u0 | u1 u2 c0 c1 | c2} (StepRow<q32, P>) and same sums as
// consistency_step_basis_kernel<q32, NS, P>; what differs is where the instructions go (the kernel issues VALU instructions
// ~98 % of its time -- rocprofv3 SQ_ACTIVE_INST_VALU -- so its duration IS its instruction count, at one wave64 VALU instruction
// per four cycles per SIMD whatever the type: tools/ubench/valu_rates.hip):
//  * the tile is STATIC LDS of kStepQ32Cap rows: its address and the piece stride are immediates of the ds_read instructions and
//    the table's 16-bit byte offset is the address register as it stands (dynamic LDS costs a v_add per row piece: 30 per centre);
//  * the per-centre tail is step_point2 (eig3_smallest_unit: adjugate eigenvector, reciprocals with one Newton step, the
//    deflation path only for needles);
//  * the second sweep is float32 (the difference to the centre is an exact int32, u and c are float32 words, the per-centre
//    factors are rounded once);
//  * the wavefront sums go through DPP row operations;
//  * with `step_rows` (dcSequenceDesc.step_rows: the rows of every block's list stored once, in staging order) a block fetches its
//    rows straight after its header, as contiguous streams, instead of its ids first and then the rows they name -- the same words.
// A fp64-difference row format ({x - ref} as doubles: no int -> fp conversions in the sweeps, 80 instructions fewer) was measured
// and dropped: 48-B rows make the kernel LDS-bound (SQ_LDS_IDX_ACTIVE 87 % of its duration, 56 % of it bank conflicts of the
// random row reads: 61 us against 52).
constexpr int kStepQ32Cap = 512;          // rows of the static LDS tile (16 KB + 8 KB for a third piece: six blocks per CU); a second
                                          // instantiation takes 768 rows (24 KB: still six blocks per CU for one or two weights); tables with
                                          // more distinct rows per block take consistency_step_basis_kernel

// second sweep, one neighbour (float32): gw[k] += c_kj (c1 (v . e_j)(v . u_j) - c2 (e_j . u_j)); vs = c1 v0, vu = v0
typedef float float2v __attribute__((ext_vector_type(2)));
template <int P, int CAP>
__device__ __forceinline__ void chain_term_q32(const int4* tile, uint32_t off, bool have, const Pt<q32>::Raw& ci, const float* cmf, const float* vs,
                                               const float* vu, float c2f, float* gw) {
  const char* row = reinterpret_cast<const char*>(tile) + (have ? off : 0u);
  const int4 p0 = *reinterpret_cast<const int4*>(row);
  const int4 p1 = *reinterpret_cast<const int4*>(row + (size_t)CAP * 16);
  // (two-wide float operations where the operands already sit in neighbouring registers: v_pk_add_f32 / v_pk_fma_f32 issue two
  //  operations in one slot)
  const float2v e01 = float2v{(float)(p0.x - ci.v[0]), (float)(p0.y - ci.v[1])} - float2v{cmf[0], cmf[1]};
  const float e0 = e01.x, e1 = e01.y, e2 = (float)(p0.z - ci.v[2]) - cmf[2];
  const float u0 = __int_as_float(p0.w), u1 = __int_as_float(p1.x), u2 = __int_as_float(p1.y);
  const float al = fmaf(vs[2], e2, fmaf(vs[1], e1, vs[0] * e0));                       // c1 (v . e_j)
  const float be = fmaf(vu[2], u2, fmaf(vu[1], u1, vu[0] * u0));                       // v . u_j
  const float ga = fmaf(e2, u2, fmaf(e1, u1, e0 * u0));                                // e_j . u_j
  float tj = fmaf(al, be, -(c2f * ga));
  if (!have) tj = 0.0f;
  if constexpr (P == 2) {
    float2v g = float2v{gw[0], gw[1]};
    g = __builtin_elementwise_fma(float2v{tj, tj}, float2v{__int_as_float(p1.z), __int_as_float(p1.w)}, g);
    gw[0] = g.x; gw[1] = g.y;
  } else {
    gw[0] = fmaf(tj, __int_as_float(p1.z), gw[0]);
    if constexpr (P > 1) gw[1] = fmaf(tj, __int_as_float(p1.w), gw[1]);
    if constexpr (P > 2) gw[2] = fmaf(tj, __int_as_float(reinterpret_cast<const int4*>(row + (size_t)CAP * 32)->x), gw[2]);
  }
}

// Blocks per CU the kernel is built for.  Seven need <= 72 VGPRs (512 per SIMD lane / 7, in granules of 8), <= 96 SGPRs (256-thread
// blocks are admitted up to 800 / (ceil(sgpr / 16) 16 + 16) per CU: 6 at 97..112) and seven tiles in the 160 KiB of LDS: the 512-row
// tile of one or two weights.  The 768-row tile and the third piece of three weights stay at six, the 768-row tile of three at four.
// (Five against six wavefronts per SIMD: 47.2 against 44.4 us per step.)
template <int P, int CAP> constexpr int step_q32_blocks() {
  constexpr int lds = StepRow<q32, P>::kPieces * CAP * 16 + 512;      // the tile and the block's few small arrays
  return 7 * lds <= 160 * 1024 ? 7 : 6 * lds <= 160 * 1024 ? 6 : 4;
}
// The lane's NS 16-bit tile positions two to a register (slot 2 j in the low half of word j): they live through both sweeps and the tail
template <int Q> __device__ __forceinline__ uint32_t pre_at(const uint32_t* pk) { return (Q & 1) ? pk[Q >> 1] >> 16 : pk[Q >> 1] & 0xFFFFu; }
// pk[] of lane `tid` from the block's stretch of the packed positions (layout: step_loc_piece_words): one load per piece of four words
template <int NW>
__device__ __forceinline__ void fetch_step_loc(const uint32_t* blk, uint32_t tid, uint32_t* pk) {
  static_assert(NW % 4 == 0 || NW % 4 == 1 || NW % 4 == 2, "the slot counts the step kernel is built for: 4, 8, 10, 16");
#pragma unroll
  for (int g = 0; 4 * g < NW; ++g) {
    const int gw = step_loc_piece_words(NW, g);
    const uint32_t* r = blk + (uint32_t)(4 * g * kBlock) + (uint32_t)gw * tid;
    if (gw == 4) {
      const uint4 v = *reinterpret_cast<const uint4*>(r);
      pk[4 * g] = v.x; pk[4 * g + 1] = v.y; pk[4 * g + 2] = v.z; pk[4 * g + 3] = v.w;
    } else if (gw == 2) {
      const uint2 v = *reinterpret_cast<const uint2*>(r);
      pk[4 * g] = v.x; pk[4 * g + 1] = v.y;
    } else {
      pk[4 * g] = r[0];
    }
  }
}
// gather_fixed<q32, NS, MISS> over packed positions: the same reads, differences and additions in the same order
template <int NS, bool MISS, int Q0 = 0>
__device__ __forceinline__ int gather_fixed_pk(const int4* tile, const Pt<q32>::Raw& ci, const uint32_t* pk, CovAcc& acc) {
  if constexpr (Q0 >= NS) return 0;
  else {
    constexpr int NQ = NS - Q0 < 4 ? NS - Q0 : 4;
    uint32_t off[NQ];
    off[0] = pre_at<Q0>(pk);
    if constexpr (NQ > 1) off[1] = pre_at<Q0 + (NQ > 1 ? 1 : 0)>(pk);
    if constexpr (NQ > 2) off[2] = pre_at<Q0 + (NQ > 2 ? 2 : 0)>(pk);
    if constexpr (NQ > 3) off[3] = pre_at<Q0 + (NQ > 3 ? 3 : 0)>(pk);
    Pt<q32>::Raw cj[NQ];
    bool have[NQ];
    int w4[NQ];
    int n_have = 0;
#pragma unroll
    for (int u_ = 0; u_ < NQ; ++u_) {
      have[u_] = !MISS || off[u_] != kNoLoc;
      int4 piece[1];
      read_row<1>(tile, 0, have[u_] ? off[u_] : 0u, piece);
      cj[u_] = Pt<q32>::from_row(piece);
      w4[u_] = piece[0].w;
    }
#pragma unroll
    for (int u_ = 0; u_ < NQ; ++u_) {
      keep_row_word(w4[u_]);                              // the row read whole: ds_read_b128, not b96
      double d[3];
      Pt<q32>::delta(have[u_] ? cj[u_] : ci, ci, d);
      cov_add_d(acc, d[0], d[1], d[2]);
      n_have += have[u_] ? 1 : 0;
    }
    return n_have + gather_fixed_pk<NS, MISS, Q0 + 4>(tile, ci, pk, acc);
  }
}
// the second sweep over packed positions, in groups of four with a scheduling fence between them (left alone, the compiler requests
// every row piece up front and the kernel loses wavefronts per SIMD to the registers)
template <int NS, int P, int CAP, bool MISS, int Q = 0>
__device__ __forceinline__ void chain_sweep_pk(const int4* tile, const uint32_t* pk, const Pt<q32>::Raw& ci, const float* cmf, const float* vs,
                                               const float* vu, float c2f, float* gwf) {
  if constexpr (Q < NS) {
    if constexpr (Q % 4 == 0 && Q > 0) __builtin_amdgcn_sched_barrier(0);
    const uint32_t off = pre_at<Q>(pk);
    chain_term_q32<P, CAP>(tile, off, !MISS || off != kNoLoc, ci, cmf, vs, vu, c2f, gwf);
    chain_sweep_pk<NS, P, CAP, MISS, Q + 1>(tile, pk, ci, cmf, vs, vu, c2f, gwf);
  }
}
// Diagnostic build only (-DDC_BLOCK_TRACE, tools/block_trace.py): every block of the two one-pass step kernels records where and
// when it ran -- {XCC | HW_ID, start, end} on the 100 MHz constant clock -- so that the schedule of a launch can be drawn (which
// CU got how many blocks, when each CU ran dry).  The product library is built without it: the macros expand to nothing.
#ifdef DC_BLOCK_TRACE
__device__ unsigned long long* g_block_trace = nullptr;
#define DC_TRACE_BEGIN() const unsigned long long trace_t0 = __builtin_amdgcn_s_memrealtime()
#define DC_TRACE_END() do { if (threadIdx.x == 0 && g_block_trace) { \
    unsigned long long* tr_ = g_block_trace + 4 * (size_t)blockIdx.x; \
    tr_[0] = ((unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 20) << 32) | (unsigned)__builtin_amdgcn_s_getreg((31 << 11) | 4); \
    tr_[1] = trace_t0; tr_[2] = __builtin_amdgcn_s_memrealtime(); tr_[3] = 1; } } while (0)
#else
#define DC_TRACE_BEGIN() do {} while (0)
#define DC_TRACE_END() do {} while (0)
#endif

// BLOCKS: what the launch bounds ask for; dc_set_option(9, 1) runs the instantiation with six where the default is seven (A-B)
template <int NS, int P, int CAP, int BLOCKS = step_q32_blocks<P, CAP>()>
__global__ __launch_bounds__(kBlock, BLOCKS) void consistency_step_q32_kernel(
    PointBasis pb, BlockTab tab, const StepHdr* __restrict__ hdr, const int32_t* __restrict__ step_rows, const uint32_t* __restrict__ step_loc,
    const int32_t* __restrict__ centre_idx, int64_t n, LossParams lp, QParams qp, double* __restrict__ p_fwd, double* __restrict__ p_bwd, StepChain ch) {
  constexpr int NV = 2 + P, NP2 = NV <= 4 ? 4 : 8;
  constexpr int cap = CAP;
  __shared__ int4 tile[StepRow<q32, P>::kPieces * CAP];
  __shared__ double s_w[DC_MAX_MODEL_TERMS];
  __shared__ double s_front[kWavesPerBlock];
  __shared__ int s_ok[2];
  DC_TRACE_BEGIN();
  const bool chained = ch.ready != nullptr;
  if (chained && (int)blockIdx.x < ch.n_front) { chain_front_block<P>(ch, s_front); return; }
  const int64_t nblocks = (n + kBlock - 1) / kBlock;
  const int64_t blk = chain_block_of(ch, chained, nblocks);
  // the lane's loss and dL/dw; the COUNT is kept per wavefront: every lane adds 0 or 1, so the wavefront's total is the number of
  // lanes that add 1 -- the same double as their sum in any order
  double loss = 0.0, gw[P];
  bool cnt_lane = false;
#pragma unroll
  for (int k = 0; k < P; ++k) gw[k] = 0.0;
  // the block's header (StepHdr): ONE scalar load of its 64 bytes, waited for once -- everything below hangs on it and on nothing else
  // the block has to fetch first.  (The wavefront's mask word is picked from the four by scalar selects: as a second load at a
  // computed offset the compiler made it wait for the first.)
  typedef int32_t int16v __attribute__((ext_vector_type(16)));
  int16v hw = {0, 0, 0, 0, 0, kStepHdrSkip, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  if (blk >= 0) hw = *reinterpret_cast<const int16v*>(hdr + blk);
  const int wave_s = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
  const uint32_t in_lo = (uint32_t)(wave_s == 0 ? hw[8] : wave_s == 1 ? hw[10] : wave_s == 2 ? hw[12] : hw[14]);
  const uint32_t in_hi = (uint32_t)(wave_s == 0 ? hw[9] : wave_s == 1 ? hw[11] : wave_s == 2 ? hw[13] : hw[15]);
  const uint64_t in_word = ((uint64_t)in_hi << 32) | in_lo;
  const int32_t s0 = hw[0], base = hw[2], nd = hw[3], own = hw[4];
  const bool skip = (hw[5] & kStepHdrSkip) != 0;                       // padding, or no centre of this block is inside the loss mask
  bool bad = !skip && hw[1] != NS;
  if (!skip && !bad) {
    // (what is the same for the whole block stays in scalar registers -- the block's first index, its part of the table -- and a
    // lane adds its 32-bit position: no 64-bit lane index lives through the kernel)
    const uint32_t tid = threadIdx.x;
    const int64_t i0 = blk * kBlock;
    const bool live = tid < (uint32_t)hw[6];
    const bool in_mask = ((in_word >> (tid & (kWave - 1))) & 1ull) != 0;
    const uint16_t* lrow = tab.loc + (int64_t)s0 * kBlock;
    constexpr int NW = (NS + 1) / 2;
    uint32_t pk[NW];
    // step_loc (launch-uniform): the words as they are, from the block's own stretch (dcSequenceDesc.step_loc) -- one or two loads and
    // nothing to join -- and only in a wavefront that sweeps (a scalar test); else the table's 16-bit positions, joined in pairs.  Two
    // branches for the reason given at the row fetch below.
    if (step_loc) {
#pragma unroll
      for (int j = 0; j < NW; ++j) pk[j] = 0u;
      if (in_word != 0) fetch_step_loc<NW>(step_loc + (int64_t)s0 * (kBlock / 2), tid, pk);
    } else {
#pragma unroll
      for (int j = 0; j < NW; ++j)
        pk[j] = (uint32_t)lrow[(uint32_t)(2 * j * kBlock) + tid] |
                (2 * j + 1 < NS ? (uint32_t)lrow[(uint32_t)((2 * j + 1 < NS ? 2 * j + 1 : 0) * kBlock) + tid] << 16 : 0u);
    }
    const int32_t* ids = tab.blk_ids + base;
    // step_rows (launch-uniform): the rows of the block's list stored once, in the order they are staged (StepRow::fetch_listed); the
    // table of ids is then not read at all
    const int32_t* crow = step_rows ? step_rows + (int64_t)base * (6 + P) : nullptr;
    double wq[P];
    if (chained) {
      // fetch the rows this lane stages before waiting for the weights of this launch (consistency_step_basis_kernel)
      typename StepRow<q32, P>::Raw r0, r1;
      const int t0 = (int)tid, t1 = (int)tid + kBlock;
      // (the two sources as two branches here, not as one address with selected operands: a wait for a load counts every load issued
      // before it, and where the paths share code the wait for the ids stays in it -- the copy's rows would then wait for the
      // positions requested above, one trip like the one they are there to save)
      if (crow) {
        if (t0 < nd) r0 = StepRow<q32, P>::fetch_copy(crow, nd, t0);
        if (t1 < nd) r1 = StepRow<q32, P>::fetch_copy(crow, nd, t1);
      } else {
        if (t0 < nd) r0 = StepRow<q32, P>::fetch(pb, ids[t0]);
        if (t1 < nd) r1 = StepRow<q32, P>::fetch(pb, ids[t1]);
      }
      chain_weights<P>(ch, pb.w_scale, s_w, s_ok);
      __syncthreads();
      if (!s_ok[0]) bad = true;
#pragma unroll
      for (int k = 0; k < P; ++k) wq[k] = s_w[k];
      if (t0 < nd) StepRow<q32, P>::place(r0, wq, tile, cap, t0);
      if (t1 < nd) StepRow<q32, P>::place(r1, wq, tile, cap, t1);
      if (crow) for (int t = (int)tid + 2 * kBlock; t < nd; t += kBlock) StepRow<q32, P>::place(StepRow<q32, P>::fetch_copy(crow, nd, t), wq, tile, cap, t);
      else for (int t = (int)tid + 2 * kBlock; t < nd; t += kBlock) StepRow<q32, P>::stage(pb, wq, ids[t], tile, cap, t);
    } else {
      stage_weights(pb, s_w);
      __syncthreads();
#pragma unroll
      for (int k = 0; k < P; ++k) wq[k] = s_w[k];
      if (crow) for (int t = (int)tid; t < nd; t += kBlock) StepRow<q32, P>::place(StepRow<q32, P>::fetch_copy(crow, nd, t), wq, tile, cap, t);
      else for (int t = (int)tid; t < nd; t += kBlock) StepRow<q32, P>::stage(pb, wq, ids[t], tile, cap, t);
    }
    Pt<q32>::Raw ci;
    if (own < 0) ci = Basis<q32>::template point<P>(pb, wq, live ? (centre_idx ? (int64_t)(centre_idx + i0)[tid] : i0 + tid) : 0);
    __syncthreads();
    if (own >= 0) ci = staged_point<q32>(tile, cap, own + (live ? (int)tid : 0));
    // a wavefront whose centres are ALL outside the loss mask adds nothing to the loss, the count or dL/dw (every term carries the
    // centre's mask): it has staged its rows and is done.  The plan groups masked-out points at the end of every block, so
    // these are whole wavefronts (bench.py reports their share).  (The wavefront's mask word is zero: a scalar test.)
    if (live && in_word != 0) {
      CovAcc acc;
      cov_init(acc);
      // positions are multiples of 16, the empty-slot mark 0xFFFF is not: bit 0 of either half of the OR of a lane's words tells
      uint32_t mo = pk[0];
#pragma unroll
      for (int j = 1; j < NW; ++j) mo |= pk[j];
      const bool any_miss = __any((int)(mo & 0x00010001u)) != 0;
      int n_have;
      if (any_miss) n_have = gather_fixed_pk<NS, true>(tile, ci, pk, acc);
      else n_have = gather_fixed_pk<NS, false>(tile, ci, pk, acc);
      acc.W = (double)n_have;
      double cm[3], v0[3], c1, c2, acc2[2] = {0.0, 0.0};
      step_point2<q32, NS>(acc, n_have, !any_miss, in_mask, lp, qp, acc2, cm, v0, &c1, &c2);
      loss = acc2[0];
      cnt_lane = acc2[1] != 0.0;
      float cmf[3], vs[3], vu[3], gwf[P];
#pragma unroll
      for (int a = 0; a < 3; ++a) { cmf[a] = (float)cm[a]; vs[a] = (float)(c1 * v0[a]); vu[a] = (float)v0[a]; }
      const float c2f = (float)c2;
#pragma unroll
      for (int k = 0; k < P; ++k) gwf[k] = 0.0f;
      // the centre is not carried through the tail (three registers at its widest point): the same words, read again
      asm volatile("" ::: "memory");
      Pt<q32>::Raw cs;
      if (own >= 0) {
        cs = staged_point<q32>(tile, cap, own + (int)tid);
      } else {
        double w2[P];
#pragma unroll
        for (int k = 0; k < P; ++k) w2[k] = s_w[k];
        cs = Basis<q32>::template point<P>(pb, w2, centre_idx ? (int64_t)(centre_idx + i0)[tid] : i0 + tid);
      }
      if (any_miss) chain_sweep_pk<NS, P, CAP, true>(tile, pk, cs, cmf, vs, vu, c2f, gwf);
      else chain_sweep_pk<NS, P, CAP, false>(tile, pk, cs, cmf, vs, vu, c2f, gwf);
      const double u = qp.scale;
#pragma unroll
      for (int k = 0; k < P; ++k) gw[k] = (double)gwf[k] * u;          // differences were in grid steps
    }
  }
  if (chained) {
    // one row per block, summed once (step_block_row); the tile is the hand-over
    static_assert(sizeof(tile) >= step_hand_bytes<P>(), "the hand-over of step_block_row lives in the tile");
    step_block_row<P>(loss, cnt_lane, gw, bad, skip, reinterpret_cast<double*>(tile), p_fwd, p_bwd, ch.n_front);
    DC_TRACE_END();
    return;
  }
  const double nan_ = __longlong_as_double(0x7ff8000000000000ll);
  if (bad) loss = nan_;
  // ---- {sum loss, count, dL/dw} of the wavefront (one row per wavefront), as step_partials; the count's
  // column of the packed reduction carries zeros and its lane takes the number of counting lanes instead (NaN when `bad`,
  // as the sum of the lanes' NaNs was)
  const double cnt = bad ? nan_ : (double)__popcll(__ballot((int)cnt_lane));
  double v[NP2];
  v[0] = loss; v[1] = 0.0;
#pragma unroll
  for (int k = 0; k < NP2 - 2; ++k) v[2 + k] = k < P ? gw[k] : 0.0;
  double tot;
  if constexpr (NP2 == 4) tot = wave_sum4_dpp(v);
  else tot = wave_sum8_regs(v);
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  if (packed_value_of_lane<NP2>(lane & (NP2 - 1)) == 1) tot = cnt;
  const int64_t rs = (int64_t)gridDim.x * kWavesPerBlock, row = (int64_t)blockIdx.x * kWavesPerBlock + wave;
  if (lane < NP2) {
    const int q = packed_value_of_lane<NP2>(lane);
    if (q < 2) p_fwd[q * rs + row] = tot;
    else if (q < NV) p_bwd[(q - 2) * rs + row] = tot;
  }
  DC_TRACE_END();
}

// the same for any slot count (radius neighbourhoods): run-time slot loops, as consistency_fwd_basis_slots_kernel
template <typename PT, int P>
__global__ __launch_bounds__(kBlock) void consistency_step_basis_slots_kernel(
    PointBasis pb, BlockTab tab, const int32_t* __restrict__ own_base, int cap, const int32_t* __restrict__ centre_idx, int64_t n,
    const uint8_t* __restrict__ mask, LossParams lp, QParams qp, double* __restrict__ p_fwd, double* __restrict__ p_bwd,
    StepChain ch, int packed) {
  extern __shared__ int4 tile[];
  __shared__ double s_w[DC_MAX_MODEL_TERMS];
  __shared__ int s_ok;
  __shared__ double s_front[kBlock / kWave];
  const bool chained = ch.ready != nullptr;
  if (chained && (int)blockIdx.x < ch.n_front) { chain_front_block<P>(ch, s_front); return; }
  const int64_t nblocks = (n + kBlock - 1) / kBlock;
  int64_t blk = xcd_block_of((int64_t)blockIdx.x - (chained ? ch.n_front : 0), nblocks);
  if (blk >= 0 && ch.blk_skip && ch.blk_skip[blk]) blk = -1;            // no centre of this block is inside the loss mask
  double acc2[2] = {0.0, 0.0}, gw[P];
#pragma unroll
  for (int k = 0; k < P; ++k) gw[k] = 0.0;
  const int64_t i = blk * kBlock + threadIdx.x;
  const bool live = blk >= 0 && i < n;
  int32_t nslots = 0, own = -1, base = 0, nd = 0;
  const uint16_t* lrow = tab.loc;
  uint32_t pre[kPreSlots];
  if (blk >= 0) {
    const int32_t s0 = tab.slot_ptr[blk];
    nslots = tab.slot_ptr[blk + 1] - s0;
    lrow = tab.loc + (int64_t)s0 * kBlock + threadIdx.x;
#pragma unroll
    for (int q = 0; q < kPreSlots; ++q) pre[q] = (live && q < nslots) ? (uint32_t)lrow[q * kBlock] : kNoLoc;
    own = (own_base && !centre_idx) ? own_base[blk] : -1;
    base = tab.blk_ptr[blk];
    nd = tab.blk_ptr[blk + 1] - base;
  }
  double wq[P];
  bool timed_out = false;
  typename Pt<PT>::Raw ci;
  if (chained) {                           // as in consistency_step_basis_kernel: fetch, wait for the weights, place
    typename StepRow<PT, P>::Raw r0, r1;
    const int t0 = threadIdx.x, t1 = threadIdx.x + kBlock;
    if (t0 < nd) r0 = StepRow<PT, P>::fetch(pb, tab.blk_ids[base + t0]);
    if (t1 < nd) r1 = StepRow<PT, P>::fetch(pb, tab.blk_ids[base + t1]);
    chain_weights<P>(ch, pb.w_scale, s_w, &s_ok);
    __syncthreads();
    timed_out = !s_ok;
#pragma unroll
    for (int k = 0; k < P; ++k) wq[k] = s_w[k];
    if (t0 < nd) StepRow<PT, P>::place(r0, wq, tile, cap, t0);
    if (t1 < nd) StepRow<PT, P>::place(r1, wq, tile, cap, t1);
    for (int t = threadIdx.x + 2 * kBlock; t < nd; t += kBlock) StepRow<PT, P>::stage(pb, wq, tab.blk_ids[base + t], tile, cap, t);
  } else {
    stage_weights(pb, s_w);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < P; ++k) wq[k] = s_w[k];
    for (int t = threadIdx.x; t < nd; t += kBlock) StepRow<PT, P>::stage(pb, wq, tab.blk_ids[base + t], tile, cap, t);
  }
  if (blk >= 0 && own < 0) ci = Basis<PT>::template point<P>(pb, wq, live ? (centre_idx ? (int64_t)centre_idx[i] : i) : 0);
  __syncthreads();
  if (live) {
    if (own >= 0) ci = staged_point<PT>(tile, cap, own + (int)threadIdx.x);
    CovAcc acc;
    cov_init(acc);
    bool miss = false;
#pragma unroll
    for (int q = 0; q < kPreSlots; ++q) miss |= (q < nslots) && pre[q] == kNoLoc;
    int n_have = 0;
    constexpr bool kWide = std::is_same<PT, q32>::value;              // (16-byte reads of the 16-byte rows: keep_row_word)
    if (__any((int)miss)) n_have = gather_slots<PT, true, kWide>(tile, cap, ci, pre, nslots, acc);
    else n_have = gather_slots<PT, false, kWide>(tile, cap, ci, pre, nslots, acc);
    if (nslots > kPreSlots) n_have += gather_tail<PT, kWide>(tile, cap, ci, lrow, nslots, packed != 0, acc);
    acc.W = (double)n_have;
    double cm[3], v0[3], c1, c2;
    // a wavefront all of whose lanes have every slot takes W and D as the fixed-K kernels' full wavefronts do (step_point2): on a
    // table with a fixed slot count this kernel then returns their sums bit for bit
    const bool full = nslots >= 2 && !__any((int)(n_have != nslots));
    step_point2<PT, 2>(acc, n_have, full, mask ? mask[i] != 0 : true, lp, qp, acc2, cm, v0, &c1, &c2, nullptr, nslots);
    const double u = Pt<PT>::unit(qp);
    if constexpr (std::is_same<PT, q32>::value) {
      float cmf[3], vs[3], vu[3], gwf[P];
#pragma unroll
      for (int a = 0; a < 3; ++a) { cmf[a] = (float)cm[a]; vs[a] = (float)(c1 * v0[a]); vu[a] = (float)v0[a]; }
      const float c2f = (float)c2;
#pragma unroll
      for (int k = 0; k < P; ++k) gwf[k] = 0.0f;
#pragma unroll
      for (int q = 0; q < kPreSlots; ++q)
        if (q < nslots) chain_term_f32<P>(tile, cap, pre[q], pre[q] != kNoLoc, ci, cmf, vs, vu, c2f, gwf);
#pragma unroll
      for (int k = 0; k < P; ++k) gw[k] = (double)gwf[k];
      if (nslots > kPreSlots) chain_tail_f32<P>(tile, cap, lrow, nslots, packed != 0, ci, cmf, vs, vu, c2f, gw);
#pragma unroll
      for (int k = 0; k < P; ++k) gw[k] *= u;
    } else {
      double mean[3];
      StepRow<PT, P>::mean_of(ci, cm, mean);
#pragma unroll
      for (int q = 0; q < kPreSlots; ++q)
        if (q < nslots) chain_term<PT, P>(tile, cap, pre[q], pre[q] != kNoLoc, mean, v0, c1, c2, gw);
      if (nslots > kPreSlots) chain_tail<PT, P>(tile, cap, lrow, nslots, packed != 0, mean, v0, c1, c2, gw);
#pragma unroll
      for (int k = 0; k < P; ++k) gw[k] *= u;
    }
  }
  if (chained) {                                         // one row per block (step_block_row)
    step_block_row<P>(acc2[0], acc2[1] != 0.0, gw, timed_out, blk < 0, reinterpret_cast<double*>(tile), p_fwd, p_bwd, ch.n_front);
    return;
  }
  step_partials<P, true>(acc2, gw, p_fwd, p_bwd);
}

// ---- the one-pass kernel for ball neighbourhoods on float32 clouds (round 4) ------------------------------------------------
// The reference's default neighbourhood is a ball (nn_type = ball, nn_r = 0.25 m, config.py:187-189; 0.4 m in train_demo:61-63):
// on voxel-filtered scans a row has 70-200 neighbours, so the time is the two sweeps over the slots, not the per-centre tail.
// consistency_step_basis_slots_kernel spent ~58 VALU instructions per (centre, neighbour) pair at 0.65 of the issue peak; the
// arithmetic needs ~40.  What went:
//   * validity handling: an empty slot reads the lane's OWN row, whose difference to the centre is exactly zero -- one select on
//     the 16-bit position instead of selects on every coordinate and a count; the number of neighbours is the row's length
//     (dcBlockTable.row_ptr);
//   * address arithmetic: the tile's row capacity is a template argument, so the second piece of a row is an immediate off the
//     16-bit position;
//   * the dependent {position load, row read} pair per slot: trips of eight, the next trip's positions requested before the
//     rows of this one are read, and a wavefront stops at ITS longest row, not the block's;
//   * the first-sixteen-slots special case (registers kept across the per-centre tail).
// The second sweep accumulates float32 per trip and fp64 across trips.  Same sums as the slots kernel to the rounding of that
// order of additions.
template <int P, int CAP>
__global__ __launch_bounds__(kBlock, (CAP <= 1024 ? 5 : 4)) void consistency_step_ragged_q32_kernel(
    PointBasis pb, BlockTab tab, const int32_t* __restrict__ own_base, const int32_t* __restrict__ row_ptr, int64_t n,
    const uint8_t* __restrict__ mask, LossParams lp, QParams qp, double* __restrict__ p_fwd, double* __restrict__ p_bwd,
    StepChain ch) {
  using Row = StepRow<q32, P>;
  extern __shared__ int4 tile[];                   // Row::kPieces * CAP rows of 16 B (dynamic: up to 128 KB, see ragged_launch)
  __shared__ double s_w[DC_MAX_MODEL_TERMS];
  __shared__ int s_ok;
  __shared__ double s_front[kBlock / kWave];
  DC_TRACE_BEGIN();
  const bool chained = ch.ready != nullptr;
  if (chained && (int)blockIdx.x < ch.n_front) { chain_front_block<P>(ch, s_front); return; }
  const int64_t nblocks = (n + kBlock - 1) / kBlock;
  int64_t blk = xcd_block_of((int64_t)blockIdx.x - (chained ? ch.n_front : 0), nblocks);
  if (blk >= 0 && ch.blk_skip && ch.blk_skip[blk]) blk = -1;            // no centre of this block is inside the loss mask
  double acc2[2] = {0.0, 0.0}, gw[P];
#pragma unroll
  for (int k = 0; k < P; ++k) gw[k] = 0.0;
  const int64_t i = blk * kBlock + threadIdx.x;
  const bool live = blk >= 0 && i < n;
  int32_t nslots = 0, own = 0, base = 0, nd = 0, deg = 0;
  const uint16_t* lrow = tab.loc;
  uint32_t first[kTrip];
  if (blk >= 0) {
    const int32_t s0 = tab.slot_ptr[blk];
    nslots = tab.slot_ptr[blk + 1] - s0;
    lrow = tab.loc + (int64_t)s0 * kBlock + threadIdx.x;
    if (live) deg = row_ptr[i + 1] - row_ptr[i];
    own = own_base[blk];
    base = tab.blk_ptr[blk];
    nd = tab.blk_ptr[blk + 1] - base;
  }
  const uint32_t own_off = (uint32_t)(own + (int)threadIdx.x) * 16u;      // where padding slots point (and idle lanes read)
#pragma unroll
  for (int u_ = 0; u_ < kTrip; ++u_) first[u_] = (live && nslots > 0) ? (uint32_t)lrow[u_ * kBlock] : kNoLoc;     // (slot counts are multiples of 8)
  double wq[P];
  bool timed_out = false;
  if (chained) {                           // as in consistency_step_basis_kernel: fetch, wait for the weights, place
    typename Row::Raw r0, r1;
    const int t0 = threadIdx.x, t1 = threadIdx.x + kBlock;
    if (t0 < nd) r0 = Row::fetch(pb, tab.blk_ids[base + t0]);
    if (t1 < nd) r1 = Row::fetch(pb, tab.blk_ids[base + t1]);
    chain_weights<P>(ch, pb.w_scale, s_w, &s_ok);
    __syncthreads();
    timed_out = !s_ok;
#pragma unroll
    for (int k = 0; k < P; ++k) wq[k] = s_w[k];
    if (t0 < nd) Row::place(r0, wq, tile, CAP, t0);
    if (t1 < nd) Row::place(r1, wq, tile, CAP, t1);
    for (int t = threadIdx.x + 2 * kBlock; t < nd; t += kBlock) Row::stage(pb, wq, tab.blk_ids[base + t], tile, CAP, t);
  } else {
    stage_weights(pb, s_w);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < P; ++k) wq[k] = s_w[k];
    for (int t = threadIdx.x; t < nd; t += kBlock) Row::stage(pb, wq, tab.blk_ids[base + t], tile, CAP, t);
  }
  __syncthreads();
  const bool in_mask = live && (mask ? mask[i] != 0 : true);
  if (live && (!mask || __any((int)in_mask))) {          // (a wavefront of masked-out centres only: nothing to add, see consistency_step_q32_kernel)
    const char* tb = reinterpret_cast<const char*>(tile);
    const Pt<q32>::Raw ci = Pt<q32>::from_row(reinterpret_cast<const int4*>(tb + own_off));
    // the longest row among this wavefront's lanes bounds its trips
    int wmax = deg;
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) wmax = max(wmax, __shfl_xor(wmax, off, kWave));
    wmax = __builtin_amdgcn_readfirstlane(min(wmax, nslots));      // (uniform: scalar loop control)
    CovAcc acc;
    cov_init(acc);
    // one trip: the eight rows at positions l[] into the moments; the NEXT trip's positions (pn, immediates off one pointer) are
    // requested first.  Slot counts are multiples of eight and the table ends with eight rows of slack: no guards.
    auto sweep1 = [&](const uint32_t* l, uint32_t* nx, const uint16_t* pn) {
#pragma unroll
      for (int u_ = 0; u_ < kTrip; ++u_) nx[u_] = (uint32_t)pn[u_ * kBlock];
      int4 r[kTrip];
#pragma unroll
      for (int u_ = 0; u_ < kTrip; ++u_) r[u_] = *reinterpret_cast<const int4*>(tb + (l[u_] == kNoLoc ? own_off : l[u_]));
#pragma unroll
      for (int u_ = 0; u_ < kTrip; ++u_) {
        keep_row_word(r[u_].w);                           // the row read whole: ds_read_b128, not b96
        cov_add_d(acc, (double)(r[u_].x - ci.v[0]), (double)(r[u_].y - ci.v[1]), (double)(r[u_].z - ci.v[2]));
      }
    };
    {
      uint32_t la[kTrip], lb[kTrip];
#pragma unroll
      for (int u_ = 0; u_ < kTrip; ++u_) la[u_] = first[u_];
      const uint16_t* pn = lrow + kTrip * kBlock;
      for (int q0 = 0; q0 < wmax; q0 += 2 * kTrip) {        // two trips per iteration: the position registers alternate, no moves
        sweep1(la, lb, pn);
        pn += kTrip * kBlock;
        if (q0 + kTrip >= wmax) break;
        sweep1(lb, la, pn);
        pn += kTrip * kBlock;
      }
    }
    acc.W = (double)deg;
    double cm[3], v0[3], c1, c2;
    step_point2<q32, 2>(acc, deg, false, in_mask, lp, qp, acc2, cm, v0, &c1, &c2);
    const double u = Pt<q32>::unit(qp);
    float cmf[3], vs[3], vu[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) { cmf[a] = (float)cm[a]; vs[a] = (float)(c1 * v0[a]); vu[a] = (float)v0[a]; }
    const float c2f = (float)c2;
    // (two neighbours per packed float32 instruction: v_pk_fma_f32 / v_pk_mul_f32 / v_pk_add_f32 do two lanes' worth of work in
    // one issue slot -- the arithmetic of a neighbour's term drops from ~24 to ~15 instructions)
    auto sweep2 = [&](const uint32_t* l, uint32_t* nx, const uint16_t* pn) {
#pragma unroll
      for (int u_ = 0; u_ < kTrip; ++u_) nx[u_] = (uint32_t)pn[u_ * kBlock];
      float2v g[P];
#pragma unroll
      for (int k = 0; k < P; ++k) g[k] = float2v{0.0f, 0.0f};
#pragma unroll
      for (int u_ = 0; u_ < kTrip; u_ += 2) {
        const bool ha = l[u_] != kNoLoc, hb = l[u_ + 1] != kNoLoc;      // (packed rows: the same as slot < deg)
        const char* ra = tb + (ha ? l[u_] : own_off);
        const char* rb = tb + (hb ? l[u_ + 1] : own_off);
        const int4 a0 = *reinterpret_cast<const int4*>(ra), a1 = *reinterpret_cast<const int4*>(ra + CAP * 16);
        const int4 b0 = *reinterpret_cast<const int4*>(rb), b1 = *reinterpret_cast<const int4*>(rb + CAP * 16);
        const float2v e0 = float2v{(float)(a0.x - ci.v[0]), (float)(b0.x - ci.v[0])} - float2v{cmf[0], cmf[0]};
        const float2v e1 = float2v{(float)(a0.y - ci.v[1]), (float)(b0.y - ci.v[1])} - float2v{cmf[1], cmf[1]};
        const float2v e2 = float2v{(float)(a0.z - ci.v[2]), (float)(b0.z - ci.v[2])} - float2v{cmf[2], cmf[2]};
        const float2v u0 = float2v{__int_as_float(a0.w), __int_as_float(b0.w)};
        const float2v u1 = float2v{__int_as_float(a1.x), __int_as_float(b1.x)};
        const float2v u2 = float2v{__int_as_float(a1.y), __int_as_float(b1.y)};
        const float2v al = __builtin_elementwise_fma(float2v{vs[2], vs[2]}, e2, __builtin_elementwise_fma(float2v{vs[1], vs[1]}, e1, float2v{vs[0], vs[0]} * e0));
        const float2v be = __builtin_elementwise_fma(float2v{vu[2], vu[2]}, u2, __builtin_elementwise_fma(float2v{vu[1], vu[1]}, u1, float2v{vu[0], vu[0]} * u0));
        const float2v ga = __builtin_elementwise_fma(e2, u2, __builtin_elementwise_fma(e1, u1, e0 * u0));
        float2v tj = __builtin_elementwise_fma(al, be, -(float2v{c2f, c2f} * ga));
        tj = float2v{ha ? tj.x : 0.0f, hb ? tj.y : 0.0f};           // an empty slot (the lane's own row) is not a neighbour
        g[0] = __builtin_elementwise_fma(tj, float2v{__int_as_float(a1.z), __int_as_float(b1.z)}, g[0]);
        if constexpr (P > 1) g[1] = __builtin_elementwise_fma(tj, float2v{__int_as_float(a1.w), __int_as_float(b1.w)}, g[1]);
        if constexpr (P > 2)
          g[2] = __builtin_elementwise_fma(tj, float2v{__int_as_float(reinterpret_cast<const int4*>(ra + CAP * 32)->x),
                                                       __int_as_float(reinterpret_cast<const int4*>(rb + CAP * 32)->x)}, g[2]);
      }
#pragma unroll
      for (int k = 0; k < P; ++k) gw[k] += (double)(g[k].x + g[k].y);
    };
    {
      uint32_t la[kTrip], lb[kTrip];
#pragma unroll
      for (int u_ = 0; u_ < kTrip; ++u_) la[u_] = first[u_];
      const uint16_t* pn = lrow + kTrip * kBlock;
      for (int q0 = 0; q0 < wmax; q0 += 2 * kTrip) {
        sweep2(la, lb, pn);
        pn += kTrip * kBlock;
        if (q0 + kTrip >= wmax) break;
        sweep2(lb, la, pn);
        pn += kTrip * kBlock;
      }
    }
#pragma unroll
    for (int k = 0; k < P; ++k) gw[k] *= u;
  }
  if (chained) step_block_row<P>(acc2[0], acc2[1] != 0.0, gw, timed_out, blk < 0, reinterpret_cast<double*>(tile), p_fwd, p_bwd, ch.n_front);
  else step_partials<P, true>(acc2, gw, p_fwd, p_bwd);
  DC_TRACE_END();
}

}  // namespace dc
