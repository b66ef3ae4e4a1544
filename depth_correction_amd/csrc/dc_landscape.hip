// Loss landscape over the model weights in one pass over the neighbourhoods (gfx950).  C ABI at the bottom; declarations and
// reference citations in include/dc_hip.h.
//
// Every model with a basis form is affine in its weights: x_j(w) = X0_j + s_j(w) u_j, s_j(w) = sum_k w_k c_jk (dc_points_basis).
// About a per-centre shift (the centre's own X0_i) a neighbour is y_j = a_j + sum_k w_k b_jk with a_j = X0_j - X0_i and
// b_jk = c_jk u_j, so the covariance of the neighbourhood is a quadratic form in w:
//   sum_j y_j y_j^T = Saa + sum_k w_k (Sab_k + Sab_k^T) + sum_kl w_k w_l Sbb_kl,   sum_j y_j = Sa + sum_k w_k Sb_k.
// One gather per centre accumulates those moments in fp64 (P = 2: 55 doubles); every candidate weight then costs one covariance,
// one 3x3 eigen-solve and the pointwise loss of consistency_point -- no further gathering.  Candidate weights are processed in
// chunks of kLsChunk rows per launch (bounded workspace for any W): per block and weight row the (sum, count) of its four
// wavefronts, summed in a fixed order, then a finishing launch sums the blocks in a fixed order.  No atomics: bitwise
// reproducible.  The points are not rounded to the q32 grid here (float32 clouds): the moments take X0 on the grid and the
// correction s u in fp64, which differs from the fused evaluation by less than one grid step per coordinate.
#include <cstdint>
#include "dc_common.h"
#include "../../include/dc_hip.h"
#include "dc_pointmath.h"

namespace dc {

namespace {
constexpr int kLBlock = 256;                 // threads of every kernel here (4 waves of 64)
constexpr int kLWaves = kLBlock / 64;
constexpr int kLsChunk = 128;                // weight rows per launch of the moment kernel
constexpr int kMaxBounds = 8;                // eigenvalue / eigenvalue-ratio bounds evaluated per weight row

struct EigBounds {
  int n;
  int num[kMaxBounds], den[kMaxBounds];      // lam[num] (/ lam[den]; den < 0: plain eigenvalue)
  double lo[kMaxBounds], hi[kMaxBounds];
};

// P weights: 1 + 3 + 6 + P (3 + 9) + P (P + 1) / 2 blocks of 6 or 9
template <int P> struct Moments {
  double W;
  double sa[3], saa[6];
  double sb[P][3], sab[P][9];                // sab[k][3 r + c] = sum a_r b_kc
  double sbb_d[P][6];                        // sum b_k b_k^T (symmetric)
  double sbb_o[P > 1 ? P * (P - 1) / 2 : 1][9];   // sum b_k b_l^T, k < l
};

template <int P> __device__ __forceinline__ void mom_init(Moments<P>& m) {
  m.W = 0.0;
#pragma unroll
  for (int r = 0; r < 3; ++r) m.sa[r] = 0.0;
#pragma unroll
  for (int r = 0; r < 6; ++r) m.saa[r] = 0.0;
#pragma unroll
  for (int k = 0; k < P; ++k) {
#pragma unroll
    for (int r = 0; r < 3; ++r) m.sb[k][r] = 0.0;
#pragma unroll
    for (int r = 0; r < 9; ++r) m.sab[k][r] = 0.0;
#pragma unroll
    for (int r = 0; r < 6; ++r) m.sbb_d[k][r] = 0.0;
  }
#pragma unroll
  for (int q = 0; q < (P > 1 ? P * (P - 1) / 2 : 1); ++q)
#pragma unroll
    for (int r = 0; r < 9; ++r) m.sbb_o[q][r] = 0.0;
}

__device__ __forceinline__ void sym_add(double* s, const double* x, const double* y) {     // s += x y^T (x == y), xx xy xz yy yz zz
  s[0] = fma(x[0], y[0], s[0]); s[1] = fma(x[0], y[1], s[1]); s[2] = fma(x[0], y[2], s[2]);
  s[3] = fma(x[1], y[1], s[3]); s[4] = fma(x[1], y[2], s[4]); s[5] = fma(x[2], y[2], s[5]);
}
__device__ __forceinline__ void full_add(double* s, const double* x, const double* y) {    // s += x y^T
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) s[3 * r + c] = fma(x[r], y[c], s[3 * r + c]);
}

// one member y = a + sum_k w_k c_k u of a neighbourhood (a: offset from the shift at w = 0)
template <int P>
__device__ __forceinline__ void mom_add(Moments<P>& m, const double* a, const double* c, const double* u) {
  m.W += 1.0;
#pragma unroll
  for (int r = 0; r < 3; ++r) m.sa[r] += a[r];
  sym_add(m.saa, a, a);
  double b[P][3];
#pragma unroll
  for (int kk = 0; kk < P; ++kk) {
#pragma unroll
    for (int r = 0; r < 3; ++r) { b[kk][r] = c[kk] * u[r]; m.sb[kk][r] += b[kk][r]; }
    full_add(m.sab[kk], a, b[kk]);
    sym_add(m.sbb_d[kk], b[kk], b[kk]);
  }
  int o = 0;
#pragma unroll
  for (int k0 = 0; k0 < P; ++k0)
#pragma unroll
    for (int k1 = k0 + 1; k1 < P; ++k1) full_add(m.sbb_o[o++], b[k0], b[k1]);
}

// a row of the basis: q32 (float32 clouds: X0 int32 on the grid, u and c float32) or fp64
template <bool Q32, int P>
__device__ __forceinline__ void load_row(const void* rows, int64_t j, int64_t* xq, double* x, double* u, double* c) {
  if (Q32) {
    const int32_t* r = static_cast<const int32_t*>(rows) + j * (6 + P);
#pragma unroll
    for (int a = 0; a < 3; ++a) { xq[a] = r[a]; u[a] = (double)__int_as_float(r[3 + a]); }
#pragma unroll
    for (int k = 0; k < P; ++k) c[k] = (double)__int_as_float(r[6 + k]);
  } else {
    const double* r = static_cast<const double*>(rows) + j * (6 + P);
#pragma unroll
    for (int a = 0; a < 3; ++a) { x[a] = r[a]; u[a] = r[3 + a]; }
#pragma unroll
    for (int k = 0; k < P; ++k) c[k] = r[6 + k];
  }
}

template <bool Q32, int P>
__device__ __forceinline__ void gather_moments(const void* rows, const int32_t* __restrict__ nbr, int64_t n, int k, int64_t i,
                                               double step, Moments<P>& m) {
  int64_t xqi[3];
  double xi[3], ui[3], ci[P];
  load_row<Q32, P>(rows, i, xqi, xi, ui, ci);
  const int32_t* row = nbr + i * (int64_t)k;
  for (int q = 0; q < k; ++q) {
    const int32_t j = row[q];
    if (j < 0 || j >= n) continue;
    int64_t xq[3];
    double x[3], u[3], c[P], a[3];
    load_row<Q32, P>(rows, j, xq, x, u, c);
#pragma unroll
    for (int r = 0; r < 3; ++r) a[r] = Q32 ? (double)(xq[r] - xqi[r]) * step : x[r] - xi[r];
    mom_add<P>(m, a, c, u);
  }
}

// C(w) with cov_finish's normalisation (validity weights, omega = 1, D = max(W - 1, 1e-6))
// (PLANE: plane_fwd_finish_kernel's normalisation 1 / (n - 1) without the clamp: one point gives NaN like torch.cov)
template <int P, bool PLANE = false>
__device__ __forceinline__ void cov_of(const Moments<P>& m, const double* w, double* C, double* D_out) {
  double s[3], S[6];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    s[r] = m.sa[r];
#pragma unroll
    for (int k = 0; k < P; ++k) s[r] = fma(w[k], m.sb[k][r], s[r]);
  }
  constexpr int rr[6] = {0, 0, 0, 1, 1, 2}, cc[6] = {0, 1, 2, 1, 2, 2};
#pragma unroll
  for (int e = 0; e < 6; ++e) {
    const int r = rr[e], c = cc[e];
    double v = m.saa[e];
#pragma unroll
    for (int k = 0; k < P; ++k) {
      v = fma(w[k], m.sab[k][3 * r + c] + m.sab[k][3 * c + r], v);
      v = fma(w[k] * w[k], m.sbb_d[k][e], v);
    }
    int o = 0;
#pragma unroll
    for (int k0 = 0; k0 < P; ++k0)
#pragma unroll
      for (int k1 = k0 + 1; k1 < P; ++k1) {
        v = fma(w[k0] * w[k1], m.sbb_o[o][3 * r + c] + m.sbb_o[o][3 * c + r], v);
        ++o;
      }
    S[e] = v;
  }
  double D = m.W - 1.0;
  if (!PLANE) D = D < 1e-6 ? 1e-6 : D;
  const double invW = recip_(m.W);                           // W = 0 -> inf: 0 * inf = NaN, like cov_finish
  const double c0 = s[0] * invW, c1 = s[1] * invW, c2 = s[2] * invW;
  const double f = PLANE ? 1.0 / D : recip_(D);
  C[0] = (S[0] - s[0] * c0) * f;
  C[1] = (S[1] - s[0] * c1) * f;
  C[2] = (S[2] - s[0] * c2) * f;
  C[3] = (S[3] - s[1] * c1) * f;
  C[4] = (S[4] - s[1] * c2) * f;
  C[5] = (S[5] - s[2] * c2) * f;
  *D_out = D;
}

__device__ __forceinline__ bool within(double v, double lo, double hi) {     // filters.within_bounds: NaN fails active bounds
  bool keep = true;
  if (lo > -INFINITY) keep = keep && (v >= lo);
  if (hi < INFINITY) keep = keep && (v <= hi);
  return keep;
}

// Pointwise loss of a centre for one weight row: the math of consistency_point after the gather (no offset, no NaN policy),
// plus the per-w eigenvalue / eigenvalue-ratio bounds of global_cloud_mask when `eb.n > 0`.  Returns whether the centre counts.
template <int P, bool BOUNDS>
__device__ __forceinline__ bool point_loss(const Moments<P>& m, const double* w, const LossParams& lp, const EigBounds& eb,
                                           double* l_out) {
  double C[6], D, lam0, tr;
  cov_of<P>(m, w, C, &D);
  bool keep = true;
  if (BOUNDS) {
    double lam[3], V[3][3];
    eig3_sym_v2(C[0], C[1], C[2], C[3], C[4], C[5], lam, V);
    lam0 = lam[0];
    tr = C[0] + C[3] + C[5];
    for (int b = 0; b < eb.n; ++b) {
      const double v = eb.den[b] >= 0 ? lam[eb.num[b]] / lam[eb.den[b]] : lam[eb.num[b]];
      keep = keep && within(v, eb.lo[b], eb.hi[b]);
    }
  } else {
    double v0[3];
    eig3_smallest(C[0], C[1], C[2], C[3], C[4], C[5], &lam0, v0, &tr);
  }
  double c1, c2;
  *l_out = loss_and_coeffs(lp, lam0, tr, D, 0.0, keep, &c1, &c2);
  return keep;
}

__device__ __forceinline__ double wave_sum_l(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// One centre per lane; weight rows w0 .. w0 + nw (nw <= kLsChunk).  partials [gridDim.x, kLsChunk, 2].
template <bool Q32, int P, bool BOUNDS>
__global__ __launch_bounds__(kLBlock) void sequence_landscape_kernel(const void* __restrict__ rows, double step,
                                                                     const int32_t* __restrict__ nbr, int64_t n, int k,
                                                                     const uint8_t* __restrict__ mask, const double* __restrict__ weights,
                                                                     int nw, LossParams lp, EigBounds eb, double* __restrict__ partials) {
  __shared__ double s_w[kLsChunk * P];
  __shared__ double s_red[kLWaves][kLsChunk][2];
  for (int t = threadIdx.x; t < nw * P; t += kLBlock) s_w[t] = weights[t];
  const int64_t i = (int64_t)blockIdx.x * kLBlock + threadIdx.x;
  const bool active = i < n && (mask ? mask[i] != 0 : true);
  Moments<P> m;
  mom_init<P>(m);
  if (active) gather_moments<Q32, P>(rows, nbr, n, k, i, step, m);
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool any = __any((int)active);
  for (int r = 0; r < nw; ++r) {
    double v[2] = {0.0, 0.0};
    if (any) {
      if (active) {
        double l;
        if (point_loss<P, BOUNDS>(m, s_w + r * P, lp, eb, &l)) { v[0] = l; v[1] = 1.0; }
      }
      v[0] = wave_sum_l(v[0]);
      v[1] = wave_sum_l(v[1]);
    }
    if (lane == 0) { s_red[wave][r][0] = v[0]; s_red[wave][r][1] = v[1]; }
  }
  __syncthreads();
  for (int t = threadIdx.x; t < nw * 2; t += kLBlock) {
    const int r = t >> 1, q = t & 1;
    double s = 0.0;
#pragma unroll
    for (int wv = 0; wv < kLWaves; ++wv) s += s_red[wv][r][q];
    partials[((int64_t)blockIdx.x * kLsChunk + r) * 2 + q] = s;
  }
}

// out[(w0 + r) * 2 + q] = sum over the blocks of partials[b, r, q], fixed order (one block per (r, q))
__global__ __launch_bounds__(kLBlock) void landscape_finish_kernel(const double* __restrict__ partials, int64_t n_blocks, int row_stride,
                                                                   double* __restrict__ out) {
  __shared__ double s[kLBlock];
  const int r = blockIdx.x >> 1, q = blockIdx.x & 1;
  double v = 0.0;
  for (int64_t b = threadIdx.x; b < n_blocks; b += kLBlock) v += partials[(b * row_stride + r) * 2 + q];
  s[threadIdx.x] = v;
  __syncthreads();
  for (int h = kLBlock / 2; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) s[threadIdx.x] += s[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[r * 2 + q] = s[0];
}

// ---- plane neighbourhoods ---------------------------------------------------------------------------------------------------
// The plane features of preproc.py:218-243 (plane_fwd_kernel): x = vp + d'(d, gamma) dir with gamma = arccos |dir . n_p| fixed per
// plane; for the polynomial models d' = d + sum_k w_k c_k, c_k = -gamma^e_k (Polynomial) or -d gamma^e_k (ScaledPolynomial), so
// x = X0 + sum_k w_k c_k dir, and the plane's covariance is the same quadratic form in w about the plane's first point at w = 0.
template <int P> constexpr int kMomentCount = (int)(sizeof(Moments<P>) / sizeof(double));

template <typename T>
__device__ __forceinline__ void plane_basis_point(const T* vps, const T* dirs, const T* depth, int64_t i, const double* n, int kind,
                                                  const double* e, int np, double* x0, double* dir, double* c) {
  double vp[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) { vp[a] = (double)vps[i * 3 + a]; dir[a] = (double)dirs[i * 3 + a]; }
  const double d = (double)depth[i];
  const double cs = fabs(dir[0] * n[0] + dir[1] * n[1] + dir[2] * n[2]);
  const double g = acos(cs > 1.0 ? 1.0 : cs);
#pragma unroll
  for (int k = 0; k < DC_MAX_MODEL_TERMS; ++k)
    if (k < np) c[k] = (kind == DC_MODEL_SCALED_POLYNOMIAL ? -d : -1.0) * pow_term(g, e[k]);
#pragma unroll
  for (int a = 0; a < 3; ++a) x0[a] = vp[a] + d * dir[a];
}

// per block (a chunk of one plane, plane_fwd_kernel's work split): the kMomentCount<P> moments about the plane's first point
template <typename T, int P>
__global__ __launch_bounds__(kLBlock) void plane_landscape_moments_kernel(const T* __restrict__ vps, const T* __restrict__ dirs,
                                                                          const T* __restrict__ depth, const int32_t* __restrict__ idx,
                                                                          const int32_t* __restrict__ pptr, const double* __restrict__ normals,
                                                                          const int32_t* __restrict__ blk_plane,
                                                                          const int32_t* __restrict__ blk_begin, int chunk, int kind,
                                                                          const double* __restrict__ e, double* __restrict__ partials) {
  constexpr int NM = kMomentCount<P>;
  __shared__ double s_red[kLWaves][NM];
  const int p = blk_plane[blockIdx.x];
  const int32_t begin = blk_begin[blockIdx.x], stop = min(begin + chunk, pptr[p + 1]);
  const double n[3] = {normals[p * 3], normals[p * 3 + 1], normals[p * 3 + 2]};
  double ek[P];
#pragma unroll
  for (int k = 0; k < P; ++k) ek[k] = e[k];
  double anchor[3], dir[3], c[P];
  plane_basis_point(vps, dirs, depth, (int64_t)idx[pptr[p]], n, kind, ek, P, anchor, dir, c);
  Moments<P> m;
  mom_init<P>(m);
  for (int32_t r = begin + threadIdx.x; r < stop; r += kLBlock) {
    double x0[3], a[3];
    plane_basis_point(vps, dirs, depth, (int64_t)idx[r], n, kind, ek, P, x0, dir, c);
#pragma unroll
    for (int q = 0; q < 3; ++q) a[q] = x0[q] - anchor[q];
    mom_add<P>(m, a, c, dir);
  }
  const double* v = reinterpret_cast<const double*>(&m);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < NM; ++q) {
    const double t = wave_sum_l(v[q]);
    if (lane == 0) s_red[wave][q] = t;
  }
  __syncthreads();
  for (int q = threadIdx.x; q < NM; q += kLBlock) {
    double t = 0.0;
#pragma unroll
    for (int wv = 0; wv < kLWaves; ++wv) t += s_red[wv][q];
    partials[(int64_t)blockIdx.x * NM + q] = t;
  }
}

// plane moments [n_planes, NM]: the plane's block partials in block order
__global__ __launch_bounds__(kLBlock) void plane_landscape_reduce_kernel(const double* __restrict__ partials, const int32_t* __restrict__ pblk,
                                                                         int n_planes, int nm, double* __restrict__ pm) {
  const int64_t t = (int64_t)blockIdx.x * kLBlock + threadIdx.x;
  if (t >= (int64_t)n_planes * nm) return;
  const int p = (int)(t / nm), q = (int)(t % nm);
  double s = 0.0;
  for (int b = pblk[p]; b < pblk[p + 1]; ++b) s += partials[(int64_t)b * nm + q];
  pm[t] = s;
}

// one thread per weight row: cov(w) of every plane (in plane order), eigenvalues, the loss of loss.py:216-294 over the planes
// (every plane is one entry; mask: the planes that count) -> out[r] = (sum, count)
template <int P>
__global__ __launch_bounds__(kLBlock) void plane_landscape_loss_kernel(const double* __restrict__ pm, int n_planes,
                                                                       const uint8_t* __restrict__ mask, const double* __restrict__ weights,
                                                                       int64_t n_w, LossParams lp, double* __restrict__ out) {
  constexpr int NM = kMomentCount<P>;
  const int64_t r = (int64_t)blockIdx.x * kLBlock + threadIdx.x;
  if (r >= n_w) return;
  double w[P];
#pragma unroll
  for (int k = 0; k < P; ++k) w[k] = weights[r * P + k];
  double sum = 0.0, cnt = 0.0;
  for (int p = 0; p < n_planes; ++p) {
    if (mask && !mask[p]) continue;
    Moments<P> m;
    double* v = reinterpret_cast<double*>(&m);
    for (int q = 0; q < NM; ++q) v[q] = pm[(int64_t)p * NM + q];
    double C[6], D, lam[3], V[3][3], c1, c2;
    cov_of<P, true>(m, w, C, &D);
    eig3_sym_v2(C[0], C[1], C[2], C[3], C[4], C[5], lam, V);
    // min_eigval_loss normalises by the eigenvalue sum, trace_loss takes the trace of cov
    const double tr = lp.kind == DC_LOSS_TRACE ? C[0] + C[3] + C[5] : lam[0] + lam[1] + lam[2];
    sum += loss_and_coeffs(lp, lam[0], tr, D, 0.0, true, &c1, &c2);
    cnt += 1.0;
  }
  out[r * 2] = sum;
  out[r * 2 + 1] = cnt;
}

inline int status() {
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? DC_OK : (int)e;
}

template <bool Q32, int P>
void launch_sequence(bool bounds, dim3 grid, hipStream_t stream, const void* rows, double step, const int32_t* nbr, int64_t n, int k,
                     const uint8_t* mask, const double* weights, int nw, const LossParams& lp, const EigBounds& eb, double* partials) {
  if (bounds)
    hipLaunchKernelGGL((sequence_landscape_kernel<Q32, P, true>), grid, dim3(kLBlock), 0, stream, rows, step, nbr, n, k, mask, weights,
                       nw, lp, eb, partials);
  else
    hipLaunchKernelGGL((sequence_landscape_kernel<Q32, P, false>), grid, dim3(kLBlock), 0, stream, rows, step, nbr, n, k, mask, weights,
                       nw, lp, eb, partials);
}
}  // namespace

}  // namespace dc

using namespace dc;

extern "C" {

int64_t dc_sequence_landscape_workspace_count(int64_t n) {
  const int64_t nb = (n + kLBlock - 1) / kLBlock;
  return (nb < 1 ? 1 : nb) * kLsChunk * 2;
}

int dc_sequence_landscape(const void* rows, int point_fmt, double step, int n_terms, const int32_t* nbr, int64_t n, int k,
                          const uint8_t* mask, const double* weights, int64_t n_w, int loss_kind, int normalization, int sqrt_,
                          int n_bounds, const double* bounds, double* workspace, int64_t workspace_count, double* out,
                          hipStream_t stream) {
  if (n_w == 0) return DC_OK;
  if (n < 0 || n > INT32_MAX || k < 0 || n_w < 0 || !weights || !out) return DC_ERR_ARG;
  if (n > 0 && (!rows || !nbr || !workspace)) return DC_ERR_ARG;
  if (point_fmt != DC_Q32 && point_fmt != DC_F64) return DC_ERR_DTYPE;
  if (point_fmt == DC_Q32 && !(step > 0.0)) return DC_ERR_ARG;
  if (n_terms != 1 && n_terms != 2) return DC_ERR_UNSUPPORTED;
  if (loss_kind != DC_LOSS_MIN_EIGVAL && loss_kind != DC_LOSS_TRACE) return DC_ERR_UNSUPPORTED;
  if (n_bounds < 0 || n_bounds > kMaxBounds || (n_bounds > 0 && !bounds)) return DC_ERR_ARG;
  EigBounds eb{};
  eb.n = n_bounds;
  for (int b = 0; b < n_bounds; ++b) {            // host array [n_bounds, 4]: num, den (-1: none), lo, hi
    eb.num[b] = (int)bounds[4 * b];
    eb.den[b] = (int)bounds[4 * b + 1];
    eb.lo[b] = bounds[4 * b + 2];
    eb.hi[b] = bounds[4 * b + 3];
    if (eb.num[b] < 0 || eb.num[b] > 2 || eb.den[b] < -1 || eb.den[b] > 2) return DC_ERR_ARG;
  }
  if (n == 0) return (int)hipMemsetAsync(out, 0, sizeof(double) * 2 * n_w, stream);
  const int64_t nb = (n + kLBlock - 1) / kLBlock;
  if (workspace_count < dc_sequence_landscape_workspace_count(n)) return DC_ERR_WORKSPACE;
  const LossParams lp = make_loss_params(loss_kind, normalization, sqrt_);
  const bool q32 = point_fmt == DC_Q32;
  for (int64_t w0 = 0; w0 < n_w; w0 += kLsChunk) {
    const int nw = (int)(n_w - w0 < kLsChunk ? n_w - w0 : kLsChunk);
    const double* wc = weights + w0 * n_terms;
    const dim3 grid((unsigned)nb);
    if (q32 && n_terms == 1) launch_sequence<true, 1>(n_bounds > 0, grid, stream, rows, step, nbr, n, k, mask, wc, nw, lp, eb, workspace);
    else if (q32) launch_sequence<true, 2>(n_bounds > 0, grid, stream, rows, step, nbr, n, k, mask, wc, nw, lp, eb, workspace);
    else if (n_terms == 1) launch_sequence<false, 1>(n_bounds > 0, grid, stream, rows, step, nbr, n, k, mask, wc, nw, lp, eb, workspace);
    else launch_sequence<false, 2>(n_bounds > 0, grid, stream, rows, step, nbr, n, k, mask, wc, nw, lp, eb, workspace);
    hipLaunchKernelGGL(landscape_finish_kernel, dim3((unsigned)(2 * nw)), dim3(kLBlock), 0, stream, workspace, nb, kLsChunk,
                       out + 2 * w0);
  }
  return status();
}

int dc_plane_landscape_partials_count(int n_blocks, int n_terms) {
  if (n_blocks < 0 || (n_terms != 1 && n_terms != 2)) return -1;
  return (n_blocks < 1 ? 1 : n_blocks) * (n_terms == 1 ? kMomentCount<1> : kMomentCount<2>);
}

int dc_plane_landscape(const void* vps, const void* dirs, const void* depth, int dtype, const int32_t* idx, const int32_t* plane_ptr,
                       const double* normals, int n_planes, const int32_t* blk_plane, const int32_t* blk_begin, const int32_t* plane_blk,
                       int n_blocks, int chunk, int model_kind, int n_terms, const double* e, const uint8_t* mask, const double* weights,
                       int64_t n_w, int loss_kind, int normalization, int sqrt_, double* partials, int64_t partials_count,
                       double* plane_moments, double* out, hipStream_t stream) {
  if (n_w == 0) return DC_OK;
  if (n_w < 0 || !weights || !out || n_planes < 0) return DC_ERR_ARG;
  if (n_terms != 1 && n_terms != 2) return DC_ERR_UNSUPPORTED;
  if (model_kind != DC_MODEL_POLYNOMIAL && model_kind != DC_MODEL_SCALED_POLYNOMIAL) return DC_ERR_UNSUPPORTED;
  if (loss_kind != DC_LOSS_MIN_EIGVAL && loss_kind != DC_LOSS_TRACE) return DC_ERR_UNSUPPORTED;
  if (dtype != DC_F32 && dtype != DC_F64) return DC_ERR_DTYPE;
  const LossParams lp = make_loss_params(loss_kind, normalization, sqrt_);
  const int nm = n_terms == 1 ? kMomentCount<1> : kMomentCount<2>;
  const dim3 wgrid((unsigned)((n_w + kLBlock - 1) / kLBlock));
  if (n_planes == 0) {                        // no plane: every row is 0 / 0 (the loop's mean over no entry)
    if (n_terms == 1) hipLaunchKernelGGL(plane_landscape_loss_kernel<1>, wgrid, dim3(kLBlock), 0, stream, plane_moments, 0, mask, weights, n_w, lp, out);
    else hipLaunchKernelGGL(plane_landscape_loss_kernel<2>, wgrid, dim3(kLBlock), 0, stream, plane_moments, 0, mask, weights, n_w, lp, out);
    return status();
  }
  if (!vps || !dirs || !depth || !idx || !plane_ptr || !normals || !blk_plane || !blk_begin || !plane_blk || !e || !partials || !plane_moments)
    return DC_ERR_ARG;
  if (n_blocks < n_planes || chunk < 1) return DC_ERR_ARG;
  if (partials_count < (int64_t)n_blocks * nm) return DC_ERR_WORKSPACE;
  const dim3 grid((unsigned)n_blocks), block(kLBlock);
#define DC_PLANE_MOMENTS(T_, P_)                                                                                                  \
  hipLaunchKernelGGL((plane_landscape_moments_kernel<T_, P_>), grid, block, 0, stream, (const T_*)vps, (const T_*)dirs,            \
                     (const T_*)depth, idx, plane_ptr, normals, blk_plane, blk_begin, chunk, model_kind, e, partials)
  if (dtype == DC_F32) { if (n_terms == 1) DC_PLANE_MOMENTS(float, 1); else DC_PLANE_MOMENTS(float, 2); }
  else { if (n_terms == 1) DC_PLANE_MOMENTS(double, 1); else DC_PLANE_MOMENTS(double, 2); }
#undef DC_PLANE_MOMENTS
  const int64_t nt = (int64_t)n_planes * nm;
  hipLaunchKernelGGL(plane_landscape_reduce_kernel, dim3((unsigned)((nt + kLBlock - 1) / kLBlock)), block, 0, stream, partials, plane_blk,
                     n_planes, nm, plane_moments);
  if (n_terms == 1)
    hipLaunchKernelGGL(plane_landscape_loss_kernel<1>, wgrid, block, 0, stream, plane_moments, n_planes, mask, weights, n_w, lp, out);
  else
    hipLaunchKernelGGL(plane_landscape_loss_kernel<2>, wgrid, block, 0, stream, plane_moments, n_planes, mask, weights, n_w, lp, out);
  return status();
}

}  // extern "C"
