// Plane neighbourhoods: deterministic RANSAC plane segmentation with a least-squares refit, DBSCAN of the support on the
// radius-search grid, and the per-iteration plane moments (forward + backward) of the training loss.
//
// Reference semantics restated here (paths relative to the reference's src/depth_correction/):
//   the round loop (host, depth_correction_amd/segmentation.py)   segmentation.py:194-276
//   RANSAC + refit (PCL, set_optimize_coefficients(True))          segmentation.py:127-140
//   DBSCAN of the support, largest cluster (open3d, 10 points)     segmentation.py:166-177
//   plane features: inc = arccos(|dir . n|), model, covs          preproc.py:218-243, depth_cloud.py:417-424, utils.py:109
//
// Hypotheses (exact formula, restated by depth_correction_amd/segmentation.py:ransac_sample for the tests):
//   round m (0-based, every RANSAC call of the loop counts), hypothesis h in [0, H), t in {0, 1, 2}:
//     j_t = splitmix64(seed ^ (m << 40) ^ (h << 2) ^ t) mod n_remaining       (uint64 arithmetic)
//     p_t = x[remaining[j_t]] in fp64; u = p1 - p0, v = p2 - p0, c = u x v
//     degenerate (score -1) when two j_t coincide or |c| <= 1e-12 |u| |v|; else n = c / |c|, d = -n . p0
//   a point is an inlier when |fma(n2, x2, fma(n1, x1, n0 x0)) + d| <= thresh (fp64 whatever the cloud's dtype); counts are integer sums, the best
//   hypothesis has the largest count, ties go to the lowest h.  All H hypotheses are scored (no adaptive early stop).
// Refit: fp64 centroid and covariance of the inliers (per-block partials summed in block order; no float atomics), n = the
//   eigenvector of the smallest eigenvalue (cyclic Jacobi, dc_planemath.h), its largest-magnitude component made positive,
//   d = -n . centroid; the inliers are selected again with the refined plane.
// The per-element arithmetic (hypothesis, inlier predicate with its stated operation order, best key, refit, model, plane point,
// covariance, per-point backward) lives in dc_planemath.h, host and device; everything up to the refit is bit-identical on both.
// DBSCAN: core = >= min_pts neighbours within eps (itself included); components over core-core edges by union-find
//   (atomicMin hooking of the larger root under the smaller one + pointer jumping, until nothing changes): every label is
//   the smallest index of its component whatever the schedule.  A non-core point takes the smallest label among its core
//   neighbours, or is noise (-1).  The largest cluster wins, ties to the smaller label.
#include "dc_common.h"
#include "../../include/dc_hip.h"
#include "dc_planemath.h"

namespace dc {

namespace {
constexpr int kPBlock = kPlaneBlock;         // threads of every kernel here (4 waves of 64)
constexpr int kPWaves = kPBlock / 64;
constexpr int kScorePts = 4;                 // points per thread of the scoring kernel
constexpr int kMaxHyp = 1024;                // LDS: 32 B of plane + 16 B of per-wave counts per hypothesis

// fixed-order tree over the block: the same sum for the same inputs whatever the schedule
template <int NV>
__device__ __forceinline__ void block_sum(double (*sh)[kPBlock], double* v) {
  const int t = threadIdx.x;
  for (int k = 0; k < NV; ++k) sh[k][t] = v[k];
  __syncthreads();
  for (int s = kPBlock / 2; s > 0; s >>= 1) {
    if (t < s)
      for (int k = 0; k < NV; ++k) sh[k][t] += sh[k][t + s];
    __syncthreads();
  }
  for (int k = 0; k < NV; ++k) v[k] = sh[k][0];
}

// ---- RANSAC -------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kPBlock) void ransac_hyp_kernel(const T* __restrict__ pts, const int32_t* __restrict__ rem,
                                                             int64_t n_rem, uint64_t seed, int64_t round, int H,
                                                             double* __restrict__ hyp, double* __restrict__ anchor,
                                                             int32_t* __restrict__ valid) {
  const int h = blockIdx.x * kPBlock + threadIdx.x;
  if (h >= H) return;
  int64_t j[3];
  ransac_draw(seed, round, h, n_rem, j);
  double p[3][3];
  for (int t = 0; t < 3; ++t) load3(pts, (int64_t)rem[j[t]], p[t]);
  double pl[4];
  const bool ok = plane_from_points(p[0], p[1], p[2], j[0] != j[1] && j[0] != j[2] && j[1] != j[2], pl);
  hyp[h * 4] = pl[0]; hyp[h * 4 + 1] = pl[1]; hyp[h * 4 + 2] = pl[2]; hyp[h * 4 + 3] = pl[3];
  anchor[h * 3] = p[0][0]; anchor[h * 3 + 1] = p[0][1]; anchor[h * 3 + 2] = p[0][2];
  valid[h] = ok ? 1 : 0;
}

// every hypothesis against kPBlock * kScorePts remaining points per block: per-wave ballot counts in LDS, one integer atomic
// per hypothesis per block
template <typename T>
__global__ __launch_bounds__(kPBlock) void ransac_score_kernel(const T* __restrict__ pts, const int32_t* __restrict__ rem,
                                                               int64_t n_rem, int H, const double* __restrict__ hyp, double thresh,
                                                               int32_t* __restrict__ counts) {
  extern __shared__ double s_dyn[];
  double* s_hyp = s_dyn;                                    // [H][4]
  int32_t* s_cnt = (int32_t*)(s_dyn + 4 * H);              // [kPWaves][H]
  for (int k = threadIdx.x; k < 4 * H; k += kPBlock) s_hyp[k] = hyp[k];
  double x[kScorePts][3];
  const int64_t base = (int64_t)blockIdx.x * kPBlock * kScorePts + threadIdx.x;
  for (int q = 0; q < kScorePts; ++q) {
    const int64_t i = base + (int64_t)q * kPBlock;
    if (i < n_rem) load3(pts, (int64_t)rem[i], x[q]);
    else x[q][0] = x[q][1] = x[q][2] = (double)NAN;        // NaN is never an inlier
  }
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int h = 0; h < H; ++h) {
    const double* pl = s_hyp + 4 * h;
    int c = 0;
#pragma unroll
    for (int q = 0; q < kScorePts; ++q) c += __popcll(__ballot(plane_inlier(pl, x[q], thresh)));
    if (lane == 0) s_cnt[wave * H + h] = c;
  }
  __syncthreads();
  for (int h = threadIdx.x; h < H; h += kPBlock) {
    int s = 0;
    for (int w = 0; w < kPWaves; ++w) s += s_cnt[w * H + h];
    if (s) atomicAdd(counts + h, s);
  }
}

// best = max count, ties to the lowest h; degenerate hypotheses score -1
__global__ __launch_bounds__(kPBlock) void ransac_best_kernel(int32_t* __restrict__ counts, const int32_t* __restrict__ valid, int H,
                                                              int32_t* __restrict__ best) {
  __shared__ int64_t s_key[kPBlock];
  int64_t key = INT64_MIN;
  for (int h = threadIdx.x; h < H; h += kPBlock) {
    const int64_t k = ransac_best_key(counts[h], valid[h] != 0, H, h);
    if (!valid[h]) counts[h] = -1;
    key = k > key ? k : key;
  }
  s_key[threadIdx.x] = key;
  __syncthreads();
  for (int s = kPBlock / 2; s > 0; s >>= 1) {
    if (threadIdx.x < s && s_key[threadIdx.x + s] > s_key[threadIdx.x]) s_key[threadIdx.x] = s_key[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) ransac_best_decode(s_key[0], H, best);
}

// inlier moments of the best hypothesis about its first sample point: [count, s(3), S(6)] per block
template <typename T>
__global__ __launch_bounds__(kPBlock) void ransac_moments_kernel(const T* __restrict__ pts, const int32_t* __restrict__ rem,
                                                                 int64_t n_rem, const double* __restrict__ hyp,
                                                                 const double* __restrict__ anchor, const int32_t* __restrict__ best,
                                                                 double thresh, double* __restrict__ partials) {
  __shared__ double sh[10][kPBlock];
  const int h = best[0];
  const double pl[4] = {hyp[h * 4], hyp[h * 4 + 1], hyp[h * 4 + 2], hyp[h * 4 + 3]};
  const double a[3] = {anchor[h * 3], anchor[h * 3 + 1], anchor[h * 3 + 2]};
  double v[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int64_t i = (int64_t)blockIdx.x * kPBlock + threadIdx.x; i < n_rem; i += (int64_t)gridDim.x * kPBlock) {
    double x[3];
    load3(pts, (int64_t)rem[i], x);
    if (!plane_inlier(pl, x, thresh)) continue;
    refit_moments_add(x, a, v);
  }
  block_sum<10>(sh, v);
  if (threadIdx.x == 0)
    for (int k = 0; k < 10; ++k) partials[blockIdx.x * 10 + k] = v[k];
}

__global__ void ransac_refit_kernel(const double* __restrict__ partials, int nblk, const double* __restrict__ anchor,
                                    const int32_t* __restrict__ best, double* __restrict__ params) {
  if (threadIdx.x != 0) return;
  double v[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int b = 0; b < nblk; ++b)
    for (int k = 0; k < 10; ++k) v[k] += partials[b * 10 + k];
  plane_refit(v, anchor + best[0] * 3, params);
}

template <typename T>
__global__ __launch_bounds__(kPBlock) void plane_select_kernel(const T* __restrict__ pts, const int32_t* __restrict__ rem, int64_t n_rem,
                                                               const double* __restrict__ params, double thresh,
                                                               uint8_t* __restrict__ mask) {
  const int64_t i = (int64_t)blockIdx.x * kPBlock + threadIdx.x;
  if (i >= n_rem) return;
  double x[3];
  load3(pts, (int64_t)rem[i], x);
  const double pl[4] = {params[0], params[1], params[2], params[3]};
  mask[i] = plane_inlier(pl, x, thresh) ? 1 : 0;
}

// ---- DBSCAN -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kPBlock) void db_init_kernel(const int32_t* __restrict__ nbr, int64_t m, int K, int min_pts,
                                                          uint8_t* __restrict__ core, int32_t* __restrict__ lab) {
  const int64_t i = (int64_t)blockIdx.x * kPBlock + threadIdx.x;
  if (i >= m) return;
  int c = 0;
  for (int k = 0; k < K; ++k) c += nbr[i * K + k] >= 0;
  core[i] = c >= min_pts;
  lab[i] = (int32_t)i;
}

__device__ __forceinline__ int32_t db_find(volatile int32_t* lab, int32_t x) {
  int32_t p = lab[x];
  while (p != x) { x = p; p = lab[x]; }        // lab[x] <= x always: the walk ends
  return x;
}

__global__ __launch_bounds__(kPBlock) void db_hook_kernel(const int32_t* __restrict__ nbr, int64_t m, int K,
                                                          const uint8_t* __restrict__ core, int32_t* lab, int32_t* changed) {
  const int64_t i = (int64_t)blockIdx.x * kPBlock + threadIdx.x;
  if (i >= m || !core[i]) return;
  for (int k = 0; k < K; ++k) {
    const int32_t j = nbr[i * K + k];
    if (j < 0) break;                                   // rows are padded with -1 at the end
    if (j == i || !core[j]) continue;
    const int32_t ri = db_find(lab, (int32_t)i), rj = db_find(lab, j);
    if (ri == rj) continue;
    const int32_t hi = ri > rj ? ri : rj, lo = ri > rj ? rj : ri;
    atomicMin(lab + hi, lo);
    *changed = 1;
  }
}

__global__ __launch_bounds__(kPBlock) void db_jump_kernel(int64_t m, int32_t* lab) {
  const int64_t i = (int64_t)blockIdx.x * kPBlock + threadIdx.x;
  if (i >= m) return;
  lab[i] = db_find(lab, (int32_t)i);
}

__global__ __launch_bounds__(kPBlock) void db_final_kernel(const int32_t* __restrict__ nbr, int64_t m, int K,
                                                           const uint8_t* __restrict__ core, const int32_t* __restrict__ lab,
                                                           int32_t* __restrict__ label, int32_t* __restrict__ sizes) {
  const int64_t i = (int64_t)blockIdx.x * kPBlock + threadIdx.x;
  if (i >= m) return;
  int32_t l = -1;
  if (core[i]) {
    l = lab[i];
  } else {
    for (int k = 0; k < K; ++k) {
      const int32_t j = nbr[i * K + k];
      if (j < 0) break;
      if (core[j] && (l < 0 || lab[j] < l)) l = lab[j];
    }
  }
  label[i] = l;
  if (l >= 0) atomicAdd(sizes + l, 1);
}

__global__ __launch_bounds__(kPBlock) void db_best_kernel(const int32_t* __restrict__ sizes, int64_t m, int32_t* __restrict__ best) {
  __shared__ int64_t s_key[kPBlock];
  int64_t key = -1;
  for (int64_t l = threadIdx.x; l < m; l += kPBlock) {
    if (sizes[l] <= 0) continue;
    const int64_t k = ((int64_t)sizes[l] << 32) | (int64_t)(uint32_t)(m - 1 - l);
    key = k > key ? k : key;
  }
  s_key[threadIdx.x] = key;
  __syncthreads();
  for (int s = kPBlock / 2; s > 0; s >>= 1) {
    if (threadIdx.x < s && s_key[threadIdx.x + s] > s_key[threadIdx.x]) s_key[threadIdx.x] = s_key[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const int64_t k = s_key[0];
    best[0] = k < 0 ? -1 : (int32_t)(m - 1 - (int64_t)(uint32_t)(k & 0xffffffffll));
    best[1] = k < 0 ? 0 : (int32_t)(k >> 32);
  }
}

// ---- plane moments: forward and backward ---------------------------------------------------------------------------
// per block: [s(3), S(6)] of x - anchor over its chunk of one plane (anchor = the plane's first point)
template <typename T>
__global__ __launch_bounds__(kPBlock) void plane_fwd_kernel(const T* __restrict__ vps, const T* __restrict__ dirs, const T* __restrict__ depth,
                                                            const int32_t* __restrict__ idx, const int32_t* __restrict__ pptr,
                                                            const double* __restrict__ normals, const int32_t* __restrict__ blk_plane,
                                                            const int32_t* __restrict__ blk_begin, int chunk, int kind, int n_terms,
                                                            const double* __restrict__ w, const double* __restrict__ e,
                                                            double* __restrict__ partials) {
  __shared__ double sh[9][kPBlock];
  ModelParams mp;
  load_model_params(kind, n_terms, w, e, mp);
  const int p = blk_plane[blockIdx.x];
  const int32_t begin = blk_begin[blockIdx.x], stop = min(begin + chunk, pptr[p + 1]);
  const double n[3] = {normals[p * 3], normals[p * 3 + 1], normals[p * 3 + 2]};
  PlanePoint q;
  plane_point(vps, dirs, depth, (int64_t)idx[pptr[p]], n, mp, q);
  const double a[3] = {q.x[0], q.x[1], q.x[2]};
  double v[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int32_t r = begin + threadIdx.x; r < stop; r += kPBlock) {
    plane_point(vps, dirs, depth, (int64_t)idx[r], n, mp, q);
    plane_moments_add(q.x, a, v);
  }
  block_sum<9>(sh, v);
  if (threadIdx.x == 0)
    for (int k = 0; k < 9; ++k) partials[(int64_t)blockIdx.x * 9 + k] = v[k];
}

// one thread per plane: its blocks' partials in block order -> cov [3,3] (Bessel) and mean
template <typename T>
__global__ void plane_fwd_finish_kernel(const T* __restrict__ vps, const T* __restrict__ dirs, const T* __restrict__ depth,
                                        const int32_t* __restrict__ idx, const int32_t* __restrict__ pptr, const double* __restrict__ normals,
                                        int P, const int32_t* __restrict__ pblk, int kind, int n_terms, const double* __restrict__ w,
                                        const double* __restrict__ e, const double* __restrict__ partials, double* __restrict__ cov,
                                        double* __restrict__ mean) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P) return;
  ModelParams mp;
  load_model_params(kind, n_terms, w, e, mp);
  const double nrm[3] = {normals[p * 3], normals[p * 3 + 1], normals[p * 3 + 2]};
  PlanePoint q;
  plane_point(vps, dirs, depth, (int64_t)idx[pptr[p]], nrm, mp, q);
  double v[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int b = pblk[p]; b < pblk[p + 1]; ++b)
    for (int k = 0; k < 9; ++k) v[k] += partials[(int64_t)b * 9 + k];
  plane_cov_finish(v, (double)(pptr[p + 1] - pptr[p]), q.x, cov + (int64_t)p * 9, mean + p * 3);
}

// dL/dx = (G + G^T) (x - mean) / (n - 1), chained through x = vp + d'(d, gamma) dir, gamma = arccos |dir . n|
template <typename T>
__global__ __launch_bounds__(kPBlock) void plane_bwd_kernel(const T* __restrict__ vps, const T* __restrict__ dirs, const T* __restrict__ depth,
                                                            const int32_t* __restrict__ idx, const int32_t* __restrict__ pptr,
                                                            const double* __restrict__ normals, const int32_t* __restrict__ blk_plane,
                                                            const int32_t* __restrict__ blk_begin, int chunk, int kind, int n_terms,
                                                            const double* __restrict__ w, const double* __restrict__ e,
                                                            const double* __restrict__ mean, const double* __restrict__ gcov,
                                                            T* __restrict__ g_vps, T* __restrict__ g_dirs, T* __restrict__ g_depth,
                                                            double* __restrict__ wpartials) {
  __shared__ double sh[DC_MAX_MODEL_TERMS][kPBlock];
  ModelParams mp;
  load_model_params(kind, n_terms, w, e, mp);
  const int p = blk_plane[blockIdx.x];
  const int32_t begin = blk_begin[blockIdx.x], stop = min(begin + chunk, pptr[p + 1]);
  const double n[3] = {normals[p * 3], normals[p * 3 + 1], normals[p * 3 + 2]};
  const double mu[3] = {mean[p * 3], mean[p * 3 + 1], mean[p * 3 + 2]};
  double M[3][3];
  plane_bwd_matrix(gcov + (int64_t)p * 9, (double)(pptr[p + 1] - pptr[p] - 1), M);
  double gw[DC_MAX_MODEL_TERMS];
#pragma unroll
  for (int k = 0; k < DC_MAX_MODEL_TERMS; ++k) gw[k] = 0.0;
  PlanePoint q;
  for (int32_t r = begin + threadIdx.x; r < stop; r += kPBlock) {
    const int64_t i = (int64_t)idx[r];
    plane_point(vps, dirs, depth, i, n, mp, q);
    double gx[3], gd[3], gdep;
    const double gdp = plane_bwd_point(q, n, M, mu, mp.kind, gx, gd, &gdep);
    for (int k = 0; k < 3; ++k) {
      g_vps[i * 3 + k] = (T)gx[k];
      g_dirs[i * 3 + k] = (T)gd[k];
    }
    g_depth[i] = (T)gdep;
    if (mp.kind != DC_MODEL_NONE) {
#pragma unroll
      for (int k = 0; k < DC_MAX_MODEL_TERMS; ++k)
        if (k < n_terms) gw[k] += gdp * model_dw(mp, k, q.d, q.g);
    }
  }
  if (n_terms > 0) {
    block_sum<DC_MAX_MODEL_TERMS>(sh, gw);
    if (threadIdx.x == 0)
      for (int k = 0; k < n_terms; ++k) wpartials[(int64_t)blockIdx.x * n_terms + k] = gw[k];
  }
}

__global__ void plane_wgrad_finish_kernel(const double* __restrict__ wpartials, int nblk, int n_terms, double* __restrict__ gw) {
  const int k = threadIdx.x;
  if (k >= n_terms) return;
  double s = 0.0;
  for (int b = 0; b < nblk; ++b) s += wpartials[(int64_t)b * n_terms + k];
  gw[k] = s;
}

inline unsigned blocks_of(int64_t n) { return (unsigned)((n + kPBlock - 1) / kPBlock); }
inline int status() {
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? DC_OK : (int)e;
}
}  // namespace

}  // namespace dc

using namespace dc;

// T_ names the cloud's element type inside the launch arguments
#define DC_DISPATCH(dtype, KERNEL, grid, block, lds, stream, ...)                      \
  do {                                                                               \
    if ((dtype) == DC_F32) {                                                         \
      using T_ = float;                                                              \
      hipLaunchKernelGGL((KERNEL<T_>), grid, block, lds, stream, __VA_ARGS__);       \
    } else {                                                                         \
      using T_ = double;                                                             \
      hipLaunchKernelGGL((KERNEL<T_>), grid, block, lds, stream, __VA_ARGS__);       \
    }                                                                                \
  } while (0)

extern "C" {

int dc_ransac_score(const void* points, int dtype, const int32_t* remaining, int64_t n_rem, int64_t seed, int64_t round, int n_hyp,
                    double thresh, double* hyp, double* anchor, int32_t* valid, int32_t* counts, int32_t* best, hipStream_t stream) {
  if (!points || !remaining || !hyp || !anchor || !valid || !counts || !best) return DC_ERR_ARG;
  if (n_rem < 3 || n_rem > INT32_MAX || n_hyp < 1 || n_hyp > kMaxHyp || !(thresh >= 0.0)) return DC_ERR_ARG;
  if (dtype != DC_F32 && dtype != DC_F64) return DC_ERR_DTYPE;
  hipError_t err = hipMemsetAsync(counts, 0, sizeof(int32_t) * n_hyp, stream);
  if (err != hipSuccess) return (int)err;
  DC_DISPATCH(dtype, ransac_hyp_kernel, dim3(blocks_of(n_hyp)), dim3(kPBlock), 0, stream, (const T_*)points, remaining, n_rem,
              (uint64_t)seed, round, n_hyp, hyp, anchor, valid);
  const int64_t per_block = (int64_t)kPBlock * kScorePts;
  const dim3 grid((unsigned)((n_rem + per_block - 1) / per_block));
  const size_t lds = sizeof(double) * 4 * n_hyp + sizeof(int32_t) * kPWaves * n_hyp;
  DC_DISPATCH(dtype, ransac_score_kernel, grid, dim3(kPBlock), lds, stream, (const T_*)points, remaining, n_rem, n_hyp, hyp, thresh,
              counts);
  hipLaunchKernelGGL(ransac_best_kernel, dim3(1), dim3(kPBlock), 0, stream, counts, valid, n_hyp, best);
  return status();
}

int dc_ransac_refit_partial_count(int64_t n_rem) {
  const int64_t b = (n_rem + kPBlock - 1) / kPBlock;
  return (int)(b < 1 ? 1 : (b > 1024 ? 1024 : b));
}

int dc_ransac_refit(const void* points, int dtype, const int32_t* remaining, int64_t n_rem, const double* hyp, const double* anchor,
                    const int32_t* best, double thresh, double* partials, int n_partials, double* params, uint8_t* mask,
                    hipStream_t stream) {
  if (!points || !remaining || !hyp || !anchor || !best || !partials || !params || !mask) return DC_ERR_ARG;
  if (n_rem < 1 || n_rem > INT32_MAX || !(thresh >= 0.0)) return DC_ERR_ARG;
  if (dtype != DC_F32 && dtype != DC_F64) return DC_ERR_DTYPE;
  const int nblk = dc_ransac_refit_partial_count(n_rem);
  if (n_partials < nblk) return DC_ERR_WORKSPACE;
  DC_DISPATCH(dtype, ransac_moments_kernel, dim3(nblk), dim3(kPBlock), 0, stream, (const T_*)points, remaining, n_rem, hyp, anchor, best,
              thresh, partials);
  hipLaunchKernelGGL(ransac_refit_kernel, dim3(1), dim3(64), 0, stream, partials, nblk, anchor, best, params);
  DC_DISPATCH(dtype, plane_select_kernel, dim3(blocks_of(n_rem)), dim3(kPBlock), 0, stream, (const T_*)points, remaining, n_rem, params,
              thresh, mask);
  return status();
}

int dc_dbscan(const int32_t* nbr, int64_t m, int k, int min_pts, uint8_t* core, int32_t* lab, int32_t* label_out, int32_t* sizes,
              int32_t* flag, int32_t* best, hipStream_t stream) {
  if (!nbr || !core || !lab || !label_out || !sizes || !flag || !best || m < 1 || m > INT32_MAX || k < 1 || min_pts < 1)
    return DC_ERR_ARG;
  const dim3 grid(blocks_of(m)), block(kPBlock);
  hipLaunchKernelGGL(db_init_kernel, grid, block, 0, stream, nbr, m, k, min_pts, core, lab);
  int32_t changed = 1;
  for (int64_t it = 0; changed; ++it) {
    if (it > m) return DC_ERR_UNSUPPORTED;              // every productive pass merges two components: unreachable
    hipError_t err = hipMemsetAsync(flag, 0, sizeof(int32_t), stream);
    if (err != hipSuccess) return (int)err;
    hipLaunchKernelGGL(db_hook_kernel, grid, block, 0, stream, nbr, m, k, core, lab, flag);
    hipLaunchKernelGGL(db_jump_kernel, grid, block, 0, stream, m, lab);
    err = hipMemcpyAsync(&changed, flag, sizeof(int32_t), hipMemcpyDeviceToHost, stream);
    if (err == hipSuccess) err = hipStreamSynchronize(stream);
    if (err != hipSuccess) return (int)err;
  }
  hipError_t err = hipMemsetAsync(sizes, 0, sizeof(int32_t) * m, stream);
  if (err != hipSuccess) return (int)err;
  hipLaunchKernelGGL(db_final_kernel, grid, block, 0, stream, nbr, m, k, core, lab, label_out, sizes);
  hipLaunchKernelGGL(db_best_kernel, dim3(1), block, 0, stream, sizes, m, best);
  return status();
}

int dc_plane_moments_fwd(const void* vps, const void* dirs, const void* depth, int dtype, const int32_t* idx, const int32_t* plane_ptr,
                         const double* normals, int n_planes, const int32_t* blk_plane, const int32_t* blk_begin, const int32_t* plane_blk,
                         int n_blocks, int chunk, int model_kind, int n_terms, const double* w, const double* e, double* partials,
                         double* cov, double* mean, hipStream_t stream) {
  if (n_planes == 0) return DC_OK;
  if (!vps || !dirs || !depth || !idx || !plane_ptr || !normals || !blk_plane || !blk_begin || !plane_blk || !partials || !cov || !mean)
    return DC_ERR_ARG;
  if (n_planes < 0 || n_blocks < n_planes || chunk < 1 || n_terms < 0 || n_terms > DC_MAX_MODEL_TERMS) return DC_ERR_ARG;
  if (model_kind < DC_MODEL_NONE || model_kind > DC_MODEL_LAST || (model_kind != DC_MODEL_NONE && !w)) return DC_ERR_ARG;
  if (dtype != DC_F32 && dtype != DC_F64) return DC_ERR_DTYPE;
  DC_DISPATCH(dtype, plane_fwd_kernel, dim3(n_blocks), dim3(kPBlock), 0, stream, (const T_*)vps, (const T_*)dirs, (const T_*)depth, idx,
              plane_ptr, normals, blk_plane, blk_begin, chunk, model_kind, n_terms, w, e, partials);
  DC_DISPATCH(dtype, plane_fwd_finish_kernel, dim3((n_planes + 63) / 64), dim3(64), 0, stream, (const T_*)vps, (const T_*)dirs,
              (const T_*)depth, idx, plane_ptr, normals, n_planes, plane_blk, model_kind, n_terms, w, e, partials, cov, mean);
  return status();
}

int dc_plane_moments_bwd(const void* vps, const void* dirs, const void* depth, int dtype, const int32_t* idx, const int32_t* plane_ptr,
                         const double* normals, int n_planes, const int32_t* blk_plane, const int32_t* blk_begin, int n_blocks, int chunk,
                         int model_kind, int n_terms, const double* w, const double* e, const double* mean, const double* gcov,
                         void* g_vps, void* g_dirs, void* g_depth, double* wpartials, double* g_w, hipStream_t stream) {
  if (n_planes == 0) return DC_OK;
  if (!vps || !dirs || !depth || !idx || !plane_ptr || !normals || !blk_plane || !blk_begin || !mean || !gcov || !g_vps || !g_dirs ||
      !g_depth)
    return DC_ERR_ARG;
  if (n_planes < 0 || n_blocks < n_planes || chunk < 1 || n_terms < 0 || n_terms > DC_MAX_MODEL_TERMS) return DC_ERR_ARG;
  if (model_kind < DC_MODEL_NONE || model_kind > DC_MODEL_LAST || (model_kind != DC_MODEL_NONE && !w)) return DC_ERR_ARG;
  if (n_terms > 0 && (!wpartials || !g_w)) return DC_ERR_ARG;
  if (dtype != DC_F32 && dtype != DC_F64) return DC_ERR_DTYPE;
  DC_DISPATCH(dtype, plane_bwd_kernel, dim3(n_blocks), dim3(kPBlock), 0, stream, (const T_*)vps, (const T_*)dirs, (const T_*)depth, idx,
              plane_ptr, normals, blk_plane, blk_begin, chunk, model_kind, n_terms, w, e, mean, gcov, (T_*)g_vps, (T_*)g_dirs,
              (T_*)g_depth, wpartials);
  if (n_terms > 0)
    hipLaunchKernelGGL(plane_wgrad_finish_kernel, dim3(1), dim3(64), 0, stream, wpartials, n_blocks, n_terms, g_w);
  return status();
}

}  // extern "C"
