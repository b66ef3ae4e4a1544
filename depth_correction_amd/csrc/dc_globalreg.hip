// Global registration, the coarse stage (DESIGN "Global registration"; the rules: dc_globalreg_math.h).
//
//   dc_pair_spfh    one wavefront per point, lane s takes neighbour slot s (k <= 64): the pair feature and its three bins; the 33
//                   counts by one ballot + popcount per bin (integers: their order is free), lane b keeps count b -- no LDS, no
//                   dynamically indexed registers, no private segment.  spfh double [n, 33] = counts / m, m int32 [n].
//   dc_pair_fpfh    a second launch, because it gathers the first's rows of OTHER points: one wavefront per point, lane b < 33 owns
//                   value b and adds (1 / L) SPFH_j[b] slot after slot in ascending slot order (slot s's row and L come from lane s by
//                   a shuffle); every block of 11 is scaled to sum 100 (the sum in ascending bin order, by shuffles), rounded once to
//                   fp32.
//   dc_feature_nn   brute-force nearest descriptor: one cloud row per lane with its 33 values in registers, the survey's rows staged
//                   through LDS in tiles of kNnTile rows padded to 16-B multiples (every lane reads the same address: a broadcast,
//                   no bank conflict), kNnRows rows at a time so that their chains of dependent additions overlap; plain fp32 VALU
//                   arithmetic in the stated order, running best (s, index), strict < keeps the lower index among equal s.
//   dc_greg_fit     one lane per hypothesis: three draws, distinctness, edge check, moments, align_solve.
//   dc_greg_score   one wavefront per VALID hypothesis (the compacted list), lanes striding over the correspondences; the count by
//                   ballot + popcount and an integer sum: exact in any order.
//
// None allocates, copies, synchronises or uses an atomic: the same inputs give the same bits.
#include "dc_common.h"
#include "../../include/dc_hip.h"
#include "dc_device.h"
#include "dc_hostutil.h"
#include "dc_globalreg_math.h"

namespace dc {

constexpr int kNnTile = 128;                    // survey rows per LDS tile of dc_feature_nn (18 KiB + the flags)
constexpr int kNnRow = 36;                      // floats per staged row: 33 padded to a multiple of 16 B, so that a row is read 16 B at a time
constexpr int kNnRows = 4;                      // survey rows a lane works on at once: four independent chains of additions

// lane s < k: the pair (i, nbr[i, s]); returns its validity, *j the neighbour's row, *L, a [3]
__device__ __forceinline__ bool greg_slot(const double* __restrict__ points, const double* __restrict__ normals, int64_t n,
                                          const int32_t* __restrict__ nbr, int k, int64_t i, int lane, int32_t* j, double* L, double* a) {
  *j = -1;
  *L = 0.0;
  if (lane >= k) return false;
  const int32_t id = nbr[i * k + lane];
  if (id < 0 || (int64_t)id >= n) return false;
  *j = id;
  const double xi[3] = {points[i * 3], points[i * 3 + 1], points[i * 3 + 2]};
  const double ni[3] = {normals[i * 3], normals[i * 3 + 1], normals[i * 3 + 2]};
  const double xj[3] = {points[(int64_t)id * 3], points[(int64_t)id * 3 + 1], points[(int64_t)id * 3 + 2]};
  const double nj[3] = {normals[(int64_t)id * 3], normals[(int64_t)id * 3 + 1], normals[(int64_t)id * 3 + 2]};
  return greg_pair_feature(xi, ni, xj, nj, a, L) != 0;
}

__global__ __launch_bounds__(kBlock) void pair_spfh_kernel(const double* __restrict__ points, const double* __restrict__ normals, int64_t n,
                                                           const int32_t* __restrict__ nbr, int k, double* __restrict__ spfh,
                                                           int32_t* __restrict__ m_out) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t i = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  if (i >= n) return;                               // wavefront-uniform
  int32_t j;
  double L, a[3];
  const bool valid = greg_slot(points, normals, n, nbr, k, i, lane, &j, &L, a);
  const int b0 = valid ? greg_bin(a[0]) : -1, b1 = valid ? greg_bin(a[1]) : -1, b2 = valid ? greg_bin(a[2]) : -1;
  const int m = __popcll(__ballot(valid));
  int mine = 0;
#pragma unroll
  for (int b = 0; b < kGregBins; ++b) {
    const int c0 = __popcll(__ballot(b0 == b)), c1 = __popcll(__ballot(b1 == b)), c2 = __popcll(__ballot(b2 == b));
    mine = lane == b ? c0 : (lane == kGregBins + b ? c1 : (lane == 2 * kGregBins + b ? c2 : mine));
  }
  if (lane < kGregFeat) spfh[i * kGregFeat + lane] = m > 0 ? (double)mine / (double)m : 0.0;
  if (lane == 0) m_out[i] = m;
}

// (The validity and L of a slot are recomputed from the points, as in pair_spfh_kernel: nothing but the spfh rows is taken from the
// first launch, in particular not its m.)
__global__ __launch_bounds__(kBlock) void pair_fpfh_kernel(const double* __restrict__ points, const double* __restrict__ normals, int64_t n,
                                                           const int32_t* __restrict__ nbr, int k, const double* __restrict__ spfh,
                                                           float* __restrict__ feat, int32_t* __restrict__ has) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t i = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  if (i >= n) return;
  int32_t j;
  double L, a[3];
  const bool valid = greg_slot(points, normals, n, nbr, k, i, lane, &j, &L, a);
  const unsigned long long vm = __ballot(valid);
  const int m = __popcll(vm);
  const int bl = lane < kGregFeat ? lane : kGregFeat - 1;           // lanes 33 .. 63 shadow value 32 and store nothing
  double acc = 0.0;
  for (int s = 0; s < k; ++s) {
    if (!((vm >> s) & 1ull)) continue;              // wavefront-uniform
    const int32_t js = __shfl(j, s);
    const double Ls = __shfl(L, s);
    acc = greg_fpfh_term(acc, Ls, spfh[(int64_t)js * kGregFeat + bl]);
  }
  const double F = m > 0 ? greg_fpfh_value(spfh[i * kGregFeat + bl], m, acc) : 0.0;
  const int base = (bl / kGregBins) * kGregBins;
  double sum = 0.0;
#pragma unroll
  for (int q = 0; q < kGregBins; ++q) sum += __shfl(F, base + q);
  const double scale = greg_block_scale(sum);
  if (lane < kGregFeat) feat[i * kGregFeat + lane] = (float)(F * scale);
  if (lane == 0) has[i] = m > 0 ? 1 : 0;
}

// The rounding contract -- t t rounded, then added -- holds because this file is compiled with -ffp-contract=off (csrc/Makefile) and
// because of the pragma below; either alone is enough, a build route that drops both would fuse the two and change the distances.
__global__ __launch_bounds__(kBlock) void feature_nn_kernel(const float* __restrict__ fq, const int32_t* __restrict__ hq, int64_t nq,
                                                            const float* __restrict__ fs, const int32_t* __restrict__ hs, int64_t ns,
                                                            int32_t* __restrict__ idx, float* __restrict__ dist) {
#pragma clang fp contract(off)
  __shared__ __align__(16) float tile[kNnTile * kNnRow];
  __shared__ int32_t thas[kNnTile];
  const int tid = threadIdx.x;
  const int64_t i = (int64_t)blockIdx.x * kBlock + tid;
  const bool active = i < nq && hq[i] != 0;
  float q[kGregFeat];
#pragma unroll
  for (int b = 0; b < kGregFeat; ++b) q[b] = active ? fq[i * kGregFeat + b] : 0.0f;
  float best = INFINITY;
  int32_t bi = -1;
  for (int64_t r0 = 0; r0 < ns; r0 += kNnTile) {
    const int rows = (int)(ns - r0 < kNnTile ? ns - r0 : kNnTile);
    __syncthreads();                                // the previous tile has been read by every wavefront
    for (int e = tid; e < rows * kGregFeat; e += kBlock) tile[(e / kGregFeat) * kNnRow + e % kGregFeat] = fs[r0 * kGregFeat + e];
    if (tid < rows) thas[tid] = hs[r0 + tid];
    __syncthreads();
    if (!active) continue;
    for (int r = 0; r < rows; r += kNnRows) {
      float s[kNnRows];
#pragma unroll
      for (int u = 0; u < kNnRows; ++u) {
        const int ru = r + u < rows ? r + u : rows - 1;             // block-uniform; a row past the tile's end counts as unusable
        const float* row = tile + ru * kNnRow;
        float acc = 0.0f;
#pragma unroll
        for (int b = 0; b < kGregFeat; ++b) {
          const float t = q[b] - row[b];
          const float tt = t * t;
          acc = acc + tt;
        }
        s[u] = (r + u < rows && thas[ru] != 0) ? acc : INFINITY;
      }
#pragma unroll
      for (int u = 0; u < kNnRows; ++u)             // ascending rows, strict <: the lower row keeps a tie
        if (s[u] < best) { best = s[u]; bi = (int32_t)(r0 + r + u); }
    }
  }
  if (i < nq) { idx[i] = bi; dist[i] = best; }
}

__global__ __launch_bounds__(kBlock) void greg_fit_kernel(const double* __restrict__ P, const double* __restrict__ Y, int64_t C, int64_t K,
                                                          uint64_t seed, double min_edge, double rho, const double* __restrict__ origins,
                                                          int32_t* __restrict__ valid, double* __restrict__ T) {
  const int64_t h = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (h >= K) return;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  double Th[16], lam[4];
  int ok = 0;
  if (C >= 3) {
    const int64_t j0 = greg_draw(seed, (uint64_t)h, 0, C), j1 = greg_draw(seed, (uint64_t)h, 1, C), j2 = greg_draw(seed, (uint64_t)h, 2, C);
    if (j0 != j1 && j0 != j2 && j1 != j2) {
      double p[9], y[9], o[6];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        p[c] = P[j0 * 3 + c]; p[3 + c] = P[j1 * 3 + c]; p[6 + c] = P[j2 * 3 + c];
        y[c] = Y[j0 * 3 + c]; y[3 + c] = Y[j1 * 3 + c]; y[6 + c] = Y[j2 * 3 + c];
      }
#pragma unroll
      for (int c = 0; c < 6; ++c) o[c] = origins[c];
      ok = greg_check_fit(p, y, o, min_edge, rho, Th, lam);
    }
  }
  valid[h] = ok;
  for (int c = 0; c < 16; ++c) T[h * 16 + c] = ok ? Th[c] : nan;
}

__global__ __launch_bounds__(kBlock) void greg_score_kernel(const int32_t* __restrict__ list, int64_t n_list, const double* __restrict__ T,
                                                            int64_t K, const double* __restrict__ P, const double* __restrict__ Y, int64_t C,
                                                            double eps2, int32_t* __restrict__ score) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t w = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  if (w >= n_list) return;                          // wavefront-uniform
  const int64_t h = list[w];
  if (h < 0 || h >= K) return;
  double Th[12];
#pragma unroll
  for (int c = 0; c < 12; ++c) Th[c] = T[h * 16 + c];
  int count = 0;
  for (int64_t t0 = 0; t0 < C; t0 += kWave) {       // every lane takes every trip: the ballot is of the whole wavefront
    const int64_t t = t0 + lane;
    bool in = false;
    if (t < C) {
      const double p[3] = {P[t * 3], P[t * 3 + 1], P[t * 3 + 2]};
      const double y[3] = {Y[t * 3], Y[t * 3 + 1], Y[t * 3 + 2]};
      in = greg_residual2(Th, p, y) <= eps2;
    }
    count += __popcll(__ballot(in));
  }
  if (lane == 0) score[h] = count;
}

static unsigned wave_grid(int64_t n) { return (unsigned)((n + kWavesPerBlock - 1) / kWavesPerBlock); }

}  // namespace dc

using namespace dc;

extern "C" {

int dc_feature_nn_tile(void) { return kNnTile; }

int dc_pair_spfh(const double* points, const double* normals, int64_t n, const int32_t* nbr, int k, double* spfh, int32_t* m,
                 hipStream_t stream) {
  if (n < 0 || k < 1 || k > kGregMaxK) return DC_ERR_ARG;
  if (n == 0) return DC_OK;
  if (!points || !normals || !nbr || !spfh || !m) return DC_ERR_ARG;
  if (n > 0x7fffffff) return DC_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(pair_spfh_kernel, dim3(wave_grid(n)), dim3(kBlock), 0, stream, points, normals, n, nbr, k, spfh, m);
  DC_HIP(hipGetLastError());
  return DC_OK;
}

int dc_pair_fpfh(const double* points, const double* normals, int64_t n, const int32_t* nbr, int k, const double* spfh, float* feat,
                 int32_t* has, hipStream_t stream) {
  if (n < 0 || k < 1 || k > kGregMaxK) return DC_ERR_ARG;
  if (n == 0) return DC_OK;
  if (!points || !normals || !nbr || !spfh || !feat || !has) return DC_ERR_ARG;
  if (n > 0x7fffffff) return DC_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(pair_fpfh_kernel, dim3(wave_grid(n)), dim3(kBlock), 0, stream, points, normals, n, nbr, k, spfh, feat, has);
  DC_HIP(hipGetLastError());
  return DC_OK;
}

int dc_feature_nn(const float* feat_q, const int32_t* has_q, int64_t n_q, const float* feat_s, const int32_t* has_s, int64_t n_s,
                  int32_t* idx_out, float* dist_out, hipStream_t stream) {
  if (n_q < 0 || n_s < 0) return DC_ERR_ARG;
  if (n_q == 0) return DC_OK;
  if (!feat_q || !has_q || !idx_out || !dist_out || (n_s > 0 && (!feat_s || !has_s))) return DC_ERR_ARG;
  if (n_q > 0x7fffffff || n_s > 0x7fffffff) return DC_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(feature_nn_kernel, dim3((unsigned)((n_q + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, feat_q, has_q, n_q, feat_s,
                     has_s, n_s, idx_out, dist_out);
  DC_HIP(hipGetLastError());
  return DC_OK;
}

int dc_greg_fit(const double* p, const double* y, int64_t n_corr, int64_t n_hyp, int64_t seed, double min_edge, double edge_ratio,
                const double* origins, int32_t* valid, double* T, hipStream_t stream) {
  if (n_corr < 0 || n_hyp < 0) return DC_ERR_ARG;
  if (n_hyp == 0) return DC_OK;
  if (!origins || !valid || !T || (n_corr > 0 && (!p || !y))) return DC_ERR_ARG;
  if (!(min_edge >= 0.0) || !(edge_ratio > 0.0) || !(edge_ratio <= 1.0)) return DC_ERR_ARG;
  if (n_corr > 0x7fffffff || n_hyp > 0x7fffffff) return DC_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(greg_fit_kernel, dim3((unsigned)((n_hyp + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, p, y, n_corr, n_hyp,
                     (uint64_t)seed, min_edge, edge_ratio, origins, valid, T);
  DC_HIP(hipGetLastError());
  return DC_OK;
}

int dc_greg_score(const int32_t* list, int64_t n_list, const double* T, int64_t n_hyp, const double* p, const double* y, int64_t n_corr,
                  double eps, int32_t* score, hipStream_t stream) {
  if (n_list < 0 || n_hyp < 0 || n_corr < 0 || n_list > n_hyp) return DC_ERR_ARG;
  if (!(eps >= 0.0) || !(eps < INFINITY)) return DC_ERR_ARG;
  if (n_list == 0) return DC_OK;
  if (!list || !T || !score || (n_corr > 0 && (!p || !y))) return DC_ERR_ARG;
  if (n_corr > 0x7fffffff || n_hyp > 0x7fffffff) return DC_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(greg_score_kernel, dim3(wave_grid(n_list)), dim3(kBlock), 0, stream, list, n_list, T, n_hyp, p, y, n_corr, eps * eps,
                     score);
  DC_HIP(hipGetLastError());
  return DC_OK;
}

}  // extern "C"
