// Plane registration, the enumeration of plane-triple pairings (DESIGN "Plane registration"; the rules: dc_planereg_math.h).
//
// Both passes are ONE kernel body (planereg_kernel<FILL>), so that they cannot disagree about which hypotheses are valid:
//   dc_planereg_count   every block owns kPregChunk consecutive hypothesis numbers of [h_begin, h_end) and walks them in tiles of
//                       kBlock, one hypothesis per lane: the number is decoded (one 64-bit decode per block, 32-bit carries per lane),
//                       rules 1 to 4 are applied from the plane tables in LDS.  That is ~60 fp64 operations, and one lane in 12 to
//                       20 passes in a room (4.8 to 8 % measured) -- the Jacobi fit, a few thousand operations, is not run here,
//                       where it would keep a wavefront busy for the few lanes that pass.
//                       The survivors are appended to a list in LDS in ascending h (ballot + popcount within a wavefront, the four
//                       wavefronts in order); when the list holds more than kBlock entries (or at the end) it is FLUSHED: lane e takes
//                       entry e, fits it (rule 5) -- at least every second lane works.  counts[block] <- the valid ones.
//   dc_planereg_fill    the same walk; a flush also scores its valid hypotheses and writes (h, T, score) at offsets[block] + the
//                       number the block has written before + the ballot prefix: the list comes out in ascending h whatever the
//                       schedule.
// Neither allocates, copies, synchronises or uses an atomic: the same inputs give the same bits.
#include "dc_common.h"
#include "../../include/dc_hip.h"
#include "dc_device.h"
#include "dc_hostutil.h"
#include "dc_planereg_math.h"

namespace dc {

constexpr int kPregTiles = 64;                                    // tiles of kBlock hypotheses a block owns
constexpr int64_t kPregChunk = (int64_t)kBlock * kPregTiles;      // 16 384 hypotheses per block
constexpr int kPregList = 2 * kBlock;                             // at most kBlock pending + kBlock new entries

// the planes of entry h: rule 1, the table bounds; returns false when h cannot be valid before any plane is read
struct PregRows {
  const double *na, *nb, *nc, *mi, *mj, *mk;
  int s;
};

__device__ __forceinline__ bool preg_rows(int64_t u, int i, int j, int k, int s, const int32_t* __restrict__ tri, int64_t n_tri, int pc,
                                          const double* s_cp, const double* s_sp, PregRows* r) {
  if (i == j || i == k || j == k || u < 0 || u >= n_tri) return false;
  const int a = tri[3 * u], b = tri[3 * u + 1], c = tri[3 * u + 2];
  if (a < 0 || a >= pc || b < 0 || b >= pc || c < 0 || c >= pc) return false;
  r->na = s_cp + 4 * a; r->nb = s_cp + 4 * b; r->nc = s_cp + 4 * c;
  r->mi = s_sp + 4 * i; r->mj = s_sp + 4 * j; r->mk = s_sp + 4 * k;
  r->s = s;
  return true;
}

// At least two waves per SIMD are asked for (the second argument of __launch_bounds__): unbounded, the compiler spends 246 / 261
// registers on the flush (one or two waves a SIMD); bounded it needs 158 / 161 and no scratch, three waves a SIMD, which is what hides
// the LDS and table latency of the rule phase.
template <bool FILL>
__global__ __launch_bounds__(kBlock, 2) void planereg_kernel(const double* __restrict__ cp, const int64_t* __restrict__ cs, int pc,
                                                          const double* __restrict__ sp, int ps, const int32_t* __restrict__ tri,
                                                          int64_t n_tri, int64_t h_begin, int64_t h_end, PregParams prm,
                                                          int32_t* __restrict__ counts, const int64_t* __restrict__ offsets,
                                                          int64_t n_valid, int64_t* __restrict__ h_out, double* __restrict__ T_out,
                                                          int64_t* __restrict__ score_out) {
  __shared__ double s_cp[kPregMaxPlanes * 4], s_sp[kPregMaxPlanes * 4];
  __shared__ int64_t s_cs[kPregMaxPlanes];
  __shared__ int64_t s_list[kPregList];
  __shared__ int s_wave[kWavesPerBlock];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
  for (int e = tid; e < pc * 4; e += kBlock) s_cp[e] = cp[e];
  for (int e = tid; e < ps * 4; e += kBlock) s_sp[e] = sp[e];
  for (int e = tid; e < pc; e += kBlock) s_cs[e] = cs[e];
  __syncthreads();
  const int64_t base = h_begin + (int64_t)blockIdx.x * kPregChunk;
  const int64_t end = base + kPregChunk < h_end ? base + kPregChunk : h_end;
  // one 64-bit decode per block: the digits of base >> 3; a lane adds its distance (< kPregChunk / 8 + kBlock) with 32-bit carries
  int64_t u0;
  int i0, j0, k0, s0;
  preg_decode(base, ps, &u0, &i0, &j0, &k0, &s0);
  const int64_t r0 = base >> 3;
  const unsigned ups = (unsigned)ps;
  int pending = 0;                                  // block-uniform: entries of s_list
  int64_t written = 0;                              // block-uniform: valid hypotheses of this block so far
  for (int64_t t0 = base; t0 < end; t0 += kBlock) {
    const int64_t h = t0 + tid;
    bool pass = false;
    if (h < end) {
      const unsigned rel = (unsigned)((h >> 3) - r0);
      unsigned v = (unsigned)k0 + rel;
      const int k = (int)(v % ups);
      v = (unsigned)j0 + v / ups;
      const int j = (int)(v % ups);
      v = (unsigned)i0 + v / ups;
      const int i = (int)(v % ups);
      const int64_t u = u0 + (int64_t)(v / ups);
      PregRows r;
      if (preg_rows(u, i, j, k, (int)(h & 7), tri, n_tri, pc, s_cp, s_sp, &r))
        pass = preg_check(r.na, r.nb, r.nc, r.mi, r.mj, r.mk, r.s, prm.min_det, prm.tol_dot) != 0;
    }
    const unsigned long long bal = __ballot(pass);
    if (lane == 0) s_wave[wave] = __popcll(bal);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kWavesPerBlock; ++w) {
      const int c = s_wave[w];
      before += w < wave ? c : 0;
      total += c;
    }
    if (pass) s_list[pending + before + __popcll(bal & ((1ull << lane) - 1ull))] = h;      // < kBlock + kBlock = kPregList
    pending += total;
    __syncthreads();
    if (pending <= kBlock && t0 + kBlock < end) continue;           // block-uniform
    for (int e0 = 0; e0 < pending; e0 += kBlock) {                  // the flush
      const int e = e0 + tid;
      bool ok = false;
      int64_t he = 0, sc = 0;
      double T[16];
      if (e < pending) {
        he = s_list[e];
        int64_t u;
        int i, j, k, s;
        preg_decode(he, ps, &u, &i, &j, &k, &s);
        PregRows r;
        if (preg_rows(u, i, j, k, s, tri, n_tri, pc, s_cp, s_sp, &r)) {
          ok = preg_fit(r.na, r.nb, r.nc, r.mi, r.mj, r.mk, r.s, T) != 0;
          if (FILL && ok) sc = preg_score(T, s_cp, s_cs, pc, s_sp, ps, prm.cos_tol, prm.tol_d);
        }
      }
      const unsigned long long vb = __ballot(ok);
      if (lane == 0) s_wave[wave] = __popcll(vb);
      __syncthreads();
      int vbefore = 0, vtotal = 0;
#pragma unroll
      for (int w = 0; w < kWavesPerBlock; ++w) {
        const int c = s_wave[w];
        vbefore += w < wave ? c : 0;
        vtotal += c;
      }
      if (FILL && ok) {
        const int64_t pos = offsets[blockIdx.x] + written + vbefore + __popcll(vb & ((1ull << lane) - 1ull));
        if (pos >= 0 && pos < n_valid) {            // offsets that are not this input's scan write nothing out of bounds
          h_out[pos] = he;
          score_out[pos] = sc;
#pragma unroll
          for (int c = 0; c < 16; ++c) T_out[pos * 16 + c] = T[c];
        }
      }
      written += vtotal;
      __syncthreads();                              // s_wave and s_list are rewritten next
    }
    pending = 0;
  }
  if (!FILL && tid == 0) counts[blockIdx.x] = (int32_t)written;
}

static int preg_launch_args(int pc, int ps, int64_t n_tri, int64_t h_begin, int64_t h_end, const PregParams& prm, int64_t* blocks) {
  if (!preg_args_ok(pc, ps, prm)) return DC_ERR_ARG;
  if (n_tri < 0 || n_tri > kPregMaxTriples) return DC_ERR_ARG;
  const int64_t total = n_tri * ps * ps * ps * 8;                   // <= 41 664 x 64^3 x 8 < 2^37
  if (h_begin < 0 || h_end < h_begin || h_end > total) return DC_ERR_ARG;
  *blocks = (h_end - h_begin + kPregChunk - 1) / kPregChunk;
  return DC_OK;
}

}  // namespace dc

using namespace dc;

extern "C" {

int64_t dc_planereg_blocks(int64_t n_hyp) { return n_hyp <= 0 ? 0 : (n_hyp + kPregChunk - 1) / kPregChunk; }

int dc_planereg_count(const double* cloud_planes, const int64_t* support, int n_cloud, const double* survey_planes, int n_survey,
                      const int32_t* triples, int64_t n_triples, int64_t h_begin, int64_t h_end, double min_det, double tol_dot,
                      double cos_tol, double tol_d, int32_t* counts, hipStream_t stream) {
  const PregParams prm{min_det, tol_dot, cos_tol, tol_d};
  int64_t blocks = 0;
  const int rc = preg_launch_args(n_cloud, n_survey, n_triples, h_begin, h_end, prm, &blocks);
  if (rc != DC_OK) return rc;
  if (blocks == 0) return DC_OK;
  if (!cloud_planes || !support || !survey_planes || !triples || !counts) return DC_ERR_ARG;
  if (blocks > 0x7fffffff) return DC_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(planereg_kernel<false>, dim3((unsigned)blocks), dim3(kBlock), 0, stream, cloud_planes, support, n_cloud,
                     survey_planes, n_survey, triples, n_triples, h_begin, h_end, prm, counts, (const int64_t*)nullptr, (int64_t)0,
                     (int64_t*)nullptr, (double*)nullptr, (int64_t*)nullptr);
  DC_HIP(hipGetLastError());
  return DC_OK;
}

int dc_planereg_fill(const double* cloud_planes, const int64_t* support, int n_cloud, const double* survey_planes, int n_survey,
                     const int32_t* triples, int64_t n_triples, int64_t h_begin, int64_t h_end, double min_det, double tol_dot,
                     double cos_tol, double tol_d, const int64_t* offsets, int64_t n_valid, int64_t* h_out, double* T_out,
                     int64_t* score_out, hipStream_t stream) {
  const PregParams prm{min_det, tol_dot, cos_tol, tol_d};
  int64_t blocks = 0;
  const int rc = preg_launch_args(n_cloud, n_survey, n_triples, h_begin, h_end, prm, &blocks);
  if (rc != DC_OK) return rc;
  if (n_valid < 0) return DC_ERR_ARG;
  if (blocks == 0 || n_valid == 0) return DC_OK;
  if (!cloud_planes || !support || !survey_planes || !triples || !offsets || !h_out || !T_out || !score_out) return DC_ERR_ARG;
  if (blocks > 0x7fffffff) return DC_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(planereg_kernel<true>, dim3((unsigned)blocks), dim3(kBlock), 0, stream, cloud_planes, support, n_cloud,
                     survey_planes, n_survey, triples, n_triples, h_begin, h_end, prm, (int32_t*)nullptr, offsets, n_valid, h_out, T_out,
                     score_out);
  DC_HIP(hipGetLastError());
  return DC_OK;
}

}  // extern "C"
