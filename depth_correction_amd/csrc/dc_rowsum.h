// The one fixed order in which rows of block partials are summed (host and device): the finish kernels of dc_slam.hip and
// dc_align.hip, the per-scan finishing of the supervised losses (dc_scanloss.h) and the host build (dc_hostcheck.cpp).  Value q of
// the rows [n_rows, stride]: lane l of LANES takes the rows l, l + LANES, ... in order, starting from 0.0 (rows_lane_sum: one
// thread of a finish kernel each); the LANES sums are then added in lane order (rows_sum: the same additions run one after the
// other, for the host build; rows_block_totals: the kernels' two stages through LDS).
#pragma once
#include "dc_common.h"
#if defined(__HIPCC__)
#include "dc_device.h"
#endif

namespace dc {

constexpr int kRowSumLanes = 8;         // lanes that share the sum of one value over the blocks of an accumulate kernel

template <int LANES>
DC_HD double rows_lane_sum(const double* rows, int64_t n_rows, int stride, int q, int l) {
  double s = 0.0;
  int64_t r = l;
  // eight rows at a time: the loads are issued together, the additions keep their order (one load per addition would wait a
  // memory round trip each)
  for (; r + 7 * LANES < n_rows; r += 8 * LANES) {
    double v[8];
    for (int u = 0; u < 8; ++u) v[u] = rows[(r + u * LANES) * stride + q];
    for (int u = 0; u < 8; ++u) s += v[u];
  }
  for (; r < n_rows; r += LANES) s += rows[r * stride + q];
  return s;
}

template <int LANES>
DC_HD double rows_sum(const double* rows, int64_t n_rows, int stride, int q) {
  double tot = 0.0;
  for (int l = 0; l < LANES; ++l) tot += rows_lane_sum<LANES>(rows, n_rows, stride, q, l);
  return tot;
}

#if defined(__HIPCC__)
// The prologue of a one-block finish kernel (kBlock threads, all of them call): thread e takes lane e % LANES of value e / LANES
// into s_part [NV * LANES], thread q < NV then adds the LANES sums of value q in order into s_tot [NV].  Ends after the barrier
// that publishes s_tot.
template <int NV, int LANES>
__device__ __forceinline__ void rows_block_totals(const double* __restrict__ partials, int64_t n_rows, double* s_part, double* s_tot) {
  const int t = threadIdx.x;
  for (int e = t; e < NV * LANES; e += kBlock) s_part[e] = rows_lane_sum<LANES>(partials, n_rows, NV, e / LANES, e % LANES);
  __syncthreads();
  if (t < NV) {
    double s = 0.0;
    for (int l = 0; l < LANES; ++l) s += s_part[t * LANES + l];
    s_tot[t] = s;
  }
  __syncthreads();
}
#endif

}  // namespace dc
