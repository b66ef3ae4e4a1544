// Sparse TSDF volumes: block-allocated fusion of posed scans and surface-nets extraction (DESIGN "Sparse TSDF volumes"; the rules:
// dc_tsdf_sparse_math.h and dc_tsdf_math.h, whose functions the kernels inline).
//
//   dc_tsdf_sparse_allocate    candidates   one lane per ray runs the sample loop and writes the key of every visit that adds and whose
//                                           block is not in the table (binary search, once per block change of the lane) into the ray's
//                                           share of 2K + 1 keys, the rest of the share the no-key;
//                              the library's 64-bit key sort; heads (first of each run of equal keys) and their exclusive scan;
//                              compact      the first capacity - n_blocks heads, ascending, are the admitted keys;
//                              merge, copy  old and admitted entries are ranked against each other by binary search into a second table,
//                                           which is copied back: the table stays sorted, the new slots are n_blocks, n_blocks + 1, ...;
//                              finish       n_blocks and info.  No compare-and-swap, no spinning, no host read.
//   dc_tsdf_sparse_integrate   one lane per ray as dc_tsdf_integrate; a visit finds its slot (the lane keeps its last key and position) and
//                              does the same two integer atomics at slot 512 + local; a visit without a block counts in dropped.
//   dc_tsdf_sparse_extract_*   neighbours   nbr [n_blocks, 27] by binary search; then count, scan, fill as in dc_tsdf.hip with one lane per
//                                           (position, local index): vertices ascend in (key, local cell), faces in (key, local q, e).
// Nothing here allocates, copies or synchronises; no floating-point atomic anywhere.
#include "dc_common.h"
#include "../../include/dc_hip.h"
#include "dc_device.h"
#include "dc_hostutil.h"
#include "dc_sort.h"
#include "dc_tsdf_sparse_math.h"

namespace dc {

// the table size a kernel may trust: n_blocks as the device holds it, kept inside [0, capacity]
__device__ __forceinline__ int64_t tsdf_sparse_blocks(const int64_t* __restrict__ n_blocks, int64_t capacity) {
  const int64_t nb = *n_blocks;
  return nb < 0 ? 0 : (nb > capacity ? capacity : nb);
}

template <typename F>
__device__ __forceinline__ void tsdf_load_ray(const F* __restrict__ vps, const F* __restrict__ dirs, const F* __restrict__ depth, int64_t i,
                                              double* vp, double* dir, double* d) {
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    vp[a] = (double)vps[3 * i + a];
    dir[a] = (double)dirs[3 * i + a];
  }
  *d = (double)depth[i];
}

// a visit that adds: its block's key goes to the ray's share unless the table holds it or the lane's last visit had it
struct TsdfCollect {
  const uint64_t* keys;
  int64_t nb;
  uint64_t* share;                                       // share[j stride]
  int64_t stride;
  int cap;
  int* used;
  TsdfBlockCache* cache;
  __device__ __forceinline__ void operator()(const TsdfSparseAddress::Voxel& x, int64_t) const {
    const uint64_t key = tsdf_voxel_key(x.i);
    if (key == cache->key) return;
    if (tsdf_cached_find(keys, nb, key, cache) >= 0) return;
    if (*used < cap) {                                   // 2K + 1 visits at the most: never refused
      share[(int64_t)*used * stride] = key;
      *used += 1;
    }
  }
};

template <typename F>
__global__ __launch_bounds__(kBlock) void tsdf_sparse_candidates_kernel(const F* __restrict__ vps, const F* __restrict__ dirs,
                                                                        const F* __restrict__ depth, const uint8_t* __restrict__ mask, int64_t n,
                                                                        const double* __restrict__ pose, TsdfGrid g, TsdfRule r, int64_t capacity,
                                                                        const uint64_t* __restrict__ keys, const int64_t* __restrict__ n_blocks,
                                                                        int per_ray, uint64_t* __restrict__ cand) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  double T[16], vp[3], dir[3], d;
  if (pose) {
#pragma unroll
    for (int q = 0; q < 16; ++q) T[q] = pose[q];
  }
  tsdf_load_ray(vps, dirs, depth, i, vp, dir, &d);
  TsdfTally t{0, 0, 0, 0};
  TsdfBlockCache cache{kTsdfNoKey, -1};
  int used = 0;
  tsdf_ray_walk(vp, dir, d, mask ? mask[i] != 0 : true, pose ? T : nullptr, TsdfSparseAddress{g}, r, &t,
                TsdfCollect{keys, tsdf_sparse_blocks(n_blocks, capacity), cand + i, n, per_ray, &used, &cache});
  for (int j = used; j < per_ray; ++j) cand[(int64_t)j * n + i] = kTsdfNoKey;
}

__global__ __launch_bounds__(kBlock) void tsdf_sparse_heads_kernel(const uint64_t* __restrict__ sorted, int64_t n_cand, int32_t* __restrict__ flag) {
  const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (j > n_cand) return;
  int head = 0;
  if (j < n_cand) {
    const uint64_t k = sorted[j];
    head = (k != kTsdfNoKey && (j == 0 || sorted[j - 1] != k)) ? 1 : 0;
  }
  flag[j] = head;
}

// wanted: the new unique keys; admitted: those that fit
__device__ __forceinline__ void tsdf_sparse_admission(const int32_t* __restrict__ off, int64_t n_cand, int64_t nb, int64_t capacity, int64_t* wanted,
                                                      int64_t* admitted) {
  const int64_t u = off ? (int64_t)(uint32_t)off[n_cand] : 0, room = capacity - nb;
  *wanted = u;
  *admitted = u < room ? u : room;
}

__global__ __launch_bounds__(kBlock) void tsdf_sparse_compact_kernel(const uint64_t* __restrict__ sorted, const int32_t* __restrict__ flag,
                                                                     const int32_t* __restrict__ off, int64_t n_cand, int64_t capacity,
                                                                     const int64_t* __restrict__ n_blocks, uint64_t* __restrict__ newk) {
  const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (j >= n_cand || flag[j] == 0) return;
  int64_t wanted, admitted;
  tsdf_sparse_admission(off, n_cand, tsdf_sparse_blocks(n_blocks, capacity), capacity, &wanted, &admitted);
  const int64_t rank = (int64_t)(uint32_t)off[j];
  if (rank < admitted) newk[rank] = sorted[j];
}

__global__ __launch_bounds__(kBlock) void tsdf_sparse_merge_kernel(const uint64_t* __restrict__ keys, const int32_t* __restrict__ slots,
                                                                   const int64_t* __restrict__ n_blocks, int64_t capacity,
                                                                   const int32_t* __restrict__ off, int64_t n_cand, const uint64_t* __restrict__ newk,
                                                                   uint64_t* __restrict__ tkeys, int32_t* __restrict__ tslots) {
  const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (t >= capacity) return;
  const int64_t nb = tsdf_sparse_blocks(n_blocks, capacity);
  int64_t wanted, admitted;
  tsdf_sparse_admission(off, n_cand, nb, capacity, &wanted, &admitted);
  if (t < nb) {
    const uint64_t k = keys[t];
    const int64_t dst = t + tsdf_table_lower(newk, admitted, k);
    tkeys[dst] = k;
    tslots[dst] = slots[t];
  }
  if (t < admitted) {
    const uint64_t k = newk[t];
    const int64_t dst = t + tsdf_table_lower(keys, nb, k);
    tkeys[dst] = k;
    tslots[dst] = (int32_t)(nb + t);
  }
}

__global__ __launch_bounds__(kBlock) void tsdf_sparse_copy_kernel(uint64_t* __restrict__ keys, int32_t* __restrict__ slots,
                                                                  const int64_t* __restrict__ n_blocks, int64_t capacity,
                                                                  const int32_t* __restrict__ off, int64_t n_cand, const uint64_t* __restrict__ tkeys,
                                                                  const int32_t* __restrict__ tslots) {
  const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (t >= capacity) return;
  const int64_t nb = tsdf_sparse_blocks(n_blocks, capacity);
  int64_t wanted, admitted;
  tsdf_sparse_admission(off, n_cand, nb, capacity, &wanted, &admitted);
  if (t < nb + admitted) {
    keys[t] = tkeys[t];
    slots[t] = tslots[t];
  }
}

__global__ void tsdf_sparse_finish_kernel(int64_t* __restrict__ n_blocks, int64_t capacity, const int32_t* __restrict__ off, int64_t n_cand,
                                          int64_t* __restrict__ info) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const int64_t nb = tsdf_sparse_blocks(n_blocks, capacity);
  int64_t wanted, admitted;
  tsdf_sparse_admission(off, n_cand, nb, capacity, &wanted, &admitted);
  *n_blocks = nb + admitted;
  info[0] = nb + admitted;
  info[1] = wanted - admitted;
}

// a visit that adds: the two integer atomics at slot 512 + local, or one more dropped visit
struct TsdfSparseAtomicAdd {
  const uint64_t* keys;
  const int32_t* slots;
  int64_t nb, capacity;
  int64_t* sum;
  int32_t* count;
  TsdfBlockCache* cache;
  long long* dropped;
  __device__ __forceinline__ void operator()(const TsdfSparseAddress::Voxel& x, int64_t q) const {
    const int64_t pos = tsdf_cached_find(keys, nb, tsdf_voxel_key(x.i), cache);
    const int64_t slot = pos < 0 ? -1 : (int64_t)slots[pos];
    if (slot < 0 || slot >= capacity) {
      *dropped += 1;
      return;
    }
    const int64_t v = slot * kTsdfBlockVoxels + tsdf_voxel_local(x.i);
    atomicAdd(reinterpret_cast<unsigned long long*>(sum + v), (unsigned long long)q);
    atomicAdd(count + v, 1);
  }
};

template <typename F>
__global__ __launch_bounds__(kBlock) void tsdf_sparse_integrate_kernel(const F* __restrict__ vps, const F* __restrict__ dirs,
                                                                       const F* __restrict__ depth, const uint8_t* __restrict__ mask, int64_t n,
                                                                       const double* __restrict__ pose, TsdfGrid g, TsdfRule r, int64_t capacity,
                                                                       const uint64_t* __restrict__ keys, const int32_t* __restrict__ slots,
                                                                       const int64_t* __restrict__ n_blocks, int64_t* __restrict__ sum,
                                                                       int32_t* __restrict__ count, int64_t* __restrict__ stats) {
  __shared__ long long s_tally[kWavesPerBlock][5];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
  const int64_t i = (int64_t)blockIdx.x * kBlock + tid;
  TsdfTally t{0, 0, 0, 0};
  long long dropped = 0;
  if (i < n) {
    double T[16], vp[3], dir[3], d;
    if (pose) {
#pragma unroll
      for (int q = 0; q < 16; ++q) T[q] = pose[q];
    }
    tsdf_load_ray(vps, dirs, depth, i, vp, dir, &d);
    TsdfBlockCache cache{kTsdfNoKey, -1};
    tsdf_ray_walk(vp, dir, d, mask ? mask[i] != 0 : true, pose ? T : nullptr, TsdfSparseAddress{g}, r, &t,
                  TsdfSparseAtomicAdd{keys, slots, tsdf_sparse_blocks(n_blocks, capacity), capacity, sum, count, &cache, &dropped});
  }
  long long v[5] = {t.used, t.skipped, t.outside, t.visits, dropped};
#pragma unroll
  for (int q = 0; q < 5; ++q) {
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) v[q] += __shfl_down(v[q], off, kWave);
    if (lane == 0) s_tally[wave][q] = v[q];
  }
  __syncthreads();
  if (tid < 5) {
    long long s = 0;
#pragma unroll
    for (int w = 0; w < kWavesPerBlock; ++w) s += s_tally[w][tid];
    if (s != 0) atomicAdd(reinterpret_cast<unsigned long long*>(stats + tid), (unsigned long long)s);
  }
}

// ---- extraction ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void tsdf_sparse_neighbours_kernel(const uint64_t* __restrict__ keys, int64_t nb, int32_t* __restrict__ nbr) {
  const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (t >= nb * 27) return;
  const int64_t p = t / 27;
  nbr[t] = tsdf_block_neighbour(keys, nb, p, (int)(t - p * 27));
}

__device__ __forceinline__ void tsdf_sparse_decode(int64_t v, int64_t* pos, int* lx, int* ly, int* lz) {
  *pos = v >> 9;
  const int local = (int)(v & 511);
  *lx = local >> 6;
  *ly = (local >> 3) & 7;
  *lz = local & 7;
}

__global__ __launch_bounds__(kBlock) void tsdf_sparse_cells_kernel(const int64_t* __restrict__ sum, const int32_t* __restrict__ count,
                                                                   const int32_t* __restrict__ nbr, const int32_t* __restrict__ slots, int min_count,
                                                                   int64_t n_vox, int32_t* __restrict__ flag) {
  const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (v > n_vox) return;
  int active = 0;
  if (v < n_vox) {
    int64_t pos, corner[8];
    int lx, ly, lz, bits;
    tsdf_sparse_decode(v, &pos, &lx, &ly, &lz);
    active = tsdf_sparse_cell_active(sum, count, nbr + 27 * pos, slots, min_count, lx, ly, lz, corner, &bits) ? 1 : 0;
  }
  flag[v] = active;
}

// the one decision both passes share: does the edge q -> q + e emit its quad, around which cells, and is q inside
template <int E>
__device__ __forceinline__ bool tsdf_sparse_edge_emits(const int64_t* __restrict__ sum, const int32_t* __restrict__ count,
                                                       const int32_t* __restrict__ nbr27, const int32_t* __restrict__ slots, int min_count,
                                                       const int32_t* __restrict__ flag, int lx, int ly, int lz, int64_t* cells, bool* q_inside) {
  if (!tsdf_sparse_edge_crosses(sum, count, nbr27, slots, min_count, lx, ly, lz, E, q_inside)) return false;
  if (!tsdf_sparse_edge_cells(nbr27, lx, ly, lz, E, cells)) return false;
  return flag[cells[0]] != 0 && flag[cells[1]] != 0 && flag[cells[2]] != 0 && flag[cells[3]] != 0;
}

__global__ __launch_bounds__(kBlock) void tsdf_sparse_edges_kernel(const int64_t* __restrict__ sum, const int32_t* __restrict__ count,
                                                                   const int32_t* __restrict__ nbr, const int32_t* __restrict__ slots, int min_count,
                                                                   int64_t n_vox, const int32_t* __restrict__ flag, int32_t* __restrict__ cnt) {
  const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (v > n_vox) return;
  int c = 0;
  if (v < n_vox) {
    int64_t pos, cells[4];
    int lx, ly, lz;
    bool in;
    tsdf_sparse_decode(v, &pos, &lx, &ly, &lz);
    const int32_t* nb27 = nbr + 27 * pos;
    c += tsdf_sparse_edge_emits<0>(sum, count, nb27, slots, min_count, flag, lx, ly, lz, cells, &in) ? 1 : 0;
    c += tsdf_sparse_edge_emits<1>(sum, count, nb27, slots, min_count, flag, lx, ly, lz, cells, &in) ? 1 : 0;
    c += tsdf_sparse_edge_emits<2>(sum, count, nb27, slots, min_count, flag, lx, ly, lz, cells, &in) ? 1 : 0;
  }
  cnt[v] = c;
}

__global__ void tsdf_sparse_totals_kernel(const int32_t* __restrict__ cell_off, const int32_t* __restrict__ edge_off, int64_t n_vox,
                                          int64_t* __restrict__ totals) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    totals[0] = (int64_t)(uint32_t)cell_off[n_vox];
    totals[1] = 2 * (int64_t)(uint32_t)edge_off[n_vox];
  }
}

template <int E>
__device__ __forceinline__ void tsdf_sparse_emit(const int64_t* __restrict__ sum, const int32_t* __restrict__ count, const int32_t* __restrict__ nbr27,
                                                 const int32_t* __restrict__ slots, int min_count, const int32_t* __restrict__ flag,
                                                 const int32_t* __restrict__ cell_off, int lx, int ly, int lz, int64_t* quad, int64_t n_faces,
                                                 int32_t* __restrict__ faces) {
  int64_t cells[4];
  bool in;
  if (!tsdf_sparse_edge_emits<E>(sum, count, nbr27, slots, min_count, flag, lx, ly, lz, cells, &in)) return;
  const int64_t f = 2 * *quad;
  *quad += 1;
  if (f + 1 >= n_faces) return;                       // offsets that are not this volume's scan write nothing out of bounds
  const int32_t a = cell_off[cells[in ? 0 : 3]], b = cell_off[cells[in ? 1 : 2]], c = cell_off[cells[in ? 2 : 1]],
                d = cell_off[cells[in ? 3 : 0]];
  int32_t* o = faces + 3 * f;
  o[0] = a; o[1] = b; o[2] = c;
  o[3] = a; o[4] = c; o[5] = d;
}

__global__ __launch_bounds__(kBlock) void tsdf_sparse_fill_kernel(const uint64_t* __restrict__ keys, const int64_t* __restrict__ sum,
                                                                  const int32_t* __restrict__ count, const int32_t* __restrict__ nbr,
                                                                  const int32_t* __restrict__ slots, TsdfGrid g, int min_count, int64_t n_vox,
                                                                  const int32_t* __restrict__ flag, const int32_t* __restrict__ cell_off,
                                                                  const int32_t* __restrict__ edge_off, int64_t n_vertices, int64_t n_faces,
                                                                  double* __restrict__ vertices, int32_t* __restrict__ faces) {
  const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (v >= n_vox) return;
  int64_t pos;
  int lx, ly, lz;
  tsdf_sparse_decode(v, &pos, &lx, &ly, &lz);
  const int32_t* nb27 = nbr + 27 * pos;
  if (flag[v] != 0) {
    int bits;
    int64_t corner[8];
    const int64_t at = (int64_t)(uint32_t)cell_off[v];
    if (tsdf_sparse_cell_active(sum, count, nb27, slots, min_count, lx, ly, lz, corner, &bits) && at < n_vertices) {
      int b[3];
      double p[3];
      tsdf_block_of_key(keys[pos], b);
      tsdf_cell_vertex(sum, count, g, 8 * b[0] + lx, 8 * b[1] + ly, 8 * b[2] + lz, corner, bits, p);
      vertices[3 * at] = p[0]; vertices[3 * at + 1] = p[1]; vertices[3 * at + 2] = p[2];
    }
  }
  int64_t quad = (int64_t)(uint32_t)edge_off[v];
  tsdf_sparse_emit<0>(sum, count, nb27, slots, min_count, flag, cell_off, lx, ly, lz, &quad, n_faces, faces);
  tsdf_sparse_emit<1>(sum, count, nb27, slots, min_count, flag, cell_off, lx, ly, lz, &quad, n_faces, faces);
  tsdf_sparse_emit<2>(sum, count, nb27, slots, min_count, flag, cell_off, lx, ly, lz, &quad, n_faces, faces);
}

// ---- workspaces ------------------------------------------------------------------------------------------------------------------
struct TsdfSparseAllocWs {
  uint64_t *cand, *sorted, *newk, *tkeys;
  int32_t *flag, *off, *tslots;
  void *sort_ws, *scan_ws;
  size_t sort_ws_bytes, scan_ws_bytes, bytes;
};

static TsdfSparseAllocWs tsdf_sparse_alloc_carve(void* ws, int64_t n, int k_steps, int64_t capacity) {
  const size_t n_cand = (size_t)n * (size_t)tsdf_sparse_ray_blocks(k_steps), cap = (size_t)capacity;
  TsdfSparseAllocWs w;
  Carver c(ws);
  w.cand = c.take<uint64_t>(n_cand);
  w.sorted = c.take<uint64_t>(n_cand);
  w.flag = c.take<int32_t>(n_cand + 1);
  w.off = c.take<int32_t>(n_cand + 1);
  w.newk = c.take<uint64_t>(cap);
  w.tkeys = c.take<uint64_t>(cap);
  w.tslots = c.take<int32_t>(cap);
  w.sort_ws_bytes = sort_keys_bytes(n_cand);
  w.sort_ws = c.take<char>(w.sort_ws_bytes);
  w.scan_ws_bytes = scan_bytes(n_cand + 1);
  w.scan_ws = c.take<char>(w.scan_ws_bytes);
  w.bytes = c.off + 256;
  return w;
}

// the candidates' 32-bit scan and the 32-bit slots
static bool tsdf_sparse_alloc_size_ok(int64_t n, int k_steps, int64_t capacity) {
  return n >= 0 && k_steps >= 1 && k_steps <= (1 << 20) && capacity >= 1 && capacity < ((int64_t)1 << 22) &&
         n <= (((int64_t)1 << 31) - 2) / tsdf_sparse_ray_blocks(k_steps);
}

struct TsdfSparseExtractWs {
  int32_t *nbr, *flag, *cell_off, *edge_cnt, *edge_off;
  void* scan_ws;
  size_t scan_ws_bytes, bytes;
};

static TsdfSparseExtractWs tsdf_sparse_extract_carve(void* ws, int64_t nb) {
  const size_t n_vox = (size_t)nb * kTsdfBlockVoxels;
  TsdfSparseExtractWs w;
  Carver c(ws);
  w.nbr = c.take<int32_t>((size_t)nb * 27);
  w.flag = c.take<int32_t>(n_vox + 1);
  w.cell_off = c.take<int32_t>(n_vox + 1);
  w.edge_cnt = c.take<int32_t>(n_vox + 1);
  w.edge_off = c.take<int32_t>(n_vox + 1);
  w.scan_ws_bytes = scan_bytes(n_vox + 1);
  w.scan_ws = c.take<char>(w.scan_ws_bytes);
  w.bytes = c.off + 256;
  return w;
}

// 3 emitting edges per voxel must fit the 32-bit scan
static bool tsdf_sparse_extract_size_ok(int64_t nb) { return nb >= 0 && nb * kTsdfBlockVoxels * 3 < ((int64_t)1 << 31); }

static bool tsdf_sparse_rule(double ox, double oy, double oz, double voxel, double trunc, int k_steps, double min_depth, double max_range,
                             TsdfGrid* g, TsdfRule* r) {
  *g = TsdfGrid{{ox, oy, oz}, voxel, {0, 0, 0}};
  *r = TsdfRule{trunc, voxel / 2.0, min_depth, max_range, -1.0, k_steps};
  return tsdf_lattice_ok(*g) && tsdf_rule_ok(*r);
}

static unsigned tsdf_grid_of(int64_t items) { return (unsigned)((items + kBlock - 1) / kBlock); }

}  // namespace dc

using namespace dc;

extern "C" {

size_t dc_tsdf_sparse_workspace_bytes(int64_t n_rays, int k_steps, int64_t capacity) {
  if (!tsdf_sparse_alloc_size_ok(n_rays, k_steps, capacity)) return 0;
  return tsdf_sparse_alloc_carve(nullptr, n_rays, k_steps, capacity).bytes;
}

int dc_tsdf_sparse_allocate(const void* vps, const void* dirs, const void* depth, int dtype, int64_t n, const uint8_t* mask, const double* pose,
                            double ox, double oy, double oz, double voxel, double trunc, int k_steps, double min_depth, double max_range,
                            int64_t capacity, uint64_t* keys, int32_t* slots, int64_t* n_blocks, int64_t* info, void* ws, size_t ws_bytes,
                            hipStream_t stream) {
  TsdfGrid g;
  TsdfRule r;
  if (!tsdf_sparse_rule(ox, oy, oz, voxel, trunc, k_steps, min_depth, max_range, &g, &r) || n < 0 || capacity < 1) return DC_ERR_ARG;
  if (dtype != DC_F32 && dtype != DC_F64) return DC_ERR_DTYPE;
  if (!keys || !slots || !n_blocks || !info) return DC_ERR_ARG;
  if (!tsdf_sparse_alloc_size_ok(n, k_steps, capacity)) return DC_ERR_UNSUPPORTED;
  if (n == 0) {
    hipLaunchKernelGGL(tsdf_sparse_finish_kernel, dim3(1), dim3(kWave), 0, stream, n_blocks, capacity, (const int32_t*)nullptr, (int64_t)0, info);
    DC_HIP(hipGetLastError());
    return DC_OK;
  }
  if (!vps || !dirs || !depth || !ws) return DC_ERR_ARG;
  if (ws_bytes < dc_tsdf_sparse_workspace_bytes(n, k_steps, capacity)) return DC_ERR_WORKSPACE;
  const TsdfSparseAllocWs w = tsdf_sparse_alloc_carve(ws, n, k_steps, capacity);
  const int per_ray = tsdf_sparse_ray_blocks(k_steps);
  const int64_t n_cand = n * per_ray;
  if (dtype == DC_F32)
    hipLaunchKernelGGL(tsdf_sparse_candidates_kernel<float>, dim3(tsdf_grid_of(n)), dim3(kBlock), 0, stream, (const float*)vps, (const float*)dirs,
                       (const float*)depth, mask, n, pose, g, r, capacity, (const uint64_t*)keys, (const int64_t*)n_blocks, per_ray, w.cand);
  else
    hipLaunchKernelGGL(tsdf_sparse_candidates_kernel<double>, dim3(tsdf_grid_of(n)), dim3(kBlock), 0, stream, (const double*)vps,
                       (const double*)dirs, (const double*)depth, mask, n, pose, g, r, capacity, (const uint64_t*)keys, (const int64_t*)n_blocks,
                       per_ray, w.cand);
  DC_HIP(sort_keys_u64(w.sort_ws, w.sort_ws_bytes, w.cand, w.sorted, (size_t)n_cand, 0, 64, stream));
  hipLaunchKernelGGL(tsdf_sparse_heads_kernel, dim3(tsdf_grid_of(n_cand + 1)), dim3(kBlock), 0, stream, (const uint64_t*)w.sorted, n_cand, w.flag);
  DC_HIP(exclusive_scan_32(w.scan_ws, w.scan_ws_bytes, w.flag, w.off, (size_t)n_cand + 1, stream));
  hipLaunchKernelGGL(tsdf_sparse_compact_kernel, dim3(tsdf_grid_of(n_cand)), dim3(kBlock), 0, stream, (const uint64_t*)w.sorted,
                     (const int32_t*)w.flag, (const int32_t*)w.off, n_cand, capacity, (const int64_t*)n_blocks, w.newk);
  hipLaunchKernelGGL(tsdf_sparse_merge_kernel, dim3(tsdf_grid_of(capacity)), dim3(kBlock), 0, stream, (const uint64_t*)keys, (const int32_t*)slots,
                     (const int64_t*)n_blocks, capacity, (const int32_t*)w.off, n_cand, (const uint64_t*)w.newk, w.tkeys, w.tslots);
  hipLaunchKernelGGL(tsdf_sparse_copy_kernel, dim3(tsdf_grid_of(capacity)), dim3(kBlock), 0, stream, keys, slots, (const int64_t*)n_blocks, capacity,
                     (const int32_t*)w.off, n_cand, (const uint64_t*)w.tkeys, (const int32_t*)w.tslots);
  hipLaunchKernelGGL(tsdf_sparse_finish_kernel, dim3(1), dim3(kWave), 0, stream, n_blocks, capacity, (const int32_t*)w.off, n_cand, info);
  DC_HIP(hipGetLastError());
  return DC_OK;
}

int dc_tsdf_sparse_integrate(const void* vps, const void* dirs, const void* depth, int dtype, int64_t n, const uint8_t* mask, const double* pose,
                             double ox, double oy, double oz, double voxel, double trunc, int k_steps, double min_depth, double max_range,
                             int64_t capacity, const uint64_t* keys, const int32_t* slots, const int64_t* n_blocks, int64_t* sum, int32_t* count,
                             int64_t* stats, hipStream_t stream) {
  TsdfGrid g;
  TsdfRule r;
  if (!tsdf_sparse_rule(ox, oy, oz, voxel, trunc, k_steps, min_depth, max_range, &g, &r) || n < 0 || capacity < 1 ||
      capacity >= ((int64_t)1 << 22))
    return DC_ERR_ARG;
  if (dtype != DC_F32 && dtype != DC_F64) return DC_ERR_DTYPE;
  if (n == 0) return DC_OK;
  if (!vps || !dirs || !depth || !keys || !slots || !n_blocks || !sum || !count || !stats) return DC_ERR_ARG;
  const int64_t blocks = (n + kBlock - 1) / kBlock;
  if (blocks > 0x7fffffff) return DC_ERR_UNSUPPORTED;
  if (dtype == DC_F32)
    hipLaunchKernelGGL(tsdf_sparse_integrate_kernel<float>, dim3((unsigned)blocks), dim3(kBlock), 0, stream, (const float*)vps, (const float*)dirs,
                       (const float*)depth, mask, n, pose, g, r, capacity, keys, slots, n_blocks, sum, count, stats);
  else
    hipLaunchKernelGGL(tsdf_sparse_integrate_kernel<double>, dim3((unsigned)blocks), dim3(kBlock), 0, stream, (const double*)vps,
                       (const double*)dirs, (const double*)depth, mask, n, pose, g, r, capacity, keys, slots, n_blocks, sum, count, stats);
  DC_HIP(hipGetLastError());
  return DC_OK;
}

size_t dc_tsdf_sparse_extract_workspace_bytes(int64_t n_blocks) {
  if (!tsdf_sparse_extract_size_ok(n_blocks)) return 0;
  return tsdf_sparse_extract_carve(nullptr, n_blocks).bytes;
}

int dc_tsdf_sparse_extract_count(const uint64_t* keys, const int32_t* slots, int64_t n_blocks, const int64_t* sum, const int32_t* count,
                                 int min_count, int64_t* totals, void* ws, size_t ws_bytes, hipStream_t stream) {
  if (n_blocks < 0 || min_count < 1 || !keys || !slots || !sum || !count || !totals || !ws) return DC_ERR_ARG;
  if (!tsdf_sparse_extract_size_ok(n_blocks)) return DC_ERR_UNSUPPORTED;
  if (ws_bytes < dc_tsdf_sparse_extract_workspace_bytes(n_blocks)) return DC_ERR_WORKSPACE;
  const TsdfSparseExtractWs w = tsdf_sparse_extract_carve(ws, n_blocks);
  const int64_t n_vox = n_blocks * kTsdfBlockVoxels;
  if (n_blocks > 0)
    hipLaunchKernelGGL(tsdf_sparse_neighbours_kernel, dim3(tsdf_grid_of(n_blocks * 27)), dim3(kBlock), 0, stream, keys, n_blocks, w.nbr);
  hipLaunchKernelGGL(tsdf_sparse_cells_kernel, dim3(tsdf_grid_of(n_vox + 1)), dim3(kBlock), 0, stream, sum, count, (const int32_t*)w.nbr, slots,
                     min_count, n_vox, w.flag);
  hipLaunchKernelGGL(tsdf_sparse_edges_kernel, dim3(tsdf_grid_of(n_vox + 1)), dim3(kBlock), 0, stream, sum, count, (const int32_t*)w.nbr, slots,
                     min_count, n_vox, (const int32_t*)w.flag, w.edge_cnt);
  DC_HIP(exclusive_scan_32(w.scan_ws, w.scan_ws_bytes, w.flag, w.cell_off, (size_t)n_vox + 1, stream));
  DC_HIP(exclusive_scan_32(w.scan_ws, w.scan_ws_bytes, w.edge_cnt, w.edge_off, (size_t)n_vox + 1, stream));
  hipLaunchKernelGGL(tsdf_sparse_totals_kernel, dim3(1), dim3(kWave), 0, stream, (const int32_t*)w.cell_off, (const int32_t*)w.edge_off, n_vox,
                     totals);
  DC_HIP(hipGetLastError());
  return DC_OK;
}

int dc_tsdf_sparse_extract_fill(const uint64_t* keys, const int32_t* slots, int64_t n_blocks, const int64_t* sum, const int32_t* count, double ox,
                                double oy, double oz, double voxel, int min_count, const void* ws, size_t ws_bytes, int64_t n_vertices,
                                int64_t n_faces, double* vertices, int32_t* faces, hipStream_t stream) {
  const TsdfGrid g{{ox, oy, oz}, voxel, {0, 0, 0}};
  if (!tsdf_lattice_ok(g) || n_blocks < 0 || min_count < 1 || !keys || !slots || !sum || !count || !ws || n_vertices < 0 || n_faces < 0)
    return DC_ERR_ARG;
  if (!tsdf_sparse_extract_size_ok(n_blocks)) return DC_ERR_UNSUPPORTED;
  if (ws_bytes < dc_tsdf_sparse_extract_workspace_bytes(n_blocks)) return DC_ERR_WORKSPACE;
  if (n_blocks == 0 || (n_vertices == 0 && n_faces == 0)) return DC_OK;
  if ((n_vertices > 0 && !vertices) || (n_faces > 0 && !faces)) return DC_ERR_ARG;
  const TsdfSparseExtractWs w = tsdf_sparse_extract_carve(const_cast<void*>(ws), n_blocks);
  const int64_t n_vox = n_blocks * kTsdfBlockVoxels;
  hipLaunchKernelGGL(tsdf_sparse_fill_kernel, dim3(tsdf_grid_of(n_vox)), dim3(kBlock), 0, stream, keys, sum, count, (const int32_t*)w.nbr, slots, g,
                     min_count, n_vox, (const int32_t*)w.flag, (const int32_t*)w.cell_off, (const int32_t*)w.edge_off, n_vertices, n_faces,
                     vertices, faces);
  DC_HIP(hipGetLastError());
  return DC_OK;
}

}  // extern "C"
