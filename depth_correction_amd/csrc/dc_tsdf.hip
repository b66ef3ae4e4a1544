// Surface reconstruction: TSDF fusion of posed scans and surface-nets extraction (DESIGN "Surface reconstruction"; the rules:
// dc_tsdf_math.h, whose functions the kernels inline).
//
//   dc_tsdf_integrate   one lane per ray, the sample loop in the lane.  A visit is two vector integer atomics, a 64-bit add on sum and a
//                       32-bit add on count; integer adds commute, so the volume holds the same bits whatever the schedule and the ray
//                       order.  The four stats are summed per wavefront (shuffles), per block (LDS) and reach memory as one atomic per
//                       stat and block.  The rays of an organised scan are neighbours in memory, so a wavefront's adds of one step land
//                       in neighbouring voxels.
//   dc_tsdf_extract_count / _fill   count, scan, fill:
//                         cells   flag [C + 1] <- the active cells (the last slot 0, so that the scan ends in the total);
//                         edges   cnt [V + 1]  <- the emitting edges (0 .. 3) of every lattice point, from the flags;
//                         the library's exclusive scans of both; totals <- {vertices, faces};
//                         fill    one lane per lattice point writes its cell's vertex at the cell's offset and its edges' faces at the
//                                 point's offset: ascending cell index, ascending (point, axis) whatever the schedule.
//                       The emitting edges are decided by ONE function in both passes.
// Nothing here allocates, copies or synchronises; no floating-point atomic anywhere.
#include "dc_common.h"
#include "../../include/dc_hip.h"
#include "dc_device.h"
#include "dc_hostutil.h"
#include "dc_sort.h"
#include "dc_tsdf_math.h"

namespace dc {

struct TsdfAtomicAdd {
  int64_t* sum;
  int32_t* count;
  __device__ __forceinline__ void operator()(int64_t v, int64_t q) const {
    atomicAdd(reinterpret_cast<unsigned long long*>(sum + v), (unsigned long long)q);
    atomicAdd(count + v, 1);
  }
};

template <typename F>
__global__ __launch_bounds__(kBlock) void tsdf_integrate_kernel(const F* __restrict__ vps, const F* __restrict__ dirs,
                                                                const F* __restrict__ depth, const uint8_t* __restrict__ mask, int64_t n,
                                                                const double* __restrict__ pose, TsdfGrid g, TsdfRule r,
                                                                int64_t* __restrict__ sum, int32_t* __restrict__ count,
                                                                int64_t* __restrict__ stats) {
  __shared__ long long s_tally[kWavesPerBlock][4];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
  const int64_t i = (int64_t)blockIdx.x * kBlock + tid;
  TsdfTally t{0, 0, 0, 0};
  if (i < n) {
    double T[16];
    if (pose) {
#pragma unroll
      for (int q = 0; q < 16; ++q) T[q] = pose[q];
    }
    const double vp[3] = {(double)vps[3 * i], (double)vps[3 * i + 1], (double)vps[3 * i + 2]};
    const double dir[3] = {(double)dirs[3 * i], (double)dirs[3 * i + 1], (double)dirs[3 * i + 2]};
    tsdf_ray(vp, dir, (double)depth[i], mask ? mask[i] != 0 : true, pose ? T : nullptr, g, r, &t, TsdfAtomicAdd{sum, count});
  }
  long long v[4] = {t.used, t.skipped, t.outside, t.visits};
#pragma unroll
  for (int q = 0; q < 4; ++q) {
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) v[q] += __shfl_down(v[q], off, kWave);
    if (lane == 0) s_tally[wave][q] = v[q];
  }
  __syncthreads();
  if (tid < 4) {
    long long s = 0;
#pragma unroll
    for (int w = 0; w < kWavesPerBlock; ++w) s += s_tally[w][tid];
    if (s != 0) atomicAdd(reinterpret_cast<unsigned long long*>(stats + tid), (unsigned long long)s);
  }
}

// (x, y, z) of the linear index v of a grid with the dims (n1, n2) behind the first
__device__ __forceinline__ void tsdf_decode(int64_t v, int n1, int n2, int* x, int* y, int* z) {
  const uint32_t u = (uint32_t)v, p = (uint32_t)n1 * (uint32_t)n2;      // v < 2^31 and n1 n2 < 2^31
  *x = (int)(u / p);
  const uint32_t rem = u - (uint32_t)*x * p;
  *y = (int)(rem / (uint32_t)n2);
  *z = (int)(rem - (uint32_t)*y * (uint32_t)n2);
}

__global__ __launch_bounds__(kBlock) void tsdf_cells_kernel(const int64_t* __restrict__ sum, const int32_t* __restrict__ count, TsdfGrid g,
                                                            int min_count, int64_t n_cells, int32_t* __restrict__ flag) {
  const int64_t ci = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (ci > n_cells) return;
  int active = 0;
  if (ci < n_cells) {
    int x, y, z, bits;
    int64_t corner[8];
    tsdf_decode(ci, g.n[1] - 1, g.n[2] - 1, &x, &y, &z);
    active = tsdf_cell_active(sum, count, g, min_count, x, y, z, corner, &bits) ? 1 : 0;
  }
  flag[ci] = active;
}

// the one decision both passes share: does the edge q -> q + e emit its quad, around which cells, and is q inside
template <int E>
__device__ __forceinline__ bool tsdf_edge_emits(const int64_t* __restrict__ sum, const int32_t* __restrict__ count, const TsdfGrid& g,
                                                int min_count, const int32_t* __restrict__ flag, int x, int y, int z, int64_t* cells,
                                                bool* q_inside) {
  if (!tsdf_edge_crosses(sum, count, g, min_count, x, y, z, E, q_inside)) return false;
  if (!tsdf_edge_cells(g, x, y, z, E, cells)) return false;
  return flag[cells[0]] != 0 && flag[cells[1]] != 0 && flag[cells[2]] != 0 && flag[cells[3]] != 0;
}

__global__ __launch_bounds__(kBlock) void tsdf_edges_kernel(const int64_t* __restrict__ sum, const int32_t* __restrict__ count, TsdfGrid g,
                                                            int min_count, int64_t n_vox, const int32_t* __restrict__ flag,
                                                            int32_t* __restrict__ cnt) {
  const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (v > n_vox) return;
  int c = 0;
  if (v < n_vox) {
    int x, y, z;
    int64_t cells[4];
    bool in;
    tsdf_decode(v, g.n[1], g.n[2], &x, &y, &z);
    c += tsdf_edge_emits<0>(sum, count, g, min_count, flag, x, y, z, cells, &in) ? 1 : 0;
    c += tsdf_edge_emits<1>(sum, count, g, min_count, flag, x, y, z, cells, &in) ? 1 : 0;
    c += tsdf_edge_emits<2>(sum, count, g, min_count, flag, x, y, z, cells, &in) ? 1 : 0;
  }
  cnt[v] = c;
}

__global__ void tsdf_totals_kernel(const int32_t* __restrict__ cell_off, int64_t n_cells, const int32_t* __restrict__ edge_off, int64_t n_vox,
                                   int64_t* __restrict__ totals) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    totals[0] = (int64_t)(uint32_t)cell_off[n_cells];
    totals[1] = 2 * (int64_t)(uint32_t)edge_off[n_vox];
  }
}

template <int E>
__device__ __forceinline__ void tsdf_emit(const int64_t* __restrict__ sum, const int32_t* __restrict__ count, const TsdfGrid& g, int min_count,
                                          const int32_t* __restrict__ flag, const int32_t* __restrict__ cell_off, int x, int y, int z,
                                          int64_t* quad, int64_t n_faces, int32_t* __restrict__ faces) {
  int64_t cells[4];
  bool in;
  if (!tsdf_edge_emits<E>(sum, count, g, min_count, flag, x, y, z, cells, &in)) return;
  const int64_t f = 2 * *quad;
  *quad += 1;
  if (f + 1 >= n_faces) return;                       // offsets that are not this volume's scan write nothing out of bounds
  const int32_t a = cell_off[cells[in ? 0 : 3]], b = cell_off[cells[in ? 1 : 2]], c = cell_off[cells[in ? 2 : 1]],
                d = cell_off[cells[in ? 3 : 0]];
  int32_t* o = faces + 3 * f;
  o[0] = a; o[1] = b; o[2] = c;
  o[3] = a; o[4] = c; o[5] = d;
}

__global__ __launch_bounds__(kBlock) void tsdf_fill_kernel(const int64_t* __restrict__ sum, const int32_t* __restrict__ count, TsdfGrid g,
                                                           int min_count, int64_t n_vox, const int32_t* __restrict__ flag,
                                                           const int32_t* __restrict__ cell_off, const int32_t* __restrict__ edge_off,
                                                           int64_t n_vertices, int64_t n_faces, double* __restrict__ vertices,
                                                           int32_t* __restrict__ faces) {
  const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (v >= n_vox) return;
  int x, y, z;
  tsdf_decode(v, g.n[1], g.n[2], &x, &y, &z);
  if (tsdf_cell_exists(g, x, y, z)) {
    const int64_t ci = tsdf_cell_index(g, x, y, z);
    if (flag[ci] != 0) {
      int bits;
      int64_t corner[8];
      const int64_t pos = (int64_t)(uint32_t)cell_off[ci];
      if (tsdf_cell_active(sum, count, g, min_count, x, y, z, corner, &bits) && pos < n_vertices) {
        double p[3];
        tsdf_cell_vertex(sum, count, g, x, y, z, corner, bits, p);
        vertices[3 * pos] = p[0]; vertices[3 * pos + 1] = p[1]; vertices[3 * pos + 2] = p[2];
      }
    }
  }
  int64_t quad = (int64_t)(uint32_t)edge_off[v];
  tsdf_emit<0>(sum, count, g, min_count, flag, cell_off, x, y, z, &quad, n_faces, faces);
  tsdf_emit<1>(sum, count, g, min_count, flag, cell_off, x, y, z, &quad, n_faces, faces);
  tsdf_emit<2>(sum, count, g, min_count, flag, cell_off, x, y, z, &quad, n_faces, faces);
}

struct TsdfWorkspace {
  int32_t *flag, *cell_off, *edge_cnt, *edge_off;
  void* scan_ws;
  size_t scan_ws_bytes, bytes;
};

static TsdfWorkspace tsdf_carve(void* ws, int nx, int ny, int nz) {
  const size_t n_cells = (size_t)tsdf_cell_count(nx, ny, nz), n_vox = (size_t)nx * ny * nz;
  TsdfWorkspace w;
  Carver c(ws);
  w.flag = c.take<int32_t>(n_cells + 1);
  w.cell_off = c.take<int32_t>(n_cells + 1);
  w.edge_cnt = c.take<int32_t>(n_vox + 1);
  w.edge_off = c.take<int32_t>(n_vox + 1);
  const size_t sv = scan_bytes(n_vox + 1), sc = scan_bytes(n_cells + 1);
  w.scan_ws_bytes = sv > sc ? sv : sc;
  w.scan_ws = c.take<char>(w.scan_ws_bytes);
  w.bytes = c.off + 256;
  return w;
}

// 3 V emitting edges must fit the 32-bit scan
static bool tsdf_extract_size_ok(int nx, int ny, int nz) { return 3 * ((int64_t)nx * ny * nz) < ((int64_t)1 << 31); }

static bool tsdf_make_grid(const double* og, double a, int nx, int ny, int nz, TsdfGrid* g) {
  g->og[0] = og[0]; g->og[1] = og[1]; g->og[2] = og[2];
  g->a = a;
  g->n[0] = nx; g->n[1] = ny; g->n[2] = nz;
  return tsdf_grid_ok(*g);
}

}  // namespace dc

using namespace dc;

extern "C" {

int dc_tsdf_integrate(const void* vps, const void* dirs, const void* depth, int dtype, int64_t n, const uint8_t* mask, const double* pose,
                      double ox, double oy, double oz, double voxel, int nx, int ny, int nz, double trunc, int k_steps, double min_depth,
                      double max_range, double carve_from, int64_t* sum, int32_t* count, int64_t* stats, hipStream_t stream) {
  const double og[3] = {ox, oy, oz};
  TsdfGrid g;
  if (!tsdf_make_grid(og, voxel, nx, ny, nz, &g)) return DC_ERR_ARG;
  const TsdfRule r{trunc, voxel / 2.0, min_depth, max_range, carve_from, k_steps};
  if (!tsdf_rule_ok(r) || n < 0) return DC_ERR_ARG;
  if (dtype != DC_F32 && dtype != DC_F64) return DC_ERR_DTYPE;
  if (n == 0) return DC_OK;
  if (!vps || !dirs || !depth || !sum || !count || !stats) return DC_ERR_ARG;
  const int64_t blocks = (n + kBlock - 1) / kBlock;
  if (blocks > 0x7fffffff) return DC_ERR_UNSUPPORTED;
  if (dtype == DC_F32)
    hipLaunchKernelGGL(tsdf_integrate_kernel<float>, dim3((unsigned)blocks), dim3(kBlock), 0, stream, (const float*)vps, (const float*)dirs,
                       (const float*)depth, mask, n, pose, g, r, sum, count, stats);
  else
    hipLaunchKernelGGL(tsdf_integrate_kernel<double>, dim3((unsigned)blocks), dim3(kBlock), 0, stream, (const double*)vps, (const double*)dirs,
                       (const double*)depth, mask, n, pose, g, r, sum, count, stats);
  DC_HIP(hipGetLastError());
  return DC_OK;
}

size_t dc_tsdf_extract_workspace_bytes(int nx, int ny, int nz) {
  if (!tsdf_dims_ok(nx, ny, nz) || !tsdf_extract_size_ok(nx, ny, nz)) return 0;
  return tsdf_carve(nullptr, nx, ny, nz).bytes;
}

int dc_tsdf_extract_count(const int64_t* sum, const int32_t* count, int nx, int ny, int nz, int min_count, int64_t* totals, void* ws,
                          size_t ws_bytes, hipStream_t stream) {
  const double og[3] = {0.0, 0.0, 0.0};
  TsdfGrid g;
  if (!tsdf_make_grid(og, 1.0, nx, ny, nz, &g) || min_count < 1 || !sum || !count || !totals || !ws) return DC_ERR_ARG;
  if (!tsdf_extract_size_ok(nx, ny, nz)) return DC_ERR_UNSUPPORTED;
  if (ws_bytes < dc_tsdf_extract_workspace_bytes(nx, ny, nz)) return DC_ERR_WORKSPACE;
  const TsdfWorkspace w = tsdf_carve(ws, nx, ny, nz);
  const int64_t n_cells = tsdf_cell_count(nx, ny, nz), n_vox = (int64_t)nx * ny * nz;
  hipLaunchKernelGGL(tsdf_cells_kernel, dim3((unsigned)((n_cells + 1 + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, sum, count, g, min_count,
                     n_cells, w.flag);
  hipLaunchKernelGGL(tsdf_edges_kernel, dim3((unsigned)((n_vox + 1 + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, sum, count, g, min_count,
                     n_vox, (const int32_t*)w.flag, w.edge_cnt);
  DC_HIP(exclusive_scan_32(w.scan_ws, w.scan_ws_bytes, w.flag, w.cell_off, (size_t)n_cells + 1, stream));
  DC_HIP(exclusive_scan_32(w.scan_ws, w.scan_ws_bytes, w.edge_cnt, w.edge_off, (size_t)n_vox + 1, stream));
  hipLaunchKernelGGL(tsdf_totals_kernel, dim3(1), dim3(kWave), 0, stream, (const int32_t*)w.cell_off, n_cells, (const int32_t*)w.edge_off, n_vox,
                     totals);
  DC_HIP(hipGetLastError());
  return DC_OK;
}

int dc_tsdf_extract_fill(const int64_t* sum, const int32_t* count, double ox, double oy, double oz, double voxel, int nx, int ny, int nz,
                         int min_count, const void* ws, size_t ws_bytes, int64_t n_vertices, int64_t n_faces, double* vertices, int32_t* faces,
                         hipStream_t stream) {
  const double og[3] = {ox, oy, oz};
  TsdfGrid g;
  if (!tsdf_make_grid(og, voxel, nx, ny, nz, &g) || min_count < 1 || !sum || !count || !ws || n_vertices < 0 || n_faces < 0) return DC_ERR_ARG;
  if (!tsdf_extract_size_ok(nx, ny, nz)) return DC_ERR_UNSUPPORTED;
  if (ws_bytes < dc_tsdf_extract_workspace_bytes(nx, ny, nz)) return DC_ERR_WORKSPACE;
  if (n_vertices == 0 && n_faces == 0) return DC_OK;
  if ((n_vertices > 0 && !vertices) || (n_faces > 0 && !faces)) return DC_ERR_ARG;
  const TsdfWorkspace w = tsdf_carve(const_cast<void*>(ws), nx, ny, nz);
  const int64_t n_vox = (int64_t)nx * ny * nz;
  hipLaunchKernelGGL(tsdf_fill_kernel, dim3((unsigned)((n_vox + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, sum, count, g, min_count, n_vox,
                     (const int32_t*)w.flag, (const int32_t*)w.cell_off, (const int32_t*)w.edge_off, n_vertices, n_faces, vertices, faces);
  DC_HIP(hipGetLastError());
  return DC_OK;
}

}  // extern "C"
