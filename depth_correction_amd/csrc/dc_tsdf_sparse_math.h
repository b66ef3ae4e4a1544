// Sparse TSDF volumes: the rules of the block-allocated fusion and extraction (DESIGN "Sparse TSDF volumes"), shared by the kernels
// (dc_tsdf_sparse.hip), the host build (dc_hostcheck.cpp) and, restated in numpy, tests/tsdf_sparse_reference.py.  Built with
// -ffp-contract=off like dc_tsdf_math.h, whose sample loop (tsdf_ray_walk), fixed point and surface-nets functions this reuses.
//
// Lattice     origin og[3], voxel size a, truncation tau, h = a / 2, K = ceil(tau / h): the parameters of dc_tsdf_math.h, without dims.
//             A sample at p lies in voxel i = floor((p - og) / a) per axis, any integer; voxel i has the centre og + ((double)i + 0.5) a.
// Blocks      voxel i lies in block b = i >> 3 (arithmetic) with the local index ((lx 8) + ly) 8 + lz, l = i - 8 b.  Block coordinates
//             are valid in [-2^20, 2^20) per axis; the key ((bx + 2^20) << 42) | ((by + 2^20) << 21) | (bz + 2^20) has 63 bits and
//             ascends with (bx, by, bz).  A sample whose block is out of range counts as outside and does not become the last voxel.
// Table       keys uint64 [capacity], the first n_blocks ascending; slots int32 [capacity], the pool slot of each key; sum int64
//             [capacity, 512], count int32 [capacity, 512].  Looked up by binary search; position = the index in key order.
// Allocation  the keys of the visits that add (s >= -tau) and are not in the table, unique and ascending, get the slots n_blocks,
//             n_blocks + 1, ... until capacity; the table stays sorted.  Slots, and so every byte, are determined by the rule.
// Extraction  surface nets of dc_tsdf_math.h on the unbounded lattice: every cell exists, a voxel of a block that is not in the table is
//             unobserved, a cell belongs to the block of its corner 0; vertices ascend in (block key, local cell), faces in (block key
//             of q, local q, e).  nbr int32 [n_blocks, 27]: the table position of the block at b + (dx, dy, dz), index ((dx + 1) 3 + (dy
//             + 1)) 3 + (dz + 1), -1 where missing.
#pragma once
#include "dc_tsdf_math.h"

namespace dc {

constexpr int kTsdfBlockVoxels = 512;                    // 8 x 8 x 8
constexpr int kTsdfBlockRange = 1 << 20;                 // block coordinates in [-2^20, 2^20)
constexpr double kTsdfVoxelRange = 8388608.0;            // 2^23: voxel indices in [-2^23, 2^23)
constexpr uint64_t kTsdfNoKey = ~(uint64_t)0;            // no block has it: keys have 63 bits

// what a ray adds to the sparse stats int64 [5] beyond TsdfTally: the visits whose block is not in the table
struct TsdfSparseTally {
  TsdfTally t;
  int64_t dropped;
};

DC_HD bool tsdf_lattice_ok(const TsdfGrid& g) {
  return g.a > 0.0 && isfinite(g.a) && isfinite(g.og[0]) && isfinite(g.og[1]) && isfinite(g.og[2]);
}

// The address policy of the unbounded lattice (see TsdfDenseAddress): in range iff the block is; identity and centre by the three indices.
struct TsdfSparseAddress {
  const TsdfGrid& g;
  struct Voxel {
    int i[3];
  };
  DC_HD static Voxel none() { return Voxel{{(int)0x80000000, 0, 0}}; }
  DC_HD bool locate(const double* gx, Voxel* out) const {
    bool in = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) in = in && gx[a] >= -kTsdfVoxelRange && gx[a] < kTsdfVoxelRange;
    if (!in) return false;
    out->i[0] = (int)gx[0]; out->i[1] = (int)gx[1]; out->i[2] = (int)gx[2];
    return true;
  }
  DC_HD static bool same(const Voxel& a, const Voxel& b) { return a.i[0] == b.i[0] && a.i[1] == b.i[1] && a.i[2] == b.i[2]; }
  DC_HD double centre(int axis, const Voxel& x) const { return tsdf_centre(g, axis, x.i[axis]); }
};

DC_HD bool tsdf_block_ok(int bx, int by, int bz) {
  return bx >= -kTsdfBlockRange && bx < kTsdfBlockRange && by >= -kTsdfBlockRange && by < kTsdfBlockRange && bz >= -kTsdfBlockRange &&
         bz < kTsdfBlockRange;
}
DC_HD uint64_t tsdf_block_key(int bx, int by, int bz) {
  return ((uint64_t)(bx + kTsdfBlockRange) << 42) | ((uint64_t)(by + kTsdfBlockRange) << 21) | (uint64_t)(bz + kTsdfBlockRange);
}
DC_HD void tsdf_block_of_key(uint64_t key, int* b) {
  b[0] = (int)(key >> 42) - kTsdfBlockRange;
  b[1] = (int)((key >> 21) & 0x1fffff) - kTsdfBlockRange;
  b[2] = (int)(key & 0x1fffff) - kTsdfBlockRange;
}
DC_HD uint64_t tsdf_voxel_key(const int* i) { return tsdf_block_key(i[0] >> 3, i[1] >> 3, i[2] >> 3); }
DC_HD int tsdf_voxel_local(const int* i) { return (((i[0] & 7) * 8) + (i[1] & 7)) * 8 + (i[2] & 7); }

// the first position in keys [n] (ascending) whose key is >= key
DC_HD int64_t tsdf_table_lower(const uint64_t* keys, int64_t n, uint64_t key) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (keys[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}
// the position of key in keys [n], or -1
DC_HD int64_t tsdf_table_find(const uint64_t* keys, int64_t n, uint64_t key) {
  const int64_t p = tsdf_table_lower(keys, n, key);
  return p < n && keys[p] == key ? p : -1;
}

// A lane's cache of its last lookup: the search runs once per block change.
struct TsdfBlockCache {
  uint64_t key;
  int64_t pos;
};
DC_HD int64_t tsdf_cached_find(const uint64_t* keys, int64_t n, uint64_t key, TsdfBlockCache* c) {
  if (key != c->key) {
    c->key = key;
    c->pos = tsdf_table_find(keys, n, key);
  }
  return c->pos;
}

// ---- extraction ------------------------------------------------------------------------------------------------------------------
// the position of the d-th of the 27 blocks around the block at position p, d = ((dx + 1) 3 + (dy + 1)) 3 + (dz + 1); -1 where missing
DC_HD int32_t tsdf_block_neighbour(const uint64_t* keys, int64_t n, int64_t p, int d) {
  if (d == 13) return (int32_t)p;
  int b[3];
  tsdf_block_of_key(keys[p], b);
  const int q[3] = {b[0] + d / 9 - 1, b[1] + (d / 3) % 3 - 1, b[2] + d % 3 - 1};
  if (!tsdf_block_ok(q[0], q[1], q[2])) return -1;
  return (int32_t)tsdf_table_find(keys, n, tsdf_block_key(q[0], q[1], q[2]));
}

// The lattice point (lx, ly, lz), each in [-1, 9), relative to a block with the neighbours nbr27: the position of its block (-1: not in
// the table) and its local index.
DC_HD int tsdf_sparse_point(const int32_t* nbr27, int lx, int ly, int lz, int* local) {
  const int dx = lx >> 3, dy = ly >> 3, dz = lz >> 3;           // -1, 0, 1
  *local = (((lx & 7) * 8) + (ly & 7)) * 8 + (lz & 7);
  return nbr27[((dx + 1) * 3 + (dy + 1)) * 3 + (dz + 1)];
}
// the same as an index into sum / count (slot 512 + local), -1 when the block is missing
DC_HD int64_t tsdf_sparse_voxel(const int32_t* nbr27, const int32_t* slots, int lx, int ly, int lz) {
  int local;
  const int pos = tsdf_sparse_point(nbr27, lx, ly, lz, &local);
  return pos < 0 ? -1 : (int64_t)slots[pos] * kTsdfBlockVoxels + local;
}

// tsdf_cell_active for the cell whose corner 0 is the local point (lx, ly, lz), each in [-1, 8): a corner in a missing block is unobserved.
DC_HD bool tsdf_sparse_cell_active(const int64_t* sum, const int32_t* count, const int32_t* nbr27, const int32_t* slots, int min_count, int lx,
                                   int ly, int lz, int64_t* corner, int* inside_bits) {
  int bits = 0;
  bool all = true;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const int64_t v = tsdf_sparse_voxel(nbr27, slots, lx + (c & 1), ly + ((c >> 1) & 1), lz + (c >> 2));
    corner[c] = v;
    const bool obs = v >= 0 && tsdf_observed(count, v, min_count);
    all = all && obs;
    bits |= (obs && tsdf_inside(sum, v)) ? 1 << c : 0;
  }
  *inside_bits = bits;
  return all && bits != 0 && bits != 255;
}

// tsdf_edge_crosses for q = the local point (lx, ly, lz) of the block itself, each in [0, 8)
DC_HD bool tsdf_sparse_edge_crosses(const int64_t* sum, const int32_t* count, const int32_t* nbr27, const int32_t* slots, int min_count, int lx,
                                    int ly, int lz, int e, bool* q_inside) {
  const int64_t va = tsdf_sparse_voxel(nbr27, slots, lx, ly, lz), vb = tsdf_sparse_voxel(nbr27, slots, lx + (e == 0), ly + (e == 1), lz + (e == 2));
  if (va < 0 || vb < 0 || !tsdf_observed(count, va, min_count) || !tsdf_observed(count, vb, min_count)) return false;
  const bool ia = tsdf_inside(sum, va), ib = tsdf_inside(sum, vb);
  *q_inside = ia;
  return ia != ib;
}

// tsdf_edge_cells: cells <- position 512 + local of the four cells around the edge, in the order of dc_tsdf_math.h; false when one of
// them belongs to a missing block (such a cell is not active).
DC_HD bool tsdf_sparse_edge_cells(const int32_t* nbr27, int lx, int ly, int lz, int e, int64_t* cells) {
  const int b = (e + 1) % 3, c = (e + 2) % 3;
  const int db[4] = {-1, 0, 0, -1}, dc_[4] = {-1, -1, 0, 0};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    int q[3] = {lx, ly, lz};
    q[b] += db[j];
    q[c] += dc_[j];
    int local;
    const int pos = tsdf_sparse_point(nbr27, q[0], q[1], q[2], &local);
    if (pos < 0) return false;
    cells[j] = (int64_t)pos * kTsdfBlockVoxels + local;
  }
  return true;
}

// the upper bound of distinct blocks a ray's visits can meet, and the share of the candidate buffer every ray gets
DC_HD int tsdf_sparse_ray_blocks(int K) { return 2 * K + 1; }

}  // namespace dc
