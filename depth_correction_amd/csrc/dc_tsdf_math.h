// Surface reconstruction: the rules of the TSDF fusion and of the surface-nets extraction (DESIGN "Surface reconstruction"), shared by
// the kernels (dc_tsdf.hip), the host build (dc_hostcheck.cpp) and, restated in numpy, tests/tsdf_reference.py.
//
// Everything is fp64 and every product and sum is rounded on its own (the translation units that include this are built with
// -ffp-contract=off); a voxel's sum is a fixed-point integer, so the order in which rays arrive does not change a bit.
//
// Volume      minimum corner og[3], voxel size a > 0, dims (nx, ny, nz), each >= 2, nx ny nz < 2^31.  Voxel (ix, iy, iz) has the linear
//             index (ix ny + iy) nz + iz and the centre og + ((double)i + 0.5) a.  Accumulators: sum int64 [V], count int32 [V].
//             Truncation tau > 0, step h = a / 2, K = ceil(tau / h) (formed by the caller).
// One ray     o = R vp + t and u = R dir for a pose (row sums left to right: ((R0 v0 + R1 v1) + R2 v2) + t), o = vp and u = dir without.
//             Skipped: mask 0, any of o, u, d not finite, d <= min_depth, d > max_range (+inf: no limit).
//             k runs ascending from -K, or with carve_from >= 0 from -max(K, (int)floor((d - carve_from) / h)) (the quotient capped at
//             2^30), to K.  Sample t = d + (double)k h, used when t > 0: p = o + t u, g = (p - og) / a, i = floor(g) per axis; a sample
//             with some g outside [0, n) (tested on the doubles; a NaN is outside) is counted as outside.  A sample in the voxel of the
//             ray's last in-grid sample is dropped.  With the voxel's centre c,
//               s = d - ((u0 (c0 - o0) + u1 (c1 - o1)) + u2 (c2 - o2));
//             s < -tau (or NaN) adds nothing, but the voxel is the last one visited; else q = llrint(min(s, tau) / tau 2^20), ties to
//             even, sum[v] += q, count[v] += 1.
// Value       f = (double)sum / ((double)count 2^20); observed iff count >= min_count (>= 1); inside iff sum < 0.
// Extraction  surface nets on the lattice of voxel centres; see tsdf_cell_vertex and tsdf_edge_cells below.
#pragma once
#include "dc_common.h"
#include <math.h>

namespace dc {

constexpr double kTsdfOne = 1048576.0;                   // 2^20: the fixed-point unit of a voxel's sum
constexpr double kTsdfMaxCarve = 1073741824.0;           // 2^30: cap of the carving's first step

struct TsdfGrid {
  double og[3], a;
  int n[3];
};
struct TsdfRule {
  double tau, h, min_depth, max_range, carve_from;       // carve_from < 0 (or NaN): no carving
  int K;
};

// what a ray adds to stats int64 [4] = {rays used, rays skipped, samples outside the grid, visits}
struct TsdfTally {
  int64_t used, skipped, outside, visits;
};

DC_HD bool tsdf_dims_ok(int nx, int ny, int nz) {
  return nx >= 2 && ny >= 2 && nz >= 2 && (int64_t)nx * ny * nz < ((int64_t)1 << 31);
}
DC_HD bool tsdf_grid_ok(const TsdfGrid& g) {
  return tsdf_dims_ok(g.n[0], g.n[1], g.n[2]) && g.a > 0.0 && isfinite(g.a) && isfinite(g.og[0]) && isfinite(g.og[1]) && isfinite(g.og[2]);
}
DC_HD bool tsdf_rule_ok(const TsdfRule& r) {
  return r.tau > 0.0 && isfinite(r.tau) && r.h > 0.0 && isfinite(r.h) && r.K >= 1 && r.K <= (1 << 20) && !isnan(r.min_depth) &&
         !isnan(r.max_range);
}

DC_HD int64_t tsdf_index(const TsdfGrid& g, int ix, int iy, int iz) { return ((int64_t)ix * g.n[1] + iy) * g.n[2] + iz; }
DC_HD double tsdf_centre(const TsdfGrid& g, int axis, int i) { return g.og[axis] + ((double)i + 0.5) * g.a; }

// The address policy of the dense volume: what the sample loop (tsdf_ray_walk) asks of a volume.  locate() is the in-range test on the
// floored doubles and gives the voxel; same() is the identity of the "voxel of the last in-grid sample" rule; centre() the voxel's centre.
// The sparse volume (dc_tsdf_sparse_math.h) supplies another policy; the loop itself exists once.
struct TsdfDenseAddress {
  const TsdfGrid& g;
  struct Voxel {
    int i[3];
    int64_t v;
  };
  DC_HD static Voxel none() { return Voxel{{0, 0, 0}, -1}; }
  DC_HD bool locate(const double* gx, Voxel* out) const {
    bool in = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) in = in && gx[a] >= 0.0 && gx[a] < (double)g.n[a];
    if (!in) return false;
    out->i[0] = (int)gx[0]; out->i[1] = (int)gx[1]; out->i[2] = (int)gx[2];
    out->v = tsdf_index(g, out->i[0], out->i[1], out->i[2]);
    return true;
  }
  DC_HD static bool same(const Voxel& a, const Voxel& b) { return a.v == b.v; }
  DC_HD double centre(int axis, const Voxel& x) const { return tsdf_centre(g, axis, x.i[axis]); }
};

// One ray.  vp, dir [3] and d are the widened inputs, pose a row-major [16] or null; add(voxel, q) receives every visit that adds.
template <typename Address, typename Add>
DC_HD void tsdf_ray_walk(const double* vp, const double* dir, double d, bool masked_in, const double* pose, const Address& ad,
                         const TsdfRule& r, TsdfTally* tally, Add add) {
  double o[3], u[3];
  if (pose) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double* R = pose + 4 * a;
      o[a] = ((R[0] * vp[0] + R[1] * vp[1]) + R[2] * vp[2]) + R[3];
      u[a] = (R[0] * dir[0] + R[1] * dir[1]) + R[2] * dir[2];
    }
  } else {
#pragma unroll
    for (int a = 0; a < 3; ++a) { o[a] = vp[a]; u[a] = dir[a]; }
  }
  const bool finite = isfinite(o[0]) && isfinite(o[1]) && isfinite(o[2]) && isfinite(u[0]) && isfinite(u[1]) && isfinite(u[2]) && isfinite(d);
  if (!masked_in || !finite || d <= r.min_depth || d > r.max_range) {
    tally->skipped += 1;
    return;
  }
  tally->used += 1;
  int k_lo = -r.K;
  if (r.carve_from >= 0.0) {
    double c = floor((d - r.carve_from) / r.h);
    c = c > kTsdfMaxCarve ? kTsdfMaxCarve : c;
    const int ci = c > 0.0 ? (int)c : 0;
    k_lo = -(r.K > ci ? r.K : ci);
  }
  typename Address::Voxel last = Address::none();
  for (int k = k_lo; k <= r.K; ++k) {
    const double t = d + (double)k * r.h;
    if (!(t > 0.0)) continue;
    double gx[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double p = o[a] + t * u[a];
      gx[a] = floor((p - ad.g.og[a]) / ad.g.a);
    }
    typename Address::Voxel x;
    if (!ad.locate(gx, &x)) {
      tally->outside += 1;
      continue;
    }
    if (Address::same(x, last)) continue;
    last = x;
    const double c0 = ad.centre(0, x), c1 = ad.centre(1, x), c2 = ad.centre(2, x);
    const double s = d - ((u[0] * (c0 - o[0]) + u[1] * (c1 - o[1])) + u[2] * (c2 - o[2]));
    if (!(s >= -r.tau)) continue;
    const double m = s < r.tau ? s : r.tau;
    add(x, (int64_t)llrint(m / r.tau * kTsdfOne));
    tally->visits += 1;
  }
}

// The dense volume's ray: add(v, q) receives the linear index of every visit that adds.
template <typename Add>
struct TsdfDenseAdd {
  Add add;
  DC_HD void operator()(const TsdfDenseAddress::Voxel& x, int64_t q) { add(x.v, q); }
};
template <typename Add>
DC_HD void tsdf_ray(const double* vp, const double* dir, double d, bool masked_in, const double* pose, const TsdfGrid& g,
                    const TsdfRule& r, TsdfTally* tally, Add add) {
  tsdf_ray_walk(vp, dir, d, masked_in, pose, TsdfDenseAddress{g}, r, tally, TsdfDenseAdd<Add>{add});
}

// ---- extraction ------------------------------------------------------------------------------------------------------------------
DC_HD bool tsdf_observed(const int32_t* count, int64_t v, int min_count) { return count[v] >= min_count; }
DC_HD bool tsdf_inside(const int64_t* sum, int64_t v) { return sum[v] < 0; }
DC_HD double tsdf_value(const int64_t* sum, const int32_t* count, int64_t v) { return (double)sum[v] / ((double)count[v] * kTsdfOne); }

DC_HD int64_t tsdf_cell_count(int nx, int ny, int nz) { return (int64_t)(nx - 1) * (ny - 1) * (nz - 1); }
DC_HD int64_t tsdf_cell_index(const TsdfGrid& g, int x, int y, int z) { return ((int64_t)x * (g.n[1] - 1) + y) * (g.n[2] - 1) + z; }
DC_HD bool tsdf_cell_exists(const TsdfGrid& g, int x, int y, int z) {
  return x >= 0 && y >= 0 && z >= 0 && x < g.n[0] - 1 && y < g.n[1] - 1 && z < g.n[2] - 1;
}

// Cell (x, y, z), which exists: its corner c = bx + 2 by + 4 bz is the lattice point (x + bx, y + by, z + bz).  Active iff all eight are
// observed and their inside flags are not all equal; *inside_bits <- the flags, bit c.
DC_HD bool tsdf_cell_active(const int64_t* sum, const int32_t* count, const TsdfGrid& g, int min_count, int x, int y, int z, int64_t* corner,
                            int* inside_bits) {
  int bits = 0;
  bool all = true;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const int64_t v = tsdf_index(g, x + (c & 1), y + ((c >> 1) & 1), z + (c >> 2));
    corner[c] = v;
    all = all && tsdf_observed(count, v, min_count);
    bits |= tsdf_inside(sum, v) ? 1 << c : 0;
  }
  *inside_bits = bits;
  return all && bits != 0 && bits != 255;
}

// The vertex of an active cell: over the edges (0,1) (0,2) (0,4) (1,3) (1,5) (2,3) (2,6) (3,7) (4,5) (4,6) (5,7) (6,7) in this order,
// those whose ends differ cross at corner(a) + r (corner(b) - corner(a)) with r = f_a / (f_a - f_b), in the cell's unit coordinates;
// the vertex is og + (((x, y, z) + 0.5) + (the sum of the crossings, left to right) / their number) a.
DC_HD void tsdf_cell_vertex(const int64_t* sum, const int32_t* count, const TsdfGrid& g, int x, int y, int z, const int64_t* corner,
                            int inside_bits, double* vertex) {
  const int ea[12] = {0, 0, 0, 1, 1, 2, 2, 3, 4, 4, 5, 6}, eb[12] = {1, 2, 4, 3, 5, 3, 6, 7, 5, 6, 7, 7};
  double acc[3] = {0.0, 0.0, 0.0};
  int n = 0;
#pragma unroll
  for (int e = 0; e < 12; ++e) {
    const int a = ea[e], b = eb[e];
    if ((((inside_bits >> a) ^ (inside_bits >> b)) & 1) == 0) continue;
    const double fa = tsdf_value(sum, count, corner[a]), fb = tsdf_value(sum, count, corner[b]);
    const double r = fa / (fa - fb);
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
      const double ca = (double)((a >> ax) & 1), cb = (double)((b >> ax) & 1);
      acc[ax] = acc[ax] + (ca + r * (cb - ca));
    }
    ++n;
  }
  const int xyz[3] = {x, y, z};
#pragma unroll
  for (int ax = 0; ax < 3; ++ax) vertex[ax] = g.og[ax] + (((double)xyz[ax] + 0.5) + acc[ax] / (double)n) * g.a;
}

// The lattice edge q -> q + e (q = (x, y, z), e = 0, 1, 2) crosses iff it is in range, both ends are observed and their inside flags
// differ; *q_inside <- q's flag.
DC_HD bool tsdf_edge_crosses(const int64_t* sum, const int32_t* count, const TsdfGrid& g, int min_count, int x, int y, int z, int e,
                             bool* q_inside) {
  const int q[3] = {x, y, z};
  if (q[e] + 1 >= g.n[e]) return false;
  const int64_t va = tsdf_index(g, x, y, z), vb = tsdf_index(g, x + (e == 0), y + (e == 1), z + (e == 2));
  if (!tsdf_observed(count, va, min_count) || !tsdf_observed(count, vb, min_count)) return false;
  const bool ia = tsdf_inside(sum, va), ib = tsdf_inside(sum, vb);
  *q_inside = ia;
  return ia != ib;
}

// The four cells around that edge: with b = (e + 1) % 3 and c = (e + 2) % 3, q offset by (-1,-1), (0,-1), (0,0), (-1,0) along (b, c).
// False when one of them does not exist.  A crossing edge emits the quad of their vertices in this order when q is inside, reversed
// otherwise, split into (q0, q1, q2) and (q0, q2, q3), if all four are active.
DC_HD bool tsdf_edge_cells(const TsdfGrid& g, int x, int y, int z, int e, int64_t* cells) {
  const int b = (e + 1) % 3, c = (e + 2) % 3;
  const int db[4] = {-1, 0, 0, -1}, dc_[4] = {-1, -1, 0, 0};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    int q[3] = {x, y, z};
    q[b] += db[j];
    q[c] += dc_[j];
    if (!tsdf_cell_exists(g, q[0], q[1], q[2])) return false;
    cells[j] = tsdf_cell_index(g, q[0], q[1], q[2]);
  }
  return true;
}

}  // namespace dc
