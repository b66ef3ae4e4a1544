// TEST-ONLY host build of the per-point math the kernels use (dc_eig3.h, dc_pointmath.h).
// Lets the CPU test-suite pin the eigen-solver and the covariance / loss / backward-coefficient
// arithmetic against LAPACK and the oracle without a GPU.  Never loaded by depth_correction_amd.
#include <algorithm>
#include <vector>
#include "dc_common.h"
#include "dc_bvh.h"
#include "dc_eig3.h"
#include "dc_pointmath.h"
#include "dc_rowsum.h"
#include "dc_slam_math.h"
#include "dc_trimath.h"
#include "dc_meshloss_math.h"
#include "dc_cloudloss_math.h"
#include "dc_biasmath.h"
#include "dc_beammath.h"
#include "dc_raymath.h"
#include "dc_sweepmath.h"
#include "dc_surfelmath.h"
#include "dc_planemath.h"
#include "dc_dynmath.h"
#include "dc_rangeimage_math.h"
#include "dc_align_math.h"
#include "dc_globalreg_math.h"
#include "dc_planereg_math.h"
#include "dc_tsdf_math.h"
#include "dc_tsdf_sparse_math.h"
#include "dc_tsdf_track_math.h"
#include "dc_tsdf_loss_math.h"
#include "dc_tsdf_cast_math.h"
#include "dc_cons_route.h"

// The finish kernels' prologue on the host: false when the registration has ended, else the NV totals of partials [n_blocks, NV]
// summed in the kernel's order.
template <int NV>
static bool host_icp_totals(const double* partials, int n_blocks, const int32_t* status, double* tot) {
  if (status[0] != 0) return false;
  for (int q = 0; q < NV; ++q) tot[q] = dc::rows_sum<dc::kRowSumLanes>(partials, n_blocks, NV, q);
  return true;
}

extern "C" {

// the kernel route of a sequence evaluation (dc_cons_route.h: what sequence_eval_impl runs before it launches anything); nothing behind
// the descriptor's pointers is read.  has_*: which of w / poses / out the call passes; options int [7] = {no_tab, fwd_generic, no_basis,
// two_pass, step_var, pose_three_pass, step_six}; out int64 [22], in the order of the assignments below.  Returns the call's status.
int dc_host_choose_route(const dcSequenceDesc* d, int has_w, int has_poses, int has_out, int want_grad, int want_exponent_grad,
                         int want_pose_grad, int chained, const int* options, int64_t* out) {
  dc::RouteOptions o;
  o.no_tab = options[0] != 0; o.fwd_generic = options[1]; o.no_basis = options[2] != 0; o.two_pass = options[3] != 0;
  o.step_var = options[4]; o.pose_three_pass = options[5] != 0; o.step_six = options[6] != 0;
  static const double dummy = 0.0;
  dc::SeqRoute r;
  const int rc = dc::dc_choose_route_call(d, has_w ? &dummy : nullptr, has_poses ? &dummy : nullptr, has_out ? &dummy : nullptr, want_grad,
                                          want_exponent_grad, want_pose_grad, chained != 0, o, &r);
  const int64_t v[22] = {r.kind, r.f64, r.k, r.P, r.cap, r.six, r.round2, r.table_loss, r.use_hdr, r.max_rows, (int64_t)r.lds_fwd, r.rows_fwd,
                         (int64_t)r.lds_bwd, r.rows_bwd, r.grouped, r.n_terms, r.n_acc, r.n_red, r.n_rows, r.g_blocks, r.rows, r.grid};
  for (int i = 0; i < 22; ++i) out[i] = v[i];
  return rc;
}

// use_table of dc_cons_route.h (the chooser and consistency_fwd_impl / consistency_bwd_impl share it): out int64 [2] = {LDS bytes, rows}
int dc_host_use_table(const dcBlockTable* t, int no_tab, int layout, int stride, int row_bytes, int extra_rows, int64_t lds_limit, int64_t* out) {
  size_t bytes = 0;
  int rows = 0;
  const bool ok = dc::use_table(t, no_tab != 0, layout, stride, (uint32_t)row_bytes, extra_rows, (size_t)lds_limit, &bytes, &rows);
  out[0] = (int64_t)bytes; out[1] = rows;
  return ok ? 1 : 0;
}

// cov: [n,6] (xx xy xz yy yz zz) -> lam [n,3], vec [n,9] (vec[i, k*3 + c] = component c of eigenvector k)
void dc_host_eig3(const double* cov, long n, double* lam, double* vec) {
  for (long i = 0; i < n; ++i) {
    const double* c = cov + i * 6;
    double V[3][3];
    dc::eig3_sym<double>(c[0], c[1], c[2], c[3], c[4], c[5], lam + i * 3, V);
    for (int k = 0; k < 3; ++k)
      for (int j = 0; j < 3; ++j) vec[i * 9 + k * 3 + j] = V[k][j];
  }
}

// round 4's full solver (what features_fwd_tile_kernel calls)
void dc_host_eig3_v2(const double* cov, long n, double* lam, double* vec) {
  for (long i = 0; i < n; ++i) {
    const double* c = cov + i * 6;
    double V[3][3];
    dc::eig3_sym_v2(c[0], c[1], c[2], c[3], c[4], c[5], lam + i * 3, V);
    for (int k = 0; k < 3; ++k)
      for (int j = 0; j < 3; ++j) vec[i * 9 + k * 3 + j] = V[k][j];
  }
}

// Hot-path variant: smallest eigenpair + trace only.
void dc_host_eig3_smallest(const double* cov, long n, double* lam0, double* v0, double* tr) {
  for (long i = 0; i < n; ++i) {
    const double* c = cov + i * 6;
    dc::eig3_smallest(c[0], c[1], c[2], c[3], c[4], c[5], lam0 + i, v0 + i * 3, tr + i);
  }
}

// round 2's solver (isolate-then-deflate with three cross products), still the A-B baseline of the step kernel
void dc_host_eig3_smallest_r2(const double* cov, long n, double* lam0, double* v0, double* tr) {
  for (long i = 0; i < n; ++i) {
    const double* c = cov + i * 6;
    dc::eig3_smallest_r2(c[0], c[1], c[2], c[3], c[4], c[5], lam0 + i, v0 + i * 3, tr + i);
  }
}

// the slimmer solver of the one-pass step kernel (trace-1 core: adjugate eigenvector, one reciprocal)
void dc_host_eig3_smallest_v2(const double* cov, long n, double* lam0, double* v0, double* tr) {
  for (long i = 0; i < n; ++i) {
    const double* c = cov + i * 6;
    dc::eig3_smallest_v2(c[0], c[1], c[2], c[3], c[4], c[5], lam0 + i, v0 + i * 3, tr + i);
  }
}

// One neighbourhood per row of nbr [n,k]; points [np,3].  Outputs per centre: mean[3], cov6[6], lam[3], v0[3],
// loss, c1, c2 (loss / backward coefficients for an unmasked point with zero offset).
void dc_host_neighbourhoods(const double* points, const int* nbr, long n, int k, double scale, int loss_kind,
                            int normalization, int sqrt_, double* mean, double* cov6, double* lam, double* v0,
                            double* loss, double* c1, double* c2) {
  dc::LossParams lp{loss_kind, normalization, sqrt_};
  for (long i = 0; i < n; ++i) {
    const double* xi = points + i * 3;
    dc::CovAcc acc;
    dc::cov_init(acc);
    for (int q = 0; q < k; ++q) {
      const int j = nbr[i * k + q];
      if (j < 0) continue;
      const double* xj = points + (long)j * 3;
      dc::cov_add(acc, xj[0] - xi[0], xj[1] - xi[1], xj[2] - xi[2], 1.0);
    }
    double moff[3], cm[3], C[6], D, omega, V[3][3], l[3];
    dc::cov_finish(acc, scale, moff, cm, C, &D, &omega);
    dc::eig3_sym<double>(C[0], C[1], C[2], C[3], C[4], C[5], l, V);
    for (int a = 0; a < 3; ++a) { mean[i * 3 + a] = xi[a] + moff[a]; lam[i * 3 + a] = l[a]; v0[i * 3 + a] = V[0][a]; }
    for (int a = 0; a < 6; ++a) cov6[i * 6 + a] = C[a];
    loss[i] = dc::loss_and_coeffs(lp, l[0], l[0] + l[1] + l[2], D, 0.0, true, c1 + i, c2 + i);
  }
}

double dc_host_model_depth(int kind, int n_terms, const double* w, const double* e, double depth, double inc, int in_mask) {
  dc::ModelParams mp;
  mp.kind = kind; mp.n_terms = n_terms;
  for (int k = 0; k < DC_MAX_MODEL_TERMS; ++k) { mp.w[k] = k < n_terms ? w[k] : 0.0; mp.e[k] = k < n_terms ? e[k] : 0.0; }
  return dc::model_depth(mp, depth, inc, in_mask != 0);
}

void dc_host_normal_inc(const double* dir, const double* v0, double* normal, double* inc) {
  dc::normal_and_incidence(dir, v0, normal, inc);
}

// ICP normal equations (dc_slam.hip's finish kernel): a21 = JtJ upper triangle row by row, b6 = Jtr -> x = -(JtJ)^-1 Jtr; 1 = singular
int dc_host_icp_solve(const double* a21, const double* b6, double* x6) {
  double A[36], L[36], y[6];
  for (int r = 0; r < 6; ++r)
    for (int c = 0; c < 6; ++c) A[r * 6 + c] = a21[dc::sym_index<6>(r, c)];
  return dc::icp_solve<6>(A, b6, x6, L, y);
}

// out = [R(x[0:3]) x[3:6]; 0 1] T (row-major 4 x 4): the finish kernel's pose update
void dc_host_icp_step(const double* x6, const double* T, double* out) { dc::icp_apply_step(x6, T, out); }

// The fixed-order row sum every finish kernel shares (dc_rowsum.h): value q of rows [n_rows, stride] on `lanes` = 4 or 8 lanes
// (the chains of dc_cloud_loss's finishing; everything else); NaN for another lane count.
double dc_host_rows_sum(const double* rows, int64_t n_rows, int stride, int q, int lanes) {
  if (lanes == 4) return dc::rows_sum<4>(rows, n_rows, stride, q);
  if (lanes == 8) return dc::rows_sum<8>(rows, n_rows, stride, q);
  return NAN;
}

// dc_icp_finish on the host: the same argument checks, the partials summed in the kernel's order, the same tail; state [DC_ICP_STATE_COUNT]
// and status [4] are host arrays.  0, or 1 for arguments dc_icp_finish refuses.
int dc_host_icp_finish(const double* partials, int n_blocks, int64_t m, double min_rot, double min_trans, int smooth, int max_iters,
                       double max_rot, double max_trans, int min_pairs, double* state, int32_t* status) {
  if (!dc::icp_finish_args_ok(partials, n_blocks, m, smooth, max_iters, state, status)) return 1;
  double tot[DC_ICP_PARTIALS];
  const dc::IcpParams prm{min_rot, min_trans, max_rot, max_trans, smooth, max_iters, min_pairs};
  if (host_icp_totals<DC_ICP_PARTIALS>(partials, n_blocks, status, tot)) dc::icp_finish_tail(tot, m, prm, state, status);
  return 0;
}

// dc_icp_ct_finish on the host, likewise: partials [n_blocks, DC_ICP_CT_PARTIALS], state [DC_ICP_STATE_COUNT], ct_state
// [DC_ICP_CT_STATE_COUNT] and status [4] are host arrays.
int dc_host_icp_ct_finish(const double* partials, int n_blocks, int64_t m, double min_rot, double min_trans, int smooth, int max_iters,
                          double max_rot, double max_trans, int min_pairs, double beta_v, double beta_w, double max_twist_trans,
                          double max_twist_rot, double* state, double* ct_state, int32_t* status) {
  if (!dc::icp_finish_args_ok(partials, n_blocks, m, smooth, max_iters, state, status) || !ct_state || !(beta_v >= 0.0) || !(beta_w >= 0.0))
    return 1;
  double tot[DC_ICP_CT_PARTIALS], work[dc::kIcpCtWork];
  const dc::IcpParams prm{min_rot, min_trans, max_rot, max_trans, smooth, max_iters, min_pairs};
  const dc::IcpCtParams cp{beta_v, beta_w, max_twist_trans, max_twist_rot};
  if (host_icp_totals<DC_ICP_CT_PARTIALS>(partials, n_blocks, status, tot)) dc::icp_ct_finish_tail(tot, m, prm, cp, state, ct_state, status, work);
  return 0;
}

// The left Jacobian of SO(3) (dc_sweepmath.h): J [9] row-major = J_l(a) for a [3]; u [3] (optional) -> jtu [3] = J_l(a)^T u.
void dc_host_sweep_left_jacobian(const double* a, double* J, const double* u, double* jtu) {
  const dc::SweepRot r = dc::sweep_rot(1.0, a[0], a[1], a[2]);
  const dc::SweepJl j = dc::sweep_left_jacobian(r);
  dc::sweep_jl_matrix(r, j, J);
  if (u && jtu) dc::sweep_jl_transposed(r, j, u[0], u[1], u[2], jtu);
}

// dc_mesh_closest's per-triangle step: closest point of tri (a, b, c) [9] to p [3] -> closest [3], *region (optional) the branch
// taken (dc::kTri*); returns the squared distance the kernel compares
double dc_host_closest_on_triangle(const double* tri, const double* p, double* closest, int* region) {
  return dc::closest_on_triangle(tri, p, closest, region);
}

// dc_mesh_loss's per-point term: x [3], c [3] -> *r = |x - c|, grad [3] = dl/dx; returns l = r (r^2 with `squared`)
double dc_host_mesh_loss_term(const double* x, const double* c, int squared, double* r, double* grad) {
  return dc::mesh_loss_term(x, c, squared != 0, r, grad);
}

// dc_cloud_loss's per-point term: x [3], y [3] (the survey point), n [3] (its normal, read with `plane`) -> *r (n . (x - y), or
// |x - y|), grad [3] = dl/dx; returns l = |r| (r^2 with `squared`)
double dc_host_cloud_loss_term(const double* x, const double* y, const double* n, int plane, int squared, double* r, double* grad) {
  return dc::cloud_loss_term(x, y, n, plane != 0, squared != 0, r, grad);
}

// dc_mesh_sample's sample i of `seed` on the triangle tri [9]: u [3] <- the three uniforms, p [3] <- the point
void dc_host_mesh_sample_point(const double* tri, int64_t seed, int64_t i, double* u, double* p) {
  dc::mesh_sample_uniforms(seed, i, u);
  dc::mesh_sample_point(tri, u[1], u[2], p);
}

// dc_mesh_sample's face for the uniform u0 and the inclusive area prefix sum area_cdf [n]
int64_t dc_host_mesh_sample_face(const double* area_cdf, int64_t n, double u0) { return dc::mesh_sample_face(area_cdf, n, u0); }

// dc_bias_accumulate on host arrays: the same argument checks, per-ray terms (dc_biasmath.h) and `out` layout; the sums run over the
// rays in index order (the kernel's order is per block, then over the blocks: equal counts, sums equal up to rounding).  0, or 1
// for arguments dc_bias_accumulate refuses.
int dc_host_bias_accumulate(const void* depth, const void* inc_est, int dtype, const uint8_t* mask, const int32_t* face,
                            const double* t_true, const double* inc_true, int64_t n, int model_kind, const double* exponent, int n_terms,
                            int n_bins, double max_residual, double* out) {
  if (n < 0 || n_bins < 1 || n_bins > DC_BIAS_MAX_BINS || n_terms < 1 || n_terms > DC_BIAS_MAX_TERMS || !exponent || !out ||
      (model_kind != DC_MODEL_POLYNOMIAL && model_kind != DC_MODEL_SCALED_POLYNOMIAL) || max_residual != max_residual)
    return 1;
  if (n > 0 && (!depth || !face || !t_true || !inc_true)) return 1;
  if (dtype != DC_F32 && dtype != DC_F64) return 1;
  dc::BiasParams prm;
  prm.kind = model_kind; prm.n_terms = n_terms; prm.n_bins = n_bins; prm.max_residual = max_residual;
  for (int k = 0; k < DC_BIAS_MAX_TERMS; ++k) {
    prm.e[k] = k < n_terms ? exponent[k] : 0.0;
    if (!(prm.e[k] - prm.e[k] == 0.0)) return 1;
  }
  const int total = DC_BIAS_OUT_COUNT(n_bins, n_terms);
  for (int q = 0; q < total; ++q) out[q] = 0.0;
  double flat[dc::kBiasFlat];
  for (int q = 0; q < dc::kBiasFlat; ++q) flat[q] = 0.0;
  for (int64_t i = 0; i < n; ++i) {
    const double d = dtype == DC_F32 ? (double)((const float*)depth)[i] : ((const double*)depth)[i];
    const double ge = !inc_est ? NAN : (dtype == DC_F32 ? (double)((const float*)inc_est)[i] : ((const double*)inc_est)[i]);
    const dc::BiasRay o = dc::bias_ray(prm, d, ge, mask ? mask[i] != 0 : true, face[i], t_true[i], inc_true[i]);
    dc::bias_flat_add(prm, o, inc_true[i], ge, flat);
    if (o.bin < 0) continue;
    double v[dc::kBiasBinVals];
    dc::bias_bin_terms(o, v);
    double* row = out + DC_BIAS_TOTALS + DC_BIAS_BIN_COLS * o.bin;
    row[0] += 1.0;
    for (int q = 0; q < dc::kBiasBinVals; ++q) row[1 + q] += v[q];
  }
  for (int j = 0; j < dc::kBiasFlat; ++j) {
    const int dst = dc::bias_flat_to_out(j, n_bins, n_terms);
    if (dst >= 0) out[dst] = flat[j];
  }
  return 0;
}

// bin of the true incidence angle g (dc_biasmath.h)
int dc_host_bias_bin(double g, int n_bins) { return dc::bias_bin(g, n_bins); }

// dc_beam_subrays on host arrays (dc_beammath.h): vps / dirs double [n,3], pattern double [n_samples,3] -> origins / dirs double
// [n, n_samples, 3]
void dc_host_beam_subrays(const double* vps, const double* dirs, int64_t n, const double* pattern, int n_samples, double r0, double spread,
                          double* origins_out, double* dirs_out) {
  for (int64_t i = 0; i < n; ++i) {
    const dc::BeamFrame f = dc::beam_frame(dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2]);
    for (int j = 0; j < n_samples; ++j)
      dc::beam_subray(f, vps[3 * i], vps[3 * i + 1], vps[3 * i + 2], pattern[3 * j], pattern[3 * j + 1], r0, spread,
                      origins_out + 3 * (i * n_samples + j), dirs_out + 3 * (i * n_samples + j));
  }
}

// the reduction of dc_raycast_beams on n bundles of sub-ray returns [n, n_samples] (dc_beammath.h), with its argument checks
int dc_host_beam_select(const int32_t* sub_face, const double* sub_t, const double* sub_w, int64_t n, int n_samples, int detection, double tau,
                        int min_hits, int32_t* face_out, double* depth_out, int32_t* n_hits_out) {
  if (n < 0 || n_samples < 1 || n_samples > DC_BEAM_MAX_SAMPLES || (n_samples & (n_samples - 1)) != 0 || !(tau > 0.0) || !(tau <= 1.0) ||
      min_hits < 1 || min_hits > n_samples || (detection != DC_BEAM_MEAN && detection != DC_BEAM_QUANTILE))
    return DC_ERR_ARG;
  for (int64_t i = 0; i < n; ++i)
    dc::beam_select(sub_face + i * n_samples, sub_t + i * n_samples, sub_w + i * n_samples, n_samples, detection, tau, min_hits, face_out + i,
                    depth_out + i, n_hits_out + i);
  return DC_OK;
}

// The moving-sweep map on host arrays (dc_sweepmath.h): row i of x double [n,3] at sweep time tau[i] under the twist row twist_index[i]
// (int32 [n]) of twists double [., 6] -> point_out = D(tau) x, dir_out = Exp(tau w) x, double [n,3] each (either may be NULL)
void dc_host_sweep_apply(const double* x, const double* tau, const int32_t* twist_index, const double* twists, int64_t n, double* point_out,
                         double* dir_out) {
  for (int64_t i = 0; i < n; ++i) {
    const double* tw = twists + 6 * (int64_t)twist_index[i];
    const dc::SweepRot r = dc::sweep_rot(tau[i], tw[3], tw[4], tw[5]);
    if (point_out) dc::sweep_point(r, tau[i], tw[0], tw[1], tw[2], x[3 * i], x[3 * i + 1], x[3 * i + 2], point_out + 3 * i);
    if (dir_out) dc::sweep_rotate(r, x[3 * i], x[3 * i + 1], x[3 * i + 2], dir_out + 3 * i);
  }
}

// ---- the BVH ray caster's per-ray arithmetic (dc_raymath.h) --------------------------------------------------------------------------
// leaf boxes of the triangles tri [n,9] -> box f32 [n,6] (lo xyz, hi xyz), as fit_kernel writes them
void dc_host_ray_boxes(const double* tri, int64_t n, float* box) {
  for (int64_t i = 0; i < n; ++i) dc::leaf_box(tri + 9 * i, box + 6 * i);
}

// box_entry of n (ray, box) pairs: o / d f64 [n,3] (world frame), box f32 [n,6], t_far f32 [n] -> tn f32 [n] (+inf: rejected)
void dc_host_ray_box_entry(const double* o, const double* d, const float* box, const float* t_far, int64_t n, float* tn) {
  for (int64_t i = 0; i < n; ++i) {
    dc::Ray64 r64;
    dc::Ray32 r32;
    dc::ray_setup(d[3 * i], d[3 * i + 1], d[3 * i + 2], o[3 * i], o[3 * i + 1], o[3 * i + 2], r64, r32);
    tn[i] = dc::box_entry(box + 6 * i, r32, t_far[i]);
  }
}

// the t_far the traversal prunes with once its best hit lies at t [n]
void dc_host_ray_prune_far(const double* t, int64_t n, float* t_far) {
  for (int64_t i = 0; i < n; ++i) t_far[i] = dc::prune_far(t[i]);
}

// The oracle of dc_raycast / dc_raycast_rays: test_triangle on every face of tri [F,9] in row order (face_id [F] the index each
// row reports, ascending for the tie rule to be the kernels'), no tree -> face i32 [R] (-1), t f64 [R] (inf), u / v f64 [R] (0).
void dc_host_ray_cast_brute(const double* tri, const int32_t* face_id, int64_t n_faces, const double* o, const double* d, const double* t_min,
                            int64_t n_rays, int cull, int32_t* face, double* t, double* u, double* v) {
  for (int64_t i = 0; i < n_rays; ++i) {
    dc::Ray64 r64;
    dc::Ray32 r32;
    dc::ray_setup(d[3 * i], d[3 * i + 1], d[3 * i + 2], o[3 * i], o[3 * i + 1], o[3 * i + 2], r64, r32);
    dc::Hit best = dc::no_hit();
    for (int64_t f = 0; f < n_faces; ++f) dc::test_triangle(tri + 9 * f, face_id[f], (int32_t)f, r64, t_min[i], cull != 0, best);
    face[i] = best.face;
    t[i] = best.t;
    u[i] = best.u;
    v[i] = best.v;
  }
}

// test_triangle pair by pair: ray i against triangle i (tri [n,9]) -> hit u8 [n], t / u / v f64 [n] (inf, 0, 0 without a hit)
void dc_host_ray_test_pairs(const double* tri, const double* o, const double* d, const double* t_min, int64_t n, int cull, uint8_t* hit,
                            double* t, double* u, double* v) {
  const int32_t zero = 0;
  for (int64_t i = 0; i < n; ++i) {
    int32_t f;
    dc_host_ray_cast_brute(tri + 9 * i, &zero, 1, o + 3 * i, d + 3 * i, t_min + i, 1, cull, &f, t + i, u + i, v + i);
    hit[i] = f == 0;
  }
}

// ---- the surfel ray caster's per-ray arithmetic (dc_surfelmath.h) -------------------------------------------------------------------
// leaf boxes of the disks (points / normals f64 [n,3], radii f64 [n]) -> box f32 [n,6], as surfel_fit_kernel writes them
void dc_host_surfel_boxes(const double* points, const double* normals, const double* radii, int64_t n, float* box) {
  for (int64_t i = 0; i < n; ++i) dc::disk_box(points + 3 * i, normals + 3 * i, radii[i], box + 6 * i);
}

// test_disk pair by pair: ray i (o / d f64 [n,3]) against row i of disk f64 [n,8] -> hit u8 [n], t / r2 f64 [n] as computed (whatever
// the verdict)
void dc_host_surfel_test_pairs(const double* disk, const double* o, const double* d, const double* t_min, int64_t n, uint8_t* hit, double* t,
                               double* r2) {
  for (int64_t i = 0; i < n; ++i) {
    const dc::SurfelRay r = {o[3 * i], o[3 * i + 1], o[3 * i + 2], d[3 * i], d[3 * i + 1], d[3 * i + 2]};
    hit[i] = dc::disk_hit(disk + dc::kDiskRow * i, r, t_min[i], t[i], r2[i]) ? 1 : 0;
  }
}

// The oracle of dc_surfel_cast_rays: both passes over every row of disk [n_disks,8] in row order (index [n_disks] the survey index each
// row reports, ascending for the tie rule to be the kernel's), no tree.
void dc_host_surfel_cast_brute(const double* disk, const int32_t* index, int64_t n_disks, const double* o, const double* d, int64_t n_rays,
                               double t_min, double window, double min_cos, int32_t* index_out, double* t_first_out, double* t_out,
                               double* inc_out, int32_t* count_out) {
  for (int64_t i = 0; i < n_rays; ++i) {
    const dc::SurfelRay r = {o[3 * i], o[3 * i + 1], o[3 * i + 2], d[3 * i], d[3 * i + 1], d[3 * i + 2]};
    dc::SurfelHit best = dc::no_surfel_hit();
    for (int64_t j = 0; j < n_disks; ++j) dc::test_disk(disk + dc::kDiskRow * j, index[j], (int32_t)j, r, t_min, best);
    dc::SurfelBlend blend;
    dc::blend_init(blend);
    const double* first = disk + dc::kDiskRow * (int64_t)(best.leaf >= 0 ? best.leaf : 0);
    if (best.leaf >= 0 && window > 0.0)
      for (int64_t j = 0; j < n_disks; ++j)
        dc::blend_disk(disk + dc::kDiskRow * j, j == best.leaf, first, r, t_min, best.t, best.t + window, min_cos, blend);
    index_out[i] = best.index;
    t_first_out[i] = best.t;
    dc::surfel_finish(best, first, blend, r, t_out[i], inc_out[i], count_out[i]);
  }
}

// ---- the one tree walk (dc_bvh.h) ----------------------------------------------------------------------------------------------------
// cast_ray on the host: bvh_walk (BLOCK = 1, lane 0) with the kernels' TriVisitor over a tree passed in as arrays (child i32 [n-1,2],
// node_box f32 [2n-1,6], leaf_tri f64 [n,9], leaf_face i32 [n]); outputs as dc_host_ray_cast_brute
void dc_host_ray_cast_walk(const int32_t* child, const float* node_box, const double* leaf_tri, const int32_t* leaf_face, int64_t n,
                           const double* o, const double* d, const double* t_min, int64_t n_rays, int cull, int32_t* face, double* t, double* u,
                           double* v) {
  int32_t stack[dc::kBvhStackDepth];
  for (int64_t i = 0; i < n_rays; ++i) {
    dc::TriVisitor vis = {node_box, leaf_tri, leaf_face, t_min[i], cull != 0};
    dc::ray_setup(d[3 * i], d[3 * i + 1], d[3 * i + 2], o[3 * i], o[3 * i + 1], o[3 * i + 2], vis.ray64, vis.ray);
    vis.best = dc::no_hit();
    dc::bvh_walk<1>(child, n, stack, 0, vis);
    face[i] = vis.best.face, t[i] = vis.best.t, u[i] = vis.best.u, v[i] = vis.best.v;
  }
}

// surfel_cast_kernel on the host: both walks with the kernel's DiskVisitor over a tree of disks (leaf_disk f64 [n,8], leaf_index i32 [n]);
// outputs as dc_host_surfel_cast_brute, the blend summed in the order of the walk
void dc_host_surfel_cast_walk(const int32_t* child, const float* node_box, const double* leaf_disk, const int32_t* leaf_index, int64_t n,
                              const double* o, const double* d, int64_t n_rays, double t_min, double window, double min_cos,
                              int32_t* index_out, double* t_first_out, double* t_out, double* inc_out, int32_t* count_out) {
  int32_t stack[dc::kBvhStackDepth];
  for (int64_t i = 0; i < n_rays; ++i) {
    const dc::SurfelRay r = {o[3 * i], o[3 * i + 1], o[3 * i + 2], d[3 * i], d[3 * i + 1], d[3 * i + 2]};
    dc::Ray64 ray64;
    dc::Ray32 ray;
    dc::ray_setup(r.d0, r.d1, r.d2, r.o0, r.o1, r.o2, ray64, ray);
    dc::SurfelHit best = dc::no_surfel_hit();
    dc::SurfelBlend blend;
    dc::blend_init(blend);
    dc::DiskVisitor<false> first = {node_box, leaf_disk, leaf_index, r, ray, t_min, 0.0, 0.0, best, blend};
    dc::bvh_walk<1>(child, n, stack, 0, first);
    if (best.leaf >= 0 && window > 0.0) {
      dc::DiskVisitor<true> rest = {node_box, leaf_disk, leaf_index, r, ray, t_min, best.t + window, min_cos, best, blend};
      dc::bvh_walk<1>(child, n, stack, 0, rest);
    }
    index_out[i] = best.index;
    t_first_out[i] = best.t;
    dc::surfel_finish(best, leaf_disk + dc::kDiskRow * (int64_t)(best.leaf >= 0 ? best.leaf : 0), blend, r, t_out[i], inc_out[i], count_out[i]);
  }
}

// acos01 of x [n], and the header's error counts (units of 2^-52) for k members
void dc_host_surfel_acos(const double* x, int64_t n, double* out) {
  for (int64_t i = 0; i < n; ++i) out[i] = dc::acos01(x[i]);
}
double dc_host_surfel_t_err(int k, double t, double t1) { return dc::surfel_t_err(k, t, t1); }
double dc_host_surfel_cos_err(int k, double kappa) { return dc::surfel_cos_err(k, kappa); }

// ---- plane neighbourhoods (dc_planemath.h) -------------------------------------------------------------------------------------------
namespace {
inline void host_load3(const void* p, int dtype, int64_t i, double* x) {
  if (dtype == DC_F32) dc::load3((const float*)p, i, x);
  else dc::load3((const double*)p, i, x);
}
inline double host_load1(const void* p, int dtype, int64_t i) { return dtype == DC_F32 ? (double)((const float*)p)[i] : ((const double*)p)[i]; }
// the kernels' fixed-order tree over the kPlaneBlock values of one block
inline double host_tree(double* sh) {
  for (int s = dc::kPlaneBlock / 2; s > 0; s >>= 1)
    for (int t = 0; t < s; ++t) sh[t] += sh[t + s];
  return sh[0];
}
}  // namespace

// the plane through p [9] (three points) -> pl [4]; returns 1 for a valid hypothesis
int dc_host_plane_from_points(const double* p, int distinct, double* pl) { return dc::plane_from_points(p, p + 3, p + 6, distinct != 0, pl) ? 1 : 0; }

// the inlier predicate of the plane pl [4] on x f64 [n,3] -> out u8 [n]
void dc_host_plane_inliers(const double* pl, const double* x, int64_t n, double thresh, uint8_t* out) {
  for (int64_t i = 0; i < n; ++i) out[i] = dc::plane_inlier(pl, x + 3 * i, thresh) ? 1 : 0;
}

// The oracle of dc_ransac_score: every hypothesis against every remaining point, no blocks, no LDS -> hyp [H,4], anchor [H,3],
// valid [H], counts [H] (-1 for a degenerate hypothesis), best [2].  0, or 1 for arguments dc_ransac_score refuses.
int dc_host_ransac_round(const void* points, int dtype, const int32_t* rem, int64_t n_rem, int64_t seed, int64_t round, int H, double thresh,
                         double* hyp, double* anchor, int32_t* valid, int32_t* counts, int32_t* best) {
  if (!points || !rem || !hyp || !anchor || !valid || !counts || !best) return 1;
  if (n_rem < 3 || n_rem > INT32_MAX || H < 1 || H > 1024 || !(thresh >= 0.0)) return 1;
  if (dtype != DC_F32 && dtype != DC_F64) return 1;
  int64_t key = INT64_MIN;
  for (int h = 0; h < H; ++h) {
    int64_t j[3];
    dc::ransac_draw((uint64_t)seed, round, h, n_rem, j);
    double p[3][3];
    for (int t = 0; t < 3; ++t) host_load3(points, dtype, (int64_t)rem[j[t]], p[t]);
    const bool ok = dc::plane_from_points(p[0], p[1], p[2], j[0] != j[1] && j[0] != j[2] && j[1] != j[2], hyp + 4 * h);
    for (int a = 0; a < 3; ++a) anchor[3 * h + a] = p[0][a];
    valid[h] = ok ? 1 : 0;
    int32_t c = 0;
    for (int64_t i = 0; i < n_rem; ++i) {
      double x[3];
      host_load3(points, dtype, (int64_t)rem[i], x);
      c += dc::plane_inlier(hyp + 4 * h, x, thresh) ? 1 : 0;
    }
    const int64_t k = dc::ransac_best_key(c, ok, H, h);
    counts[h] = ok ? c : -1;
    key = k > key ? k : key;
  }
  dc::ransac_best_decode(key, H, best);
  return 0;
}

// the blocks of dc_ransac_refit's moments kernel (dc_ransac_refit_partial_count of the product library)
int dc_host_ransac_refit_partial_count(int64_t n_rem) {
  const int64_t b = (n_rem + dc::kPlaneBlock - 1) / dc::kPlaneBlock;
  return (int)(b < 1 ? 1 : (b > dc::kRefitBlocksMax ? dc::kRefitBlocksMax : b));
}

// The oracle of dc_ransac_refit with the kernel's order of summation: every block's threads stride over the remaining points, the
// 256-thread tree, then the blocks in order -> totals [10] (optional), params [4], mask u8 [n_rem]
int dc_host_ransac_refit(const void* points, int dtype, const int32_t* rem, int64_t n_rem, const double* hyp, const double* anchor,
                         const int32_t* best, double thresh, double* totals, double* params, uint8_t* mask) {
  if (!points || !rem || !hyp || !anchor || !best || !params || !mask) return 1;
  if (n_rem < 1 || n_rem > INT32_MAX || !(thresh >= 0.0)) return 1;
  if (dtype != DC_F32 && dtype != DC_F64) return 1;
  const int nblk = dc_host_ransac_refit_partial_count(n_rem);
  const int h = best[0];
  const double* pl = hyp + 4 * h;
  const double* a = anchor + 3 * h;
  double tot[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  static thread_local double sh[10][dc::kPlaneBlock];
  for (int b = 0; b < nblk; ++b) {
    for (int t = 0; t < dc::kPlaneBlock; ++t) {
      double v[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
      for (int64_t i = (int64_t)b * dc::kPlaneBlock + t; i < n_rem; i += (int64_t)nblk * dc::kPlaneBlock) {
        double x[3];
        host_load3(points, dtype, (int64_t)rem[i], x);
        if (dc::plane_inlier(pl, x, thresh)) dc::refit_moments_add(x, a, v);
      }
      for (int k = 0; k < 10; ++k) sh[k][t] = v[k];
    }
    for (int k = 0; k < 10; ++k) tot[k] += host_tree(sh[k]);
  }
  if (totals)
    for (int k = 0; k < 10; ++k) totals[k] = tot[k];
  dc::plane_refit(tot, a, params);
  for (int64_t i = 0; i < n_rem; ++i) {
    double x[3];
    host_load3(points, dtype, (int64_t)rem[i], x);
    mask[i] = dc::plane_inlier(params, x, thresh) ? 1 : 0;
  }
  return 0;
}

// the refit's eigenvector step alone: C [6] (xx xy xz yy yz zz) -> nv [3], before the sign rule and the normalisation
void dc_host_smallest_eigvec_jacobi(const double* C, double* nv) { dc::smallest_eigvec_jacobi(C, nv); }

// plane_refit on ten given moments
void dc_host_plane_refit(const double* v, const double* anchor, double* params) { dc::plane_refit(v, anchor, params); }

// Sequential DBSCAN on the padded neighbour table nbr [m,K] (rows end with -1; a row holds the point itself): core = at least
// min_pts entries, union-find over the core-core edges in row order with the smaller root on top, so a component's label is its
// smallest index; a non-core point takes the smallest label among its core neighbours -> label [m] (-1 noise), best [2]
int dc_host_dbscan(const int32_t* nbr, int64_t m, int K, int min_pts, int32_t* label, int32_t* best) {
  if (!nbr || !label || !best || m < 1 || m > INT32_MAX || K < 1 || min_pts < 1) return 1;
  int32_t* par = new int32_t[m];
  int32_t* size = new int32_t[m];
  uint8_t* core = new uint8_t[m];
  for (int64_t i = 0; i < m; ++i) {
    int c = 0;
    for (int k = 0; k < K; ++k) c += nbr[i * K + k] >= 0;
    core[i] = c >= min_pts;
    par[i] = (int32_t)i;
    size[i] = 0;
  }
  auto find = [&](int32_t x) {
    while (par[x] != x) { par[x] = par[par[x]]; x = par[x]; }
    return x;
  };
  for (int64_t i = 0; i < m; ++i) {
    if (!core[i]) continue;
    for (int k = 0; k < K; ++k) {
      const int32_t j = nbr[i * K + k];
      if (j < 0) break;
      if (j == i || !core[j]) continue;
      const int32_t ri = find((int32_t)i), rj = find(j);
      if (ri != rj) par[ri > rj ? ri : rj] = ri > rj ? rj : ri;
    }
  }
  for (int64_t i = 0; i < m; ++i) {
    int32_t l = -1;
    if (core[i]) {
      l = find((int32_t)i);
    } else {
      for (int k = 0; k < K; ++k) {
        const int32_t j = nbr[i * K + k];
        if (j < 0) break;
        if (!core[j]) continue;
        const int32_t lj = find(j);
        if (l < 0 || lj < l) l = lj;
      }
    }
    label[i] = l;
    if (l >= 0) ++size[l];
  }
  best[0] = -1;
  best[1] = 0;
  for (int64_t l = 0; l < m; ++l)
    if (size[l] > best[1]) { best[0] = (int32_t)l; best[1] = size[l]; }
  delete[] par;
  delete[] size;
  delete[] core;
  return 0;
}

// model_eval and model_dw at (d, g): out [3 + n_terms] <- d', dd'/dd, dd'/dg, dd'/dw_k
void dc_host_plane_model(int kind, int n_terms, const double* w, const double* e, double d, double g, double* out) {
  dc::ModelParams mp;
  dc::load_model_params(kind, n_terms, w, e, mp);
  out[0] = dc::model_eval(mp, d, g, out + 1, out + 2);
  if (kind != DC_MODEL_NONE)
    for (int k = 0; k < n_terms; ++k) out[3 + k] = dc::model_dw(mp, k, d, g);
}

// dc_plane_moments_fwd for one plane: the rows idx [n] of the cloud (vps / dirs [N,3], depth [N], `dtype`), normal [3] -> cov [9],
// mean [3], x f64 [n,3] (optional: the corrected points).  The moments are summed in index order about the first point.
int dc_host_plane_moments_fwd(const void* vps, const void* dirs, const void* depth, int dtype, const int32_t* idx, int64_t n, const double* normal,
                              int kind, int n_terms, const double* w, const double* e, double* cov, double* mean, double* x_out) {
  if (!vps || !dirs || !depth || !idx || !normal || !cov || !mean || n < 1 || n_terms < 0 || n_terms > DC_MAX_MODEL_TERMS) return 1;
  if (kind < DC_MODEL_NONE || kind > DC_MODEL_LAST || (kind != DC_MODEL_NONE && !w)) return 1;
  dc::ModelParams mp;
  dc::load_model_params(kind, n_terms, w, e, mp);
  dc::PlanePoint q;
  double a[3], v[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int64_t r = 0; r < n; ++r) {
    if (dtype == DC_F32) dc::plane_point((const float*)vps, (const float*)dirs, (const float*)depth, (int64_t)idx[r], normal, mp, q);
    else dc::plane_point((const double*)vps, (const double*)dirs, (const double*)depth, (int64_t)idx[r], normal, mp, q);
    if (r == 0)
      for (int k = 0; k < 3; ++k) a[k] = q.x[k];
    dc::plane_moments_add(q.x, a, v);
    if (x_out)
      for (int k = 0; k < 3; ++k) x_out[3 * r + k] = q.x[k];
  }
  dc::plane_cov_finish(v, (double)n, a, cov, mean);
  return 0;
}

// dc_plane_moments_bwd for one plane: mean [3] of the forward, gcov [9] -> g_vps / g_dirs f64 [n,3], g_depth f64 [n] (per row of idx,
// before the rounding to the cloud's dtype), g_w [n_terms] (summed in index order)
int dc_host_plane_moments_bwd(const void* vps, const void* dirs, const void* depth, int dtype, const int32_t* idx, int64_t n, const double* normal,
                              int kind, int n_terms, const double* w, const double* e, const double* mean, const double* gcov, double* g_vps,
                              double* g_dirs, double* g_depth, double* g_w) {
  if (!vps || !dirs || !depth || !idx || !normal || !mean || !gcov || !g_vps || !g_dirs || !g_depth || n < 1) return 1;
  if (n_terms < 0 || n_terms > DC_MAX_MODEL_TERMS || (n_terms > 0 && !g_w)) return 1;
  if (kind < DC_MODEL_NONE || kind > DC_MODEL_LAST || (kind != DC_MODEL_NONE && !w)) return 1;
  dc::ModelParams mp;
  dc::load_model_params(kind, n_terms, w, e, mp);
  double M[3][3];
  dc::plane_bwd_matrix(gcov, (double)(n - 1), M);
  for (int k = 0; k < n_terms; ++k) g_w[k] = 0.0;
  dc::PlanePoint q;
  for (int64_t r = 0; r < n; ++r) {
    if (dtype == DC_F32) dc::plane_point((const float*)vps, (const float*)dirs, (const float*)depth, (int64_t)idx[r], normal, mp, q);
    else dc::plane_point((const double*)vps, (const double*)dirs, (const double*)depth, (int64_t)idx[r], normal, mp, q);
    const double gdp = dc::plane_bwd_point(q, normal, M, mean, kind, g_vps + 3 * r, g_dirs + 3 * r, g_depth + r);
    if (kind != DC_MODEL_NONE)
      for (int k = 0; k < n_terms; ++k) g_w[k] += gdp * dc::model_dw(mp, k, q.d, q.g);
  }
  return 0;
}

// ---- dynamic-point probabilities (dc_dynmath.h) --------------------------------------------------------------------------------------
// dc_dyn_directions on host arrays: the same loop over dyn_direction; pose NULL is the reading form
void dc_host_dyn_directions(const double* points, int64_t n, const double* pose, double max_range, double* dirs_out, double* depth_out,
                            uint8_t* valid_out) {
  for (int64_t i = 0; i < n; ++i) {
    double d[3], x[3];
    valid_out[i] = dc::dyn_direction(pose, points + 3 * i, max_range, d, x, depth_out + i, dirs_out + 3 * i) ? 1 : 0;
  }
}

// dc_dyn_update on host arrays: the same argument checks and the same per-entry function.  0, or DC_ERR_ARG.
int dc_host_dyn_update(const double* map_points, const double* map_normals, int64_t n_map, const double* pose, const double* reading, int64_t m,
                       const int32_t* rows, const int32_t* match_idx, const double* match_chord, int64_t n_rows, double chord_max,
                       double epsilon_a, double epsilon_d, double alpha, double beta, double threshold, double max_range, double* prob,
                       uint8_t* seen_out) {
  const dc::DynParams prm{chord_max, epsilon_a, epsilon_d, alpha, beta, threshold, max_range};
  if (n_rows < 0 || n_map < 0 || m < 0 || !dc::dyn_params_ok(prm)) return DC_ERR_ARG;
  if (n_rows == 0) return DC_OK;
  if (!map_points || !map_normals || !pose || !reading || !rows || !match_idx || !match_chord || !prob) return DC_ERR_ARG;
  for (int64_t i = 0; i < n_rows; ++i)
    dc::dyn_update_entry(prm, map_points, map_normals, n_map, pose, reading, m, (int64_t)rows[i], (int64_t)match_idx[i], match_chord[i], prob,
                         seen_out);
  return DC_OK;
}

// ---- range-image neighbourhoods (dc_rangeimage_math.h) -----------------------------------------------------------------------------
// range_pixel of sensor-frame points fp64 [n,3]: pixel_out int32 [n] (r W + c or -1), depth_out fp64 [n] (optional)
void dc_host_range_pixel(const double* points, int64_t n, int rows, int cols, double fov_up, double fov_down, int clamp, double min_depth,
                         int32_t* pixel_out, double* depth_out) {
  const dc::RangeGrid g{rows, cols, fov_up, fov_down, 1};
  for (int64_t i = 0; i < n; ++i) {
    double d;
    pixel_out[i] = dc::range_pixel(g, points[3 * i], points[3 * i + 1], points[3 * i + 2], clamp, min_depth, &d);
    if (depth_out) depth_out[i] = d;
  }
}

// the slot list of pixel (r, c): slots_out int32 [(2 ah + 1)(2 aw + 1)] in window order, -1 outside the image.  The number of slots, or
// DC_ERR_ARG for a window the grid does not admit.
int dc_host_image_window(int rows, int cols, int wrap, int r, int c, int ah, int aw, int32_t* slots_out) {
  const dc::RangeGrid g{rows, cols, 1.0, -1.0, wrap};
  if (!dc::range_grid_ok(g) || !dc::image_window_ok(g, ah, aw) || r < 0 || r >= rows || c < 0 || c >= cols) return DC_ERR_ARG;
  int slot = 0;
  for (int dr = -ah; dr <= ah; ++dr)
    for (int dc_ = -aw; dc_ <= aw; ++dc_) slots_out[slot++] = dc::image_window_pixel(g, r, c, dr, dc_);
  return slot;
}

// membership of one slot
int dc_host_image_member(int occupied, int centre, const double* xi, const double* xj, double r) {
  return dc::image_member(occupied != 0, centre != 0, xi, xj, r) ? 1 : 0;
}

// dc_range_project's winner rule as a host loop: the two passes in sequence (the minimum of the depth keys, then the lowest index among
// the points at the minimum).  points fp64 [n,3] in the sensor frame; pixel_out int32 [n], index_image int32 [H W], range_image fp64 [H W].
int dc_host_range_project(const double* points, int64_t n, int rows, int cols, double fov_up, double fov_down, int clamp, double min_depth,
                          int32_t* pixel_out, int32_t* index_image, double* range_image) {
  const dc::RangeGrid g{rows, cols, fov_up, fov_down, 1};
  if (!dc::range_grid_ok(g) || n < 0 || n >= (int64_t)0x7f000000) return DC_ERR_ARG;
  const int64_t hw = (int64_t)rows * cols;
  uint64_t* keys = new uint64_t[hw];
  for (int64_t p = 0; p < hw; ++p) { keys[p] = DC_RANGE_EMPTY_KEY; index_image[p] = 0x7f7f7f7f; }
  for (int64_t i = 0; i < n; ++i) {
    double d;
    const int32_t p = pixel_out[i] = dc::range_pixel(g, points[3 * i], points[3 * i + 1], points[3 * i + 2], clamp, min_depth, &d);
    if (p >= 0 && dc::range_depth_key(d) < keys[p]) keys[p] = dc::range_depth_key(d);
  }
  for (int64_t i = 0; i < n; ++i) {
    const int32_t p = pixel_out[i];
    if (p < 0) continue;
    const double d = dc::range_depth(points[3 * i], points[3 * i + 1], points[3 * i + 2]);
    if (dc::range_depth_key(d) == keys[p] && (int32_t)i < index_image[p]) index_image[p] = (int32_t)i;
  }
  for (int64_t p = 0; p < hw; ++p) {
    const bool empty = keys[p] == DC_RANGE_EMPTY_KEY;
    if (empty) index_image[p] = -1;
    if (range_image) range_image[p] = empty ? -1.0 : dc::range_key_depth(keys[p]);
  }
  delete[] keys;
  return DC_OK;
}

// ---- survey registration (dc_align_math.h; dc_align.hip's finish kernel) ----
// The closed-form fit from the totals tot [17] and the origins o [6]: T [16], lam [4] descending; 1 = the rotation is not unique
int dc_host_align_solve(const double* tot, const double* o, double* T, double* lam) { return dc::align_solve(tot, o, T, lam); }

// Angle of Ra Rb^T for two row-major 4 x 4 transforms (atan2 of the axial vector and the trace)
double dc_host_align_angle(const double* Ta, const double* Tb) { return dc::rotation_angle_between(Ta, 4, Tb, 4); }

// dc_align_finish on the host: the same argument checks, the partials summed in the kernel's order, the same tail; state
// [DC_ALIGN_STATE_COUNT], status [4] and history [n_history_rows, 5] (optional) are host arrays.  0, or 1 for refused arguments.
int dc_host_align_finish(const double* partials, int n_blocks, const double* origins, double min_rot, double min_trans, int min_pairs,
                         int max_iters, double* state, int32_t* status, double* history, int n_history_rows) {
  if (!partials || !origins || !state || !status || n_blocks < 1 || n_blocks > dc::kAlignBlocksMax) return 1;
  if (!(min_rot >= 0.0) || !(min_trans >= 0.0) || min_pairs < 3 || max_iters < 1 || n_history_rows < 0) return 1;
  if (status[0] != 0) return 0;
  double tot[DC_ALIGN_PARTIALS];
  for (int q = 0; q < DC_ALIGN_PARTIALS; ++q) tot[q] = dc::rows_sum<dc::kRowSumLanes>(partials, n_blocks, DC_ALIGN_PARTIALS, q);
  const dc::AlignParams prm{min_rot, min_trans, min_pairs, max_iters};
  const int row = status[1];
  double* hist = (history && row >= 0 && row < n_history_rows) ? history + (int64_t)row * DC_ALIGN_HISTORY_COLS : nullptr;
  dc::align_finish_tail(tot, origins, prm, state, status, hist);
  return 0;
}

// ---- global registration (dc_globalreg_math.h; dc_globalreg.hip) ----
// The pair feature: 1 and a [3], bins [3], *L for a valid pair, 0 otherwise
int dc_host_pair_feature(const double* xi, const double* ni, const double* xj, const double* nj, double* a, int32_t* bins, double* L) {
  const int ok = dc::greg_pair_feature(xi, ni, xj, nj, a, L);
  if (ok) for (int c = 0; c < 3; ++c) bins[c] = dc::greg_bin(a[c]);
  return ok;
}

float dc_host_feature_dist(const float* fq, const float* fs) { return dc::greg_feature_dist(fq, fs); }

int64_t dc_host_greg_draw(int64_t seed, int64_t h, int t, int64_t C) { return dc::greg_draw((uint64_t)seed, (uint64_t)h, t, C); }

int dc_host_greg_check_fit(const double* p, const double* y, const double* o, double min_edge, double rho, double* T, double* lam) {
  return dc::greg_check_fit(p, y, o, min_edge, rho, T, lam);
}

double dc_host_greg_residual2(const double* T, const double* p, const double* y) { return dc::greg_residual2(T, p, y); }

// dc_pair_spfh + dc_pair_fpfh on the host, point by point in the kernels' order: spfh double [n, 33] (scratch of the caller), m int32
// [n], feat float [n, 33], has int32 [n].  0, or 1 for refused arguments.
int dc_host_pair_histograms(const double* points, const double* normals, int64_t n, const int32_t* nbr, int k, double* spfh, int32_t* m,
                            float* feat, int32_t* has) {
  if (n < 0 || k < 1 || k > dc::kGregMaxK || (n > 0 && (!points || !normals || !nbr || !spfh || !m || !feat || !has))) return 1;
  for (int64_t i = 0; i < n; ++i) {
    int cnt[dc::kGregFeat] = {0};
    int mi = 0;
    for (int s = 0; s < k; ++s) {
      const int32_t j = nbr[i * k + s];
      double a[3], L;
      if (j < 0 || j >= n || !dc::greg_pair_feature(points + 3 * i, normals + 3 * i, points + 3 * (int64_t)j, normals + 3 * (int64_t)j, a, &L))
        continue;
      ++mi;
      for (int c = 0; c < 3; ++c) ++cnt[c * dc::kGregBins + dc::greg_bin(a[c])];
    }
    m[i] = mi;
    for (int b = 0; b < dc::kGregFeat; ++b) spfh[i * dc::kGregFeat + b] = mi > 0 ? (double)cnt[b] / (double)mi : 0.0;
  }
  for (int64_t i = 0; i < n; ++i) {
    double acc[dc::kGregFeat] = {0.0}, F[dc::kGregFeat];
    for (int s = 0; s < k; ++s) {
      const int32_t j = nbr[i * k + s];
      double a[3], L;
      if (j < 0 || j >= n || !dc::greg_pair_feature(points + 3 * i, normals + 3 * i, points + 3 * (int64_t)j, normals + 3 * (int64_t)j, a, &L))
        continue;
      for (int b = 0; b < dc::kGregFeat; ++b) acc[b] = dc::greg_fpfh_term(acc[b], L, spfh[(int64_t)j * dc::kGregFeat + b]);
    }
    for (int b = 0; b < dc::kGregFeat; ++b) F[b] = m[i] > 0 ? dc::greg_fpfh_value(spfh[i * dc::kGregFeat + b], m[i], acc[b]) : 0.0;
    for (int c = 0; c < 3; ++c) {
      double sum = 0.0;
      for (int b = 0; b < dc::kGregBins; ++b) sum += F[c * dc::kGregBins + b];
      const double scale = dc::greg_block_scale(sum);
      for (int b = 0; b < dc::kGregBins; ++b) feat[i * dc::kGregFeat + c * dc::kGregBins + b] = (float)(F[c * dc::kGregBins + b] * scale);
    }
    has[i] = m[i] > 0 ? 1 : 0;
  }
  return 0;
}

// ---- plane registration (dc_planereg_math.h; dc_planereg.hip) ----
// The enumeration of [h_begin, h_end) done sequentially: the valid hypotheses in ascending h; the first `cap` of them are written to
// h_out [cap], T_out [cap, 16] and score_out [cap] (any of them may be null).  Returns their number, or -1 for refused arguments
// (the kernels' DC_ERR_ARG cases: plane counts, tolerances, more than 41 664 triples, the range).
int64_t dc_host_planereg_enumerate(const double* cp, const int64_t* cs, int pc, const double* sp, int ps, const int32_t* tri, int64_t n_tri,
                                   int64_t h_begin, int64_t h_end, double min_det, double tol_dot, double cos_tol, double tol_d,
                                   int64_t cap, int64_t* h_out, double* T_out, int64_t* score_out) {
  const dc::PregParams prm{min_det, tol_dot, cos_tol, tol_d};
  if (!dc::preg_args_ok(pc, ps, prm) || n_tri < 0 || n_tri > dc::kPregMaxTriples || h_begin < 0 || h_end < h_begin || h_end > n_tri * ps * ps * ps * 8) return -1;
  int64_t n = 0;
  for (int64_t h = h_begin; h < h_end; ++h) {
    double T[16];
    int64_t score = 0;
    if (!dc::preg_hypothesis(h, cp, cs, pc, sp, ps, tri, prm, T, &score)) continue;
    if (n < cap) {
      if (h_out) h_out[n] = h;
      if (score_out) score_out[n] = score;
      if (T_out) for (int c = 0; c < 16; ++c) T_out[n * 16 + c] = T[c];
    }
    ++n;
  }
  return n;
}

// The score of one transform T [16] over the plane tables
int64_t dc_host_planereg_score(const double* T, const double* cp, const int64_t* cs, int pc, const double* sp, int ps, double cos_tol,
                               double tol_d) {
  return dc::preg_score(T, cp, cs, pc, sp, ps, cos_tol, tol_d);
}

// Rules 2 to 4 and the fit of one pairing (rows of 4): 1 and T [16] when valid
int dc_host_planereg_pair(const double* na, const double* nb, const double* nc, const double* mi, const double* mj, const double* mk, int s,
                          double min_det, double tol_dot, double* T) {
  if (!dc::preg_check(na, nb, nc, mi, mj, mk, s, min_det, tol_dot)) return 0;
  return dc::preg_fit(na, nb, nc, mi, mj, mk, s, T);
}

// ---- surface reconstruction (dc_tsdf_math.h; dc_tsdf.hip) ----
// dc_tsdf_integrate over a list of rays into host arrays, ray after ray: vps / dirs [n,3], depth [n] of `dtype`, mask uint8 [n] or null,
// pose [16] or null, og [3]; sum int64 [V], count int32 [V] and stats int64 [4] are added to.  Returns the kernels' status.
int dc_host_tsdf_integrate(const void* vps, const void* dirs, const void* depth, int dtype, int64_t n, const uint8_t* mask, const double* pose,
                           const double* og, double voxel, int nx, int ny, int nz, double trunc, int k_steps, double min_depth,
                           double max_range, double carve_from, int64_t* sum, int32_t* count, int64_t* stats) {
  const dc::TsdfGrid g{{og[0], og[1], og[2]}, voxel, {nx, ny, nz}};
  const dc::TsdfRule r{trunc, voxel / 2.0, min_depth, max_range, carve_from, k_steps};
  if (!dc::tsdf_grid_ok(g) || !dc::tsdf_rule_ok(r) || n < 0) return DC_ERR_ARG;
  if (dtype != DC_F32 && dtype != DC_F64) return DC_ERR_DTYPE;
  dc::TsdfTally t{0, 0, 0, 0};
  for (int64_t i = 0; i < n; ++i) {
    double vp[3], dir[3], d;
    for (int a = 0; a < 3; ++a) {
      vp[a] = dtype == DC_F32 ? (double)((const float*)vps)[3 * i + a] : ((const double*)vps)[3 * i + a];
      dir[a] = dtype == DC_F32 ? (double)((const float*)dirs)[3 * i + a] : ((const double*)dirs)[3 * i + a];
    }
    d = dtype == DC_F32 ? (double)((const float*)depth)[i] : ((const double*)depth)[i];
    dc::tsdf_ray(vp, dir, d, mask ? mask[i] != 0 : true, pose, g, r, &t, [&](int64_t v, int64_t q) { sum[v] += q; count[v] += 1; });
  }
  stats[0] += t.used; stats[1] += t.skipped; stats[2] += t.outside; stats[3] += t.visits;
  return DC_OK;
}

// dc_tsdf_extract_count + _fill on host arrays, done sequentially: totals [2] <- {vertices, faces}; the first cap_v vertices go to
// vertices [cap_v,3] and the first cap_f faces to faces [cap_f,3] (either may be null).  Returns the kernels' status.
int dc_host_tsdf_extract(const int64_t* sum, const int32_t* count, const double* og, double voxel, int nx, int ny, int nz, int min_count,
                         int64_t cap_v, int64_t cap_f, double* vertices, int32_t* faces, int64_t* totals) {
  const dc::TsdfGrid g{{og[0], og[1], og[2]}, voxel, {nx, ny, nz}};
  if (!dc::tsdf_grid_ok(g) || min_count < 1) return DC_ERR_ARG;
  const int64_t n_cells = dc::tsdf_cell_count(nx, ny, nz);
  std::vector<int32_t> id((size_t)n_cells, -1);
  int64_t nv = 0, nf = 0;
  for (int x = 0; x < nx - 1; ++x)
    for (int y = 0; y < ny - 1; ++y)
      for (int z = 0; z < nz - 1; ++z) {
        int64_t corner[8];
        int bits;
        if (!dc::tsdf_cell_active(sum, count, g, min_count, x, y, z, corner, &bits)) continue;
        if (vertices && nv < cap_v) dc::tsdf_cell_vertex(sum, count, g, x, y, z, corner, bits, vertices + 3 * nv);
        id[(size_t)dc::tsdf_cell_index(g, x, y, z)] = (int32_t)nv++;
      }
  for (int x = 0; x < nx; ++x)
    for (int y = 0; y < ny; ++y)
      for (int z = 0; z < nz; ++z)
        for (int e = 0; e < 3; ++e) {
          bool in;
          int64_t cells[4];
          if (!dc::tsdf_edge_crosses(sum, count, g, min_count, x, y, z, e, &in) || !dc::tsdf_edge_cells(g, x, y, z, e, cells)) continue;
          const int32_t q[4] = {id[(size_t)cells[in ? 0 : 3]], id[(size_t)cells[in ? 1 : 2]], id[(size_t)cells[in ? 2 : 1]], id[(size_t)cells[in ? 3 : 0]]};
          if (q[0] < 0 || q[1] < 0 || q[2] < 0 || q[3] < 0) continue;
          if (faces && nf + 1 < cap_f) {
            int32_t* o = faces + 3 * nf;
            o[0] = q[0]; o[1] = q[1]; o[2] = q[2];
            o[3] = q[0]; o[4] = q[2]; o[5] = q[3];
          }
          nf += 2;
        }
  totals[0] = nv;
  totals[1] = nf;
  return DC_OK;
}

// ---- sparse TSDF volumes (dc_tsdf_sparse_math.h; dc_tsdf_sparse.hip) ----
namespace {
struct HostRays {
  const void *vps, *dirs, *depth;
  int dtype;
  const uint8_t* mask;
  void load(int64_t i, double* vp, double* dir, double* d, bool* in) const {
    for (int a = 0; a < 3; ++a) {
      vp[a] = dtype == DC_F32 ? (double)((const float*)vps)[3 * i + a] : ((const double*)vps)[3 * i + a];
      dir[a] = dtype == DC_F32 ? (double)((const float*)dirs)[3 * i + a] : ((const double*)dirs)[3 * i + a];
    }
    *d = dtype == DC_F32 ? (double)((const float*)depth)[i] : ((const double*)depth)[i];
    *in = mask ? mask[i] != 0 : true;
  }
};
bool host_sparse_rule(const double* og, double voxel, double trunc, int k_steps, double min_depth, double max_range, int64_t capacity,
                      dc::TsdfGrid* g, dc::TsdfRule* r) {
  *g = dc::TsdfGrid{{og[0], og[1], og[2]}, voxel, {0, 0, 0}};
  *r = dc::TsdfRule{trunc, voxel / 2.0, min_depth, max_range, -1.0, k_steps};
  return dc::tsdf_lattice_ok(*g) && dc::tsdf_rule_ok(*r) && capacity >= 1 && capacity < ((int64_t)1 << 22);
}
}  // namespace

// dc_tsdf_sparse_allocate on host arrays, ray after ray: keys uint64 [capacity], slots int32 [capacity], n_blocks int64 [1], info int64 [2].
// max_ray_blocks (or null) <- the most distinct wanted blocks any one ray met, table or not: what the candidate buffer's share must hold.
int dc_host_tsdf_sparse_allocate(const void* vps, const void* dirs, const void* depth, int dtype, int64_t n, const uint8_t* mask,
                                 const double* pose, const double* og, double voxel, double trunc, int k_steps, double min_depth,
                                 double max_range, int64_t capacity, uint64_t* keys, int32_t* slots, int64_t* n_blocks, int64_t* info,
                                 int64_t* max_ray_blocks) {
  dc::TsdfGrid g;
  dc::TsdfRule r;
  if (!host_sparse_rule(og, voxel, trunc, k_steps, min_depth, max_range, capacity, &g, &r) || n < 0) return DC_ERR_ARG;
  if (dtype != DC_F32 && dtype != DC_F64) return DC_ERR_DTYPE;
  const int64_t nb = *n_blocks < 0 ? 0 : (*n_blocks > capacity ? capacity : *n_blocks);
  const HostRays rays{vps, dirs, depth, dtype, mask};
  std::vector<uint64_t> cand;
  int64_t most = 0;
  for (int64_t i = 0; i < n; ++i) {
    double vp[3], dir[3], d;
    bool in;
    rays.load(i, vp, dir, &d, &in);
    dc::TsdfTally t{0, 0, 0, 0};
    std::vector<uint64_t> mine;
    dc::tsdf_ray_walk(vp, dir, d, in, pose, dc::TsdfSparseAddress{g}, r, &t, [&](const dc::TsdfSparseAddress::Voxel& x, int64_t) {
      const uint64_t key = dc::tsdf_voxel_key(x.i);
      if (std::find(mine.begin(), mine.end(), key) == mine.end()) mine.push_back(key);
      if (dc::tsdf_table_find(keys, nb, key) < 0) cand.push_back(key);
    });
    most = std::max<int64_t>(most, (int64_t)mine.size());
  }
  std::sort(cand.begin(), cand.end());
  cand.erase(std::unique(cand.begin(), cand.end()), cand.end());
  const int64_t wanted = (int64_t)cand.size(), admitted = std::min<int64_t>(wanted, capacity - nb);
  std::vector<std::pair<uint64_t, int32_t>> table;
  for (int64_t t = 0; t < nb; ++t) table.emplace_back(keys[t], slots[t]);
  for (int64_t t = 0; t < admitted; ++t) table.emplace_back(cand[(size_t)t], (int32_t)(nb + t));
  std::sort(table.begin(), table.end());
  for (size_t t = 0; t < table.size(); ++t) { keys[t] = table[t].first; slots[t] = table[t].second; }
  *n_blocks = nb + admitted;
  info[0] = nb + admitted;
  info[1] = wanted - admitted;
  if (max_ray_blocks) *max_ray_blocks = most;
  return DC_OK;
}

// dc_tsdf_sparse_integrate on host arrays: sum int64 [capacity,512], count int32 [capacity,512] and stats int64 [5] are added to.
int dc_host_tsdf_sparse_integrate(const void* vps, const void* dirs, const void* depth, int dtype, int64_t n, const uint8_t* mask,
                                  const double* pose, const double* og, double voxel, double trunc, int k_steps, double min_depth,
                                  double max_range, int64_t capacity, const uint64_t* keys, const int32_t* slots, const int64_t* n_blocks,
                                  int64_t* sum, int32_t* count, int64_t* stats) {
  dc::TsdfGrid g;
  dc::TsdfRule r;
  if (!host_sparse_rule(og, voxel, trunc, k_steps, min_depth, max_range, capacity, &g, &r) || n < 0) return DC_ERR_ARG;
  if (dtype != DC_F32 && dtype != DC_F64) return DC_ERR_DTYPE;
  const int64_t nb = *n_blocks < 0 ? 0 : (*n_blocks > capacity ? capacity : *n_blocks);
  const HostRays rays{vps, dirs, depth, dtype, mask};
  dc::TsdfTally t{0, 0, 0, 0};
  int64_t dropped = 0;
  for (int64_t i = 0; i < n; ++i) {
    double vp[3], dir[3], d;
    bool in;
    rays.load(i, vp, dir, &d, &in);
    dc::TsdfBlockCache cache{dc::kTsdfNoKey, -1};
    dc::tsdf_ray_walk(vp, dir, d, in, pose, dc::TsdfSparseAddress{g}, r, &t, [&](const dc::TsdfSparseAddress::Voxel& x, int64_t q) {
      const int64_t pos = dc::tsdf_cached_find(keys, nb, dc::tsdf_voxel_key(x.i), &cache);
      const int64_t slot = pos < 0 ? -1 : (int64_t)slots[pos];
      if (slot < 0 || slot >= capacity) { ++dropped; return; }
      const int64_t v = slot * dc::kTsdfBlockVoxels + dc::tsdf_voxel_local(x.i);
      sum[v] += q;
      count[v] += 1;
    });
  }
  stats[0] += t.used; stats[1] += t.skipped; stats[2] += t.outside; stats[3] += t.visits; stats[4] += dropped;
  return DC_OK;
}

// dc_tsdf_sparse_extract_count + _fill on host arrays, block after block in key order; outputs as dc_host_tsdf_extract.
int dc_host_tsdf_sparse_extract(const uint64_t* keys, const int32_t* slots, int64_t n_blocks, const int64_t* sum, const int32_t* count,
                                const double* og, double voxel, int min_count, int64_t cap_v, int64_t cap_f, double* vertices, int32_t* faces,
                                int64_t* totals) {
  const dc::TsdfGrid g{{og[0], og[1], og[2]}, voxel, {0, 0, 0}};
  if (!dc::tsdf_lattice_ok(g) || min_count < 1 || n_blocks < 0) return DC_ERR_ARG;
  if (n_blocks * dc::kTsdfBlockVoxels * 3 >= ((int64_t)1 << 31)) return DC_ERR_UNSUPPORTED;
  std::vector<int32_t> nbr((size_t)n_blocks * 27), id((size_t)n_blocks * dc::kTsdfBlockVoxels, -1);
  for (int64_t t = 0; t < n_blocks * 27; ++t) nbr[(size_t)t] = dc::tsdf_block_neighbour(keys, n_blocks, t / 27, (int)(t % 27));
  int64_t nv = 0, nf = 0;
  for (int64_t p = 0; p < n_blocks; ++p) {
    int b[3];
    dc::tsdf_block_of_key(keys[p], b);
    for (int lx = 0; lx < 8; ++lx)
      for (int ly = 0; ly < 8; ++ly)
        for (int lz = 0; lz < 8; ++lz) {
          int64_t corner[8];
          int bits;
          if (!dc::tsdf_sparse_cell_active(sum, count, nbr.data() + 27 * p, slots, min_count, lx, ly, lz, corner, &bits)) continue;
          if (vertices && nv < cap_v)
            dc::tsdf_cell_vertex(sum, count, g, 8 * b[0] + lx, 8 * b[1] + ly, 8 * b[2] + lz, corner, bits, vertices + 3 * nv);
          id[(size_t)(p * dc::kTsdfBlockVoxels + (lx * 8 + ly) * 8 + lz)] = (int32_t)nv++;
        }
  }
  for (int64_t p = 0; p < n_blocks; ++p)
    for (int lx = 0; lx < 8; ++lx)
      for (int ly = 0; ly < 8; ++ly)
        for (int lz = 0; lz < 8; ++lz)
          for (int e = 0; e < 3; ++e) {
            bool in;
            int64_t cells[4];
            const int32_t* nb27 = nbr.data() + 27 * p;
            if (!dc::tsdf_sparse_edge_crosses(sum, count, nb27, slots, min_count, lx, ly, lz, e, &in) ||
                !dc::tsdf_sparse_edge_cells(nb27, lx, ly, lz, e, cells))
              continue;
            const int32_t q[4] = {id[(size_t)cells[in ? 0 : 3]], id[(size_t)cells[in ? 1 : 2]], id[(size_t)cells[in ? 2 : 1]], id[(size_t)cells[in ? 3 : 0]]};
            if (q[0] < 0 || q[1] < 0 || q[2] < 0 || q[3] < 0) continue;
            if (faces && nf + 1 < cap_f) {
              int32_t* o = faces + 3 * nf;
              o[0] = q[0]; o[1] = q[1]; o[2] = q[2];
              o[3] = q[0]; o[4] = q[2]; o[5] = q[3];
            }
            nf += 2;
          }
  totals[0] = nv;
  totals[1] = nf;
  return DC_OK;
}

// ---- scan-to-TSDF registration (dc_tsdf_track_math.h; dc_tsdf_track.hip) ----
// dc_tsdf_sparse_sample on host arrays, point after point; stop (or null) as the kernel reads it.
int dc_host_tsdf_sparse_sample(const uint64_t* keys, const int32_t* slots, const int64_t* n_blocks, int64_t capacity, const int64_t* sum,
                               const int32_t* count, const double* og, double voxel, double trunc, int min_count, const double* points, int64_t m,
                               const double* pose, const int32_t* stop, double* x_out, double* value_out, double* grad_out, double* dist_out,
                               uint8_t* flag_out) {
  const dc::TsdfGrid g{{og[0], og[1], og[2]}, voxel, {0, 0, 0}};
  if (!dc::tsdf_lattice_ok(g) || !(trunc > 0.0) || !std::isfinite(trunc) || min_count < 1 || m < 0 || capacity < 1 ||
      capacity >= ((int64_t)1 << 22))
    return DC_ERR_ARG;
  if (stop && *stop != 0) return DC_OK;
  const int64_t nb = *n_blocks < 0 ? 0 : (*n_blocks > capacity ? capacity : *n_blocks);
  for (int64_t i = 0; i < m; ++i) {
    double x[3] = {points[3 * i], points[3 * i + 1], points[3 * i + 2]};
    if (pose) dc::move_point(pose, points + 3 * i, x);
    const dc::TsdfSample s = dc::tsdf_sample_point(x, g, trunc, min_count, keys, slots, nb, capacity, sum, count);
    for (int a = 0; a < 3; ++a) { x_out[3 * i + a] = x[a]; grad_out[3 * i + a] = s.grad[a]; }
    value_out[i] = s.phi;
    dist_out[i] = s.dist;
    flag_out[i] = (uint8_t)s.flag;
  }
  return DC_OK;
}

// dc_tsdf_icp_accumulate on host arrays: the pair rule and the 30 sums, added point after point into ONE row (row [DC_ICP_PARTIALS]).
int dc_host_tsdf_icp_accumulate(const double* x, const double* value, const double* grad, const double* dist, const uint8_t* flag, int64_t m,
                                const double* threshold, double max_residual, const int32_t* status, double* row, uint8_t* kept_out) {
  if (m < 0 || !threshold || !status || !row || std::isnan(max_residual)) return DC_ERR_ARG;
  if (status[0] != 0) return DC_OK;
  for (int q = 0; q < DC_ICP_PARTIALS; ++q) row[q] = 0.0;
  for (int64_t i = 0; i < m; ++i) {
    const bool keep = dc::tsdf_track_keep(flag[i], dist[i], *threshold, max_residual);
    if (kept_out) kept_out[i] = keep ? 1 : 0;
    if (!keep) continue;
    dc::tsdf_track_add(x + 3 * i, value[i], grad + 3 * i, row);
    row[dc::IcpRow<6>::kUsed] += 1.0;
  }
  return DC_OK;
}

// ---- self-supervised training against the fused volume (dc_tsdf_loss_math.h; dc_tsdf_loss.hip) ----
// The sample with exclusion and the term at one world point x [3]: own_keys (or null) is ONE scan's segment of own_nb keys.  Returns the
// class (0 used, 1 invalid, 2 unobserved, 3 gated); *phi, grad [3] the sample, *l and dl_dx [3] the term (0 unless used).
int dc_host_tsdf_loss_point(const uint64_t* keys, const int32_t* slots, int64_t nb, int64_t capacity, const int64_t* sum, const int32_t* count,
                            const uint64_t* own_keys, const int32_t* own_slots, int64_t own_nb, int64_t own_capacity, const int64_t* own_sum,
                            const int32_t* own_count, const double* og, double voxel, double trunc, int min_count, const double* x, int squared,
                            double max_residual, double* phi, double* grad, double* l, double* dl_dx) {
  const dc::TsdfGrid g{{og[0], og[1], og[2]}, voxel, {0, 0, 0}};
  const dc::TsdfTable total{keys, slots, nb < 0 ? 0 : (nb > capacity ? capacity : nb), capacity, sum, count};
  const dc::TsdfTable own{own_keys, own_slots, own_nb, own_capacity, own_sum, own_count};
  const dc::TsdfSample s = dc::tsdf_sample_point_minus(x, g, trunc, min_count, total, own);
  const int cls = dc::tsdf_loss_class(s, max_residual);
  *phi = s.phi;
  for (int a = 0; a < 3; ++a) { grad[a] = s.grad[a]; dl_dx[a] = 0.0; }
  *l = 0.0;
  if (cls == dc::kTsdfLossUsed) *l = dc::tsdf_loss_term(s.phi, s.grad, squared != 0, dl_dx);
  return cls;
}

// dc_tsdf_loss on host arrays with plain loops, point after point in index order (NOT the kernel's summation order: the tests compare
// it with the extended-precision oracle within the derived bound).  The arguments and the outputs are those of dc_tsdf_loss.
int dc_host_tsdf_loss(const uint64_t* keys, const int32_t* slots, const int64_t* n_blocks, int64_t capacity, const int64_t* sum,
                      const int32_t* count, const uint64_t* own_keys, const int32_t* own_slots, const int64_t* own_ptr, int64_t n_own_keys,
                      int64_t own_capacity, const int64_t* own_sum, const int32_t* own_count, const double* og, double voxel, double trunc,
                      int min_count, const void* vps, const void* dirs, const void* depth, const void* inc, const uint8_t* lmask,
                      const uint8_t* mask, int dtype, int64_t n, const int64_t* scan_ptr, const double* poses, int n_scans, int model_kind,
                      int n_terms, const double* w, const double* e, int want_exponent, int squared, double max_residual, double* value_out,
                      uint8_t* flag_out, double* x_out, double* out) {
  const dc::TsdfGrid g{{og[0], og[1], og[2]}, voxel, {0, 0, 0}};
  if (n < 0 || n_scans < 0 || !out || !keys || !slots || !n_blocks || !sum || !count) return DC_ERR_ARG;
  if (dtype != DC_F32 && dtype != DC_F64) return DC_ERR_DTYPE;
  if (!dc::tsdf_lattice_ok(g) || !(trunc > 0.0) || !std::isfinite(trunc) || min_count < 1 || capacity < 1 || capacity >= ((int64_t)1 << 22) ||
      std::isnan(max_residual))
    return DC_ERR_ARG;
  if (own_keys && (!own_slots || !own_ptr || !own_sum || !own_count || n_own_keys < 0 || own_capacity < 1)) return DC_ERR_ARG;
  if (model_kind < DC_MODEL_NONE || model_kind > DC_MODEL_LAST) return DC_ERR_ARG;
  if (model_kind == DC_MODEL_NONE) n_terms = 0;
  else if (n_terms < 1 || n_terms > DC_MAX_MODEL_TERMS || !w || !e || (n > 0 && !inc)) return DC_ERR_ARG;
  if (n > 0 && (n_scans < 1 || !dirs || !depth)) return DC_ERR_ARG;
  if (n_scans > 1 && !scan_ptr) return DC_ERR_ARG;
  dc::ModelParams mp;
  mp.kind = model_kind;
  mp.n_terms = n_terms;
  for (int k = 0; k < DC_MAX_MODEL_TERMS; ++k) { mp.w[k] = k < n_terms ? w[k] : 0.0; mp.e[k] = k < n_terms ? e[k] : 0.0; }
  const int nt = n_terms, o_grad = 5 + 2 * nt;
  for (int q = 0; q < o_grad + 12 * n_scans; ++q) out[q] = 0.0;
  const int64_t nb = *n_blocks < 0 ? 0 : (*n_blocks > capacity ? capacity : *n_blocks);
  const dc::TsdfTable total{keys, slots, nb, capacity, sum, count};
  const double nan = std::nan("");
  for (int s = 0; s < n_scans; ++s) {
    int64_t a = scan_ptr ? scan_ptr[s] : 0, b = scan_ptr ? scan_ptr[s + 1] : n;
    a = a < 0 ? 0 : (a > n ? n : a);
    b = b < a ? a : (b > n ? n : b);
    dc::TsdfTable own{nullptr, nullptr, 0, own_capacity, own_sum, own_count};
    if (own_keys) {
      int64_t oa = own_ptr[s], ob = own_ptr[s + 1];
      oa = oa < 0 ? 0 : (oa > n_own_keys ? n_own_keys : oa);
      ob = ob < oa ? oa : (ob > n_own_keys ? n_own_keys : ob);
      own.keys = own_keys + oa; own.slots = own_slots + oa; own.nb = ob - oa;
    }
    double T12[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    if (poses) for (int q = 0; q < 12; ++q) T12[q] = poses[(int64_t)s * 12 + q];
    double* gT = out + o_grad + (int64_t)s * 12;
    for (int64_t j = a; j < b; ++j) {
      double x[3] = {nan, nan, nan}, value = nan;
      int cls = dc::kTsdfLossMasked;
      if (mask ? mask[j] != 0 : true) {
        double vp[3] = {0.0, 0.0, 0.0}, dr[3], vr[3], drr[3];
        if (vps) host_load3(vps, dtype, j, vp);
        host_load3(dirs, dtype, j, dr);
        const double d = host_load1(depth, dtype, j);
        const bool lm = lmask ? lmask[j] != 0 : true;
        const double ia = model_kind != DC_MODEL_NONE ? host_load1(inc, dtype, j) : 0.0;
        const double dcorr = dc::model_depth(mp, d, lm ? ia : 0.0, lm);
        dc::rot3(T12, vp, vr);
        dc::rot3(T12, dr, drr);
        for (int c = 0; c < 3; ++c) x[c] = (vr[c] + T12[4 * c + 3]) + dcorr * drr[c];
        const dc::TsdfSample sm = dc::tsdf_sample_point_minus(x, g, trunc, min_count, total, own);
        cls = dc::tsdf_loss_class(sm, max_residual);
        if (sm.flag == 0) value = sm.phi;
        if (cls == dc::kTsdfLossUsed) {
          double gx[3];
          out[0] += dc::tsdf_loss_term(sm.phi, sm.grad, squared != 0, gx);
          out[1] += 1.0;
          // dL/dd' = dir . (R^T g)
          double gd = 0.0;
          for (int c = 0; c < 3; ++c) gd += dr[c] * (T12[c] * gx[0] + T12[4 + c] * gx[1] + T12[8 + c] * gx[2]);
          if (model_kind > DC_MODEL_SCALED_POLYNOMIAL && lm) {
            for (int k = 0; k < nt && k < 3; ++k) out[5 + k] += gd * dc::model_dw_other(mp, k, d, ia);
          } else if (model_kind != DC_MODEL_NONE && lm) {
            const double base = model_kind == DC_MODEL_SCALED_POLYNOMIAL ? -d * gd : -gd;
            for (int k = 0; k < nt; ++k) {
              const double pk = dc::pow_term(ia, mp.e[k]);
              out[5 + k] += base * pk;
              if (want_exponent) out[5 + nt + k] += ia > 0.0 ? base * mp.w[k] * pk * std::log(ia) : 0.0;
            }
          }
          const double xl[4] = {vp[0] + dcorr * dr[0], vp[1] + dcorr * dr[1], vp[2] + dcorr * dr[2], 1.0};
          for (int q = 0; q < 12; ++q) gT[q] += gx[q >> 2] * xl[q & 3];
        } else {
          out[cls == dc::kTsdfLossGated ? 2 : (cls == dc::kTsdfLossUnobserved ? 3 : 4)] += 1.0;
        }
      }
      if (value_out) value_out[j] = value;
      if (flag_out) flag_out[j] = (uint8_t)cls;
      if (x_out) for (int c = 0; c < 3; ++c) x_out[3 * j + c] = x[c];
    }
  }
  const double M = out[1];
  out[0] = M > 0.0 ? out[0] / M : nan;
  for (int q = 5; q < o_grad + 12 * n_scans; ++q) out[q] = M > 0.0 ? out[q] / M : 0.0;
  return DC_OK;
}

// ---- ray casting the fused volume (dc_tsdf_cast_math.h; dc_tsdf_cast.hip) ----
// dc_tsdf_sparse_cast_rays on host arrays, ray after ray: the arguments and the outputs are those of the device call.
int dc_host_tsdf_sparse_cast_rays(const uint64_t* keys, const int32_t* slots, const int64_t* n_blocks, int64_t capacity, const int64_t* sum,
                                  const int32_t* count, const uint64_t* own_keys, const int32_t* own_slots, const int64_t* own_ptr,
                                  int64_t n_own_keys, int64_t own_capacity, const int64_t* own_sum, const int32_t* own_count, const double* og,
                                  double voxel, double trunc, int min_count, const void* vps, const void* dirs, const uint8_t* mask, int dtype,
                                  int64_t n, const int64_t* scan_offset, const double* poses, int n_scans, double t_min, double t_max,
                                  double step, int refine, int skip, int32_t* face_out, double* t_out, double* inc_out, double* normal_out,
                                  double* phi_out, uint8_t* status_out, int32_t* samples_out) {
  const dc::TsdfGrid g{{og[0], og[1], og[2]}, voxel, {0, 0, 0}};
  if (dtype != DC_F32 && dtype != DC_F64) return DC_ERR_DTYPE;
  if (!dc::tsdf_lattice_ok(g) || !(trunc > 0.0) || !std::isfinite(trunc) || min_count < 1 || n < 0 || capacity < 1 ||
      capacity >= ((int64_t)1 << 22) || refine < 0)
    return DC_ERR_ARG;
  const int J = dc::tsdf_cast_steps(t_min, t_max, step, trunc);
  if (J < 0) return DC_ERR_ARG;
  if (own_keys && (!own_slots || !own_ptr || !own_sum || !own_count || n_own_keys < 0 || own_capacity < 1)) return DC_ERR_ARG;
  if (n == 0) return DC_OK;
  if (!keys || !slots || !n_blocks || !sum || !count || !vps || !dirs || !scan_offset || !poses || n_scans < 1) return DC_ERR_ARG;
  const int64_t nb = *n_blocks < 0 ? 0 : (*n_blocks > capacity ? capacity : *n_blocks);
  const dc::TsdfTable total{keys, slots, nb, capacity, sum, count};
  const dc::TsdfCastRule rule{t_min, step, trunc, J, refine, min_count, skip != 0};
  for (int64_t i = 0; i < n; ++i) {
    const int s = dc::scan_of(scan_offset, n_scans, i);
    dc::TsdfTable own{nullptr, nullptr, 0, own_capacity, own_sum, own_count};
    if (own_keys) {
      int64_t oa = own_ptr[s], ob = own_ptr[s + 1];
      oa = oa < 0 ? 0 : (oa > n_own_keys ? n_own_keys : oa);
      ob = ob < oa ? oa : (ob > n_own_keys ? n_own_keys : ob);
      own.keys = own_keys + oa; own.slots = own_slots + oa; own.nb = ob - oa;
    }
    double vp[3], dir[3];
    host_load3(vps, dtype, i, vp);
    host_load3(dirs, dtype, i, dir);
    dc::TsdfCastLane lane;
    dc::TsdfCastResult r{-1, INFINITY, NAN, {NAN, NAN, NAN}, NAN, dc::kTsdfCastSkipped, 0};
    if (dc::tsdf_cast_setup(vp, dir, poses + 16 * (int64_t)s, mask ? mask[i] != 0 : true, &lane)) r = dc::tsdf_cast_ray(lane, g, rule, total, own);
    face_out[i] = r.face;
    t_out[i] = r.t;
    inc_out[i] = r.inc;
    for (int a = 0; a < 3; ++a) normal_out[3 * i + a] = r.normal[a];
    phi_out[i] = r.phi;
    status_out[i] = (uint8_t)r.status;
    samples_out[i] = r.samples;
  }
  return DC_OK;
}

}  // extern "C"
