// Which kernels an evaluation of a dcSequenceDesc runs (sequence_eval_impl in dc_consistency.hip): the decision and nothing else.
// Plain host C++ -- no HIP, nothing of dc_device.h -- so dc_hostcheck.cpp exports it and tests/test_route_host.py pins it on the CPU.
// It reads descriptor scalars, whether pointers are null and the host-side fields of dcBlockTable / dcPoseTable; it never
// dereferences a device pointer, allocates or takes a lock.  DESIGN.md 4 has the table route kind -> conditions -> kernel.
#pragma once
#include "dc_common.h"
#include "../../include/dc_hip.h"

namespace dc {

// The device headers own these; dc_consistency.hip static_asserts every one of them against the device definition.
constexpr int kRouteBlock = 256;             // kBlock
constexpr int kRouteXcds = 8;                // kXcds: the rounding of xcd_grid
constexpr int kRouteWavesPerBlock = 4;       // kWavesPerBlock
constexpr int kRouteLdsScans = 32;           // kLdsScans
constexpr int kRouteMaxBlockScans = 64;      // kMaxBlockScans
constexpr int kRouteStepQ32Cap = 512;        // kStepQ32Cap
constexpr int kRouteChainFront = 8;          // kChainFront
constexpr uint32_t route_x_row_bytes(bool f64) { return f64 ? 32u : 16u; }                            // RowBytes<PT>::x
constexpr uint32_t route_rec_row_bytes(bool f64) { return f64 ? 64u : 32u; }                          // RowBytes<PT>::rec
constexpr uint32_t route_step_row_bytes(bool f64, int P) { return 16u * (f64 ? 3u : (unsigned)(6 + P + 3) / 4u); }   // StepRow<PT, P>::kPieces * 16
constexpr int64_t route_blocks(int64_t n) { return (n + kRouteBlock - 1) / kRouteBlock; }
constexpr int64_t route_xcd_grid(int64_t n_logical) { return ((n_logical + kRouteXcds - 1) / kRouteXcds) * kRouteXcds; }   // xcd_grid

// the row counts of a sequence, for everything that sizes a grid or finds a buffer of dcSequenceDesc.partials
struct SeqRows {
  int64_t n_rows;      // forward rows: the centres (the backward runs over all n points)
  int64_t g_blocks;    // blocks of a launch over the centres, rounded to the XCDs; a chained launch leaves one partial row per block
  int64_t rows;        // partial rows of an ordinary launch over all n points: one per wavefront
};
inline SeqRows route_seq_rows(const dcSequenceDesc* d) {
  const int64_t n_rows = d->centre_idx ? d->n_centres : d->n;
  return SeqRows{n_rows, route_xcd_grid(route_blocks(n_rows)), route_xcd_grid(route_blocks(d->n)) * kRouteWavesPerBlock};
}
// doubles of dcSequenceDesc.partials (dc_sequence_partials_count): the columns of ordinary evaluations, then the two buffers of a chain
inline int64_t route_partials_count(int64_t n, int n_terms, int n_scans) {
  if (n < 0 || n_terms < 0 || n_scans < 0) return 0;
  const int64_t rows = route_xcd_grid(route_blocks(n)) * kRouteWavesPerBlock;
  return rows * (2 + 2 * (int64_t)n_terms + 12 * (int64_t)n_scans) + 2 * (2 + (int64_t)n_terms) * rows;
}

// the dc_set_option switches the decision reads, taken from the atomics once per call
struct RouteOptions {
  bool no_tab = false, no_basis = false, two_pass = false, pose_three_pass = false, step_six = false;
  int fwd_generic = 0, step_var = 1;
};

enum RouteKind {
  ROUTE_EMPTY = 0,     // n == 0: the memset of `out`
  ROUTE_STEP_RAGGED,   // consistency_step_ragged_q32_kernel<P, cap>
  ROUTE_STEP_Q32,      // consistency_step_q32_kernel<k, P, cap[, 6]>
  ROUTE_STEP_BASIS,    // consistency_step_basis_kernel<PT, k, P, kStepVar | 0>
  ROUTE_STEP_SLOTS,    // consistency_step_basis_slots_kernel<PT, P>
  ROUTE_TWO_PASS,      // consistency_fwd_basis[_slots]_kernel (+ consistency_bwd_basis_kernel with want_grad)
  ROUTE_POSE,          // consistency_step_pose_kernel<k, P>
  ROUTE_GENERAL        // dc_points_fwd + consistency_fwd_impl (+ consistency_bwd_impl)
};

// What the launch code needs, and nothing it must work out again.
struct SeqRoute {
  int kind = ROUTE_EMPTY;
  // template coordinates of the instantiation
  bool f64 = false;        // point type: q32 (float32 clouds) or double
  int k = 0;               // 4 / 8 / 10 / 16, or 0: the run-time slot loop
  int P = 0;               // weights; ROUTE_TWO_PASS: 0 for n_terms > 3
  int cap = 0;             // rows of the tile: ROUTE_STEP_Q32 512 / 768, ROUTE_STEP_RAGGED 1024 .. 4096
  bool six = false;        // ROUTE_STEP_Q32: the six-blocks-per-CU build (dc_set_option(9, 1))
  bool round2 = false;     // ROUTE_STEP_BASIS: the <PT, 10, 2, 0> form (dc_set_option(6, 0))
  const dcBlockTable* table = nullptr;   // the forward table that is staged ...
  bool table_loss = false; // ... which is dcSequenceDesc.fwd_table_loss
  bool use_hdr = false;    // the kernel reads dcSequenceDesc.step_hdr
  int max_rows = 0;        // the longest list among the blocks that are staged (fwd_rows_active where it applies)
  size_t lds_fwd = 0, lds_bwd = 0;       // LDS bytes and rows of the staged tiles: forward / one-pass kernel, two-pass backward
  int rows_fwd = 0, rows_bwd = 0;
  bool grouped = false;    // ROUTE_GENERAL: the backward leaves the pose slots row-major, one row per block (dcSequenceDesc.scan_seg)
  int n_terms = 0, n_acc = 0, n_red = 0; // weights in use, gradient slots of `out`, slots the kernels produce
  int64_t n_rows = 0, g_blocks = 0, rows = 0;   // SeqRows
  int64_t grid = 0;        // blocks of the one-pass launch: g_blocks (+ kRouteChainFront in a chain)
};

// a usable table of the wanted layout -> LDS bytes / rows of the staged tile (+ `extra_rows`), which must fit `lds_limit`; max_rows: the
// longest list that is staged (-1: the table's own)
inline bool use_table(const dcBlockTable* t, bool no_tab, int layout, int stride, uint32_t row_bytes, int extra_rows, size_t lds_limit,
                      size_t* lds_bytes, int* lds_rows, int max_rows = -1) {
  if (t && max_rows < 0) max_rows = t->max_rows;
  if (!t || no_tab || stride != 4 || t->layout != layout || !t->blk_ptr || !t->loc || max_rows < 0) return false;
  if (layout == DC_TABLE_SLOTS ? !t->slot_ptr : !t->run_ptr) return false;
  if (max_rows > 0 && !t->blk_ids) return false;
  const size_t rows = (size_t)max_rows + extra_rows + (max_rows + extra_rows == 0 ? 1 : 0);
  const size_t need = rows * row_bytes;
  if (need > lds_limit || max_rows >= 0xFFF) return false;       // positions are 16 x row in 16 bits
  *lds_bytes = need;
  *lds_rows = (int)rows;
  return true;
}

inline bool route_fixed_k(int k) { return k == 10 || k == 4 || k == 8 || k == 16; }

// One pass of the decision over forward table `ft` (`rows_active`: its fwd_rows_active).  loss_pass: `ft` is fwd_table_loss; only a
// one-pass route will do, anything else is DC_ERR_UNSUPPORTED ("take fwd_table").
inline int route_pass(const dcSequenceDesc* d, const dcBlockTable* ft, int rows_active, bool loss_pass, bool has_w, int want_grad,
                      int want_exponent_grad, int want_pose_grad, bool chained, const RouteOptions& o, SeqRoute* r) {
  *r = SeqRoute{};
  const int stride = 4;
  const int n_terms = d->model_kind == DC_MODEL_NONE ? 0 : d->n_terms;
  r->n_terms = n_terms;
  r->n_acc = 2 * n_terms + 12 * d->n_scans;
  if (d->n == 0) return DC_OK;                                     // ROUTE_EMPTY
  if (d->partials_count < route_partials_count(d->n, n_terms, d->n_scans)) return DC_ERR_WORKSPACE;
  if (d->centre_idx && (d->n_centres < 0 || d->n_centres > d->n)) return DC_ERR_ARG;
  const SeqRows sr = route_seq_rows(d);
  r->n_rows = sr.n_rows; r->g_blocks = sr.g_blocks; r->rows = sr.rows;
  r->n_red = !want_grad ? 0 : (want_pose_grad ? r->n_acc : 2 * n_terms);
  r->table = ft; r->table_loss = loss_pass;
  const bool q32_pts = d->point_fmt == DC_Q32 && d->dtype == DC_F32, f64_pts = d->point_fmt == DC_F64 && d->dtype == DC_F64;
  r->f64 = f64_pts;
  // the one-pass kernels never stage the blocks they skip: their tile is sized by the longest list among the others
  const int act_rows = !ft ? 0 : ((d->blk_skip && d->mask && !d->centre_idx && rows_active > 0 && rows_active < ft->max_rows) ? rows_active : ft->max_rows);
  r->max_rows = act_rows;
  // ball neighbourhoods on float32 clouds (a packed table from CSR lists that knows its rows' lengths): the ragged one-pass kernel,
  // whose tile may take up to 128 KB of LDS
  const bool ragged_ok = q32_pts && ft && ft->layout == DC_TABLE_SLOTS && ft->packed == 1 && ft->row_ptr && ft->own_base && !d->centre_idx &&
                         ft->max_rows > 0 && !o.no_tab && o.step_var != 8 &&
                         (size_t)act_rows * route_step_row_bytes(false, n_terms <= 2 ? 2 : 3) <= 128 * 1024 && act_rows <= (n_terms <= 2 ? 4096 : 2560);
  // basis form: the basis rows of the current poses and exponents are valid (the caller says so by passing them), only the weights
  // change between evaluations -> no pass over the points
  const bool basis_fwd = d->basis && (q32_pts || f64_pts) && n_terms > 0 && has_w && !want_exponent_grad && !want_pose_grad && !o.no_basis &&
                         (use_table(ft, o.no_tab, DC_TABLE_SLOTS, stride, route_x_row_bytes(f64_pts), 0, 60 * 1024, &r->lds_fwd, &r->rows_fwd) ||
                          (ragged_ok && want_grad && n_terms <= 3 && !o.two_pass));
  // loss and dL/dw in ONE pass (forward-mode) for up to three weights: no record, no backward launch, no transposed table
  size_t lds_s = 0;
  int rows_s = 0;
  const bool one_pass = basis_fwd && want_grad && n_terms <= 3 && !o.two_pass &&
                        (use_table(ft, o.no_tab, DC_TABLE_SLOTS, stride, route_step_row_bytes(f64_pts, n_terms), 0, 60 * 1024, &lds_s, &rows_s, act_rows) ||
                         ragged_ok);
  // pose gradients (no exponent gradients) of a float32 sequence with a [rows, K] table whose pose tables and local basis rows the
  // plan has built: one launch, no transposed lists
  const bool pose_one_pass = want_grad && want_pose_grad && !want_exponent_grad && d->pose_table && d->local_basis && !d->vps && !d->centre_idx &&
                             q32_pts && (n_terms == 1 || n_terms == 2) && d->n_scans <= kRouteLdsScans && has_w && route_fixed_k(d->k) &&
                             !o.pose_three_pass;
  // every other way to a gradient walks the transposed neighbour lists: the caller provides them on demand
  if (want_grad && !one_pass && !pose_one_pass && (!d->csr_ptr || !d->csr_src)) return DC_ERR_BACKWARD_TABLES;
  const bool basis = basis_fwd && (!want_grad || one_pass ||
                                   use_table(d->bwd_table, o.no_tab, DC_TABLE_RUNS, stride, route_rec_row_bytes(f64_pts), 1, 44 * 1024, &r->lds_bwd, &r->rows_bwd));
  // a chained step exists for the one-pass kernels only: the caller steps without a chain otherwise
  if ((chained || loss_pass) && !(basis && one_pass)) return DC_ERR_UNSUPPORTED;
  if ((basis || pose_one_pass) && q32_pts && !(d->qparams[3] > 0.0)) return DC_ERR_ARG;      // (make_qparams)
  const int fixed_k = o.fwd_generic ? 0 : d->k;
  r->k = route_fixed_k(fixed_k) ? fixed_k : 0;
  r->P = n_terms;
  if (basis && one_pass) {
    r->lds_fwd = lds_s; r->rows_fwd = rows_s;
    r->grid = sr.g_blocks + (chained ? kRouteChainFront : 0);
    // the block headers belong to the table this pass stages from (fwd_table_loss's where the descriptor has one); with a compact
    // centre list the kernel takes the centres by index: a header that names own rows does not describe that
    const bool hdr = (loss_pass || !d->fwd_table_loss) && !(d->centre_idx && ft->own_base) && d->step_hdr;
    if (ragged_ok) {
      r->kind = ROUTE_STEP_RAGGED;
      const int mr = act_rows;
      r->cap = n_terms <= 2 ? (mr <= 1024 ? 1024 : mr <= 1280 ? 1280 : mr <= 1600 ? 1600 : mr <= 2048 ? 2048 : mr <= 2560 ? 2560 : 4096)
                            : (mr <= 1024 ? 1024 : mr <= 1600 ? 1600 : 2560);
      r->k = 0;
      r->lds_fwd = (size_t)route_step_row_bytes(false, n_terms) * r->cap; r->rows_fwd = r->cap;
    } else if (q32_pts && o.step_var == 1 && r->k && rows_s <= 768 && hdr) {
      r->kind = ROUTE_STEP_Q32;
      r->use_hdr = true;
      r->cap = rows_s <= kRouteStepQ32Cap ? kRouteStepQ32Cap : 768;
      r->six = rows_s <= kRouteStepQ32Cap && n_terms <= 2 && o.step_six;
    } else {
      r->kind = r->k ? ROUTE_STEP_BASIS : ROUTE_STEP_SLOTS;
      r->round2 = r->k == 10 && n_terms == 2 && o.step_var == 0;
    }
    return DC_OK;
  }
  if (basis) {
    r->kind = ROUTE_TWO_PASS;
    r->P = n_terms <= 3 ? n_terms : 0;         // (more than three weights reach the <.., 0> instantiations)
    r->max_rows = ft->max_rows;
    return DC_OK;
  }
  r->table = d->fwd_table; r->max_rows = 0; r->lds_fwd = r->lds_bwd = 0; r->rows_fwd = r->rows_bwd = 0;
  if (pose_one_pass) {
    r->kind = ROUTE_POSE;
    r->k = d->k;
    r->f64 = false;
    return DC_OK;
  }
  r->kind = ROUTE_GENERAL;
  r->k = 0; r->P = 0;
  // (as consistency_bwd_impl decides)
  r->grouped = want_grad && want_pose_grad && d->scan_seg && !d->lane_perm && d->n_scans <= kRouteMaxBlockScans;
  return DC_OK;
}

// The route of one evaluation; returns what sequence_eval_impl returns for the same input (DC_OK, DC_ERR_ARG, DC_ERR_WORKSPACE,
// DC_ERR_BACKWARD_TABLES, DC_ERR_UNSUPPORTED: a chained call that no one-pass kernel takes).
inline int dc_choose_route(const dcSequenceDesc* d, bool has_w, int want_grad, int want_exponent_grad, int want_pose_grad, bool chained,
                           const RouteOptions& o, SeqRoute* r) {
  if (!d || !d->partials) return DC_ERR_ARG;
  // the one-pass evaluation first tries the table that lists only what the centres INSIDE the mask gather (fwd_table_loss); only
  // "no one-pass kernel takes it" falls through to fwd_table
  if (d->fwd_table_loss && d->mask && !d->centre_idx && want_grad && !want_exponent_grad && !want_pose_grad && d->basis &&
      d->model_kind != DC_MODEL_NONE && d->n_terms >= 1 && d->n_terms <= 3 && d->n > 0) {
    const int rc = route_pass(d, d->fwd_table_loss, d->fwd_rows_active_loss, true, has_w, want_grad, 0, 0, chained, o, r);
    if (rc != DC_ERR_UNSUPPORTED) return rc;
  }
  return route_pass(d, d->fwd_table, d->fwd_rows_active, false, has_w, want_grad, want_exponent_grad, want_pose_grad, chained, o, r);
}

// ... with the argument check of the entry points in front (what dc_sequence_eval and the step calls run)
inline int dc_choose_route_call(const dcSequenceDesc* d, const void* w, const void* poses, const void* out, int want_grad,
                                int want_exponent_grad, int want_pose_grad, bool chained, const RouteOptions& o, SeqRoute* r) {
  if (!d || !out || !poses || !d->partials) return DC_ERR_ARG;
  return dc_choose_route(d, w != nullptr, want_grad, want_exponent_grad, want_pose_grad, chained, o, r);
}

}  // namespace dc
