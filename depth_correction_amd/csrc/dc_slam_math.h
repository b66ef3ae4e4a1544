// The per-iteration algebra of the scan-to-map point-to-plane ICP (dc_slam.hip), shared by the finish kernels and the
// test-only host build (dc_hostcheck.cpp): the fp64 normal equations of 6 unknowns (the pose) or 12 (pose and sweep twist), the
// pose update and the checks that end a registration.  Reference configuration: config/slam/icp.yaml (PointToPlaneErrorMinimizer, transformationCheckers); DESIGN
// "SLAM evaluation" states the algorithm.
#pragma once
#include <math.h>
#include "dc_common.h"
#include "../../include/dc_hip.h"

namespace dc {

// x = R p + t with the products and sums rounded in this order (dc_knn_grid_query moves the queries with the same arithmetic,
// so the point a pair is formed with is the point that was matched; dc_tsdf_sparse_sample samples the volume at this point).  Plain
// operators with contraction switched off for this function: __dmul_rn / __dadd_rn are inline functions of plain operators, which
// the compiler fuses into fma where it inlines them.
DC_HD void move_point(const double* T, const double* p, double* x) {
#pragma clang fp contract(off)
#pragma unroll
  for (int r = 0; r < 3; ++r) x[r] = ((T[r * 4] * p[0] + T[r * 4 + 1] * p[1]) + T[r * 4 + 2] * p[2]) + T[r * 4 + 3];
}

// JtJ of N unknowns packed as its upper triangle row by row: (0,0) (0,1) .. (0,N-1) (1,1) .. (N-1,N-1) -- N (N + 1) / 2 entries.
template <int N>
DC_HD int sym_index(int r, int c) {
  if (r > c) { const int t = r; r = c; c = t; }
  return r * N - (r * (r - 1)) / 2 + (c - r);
}

// The row of partials and totals of a registration with NU unknowns: the packed JtJ, Jtr, then pairs, sum r^2 and points with a
// kept pair (DC_ICP_PARTIALS for 6 unknowns, DC_ICP_CT_PARTIALS for 12).
template <int NU>
struct IcpRow {
  static constexpr int kJtr = NU * (NU + 1) / 2, kPairs = kJtr + NU, kSse = kPairs + 1, kUsed = kPairs + 2, kWidth = kPairs + 3;
};
static_assert(IcpRow<6>::kWidth == DC_ICP_PARTIALS && IcpRow<12>::kWidth == DC_ICP_CT_PARTIALS, "row layouts of include/dc_hip.h");

// A (N x N row-major, both triangles) and b from a row of totals.
template <int N>
DC_HD void icp_unpack(const double* tot, double* A, double* b) {
  for (int r = 0; r < N; ++r) {
    for (int c = 0; c < N; ++c) A[r * N + c] = tot[sym_index<N>(r, c)];
    b[r] = tot[IcpRow<N>::kJtr + r];
  }
}

// x = -A^-1 b by a Cholesky factorisation in fp64 (A row-major N x N, its lower triangle is read).  Returns 0, or 1 when a pivot is
// not above rel_eps times the largest diagonal entry (the system is singular: the pairs do not constrain every unknown) or is not
// finite.  Lw [N * N] and y [N] are the caller's: local arrays for N = 6; for N = 12 the finish kernel keeps them in LDS, where a
// runtime index costs no private segment.
template <int N>
DC_HD int icp_solve(const double* A, const double* b, double* x, double* Lw, double* y, double rel_eps = 1e-12) {
  double (*L)[N] = (double (*)[N])Lw;
  double dmax = 0.0;
  for (int i = 0; i < N; ++i) dmax = fmax(dmax, fabs(A[i * N + i]));
  if (!(dmax > 0.0) || !isfinite(dmax)) return 1;
  for (int j = 0; j < N; ++j) {
    double s = A[j * N + j];
    for (int k = 0; k < j; ++k) s -= L[j][k] * L[j][k];
    if (!(s > rel_eps * dmax) || !isfinite(s)) return 1;
    const double d = sqrt(s);
    L[j][j] = d;
    for (int i = j + 1; i < N; ++i) {
      double t = A[i * N + j];
      for (int k = 0; k < j; ++k) t -= L[i][k] * L[j][k];
      L[i][j] = t / d;
    }
  }
  for (int i = 0; i < N; ++i) {                  // L y = -b
    double t = -b[i];
    for (int k = 0; k < i; ++k) t -= L[i][k] * y[k];
    y[i] = t / L[i][i];
  }
  for (int i = N - 1; i >= 0; --i) {             // L^T x = y
    double t = y[i];
    for (int k = i + 1; k < N; ++k) t -= L[k][i] * x[k];
    x[i] = t / L[i][i];
  }
  return 0;
}

// Rotation of the axis-angle w (row-major 3 x 3), the arithmetic of transform.axis_angle_to_matrix: quaternion with the
// small-angle series of sin(a/2)/a below 1e-6, then the quaternion's matrix.
DC_HD void axis_angle_matrix(const double* w, double* R) {
  const double a = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
  const double k = fabs(a) < 1e-6 ? 0.5 - a * a / 48.0 : sin(0.5 * a) / a;
  const double qr = cos(0.5 * a), qi = w[0] * k, qj = w[1] * k, qk = w[2] * k;
  const double s = 2.0 / (qr * qr + qi * qi + qj * qj + qk * qk);
  R[0] = 1.0 - s * (qj * qj + qk * qk); R[1] = s * (qi * qj - qk * qr); R[2] = s * (qi * qk + qj * qr);
  R[3] = s * (qi * qj + qk * qr); R[4] = 1.0 - s * (qi * qi + qk * qk); R[5] = s * (qj * qk - qi * qr);
  R[6] = s * (qi * qk - qj * qr); R[7] = s * (qj * qk + qi * qr); R[8] = 1.0 - s * (qi * qi + qj * qj);
}

// out = D T with D = [R(x[0:3]) x[3:6]; 0 1]: the step (rotation first, as the Jacobian rows [p x n, n] order it) left-multiplied
// onto the estimate T (row-major 4 x 4).
DC_HD void icp_apply_step(const double* x6, const double* T, double* out) {
  double R[9];
  axis_angle_matrix(x6, R);
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 4; ++c)
      out[r * 4 + c] = R[r * 3] * T[c] + R[r * 3 + 1] * T[4 + c] + R[r * 3 + 2] * T[8 + c] + (c == 3 ? x6[3 + r] : 0.0);
  }
  out[12] = 0.0; out[13] = 0.0; out[14] = 0.0; out[15] = 1.0;
}

// Angle of the rotation part of a row-major 4 x 4 (utils.rotation_angle: arccos of (trace - 1) / 2, clipped).
DC_HD double rotation_angle4(const double* T) {
  const double c = (T[0] + T[5] + T[10] - 1.0) * 0.5;
  return acos(c > 1.0 ? 1.0 : (c < -1.0 ? -1.0 : c));
}

// C = A B^-1 for rigid A, B (row-major 4 x 4): B^-1 = [R^T, -R^T t].
DC_HD void rigid_div(const double* A, const double* B, double* C) {
  double Bi[16];
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) Bi[r * 4 + c] = B[c * 4 + r];
    Bi[r * 4 + 3] = -(B[r] * B[3] + B[4 + r] * B[7] + B[8 + r] * B[11]);
  }
  Bi[12] = 0.0; Bi[13] = 0.0; Bi[14] = 0.0; Bi[15] = 1.0;
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) {
      double s = 0.0;
      for (int k = 0; k < 4; ++k) s += A[r * 4 + k] * Bi[k * 4 + c];
      C[r * 4 + c] = s;
    }
}

struct IcpParams {
  double min_rot, min_trans, max_rot, max_trans;
  int smooth, max_iters, min_pairs;
};

constexpr int kIcpBlocksMax = 512;      // most blocks (rows of partials) of dc_icp_accumulate

// The arguments dc_icp_finish and dc_icp_ct_finish, on the device and in the host build, both refuse.
inline bool icp_finish_args_ok(const double* partials, int n_blocks, int64_t m, int smooth, int max_iters, const double* state,
                               const int32_t* status) {
  return partials && state && status && n_blocks >= 1 && n_blocks <= kIcpBlocksMax && m >= 0 && smooth >= 1 && smooth <= DC_ICP_MAX_SMOOTH &&
         max_iters >= 1;
}

DC_HD double icp_norm3(const double* a) { return sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]); }

// ---- the steps both single-thread tails take, in the order they take them ----

// Counts the iteration and records pairs / SSE / overlap from the three counters at the end of a row of totals.  Returns the
// iteration's number (from 1), or 0 with DC_ICP_FAIL_PAIRS set.
DC_HD int icp_begin_iteration(const double* counters, int64_t m, const IcpParams& prm, double* st, int32_t* status) {
  const int iter = status[1] + 1;
  status[1] = iter;
  st[DC_ICP_STATE_PAIRS] = counters[0];
  st[DC_ICP_STATE_SSE] = counters[1];
  st[DC_ICP_STATE_OVERLAP] = m > 0 ? counters[2] / (double)m : 0.0;
  if (counters[0] < (double)prm.min_pairs) { status[0] = DC_ICP_FAIL_PAIRS; return 0; }
  return iter;
}

// The candidate pose Tn = D(x[0:6]) T of the step x [nx]; false when an entry of x or of Tn is not finite.  The tests are joined
// with & so that no branch splits the block that holds the rotation's products and their sums: the device compiler contracts
// within a basic block only, and a split there changes which products of icp_apply_step become fma.
DC_HD bool icp_candidate_pose(const double* x, int nx, const double* st, double* Tn) {
  icp_apply_step(x, st + DC_ICP_STATE_POSE, Tn);
  bool finite = true;
  for (int q = 0; q < nx; ++q) finite &= isfinite(x[q]);
  for (int q = 0; q < 16; ++q) finite &= isfinite(Tn[q]);
  return finite;
}

// BoundTransformationChecker: the total correction of the candidate relative to the prior inside max_rot / max_trans.
DC_HD bool icp_pose_in_bound(const double* Tn, const double* st, const IcpParams& prm) {
  double C[16];
  rigid_div(Tn, st + DC_ICP_STATE_PRIOR, C);
  const double c_rot = rotation_angle4(C), c_trans = sqrt(C[3] * C[3] + C[7] * C[7] + C[11] * C[11]);
  return c_rot <= prm.max_rot && c_trans <= prm.max_trans;
}

// DifferentialTransformationChecker on the history ring: records the rotation / translation sizes of iteration iter's increment,
// then DC_ICP_CONVERGED when the means of the last `smooth` are below min_rot / min_trans, else DC_ICP_MAX_ITERS at the counter
// (CounterTransformationChecker: stop, keep the estimate).
DC_HD void icp_record_increment(int iter, double d_rot, double d_trans, const IcpParams& prm, double* st, int32_t* status) {
  const int slot = (iter - 1) % DC_ICP_MAX_SMOOTH;
  st[DC_ICP_STATE_HIST_ROT + slot] = d_rot;
  st[DC_ICP_STATE_HIST_TRANS + slot] = d_trans;
  if (iter >= prm.smooth) {
    double mr = 0.0, mt = 0.0;
    for (int h = 0; h < prm.smooth; ++h) {
      const int s = (iter - 1 - h) % DC_ICP_MAX_SMOOTH;
      mr += st[DC_ICP_STATE_HIST_ROT + s];
      mt += st[DC_ICP_STATE_HIST_TRANS + s];
    }
    mr /= (double)prm.smooth;
    mt /= (double)prm.smooth;
    if (mr < prm.min_rot && mt < prm.min_trans) { status[0] = DC_ICP_CONVERGED; return; }
  }
  if (iter >= prm.max_iters) status[0] = DC_ICP_MAX_ITERS;
}

// The single-thread tail of dc_icp_finish once the DC_ICP_PARTIALS totals of an iteration are complete (the block partials
// [n_blocks, DC_ICP_PARTIALS] added in the order of dc_rowsum.h, eight lanes): counts the iteration,
// records pairs / SSE / overlap, solves, and then in this order: DC_ICP_FAIL_PAIRS, DC_ICP_FAIL_SINGULAR, DC_ICP_FAIL_NONFINITE,
// DC_ICP_FAIL_BOUND (each leaves the estimate as it was), the estimate and the increment history updated, DC_ICP_CONVERGED,
// DC_ICP_MAX_ITERS.  A status word that is already set is the caller's to test: this function is not called then.
DC_HD void icp_finish_tail(const double* tot, int64_t m, const IcpParams& prm, double* st, int32_t* status) {
  const int iter = icp_begin_iteration(tot + IcpRow<6>::kPairs, m, prm, st, status);
  if (!iter) return;
  double A[36], L[36], b[6], x[6], y[6];
  icp_unpack<6>(tot, A, b);
  if (icp_solve<6>(A, b, x, L, y)) { status[0] = DC_ICP_FAIL_SINGULAR; return; }
  double Tn[16];
  if (!icp_candidate_pose(x, 6, st, Tn)) { status[0] = DC_ICP_FAIL_NONFINITE; return; }
  if (!icp_pose_in_bound(Tn, st, prm)) { status[0] = DC_ICP_FAIL_BOUND; return; }
  for (int q = 0; q < 16; ++q) st[DC_ICP_STATE_POSE + q] = Tn[q];
  icp_record_increment(iter, icp_norm3(x), icp_norm3(x + 3), prm, st, status);
}

// ---- the sweep-aware (12-dof) iteration: pose at the sweep's start and the twist (v, w) of the sweep; DESIGN "Sweep-aware
// registration", include/dc_hip.h.  Unknowns in the order (d theta, d t, d v, d w). ----

struct IcpCtParams {
  double beta_v, beta_w;                  // the constant-velocity prior's weights (dimensionless, per kept pair)
  double max_twist_trans, max_twist_rot;  // largest |v - v0| and |w - w0|
};

constexpr int kIcpCtWork = 144 + 144 + 3 * 12;      // doubles of icp_ct_finish_tail's workspace: A, L, b, x, y

// The single-thread tail of dc_icp_ct_finish once the DC_ICP_CT_PARTIALS totals are complete; st is the 6-dof state
// [DC_ICP_STATE_COUNT] (pose, prior, history, pairs / SSE / overlap as icp_finish_tail keeps them), ct the twist state
// [DC_ICP_CT_STATE_COUNT].  icp_finish_tail's steps with the twist's between them: count, record, DC_ICP_FAIL_PAIRS, the prior
// N beta (twist - prior twist) added to the system, DC_ICP_FAIL_SINGULAR, DC_ICP_FAIL_NONFINITE, DC_ICP_FAIL_BOUND (the pose bound,
// |w| > pi, the twist bound; every failure leaves pose and twist as they were), pose, twist and history updated (the history
// holds the larger of the pose's and the twist's increment), DC_ICP_CONVERGED, DC_ICP_MAX_ITERS.
DC_HD void icp_ct_finish_tail(const double* tot, int64_t m, const IcpParams& prm, const IcpCtParams& cp, double* st, double* ct,
                              int32_t* status, double* work) {
  const int iter = icp_begin_iteration(tot + IcpRow<12>::kPairs, m, prm, st, status);
  if (!iter) return;
  double *A = work, *L = work + 144, *b = work + 288, *x = work + 300, *y = work + 312;
  icp_unpack<12>(tot, A, b);
  const double pairs = tot[IcpRow<12>::kPairs];
  const double* tw = ct + DC_ICP_CT_STATE_TWIST;
  const double* tw0 = ct + DC_ICP_CT_STATE_PRIOR_TWIST;
  for (int q = 0; q < 6; ++q) {
    const double wgt = pairs * (q < 3 ? cp.beta_v : cp.beta_w);
    A[(6 + q) * 12 + 6 + q] += wgt;
    b[6 + q] += wgt * (tw[q] - tw0[q]);
  }
  if (icp_solve<12>(A, b, x, L, y)) { status[0] = DC_ICP_FAIL_SINGULAR; return; }
  double Tn[16], twn[6];
  bool finite = icp_candidate_pose(x, 12, st, Tn);
  for (int q = 0; q < 6; ++q) twn[q] = tw[q] + x[6 + q];
  for (int q = 0; q < 6; ++q) finite = finite && isfinite(twn[q]);
  if (!finite) { status[0] = DC_ICP_FAIL_NONFINITE; return; }
  if (!icp_pose_in_bound(Tn, st, prm)) { status[0] = DC_ICP_FAIL_BOUND; return; }
  double dtw[6];
  for (int q = 0; q < 6; ++q) dtw[q] = twn[q] - tw0[q];
  if (!(icp_norm3(twn + 3) <= 3.14159265358979323846) || !(icp_norm3(dtw) <= cp.max_twist_trans) || !(icp_norm3(dtw + 3) <= cp.max_twist_rot)) {
    status[0] = DC_ICP_FAIL_BOUND;
    return;
  }
  for (int q = 0; q < 16; ++q) st[DC_ICP_STATE_POSE + q] = Tn[q];
  for (int q = 0; q < 6; ++q) ct[DC_ICP_CT_STATE_TWIST + q] = twn[q];
  icp_record_increment(iter, fmax(icp_norm3(x), icp_norm3(x + 9)), fmax(icp_norm3(x + 3), icp_norm3(x + 6)), prm, st, status);
}

}  // namespace dc
