// The per-iteration algebra of the scan-to-map point-to-plane ICP (dc_slam.hip), shared by the finish kernel and the
// test-only host build (dc_hostcheck.cpp): the 6 x 6 fp64 normal equations, the pose update and the checks that end a
// registration.  Reference configuration: config/slam/icp.yaml (PointToPlaneErrorMinimizer, transformationCheckers); DESIGN
// "SLAM evaluation" states the algorithm.
#pragma once
#include <math.h>
#include "dc_common.h"
#include "../../include/dc_hip.h"

namespace dc {

// JtJ packed as its upper triangle row by row: (0,0) (0,1) .. (0,5) (1,1) .. (5,5) -- 21 entries.
DC_HD int sym6_index(int r, int c) {
  if (r > c) { const int t = r; r = c; c = t; }
  return r * 6 - (r * (r - 1)) / 2 + (c - r);
}

// x = -(JtJ)^-1 Jtr by a Cholesky factorisation in fp64.  Returns 0, or 1 when a pivot is not above rel_eps times the largest
// diagonal entry (the system is singular: the pairs do not constrain all six degrees of freedom) or is not finite.
DC_HD int icp_solve6(const double* a21, const double* b6, double* x6, double rel_eps = 1e-12) {
  double L[6][6];
  double dmax = 0.0;
  for (int i = 0; i < 6; ++i) dmax = fmax(dmax, fabs(a21[sym6_index(i, i)]));
  if (!(dmax > 0.0) || !isfinite(dmax)) return 1;
  for (int j = 0; j < 6; ++j) {
    double s = a21[sym6_index(j, j)];
    for (int k = 0; k < j; ++k) s -= L[j][k] * L[j][k];
    if (!(s > rel_eps * dmax) || !isfinite(s)) return 1;
    const double d = sqrt(s);
    L[j][j] = d;
    for (int i = j + 1; i < 6; ++i) {
      double t = a21[sym6_index(i, j)];
      for (int k = 0; k < j; ++k) t -= L[i][k] * L[j][k];
      L[i][j] = t / d;
    }
  }
  double y[6];
  for (int i = 0; i < 6; ++i) {                  // L y = -b
    double t = -b6[i];
    for (int k = 0; k < i; ++k) t -= L[i][k] * y[k];
    y[i] = t / L[i][i];
  }
  for (int i = 5; i >= 0; --i) {                 // L^T x = y
    double t = y[i];
    for (int k = i + 1; k < 6; ++k) t -= L[k][i] * x6[k];
    x6[i] = t / L[i][i];
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

// The single-thread tail of dc_icp_finish once the DC_ICP_PARTIALS totals of an iteration are complete (the block partials
// [n_blocks, DC_ICP_PARTIALS] added in the order of dc_rowsum.h, eight lanes): counts the iteration,
// records pairs / SSE / overlap, solves, and then in this order: DC_ICP_FAIL_PAIRS, DC_ICP_FAIL_SINGULAR, DC_ICP_FAIL_NONFINITE,
// DC_ICP_FAIL_BOUND (each leaves the estimate as it was), the estimate and the increment history updated, DC_ICP_CONVERGED,
// DC_ICP_MAX_ITERS.  A status word that is already set is the caller's to test: this function is not called then.
DC_HD void icp_finish_tail(const double* tot, int64_t m, const IcpParams& prm, double* st, int32_t* status) {
  const int iter = status[1] + 1;
  status[1] = iter;
  st[DC_ICP_STATE_PAIRS] = tot[27];
  st[DC_ICP_STATE_SSE] = tot[28];
  st[DC_ICP_STATE_OVERLAP] = m > 0 ? tot[29] / (double)m : 0.0;
  if (tot[27] < (double)prm.min_pairs) { status[0] = DC_ICP_FAIL_PAIRS; return; }
  double x[6];
  if (icp_solve6(tot, tot + 21, x)) { status[0] = DC_ICP_FAIL_SINGULAR; return; }
  double Tn[16];
  icp_apply_step(x, st + DC_ICP_STATE_POSE, Tn);
  bool finite = true;
  for (int q = 0; q < 6; ++q) finite = finite && isfinite(x[q]);
  for (int q = 0; q < 16; ++q) finite = finite && isfinite(Tn[q]);
  if (!finite) { status[0] = DC_ICP_FAIL_NONFINITE; return; }
  double C[16];
  rigid_div(Tn, st + DC_ICP_STATE_PRIOR, C);            // the total correction relative to the prior (BoundTransformationChecker)
  const double c_rot = rotation_angle4(C), c_trans = sqrt(C[3] * C[3] + C[7] * C[7] + C[11] * C[11]);
  if (!(c_rot <= prm.max_rot) || !(c_trans <= prm.max_trans)) { status[0] = DC_ICP_FAIL_BOUND; return; }
  for (int q = 0; q < 16; ++q) st[DC_ICP_STATE_POSE + q] = Tn[q];
  // DifferentialTransformationChecker: the mean rotation / translation of the last `smooth` increments
  const int slot = (iter - 1) % DC_ICP_MAX_SMOOTH;
  st[DC_ICP_STATE_HIST_ROT + slot] = sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
  st[DC_ICP_STATE_HIST_TRANS + slot] = sqrt(x[3] * x[3] + x[4] * x[4] + x[5] * x[5]);
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
  if (iter >= prm.max_iters) status[0] = DC_ICP_MAX_ITERS;      // CounterTransformationChecker: stop, keep the estimate
}

// ---- the sweep-aware (12-dof) iteration: pose at the sweep's start and the twist (v, w) of the sweep; DESIGN "Sweep-aware
// registration", include/dc_hip.h.  Unknowns in the order (d theta, d t, d v, d w). ----

// JtJ packed as its upper triangle row by row: 78 entries.
DC_HD int sym12_index(int r, int c) {
  if (r > c) { const int t = r; r = c; c = t; }
  return r * 12 - (r * (r - 1)) / 2 + (c - r);
}

// icp_solve6's factorisation and pivot rule for the 12 x 12 system (A row-major, full): x = -A^-1 b, 1 = singular.  L [144] and
// y [12] are the caller's: the finish kernel keeps them in LDS, where a runtime index costs no private segment.
DC_HD int icp_solve12(const double* A, const double* b12, double* x12, double* Lw, double* y, double rel_eps = 1e-12) {
  double (*L)[12] = (double (*)[12])Lw;
  double dmax = 0.0;
  for (int i = 0; i < 12; ++i) dmax = fmax(dmax, fabs(A[i * 12 + i]));
  if (!(dmax > 0.0) || !isfinite(dmax)) return 1;
  for (int j = 0; j < 12; ++j) {
    double s = A[j * 12 + j];
    for (int k = 0; k < j; ++k) s -= L[j][k] * L[j][k];
    if (!(s > rel_eps * dmax) || !isfinite(s)) return 1;
    const double d = sqrt(s);
    L[j][j] = d;
    for (int i = j + 1; i < 12; ++i) {
      double t = A[i * 12 + j];
      for (int k = 0; k < j; ++k) t -= L[i][k] * L[j][k];
      L[i][j] = t / d;
    }
  }
  for (int i = 0; i < 12; ++i) {                 // L y = -b
    double t = -b12[i];
    for (int k = 0; k < i; ++k) t -= L[i][k] * y[k];
    y[i] = t / L[i][i];
  }
  for (int i = 11; i >= 0; --i) {                // L^T x = y
    double t = y[i];
    for (int k = i + 1; k < 12; ++k) t -= L[k][i] * x12[k];
    x12[i] = t / L[i][i];
  }
  return 0;
}

struct IcpCtParams {
  double beta_v, beta_w;                  // the constant-velocity prior's weights (dimensionless, per kept pair)
  double max_twist_trans, max_twist_rot;  // largest |v - v0| and |w - w0|
};

DC_HD double icp_norm3(const double* a) { return sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]); }

// The single-thread tail of dc_icp_ct_finish once the DC_ICP_CT_PARTIALS totals are complete; st is the 6-dof state
// [DC_ICP_STATE_COUNT] (pose, prior, history, pairs / SSE / overlap as icp_finish_tail keeps them), ct the twist state
// [DC_ICP_CT_STATE_COUNT].  The order of icp_finish_tail: count, record, DC_ICP_FAIL_PAIRS, the prior N beta (twist - prior twist)
// added to the system, DC_ICP_FAIL_SINGULAR, DC_ICP_FAIL_NONFINITE, DC_ICP_FAIL_BOUND (the pose bound, |w| > pi, the twist bound;
// every failure leaves pose and twist as they were), pose, twist and history updated, DC_ICP_CONVERGED, DC_ICP_MAX_ITERS.
constexpr int kIcpCtWork = 144 + 144 + 3 * 12;      // doubles of icp_ct_finish_tail's workspace: A, L, b, x, y

DC_HD void icp_ct_finish_tail(const double* tot, int64_t m, const IcpParams& prm, const IcpCtParams& cp, double* st, double* ct,
                              int32_t* status, double* work) {
  const int iter = status[1] + 1;
  status[1] = iter;
  const double pairs = tot[90];
  st[DC_ICP_STATE_PAIRS] = pairs;
  st[DC_ICP_STATE_SSE] = tot[91];
  st[DC_ICP_STATE_OVERLAP] = m > 0 ? tot[92] / (double)m : 0.0;
  if (pairs < (double)prm.min_pairs) { status[0] = DC_ICP_FAIL_PAIRS; return; }
  double *A = work, *L = work + 144, *b = work + 288, *x = work + 300, *y = work + 312;
  for (int r = 0; r < 12; ++r) {
    for (int c = 0; c < 12; ++c) A[r * 12 + c] = tot[sym12_index(r, c)];
    b[r] = tot[78 + r];
  }
  const double* tw = ct + DC_ICP_CT_STATE_TWIST;
  const double* tw0 = ct + DC_ICP_CT_STATE_PRIOR_TWIST;
  for (int q = 0; q < 6; ++q) {
    const double wgt = pairs * (q < 3 ? cp.beta_v : cp.beta_w);
    A[(6 + q) * 12 + 6 + q] += wgt;
    b[6 + q] += wgt * (tw[q] - tw0[q]);
  }
  if (icp_solve12(A, b, x, L, y)) { status[0] = DC_ICP_FAIL_SINGULAR; return; }
  double Tn[16], twn[6];
  icp_apply_step(x, st + DC_ICP_STATE_POSE, Tn);
  for (int q = 0; q < 6; ++q) twn[q] = tw[q] + x[6 + q];
  bool finite = true;
  for (int q = 0; q < 12; ++q) finite = finite && isfinite(x[q]);
  for (int q = 0; q < 16; ++q) finite = finite && isfinite(Tn[q]);
  for (int q = 0; q < 6; ++q) finite = finite && isfinite(twn[q]);
  if (!finite) { status[0] = DC_ICP_FAIL_NONFINITE; return; }
  double C[16];
  rigid_div(Tn, st + DC_ICP_STATE_PRIOR, C);
  const double c_rot = rotation_angle4(C), c_trans = sqrt(C[3] * C[3] + C[7] * C[7] + C[11] * C[11]);
  if (!(c_rot <= prm.max_rot) || !(c_trans <= prm.max_trans)) { status[0] = DC_ICP_FAIL_BOUND; return; }
  double dtw[6];
  for (int q = 0; q < 6; ++q) dtw[q] = twn[q] - tw0[q];
  if (!(icp_norm3(twn + 3) <= 3.14159265358979323846) || !(icp_norm3(dtw) <= cp.max_twist_trans) || !(icp_norm3(dtw + 3) <= cp.max_twist_rot)) {
    status[0] = DC_ICP_FAIL_BOUND;
    return;
  }
  for (int q = 0; q < 16; ++q) st[DC_ICP_STATE_POSE + q] = Tn[q];
  for (int q = 0; q < 6; ++q) ct[DC_ICP_CT_STATE_TWIST + q] = twn[q];
  const int slot = (iter - 1) % DC_ICP_MAX_SMOOTH;
  st[DC_ICP_STATE_HIST_ROT + slot] = fmax(icp_norm3(x), icp_norm3(x + 9));
  st[DC_ICP_STATE_HIST_TRANS + slot] = fmax(icp_norm3(x + 3), icp_norm3(x + 6));
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

}  // namespace dc
