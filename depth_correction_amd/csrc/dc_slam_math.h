// The per-iteration algebra of the scan-to-map point-to-plane ICP (dc_slam.hip), shared by the finish kernel and the
// test-only host build (dc_hostcheck.cpp): the 6 x 6 fp64 normal equations and the pose update.  Reference configuration:
// config/slam/icp.yaml (PointToPlaneErrorMinimizer); DESIGN "SLAM evaluation" states the algorithm.
#pragma once
#include <math.h>
#include "dc_common.h"

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

}  // namespace dc
