// Survey registration: the closed-form rigid fit of dc_align_finish (dc_align.hip; DESIGN "Survey registration"), host and device.
// From the 17 moments of the kept pairs (p, y) taken about two fixed origins -- W, a = sum(p - o_p), b = sum(y - o_y),
// S = sum (p - o_p)(y - o_y)^T, E = sum d^2 -- the rotation is the eigenvector of largest eigenvalue of Horn's symmetric 4 x 4 matrix
// of C = S - a b^T / W (B. K. P. Horn, "Closed-form solution of absolute orientation using unit quaternions", JOSA A 4(4), 1987),
// found by cyclic Jacobi in fp64: always the best PROPER rotation, also where the unconstrained optimum is a reflection.
#pragma once
#include <math.h>
#include "dc_common.h"
#include "../../include/dc_hip.h"

namespace dc {

struct AlignParams {
  double min_rot, min_trans;
  int min_pairs, max_iters;
};

constexpr int kAlignBlocksMax = 1024;   // most blocks (rows of partials) of dc_align_accumulate
constexpr double kAlignRelEps = 1e-12;  // icp_solve's rel_eps: the relative eigenvalue gap below which the fit is not unique
constexpr int kAlignSweeps = 16;        // cyclic Jacobi sweeps at most (a 4 x 4 matrix converges in 4 - 6)

// Horn's matrix N (row-major 4 x 4, symmetric) of C (row-major 3 x 3, C_ij = sum p_i y_j): q^T N q = trace(R(q)^T ... ) is largest
// for the unit quaternion q = (q0, qx, qy, qz) of the rotation that takes p to y.
DC_HD void horn_matrix(const double* C, double* N) {
  const double xx = C[0], xy = C[1], xz = C[2], yx = C[3], yy = C[4], yz = C[5], zx = C[6], zy = C[7], zz = C[8];
  N[0] = (xx + yy) + zz;  N[1] = yz - zy;          N[2] = zx - xz;           N[3] = xy - yx;
  N[4] = N[1];            N[5] = (xx - yy) - zz;   N[6] = xy + yx;           N[7] = zx + xz;
  N[8] = N[2];            N[9] = N[6];             N[10] = (yy - xx) - zz;   N[11] = yz + zy;
  N[12] = N[3];           N[13] = N[7];            N[14] = N[11];            N[15] = (zz - xx) - yy;
}

// Cyclic Jacobi on the symmetric A (row-major 4 x 4, destroyed): lam [4] its diagonal at the end, V (row-major, the columns the
// eigenvectors).  The pairs are visited in the fixed order (0,1) (0,2) (0,3) (1,2) (1,3) (2,3); a sweep that rotates nothing ends it.
DC_HD void jacobi4(double* A, double* lam, double* V) {
  for (int i = 0; i < 16; ++i) V[i] = (i % 5 == 0) ? 1.0 : 0.0;
  for (int sweep = 0; sweep < kAlignSweeps; ++sweep) {
    bool rotated = false;
    for (int p = 0; p < 3; ++p) {
      for (int q = p + 1; q < 4; ++q) {
        const double apq = A[p * 4 + q];
        if (apq == 0.0) continue;
        const double app = A[p * 4 + p], aqq = A[q * 4 + q];
        // an off-diagonal entry that no longer changes either diagonal entry is set to zero (the classical stopping rule)
        if (fabs(app) + fabs(apq) == fabs(app) && fabs(aqq) + fabs(apq) == fabs(aqq)) {
          A[p * 4 + q] = A[q * 4 + p] = 0.0;
          continue;
        }
        rotated = true;
        const double theta = (aqq - app) / (2.0 * apq);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < 4; ++k) {               // A <- A J
          const double akp = A[k * 4 + p], akq = A[k * 4 + q];
          A[k * 4 + p] = c * akp - s * akq;
          A[k * 4 + q] = s * akp + c * akq;
        }
        for (int k = 0; k < 4; ++k) {               // A <- J^T A
          const double apk = A[p * 4 + k], aqk = A[q * 4 + k];
          A[p * 4 + k] = c * apk - s * aqk;
          A[q * 4 + k] = s * apk + c * aqk;
        }
        A[p * 4 + q] = A[q * 4 + p] = 0.0;
        for (int k = 0; k < 4; ++k) {               // V <- V J
          const double vkp = V[k * 4 + p], vkq = V[k * 4 + q];
          V[k * 4 + p] = c * vkp - s * vkq;
          V[k * 4 + q] = s * vkp + c * vkq;
        }
      }
    }
    if (!rotated) break;
  }
  for (int i = 0; i < 4; ++i) lam[i] = A[i * 5];
}

// R (row-major 3 x 3) of the quaternion q = (q0, qx, qy, qz), normalised here
DC_HD void quat_to_matrix(const double* q, double* R) {
  const double n = sqrt((q[0] * q[0] + q[1] * q[1]) + (q[2] * q[2] + q[3] * q[3]));
  const double w = q[0] / n, x = q[1] / n, y = q[2] / n, z = q[3] / n;
  R[0] = 1.0 - 2.0 * (y * y + z * z);  R[1] = 2.0 * (x * y - w * z);        R[2] = 2.0 * (x * z + w * y);
  R[3] = 2.0 * (x * y + w * z);        R[4] = 1.0 - 2.0 * (x * x + z * z);  R[5] = 2.0 * (y * z - w * x);
  R[6] = 2.0 * (x * z - w * y);        R[7] = 2.0 * (y * z + w * x);        R[8] = 1.0 - 2.0 * (x * x + y * y);
}

// Angle of the rotation Ra Rb^T (both row-major with row stride `lda` / `ldb`): atan2(|axial vector|, (trace - 1) / 2).  Unlike the
// arccos of rotation_angle4 it resolves angles far below sqrt(eps): the axial vector of a small rotation is the angle itself.
DC_HD double rotation_angle_between(const double* Ra, int lda, const double* Rb, int ldb) {
  double D[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j)
      D[i * 3 + j] = (Ra[i * lda] * Rb[j * ldb] + Ra[i * lda + 1] * Rb[j * ldb + 1]) + Ra[i * lda + 2] * Rb[j * ldb + 2];
  const double vx = 0.5 * (D[7] - D[5]), vy = 0.5 * (D[2] - D[6]), vz = 0.5 * (D[3] - D[1]);
  const double sn = sqrt((vx * vx + vy * vy) + vz * vz), cs = 0.5 * (((D[0] + D[4]) + D[8]) - 1.0);
  return atan2(sn, cs);
}

// The closed-form fit from the totals tot [DC_ALIGN_PARTIALS] and the origins o [6] = (o_p, o_y): T (row-major 4 x 4) <- [R t] with
// t = (o_y + b / W) - R (o_p + a / W); lam [4] the eigenvalues of Horn's matrix in descending order.  Returns 0, or 1 when the
// rotation is not unique: lam1 - lam2 <= kAlignRelEps max|lam| (collinear pairs), or max|lam| is itself within the rounding of the
// moments it was formed from (coincident pairs: C is what the cancellation of S against a b^T / W left).  W > 0 is the caller's.
DC_HD int align_solve(const double* tot, const double* o, double* T, double* lam) {
  const double W = tot[0];
  const double* a = tot + 1;
  const double* b = tot + 4;
  const double* S = tot + 7;
  double C[9], N[16], V[16], ev[4], scale = 0.0;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      const double ab = a[i] * b[j] / W;
      C[i * 3 + j] = S[i * 3 + j] - ab;
      scale = fmax(scale, fmax(fabs(S[i * 3 + j]), fabs(ab)));
    }
  horn_matrix(C, N);
  jacobi4(N, ev, V);
  int order[4] = {0, 1, 2, 3};
  for (int i = 1; i < 4; ++i)                       // insertion sort, descending; equal values keep their order
    for (int j = i; j > 0 && ev[order[j]] > ev[order[j - 1]]; --j) { const int s = order[j]; order[j] = order[j - 1]; order[j - 1] = s; }
  double amax = 0.0;
  for (int i = 0; i < 4; ++i) { lam[i] = ev[order[i]]; amax = fmax(amax, fabs(ev[i])); }
  const int k = order[0];
  double q[4] = {V[k], V[4 + k], V[8 + k], V[12 + k]};
  if (q[0] < 0.0) { q[0] = -q[0]; q[1] = -q[1]; q[2] = -q[2]; q[3] = -q[3]; }
  double R[9];
  quat_to_matrix(q, R);
  const double mp[3] = {o[0] + a[0] / W, o[1] + a[1] / W, o[2] + a[2] / W};
  const double my[3] = {o[3] + b[0] / W, o[4] + b[1] / W, o[5] + b[2] / W};
  for (int r = 0; r < 3; ++r) {
    T[r * 4] = R[r * 3]; T[r * 4 + 1] = R[r * 3 + 1]; T[r * 4 + 2] = R[r * 3 + 2];
    T[r * 4 + 3] = my[r] - ((R[r * 3] * mp[0] + R[r * 3 + 1] * mp[1]) + R[r * 3 + 2] * mp[2]);
  }
  T[12] = T[13] = T[14] = 0.0;
  T[15] = 1.0;
  if (lam[0] - lam[1] <= kAlignRelEps * amax) return 1;
  if (amax <= 64.0 * 2.220446049250313e-16 * scale) return 1;
  return 0;
}

// The single-thread tail of dc_align_finish once the totals of an iteration are complete.  Counts the iteration, records pairs / rms
// in the state and the history row hist [DC_ALIGN_HISTORY_COLS] = {W, sqrt(E / W), threshold, d_rot, d_trans} (NaN where not
// reached), then in this order: DC_ALIGN_FAIL_PAIRS, DC_ALIGN_FAIL_DEGENERATE, DC_ALIGN_FAIL_NONFINITE (each leaves the estimate as it
// was; moments that are not finite cannot be degenerate and go to FAIL_NONFINITE without a solve), the estimate updated,
// DC_ALIGN_CONVERGED (d_rot < min_rot and d_trans < min_trans, strict), DC_ALIGN_MAX_ITERS.  A status word that is already set is
// the caller's to test: this function is not called then.
DC_HD void align_finish_tail(const double* tot, const double* o, const AlignParams& prm, double* st, int32_t* status, double* hist) {
  const double nan = NAN;
  const int iter = status[1] + 1;
  status[1] = iter;
  const double W = tot[0], rms = sqrt(tot[16] / W);
  st[DC_ALIGN_STATE_PAIRS] = W;
  st[DC_ALIGN_STATE_RMS] = rms;
  st[DC_ALIGN_STATE_D_ROT] = nan;
  st[DC_ALIGN_STATE_D_TRANS] = nan;
  if (hist) { hist[0] = W; hist[1] = rms; hist[2] = st[DC_ALIGN_STATE_THRESHOLD]; hist[3] = nan; hist[4] = nan; }
  if (W < (double)prm.min_pairs) { status[0] = DC_ALIGN_FAIL_PAIRS; return; }
  bool finite = true;
  for (int q = 0; q < DC_ALIGN_PARTIALS; ++q) finite = finite && isfinite(tot[q]);
  for (int q = 0; q < 6; ++q) finite = finite && isfinite(o[q]);
  if (!finite) { status[0] = DC_ALIGN_FAIL_NONFINITE; return; }
  double Tn[16], lam[4];
  if (align_solve(tot, o, Tn, lam)) { status[0] = DC_ALIGN_FAIL_DEGENERATE; return; }
  const double* Tk = st + DC_ALIGN_STATE_POSE;
  const double d_rot = rotation_angle_between(Tn, 4, Tk, 4);
  double dt[3];
  for (int r = 0; r < 3; ++r) {
    const double xn = ((Tn[r * 4] * o[0] + Tn[r * 4 + 1] * o[1]) + Tn[r * 4 + 2] * o[2]) + Tn[r * 4 + 3];
    const double xk = ((Tk[r * 4] * o[0] + Tk[r * 4 + 1] * o[1]) + Tk[r * 4 + 2] * o[2]) + Tk[r * 4 + 3];
    dt[r] = xn - xk;
  }
  const double d_trans = sqrt((dt[0] * dt[0] + dt[1] * dt[1]) + dt[2] * dt[2]);
  for (int q = 0; q < 12; ++q) finite = finite && isfinite(Tn[q]);
  finite = finite && isfinite(d_rot) && isfinite(d_trans);
  if (!finite) { status[0] = DC_ALIGN_FAIL_NONFINITE; return; }
  for (int q = 0; q < 16; ++q) st[DC_ALIGN_STATE_POSE + q] = Tn[q];
  st[DC_ALIGN_STATE_D_ROT] = d_rot;
  st[DC_ALIGN_STATE_D_TRANS] = d_trans;
  if (hist) { hist[3] = d_rot; hist[4] = d_trans; }
  if (d_rot < prm.min_rot && d_trans < prm.min_trans) { status[0] = DC_ALIGN_CONVERGED; return; }
  if (iter >= prm.max_iters) status[0] = DC_ALIGN_MAX_ITERS;
}

}  // namespace dc
