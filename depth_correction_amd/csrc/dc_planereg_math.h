// Plane registration: the rules of the coarse stage from plane correspondences (dc_planereg.hip; DESIGN "Plane registration"), host
// and device.  Scalars only, fp64, no fused multiply-adds; every dot product is (x0 y0 + x1 y1) + x2 y2, every determinant
// det[a b c] = (a0 (b1 c2 - b2 c1) + a1 (b2 c0 - b0 c2)) + a2 (b0 c1 - b1 c0).
//
// A plane is a row (n, d) with n.x + d = 0 and |n| = 1; the sign of n carries no meaning.  Cloud planes (n_q, d_q) with supports
// cs_q, survey planes (m_r, e_r).  The cloud triples a < b < c with |det[n_a n_b n_c]| >= min_det, in lexicographic order, are
// numbered u = 0 .. U - 1 (the caller's table); hypothesis h = (((u Ps + i) Ps + j) Ps + k) 8 + s pairs (a, b, c) with the survey
// planes (i, j, k) under the signs sigma_a, sigma_b, sigma_c = bits 0, 1, 2 of s (0: +1, 1: -1).  It is valid iff
//   1. i, j, k are distinct;
//   2. |det[m_i m_j m_k]| >= min_det;
//   3. |sigma_a sigma_b (n_a.n_b) - m_i.m_j| <= tol_dot, and likewise (a, c | i, k) and (b, c | j, k);
//   4. (sigma_a sigma_b sigma_c det[n_a n_b n_c]) det[m_i m_j m_k] > 0;
//   5. the fitted T is finite.
// Fit: M = sum_t m_t (sigma_t n_t)^T over t = a, b, c in that order; horn_matrix takes its transpose (C_ij = sum (sigma_t n_t)_i
// (m_t)_j: the rotation takes the cloud normals to the survey normals), jacobi4, the eigenvector of the largest eigenvalue (the lowest
// column among equal ones), quat_to_matrix.  The translation solves m_t . t = sigma_t d_t - e_t by Cramer's rule on the COLUMNS
// c0, c1, c2 of the matrix whose rows are m_i, m_j, m_k: D = det[c0 c1 c2], t = (det[b c1 c2], det[c0 b c2], det[c0 c1 b]) / D.
// T is survey frame from cloud frame.
// Score: the sum of cs_q over the cloud planes q for which some survey plane r has |n'_q.m_r| >= cos_tol and
// |sgn(n'_q.m_r) d'_q - e_r| <= tol_d, n'_q = R n_q (row by row), d'_q = d_q - n'_q.t, sgn(x) = +1 for x >= 0, else -1.
#pragma once
#include <math.h>
#include "dc_common.h"
#include "dc_align_math.h"

namespace dc {

constexpr int kPregMaxPlanes = 64;              // most planes a side
constexpr int kPregMinPlanes = 3;
constexpr int64_t kPregMaxTriples = 41664;      // C(64, 3): most cloud triples

struct PregParams {
  double min_det, tol_dot, cos_tol, tol_d;
};

DC_HD double preg_dot(const double* x, const double* y) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2];
}

DC_HD double preg_det3(const double* a, const double* b, const double* c) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double m0 = b[1] * c[2] - b[2] * c[1];
  const double m1 = b[2] * c[0] - b[0] * c[2];
  const double m2 = b[0] * c[1] - b[1] * c[0];
  return (a[0] * m0 + a[1] * m1) + a[2] * m2;
}

// h -> (u, i, j, k, s); h >= 0, ps in 3 .. 64
DC_HD void preg_decode(int64_t h, int ps, int64_t* u, int* i, int* j, int* k, int* s) {
  *s = (int)(h & 7);
  int64_t r = h >> 3;
  *k = (int)(r % ps); r /= ps;
  *j = (int)(r % ps); r /= ps;
  *i = (int)(r % ps);
  *u = r / ps;
}

DC_HD double preg_sign(int s, int bit) { return ((s >> bit) & 1) ? -1.0 : 1.0; }

// Rules 2 to 4 of the pairing (na, nb, nc | mi, mj, mk) under the signs s; rule 1 is the caller's (it needs no plane).  A NaN anywhere
// fails a comparison, so the hypothesis is not valid.
DC_HD int preg_check(const double* na, const double* nb, const double* nc, const double* mi, const double* mj, const double* mk, int s,
                     double min_det, double tol_dot) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double dm = preg_det3(mi, mj, mk);
  if (!(fabs(dm) >= min_det)) return 0;
  const double sa = preg_sign(s, 0), sb = preg_sign(s, 1), sc = preg_sign(s, 2);
  if (!(fabs((sa * sb) * preg_dot(na, nb) - preg_dot(mi, mj)) <= tol_dot)) return 0;
  if (!(fabs((sa * sc) * preg_dot(na, nc) - preg_dot(mi, mk)) <= tol_dot)) return 0;
  if (!(fabs((sb * sc) * preg_dot(nb, nc) - preg_dot(mj, mk)) <= tol_dot)) return 0;
  const double dn = ((sa * sb) * sc) * preg_det3(na, nb, nc);
  return dn * dm > 0.0 ? 1 : 0;
}

// The closed-form fit of the pairing (rows of 4: n, d and m, e): T [16] row-major 4 x 4.  Returns 1 when every entry is finite (rule 5).
DC_HD int preg_fit(const double* pa, const double* pb, const double* pc, const double* qi, const double* qj, const double* qk, int s,
                   double* T) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double sg[3] = {preg_sign(s, 0), preg_sign(s, 1), preg_sign(s, 2)};
  const double* n[3] = {pa, pb, pc};
  const double* m[3] = {qi, qj, qk};
  double C[9], N[16], V[16], lam[4];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c)
      C[r * 3 + c] = ((sg[0] * n[0][r]) * m[0][c] + (sg[1] * n[1][r]) * m[1][c]) + (sg[2] * n[2][r]) * m[2][c];
  horn_matrix(C, N);
  jacobi4(N, lam, V);
  int best = 0;
  for (int c = 1; c < 4; ++c)
    if (lam[c] > lam[best]) best = c;
  double q[4] = {V[best], V[4 + best], V[8 + best], V[12 + best]};
  if (q[0] < 0.0) { q[0] = -q[0]; q[1] = -q[1]; q[2] = -q[2]; q[3] = -q[3]; }
  double R[9];
  quat_to_matrix(q, R);
  const double c0[3] = {m[0][0], m[1][0], m[2][0]}, c1[3] = {m[0][1], m[1][1], m[2][1]}, c2[3] = {m[0][2], m[1][2], m[2][2]};
  const double b[3] = {sg[0] * n[0][3] - m[0][3], sg[1] * n[1][3] - m[1][3], sg[2] * n[2][3] - m[2][3]};
  const double D = preg_det3(c0, c1, c2);
  const double t[3] = {preg_det3(b, c1, c2) / D, preg_det3(c0, b, c2) / D, preg_det3(c0, c1, b) / D};
  bool finite = true;
  for (int r = 0; r < 3; ++r) {
    T[r * 4] = R[r * 3]; T[r * 4 + 1] = R[r * 3 + 1]; T[r * 4 + 2] = R[r * 3 + 2]; T[r * 4 + 3] = t[r];
    finite = finite && isfinite(R[r * 3]) && isfinite(R[r * 3 + 1]) && isfinite(R[r * 3 + 2]) && isfinite(t[r]);
  }
  T[12] = T[13] = T[14] = 0.0;
  T[15] = 1.0;
  return finite ? 1 : 0;
}

// The plane agreement of the cloud plane (n, d) moved by T with the survey plane (m, e): 1 or 0
DC_HD int preg_agree(const double* T, const double* p, const double* q, double cos_tol, double tol_d) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double n[3] = {preg_dot(T, p), preg_dot(T + 4, p), preg_dot(T + 8, p)};
  const double t[3] = {T[3], T[7], T[11]};
  const double d = p[3] - preg_dot(n, t);
  const double c = preg_dot(n, q);
  if (!(fabs(c) >= cos_tol)) return 0;
  const double sd = c >= 0.0 ? d : -d;
  return fabs(sd - q[3]) <= tol_d ? 1 : 0;
}

// The score of T over the tables cp [pc, 4], cs [pc], sp [ps, 4]: an exact integer, any order of the sum gives it
DC_HD int64_t preg_score(const double* T, const double* cp, const int64_t* cs, int pc, const double* sp, int ps, double cos_tol,
                         double tol_d) {
  int64_t score = 0;
  for (int q = 0; q < pc; ++q) {
    int hit = 0;
    for (int r = 0; r < ps; ++r) hit |= preg_agree(T, cp + 4 * q, sp + 4 * r, cos_tol, tol_d);
    if (hit) score += cs[q];
  }
  return score;
}

// One whole hypothesis against the tables (tri int32 [U, 3]): 1 and T [16], *score when it is valid
DC_HD int preg_hypothesis(int64_t h, const double* cp, const int64_t* cs, int pc, const double* sp, int ps, const int32_t* tri,
                          const PregParams& prm, double* T, int64_t* score) {
  int64_t u;
  int i, j, k, s;
  preg_decode(h, ps, &u, &i, &j, &k, &s);
  if (i == j || i == k || j == k) return 0;
  const int a = tri[3 * u], b = tri[3 * u + 1], c = tri[3 * u + 2];
  if (a < 0 || a >= pc || b < 0 || b >= pc || c < 0 || c >= pc) return 0;     // a table that is not this cloud's
  const double* na = cp + 4 * a;
  const double* nb = cp + 4 * b;
  const double* nc = cp + 4 * c;
  if (!preg_check(na, nb, nc, sp + 4 * i, sp + 4 * j, sp + 4 * k, s, prm.min_det, prm.tol_dot)) return 0;
  if (!preg_fit(na, nb, nc, sp + 4 * i, sp + 4 * j, sp + 4 * k, s, T)) return 0;
  *score = preg_score(T, cp, cs, pc, sp, ps, prm.cos_tol, prm.tol_d);
  return 1;
}

// Arguments every entry point refuses: plane counts outside 3 .. 64, tolerances that are not finite or negative
DC_HD int preg_args_ok(int pc, int ps, const PregParams& prm) {
  if (pc < kPregMinPlanes || pc > kPregMaxPlanes || ps < kPregMinPlanes || ps > kPregMaxPlanes) return 0;
  if (!(prm.min_det >= 0.0) || !(prm.tol_dot >= 0.0) || !(prm.tol_d >= 0.0)) return 0;
  if (!isfinite(prm.min_det) || !isfinite(prm.tol_dot) || !isfinite(prm.cos_tol) || !isfinite(prm.tol_d)) return 0;
  return 1;
}

}  // namespace dc
