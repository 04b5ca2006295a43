// p3p_math.h — absolute pose from 2D-3D matches: the sample rows, the P3P hypothesis and the score of a model.
//
// These inline functions are the bodies of the kernel in absolute_pose.hip. Like tri_math.h they are
// __host__ __device__, so tests/ can compile this header with g++ and check it without a GPU.
// There is no CPU path in the library: nothing here iterates over a batch.
//
// What is evaluated (reference file:line):
//   samples       src/util/estimation.cc:71-93: four distinct indices, used in ascending order (std::set); the
//                 generator, the dynamic trial limit and the selection among the trials are ransac_core.h's
//   hypothesis    P3PEstimator::estimate, src/base3d/p3p.cc:26-169, with poly_solve (Durand-Kerner),
//                 src/util/math.cc:52-87, and Eigen::umeyama(src, dst, false)
//   score         P3PEstimator::residuals, src/base3d/p3p.cc:172-199, and src/util/estimation.cc:104-117
//   rvec          Eigen::AngleAxisd(R), angle times axis, src/sfm/sequential_mapper.cc:710-712
//
// Everything up to the model is evaluated operation for operation as written, without fused multiply-adds
// (MAVBA_TRI_AS_WRITTEN): it needs only + - * / and sqrt, which round the same on the host and on the device, so the
// device build's models are the host build's. Gao's formulas cancel heavily; a contraction would change every digit
// that the cancellation leaves.
#ifndef MAVBA_P3P_MATH_H_
#define MAVBA_P3P_MATH_H_

#include <float.h>
#include <stdint.h>

#include "ransac_core.h"
#include "tri_math.h"

namespace mavba {

constexpr int kAbsposeOk = 0, kAbsposeNoConsensus = 1;  // MAVBA_ABSPOSE_* (absolute_pose.hip asserts that they are equal)

// ---------------------------------------------------------------------------
// Samples (the generator is ransac_core.h's; the row is used in ascending order)
// ---------------------------------------------------------------------------
MAVBA_HD void p3p_sort4(int& a0, int& a1, int& a2, int& a3) {
  cswap(a0, a1); cswap(a2, a3); cswap(a0, a2); cswap(a1, a3); cswap(a1, a2);
}

// The row of trial `trial` for n >= 4 points (the call needs n >= 5), ascending.
MAVBA_HD void p3p_draw_sample(unsigned long long seed, unsigned trial, unsigned n, int& a0, int& a1, int& a2, int& a3) {
  int a[4];
  ransac_draw_row<4>(seed, trial, n, a);
  a0 = a[0]; a1 = a[1]; a2 = a[2]; a3 = a[3];
  p3p_sort4(a0, a1, a2, a3);
}

// ---------------------------------------------------------------------------
// Hypothesis
// ---------------------------------------------------------------------------
// What the candidates of one trial share: the bearing vectors, the constants of Gao's system and the four roots.
struct P3PSetup {
  double u[3], v[3], w[3];     // unit bearing vectors of A, B, C
  double cos_uv, dist_AB;
  double a, b, p, q, r;
  double re[4], im[4];         // roots of the quartic in x, in poly_solve's order
};

MAVBA_HD void p3p_bearing(double x, double y, double* o) {
  MAVBA_TRI_AS_WRITTEN
  const double N = sqrt(x * x + y * y + 1.0);
  o[0] = x / N; o[1] = y / N; o[2] = 1.0 / N;
}

MAVBA_HD double p3p_dist(const double* P, const double* Q) {
  MAVBA_TRI_AS_WRITTEN
  const double d0 = P[0] - Q[0], d1 = P[1] - Q[1], d2 = P[2] - Q[2];
  return sqrt(d0 * d0 + d1 * d1 + d2 * d2);
}

// poly_solve for degree 4: Durand-Kerner from the reference's starting values 1, (1+i), (1+i)^2, (1+i)^3, each root
// updated in turn with the roots already updated, at most 100 sweeps, ends when the largest correction is <= 1e-10.
// c[k] is the coefficient of x^k. NaN coefficients end it too (a NaN correction never raises the maximum).
MAVBA_HD int p3p_quartic_roots(const double* c, double* re, double* im) {
  MAVBA_TRI_AS_WRITTEN
  // (the four roots are named scalars and the update is written out per root: an indexed array would leave the registers)
  double r0 = 1.0, i0 = 0.0, r1 = 1.0, i1 = 1.0, r2 = 0.0, i2 = 2.0, r3 = -2.0, i3 = 2.0;
  const double c0 = c[0], c1 = c[1], c2 = c[2], c3 = c[3], c4 = c[4];
  int iter = 0;
  for (; iter < 100; ++iter) {
    double max_diff = 0.0;
// num = Horner at p; d = c4 (p - a)(p - b)(p - c) over the other roots in index order; p -= num / d
#define MAVBA_P3P_DK(PR, PI, AR, AI, BR, BI, CR, CI)                                              \
  {                                                                                               \
    const double pr = PR, pi = PI;                                                                \
    double nr = c4, ni = 0.0, dr = c4, di = 0.0, tr, ti;                                          \
    tr = nr * pr - ni * pi; ti = nr * pi + ni * pr; nr = tr + c3; ni = ti;                        \
    tr = nr * pr - ni * pi; ti = nr * pi + ni * pr; nr = tr + c2; ni = ti;                        \
    tr = nr * pr - ni * pi; ti = nr * pi + ni * pr; nr = tr + c1; ni = ti;                        \
    tr = nr * pr - ni * pi; ti = nr * pi + ni * pr; nr = tr + c0; ni = ti;                        \
    tr = dr * (pr - AR) - di * (pi - AI); ti = dr * (pi - AI) + di * (pr - AR); dr = tr; di = ti; \
    tr = dr * (pr - BR) - di * (pi - BI); ti = dr * (pi - BI) + di * (pr - BR); dr = tr; di = ti; \
    tr = dr * (pr - CR) - di * (pi - CI); ti = dr * (pi - CI) + di * (pr - CR); dr = tr; di = ti; \
    const double den = dr * dr + di * di;                                                         \
    const double qr = (nr * dr + ni * di) / den, qi = (ni * dr - nr * di) / den;                  \
    PR = pr - qr; PI = pi - qi;                                                                   \
    const double mag = sqrt(qr * qr + qi * qi);                                                   \
    max_diff = max_diff < mag ? mag : max_diff;                                                   \
  }
    MAVBA_P3P_DK(r0, i0, r1, i1, r2, i2, r3, i3)
    MAVBA_P3P_DK(r1, i1, r0, i0, r2, i2, r3, i3)
    MAVBA_P3P_DK(r2, i2, r0, i0, r1, i1, r3, i3)
    MAVBA_P3P_DK(r3, i3, r0, i0, r1, i1, r2, i2)
#undef MAVBA_P3P_DK
    if (max_diff <= 1e-10) break;
  }
  re[0] = r0; re[1] = r1; re[2] = r2; re[3] = r3;
  im[0] = i0; im[1] = i1; im[2] = i2; im[3] = i3;
  return iter;
}

// x2d: the four lifted observations [4][2]; X: the four world points [4][3] (rows in ascending sample order).
MAVBA_HD void p3p_setup(const double* x2d, const double* X, P3PSetup& s) {
  MAVBA_TRI_AS_WRITTEN
  p3p_bearing(x2d[0], x2d[1], s.u);
  p3p_bearing(x2d[2], x2d[3], s.v);
  p3p_bearing(x2d[4], x2d[5], s.w);
  s.cos_uv = s.u[0] * s.v[0] + s.u[1] * s.v[1] + s.u[2] * s.v[2];
  const double cos_uw = s.u[0] * s.w[0] + s.u[1] * s.w[1] + s.u[2] * s.w[2];
  const double cos_vw = s.v[0] * s.w[0] + s.v[1] * s.w[1] + s.v[2] * s.w[2];
  s.dist_AB = p3p_dist(X, X + 3);
  const double dist_AC = p3p_dist(X, X + 6), dist_BC = p3p_dist(X + 3, X + 6);
  const double dist_AB_2 = s.dist_AB * s.dist_AB;
  const double a = (dist_BC * dist_BC) / dist_AB_2, b = (dist_AC * dist_AC) / dist_AB_2;
  const double a2 = a * a, b2 = b * b;
  const double p = 2 * cos_vw, q = 2 * cos_uw, r = 2 * s.cos_uv;
  const double p2 = p * p, q2 = q * q, r2 = r * r;
  s.a = a; s.b = b; s.p = p; s.q = q; s.r = r;
  double c[5];
  c[4] = -2 * b + b2 + a2 + 1 + a * b * (2 - r2) - 2 * a;
  c[3] = -2 * q * a2 - r * p * b2 + 4 * q * a + (2 * q + p * r) * b + (r2 * q - 2 * q + r * p) * a * b - 2 * q;
  c[2] = (2 + q2) * a2 + (p2 + r2 - 2) * b2 - (4 + 2 * q2) * a - (p * q * r + p2) * b - (p * q * r + r2) * a * b + q2 + 2;
  c[1] = -2 * q * a2 - r * p * b2 + 4 * q * a + (p * r + q * p2 - 2 * q) * b + (r * p + 2 * q) * a * b - 2 * q;
  c[0] = a2 + b2 - 2 * a + (2 - p2) * b - 2 * a * b + 1;
  p3p_quartic_roots(c, s.re, s.im);
}

// y of Gao's system for a root x: b0 / b1 (p3p.cc:118-124)
MAVBA_HD double p3p_y_of_x(const P3PSetup& s, double x) {
  MAVBA_TRI_AS_WRITTEN
  const double a = s.a, b = s.b, p = s.p, q = s.q, r = s.r;
  const double a2 = a * a, b2 = b * b, p2 = p * p, p3 = p2 * p, q2 = q * q, r2 = r * r, r3 = r2 * r, r4 = r3 * r, r5 = r4 * r;
  const double x2 = x * x, x3 = x2 * x;
  const double _b1 = (p2 - p * q * r + r2) * a + (p2 - r2) * b - p2 + p * q * r - r2;
  const double b1 = b * _b1 * _b1;
  const double f1 = (1 - a - b) * x2 + (a - 1) * q * x - a + b + 1;
  const double k3 = r3 * (a2 + b2 - 2 * a - 2 * b + (2 - r2) * a * b + 1);
  const double k2 = r2 * (p + p * a2 - 2 * r * q * a * b + 2 * r * q * b - 2 * r * q - 2 * p * a - 2 * p * b + p * r2 * b + 4 * r * q * a
                          + q * r3 * a * b - 2 * r * q * a2 + 2 * p * a * b + p * b2 - r2 * p * b2);
  const double k1 = r5 * (b2 - a * b) - r4 * p * q * b + r3 * (q2 - 4 * a - 2 * q2 * a + q2 * a2 + 2 * a2 - 2 * b2 + 2)
                    + r2 * (4 * p * q * a - 2 * p * q * a * b + 2 * p * q * b - 2 * p * q - 2 * p * q * a2)
                    + r * (p2 * b2 - 2 * p2 * b + 2 * p2 * a * b - 2 * p2 * a + p2 + p2 * a2);
  const double b0 = f1 * (k3 * x3 + k2 * x2 + k1 * x
                          + (2 * p * r2 - 2 * r3 * q + p3 - 2 * p2 * q * r + p * q2 * r2) * a2 + (p3 - 2 * p * r2) * b2
                          + (4 * q * r3 - 4 * p * r2 - 2 * p3 + 4 * p2 * q * r - 2 * p * q2 * r2) * a
                          + (-2 * q * r3 + p * r4 + 2 * p2 * q * r - 2 * p3) * b + (2 * p3 + 2 * q * r3 - 2 * p2 * q * r) * a * b
                          + p * q2 * r2 - 2 * p2 * q * r + 2 * p * r2 + p3 - 2 * r3 * q);
  return b0 / b1;
}

// One Hestenes rotation on two columns of a 3 x 3 matrix and of V (tri_jacobi_pair for three rows; tol = sqrt(3) eps).
MAVBA_HD bool p3p_jacobi_pair(double* ap, double* aq, double* vp, double* vq) {
  MAVBA_TRI_AS_WRITTEN
  const double alpha = ap[0] * ap[0] + ap[1] * ap[1] + ap[2] * ap[2];
  const double beta = aq[0] * aq[0] + aq[1] * aq[1] + aq[2] * aq[2];
  const double gamma = ap[0] * aq[0] + ap[1] * aq[1] + ap[2] * aq[2];
  if (!(gamma * gamma > 1.4791141972893971e-31 * (alpha * beta))) return false;
  const double zeta = (beta - alpha) / (2.0 * gamma);
  const double t = (zeta < 0.0 ? -1.0 : 1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
  const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
#define MAVBA_P3P_ROT(P, Q) { const double x_ = (P), y_ = (Q); (P) = c * x_ - s * y_; (Q) = s * x_ + c * y_; }
  MAVBA_P3P_ROT(ap[0], aq[0]) MAVBA_P3P_ROT(ap[1], aq[1]) MAVBA_P3P_ROT(ap[2], aq[2])
  MAVBA_P3P_ROT(vp[0], vq[0]) MAVBA_P3P_ROT(vp[1], vq[1]) MAVBA_P3P_ROT(vp[2], vq[2])
#undef MAVBA_P3P_ROT
  return true;
}

MAVBA_HD void p3p_cross(const double* a, const double* b, double* o) {
  MAVBA_TRI_AS_WRITTEN
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}

MAVBA_HD void p3p_unit(double* a) {
  MAVBA_TRI_AS_WRITTEN
  const double n = sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
  a[0] /= n; a[1] /= n; a[2] /= n;
}

// (e1, e2) -> the right-handed orthonormal frame (e1, e2', e3) with e3 = e1 x e2 / |.|, e2' = e3 x e1
MAVBA_HD void p3p_frame(double* e1, double* e2, double* e3) {
  p3p_unit(e1);
  p3p_cross(e1, e2, e3);
  p3p_unit(e3);
  p3p_cross(e3, e1, e2);
}

constexpr int kP3PMaxSweeps = 12;  // as kTriMaxSweeps: the rotations end after 3-5 sweeps, the cap bounds the loop for any input

// Eigen::umeyama(src, dst, false) for three points: the rotation R and translation t that fit dst ~ R src + t in
// the least-squares sense. src[k], dst[k]: point k. sigma = (1/3) sum dst_c src_c^T = U S V^T; three points span a
// plane, so sigma has rank two and Eigen's rank-deficient branch applies: R = U diag(1, 1, det U det V) V^T, which is
//   R = u1 v1^T + u2 v2^T + (u1 x u2)(v1 x v2)^T
// for the two leading singular pairs. They come from a one-sided Jacobi iteration on sigma's columns (sigma V = U S),
// in registers; the column of the smallest norm is the one left out. M = [R | t] row-major 3 x 4.
MAVBA_HD void p3p_rigid_fit(const double (*src)[3], const double (*dst)[3], double* M) {
  MAVBA_TRI_AS_WRITTEN
  const double third = 1.0 / 3.0;
  double sm[3], dm[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    sm[k] = (src[0][k] + src[1][k] + src[2][k]) * third;
    dm[k] = (dst[0][k] + dst[1][k] + dst[2][k]) * third;
  }
  double A[3][3];  // A[c] = column c of sigma
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int r = 0; r < 3; ++r)
      A[c][r] = third * ((dst[0][r] - dm[r]) * (src[0][c] - sm[c]) + (dst[1][r] - dm[r]) * (src[1][c] - sm[c]) + (dst[2][r] - dm[r]) * (src[2][c] - sm[c]));
  double V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
  for (int sweep = 0; sweep < kP3PMaxSweeps; ++sweep) {
    bool any = p3p_jacobi_pair(A[0], A[1], V[0], V[1]);
    any = p3p_jacobi_pair(A[0], A[2], V[0], V[2]) || any;
    any = p3p_jacobi_pair(A[1], A[2], V[1], V[2]) || any;
    if (!any) break;
  }
  double n[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) n[c] = A[c][0] * A[c][0] + A[c][1] * A[c][1] + A[c][2] * A[c][2];
  // the two columns of the larger norms into u1 / u2 (v1 / v2)
  const bool drop0 = n[0] < n[1] && n[0] < n[2], drop1 = !drop0 && n[1] < n[2];
  double u1[3], u2[3], u3[3], v1[3], v2[3], v3[3];
#define MAVBA_P3P_PICK(R)                                                     \
  {                                                                           \
    const double a0_ = A[0][R], a1_ = A[1][R], a2_ = A[2][R];                 \
    const double w0_ = V[0][R], w1_ = V[1][R], w2_ = V[2][R];                 \
    u1[R] = drop0 ? a2_ : a0_; v1[R] = drop0 ? w2_ : w0_;                     \
    u2[R] = drop1 ? a2_ : a1_; v2[R] = drop1 ? w2_ : w1_;                     \
  }
  MAVBA_P3P_PICK(0) MAVBA_P3P_PICK(1) MAVBA_P3P_PICK(2)
#undef MAVBA_P3P_PICK
  p3p_unit(u2);
  p3p_frame(u1, u2, u3);
  p3p_frame(v1, v2, v3);
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) M[4 * r + c] = u1[r] * v1[c] + u2[r] * v2[c] + u3[r] * v3[c];
  }
#pragma unroll
  for (int r = 0; r < 3; ++r) M[4 * r + 3] = dm[r] - (M[4 * r] * sm[0] + M[4 * r + 1] * sm[1] + M[4 * r + 2] * sm[2]);
}

// Reprojection residual of the world point X under M = [R | t] against the lifted observation (x, y): p3p.cc:190-195.
MAVBA_HD double p3p_residual(const double* M, double X, double Y, double Z, double x, double y) {
  MAVBA_TRI_AS_WRITTEN
  double p0 = (M[0] * X + M[1] * Y + M[2] * Z) + M[3];
  double p1 = (M[4] * X + M[5] * Y + M[6] * Z) + M[7];
  const double p2 = (M[8] * X + M[9] * Y + M[10] * Z) + M[11];
  p0 /= p2;
  p1 /= p2;
  const double dx = p0 - x, dy = p1 - y;
  return sqrt(dx * dx + dy * dy);
}

MAVBA_HD bool p3p_finite(double v) { return v - v == 0.0; }

// v[k] for a k known only at run time, on the bit patterns: a chain of conditional expressions over the members of a
// record becomes an indexed load, and the record then leaves the registers
MAVBA_HD double p3p_pick4(int k, double v0, double v1, double v2, double v3) {
  unsigned long long b0, b1, b2, b3;
  __builtin_memcpy(&b0, &v0, 8); __builtin_memcpy(&b1, &v1, 8); __builtin_memcpy(&b2, &v2, 8); __builtin_memcpy(&b3, &v3, 8);
  const unsigned long long b = (b0 & (0ull - (unsigned long long)(k == 0))) | (b1 & (0ull - (unsigned long long)(k == 1)))
                               | (b2 & (0ull - (unsigned long long)(k == 2))) | (b3 & (0ull - (unsigned long long)(k == 3)));
  double v;
  __builtin_memcpy(&v, &b, 8);
  return v;
}

// Candidate `cand` (root number) of a trial: false when the reference skips the root. Otherwise M and the
// reprojection error of D (which may be NaN: such a candidate never wins).
MAVBA_HD bool p3p_candidate(const P3PSetup& s, const double* x2d, const double* X, int cand, double* M, double& err) {
  MAVBA_TRI_AS_WRITTEN
  const double x = p3p_pick4(cand, s.re[0], s.re[1], s.re[2], s.re[3]);
  const double xi = p3p_pick4(cand, s.im[0], s.im[1], s.im[2], s.im[3]);
  if (xi > 1e-10 || x < 0) return false;
  const double y = p3p_y_of_x(s, x);
  const double x2 = x * x, y2 = y * y;
  const double nu = x2 + y2 - 2 * x * y * s.cos_uv;
  const double dist_PC = s.dist_AB / sqrt(nu);
  const double dist_PB = y * dist_PC;
  const double dist_PA = x * dist_PC;
  double cam[3][3];
#pragma unroll
  for (int k = 0; k < 3; ++k) { cam[0][k] = s.u[k] * dist_PA; cam[1][k] = s.v[k] * dist_PB; cam[2][k] = s.w[k] * dist_PC; }
  const double world[3][3] = {{X[0], X[1], X[2]}, {X[3], X[4], X[5]}, {X[6], X[7], X[8]}};
  p3p_rigid_fit(world, cam, M);
  // (model * D with D = (X, 1): the four products summed left to right)
  double z0 = M[0] * X[9] + M[1] * X[10] + M[2] * X[11] + M[3];
  double z1 = M[4] * X[9] + M[5] * X[10] + M[6] * X[11] + M[7];
  const double z2 = M[8] * X[9] + M[9] * X[10] + M[10] * X[11] + M[11];
  z0 /= z2;
  z1 /= z2;
  const double dx = z0 - x2d[6], dy = z1 - x2d[7];
  err = sqrt(dx * dx + dy * dy);
  return true;
}

MAVBA_HD bool p3p_model_finite(const double* M) {
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 12; ++k) ok = ok && p3p_finite(M[k]);
  return ok;
}

// The whole hypothesis on one thread (the kernel spreads the candidates over four lanes and takes the same
// minimum: the smallest error, of equal ones the lowest root number). Returns false for an invalid trial (M = NaN).
MAVBA_HD bool p3p_estimate(const double* x2d, const double* X, double* M) {
  P3PSetup s;
  p3p_setup(x2d, X, s);
  double best = DBL_MAX;
  bool have = false;
  for (int cand = 0; cand < 4; ++cand) {
    double Mc[12], err;
    if (!p3p_candidate(s, x2d, X, cand, Mc, err)) continue;
    if (err < best) {
      best = err;
      have = true;
      for (int k = 0; k < 12; ++k) M[k] = Mc[k];
    }
  }
  if (have && p3p_model_finite(M)) return true;
  for (int k = 0; k < 12; ++k) M[k] = NAN;
  return false;
}

// Selection and trial limit: ransac_core.h's with one model per trial, the trial's own `valid` flag and samples of four.
using P3PSelect = RansacSelect;
MAVBA_HD bool p3p_select_step(P3PSelect& s, int t, bool valid, int count, double sum, int limit, long long stop) { return ransac_select_step(s, t, 0, valid, count, sum, limit, stop); }
inline int p3p_dynamic_limit(long long k, long long n, double probability) { return ransac_dynamic_limit(k, n, 4, probability); }

// ---------------------------------------------------------------------------
// rvec
// ---------------------------------------------------------------------------
// One branch of Eigen's quaternion-from-matrix for the largest diagonal entry i (j, k the next two, cyclic).
template <int I, int J, int K>
MAVBA_HD void p3p_quat_branch(const double* M, double* q /* x y z w */) {
  double t = sqrt(M[4 * I + I] - M[4 * J + J] - M[4 * K + K] + 1.0);
  q[I] = 0.5 * t;
  t = 0.5 / t;
  q[3] = (M[4 * K + J] - M[4 * J + K]) * t;
  q[J] = (M[4 * J + I] + M[4 * I + J]) * t;
  q[K] = (M[4 * K + I] + M[4 * I + K]) * t;
}

// Eigen::AngleAxisd(R): the quaternion of R, angle = 2 atan2(|vec|, |w|), axis = vec / (+-|vec|); rvec = angle * axis.
MAVBA_HD void p3p_rvec_from_model(const double* M, double* rvec) {
  double q[4];
  const double tr = M[0] + M[5] + M[10];
  if (tr > 0.0) {
    double t = sqrt(tr + 1.0);
    q[3] = 0.5 * t;
    t = 0.5 / t;
    q[0] = (M[9] - M[6]) * t;
    q[1] = (M[2] - M[8]) * t;
    q[2] = (M[4] - M[1]) * t;
  } else if (M[5] > M[0] && !(M[10] > M[5])) {
    p3p_quat_branch<1, 2, 0>(M, q);
  } else if (M[10] > M[0] && M[10] > M[5]) {
    p3p_quat_branch<2, 0, 1>(M, q);
  } else {
    p3p_quat_branch<0, 1, 2>(M, q);
  }
  double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]);
  if (n != 0.0) {
    const double angle = 2.0 * atan2(n, fabs(q[3]));
    if (q[3] < 0.0) n = -n;
    rvec[0] = angle * (q[0] / n); rvec[1] = angle * (q[1] / n); rvec[2] = angle * (q[2] / n);
  } else {
    rvec[0] = rvec[1] = rvec[2] = 0.0;  // (angle 0 times the axis (1, 0, 0))
  }
}

}  // namespace mavba
#endif  // MAVBA_P3P_MATH_H_
