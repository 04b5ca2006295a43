// tri_math.h — per-correspondence maths of two-view triangulation and its acceptance tests.
//
// These inline functions are the bodies of the kernel in triangulate.hip. Like ba_math.h they are
// __host__ __device__, so tests/ can compile this header with g++ and check it without a GPU.
// There is no CPU path in the library: nothing here iterates over a batch.
//
// What is evaluated (reference file:line):
//   image2world   src/base3d/camera_models.h:132-145 (PINHOLE), :195-223 (OPENCV), :304-338 (CATA), the division by z of
//                 camera_model_image2world, src/base3d/camera_models.cc:24-44, the threshold conversion :47-52
//   DLT           triangulate_point, src/base3d/triangulation.cc:18-48: the 6 x 4 matrix of  x × (P X) = 0  for both
//                 images, homogeneous point = right singular vector of the smallest singular value
//   angle         calc_tri_angles, src/base3d/triangulation.cc:101-147 (law of cosines, NaN -> 0)
//   reprojection  calc_reproj_errors, src/base3d/projection.cc:107-130 (normalised coordinates)
//   depth         calc_depth, src/base3d/projection.cc:133-149 (w times the norm of the third column, as written)
//   acceptance    src/sfm/sequential_mapper.cc:755-810 (map extension), :302-349 (initial pair)
#ifndef MAVBA_TRI_MATH_H_
#define MAVBA_TRI_MATH_H_

#include "ba_math.h"

namespace mavba {

// status bits (the MAVBA_TRI_* constants of include/mavba_triangulate.h; triangulate.hip asserts that they are equal)
constexpr int kTriReproj = 1, kTriAngle = 2, kTriDepth2 = 4, kTriDepth1 = 8;

constexpr double kTriPi = 3.14159265358979323846;

// The inverse camera models and the quantities the thresholds are applied to are evaluated operation for operation as written, without fused
// multiply-adds: the device build then rounds every step as the host build does (division and square root are correctly
// rounded on both), and a correspondence gets the same verdict on either side unless the library's acos differs.
#if defined(__clang__)
#define MAVBA_TRI_AS_WRITTEN _Pragma("clang fp contract(off)")
#else
#define MAVBA_TRI_AS_WRITTEN
#endif

// ---------------------------------------------------------------------------
// Inverse camera models
// ---------------------------------------------------------------------------
// distortion() of the OPENCV and CATA models (camera_models.h:225-242, :340-357)
MAVBA_HD void tri_distortion(const double* cam, double u, double v, double& du, double& dv) {
  MAVBA_TRI_AS_WRITTEN
  const double k1 = cam[4], k2 = cam[5], p1 = cam[6], p2 = cam[7];
  const double u2 = u * u, uy = u * v, y2 = v * v;
  const double r2 = u2 + y2;
  const double radial = k1 * r2 + k2 * r2 * r2;
  du = u * radial + 2.0 * p1 * uy + p2 * (r2 + 2.0 * u2);
  dv = v * radial + 2.0 * p2 * uy + p1 * (r2 + 2.0 * y2);
}

// Pixel -> ray (x, y, z) of the model, then (x / z, y / z) as camera_model_image2world does for the mapper.
MAVBA_HD void image2world(int model, const double* cam, double u, double v, double& xn, double& yn) {
  MAVBA_TRI_AS_WRITTEN
  double x = (u - cam[2]) / cam[0];
  double y = (v - cam[3]) / cam[1];
  double z = 1.0;
  if (model != MAVBA_M_PINHOLE) {
    // recursive inverse distortion: ten fixed-point iterations, no convergence test (the reference's)
    double xx = x, yy = y;
    for (int i = 0; i < 10; ++i) {
      double dx, dy;
      tri_distortion(cam, xx, yy, dx, dy);
      xx = x - dx;
      yy = y - dy;
    }
    x = xx; y = yy;
    if (model == MAVBA_M_CATA) {
      const double xi = cam[8];
      if (xi == 1.0) {
        z = (1.0 - xx * xx - yy * yy) / 2.0;
      } else {
        const double r2 = xx * xx + yy * yy;
        z = 1.0 - xi * (r2 + 1.0) / (xi + sqrt(1.0 + (1.0 - xi * xi) * r2));
      }
    }
  }
  xn = x / z;
  yn = y / z;
}

// camera_model_image2world_threshold: a pixel threshold in normalised coordinates
MAVBA_HD double image2world_threshold(double threshold, const double* cam) { return threshold / ((cam[0] + cam[1]) / 2.0); }

// ---------------------------------------------------------------------------
// Pair record: what both poses cost per correspondence once hoisted. The calibration is the identity, so
// compose_proj_matrix(rvec, tvec) = [R(rvec) | t].
//   rec = { P1[12] | P2[12] | C1[3] | C2[3] | baseline^2 | m1 | m2 }      P row-major 3 x 4, C = -R^T t,
//   m = norm of the third column of P (calc_depth's factor)
// ---------------------------------------------------------------------------
constexpr int kTriRec = 33;

MAVBA_HD void tri_proj_matrix(const double* rvec, const double* tvec, double* P, double* C) {
  double R[9];  // column-major
  rot_matrix_colmajor(rvec, R);
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    P[4 * r + 0] = R[r]; P[4 * r + 1] = R[3 + r]; P[4 * r + 2] = R[6 + r];
    P[4 * r + 3] = tvec[r];
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) C[c] = -(R[3 * c] * tvec[0] + R[3 * c + 1] * tvec[1] + R[3 * c + 2] * tvec[2]);
}

MAVBA_HD void tri_pair_prepare(const double* rvec1, const double* tvec1, const double* rvec2, const double* tvec2, double* rec) {
  tri_proj_matrix(rvec1, tvec1, rec, rec + 24);
  tri_proj_matrix(rvec2, tvec2, rec + 12, rec + 27);
  const double bx = rec[24] - rec[27], by = rec[25] - rec[28], bz = rec[26] - rec[29];
  const double baseline = sqrt(bx * bx + by * by + bz * bz);
  rec[30] = baseline * baseline;
  rec[31] = sqrt(rec[2] * rec[2] + rec[6] * rec[6] + rec[10] * rec[10]);
  rec[32] = sqrt(rec[14] * rec[14] + rec[18] * rec[18] + rec[22] * rec[22]);
}

// ---------------------------------------------------------------------------
// Two-view DLT
// ---------------------------------------------------------------------------
// One Hestenes rotation: makes the columns p and q of A orthogonal and applies the same rotation to V.
// Returns false when they already are, to working precision (also for a zero column and for NaN / inf input:
// every comparison with NaN is false, so such columns are never rotated and the sweep loop ends).
MAVBA_HD bool tri_jacobi_pair(double* ap, double* aq, double* vp, double* vq) {
  double alpha = 0.0, beta = 0.0, gamma = 0.0;
#pragma unroll
  for (int r = 0; r < 6; ++r) { alpha += ap[r] * ap[r]; beta += aq[r] * aq[r]; gamma += ap[r] * aq[r]; }
  // |ap . aq| <= tol |ap| |aq| with tol = sqrt(6) eps (the criterion of LAPACK's one-sided Jacobi, sqrt(m) eps)
  if (!(gamma * gamma > 2.9582283945787943e-31 * (alpha * beta))) return false;
  const double zeta = (beta - alpha) / (2.0 * gamma);
  const double t = (zeta < 0.0 ? -1.0 : 1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
  const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
#pragma unroll
  for (int r = 0; r < 6; ++r) {
    const double x = ap[r], y = aq[r];
    ap[r] = c * x - s * y;
    aq[r] = s * x + c * y;
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const double x = vp[r], y = vq[r];
    vp[r] = c * x - s * y;
    vq[r] = s * x + c * y;
  }
  return true;
}

// Sweep cap of the one-sided Jacobi iteration. Measured with the host build over the inputs of
// tests/test_triangulate_host.py (nadir pairs, baselines 3-20 at altitude 50, three model pairs, the degenerate
// cases): at most 5 sweeps rotate anything, the 6th finds every pair orthogonal. The cap leaves a factor two.
constexpr int kTriMaxSweeps = 12;

// Right singular vector of the smallest singular value of the 6 x 4 matrix A (column-major: A[4][6]), by a
// one-sided (Hestenes) Jacobi SVD on A itself: A^T A is never formed - column 3 carries the translations, tens to
// hundreds of units, and squaring it would cost half the digits (the reference uses Eigen's JacobiSVD for the same
// reason). The six column pairs are written out, so A and V stay in registers (no dynamic index).
// Returns the number of sweeps that rotated at least one pair.
MAVBA_HD int tri_null_vector(double (*A)[6], double* h) {
  double V[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};  // V[c] = column c
  int sweeps = 0;
  for (; sweeps < kTriMaxSweeps; ++sweeps) {
    bool any = tri_jacobi_pair(A[0], A[1], V[0], V[1]);
    any = tri_jacobi_pair(A[0], A[2], V[0], V[2]) || any;
    any = tri_jacobi_pair(A[0], A[3], V[0], V[3]) || any;
    any = tri_jacobi_pair(A[1], A[2], V[1], V[2]) || any;
    any = tri_jacobi_pair(A[1], A[3], V[1], V[3]) || any;
    any = tri_jacobi_pair(A[2], A[3], V[2], V[3]) || any;
    if (!any) break;
  }
  double n[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    n[c] = 0.0;
#pragma unroll
    for (int r = 0; r < 6; ++r) n[c] += A[c][r] * A[c][r];
  }
  // the column of the smallest norm; of equal ones the last, where a sorted decomposition puts it
  const bool s01 = n[1] <= n[0], s23 = n[3] <= n[2];
  const double n01 = s01 ? n[1] : n[0], n23 = s23 ? n[3] : n[2];
  const bool hi = n23 <= n01;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const double a = s01 ? V[1][r] : V[0][r], b = s23 ? V[3][r] : V[2][r];
    h[r] = hi ? b : a;
  }
  return sweeps;
}

// triangulate_point: x1, x2 in normalised coordinates, P1 / P2 row-major 3 x 4. h = the unit homogeneous vector,
// X = h[0..2] / h[3] (non-finite for a point at infinity, as in the reference).
MAVBA_HD int triangulate_dlt(const double* P1, const double* P2, double x1, double y1, double x2, double y2, double* h, double* X) {
  double A[4][6];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    A[k][0] = x1 * P1[8 + k] - P1[k];
    A[k][1] = y1 * P1[8 + k] - P1[4 + k];
    A[k][2] = x1 * P1[4 + k] - y1 * P1[k];
    A[k][3] = x2 * P2[8 + k] - P2[k];
    A[k][4] = y2 * P2[8 + k] - P2[4 + k];
    A[k][5] = x2 * P2[4 + k] - y2 * P2[k];
  }
  const int sweeps = tri_null_vector(A, h);
  X[0] = h[0] / h[3]; X[1] = h[1] / h[3]; X[2] = h[2] / h[3];
  return sweeps;
}

// ---------------------------------------------------------------------------
// Per-point quantities and the acceptance tests
// ---------------------------------------------------------------------------
// Angle between the two rays at X (radians, unfolded); NaN becomes 0.
MAVBA_HD double tri_angle(const double* rec, const double* X) {
  MAVBA_TRI_AS_WRITTEN
  const double* C1 = rec + 24;
  const double* C2 = rec + 27;
  const double a0 = X[0] - C1[0], a1 = X[1] - C1[1], a2 = X[2] - C1[2];
  const double b0 = X[0] - C2[0], b1 = X[1] - C2[1], b2 = X[2] - C2[2];
  const double ray1 = sqrt(a0 * a0 + a1 * a1 + a2 * a2);
  const double ray2 = sqrt(b0 * b0 + b1 * b1 + b2 * b2);
  const double angle = acos((ray1 * ray1 + ray2 * ray2 - rec[30]) / (2.0 * ray1 * ray2));
  return angle != angle ? 0.0 : angle;
}

// options.tri_min_angle * DEG2RAD with the reference's macro (M_PI / 180.0, unparenthesised) expanded
MAVBA_HD double tri_min_angle_rad(double deg) { return deg * kTriPi / 180.0; }

// std::min(angle, 180 * DEG2RAD - angle); 180 * M_PI / 180.0 is M_PI exactly
MAVBA_HD double tri_fold(double angle) {
  const double o = kTriPi - angle;
  return o < angle ? o : angle;
}

// Reprojection error of X against the normalised point (x, y) under P.
MAVBA_HD double tri_reproj_error(const double* P, const double* X, double x, double y) {
  MAVBA_TRI_AS_WRITTEN
  double p0 = P[0] * X[0] + P[1] * X[1] + P[2] * X[2] + P[3];
  double p1 = P[4] * X[0] + P[5] * X[1] + P[6] * X[2] + P[7];
  const double p2 = P[8] * X[0] + P[9] * X[1] + P[10] * X[2] + P[11];
  p0 /= p2;
  p1 /= p2;
  const double dx = p0 - x, dy = p1 - y;
  return sqrt(dx * dx + dy * dy);
}

// calc_depth: third row of P times (X, 1), times the norm m of P's third column
MAVBA_HD double tri_depth(const double* P, double m, const double* X) {
  MAVBA_TRI_AS_WRITTEN
  const double w = P[8] * X[0] + P[9] * X[1] + P[10] * X[2] + P[11];
  return w * m;
}

// Each bit is the negation of the reference's positive test, so NaN sets it where the reference rejects.
MAVBA_HD int tri_status(double err, double thr_n, double folded, double min_angle_rad, double depth1, double depth2) {
  int s = 0;
  if (!(err < thr_n)) s |= kTriReproj;
  if (!(min_angle_rad < folded)) s |= kTriAngle;
  if (!(depth2 > 0.0)) s |= kTriDepth2;
  if (!(depth1 > 0.0)) s |= kTriDepth1;
  return s;
}

// A continued track keeps its 3D position: only the reprojection test can reject it.
MAVBA_HD bool tri_accept(int status, bool have_xyz, int reject_bits) {
  return (status & (have_xyz ? (reject_bits & kTriReproj) : reject_bits)) == 0;
}

// One correspondence from pixels to its verdict. have_xyz: a continued track - X is xyz_in and only the
// reprojection test can reject it (sequential_mapper.cc:766-777).
// out = { X[3], angle, err, depth1, depth2 }; returns the status bits, `accept` the verdict.
MAVBA_HD int tri_correspondence(const double* rec, int model1, const double* cam1, int model2, const double* cam2, double u1, double v1,
                                double u2, double v2, bool have_xyz, const double* xyz_in, double thr_n, double min_angle_rad,
                                int reject_bits, double* out, bool& accept) {
  double x2, y2;
  image2world(model2, cam2, u2, v2, x2, y2);
  double X[3];
  if (have_xyz) {
    X[0] = xyz_in[0]; X[1] = xyz_in[1]; X[2] = xyz_in[2];
  } else {
    double x1, y1, h[4];
    image2world(model1, cam1, u1, v1, x1, y1);
    triangulate_dlt(rec, rec + 12, x1, y1, x2, y2, h, X);
  }
  const double angle = tri_angle(rec, X);
  const double err = tri_reproj_error(rec + 12, X, x2, y2);
  const double d1 = tri_depth(rec, rec[31], X), d2 = tri_depth(rec + 12, rec[32], X);
  const int status = tri_status(err, thr_n, tri_fold(angle), min_angle_rad, d1, d2);
  out[0] = X[0]; out[1] = X[1]; out[2] = X[2];
  out[3] = angle; out[4] = err; out[5] = d1; out[6] = d2;
  accept = tri_accept(status, have_xyz, reject_bits);
  return status;
}

}  // namespace mavba
#endif  // MAVBA_TRI_MATH_H_
