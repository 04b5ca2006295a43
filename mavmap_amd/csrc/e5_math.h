// e5_math.h — relative pose from 2D-2D matches: the five-point hypothesis (up to ten essential matrices per sample),
// the Sampson score and the recovery of (R, t).
//
// These inline functions are the bodies of the kernel in relative_pose.hip. Like p3p_math.h they are
// __host__ __device__, so tests/ can compile this header with g++ and check it without a GPU.
// There is no CPU path in the library: nothing here iterates over a batch.
//
// What is evaluated (reference file:line):
//   samples       src/util/estimation.cc:71-93: five distinct indices in ascending order (std::set); the generator,
//                 the dynamic trial limit and the selection among the (trial, model) sequence are ransac_core.h's.
//                 A trial without a model never steps the selection: it updates nothing and cannot end the run
//   hypothesis    EssentialMatrixEstimator::estimate, src/base3d/essential_matrix.cc:12-128, with poly_solve
//                 (Durand-Kerner), src/util/math.cc:52-87
//   score         EssentialMatrixEstimator::residuals, src/base3d/essential_matrix.cc:131-162, and
//                 src/util/estimation.cc:104-117
//   pose          decompose_essential_matrix and pose_from_essential_matrix, src/base3d/essential_matrix.cc:165-269
//
// The reference includes two generated files for the 10 x 20 constraint matrix and for the determinant polynomial.
// Here both are formed by polynomial arithmetic on the four null-space matrices: products of linear forms in
// (x, y, z, 1) accumulated per monomial, then products of short coefficient arrays in z.
//
// A hypothesis works on a caller-provided workspace of kE5Work doubles (the kernel: LDS; the host build: the stack):
// every array that is indexed at run time lives there, so the device build needs no scratch memory.
// Everything up to the models is evaluated operation for operation as written, without fused multiply-adds
// (MAVBA_TRI_AS_WRITTEN), so the device build's models are the host build's.
#ifndef MAVBA_E5_MATH_H_
#define MAVBA_E5_MATH_H_

#include "p3p_math.h"
#include "tri_math.h"

namespace mavba {

constexpr int kRelposeOk = 0, kRelposeNoConsensus = 1;  // MAVBA_RELPOSE_* (relative_pose.hip asserts that they are equal)
constexpr int kE5MaxModels = 10;

// Workspace layout (doubles)
constexpr int kE5Basis = 0;     // [4][9]  X, Y, Z, W: an orthonormal basis of the null space of Q
constexpr int kE5A = 36;        // [10][20] the cubic constraints, then their reduced form
constexpr int kE5Tmp = 236;     // [60]    Q^T [9][5] + the five Householder factors; then the six quadrics of E E^T
constexpr int kE5B = 296;       // [3][13] B(z): per row 4 + 4 + 5 coefficients, ascending powers of z
constexpr int kE5Poly = 335;    // [11]    det B(z), c[k] the coefficient of z^k
constexpr int kE5Re = 346;      // [10]    roots
constexpr int kE5Im = 356;      // [10]
constexpr int kE5T1 = 366;      // [12]    a product of two polynomials
constexpr int kE5Models = 378;  // [10][9] the models, row-major, ascending z, NaN beyond the count
constexpr int kE5Z = 468;       // [10]
constexpr int kE5Work = 479;    // (odd: the workspaces of neighbouring lanes start on different LDS banks)

// ---------------------------------------------------------------------------
// Samples
// ---------------------------------------------------------------------------
MAVBA_HD void e5_sort5(int& a0, int& a1, int& a2, int& a3, int& a4) {
  cswap(a0, a1); cswap(a3, a4); cswap(a2, a4); cswap(a2, a3); cswap(a1, a4);
  cswap(a0, a3); cswap(a0, a2); cswap(a1, a3); cswap(a1, a2);
}

// The row of trial `trial` for n >= 5 points (the call needs n >= 6), ascending.
MAVBA_HD void e5_draw_sample(unsigned long long seed, unsigned trial, unsigned n, int& a0, int& a1, int& a2, int& a3, int& a4) {
  int a[5];
  ransac_draw_row<5>(seed, trial, n, a);
  a0 = a[0]; a1 = a[1]; a2 = a[2]; a3 = a[3]; a4 = a[4];
  e5_sort5(a0, a1, a2, a3, a4);
}

// ---------------------------------------------------------------------------
// Monomials. Linear forms: (x, y, z, 1) = 0..3. Quadrics: the pairs (a <= b) of those in row order,
//   x2 xy xz x y2 yz y z2 z 1 = 0..9.
// Cubics, in the column order of the elimination (the ten pivots first):
//   x3 y3 x2y xy2 x2z x2 y2z y2 xyz xy | xz2 xz x yz2 yz y z3 z2 z 1 = 0..19
// ---------------------------------------------------------------------------
MAVBA_HD constexpr int e5_q2(int a, int b) { return a <= b ? a * 4 - a * (a - 1) / 2 + (b - a) : b * 4 - b * (b - 1) / 2 + (a - b); }

// quadric q times linear l: four 5-bit fields per quadric
MAVBA_HD constexpr int e5_c3(int q, int l) {
#define MAVBA_E5_PACK(A, B, C, D) ((A) | ((B) << 5) | ((C) << 10) | ((D) << 15))
  const int w = q == 0 ? MAVBA_E5_PACK(0, 2, 4, 5) : q == 1 ? MAVBA_E5_PACK(2, 3, 8, 9) : q == 2 ? MAVBA_E5_PACK(4, 8, 10, 11)
              : q == 3 ? MAVBA_E5_PACK(5, 9, 11, 12) : q == 4 ? MAVBA_E5_PACK(3, 1, 6, 7) : q == 5 ? MAVBA_E5_PACK(8, 6, 13, 14)
              : q == 6 ? MAVBA_E5_PACK(9, 7, 14, 15) : q == 7 ? MAVBA_E5_PACK(10, 13, 16, 17) : q == 8 ? MAVBA_E5_PACK(11, 14, 17, 18)
                                                                                                        : MAVBA_E5_PACK(12, 15, 18, 19);
#undef MAVBA_E5_PACK
  return (w >> (5 * l)) & 31;
}

// entry e of E(x, y, z) = x X + y Y + z Z + W: the coefficient of linear monomial l
MAVBA_HD double e5_lin(const double* ws, int e, int l) { return ws[kE5Basis + 9 * l + e]; }

// out[10] += s * (entry ea) * (entry eb)
MAVBA_HD void e5_quad_acc(const double* ws, int ea, int eb, double s, double* out) {
  MAVBA_TRI_AS_WRITTEN
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) out[e5_q2(a, b)] += s * (e5_lin(ws, ea, a) * e5_lin(ws, eb, b));
}

// out[20] += s * quad[10] * (entry e)
MAVBA_HD void e5_cubic_acc(const double* ws, const double* quad, int e, double s, double* out) {
  MAVBA_TRI_AS_WRITTEN
#pragma unroll
  for (int q = 0; q < 10; ++q)
#pragma unroll
    for (int l = 0; l < 4; ++l) out[e5_c3(q, l)] += s * (quad[q] * e5_lin(ws, e, l));
}

// ---------------------------------------------------------------------------
// Hypothesis
// ---------------------------------------------------------------------------
// Step 1-2: Q [5][9] from the five correspondences, and an orthonormal basis of its null space: five Householder
// reflections H0 .. H4 triangularise Q^T [9][5]; the last four columns of H0 H1 H2 H3 H4 span the null space.
MAVBA_HD void e5_null_space(const double* x1, const double* x2, double* ws) {
  MAVBA_TRI_AS_WRITTEN
  double* QT = ws + kE5Tmp;       // QT[5 * r + k] = Q(k, r)
  double* beta = ws + kE5Tmp + 45;
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    const double a1 = x1[2 * k], b1 = x1[2 * k + 1], a2 = x2[2 * k], b2 = x2[2 * k + 1];
    QT[5 * 0 + k] = a1 * a2; QT[5 * 1 + k] = b1 * a2; QT[5 * 2 + k] = a2;
    QT[5 * 3 + k] = a1 * b2; QT[5 * 4 + k] = b1 * b2; QT[5 * 5 + k] = b2;
    QT[5 * 6 + k] = a1;      QT[5 * 7 + k] = b1;      QT[5 * 8 + k] = 1.0;
  }
  for (int k = 0; k < 5; ++k) {
    double nn = 0.0;
    for (int r = k; r < 9; ++r) nn += QT[5 * r + k] * QT[5 * r + k];
    double alpha = sqrt(nn);
    if (QT[5 * k + k] > 0.0) alpha = -alpha;
    QT[5 * k + k] -= alpha;  // the column now holds v
    double vtv = 0.0;
    for (int r = k; r < 9; ++r) vtv += QT[5 * r + k] * QT[5 * r + k];
    const double bk = vtv > 0.0 ? 2.0 / vtv : 0.0;  // (a zero column: no reflection)
    beta[k] = bk;
    for (int j = k + 1; j < 5; ++j) {
      double s = 0.0;
      for (int r = k; r < 9; ++r) s += QT[5 * r + k] * QT[5 * r + j];
      s *= bk;
      for (int r = k; r < 9; ++r) QT[5 * r + j] -= s * QT[5 * r + k];
    }
  }
  for (int v = 0; v < 4; ++v) {
    double* nv = ws + kE5Basis + 9 * v;
    for (int r = 0; r < 9; ++r) nv[r] = r == 5 + v ? 1.0 : 0.0;
    for (int k = 4; k >= 0; --k) {
      double s = 0.0;
      for (int r = k; r < 9; ++r) s += QT[5 * r + k] * nv[r];
      s *= beta[k];
      for (int r = k; r < 9; ++r) nv[r] -= s * QT[5 * r + k];
    }
  }
}

// Step 3: the ten cubic constraints of E = x X + y Y + z Z + W over the 20 monomials. Rows 0-8: the entries of
// (E E^T - 1/2 tr(E E^T) I) E (half of 2 E E^T E - tr(E E^T) E); row 9: det E.
MAVBA_HD void e5_constraints(double* ws) {
  MAVBA_TRI_AS_WRITTEN
  double* L = ws + kE5Tmp;  // six quadrics [10]: (0,0) (0,1) (0,2) (1,1) (1,2) (2,2) of E E^T
  double* A = ws + kE5A;
  for (int k = 0; k < 60; ++k) L[k] = 0.0;
  for (int k = 0; k < 200; ++k) A[k] = 0.0;
  int s = 0;
  for (int i = 0; i < 3; ++i)
    for (int j = i; j < 3; ++j, ++s)
      for (int k = 0; k < 3; ++k) e5_quad_acc(ws, 3 * i + k, 3 * j + k, 1.0, L + 10 * s);
  for (int m = 0; m < 10; ++m) {
    const double h = 0.5 * ((L[m] + L[30 + m]) + L[50 + m]);
    L[m] -= h; L[30 + m] -= h; L[50 + m] -= h;
  }
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j)
      for (int k = 0; k < 3; ++k) {
        const int lo = i < k ? i : k, hi = i < k ? k : i;
        const int sym = lo == 0 ? hi : (lo == 1 ? 2 + hi : 5);
        e5_cubic_acc(ws, L + 10 * sym, 3 * k + j, 1.0, A + 20 * (3 * i + j));
      }
  // det E by the first row: e00 (e11 e22 - e12 e21) - e01 (e10 e22 - e12 e20) + e02 (e10 e21 - e11 e20)
  double* T = ws + kE5T1;
  for (int c = 0; c < 3; ++c) {
    const int c1 = c == 0 ? 1 : 0, c2 = c == 2 ? 1 : 2;
    for (int m = 0; m < 10; ++m) T[m] = 0.0;
    e5_quad_acc(ws, 3 + c1, 6 + c2, 1.0, T);
    e5_quad_acc(ws, 3 + c2, 6 + c1, -1.0, T);
    e5_cubic_acc(ws, T, c, c == 1 ? -1.0 : 1.0, A + 180);
  }
}

// Step 4: Gauss-Jordan elimination with partial pivoting on the 10 x 20 matrix, pivots in columns 0-9 in order.
MAVBA_HD void e5_gauss_jordan(double* ws) {
  MAVBA_TRI_AS_WRITTEN
  double* A = ws + kE5A;
  for (int c = 0; c < 10; ++c) {
    int piv = c;
    double big = fabs(A[20 * c + c]);
    for (int r = c + 1; r < 10; ++r) {
      const double v = fabs(A[20 * r + c]);
      if (v > big) { big = v; piv = r; }
    }
    if (piv != c)
      for (int k = c; k < 20; ++k) { const double t = A[20 * c + k]; A[20 * c + k] = A[20 * piv + k]; A[20 * piv + k] = t; }
    const double d = A[20 * c + c];
    for (int k = c; k < 20; ++k) A[20 * c + k] /= d;
    for (int r = 0; r < 10; ++r) {
      if (r == c) continue;
      const double f = A[20 * r + c];
      for (int k = c; k < 20; ++k) A[20 * r + k] -= f * A[20 * c + k];
    }
  }
}

// Step 5: B(z), rows <x2z> - z <x2>, <y2z> - z <y2>, <xyz> - z <xy> (rows 4 .. 9 of the reduced matrix); per row the
// coefficients of x (degree 3), of y (degree 3) and of 1 (degree 4), each in ascending powers of z.
MAVBA_HD void e5_form_b(double* ws) {
  MAVBA_TRI_AS_WRITTEN
  const double* A = ws + kE5A;
  double* B = ws + kE5B;
  for (int j = 0; j < 3; ++j) {
    const double* p = A + 20 * (4 + 2 * j) + 10;  // xz2 xz x yz2 yz y z3 z2 z 1
    const double* q = A + 20 * (5 + 2 * j) + 10;
    double* b = B + 13 * j;
    for (int g = 0; g < 2; ++g) {
      b[4 * g + 0] = p[3 * g + 2];
      b[4 * g + 1] = p[3 * g + 1] - q[3 * g + 2];
      b[4 * g + 2] = p[3 * g + 0] - q[3 * g + 1];
      b[4 * g + 3] = -q[3 * g + 0];
    }
    b[8] = p[9];
    b[9] = p[8] - q[9];
    b[10] = p[7] - q[8];
    b[11] = p[6] - q[7];
    b[12] = -q[6];
  }
}

// out[na + nb - 1] += s * a * b (coefficient arrays, ascending)
MAVBA_HD void e5_polymul_acc(const double* a, int na, const double* b, int nb, double s, double* out) {
  MAVBA_TRI_AS_WRITTEN
  for (int i = 0; i < na; ++i)
    for (int j = 0; j < nb; ++j) out[i + j] += s * (a[i] * b[j]);
}

// Step 6: det B(z) by the first row, degree 10.
MAVBA_HD void e5_det_poly(double* ws) {
  const double* B = ws + kE5B;
  double* T = ws + kE5T1;
  double* P = ws + kE5Poly;
  for (int k = 0; k < 11; ++k) P[k] = 0.0;
  for (int c = 0; c < 3; ++c) {
    const int c1 = c == 0 ? 1 : 0, c2 = c == 2 ? 1 : 2;
    const int n1 = c1 == 2 ? 5 : 4, n2 = c2 == 2 ? 5 : 4, n0 = c == 2 ? 5 : 4;
    for (int k = 0; k < 12; ++k) T[k] = 0.0;
    e5_polymul_acc(B + 13 + 4 * c1, n1, B + 26 + 4 * c2, n2, 1.0, T);
    e5_polymul_acc(B + 13 + 4 * c2, n2, B + 26 + 4 * c1, n1, -1.0, T);
    e5_polymul_acc(B + 4 * c, n0, T, n1 + n2 - 1, c == 1 ? -1.0 : 1.0, P);
  }
}

// Step 7: poly_solve for degree 10, the reference's rule: starting values (1 + i)^k, each root updated in turn with the
// roots already updated (Gauss-Seidel, as the reference; one thread owns a trial), at most 100 sweeps, ends when the
// largest correction is <= 1e-10. A NaN correction never raises the maximum. Returns the number of sweeps.
MAVBA_HD int e5_roots(double* ws) {
  MAVBA_TRI_AS_WRITTEN
  const double* c = ws + kE5Poly;
  double* re = ws + kE5Re;
  double* im = ws + kE5Im;
  double pr = 1.0, pi = 0.0;
  for (int i = 0; i < 10; ++i) {
    re[i] = pr; im[i] = pi;
    const double tr = pr - pi, ti = pr + pi;  // times (1 + i)
    pr = tr; pi = ti;
  }
  const double lead = c[10];
  int iter = 0;
  for (; iter < 100; ++iter) {
    double max_diff = 0.0;
    for (int i = 0; i < 10; ++i) {
      pr = re[i]; pi = im[i];
      double nr = lead, ni = 0.0, dr = lead, di = 0.0;
      for (int j = 0; j < 10; ++j) {
        const double tr = nr * pr - ni * pi, ti = nr * pi + ni * pr;
        nr = tr + c[9 - j]; ni = ti;
        if (j != i) {
          const double ar = pr - re[j], ai = pi - im[j];
          const double ur = dr * ar - di * ai, ui = dr * ai + di * ar;
          dr = ur; di = ui;
        }
      }
      const double den = dr * dr + di * di;
      const double qr = (nr * dr + ni * di) / den, qi = (ni * dr - nr * di) / den;
      re[i] = pr - qr; im[i] = pi - qi;
      const double mag = sqrt(qr * qr + qi * qi);
      max_diff = max_diff < mag ? mag : max_diff;
    }
    if (max_diff <= 1e-10) break;
  }
  return iter;
}

// Step 9: the null vector of the 3 x 3 matrix B(z): the right singular vector of the smallest singular value by the
// one-sided Jacobi iteration of p3p_math.h; of equal norms the last column.
MAVBA_HD void e5_null3(const double* ws, double z, double* X) {
  MAVBA_TRI_AS_WRITTEN
  const double* B = ws + kE5B;
  double A[3][3];  // A[c] = column c
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const double* b = B + 13 * j;
    A[0][j] = ((b[3] * z + b[2]) * z + b[1]) * z + b[0];
    A[1][j] = ((b[7] * z + b[6]) * z + b[5]) * z + b[4];
    A[2][j] = (((b[12] * z + b[11]) * z + b[10]) * z + b[9]) * z + b[8];
  }
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
  const bool s01 = n[1] <= n[0];
  const double n01 = s01 ? n[1] : n[0];
  const bool last = n[2] <= n01;
#pragma unroll
  for (int r = 0; r < 3; ++r) X[r] = last ? V[2][r] : (s01 ? V[1][r] : V[0][r]);
}

// EssentialMatrixEstimator::estimate on five lifted correspondences x1, x2 [5][2] (rows in ascending sample order).
// Writes ws[kE5Models] (row-major E of unit Frobenius norm, x2^T E x1 = 0, NaN beyond the count) and ws[kE5Z], the
// models in ascending z. Returns the number of models.
MAVBA_HD int e5_estimate(const double* x1, const double* x2, double* ws) {
  MAVBA_TRI_AS_WRITTEN
  e5_null_space(x1, x2, ws);
  e5_constraints(ws);
  e5_gauss_jordan(ws);
  e5_form_b(ws);
  e5_det_poly(ws);
  e5_roots(ws);
  // Step 8: the real roots, sorted ascending (insertion; equal ones keep the root finder's order)
  double* re = ws + kE5Re;
  const double* im = ws + kE5Im;
  double* zs = ws + kE5Z;
  int nr = 0;
  for (int i = 0; i < 10; ++i) {
    const double z = re[i];
    if (!(fabs(im[i]) <= 1e-10) || !p3p_finite(z)) continue;
    int k = nr++;
    for (; k > 0 && zs[k - 1] > z; --k) zs[k] = zs[k - 1];
    zs[k] = z;
  }
  double* M = ws + kE5Models;
  const double* N = ws + kE5Basis;
  int nm = 0;
  for (int i = 0; i < nr; ++i) {
    const double z = zs[i];
    double X[3];
    e5_null3(ws, z, X);
    if (fabs(X[2]) < 1e-10) continue;
    const double x = X[0] / X[2], y = X[1] / X[2];
    double* E = M + 9 * nm;
    double nn = 0.0;
    for (int e = 0; e < 9; ++e) {
      E[e] = N[e] * x + N[9 + e] * y + N[18 + e] * z + N[27 + e];
      nn += E[e] * E[e];
    }
    nn = sqrt(nn);
    bool ok = true;
    for (int e = 0; e < 9; ++e) {
      E[e] /= nn;
      ok = ok && p3p_finite(E[e]);
    }
    if (!ok) continue;
    zs[nm++] = z;
  }
  for (int k = 9 * nm; k < 90; ++k) M[k] = NAN;
  for (int k = nm; k < 10; ++k) zs[k] = NAN;
  return nm;
}

// ---------------------------------------------------------------------------
// Score
// ---------------------------------------------------------------------------
// The signed Sampson quotient of essential_matrix.cc:149-157 for E row-major.
MAVBA_HD double e5_residual(const double* E, double x1, double y1, double x2, double y2) {
  MAVBA_TRI_AS_WRITTEN
  const double a0 = E[0] * x1 + E[1] * y1 + E[2];
  const double a1 = E[3] * x1 + E[4] * y1 + E[5];
  const double a2 = E[6] * x1 + E[7] * y1 + E[8];
  const double b0 = E[0] * x2 + E[3] * y2 + E[6];
  const double b1 = E[1] * x2 + E[4] * y2 + E[7];
  const double num = x2 * a0 + y2 * a1 + a2;
  return num / sqrt(a0 * a0 + a1 * a1 + b0 * b0 + b1 * b1);
}

// Selection and trial limit: ransac_core.h's over the (trial, model) sequence - every model that gets here is valid - and samples of five.
using E5Select = RansacSelect;
MAVBA_HD bool e5_select_step(E5Select& s, int t, int m, int count, double sum, int limit, long long stop) { return ransac_select_step(s, t, m, true, count, sum, limit, stop); }
inline int e5_dynamic_limit(long long k, long long n, double probability) { return ransac_dynamic_limit(k, n, 5, probability); }

// ---------------------------------------------------------------------------
// Pose recovery
// ---------------------------------------------------------------------------
// decompose_essential_matrix + the four candidates of pose_from_essential_matrix. E V = U S by the one-sided Jacobi
// iteration on E's columns; the column of the smallest norm is the null direction; (u1, u2, u1 x u2) and
// (v1, v2, v1 x v2) are completed to right-handed frames, which is the reference's "times -1 when det < 0" up to a
// half-turn about the third axis that exchanges R1 and R2 and flips t: the set of four candidates is the reference's,
// their order is this library's. With W = [0 1 0; -1 0 0; 0 0 1]:
//   R1 = U W V^T = -u2 v1^T + u1 v2^T + u3 v3^T,  R2 = U W^T V^T = u2 v1^T - u1 v2^T + u3 v3^T,  t = u3.
// P [4][12]: the candidates (R1, t), (R2, t), (R1, -t), (R2, -t) as row-major [R | t]; m [4]: the norm of P's third
// column (calc_depth's factor).
MAVBA_HD void e5_pose_candidates(const double* E, double* P, double* m) {
  MAVBA_TRI_AS_WRITTEN
  double A[3][3], V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int r = 0; r < 3; ++r) A[c][r] = E[3 * r + c];
  for (int sweep = 0; sweep < kP3PMaxSweeps; ++sweep) {
    bool any = p3p_jacobi_pair(A[0], A[1], V[0], V[1]);
    any = p3p_jacobi_pair(A[0], A[2], V[0], V[2]) || any;
    any = p3p_jacobi_pair(A[1], A[2], V[1], V[2]) || any;
    if (!any) break;
  }
  double n[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) n[c] = A[c][0] * A[c][0] + A[c][1] * A[c][1] + A[c][2] * A[c][2];
  const bool drop0 = n[0] < n[1] && n[0] < n[2], drop1 = !drop0 && n[1] < n[2];
  double u1[3], u2[3], u3[3], v1[3], v2[3], v3[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    u1[r] = drop0 ? A[2][r] : A[0][r]; v1[r] = drop0 ? V[2][r] : V[0][r];
    u2[r] = drop1 ? A[2][r] : A[1][r]; v2[r] = drop1 ? V[2][r] : V[1][r];
  }
  p3p_unit(u2);
  p3p_frame(u1, u2, u3);
  p3p_frame(v1, v2, v3);
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double s = u1[r] * v2[c] - u2[r] * v1[c], w = u3[r] * v3[c];
      P[4 * r + c] = P[24 + 4 * r + c] = s + w;
      P[12 + 4 * r + c] = P[36 + 4 * r + c] = w - s;
    }
    P[4 * r + 3] = P[12 + 4 * r + 3] = u3[r];
    P[24 + 4 * r + 3] = P[36 + 4 * r + 3] = -u3[r];
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) m[k] = sqrt(P[12 * k + 2] * P[12 * k + 2] + P[12 * k + 6] * P[12 * k + 6] + P[12 * k + 10] * P[12 * k + 10]);
}

// One candidate's cheirality test of one correspondence: the DLT against [I | 0] (tri_math.h), 0 < depth < 100 in both
// views (essential_matrix.cc:244-256).
MAVBA_HD bool e5_cheirality(const double* P2, double m2, double x1, double y1, double x2, double y2) {
  const double P1[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  double h[4], X[3];
  triangulate_dlt(P1, P2, x1, y1, x2, y2, h, X);
  const double d0 = tri_depth(P1, 1.0, X);
  if (!(d0 > 0.0 && d0 < 100.0)) return false;
  const double dj = tri_depth(P2, m2, X);
  return dj > 0.0 && dj < 100.0;
}

// The first candidate with a strictly larger count than every one before it (-1: every count is zero, where the
// reference leaves R and t unset).
MAVBA_HD int e5_cheirality_best(const int* counts) {
  int best = -1, bc = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (counts[k] > bc) { bc = counts[k]; best = k; }
  return best;
}

// inv_second_proj_matrix(2, 3) = -(R^T t)_z of P = [R | t] (sequential_mapper.cc:291-299)
MAVBA_HD double e5_forward_z(const double* P) {
  MAVBA_TRI_AS_WRITTEN
  return -(P[2] * P[3] + P[6] * P[7] + P[10] * P[11]);
}

}  // namespace mavba
#endif  // MAVBA_E5_MATH_H_
