// h4_math.h — the view-change test of an image pair: the sample rows, the four-point homography and the score of a model.
//
// These inline functions are the bodies of the kernel in homography.hip. Like p3p_math.h they are
// __host__ __device__, so tests/ can compile this header with g++ and check it without a GPU.
// There is no CPU path in the library: h4_run_item below is the one-thread run of the g++ harnesses.
//
// What is evaluated (reference file:line):
//   samples       src/util/estimation.cc:71-93: four distinct indices, used in ascending order (std::set); the
//                 generator, the dynamic trial limit and the selection among the trials are ransac_core.h's
//   hypothesis    ProjectiveTransformEstimator::estimate, src/base3d/projective_transform.cc:12-45: the null vector of
//                 the 8 x 9 system, here by scaled elimination with complete pivoting where the reference has an SVD
//   score         ProjectiveTransformEstimator::residuals, src/base3d/projective_transform.cc:48-74, and
//                 src/util/estimation.cc:104-117
//
// Everything is evaluated operation for operation as written, without fused multiply-adds (MAVBA_TRI_AS_WRITTEN): it
// needs only + - * / and sqrt, which round the same on the host and on the device, so the device build's models are
// the host build's. Nothing is indexed at run time: every loop has constant bounds and is unrolled, and a pivot
// exchange is a chain of selects, so the system stays in registers on the device.
#ifndef MAVBA_H4_MATH_H_
#define MAVBA_H4_MATH_H_

#include <float.h>
#include <stdint.h>

#include <vector>

#include "ransac_core.h"
#include "tri_math.h"

namespace mavba {

constexpr int kHomographyOk = 0, kHomographyNoConsensus = 1;  // MAVBA_HOMOGRAPHY_* (homography.hip asserts that they are equal)

// ---------------------------------------------------------------------------
// Samples (the generator is ransac_core.h's; the row is used in ascending order)
// ---------------------------------------------------------------------------
MAVBA_HD void h4_sort4(int* a) {
  cswap(a[0], a[1]); cswap(a[2], a[3]); cswap(a[0], a[2]); cswap(a[1], a[3]); cswap(a[1], a[2]);
}

// The row of trial `trial` for n >= 4 matches (the call needs n >= 5), ascending.
MAVBA_HD void h4_draw_sample(unsigned long long seed, unsigned trial, unsigned n, int* a) {
  ransac_draw_row<4>(seed, trial, n, a);
  h4_sort4(a);
}

MAVBA_HD bool h4_finite(double v) { return v - v == 0.0; }
MAVBA_HD double h4_abs(double v) { return v < 0.0 ? -v : v; }

// ---------------------------------------------------------------------------
// Hypothesis
// ---------------------------------------------------------------------------
// The homography of four matches m[k] = (x, y, u, v), k in sample order: H row-major with H[8] = 1, (x, y, 1) -> a
// multiple of (u, v, 1). Returns false for an invalid trial (H = NaN).
//   1. A [8][9]: rows 0-3 ( x y 1 0 0 0 -xu -yu u ), rows 4-7 ( 0 0 0 x y 1 -xv -yv v )   (projective_transform.cc:18-31)
//   2. every column divided by its largest magnitude (a column of zeros is left alone)
//   3. eight steps of elimination; the pivot of step k is the entry of the largest magnitude in rows k.. and columns
//      k.., of equal ones the first row, then the first column; its row and column are exchanged into place
//   4. the unknown of the last column is 1, the others follow from the bottom row up
//   5. the exchanges and the scaling are undone, h is divided by -h[8], then h[8] = 1           (projective_transform.cc:35-38)
// A system of rank below 8 ends with a zero pivot (an invalid trial) or, when rounding leaves a tiny one, with some
// member of its null space.
MAVBA_HD bool h4_estimate(const double (*m)[4], double* H) {
  MAVBA_TRI_AS_WRITTEN
  double A[8][9];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double x = m[k][0], y = m[k][1], u = m[k][2], v = m[k][3];
    A[k][0] = x; A[k][1] = y; A[k][2] = 1.0; A[k][3] = 0.0; A[k][4] = 0.0; A[k][5] = 0.0;
    A[k][6] = -(x * u); A[k][7] = -(y * u); A[k][8] = u;
    A[4 + k][0] = 0.0; A[4 + k][1] = 0.0; A[4 + k][2] = 0.0; A[4 + k][3] = x; A[4 + k][4] = y; A[4 + k][5] = 1.0;
    A[4 + k][6] = -(x * v); A[4 + k][7] = -(y * v); A[4 + k][8] = v;
  }
  double sc[9];  // the scale of the column that stands at each place
  int col[9];    // the unknown that stands at each place
#pragma unroll
  for (int j = 0; j < 9; ++j) {
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < 8; ++i) { const double a = h4_abs(A[i][j]); s = a > s ? a : s; }
    s = s > 0.0 ? s : 1.0;
#pragma unroll
    for (int i = 0; i < 8; ++i) A[i][j] = A[i][j] / s;
    sc[j] = s;
    col[j] = j;
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    double best = -1.0;
    int pi = k, pj = k;
#pragma unroll
    for (int i = k; i < 8; ++i) {
#pragma unroll
      for (int j = k; j < 9; ++j) {
        const double a = h4_abs(A[i][j]);
        const bool g = a > best;
        best = g ? a : best; pi = g ? i : pi; pj = g ? j : pj;
      }
    }
    // row pi <-> row k, in the columns still alive
#pragma unroll
    for (int j = k; j < 9; ++j) {
      const double top = A[k][j];
      double pr = top;
#pragma unroll
      for (int i = k + 1; i < 8; ++i) {
        const double a = A[i][j];
        pr = pi == i ? a : pr;
        A[i][j] = pi == i ? top : a;
      }
      A[k][j] = pr;
    }
    // column pj <-> column k, in every row (the finished rows above are read again by step 4)
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const double left = A[i][k];
      double pc = left;
#pragma unroll
      for (int j = k + 1; j < 9; ++j) {
        const double a = A[i][j];
        pc = pj == j ? a : pc;
        A[i][j] = pj == j ? left : a;
      }
      A[i][k] = pc;
    }
    {
      const double s0 = sc[k];
      const int c0 = col[k];
      double ps = s0;
      int pcl = c0;
#pragma unroll
      for (int j = k + 1; j < 9; ++j) {
        const double s = sc[j];
        const int c = col[j];
        ps = pj == j ? s : ps; pcl = pj == j ? c : pcl;
        sc[j] = pj == j ? s0 : s; col[j] = pj == j ? c0 : c;
      }
      sc[k] = ps; col[k] = pcl;
    }
    const double piv = A[k][k];
#pragma unroll
    for (int i = k + 1; i < 8; ++i) {
      const double f = A[i][k] / piv;
#pragma unroll
      for (int j = k + 1; j < 9; ++j) A[i][j] = A[i][j] - f * A[k][j];
    }
  }
  double z[9];
  z[8] = 1.0;
#pragma unroll
  for (int k = 7; k >= 0; --k) {
    double s = 0.0;
#pragma unroll
    for (int j = 8; j > k; --j) s = s + A[k][j] * z[j];
    z[k] = -s / A[k][k];
  }
  double h[9];
#pragma unroll
  for (int j = 0; j < 9; ++j) z[j] = z[j] / sc[j];
#pragma unroll
  for (int c = 0; c < 9; ++c) {
    double v = 0.0;
#pragma unroll
    for (int j = 0; j < 9; ++j) v = col[j] == c ? z[j] : v;
    h[c] = v;
  }
  const double d = -h[8];
  bool ok = true;
#pragma unroll
  for (int c = 0; c < 8; ++c) { H[c] = h[c] / d; ok = ok && h4_finite(H[c]); }
  H[8] = 1.0;
  if (!ok) {
#pragma unroll
    for (int c = 0; c < 9; ++c) H[c] = NAN;
  }
  return ok;
}

// Residual of the match (x, y) -> (u, v) under H: projective_transform.cc:61-68 (the sign of the third component is
// not tested; a zero there gives an infinite or NaN residual, which is no inlier).
MAVBA_HD double h4_residual(const double* H, double x, double y, double u, double v) {
  MAVBA_TRI_AS_WRITTEN
  const double p0 = (H[0] * x + H[1] * y) + H[2];
  const double p1 = (H[3] * x + H[4] * y) + H[5];
  const double p2 = (H[6] * x + H[7] * y) + H[8];
  const double dx = p0 / p2 - u, dy = p1 / p2 - v;
  return sqrt(dx * dx + dy * dy);
}

// Selection and trial limit: ransac_core.h's with one model per trial, the trial's own `valid` flag and samples of four.
MAVBA_HD bool h4_select_step(RansacSelect& s, int t, bool valid, int count, double sum, int limit, long long stop) { return ransac_select_step(s, t, 0, valid, count, sum, limit, stop); }
inline int h4_dynamic_limit(long long k, long long n, double probability) { return ransac_dynamic_limit(k, n, 4, probability); }

// ---------------------------------------------------------------------------
// Host only: what the host answers without the device, and one item on one thread (the g++ harnesses)
// ---------------------------------------------------------------------------
// The scalars of an item without consensus. Item: mavba_homography_item (a template so that this header needs no C header).
template <typename Item>
inline void h4_no_consensus(Item& it, int trials_used) {
  for (int k = 0; k < 9; ++k) it.H[k] = NAN;
  it.num_inliers = 0; it.inlier_ratio = 0.0; it.best_trial = -1; it.trials_used = trials_used; it.status = kHomographyNoConsensus;
}

// An item that does not run (n <= 4 or max_trials <= 0): its arrays filled as invalid trials with samples -1.
template <typename Item>
inline void h4_answer_without_run(Item& it) {
  h4_no_consensus(it, 0);
  const long long mt = it.max_trials > 0 ? it.max_trials : 0;
  if (it.inlier_mask) for (long long i = 0; i < it.n; ++i) it.inlier_mask[i] = 0;
  for (long long t = 0; t < mt; ++t) {
    if (it.trial_models) for (int k = 0; k < 9; ++k) it.trial_models[9 * t + k] = NAN;
    if (it.trial_num_inliers) it.trial_num_inliers[t] = 0;
    if (it.trial_residual_sum) it.trial_residual_sum[t] = 0.0;
    if (it.trial_samples) for (int k = 0; k < 4; ++k) it.trial_samples[4 * t + k] = -1;
  }
}

// The kernel's sum over 64 lanes (dev_reduce.h wave_sum): a butterfly over each row of 16 lanes (8, 4, 2, 1), then the
// four rows as (r0 + r1) + (r2 + r3).
inline double h4_lanes_sum(double* v) {
  for (int step = 8; step >= 1; step >>= 1) {
    double w[64];
    for (int l = 0; l < 64; ++l) w[l] = v[l] + v[(l & ~15) | ((l - step) & 15)];
    for (int l = 0; l < 64; ++l) v[l] = w[l];
  }
  return (v[0] + v[16]) + (v[32] + v[48]);
}

// One item as the kernel runs it, on one thread: the same outputs, the same shape of every sum (kernel_seconds is left
// alone). The item's arguments are taken as valid (the library's entry point judges them).
template <typename Item>
inline void h4_run_item(Item& it) {
  const long long n = it.n;
  const int mt = it.max_trials;
  if (n <= 4 || mt <= 0) { h4_answer_without_run(it); return; }
  const double thr = it.max_reproj_error_px;
  std::vector<int> table((size_t)n + 1);
  for (long long k = 0; k <= n; ++k) table[(size_t)k] = h4_dynamic_limit(k, n, it.probability);
  std::vector<double> models(9 * (size_t)mt), sums((size_t)mt);
  std::vector<int> counts((size_t)mt);
  for (int t = 0; t < mt; ++t) {
    int a[4];
    if (it.samples) { for (int k = 0; k < 4; ++k) a[k] = it.samples[4 * t + k]; h4_sort4(a); }
    else h4_draw_sample(it.seed, (unsigned)t, (unsigned)n, a);
    double m[4][4];
    for (int k = 0; k < 4; ++k) {
      m[k][0] = it.uv1[2 * a[k]]; m[k][1] = it.uv1[2 * a[k] + 1]; m[k][2] = it.uv2[2 * a[k]]; m[k][3] = it.uv2[2 * a[k] + 1];
    }
    double* H = models.data() + 9 * (size_t)t;
    const bool valid = h4_estimate(m, H);
    double lanes[64];
    for (int l = 0; l < 64; ++l) lanes[l] = 0.0;
    int c = 0;
    if (valid)
      for (long long i = 0; i < n; ++i) {
        const double r = h4_residual(H, it.uv1[2 * i], it.uv1[2 * i + 1], it.uv2[2 * i], it.uv2[2 * i + 1]);
        if (r <= thr) { lanes[i & 63] += r; ++c; }
      }
    counts[(size_t)t] = c;
    sums[(size_t)t] = h4_lanes_sum(lanes);
    if (it.trial_samples) for (int k = 0; k < 4; ++k) it.trial_samples[4 * t + k] = a[k];
  }
  RansacSelect sel;
  for (int t = 0; t < mt; ++t)
    if (h4_select_step(sel, t, h4_finite(models[9 * (size_t)t]), counts[(size_t)t], sums[(size_t)t], table[(size_t)counts[(size_t)t]], it.stop_num_inliers)) break;
  if (it.trial_models) for (size_t k = 0; k < models.size(); ++k) it.trial_models[k] = models[k];
  if (it.trial_num_inliers) for (int t = 0; t < mt; ++t) it.trial_num_inliers[t] = counts[(size_t)t];
  if (it.trial_residual_sum) for (int t = 0; t < mt; ++t) it.trial_residual_sum[t] = sums[(size_t)t];
  const bool found = sel.best_trial >= 0 && sel.best_inliers >= 4;
  if (!found) {
    h4_no_consensus(it, sel.trials_used);
    if (it.inlier_mask) for (long long i = 0; i < n; ++i) it.inlier_mask[i] = 0;
    return;
  }
  const double* B = models.data() + 9 * (size_t)sel.best_trial;
  for (int k = 0; k < 9; ++k) it.H[k] = B[k];
  it.num_inliers = (int)sel.best_inliers; it.inlier_ratio = (double)it.num_inliers / (double)n;
  it.best_trial = sel.best_trial; it.trials_used = sel.trials_used; it.status = kHomographyOk;
  if (it.inlier_mask)
    for (long long i = 0; i < n; ++i)
      it.inlier_mask[i] = h4_residual(B, it.uv1[2 * i], it.uv1[2 * i + 1], it.uv2[2 * i], it.uv2[2 * i + 1]) <= thr ? 1 : 0;
}

}  // namespace mavba
#endif  // MAVBA_H4_MATH_H_
