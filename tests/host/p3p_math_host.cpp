// Host build (g++) of mavmap_amd/csrc/p3p_math.h — TEST HARNESS ONLY.
// Lets the CPU test-suite check the bodies of the absolute-pose kernel without a GPU, and gives the one-thread host
// time the design notes compare the kernel with.
#include <vector>

#include "../../include/mavba_absolute_pose.h"
#include "../../mavmap_amd/csrc/p3p_math.h"

namespace {
// The kernel's sum over 64 lanes (dev_reduce.h wave_sum): a butterfly over each row of 16 lanes (8, 4, 2, 1), then the
// four rows as (r0 + r1) + (r2 + r3).
double lanes_sum(double* v) {
  for (int step = 8; step >= 1; step >>= 1) {
    double w[64];
    for (int l = 0; l < 64; ++l) w[l] = v[l] + v[(l & ~15) | ((l - step) & 15)];
    for (int l = 0; l < 64; ++l) v[l] = w[l];
  }
  return (v[0] + v[16]) + (v[32] + v[48]);
}
}  // namespace

extern "C" {
void hp_draw_samples(unsigned long long seed, long long n, int trials, int* out) {
  for (int t = 0; t < trials; ++t) mavba::p3p_draw_sample(seed, (unsigned)t, (unsigned)n, out[4 * t], out[4 * t + 1], out[4 * t + 2], out[4 * t + 3]);
}
void hp_image2world(int model, const double* cam, long long n, const double* uv, double* xy) {
  for (long long i = 0; i < n; ++i) mavba::image2world(model, cam, uv[2 * i], uv[2 * i + 1], xy[2 * i], xy[2 * i + 1]);
}
// m hypotheses: x2d [m][4][2] lifted observations, X [m][4][3] world points (rows ascending), M [m][12], valid [m]
void hp_estimate(long long m, const double* x2d, const double* X, double* M, unsigned char* valid) {
  for (long long i = 0; i < m; ++i) valid[i] = mavba::p3p_estimate(x2d + 8 * i, X + 12 * i, M + 12 * i) ? 1 : 0;
}
void hp_rvec(const double* M, double* rvec) { mavba::p3p_rvec_from_model(M, rvec); }
int hp_dynamic_limit(long long k, long long n, double probability) { return mavba::p3p_dynamic_limit(k, n, probability); }

// One item as the kernel runs it, on one thread: the same outputs, the same shape of every sum (kernel_seconds is left alone).
void hp_absolute_pose(mavba_abspose_item* it) {
  using namespace mavba;
  const long long n = it->n;
  const int mt = it->max_trials;
  const double nan = NAN;
  for (int k = 0; k < 3; ++k) it->rvec[k] = it->tvec[k] = nan;
  for (int k = 0; k < 12; ++k) it->proj_matrix[k] = nan;
  it->num_inliers = 0; it->best_trial = -1; it->trials_used = 0; it->status = kAbsposeNoConsensus;
  if (it->inlier_mask) for (long long i = 0; i < n; ++i) it->inlier_mask[i] = 0;
  if (n <= 4 || mt <= 0) {
    for (int t = 0; t < mt; ++t) {
      if (it->trial_models) for (int k = 0; k < 12; ++k) it->trial_models[12 * t + k] = nan;
      if (it->trial_num_inliers) it->trial_num_inliers[t] = 0;
      if (it->trial_residual_sum) it->trial_residual_sum[t] = 0.0;
      if (it->trial_samples) for (int k = 0; k < 4; ++k) it->trial_samples[4 * t + k] = -1;
    }
    return;
  }
  double cam[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  const int K = it->camera_model == 1 ? 4 : (it->camera_model == 2 ? 8 : 9);
  for (int k = 0; k < K; ++k) cam[k] = it->intrinsics[k];
  const double thr = image2world_threshold(it->max_reproj_error_px, cam);
  std::vector<double> xy(2 * n);
  for (long long i = 0; i < n; ++i) image2world(it->camera_model, cam, it->uv[2 * i], it->uv[2 * i + 1], xy[2 * i], xy[2 * i + 1]);
  std::vector<int> table(n + 1);
  for (long long k = 0; k <= n; ++k) table[k] = p3p_dynamic_limit(k, n, it->probability);
  std::vector<double> models(12 * (size_t)mt), sums(mt);
  std::vector<int> counts(mt);
  for (int t = 0; t < mt; ++t) {
    int a[4];
    if (it->samples) { for (int k = 0; k < 4; ++k) a[k] = it->samples[4 * t + k]; p3p_sort4(a[0], a[1], a[2], a[3]); }
    else p3p_draw_sample(it->seed, (unsigned)t, (unsigned)n, a[0], a[1], a[2], a[3]);
    double x2d[8], X[12];
    for (int k = 0; k < 4; ++k) {
      x2d[2 * k] = xy[2 * a[k]]; x2d[2 * k + 1] = xy[2 * a[k] + 1];
      for (int c = 0; c < 3; ++c) X[3 * k + c] = it->xyz[3 * a[k] + c];
    }
    double* M = models.data() + 12 * t;
    const bool valid = p3p_estimate(x2d, X, M);
    double lanes[64];
    for (int l = 0; l < 64; ++l) lanes[l] = 0.0;
    int c = 0;
    if (valid)
      for (long long i = 0; i < n; ++i) {
        const double r = p3p_residual(M, it->xyz[3 * i], it->xyz[3 * i + 1], it->xyz[3 * i + 2], xy[2 * i], xy[2 * i + 1]);
        if (r <= thr) { lanes[i & 63] += r; ++c; }
      }
    counts[t] = c;
    sums[t] = lanes_sum(lanes);
    if (it->trial_samples) for (int k = 0; k < 4; ++k) it->trial_samples[4 * t + k] = a[k];
  }
  P3PSelect sel;
  for (int t = 0; t < mt; ++t)
    if (p3p_select_step(sel, t, p3p_finite(models[12 * t]), counts[t], sums[t], table[counts[t]], it->stop_num_inliers)) break;
  if (it->trial_models) for (size_t k = 0; k < models.size(); ++k) it->trial_models[k] = models[k];
  if (it->trial_num_inliers) for (int t = 0; t < mt; ++t) it->trial_num_inliers[t] = counts[t];
  if (it->trial_residual_sum) for (int t = 0; t < mt; ++t) it->trial_residual_sum[t] = sums[t];
  it->trials_used = sel.trials_used;
  if (sel.best_trial < 0 || sel.best_inliers < 4) return;
  const double* B = models.data() + 12 * sel.best_trial;
  for (int k = 0; k < 12; ++k) it->proj_matrix[k] = B[k];
  it->tvec[0] = B[3]; it->tvec[1] = B[7]; it->tvec[2] = B[11];
  p3p_rvec_from_model(B, it->rvec);
  it->num_inliers = (int)sel.best_inliers; it->best_trial = sel.best_trial; it->status = kAbsposeOk;
  if (it->inlier_mask)
    for (long long i = 0; i < n; ++i)
      it->inlier_mask[i] = p3p_residual(B, it->xyz[3 * i], it->xyz[3 * i + 1], it->xyz[3 * i + 2], xy[2 * i], xy[2 * i + 1]) <= thr ? 1 : 0;
}
}
