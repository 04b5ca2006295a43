// Host build (g++) of mavmap_amd/csrc/e5_math.h — TEST HARNESS ONLY.
// Lets the CPU test-suite check the bodies of the relative-pose kernel without a GPU, and gives the one-thread host
// time the design notes compare the kernel with.
#include <vector>

#include "../../include/mavba_relative_pose.h"
#include "../../mavmap_amd/csrc/e5_math.h"

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
int model_k(int model) { return model == 1 ? 4 : (model == 2 ? 8 : 9); }
}  // namespace

extern "C" {
void he_draw_samples(unsigned long long seed, long long n, int trials, int* out) {
  for (int t = 0; t < trials; ++t)
    mavba::e5_draw_sample(seed, (unsigned)t, (unsigned)n, out[5 * t], out[5 * t + 1], out[5 * t + 2], out[5 * t + 3], out[5 * t + 4]);
}
void he_image2world(int model, const double* cam, long long n, const double* uv, double* xy) {
  for (long long i = 0; i < n; ++i) mavba::image2world(model, cam, uv[2 * i], uv[2 * i + 1], xy[2 * i], xy[2 * i + 1]);
}
// m hypotheses: x1, x2 [m][5][2] lifted observations (rows ascending); models [m][10][9], zs [m][10], counts [m],
// sweeps [m] (of the root finder; 100 = the limit)
void he_estimate(long long m, const double* x1, const double* x2, double* models, double* zs, int* counts, int* sweeps) {
  std::vector<double> ws(mavba::kE5Work);
  for (long long i = 0; i < m; ++i) {
    counts[i] = mavba::e5_estimate(x1 + 10 * i, x2 + 10 * i, ws.data());
    for (int k = 0; k < 90; ++k) models[90 * i + k] = ws[mavba::kE5Models + k];
    for (int k = 0; k < 10; ++k) zs[10 * i + k] = ws[mavba::kE5Z + k];
    if (sweeps) {  // (the root finder again on the polynomial the estimate left)
      sweeps[i] = mavba::e5_roots(ws.data());
    }
  }
}
int he_dynamic_limit(long long k, long long n, double probability) { return mavba::e5_dynamic_limit(k, n, probability); }
void he_pose_candidates(const double* E, double* P, double* m) { mavba::e5_pose_candidates(E, P, m); }

// One item as the kernel runs it, on one thread: the same outputs, the same shape of every sum (kernel_seconds is left alone).
void he_relative_pose(mavba_relpose_item* it) {
  using namespace mavba;
  const long long n = it->n;
  const int mt = it->max_trials;
  const double nan = NAN;
  for (int k = 0; k < 9; ++k) it->E[k] = it->R[k] = nan;
  for (int k = 0; k < 3; ++k) it->rvec[k] = it->tvec[k] = nan;
  for (int k = 0; k < 4; ++k) it->cheirality_counts[k] = 0;
  it->cheirality_best = -1; it->forward_z = nan;
  it->num_inliers = 0; it->best_trial = -1; it->best_model = -1; it->trials_used = 0; it->status = kRelposeNoConsensus;
  if (it->inlier_mask) for (long long i = 0; i < n; ++i) it->inlier_mask[i] = 0;
  if (n <= 5 || mt <= 0) {
    for (int t = 0; t < mt; ++t) {
      if (it->trial_num_models) it->trial_num_models[t] = 0;
      if (it->trial_models) for (int k = 0; k < 90; ++k) it->trial_models[90 * t + k] = nan;
      if (it->trial_z) for (int k = 0; k < 10; ++k) it->trial_z[10 * t + k] = nan;
      if (it->trial_num_inliers) for (int k = 0; k < 10; ++k) it->trial_num_inliers[10 * t + k] = 0;
      if (it->trial_residual_sum) for (int k = 0; k < 10; ++k) it->trial_residual_sum[10 * t + k] = 0.0;
      if (it->trial_samples) for (int k = 0; k < 5; ++k) it->trial_samples[5 * t + k] = -1;
    }
    return;
  }
  double cam1[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, cam2[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int k = 0; k < model_k(it->camera_model1); ++k) cam1[k] = it->intrinsics1[k];
  for (int k = 0; k < model_k(it->camera_model2); ++k) cam2[k] = it->intrinsics2[k];
  const double thr = (image2world_threshold(it->max_reproj_error_px, cam1) + image2world_threshold(it->max_reproj_error_px, cam2)) / 2;
  std::vector<double> p1(2 * n), p2(2 * n);
  for (long long i = 0; i < n; ++i) {
    image2world(it->camera_model1, cam1, it->uv1[2 * i], it->uv1[2 * i + 1], p1[2 * i], p1[2 * i + 1]);
    image2world(it->camera_model2, cam2, it->uv2[2 * i], it->uv2[2 * i + 1], p2[2 * i], p2[2 * i + 1]);
  }
  std::vector<int> table(n + 1);
  for (long long k = 0; k <= n; ++k) table[k] = e5_dynamic_limit(k, n, it->probability);
  std::vector<double> models(90 * (size_t)mt), zs(10 * (size_t)mt), sums(10 * (size_t)mt, 0.0), ws(kE5Work);
  std::vector<int> counts(10 * (size_t)mt, 0), nms(mt);
  for (int t = 0; t < mt; ++t) {
    int a[5];
    if (it->samples) { for (int k = 0; k < 5; ++k) a[k] = it->samples[5 * t + k]; e5_sort5(a[0], a[1], a[2], a[3], a[4]); }
    else e5_draw_sample(it->seed, (unsigned)t, (unsigned)n, a[0], a[1], a[2], a[3], a[4]);
    double x1[10], x2[10];
    for (int k = 0; k < 5; ++k) {
      x1[2 * k] = p1[2 * a[k]]; x1[2 * k + 1] = p1[2 * a[k] + 1];
      x2[2 * k] = p2[2 * a[k]]; x2[2 * k + 1] = p2[2 * a[k] + 1];
    }
    const int nm = nms[t] = e5_estimate(x1, x2, ws.data());
    for (int k = 0; k < 90; ++k) models[90 * (size_t)t + k] = ws[kE5Models + k];
    for (int k = 0; k < 10; ++k) zs[10 * (size_t)t + k] = ws[kE5Z + k];
    for (int m = 0; m < nm; ++m) {
      const double* E = models.data() + 90 * (size_t)t + 9 * m;
      double lanes[64];
      for (int l = 0; l < 64; ++l) lanes[l] = 0.0;
      int c = 0;
      for (long long i = 0; i < n; ++i) {
        const double r = fabs(e5_residual(E, p1[2 * i], p1[2 * i + 1], p2[2 * i], p2[2 * i + 1]));
        if (r <= thr) { lanes[i & 63] += r; ++c; }
      }
      counts[10 * (size_t)t + m] = c;
      sums[10 * (size_t)t + m] = lanes_sum(lanes);
    }
    if (it->trial_samples) for (int k = 0; k < 5; ++k) it->trial_samples[5 * t + k] = a[k];
  }
  E5Select sel;
  bool ended = false;
  for (int t = 0; t < mt && !ended; ++t)
    for (int m = 0; m < nms[t] && !ended; ++m) {
      const int c = counts[10 * (size_t)t + m];
      ended = e5_select_step(sel, t, m, c, sums[10 * (size_t)t + m], table[c], it->stop_num_inliers);
    }
  if (!ended) sel.trials_used = mt;
  if (it->trial_num_models) for (int t = 0; t < mt; ++t) it->trial_num_models[t] = nms[t];
  if (it->trial_models) for (size_t k = 0; k < models.size(); ++k) it->trial_models[k] = models[k];
  if (it->trial_z) for (size_t k = 0; k < zs.size(); ++k) it->trial_z[k] = zs[k];
  if (it->trial_num_inliers) for (size_t k = 0; k < counts.size(); ++k) it->trial_num_inliers[k] = counts[k];
  if (it->trial_residual_sum) for (size_t k = 0; k < sums.size(); ++k) it->trial_residual_sum[k] = sums[k];
  it->trials_used = sel.trials_used;
  if (sel.best_trial < 0 || sel.best_inliers < 5) return;
  const double* B = models.data() + 90 * (size_t)sel.best_trial + 9 * sel.best_model;
  for (int k = 0; k < 9; ++k) it->E[k] = B[k];
  it->num_inliers = (int)sel.best_inliers; it->best_trial = sel.best_trial; it->best_model = sel.best_model; it->status = kRelposeOk;
  double P[48], m4[4];
  e5_pose_candidates(B, P, m4);
  int cc[4] = {0, 0, 0, 0};
  for (long long i = 0; i < n; ++i) {
    const bool inl = fabs(e5_residual(B, p1[2 * i], p1[2 * i + 1], p2[2 * i], p2[2 * i + 1])) <= thr;
    if (it->inlier_mask) it->inlier_mask[i] = inl ? 1 : 0;
    if (!inl) continue;
    for (int k = 0; k < 4; ++k) cc[k] += e5_cheirality(P + 12 * k, m4[k], p1[2 * i], p1[2 * i + 1], p2[2 * i], p2[2 * i + 1]) ? 1 : 0;
  }
  for (int k = 0; k < 4; ++k) it->cheirality_counts[k] = cc[k];
  const int best = e5_cheirality_best(cc);
  it->cheirality_best = best;
  if (best < 0) return;
  const double* Pb = P + 12 * best;
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) it->R[3 * r + c] = Pb[4 * r + c];
    it->tvec[r] = Pb[4 * r + 3];
  }
  p3p_rvec_from_model(Pb, it->rvec);
  it->forward_z = e5_forward_z(Pb);
}
}
