// relative_pose.hip - batched relative pose from 2D-2D matches: the five-point solver inside RANSAC and the recovery
// of (R, t), ONE launch for any number of image pairs.
//
// Replaces, per candidate initial pair, the host step of reference src/sfm/sequential_mapper.cc:174-216 and :269-299
// (with src/base3d/essential_matrix.cc and src/util/estimation.cc): 1000 independent samples, up to ten models each,
// every model scored against every match. The maths is e5_math.h; this file is the launch shape and the host packing.
// The observations are lifted (image2world) and the dynamic trial limit is tabulated once per item while packing.
//
// Grid: the sum over items of ceil(max_trials_i / 16) work-groups; block_map[g] = (item, group of 16 trials). A wave
// owns four trials from sample to score and never talks to another wave:
//   hypothesis    lanes 0-3: one trial each, on a workspace of kE5Work doubles in LDS. Every array of the solver that
//                 is indexed at run time (the 10 x 20 system, the polynomials, the roots) lives there, so nothing
//                 spills to scratch; the 3 x 3 Jacobi iterations stay in registers
//   score         each of the wave's up to 40 models is broadcast from the workspace into scalar registers
//                 (v_readlane); the 64 lanes stride the item's points. Lane l adds the |residuals| of its inliers
//                 l, l + 64, ... in order, the wave reduction of dev_reduce.h adds the lanes: a fixed shape, so a
//                 model's sum does not depend on the batch
// The item's LAST work-group to finish (an integer ticket, as in absolute_pose.hip) replays the selection over the
// (trial, model) sequence, writes the best model's inlier mask, counts the four pose candidates' points in front of
// both cameras and converts the chosen R to rvec. No floating-point atomics, no spinning: a work-group never waits
// for another one.
#include "batch_call.h"
#include "dev_reduce.h"
#include "e5_math.h"

namespace mavba {

static_assert(kRelposeOk == MAVBA_RELPOSE_OK && kRelposeNoConsensus == MAVBA_RELPOSE_NO_CONSENSUS, "status codes of e5_math.h and mavba_relative_pose.h");

constexpr int kRelTrialsPerWave = 4;
constexpr int kRelTrialsPerGroup = 4 * kRelTrialsPerWave;  // tests/test_gpu_relative_pose.py runs 15, 16 and 17 trials
constexpr int kRelReplayChunk = 256;                        // trials per pass of the selection replay
static_assert(kRelReplayChunk * (kE5MaxModels * 3 + 1) / 2 + 8 <= kRelTrialsPerGroup * kE5Work, "the replay's tables fit in the workspaces");

struct RelResultDev {
  double E[9], R[9], tvec[3], rvec[3], forward_z;
  int cheir[4], cheir_best, num_inliers, best_trial, best_model, trials_used, status;
};

// Packed inputs: pts [N] = (x1, y1, x2, y2) lifted, samples_in: the supplied rows [.][5] (sorted), table: the dynamic
// limits. Per trial: nmod [T], samp [T][5]; per (trial, model): models [T][10][9], zs [T][10], cnt [T][10], sum [T][10].
// mask [N]. done: one ticket counter per item, zero on entry.
__global__ void __launch_bounds__(256) k_relative_pose(const RansacItemDev* __restrict__ items, const int2* __restrict__ block_map,
                                                       const double4* __restrict__ pts, const int* __restrict__ samples_in,
                                                       const int* __restrict__ table, int* nmod, double* models, double* zs, int* cnt,
                                                       double* sum, int* samp, unsigned char* mask, unsigned* done, RelResultDev* results) {
  __shared__ double s_ws[kRelTrialsPerGroup * kE5Work];
  __shared__ int s_nm[kRelTrialsPerGroup];
  __shared__ double s_P[48], s_m[4];
  __shared__ int s_last, s_end, s_best, s_bestm, s_used, s_inl, s_ch[4];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int2 bm = block_map[blockIdx.x];
  const RansacItemDev& it = items[bm.x];
  const int n = it.n, max_trials = it.max_trials;
  const size_t pb = (size_t)it.pt_begin, tb = (size_t)it.trial_begin;
  const double thr = it.thr;
  const int t0 = bm.y * kRelTrialsPerGroup + wv * kRelTrialsPerWave;  // the wave's first trial

  // ---- hypothesis: lane = trial of the wave ----
  if (lane < kRelTrialsPerWave && t0 + lane < max_trials) {
    const int t = t0 + lane;
    double* ws = s_ws + (wv * kRelTrialsPerWave + lane) * kE5Work;
    int a0, a1, a2, a3, a4;
    if (it.samples_begin >= 0) {
      const int* row = samples_in + 5 * ((size_t)it.samples_begin + t);
      a0 = row[0]; a1 = row[1]; a2 = row[2]; a3 = row[3]; a4 = row[4];
    } else {
      e5_draw_sample(it.seed, (unsigned)t, (unsigned)n, a0, a1, a2, a3, a4);
    }
    int* so = samp + 5 * (tb + t);
    so[0] = a0; so[1] = a1; so[2] = a2; so[3] = a3; so[4] = a4;
    double x1[10], x2[10];
    const int idx[5] = {a0, a1, a2, a3, a4};
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      const double4 p = pts[pb + idx[k]];
      x1[2 * k] = p.x; x1[2 * k + 1] = p.y; x2[2 * k] = p.z; x2[2 * k + 1] = p.w;
    }
    const int nm = e5_estimate(x1, x2, ws);
    s_nm[wv * kRelTrialsPerWave + lane] = nm;
    nmod[tb + t] = nm;
    double* mo = models + 90 * (tb + t);
    for (int k = 0; k < 90; ++k) mo[k] = ws[kE5Models + k];
    double* zo = zs + 10 * (tb + t);
    for (int k = 0; k < 10; ++k) zo[k] = ws[kE5Z + k];
  }
  __syncthreads();

  // ---- score: the wave's models one after the other, the lanes stride the points ----
  for (int j = 0; j < kRelTrialsPerWave; ++j) {
    const int t = t0 + j;
    if (t >= max_trials) break;
    const double* ws = s_ws + (wv * kRelTrialsPerWave + j) * kE5Work;
    const int nm = __builtin_amdgcn_readfirstlane(s_nm[wv * kRelTrialsPerWave + j]);
    for (int m = 0; m < kE5MaxModels; ++m) {
      double s = 0.0;
      int c = 0;
      if (m < nm) {
        double E[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) E[k] = wave_bcast(ws[kE5Models + 9 * m + k], 0);
        for (int i = lane; i < n; i += 64) {
          const double4 p = pts[pb + i];
          const double r = fabs(e5_residual(E, p.x, p.y, p.z, p.w));
          const bool inl = r <= thr;
          if (inl) s += r;
          c += __popcll(__ballot(inl));
        }
        c = __builtin_amdgcn_readfirstlane(c);  // (lane 0 runs every iteration of the loop above: n >= 6)
        s = wave_sum(s);
      }
      if (lane == 0) { cnt[10 * (tb + t) + m] = c; sum[10 * (tb + t) + m] = s; }
    }
  }

  // ---- the item's last work-group to get here finishes the item ----
  if (!last_block_of_item(done, bm.x, it.num_blocks, &s_last)) return;

  // the replay's tables lie over the workspaces, which are no longer needed
  double* r_sum = s_ws;                                                            // [256][10]
  int* r_cnt = reinterpret_cast<int*>(s_ws + kRelReplayChunk * kE5MaxModels);      // [256][10]
  int* r_nm = r_cnt + kRelReplayChunk * kE5MaxModels;                              // [256]
  E5Select sel;  // (thread 0's)
  if (tid == 0) s_end = 0;
  for (int base = 0; base < max_trials; base += kRelReplayChunk) {
    const int m = max_trials - base < kRelReplayChunk ? max_trials - base : kRelReplayChunk;
    for (int k = tid; k < m; k += 256) r_nm[k] = __hip_atomic_load(nmod + tb + base + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (int k = tid; k < m * kE5MaxModels; k += 256) {
      r_cnt[k] = __hip_atomic_load(cnt + 10 * (tb + base) + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      r_sum[k] = __hip_atomic_load(sum + 10 * (tb + base) + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    if (tid == 0) {
      int ended = 0;
      for (int k = 0; k < m && !ended; ++k)
        for (int q = 0; q < r_nm[k] && !ended; ++q) {
          const int c = r_cnt[10 * k + q];
          ended = e5_select_step(sel, base + k, q, c, r_sum[10 * k + q], table[(size_t)it.table_begin + c], it.stop) ? 1 : 0;
        }
      s_end = ended;
    }
    __syncthreads();
    if (s_end) break;
  }
  if (tid == 0) {
    s_best = sel.best_trial; s_bestm = sel.best_model; s_inl = (int)sel.best_inliers;
    s_used = s_end ? sel.trials_used : max_trials;
    s_ch[0] = s_ch[1] = s_ch[2] = s_ch[3] = 0;
  }
  __syncthreads();
  const int best = s_best, bestm = s_bestm;
  const bool found = best >= 0 && s_inl >= 5;
  double B[9];
#pragma unroll
  for (int k = 0; k < 9; ++k)
    B[k] = found ? __hip_atomic_load(models + 90 * (tb + best) + 9 * bestm + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : NAN;
  if (tid == 0 && found) e5_pose_candidates(B, s_P, s_m);
  __syncthreads();
  int c0 = 0, c1 = 0, c2 = 0, c3 = 0;
  for (int i = tid; i < n; i += 256) {
    bool inl = false;
    if (found) {
      const double4 p = pts[pb + i];
      inl = fabs(e5_residual(B, p.x, p.y, p.z, p.w)) <= thr;
      if (inl) {
        c0 += e5_cheirality(s_P, s_m[0], p.x, p.y, p.z, p.w) ? 1 : 0;
        c1 += e5_cheirality(s_P + 12, s_m[1], p.x, p.y, p.z, p.w) ? 1 : 0;
        c2 += e5_cheirality(s_P + 24, s_m[2], p.x, p.y, p.z, p.w) ? 1 : 0;
        c3 += e5_cheirality(s_P + 36, s_m[3], p.x, p.y, p.z, p.w) ? 1 : 0;
      }
    }
    mask[pb + i] = inl ? 1 : 0;
  }
  if (c0) atomicAdd(&s_ch[0], c0);
  if (c1) atomicAdd(&s_ch[1], c1);
  if (c2) atomicAdd(&s_ch[2], c2);
  if (c3) atomicAdd(&s_ch[3], c3);
  __syncthreads();
  if (tid == 0) {
    RelResultDev& r = results[bm.x];
    const int cc[4] = {s_ch[0], s_ch[1], s_ch[2], s_ch[3]};
    const int cb = found ? e5_cheirality_best(cc) : -1;
#pragma unroll
    for (int k = 0; k < 9; ++k) { r.E[k] = B[k]; r.R[k] = NAN; }
#pragma unroll
    for (int k = 0; k < 3; ++k) r.tvec[k] = r.rvec[k] = NAN;
    r.forward_z = NAN;
    if (cb >= 0) {
      const double* P = s_P + 12 * cb;
      double M[12];
#pragma unroll
      for (int k = 0; k < 12; ++k) M[k] = P[k];
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        r.R[3 * q] = M[4 * q]; r.R[3 * q + 1] = M[4 * q + 1]; r.R[3 * q + 2] = M[4 * q + 2];
        r.tvec[q] = M[4 * q + 3];
      }
      p3p_rvec_from_model(M, r.rvec);
      r.forward_z = e5_forward_z(M);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) r.cheir[k] = cc[k];
    r.cheir_best = cb;
    r.num_inliers = found ? s_inl : 0;
    r.best_trial = found ? best : -1;
    r.best_model = found ? bestm : -1;
    r.trials_used = s_used;
    r.status = found ? kRelposeOk : kRelposeNoConsensus;
  }
}

// Host side, on the frame of batch_call.h: validate, lift and pack, launch, download, scatter.
void relative_pose_ransac(int count, mavba_relpose_item* items, int device) {
  // ---- validate: every item is judged before the device is touched ----
  std::vector<RansacItemDev> hd((size_t)count);
  RansacBatch batch;
  bool want_mask = false, want_nm = false, want_models = false, want_z = false, want_cnt = false, want_sum = false, want_samp = false;
  for (int q = 0; q < count; ++q) {
    const mavba_relpose_item& it = items[q];
    check_item(it.n, it.max_trials >= 0 && !(it.n > 0 && (!it.intrinsics1 || !it.intrinsics2 || !it.uv1 || !it.uv2)), "relative-pose");
    check_model(it.camera_model1);
    check_model(it.camera_model2);
    if (!(it.n > 5 && it.max_trials > 0)) continue;  // (such an item owns no work-group and is answered by the host)
    batch.place<5>(hd[q], it.n, it.max_trials, it.stop_num_inliers, it.seed, it.samples, kRelTrialsPerGroup, 9 * kE5MaxModels);
    want_mask |= it.inlier_mask != nullptr; want_nm |= it.trial_num_models != nullptr; want_models |= it.trial_models != nullptr;
    want_z |= it.trial_z != nullptr; want_cnt |= it.trial_num_inliers != nullptr; want_sum |= it.trial_residual_sum != nullptr;
    want_samp |= it.trial_samples != nullptr;
  }
  require_device();
  DeviceScope on_device(device);
  double kernel_seconds = 0.0;
  std::vector<RelResultDev> h_res((size_t)count);
  std::vector<double> h_models, h_z, h_sum;
  std::vector<int> h_nm, h_cnt, h_samp;
  std::vector<unsigned char> h_mask;
  if (batch.blocks > 0) {
    // ---- lift and pack ----
    const size_t N = (size_t)batch.points, T = (size_t)batch.trials;
    const std::vector<int2> map = make_block_map(hd, batch.blocks);
    std::vector<double4> pts(N);
    std::vector<int> srows(5 * (size_t)batch.rows);
    std::vector<int> table((size_t)batch.table_len);
    for (int q = 0; q < count; ++q) {
      const mavba_relpose_item& it = items[q];
      RansacItemDev& d = hd[q];
      if (d.num_blocks == 0) continue;
      double cam1[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, cam2[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
      for (int k = 0; k < model_k(it.camera_model1); ++k) cam1[k] = it.intrinsics1[k];
      for (int k = 0; k < model_k(it.camera_model2); ++k) cam2[k] = it.intrinsics2[k];
      d.thr = (image2world_threshold(it.max_reproj_error_px, cam1) + image2world_threshold(it.max_reproj_error_px, cam2)) / 2;
      const size_t b = (size_t)d.pt_begin;
      for (size_t i = 0; i < (size_t)it.n; ++i) {
        double x1, y1, x2, y2;
        image2world(it.camera_model1, cam1, it.uv1[2 * i], it.uv1[2 * i + 1], x1, y1);
        image2world(it.camera_model2, cam2, it.uv2[2 * i], it.uv2[2 * i + 1], x2, y2);
        pts[b + i] = make_double4(x1, y1, x2, y2);
      }
      for (long long k = 0; k <= it.n; ++k) table[(size_t)(d.table_begin + k)] = e5_dynamic_limit(k, it.n, it.probability);
      if (it.samples)
        for (int t = 0; t < it.max_trials; ++t) {
          int a0 = it.samples[5 * t], a1 = it.samples[5 * t + 1], a2 = it.samples[5 * t + 2], a3 = it.samples[5 * t + 3], a4 = it.samples[5 * t + 4];
          e5_sort5(a0, a1, a2, a3, a4);
          int* o = srows.data() + 5 * ((size_t)d.samples_begin + t);
          o[0] = a0; o[1] = a1; o[2] = a2; o[3] = a3; o[4] = a4;
        }
    }
    // ---- launch ----
    StreamScope call;
    hipStream_t st = call.st;
    DevBuf<RansacItemDev> d_items; DevBuf<int2> d_map; DevBuf<double4> d_pts; DevBuf<int> d_srows, d_table, d_nm, d_cnt, d_samp;
    DevBuf<double> d_models, d_z, d_sum; DevBuf<unsigned char> d_mask; DevBuf<unsigned> d_done; DevBuf<RelResultDev> d_res;
    d_items.upload(hd, st); d_map.upload(map, st); d_pts.upload(pts, st); d_srows.upload(srows, st); d_table.upload(table, st);
    d_nm.alloc(T); d_models.alloc(90 * T); d_z.alloc(10 * T); d_cnt.alloc(10 * T); d_sum.alloc(10 * T); d_samp.alloc(5 * T); d_mask.alloc(N);
    d_done.alloc((size_t)count); d_res.alloc((size_t)count);
    d_done.zero(st);
    call.begin();
    hipLaunchKernelGGL(k_relative_pose, dim3((unsigned)batch.blocks), dim3(256), 0, st, d_items.p, d_map.p, d_pts.p, d_srows.p, d_table.p, d_nm.p,
                       d_models.p, d_z.p, d_cnt.p, d_sum.p, d_samp.p, d_mask.p, d_done.p, d_res.p);
    call.end();
    // ---- download: one array per kind some item asked for ----
    call.download(h_res, d_res.p, (size_t)count);
    call.download(h_nm, d_nm.p, T, want_nm);
    call.download(h_models, d_models.p, 90 * T, want_models);
    call.download(h_z, d_z.p, 10 * T, want_z);
    call.download(h_cnt, d_cnt.p, 10 * T, want_cnt);
    call.download(h_sum, d_sum.p, 10 * T, want_sum);
    call.download(h_samp, d_samp.p, 5 * T, want_samp);
    call.download(h_mask, d_mask.p, N, want_mask);
    call.finish();
    kernel_seconds = call.seconds();
  }
  // ---- scatter: nothing of the caller's was written before this point ----
  const double nan = std::numeric_limits<double>::quiet_NaN();
  for (int q = 0; q < count; ++q) {
    mavba_relpose_item& it = items[q];
    const RansacItemDev& d = hd[q];
    const size_t n = (size_t)it.n, mt = (size_t)it.max_trials;
    if (d.num_blocks == 0) {  // n <= 5 (the reference's first domain_error) or no trial at all
      RelResultDev& r = h_res[q];
      for (int k = 0; k < 9; ++k) r.E[k] = r.R[k] = nan;
      for (int k = 0; k < 3; ++k) r.rvec[k] = r.tvec[k] = nan;
      for (int k = 0; k < 4; ++k) r.cheir[k] = 0;
      r.forward_z = nan;
      r.cheir_best = -1; r.num_inliers = 0; r.best_trial = -1; r.best_model = -1; r.trials_used = 0; r.status = kRelposeNoConsensus;
      if (it.inlier_mask && n) std::memset(it.inlier_mask, 0, n);
      if (it.trial_num_models) std::fill(it.trial_num_models, it.trial_num_models + mt, 0);
      if (it.trial_models) std::fill(it.trial_models, it.trial_models + 90 * mt, nan);
      if (it.trial_z) std::fill(it.trial_z, it.trial_z + 10 * mt, nan);
      if (it.trial_num_inliers) std::fill(it.trial_num_inliers, it.trial_num_inliers + 10 * mt, 0);
      if (it.trial_residual_sum) std::fill(it.trial_residual_sum, it.trial_residual_sum + 10 * mt, 0.0);
      if (it.trial_samples) std::fill(it.trial_samples, it.trial_samples + 5 * mt, -1);
    } else {
      const size_t pb = (size_t)d.pt_begin, tb = (size_t)d.trial_begin;
      if (it.inlier_mask) std::memcpy(it.inlier_mask, h_mask.data() + pb, n);
      if (it.trial_num_models) std::memcpy(it.trial_num_models, h_nm.data() + tb, mt * sizeof(int));
      if (it.trial_models) std::memcpy(it.trial_models, h_models.data() + 90 * tb, 90 * mt * sizeof(double));
      if (it.trial_z) std::memcpy(it.trial_z, h_z.data() + 10 * tb, 10 * mt * sizeof(double));
      if (it.trial_num_inliers) std::memcpy(it.trial_num_inliers, h_cnt.data() + 10 * tb, 10 * mt * sizeof(int));
      if (it.trial_residual_sum) std::memcpy(it.trial_residual_sum, h_sum.data() + 10 * tb, 10 * mt * sizeof(double));
      if (it.trial_samples) std::memcpy(it.trial_samples, h_samp.data() + 5 * tb, 5 * mt * sizeof(int));
    }
    const RelResultDev& r = h_res[q];
    for (int k = 0; k < 9; ++k) { it.E[k] = r.E[k]; it.R[k] = r.R[k]; }
    for (int k = 0; k < 3; ++k) { it.rvec[k] = r.rvec[k]; it.tvec[k] = r.tvec[k]; }
    for (int k = 0; k < 4; ++k) it.cheirality_counts[k] = r.cheir[k];
    it.cheirality_best = r.cheir_best; it.forward_z = r.forward_z;
    it.num_inliers = r.num_inliers; it.best_trial = r.best_trial; it.best_model = r.best_model; it.trials_used = r.trials_used; it.status = r.status;
    it.kernel_seconds = kernel_seconds;
  }
}

}  // namespace mavba

