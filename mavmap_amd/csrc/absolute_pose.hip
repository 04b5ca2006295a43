// absolute_pose.hip - batched absolute pose from 2D-3D matches: P3P inside RANSAC, ONE launch for any number of images.
//
// Replaces, per registered image, the host step before pose refinement (reference src/sfm/sequential_mapper.cc:621-659
// with src/base3d/p3p.cc and src/util/estimation.cc): 500 independent hypotheses, each scored against every match.
// The maths is p3p_math.h; this file is the launch shape and the host packing. The observations are lifted
// (image2world) and the dynamic trial limit is tabulated once per item while packing; the per-item constants
// (threshold, offsets, seed) are uniform and the kernel reads them through scalar loads.
//
// Grid: the sum over items of ceil(max_trials_i / 16) work-groups; block_map[g] = (item, group of 16 trials). A wave
// owns four trials from sample to score and never talks to another wave:
//   hypothesis    lanes 0-15: lane = 4 * trial + candidate. The four lanes of a trial form Gao's system and find the
//                 roots (redundantly: that is shorter than exchanging them), each carries ONE root through the
//                 distances and the rigid fit; the minimum over a trial's candidates is taken with lane shuffles
//   score         the winning model is broadcast into scalar registers (v_readlane); the 64 lanes stride the item's
//                 points. Lane l adds the residuals of its inliers l, l + 64, ... in order, the wave reduction of
//                 dev_reduce.h adds the lanes: a fixed shape, so a trial's sum does not depend on the batch
// The item's LAST work-group to finish (an integer ticket, as in triangulate.hip) replays the selection over the trials
// in trial order, writes the best model's inlier mask and converts R to rvec. No floating-point atomics, no
// spinning: a work-group never waits for another one.
#include "batch_call.h"
#include "dev_reduce.h"
#include "p3p_math.h"

namespace mavba {

static_assert(kAbsposeOk == MAVBA_ABSPOSE_OK && kAbsposeNoConsensus == MAVBA_ABSPOSE_NO_CONSENSUS, "status codes of p3p_math.h and mavba_absolute_pose.h");

constexpr int kAbsTrialsPerWave = 4;
constexpr int kAbsTrialsPerGroup = 4 * kAbsTrialsPerWave;  // tests/test_gpu_absolute_pose.py runs 15, 16 and 17 trials

struct AbsResultDev {
  double rvec[3], tvec[3], P[12];
  int num_inliers, best_trial, trials_used, status;
};

// Packed inputs: xy [N] lifted observations, xyz [N] (w unused), samples_in: the supplied rows (sorted), table: the
// dynamic limits. Per trial: models [T][12], cnt [T], sum [T], samp [T]. mask [N]. done: one ticket counter per item,
// zero on entry.
__global__ void __launch_bounds__(256) k_absolute_pose(const RansacItemDev* __restrict__ items, const int2* __restrict__ block_map,
                                                       const double2* __restrict__ xy, const double4* __restrict__ xyz,
                                                       const int4* __restrict__ samples_in, const int* __restrict__ table, double* models,
                                                       int* cnt, double* sum, int4* samp, unsigned char* mask, unsigned* done,
                                                       AbsResultDev* results) {
  __shared__ int s_cnt[256];
  __shared__ double s_sum[256];
  __shared__ unsigned char s_valid[256];
  __shared__ int s_last, s_end, s_best, s_used, s_inl;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int2 bm = block_map[blockIdx.x];
  const RansacItemDev& it = items[bm.x];
  const int n = it.n, max_trials = it.max_trials;
  const size_t pb = (size_t)it.pt_begin, tb = (size_t)it.trial_begin;
  const double thr = it.thr;
  const int t0 = bm.y * kAbsTrialsPerGroup + wv * kAbsTrialsPerWave;  // the wave's first trial

  // ---- hypothesis: lane = 4 * trial + candidate ----
  double M[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) M[k] = NAN;
  double err = INFINITY;
  {
    const int t = t0 + (lane >> 2);
    if (lane < 4 * kAbsTrialsPerWave && t < max_trials) {
      int4 row;
      if (it.samples_begin >= 0) row = samples_in[(size_t)it.samples_begin + t];
      else p3p_draw_sample(it.seed, (unsigned)t, (unsigned)n, row.x, row.y, row.z, row.w);
      if ((lane & 3) == 0) samp[tb + t] = row;
      double x2d[8], X[12];
      const int idx[4] = {row.x, row.y, row.z, row.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const double2 o = xy[pb + idx[k]];
        const double4 p = xyz[pb + idx[k]];
        x2d[2 * k] = o.x; x2d[2 * k + 1] = o.y;
        X[3 * k] = p.x; X[3 * k + 1] = p.y; X[3 * k + 2] = p.z;
      }
      P3PSetup s;
      p3p_setup(x2d, X, s);
      double e;
      if (p3p_candidate(s, x2d, X, lane & 3, M, e) && e < DBL_MAX) err = e;
    }
  }
  // the minimum over the four lanes of a trial: the smallest error, of equal ones the lowest root number
  const int quad = lane & ~3;
  int win = -1;
  {
    double best = DBL_MAX;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const double e = __shfl(err, quad + c, 64);
      if (e < best) { best = e; win = c; }
    }
  }
  bool valid = win >= 0;
#pragma unroll
  for (int k = 0; k < 12; ++k) {
    M[k] = __shfl(M[k], quad + (win < 0 ? 0 : win), 64);
    valid = valid && p3p_finite(M[k]);
  }
  if (!valid) {
#pragma unroll
    for (int k = 0; k < 12; ++k) M[k] = NAN;
  }
  if (lane < 4 * kAbsTrialsPerWave && (lane & 3) == 0 && t0 + (lane >> 2) < max_trials) {
    double* out = models + 12 * (tb + t0 + (lane >> 2));
#pragma unroll
    for (int k = 0; k < 12; ++k) out[k] = M[k];
  }

  // ---- score: the wave's trials one after the other, the lanes stride the points ----
  for (int j = 0; j < kAbsTrialsPerWave; ++j) {
    const int t = t0 + j;
    if (t >= max_trials) break;
    double Mj[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) Mj[k] = wave_bcast(M[k], 4 * j);
    const bool ok = __builtin_amdgcn_readlane((int)valid, 4 * j) != 0;
    double s = 0.0;
    int c = 0;
    if (ok) {
      for (int i = lane; i < n; i += 64) {
        const double2 o = xy[pb + i];
        const double4 p = xyz[pb + i];
        const double r = p3p_residual(Mj, p.x, p.y, p.z, o.x, o.y);
        const bool inl = r <= thr;
        if (inl) s += r;
        c += __popcll(__ballot(inl));
      }
    }
    c = __builtin_amdgcn_readfirstlane(c);  // (lane 0 runs every iteration of the loop above: n >= 5)
    s = wave_sum(s);
    if (lane == 0) { cnt[tb + t] = c; sum[tb + t] = s; }
  }

  // ---- the item's last work-group to get here finishes the item ----
  if (!last_block_of_item(done, bm.x, it.num_blocks, &s_last)) return;

  P3PSelect sel;  // (thread 0's)
  for (int base = 0; base < max_trials; base += 256) {
    const int t = base + tid;
    if (t < max_trials) {
      s_cnt[tid] = __hip_atomic_load(cnt + tb + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      s_sum[tid] = __hip_atomic_load(sum + tb + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      s_valid[tid] = p3p_finite(__hip_atomic_load(models + 12 * (tb + t), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) ? 1 : 0;
    }
    __syncthreads();
    if (tid == 0) {
      const int m = max_trials - base < 256 ? max_trials - base : 256;
      int ended = 0;
      for (int k = 0; k < m && !ended; ++k)
        ended = p3p_select_step(sel, base + k, s_valid[k] != 0, s_cnt[k], s_sum[k], table[(size_t)it.table_begin + s_cnt[k]], it.stop) ? 1 : 0;
      s_end = ended;
      s_best = sel.best_trial; s_used = sel.trials_used; s_inl = (int)sel.best_inliers;
    }
    __syncthreads();
    if (s_end) break;
  }
  const int best = s_best;
  const bool found = best >= 0 && s_inl >= 4;
  double B[12];
#pragma unroll
  for (int k = 0; k < 12; ++k)
    B[k] = found ? __hip_atomic_load(models + 12 * (tb + best) + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : NAN;
  for (int i = tid; i < n; i += 256) {
    bool inl = false;
    if (found) {
      const double2 o = xy[pb + i];
      const double4 p = xyz[pb + i];
      inl = p3p_residual(B, p.x, p.y, p.z, o.x, o.y) <= thr;
    }
    mask[pb + i] = inl ? 1 : 0;
  }
  if (tid == 0) {
    AbsResultDev& r = results[bm.x];
#pragma unroll
    for (int k = 0; k < 12; ++k) r.P[k] = B[k];
    r.tvec[0] = B[3]; r.tvec[1] = B[7]; r.tvec[2] = B[11];
    if (found) {
      p3p_rvec_from_model(B, r.rvec);
    } else {
      r.rvec[0] = r.rvec[1] = r.rvec[2] = NAN;
    }
    r.num_inliers = found ? s_inl : 0;
    r.best_trial = found ? best : -1;
    r.trials_used = s_used;
    r.status = found ? kAbsposeOk : kAbsposeNoConsensus;
  }
}

// Host side, on the frame of batch_call.h: validate, lift and pack, launch, download, scatter.
void absolute_pose_ransac(int count, mavba_abspose_item* items, int device) {
  // ---- validate: every item is judged before the device is touched ----
  std::vector<RansacItemDev> hd((size_t)count);
  RansacBatch batch;
  bool want_mask = false, want_models = false, want_cnt = false, want_sum = false, want_samp = false;
  for (int q = 0; q < count; ++q) {
    const mavba_abspose_item& it = items[q];
    check_item(it.n, it.max_trials >= 0 && !(it.n > 0 && (!it.intrinsics || !it.uv || !it.xyz)), "absolute-pose");
    check_model(it.camera_model);
    if (!(it.n > 4 && it.max_trials > 0)) continue;  // (such an item owns no work-group and is answered by the host)
    batch.place<4>(hd[q], it.n, it.max_trials, it.stop_num_inliers, it.seed, it.samples, kAbsTrialsPerGroup, 12);
    want_mask |= it.inlier_mask != nullptr; want_models |= it.trial_models != nullptr; want_cnt |= it.trial_num_inliers != nullptr;
    want_sum |= it.trial_residual_sum != nullptr; want_samp |= it.trial_samples != nullptr;
  }
  require_device();
  DeviceScope on_device(device);
  double kernel_seconds = 0.0;
  std::vector<AbsResultDev> h_res((size_t)count);
  std::vector<double> h_models, h_sum;
  std::vector<int> h_cnt;
  std::vector<int4> h_samp;
  std::vector<unsigned char> h_mask;
  if (batch.blocks > 0) {
    // ---- lift and pack ----
    const size_t N = (size_t)batch.points, T = (size_t)batch.trials;
    const std::vector<int2> map = make_block_map(hd, batch.blocks);
    std::vector<double2> xy(N);
    std::vector<double4> xyz(N);
    std::vector<int4> srows((size_t)batch.rows);
    std::vector<int> table((size_t)batch.table_len);
    for (int q = 0; q < count; ++q) {
      const mavba_abspose_item& it = items[q];
      RansacItemDev& d = hd[q];
      if (d.num_blocks == 0) continue;
      double cam[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
      for (int k = 0; k < model_k(it.camera_model); ++k) cam[k] = it.intrinsics[k];
      d.thr = image2world_threshold(it.max_reproj_error_px, cam);
      const size_t b = (size_t)d.pt_begin;
      for (size_t i = 0; i < (size_t)it.n; ++i) {
        double x, y;
        image2world(it.camera_model, cam, it.uv[2 * i], it.uv[2 * i + 1], x, y);
        xy[b + i] = make_double2(x, y);
        xyz[b + i] = make_double4(it.xyz[3 * i], it.xyz[3 * i + 1], it.xyz[3 * i + 2], 0.0);
      }
      for (long long k = 0; k <= it.n; ++k) table[(size_t)(d.table_begin + k)] = p3p_dynamic_limit(k, it.n, it.probability);
      if (it.samples)
        for (int t = 0; t < it.max_trials; ++t) {
          int a0 = it.samples[4 * t], a1 = it.samples[4 * t + 1], a2 = it.samples[4 * t + 2], a3 = it.samples[4 * t + 3];
          p3p_sort4(a0, a1, a2, a3);
          srows[(size_t)d.samples_begin + t] = make_int4(a0, a1, a2, a3);
        }
    }
    // ---- launch ----
    StreamScope call;
    hipStream_t st = call.st;
    DevBuf<RansacItemDev> d_items; DevBuf<int2> d_map; DevBuf<double2> d_xy; DevBuf<double4> d_xyz; DevBuf<int4> d_srows, d_samp; DevBuf<int> d_table, d_cnt;
    DevBuf<double> d_models, d_sum; DevBuf<unsigned char> d_mask; DevBuf<unsigned> d_done; DevBuf<AbsResultDev> d_res;
    d_items.upload(hd, st); d_map.upload(map, st); d_xy.upload(xy, st); d_xyz.upload(xyz, st); d_srows.upload(srows, st); d_table.upload(table, st);
    d_models.alloc(12 * T); d_cnt.alloc(T); d_sum.alloc(T); d_samp.alloc(T); d_mask.alloc(N); d_done.alloc((size_t)count); d_res.alloc((size_t)count);
    d_done.zero(st);
    call.begin();
    hipLaunchKernelGGL(k_absolute_pose, dim3((unsigned)batch.blocks), dim3(256), 0, st, d_items.p, d_map.p, d_xy.p, d_xyz.p, d_srows.p, d_table.p,
                       d_models.p, d_cnt.p, d_sum.p, d_samp.p, d_mask.p, d_done.p, d_res.p);
    call.end();
    // ---- download: one array per kind some item asked for ----
    call.download(h_res, d_res.p, (size_t)count);
    call.download(h_models, d_models.p, 12 * T, want_models);
    call.download(h_cnt, d_cnt.p, T, want_cnt);
    call.download(h_sum, d_sum.p, T, want_sum);
    call.download(h_samp, d_samp.p, T, want_samp);
    call.download(h_mask, d_mask.p, N, want_mask);
    call.finish();
    kernel_seconds = call.seconds();
  }
  // ---- scatter: nothing of the caller's was written before this point ----
  const double nan = std::numeric_limits<double>::quiet_NaN();
  for (int q = 0; q < count; ++q) {
    mavba_abspose_item& it = items[q];
    const RansacItemDev& d = hd[q];
    const size_t n = (size_t)it.n, mt = (size_t)it.max_trials;
    if (d.num_blocks == 0) {  // n <= 4 (the reference's first domain_error) or no trial at all
      AbsResultDev& r = h_res[q];
      for (int k = 0; k < 3; ++k) r.rvec[k] = r.tvec[k] = nan;
      for (int k = 0; k < 12; ++k) r.P[k] = nan;
      r.num_inliers = 0; r.best_trial = -1; r.trials_used = 0; r.status = kAbsposeNoConsensus;
      if (it.inlier_mask && n) std::memset(it.inlier_mask, 0, n);
      if (it.trial_models) std::fill(it.trial_models, it.trial_models + 12 * mt, nan);
      if (it.trial_num_inliers) std::fill(it.trial_num_inliers, it.trial_num_inliers + mt, 0);
      if (it.trial_residual_sum) std::fill(it.trial_residual_sum, it.trial_residual_sum + mt, 0.0);
      if (it.trial_samples) std::fill(it.trial_samples, it.trial_samples + 4 * mt, -1);
    } else {
      const size_t pb = (size_t)d.pt_begin, tb = (size_t)d.trial_begin;
      if (it.inlier_mask) std::memcpy(it.inlier_mask, h_mask.data() + pb, n);
      if (it.trial_models) std::memcpy(it.trial_models, h_models.data() + 12 * tb, 12 * mt * sizeof(double));
      if (it.trial_num_inliers) std::memcpy(it.trial_num_inliers, h_cnt.data() + tb, mt * sizeof(int));
      if (it.trial_residual_sum) std::memcpy(it.trial_residual_sum, h_sum.data() + tb, mt * sizeof(double));
      if (it.trial_samples) std::memcpy(it.trial_samples, h_samp.data() + tb, mt * sizeof(int4));
    }
    const AbsResultDev& r = h_res[q];
    for (int k = 0; k < 3; ++k) { it.rvec[k] = r.rvec[k]; it.tvec[k] = r.tvec[k]; }
    for (int k = 0; k < 12; ++k) it.proj_matrix[k] = r.P[k];
    it.num_inliers = r.num_inliers; it.best_trial = r.best_trial; it.trials_used = r.trials_used; it.status = r.status;
    it.kernel_seconds = kernel_seconds;
  }
}

}  // namespace mavba

