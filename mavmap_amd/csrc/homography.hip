// homography.hip - the batched view-change test of image pairs: a four-point homography inside RANSAC, ONE launch for
// any number of pairs.
//
// Replaces, per candidate pair, the host step before relative or absolute pose (reference
// src/sfm/sequential_mapper.cc:116-158 and :465-503 with src/base3d/projective_transform.cc and
// src/util/estimation.cc): 100 independent hypotheses, each scored against every match. The maths is h4_math.h; this
// file is the launch shape and the host packing. Nothing is lifted: the matches stay pixels, packed as one
// double4 (x, y, u, v) per match so that one load feeds a residual. The dynamic trial limit is tabulated once per item
// while packing; the per-item constants (threshold, offsets, seed) are uniform and the kernel reads them through
// scalar loads.
//
// Grid: the sum over items of ceil(max_trials_i / 16) work-groups; block_map[g] = (item, group of 16 trials). A wave
// owns four trials from sample to score and never talks to another wave:
//   hypothesis    lanes 0-3: lane = trial. The 8 x 9 system of a trial lives in the registers of its lane (h4_math.h
//                 indexes nothing at run time)
//   score         the model is broadcast into scalar registers (v_readlane); the 64 lanes stride the item's matches.
//                 Lane l adds the residuals of its inliers l, l + 64, ... in order, the wave reduction of dev_reduce.h
//                 adds the lanes: a fixed shape, so a trial's sum does not depend on the batch
// The item's LAST work-group to finish (an integer ticket, as in absolute_pose.hip) replays the selection over the
// trials in trial order, writes the best model's inlier mask and the item's record. No floating-point atomics, no
// spinning: a work-group never waits for another one.
#include "../../include/mavba_homography.h"
#include "batch_call.h"
#include "dev_reduce.h"
#include "h4_math.h"

namespace mavba {

static_assert(kHomographyOk == MAVBA_HOMOGRAPHY_OK && kHomographyNoConsensus == MAVBA_HOMOGRAPHY_NO_CONSENSUS, "status codes of h4_math.h and mavba_homography.h");

constexpr int kH4TrialsPerWave = 4;
constexpr int kH4TrialsPerGroup = 4 * kH4TrialsPerWave;  // tests/test_gpu_homography.py runs 15, 16 and 17 trials

struct H4ResultDev {
  double H[9];
  int num_inliers, best_trial, trials_used, status;
};

// Packed inputs: pts [N] matches (x, y, u, v), samples_in: the supplied rows (sorted), table: the dynamic limits.
// Per trial: models [T][9], cnt [T], sum [T], samp [T]. mask [N]. done: one ticket counter per item, zero on entry.
__global__ void __launch_bounds__(256) k_homography(const RansacItemDev* __restrict__ items, const int2* __restrict__ block_map,
                                                    const double4* __restrict__ pts, const int4* __restrict__ samples_in,
                                                    const int* __restrict__ table, double* models, int* cnt, double* sum, int4* samp,
                                                    unsigned char* mask, unsigned* done, H4ResultDev* results) {
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
  const int t0 = bm.y * kH4TrialsPerGroup + wv * kH4TrialsPerWave;  // the wave's first trial

  // ---- hypothesis: lane = trial ----
  double M[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) M[k] = NAN;
  bool valid = false;
  if (lane < kH4TrialsPerWave && t0 + lane < max_trials) {
    const int t = t0 + lane;
    int a[4];
    if (it.samples_begin >= 0) {
      const int4 row = samples_in[(size_t)it.samples_begin + t];
      a[0] = row.x; a[1] = row.y; a[2] = row.z; a[3] = row.w;
    } else {
      h4_draw_sample(it.seed, (unsigned)t, (unsigned)n, a);
    }
    samp[tb + t] = make_int4(a[0], a[1], a[2], a[3]);
    double m[4][4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const double4 p = pts[pb + a[k]];
      m[k][0] = p.x; m[k][1] = p.y; m[k][2] = p.z; m[k][3] = p.w;
    }
    valid = h4_estimate(m, M);
    double* out = models + 9 * (tb + t);
#pragma unroll
    for (int k = 0; k < 9; ++k) out[k] = M[k];
  }

  // ---- score: the wave's trials one after the other, the lanes stride the matches ----
  for (int j = 0; j < kH4TrialsPerWave; ++j) {
    const int t = t0 + j;
    if (t >= max_trials) break;
    double Mj[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) Mj[k] = wave_bcast(M[k], j);
    const bool ok = __builtin_amdgcn_readlane((int)valid, j) != 0;
    double s = 0.0;
    int c = 0;
    if (ok) {
      for (int i = lane; i < n; i += 64) {
        const double4 p = pts[pb + i];
        const double r = h4_residual(Mj, p.x, p.y, p.z, p.w);
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

  RansacSelect sel;  // (thread 0's)
  for (int base = 0; base < max_trials; base += 256) {
    const int t = base + tid;
    if (t < max_trials) {
      s_cnt[tid] = __hip_atomic_load(cnt + tb + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      s_sum[tid] = __hip_atomic_load(sum + tb + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      s_valid[tid] = h4_finite(__hip_atomic_load(models + 9 * (tb + t), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) ? 1 : 0;
    }
    __syncthreads();
    if (tid == 0) {
      const int m = max_trials - base < 256 ? max_trials - base : 256;
      int ended = 0;
      for (int k = 0; k < m && !ended; ++k)
        ended = h4_select_step(sel, base + k, s_valid[k] != 0, s_cnt[k], s_sum[k], table[(size_t)it.table_begin + s_cnt[k]], it.stop) ? 1 : 0;
      s_end = ended;
      s_best = sel.best_trial; s_used = sel.trials_used; s_inl = (int)sel.best_inliers;
    }
    __syncthreads();
    if (s_end) break;
  }
  const int best = s_best;
  const bool found = best >= 0 && s_inl >= 4;
  double B[9];
#pragma unroll
  for (int k = 0; k < 9; ++k)
    B[k] = found ? __hip_atomic_load(models + 9 * (tb + best) + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : NAN;
  for (int i = tid; i < n; i += 256) {
    bool inl = false;
    if (found) {
      const double4 p = pts[pb + i];
      inl = h4_residual(B, p.x, p.y, p.z, p.w) <= thr;
    }
    mask[pb + i] = inl ? 1 : 0;
  }
  if (tid == 0) {
    H4ResultDev& r = results[bm.x];
#pragma unroll
    for (int k = 0; k < 9; ++k) r.H[k] = B[k];
    r.num_inliers = found ? s_inl : 0;
    r.best_trial = found ? best : -1;
    r.trials_used = s_used;
    r.status = found ? kHomographyOk : kHomographyNoConsensus;
  }
}

// Host side, on the frame of batch_call.h: validate, pack, launch, download, scatter.
void homography_ransac(int count, mavba_homography_item* items, int device) {
  // ---- validate: every item is judged before the device is touched ----
  std::vector<RansacItemDev> hd((size_t)count);
  RansacBatch batch;
  bool want_mask = false, want_models = false, want_cnt = false, want_sum = false, want_samp = false;
  for (int q = 0; q < count; ++q) {
    const mavba_homography_item& it = items[q];
    check_item(it.n, it.max_trials >= 0 && !(it.n > 0 && (!it.uv1 || !it.uv2)), "homography");
    if (!(it.n > 4 && it.max_trials > 0)) continue;  // (such an item owns no work-group and is answered by the host)
    batch.place<4>(hd[q], it.n, it.max_trials, it.stop_num_inliers, it.seed, it.samples, kH4TrialsPerGroup, 9);
    hd[q].thr = it.max_reproj_error_px;
    want_mask |= it.inlier_mask != nullptr; want_models |= it.trial_models != nullptr; want_cnt |= it.trial_num_inliers != nullptr;
    want_sum |= it.trial_residual_sum != nullptr; want_samp |= it.trial_samples != nullptr;
  }
  require_device();
  DeviceScope on_device(device);
  double kernel_seconds = 0.0;
  std::vector<H4ResultDev> h_res((size_t)count);
  std::vector<double> h_models, h_sum;
  std::vector<int> h_cnt;
  std::vector<int4> h_samp;
  std::vector<unsigned char> h_mask;
  if (batch.blocks > 0) {
    // ---- pack ----
    const size_t N = (size_t)batch.points, T = (size_t)batch.trials;
    const std::vector<int2> map = make_block_map(hd, batch.blocks);
    std::vector<double4> pts(N);
    std::vector<int4> srows((size_t)batch.rows);
    std::vector<int> table((size_t)batch.table_len);
    for (int q = 0; q < count; ++q) {
      const mavba_homography_item& it = items[q];
      const RansacItemDev& d = hd[q];
      if (d.num_blocks == 0) continue;
      const size_t b = (size_t)d.pt_begin;
      for (size_t i = 0; i < (size_t)it.n; ++i) pts[b + i] = make_double4(it.uv1[2 * i], it.uv1[2 * i + 1], it.uv2[2 * i], it.uv2[2 * i + 1]);
      for (long long k = 0; k <= it.n; ++k) table[(size_t)(d.table_begin + k)] = h4_dynamic_limit(k, it.n, it.probability);
      if (it.samples)
        for (int t = 0; t < it.max_trials; ++t) {
          int a[4] = {it.samples[4 * t], it.samples[4 * t + 1], it.samples[4 * t + 2], it.samples[4 * t + 3]};
          h4_sort4(a);
          srows[(size_t)d.samples_begin + t] = make_int4(a[0], a[1], a[2], a[3]);
        }
    }
    // ---- launch ----
    StreamScope call;
    hipStream_t st = call.st;
    DevBuf<RansacItemDev> d_items; DevBuf<int2> d_map; DevBuf<double4> d_pts; DevBuf<int4> d_srows, d_samp; DevBuf<int> d_table, d_cnt;
    DevBuf<double> d_models, d_sum; DevBuf<unsigned char> d_mask; DevBuf<unsigned> d_done; DevBuf<H4ResultDev> d_res;
    d_items.upload(hd, st); d_map.upload(map, st); d_pts.upload(pts, st); d_srows.upload(srows, st); d_table.upload(table, st);
    d_models.alloc(9 * T); d_cnt.alloc(T); d_sum.alloc(T); d_samp.alloc(T); d_mask.alloc(N); d_done.alloc((size_t)count); d_res.alloc((size_t)count);
    d_done.zero(st);
    call.begin();
    hipLaunchKernelGGL(k_homography, dim3((unsigned)batch.blocks), dim3(256), 0, st, d_items.p, d_map.p, d_pts.p, d_srows.p, d_table.p,
                       d_models.p, d_cnt.p, d_sum.p, d_samp.p, d_mask.p, d_done.p, d_res.p);
    call.end();
    // ---- download: one array per kind some item asked for ----
    call.download(h_res, d_res.p, (size_t)count);
    call.download(h_models, d_models.p, 9 * T, want_models);
    call.download(h_cnt, d_cnt.p, T, want_cnt);
    call.download(h_sum, d_sum.p, T, want_sum);
    call.download(h_samp, d_samp.p, T, want_samp);
    call.download(h_mask, d_mask.p, N, want_mask);
    call.finish();
    kernel_seconds = call.seconds();
  }
  // ---- scatter: nothing of the caller's was written before this point ----
  for (int q = 0; q < count; ++q) {
    mavba_homography_item& it = items[q];
    const RansacItemDev& d = hd[q];
    const size_t n = (size_t)it.n, mt = (size_t)it.max_trials;
    if (d.num_blocks == 0) {  // n <= 4 (the reference's first domain_error) or no trial at all
      h4_answer_without_run(it);
    } else {
      const size_t pb = (size_t)d.pt_begin, tb = (size_t)d.trial_begin;
      if (it.inlier_mask) std::memcpy(it.inlier_mask, h_mask.data() + pb, n);
      if (it.trial_models) std::memcpy(it.trial_models, h_models.data() + 9 * tb, 9 * mt * sizeof(double));
      if (it.trial_num_inliers) std::memcpy(it.trial_num_inliers, h_cnt.data() + tb, mt * sizeof(int));
      if (it.trial_residual_sum) std::memcpy(it.trial_residual_sum, h_sum.data() + tb, mt * sizeof(double));
      if (it.trial_samples) std::memcpy(it.trial_samples, h_samp.data() + tb, mt * sizeof(int4));
      const H4ResultDev& r = h_res[q];
      for (int k = 0; k < 9; ++k) it.H[k] = r.H[k];
      it.num_inliers = r.num_inliers; it.inlier_ratio = (double)r.num_inliers / (double)it.n;
      it.best_trial = r.best_trial; it.trials_used = r.trials_used; it.status = r.status;
    }
    it.kernel_seconds = kernel_seconds;
  }
}

}  // namespace mavba
