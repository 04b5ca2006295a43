// triangulate.hip - batched two-view triangulation with the mapper's acceptance tests: ONE launch for any number of
// image pairs, one thread per correspondence.
//
// Replaces, per processed image pair, the host step between pose refinement and local BA (reference
// src/sfm/sequential_mapper.cc:755-810, and :302-349 for the initial pair): image2world of both point sets, the
// reprojection test of the continued tracks, DLT triangulation of the new pairs, triangulation angle, reprojection
// error and depth with their thresholds. The maths is tri_math.h; this file is the launch shape. What depends on the
// two poses only (both [R|t], the camera centres, the baseline: tri_pair_prepare) and the thresholds in their units are
// formed once per pair while packing; the kernel reads them through scalar loads.
//
// Grid: the sum over items of ceil(n_i / 256) work-groups; block_map[g] = (item, chunk) of work-group g. Per item
// the kernel also gives the mean folded angle, the number accepted and the ascending list of accepted indices. Their
// shape is fixed, so results are bit-reproducible and do not depend on what else is in the batch:
//   angle sum     DPP sum over each wave, the four waves in a fixed tree, one partial per work-group; the item's
//                 LAST work-group to finish (an integer ticket) adds the partials in chunk order
//   compaction    the same last work-group walks the item's status words chunk by chunk: ballot + popcount of the
//                 lanes below inside a wave, the four wave counts and the running base across waves and chunks
// No floating-point atomics, no spinning: a work-group never waits for another one.
#include "batch_call.h"
#include "dev_reduce.h"
#include "tri_math.h"

namespace mavba {

static_assert(kTriReproj == MAVBA_TRI_REPROJ && kTriAngle == MAVBA_TRI_ANGLE && kTriDepth2 == MAVBA_TRI_DEPTH2 && kTriDepth1 == MAVBA_TRI_DEPTH1,
              "status bits of tri_math.h and mavba_triangulate.h");

struct TriItemDev {
  long long begin;  // first correspondence of the item in the packed arrays
  int n, first_block, num_blocks;
  int model1, model2, reject_bits;
  double cam1[9], cam2[9];
  double rec[kTriRec];          // tri_pair_prepare: both projection matrices, camera centres, baseline (uniform: scalar loads)
  double thr_n, min_angle_rad;  // the two thresholds in the units of the tests
};

// Packed inputs: uv [N][4] = (u1, v1, u2, v2); has_xyz [N] and xyz_in [N][3] only when some item continues tracks (else null).
// Outputs over all N correspondences: xyz [N][3], angle [N], err [N], depth [N][2], status [N], accepted [N] (per item:
// its first num_accepted entries). part_angle: one partial per work-group. done: one ticket counter per item, zero on entry.
__global__ void __launch_bounds__(256) k_triangulate_pairs(const TriItemDev* __restrict__ items, const int2* __restrict__ block_map,
                                                           const double4* __restrict__ uv, const unsigned char* __restrict__ has_xyz,
                                                           const double* __restrict__ xyz_in, double* xyz, double* angle, double* err,
                                                           double2* depth, int* status, int* accepted, double* part_angle,
                                                           unsigned* done, int* num_accepted, double* mean_deg) {
  __shared__ double s_sum[4];
  __shared__ int s_cnt[4];
  __shared__ int s_last;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int2 bm = block_map[blockIdx.x];
  const TriItemDev& it = items[bm.x];
  const int n = it.n, reject_bits = it.reject_bits;
  const size_t begin = (size_t)it.begin;

  const int i = bm.y * 256 + tid;
  double folded = 0.0;
  if (i < n) {
    const size_t g = begin + (size_t)i;
    const double4 m = uv[g];
    const bool have = has_xyz != nullptr && has_xyz[g] != 0;
    double xin[3] = {0.0, 0.0, 0.0};
    if (have) { xin[0] = xyz_in[3 * g]; xin[1] = xyz_in[3 * g + 1]; xin[2] = xyz_in[3 * g + 2]; }
    double out[7];
    bool acc;
    const int st = tri_correspondence(it.rec, it.model1, it.cam1, it.model2, it.cam2, m.x, m.y, m.z, m.w, have, xin, it.thr_n,
                                      it.min_angle_rad, reject_bits, out, acc);
    xyz[3 * g] = out[0]; xyz[3 * g + 1] = out[1]; xyz[3 * g + 2] = out[2];
    angle[g] = out[3];
    err[g] = out[4];
    depth[g] = make_double2(out[5], out[6]);
    status[g] = st;
    folded = tri_fold(out[3]);
  }
  // this work-group's share of the angle sum (lanes past the end add 0)
  const double ws = wave_sum(folded);
  if (lane == 0) s_sum[wv] = ws;
  __syncthreads();
  if (tid == 0) part_angle[blockIdx.x] = (s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3]);

  // the item's last work-group to get here finishes the item
  if (!last_block_of_item(done, bm.x, it.num_blocks, &s_last)) return;

  if (tid == 0) {
    double s = 0.0;
    for (int c = 0; c < it.num_blocks; ++c) s += __hip_atomic_load(part_angle + it.first_block + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s /= (double)n;  // mean_tri_angle /= tri_angles.size(); mean_tri_angle *= RAD2DEG;
    mean_deg[bm.x] = s * (180.0 / kTriPi);
  }
  int base = 0;
  for (int c = 0; c < it.num_blocks; ++c) {
    const int j = c * 256 + tid;
    bool acc = false;
    if (j < n) {
      const size_t q = begin + (size_t)j;
      const int st = __hip_atomic_load(status + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      acc = tri_accept(st, has_xyz != nullptr && has_xyz[q] != 0, reject_bits);
    }
    const unsigned long long peers = __ballot(acc);
    const int below = __popcll(peers & ((1ull << lane) - 1ull));
    __syncthreads();  // s_cnt of the previous chunk has been read
    if (lane == 0) s_cnt[wv] = __popcll(peers);
    __syncthreads();
    const int c0 = s_cnt[0], c1 = s_cnt[1], c2 = s_cnt[2], c3 = s_cnt[3];
    const int before = wv == 0 ? 0 : (wv == 1 ? c0 : (wv == 2 ? c0 + c1 : c0 + c1 + c2));
    if (acc) accepted[begin + (size_t)(base + before + below)] = j;
    base += (c0 + c1) + (c2 + c3);
  }
  if (tid == 0) num_accepted[bm.x] = base;
}

// Host side, on the frame of batch_call.h: validate, pack, launch, download, scatter.
void triangulate_pairs(int count, mavba_tri_pair* items, int device) {
  // ---- validate: every item is judged before the device is touched ----
  std::vector<TriItemDev> hd((size_t)count);
  long long total = 0, blocks = 0;
  bool tracks = false, want_xyz = false, want_angle = false, want_err = false, want_depth = false, want_status = false, want_acc = false;
  for (int q = 0; q < count; ++q) {
    const mavba_tri_pair& it = items[q];
    check_item(it.n, !(it.n > 0 && (!it.intrinsics1 || !it.intrinsics2 || !it.uv1 || !it.uv2)) && !(it.has_xyz && !it.xyz_in), "triangulation");
    check_model(it.camera_model1);
    check_model(it.camera_model2);
    TriItemDev& d = hd[q];
    std::memset(&d, 0, sizeof(d));
    d.begin = total; d.n = (int)it.n; d.first_block = (int)blocks; d.num_blocks = (int)((it.n + 255) / 256);
    d.model1 = it.camera_model1; d.model2 = it.camera_model2; d.reject_bits = (int)it.reject_bits;
    if (it.n > 0) {  // (an empty item owns no work-group: its inputs may be NULL and are never read)
      for (int k = 0; k < model_k(it.camera_model1); ++k) d.cam1[k] = it.intrinsics1[k];
      for (int k = 0; k < model_k(it.camera_model2); ++k) d.cam2[k] = it.intrinsics2[k];
      // per pair, not per correspondence: the transcendental part of both poses is hoisted out of the kernel (as cam_prepare is)
      tri_pair_prepare(it.rvec1, it.tvec1, it.rvec2, it.tvec2, d.rec);
      d.thr_n = image2world_threshold(it.max_reproj_error_px, d.cam2);
      d.min_angle_rad = tri_min_angle_rad(it.min_angle_deg);
      tracks |= it.has_xyz != nullptr;
      want_xyz |= it.xyz != nullptr; want_angle |= it.angle != nullptr; want_err |= it.reproj_error != nullptr;
      want_depth |= it.depth != nullptr; want_status |= it.status != nullptr; want_acc |= it.accepted != nullptr;
    }
    total += it.n; blocks += d.num_blocks;
    if (total > kBatchMax) throw Failure(MAVBA_ERR_INVALID_ARGUMENT, "more than 2^31 - 1 correspondences in one batch");
  }
  require_device();
  DeviceScope on_device(device);
  double kernel_seconds = 0.0;
  std::vector<int> h_num((size_t)count, 0);
  std::vector<double> h_mean((size_t)count, std::numeric_limits<double>::quiet_NaN());  // n == 0: 0 / 0
  std::vector<double> h_xyz, h_angle, h_err, h_depth;
  std::vector<int> h_status, h_acc;
  if (blocks > 0) {
    // ---- pack ----
    const size_t N = (size_t)total;
    const std::vector<int2> map = make_block_map(hd, blocks);
    std::vector<double4> uv(N);
    std::vector<unsigned char> has(tracks ? N : 0, 0);
    std::vector<double> xin(tracks ? 3 * N : 0, 0.0);
    for (int q = 0; q < count; ++q) {
      const mavba_tri_pair& it = items[q];
      const size_t b = (size_t)hd[q].begin;
      for (size_t i = 0; i < (size_t)it.n; ++i) uv[b + i] = make_double4(it.uv1[2 * i], it.uv1[2 * i + 1], it.uv2[2 * i], it.uv2[2 * i + 1]);
      if (it.has_xyz)
        for (size_t i = 0; i < (size_t)it.n; ++i)
          if (it.has_xyz[i]) { has[b + i] = 1; xin[3 * (b + i)] = it.xyz_in[3 * i]; xin[3 * (b + i) + 1] = it.xyz_in[3 * i + 1]; xin[3 * (b + i) + 2] = it.xyz_in[3 * i + 2]; }
    }
    // ---- launch ----
    StreamScope call;
    hipStream_t st = call.st;
    DevBuf<TriItemDev> d_items; DevBuf<int2> d_map; DevBuf<double4> d_uv; DevBuf<unsigned char> d_has; DevBuf<double> d_xin;
    DevBuf<double> d_xyz, d_angle, d_err, d_part, d_mean; DevBuf<double2> d_depth; DevBuf<int> d_status, d_acc, d_num; DevBuf<unsigned> d_done;
    d_items.upload(hd, st); d_map.upload(map, st); d_uv.upload(uv, st);
    if (tracks) { d_has.upload(has, st); d_xin.upload(xin, st); }
    d_xyz.alloc(3 * N); d_angle.alloc(N); d_err.alloc(N); d_depth.alloc(N); d_status.alloc(N); d_acc.alloc(N);
    d_part.alloc((size_t)blocks); d_mean.alloc((size_t)count); d_num.alloc((size_t)count); d_done.alloc((size_t)count);
    d_done.zero(st);
    call.begin();
    hipLaunchKernelGGL(k_triangulate_pairs, dim3((unsigned)blocks), dim3(256), 0, st, d_items.p, d_map.p, d_uv.p, d_has.p, d_xin.p, d_xyz.p,
                       d_angle.p, d_err.p, d_depth.p, d_status.p, d_acc.p, d_part.p, d_done.p, d_num.p, d_mean.p);
    call.end();
    // ---- download: one array per kind some item asked for ----
    std::vector<int> num;
    std::vector<double> mean;
    call.download(num, d_num.p, (size_t)count);
    call.download(mean, d_mean.p, (size_t)count);
    for (int q = 0; q < count; ++q)  // (items with n == 0 own no work-group: their slots keep the host's values)
      if (hd[q].n > 0) { h_num[q] = num[q]; h_mean[q] = mean[q]; }
    call.download(h_xyz, d_xyz.p, 3 * N, want_xyz);
    call.download(h_angle, d_angle.p, N, want_angle);
    call.download(h_err, d_err.p, N, want_err);
    call.download(h_depth, d_depth.p, 2 * N, want_depth);
    call.download(h_status, d_status.p, N, want_status);
    call.download(h_acc, d_acc.p, N, want_acc);
    call.finish();
    kernel_seconds = call.seconds();
  }
  // ---- scatter: nothing of the caller's was written before this point ----
  for (int q = 0; q < count; ++q) {
    mavba_tri_pair& it = items[q];
    const size_t b = (size_t)hd[q].begin, n = (size_t)it.n;
    if (n > 0) {
      if (it.xyz) std::memcpy(it.xyz, h_xyz.data() + 3 * b, 3 * n * sizeof(double));
      if (it.angle) std::memcpy(it.angle, h_angle.data() + b, n * sizeof(double));
      if (it.reproj_error) std::memcpy(it.reproj_error, h_err.data() + b, n * sizeof(double));
      if (it.depth) std::memcpy(it.depth, h_depth.data() + 2 * b, 2 * n * sizeof(double));
      if (it.status) std::memcpy(it.status, h_status.data() + b, n * sizeof(int));
      if (it.accepted) std::memcpy(it.accepted, h_acc.data() + b, (size_t)h_num[q] * sizeof(int));
    }
    it.num_accepted = h_num[q];
    it.mean_folded_angle_deg = h_mean[q];
    it.kernel_seconds = kernel_seconds;
  }
}

}  // namespace mavba
