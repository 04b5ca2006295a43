// match.hip - batched brute-force descriptor matching of image pairs: the two nearest neighbours in both directions,
// the ratio test, the cross-check and the ordered list of matches, TWO launches for any number of pairs.
//
// Replaces, per image pair, match_brute_force() of reference src/base2d/feature.cc:52-102 as the mapper calls it
// (src/sfm/sequential_mapper.cc:2079-2083): the one dense n1 x n2 x dim product of process(). The rules are
// include/mavba_match.h's, the maths is match_math.h; this file is the launch shape and the host packing.
//
// k_match_screen, grid: the sum over items of ceil(n1 / 64) + ceil(n2 / 64) work-groups; block_map[g] = (item, strip).
// A strip is 64 keypoints of one image (its first ceil(n1 / 64) strips are image 1's, direction 1->2); it walks ALL
// descriptors of the other image in tiles of 64, each staged once in LDS with the squared norm of every row. A wave
// owns 16 keypoints of the strip and never talks to another wave:
//   product      v_mfma_f32_16x16x4_f32. The wave's own keypoints are the B operand (the column, lane & 15, is the
//                keypoint) and stay in registers for the whole walk; the walked descriptors are the A operand (rows).
//                The k of a step is permuted - lane group g of step (s, j) takes k = 16 s + 4 g + j in both operands -
//                so that a lane reads its A values as one 16-byte LDS load per 16 x 16 x 16 block; a descriptor is
//                padded with zeros to a multiple of 16. Four independent accumulators (the four 16-row blocks of a
//                tile) cover the instruction's 40-cycle dependent latency.
//   screening    score = (|a|^2 + |b|^2) - 2 a.b, rule 7 of the header. Every lane holds candidates of ONE keypoint, in
//                ascending index, and keeps its running two best in registers; the four lane groups of a column are
//                merged once at the end by (score, index).
//   epilogue     the two survivors of a keypoint are re-evaluated by rule 2 (lane groups 0 and 1, one survivor each),
//                ordered by rule 3 and written as nn / dist. Nothing behind this point sees a screening score.
// Both directions are strips of the same launch: the product is computed twice, there are no partial buffers, no merge
// pass, memory stays O(n) and the summation shape of a keypoint is fixed, whatever else is in the batch.
//
// k_match_decide, one work-group per item: the ratio test of both sides and the cross-check per keypoint of image 1
// (match_is_match), then an ordered compaction - a block scan over chunks of 256 keypoints with a carried offset - so
// the matches are ascending in i without atomics.
//
// One upload (records, block map, descriptors and coordinates in one buffer), one download (counts, nn, dist, matches).
// The median disparity is the host's (rule 6: it needs a full sort of at most min(n1, n2) values).
#include "../../include/mavba_match.h"
#include "batch_call.h"
#include "match_math.h"

namespace mavba {

constexpr int kMatchStrip = 64;                  // keypoints of a work-group: 16 per wave
constexpr int kMatchTile = 64;                   // walked descriptors staged at once: four 16-row blocks
constexpr int kMatchSteps = kMatchMaxDim / 16;   // blocks of 16 k of the longest descriptor
constexpr int kMatchMaxStride = kMatchMaxDim + 4;  // an LDS row: the padded descriptor + 4 floats (16 rows hit 16 x 4 banks)

typedef float match_f32x4 __attribute__((ext_vector_type(4)));

struct MatchItemDev {
  long long desc[2];  // where the descriptors of image 1 / 2 begin in the input floats (a multiple of 4)
  long long xy[2];    // where the coordinates begin (read when masked)
  long long out[2];   // where direction 1->2 / 2->1 begins in the output words: nn [n][2], then dist [n][2]
  long long out_matches;  // matches [min(n1, n2)][2], then distances [min(n1, n2)]
  double md2, max_ratio;
  int n[2];
  int dim, masked;
  int first_block = 0, num_blocks = 0, blocks1 = 0;  // num_blocks == 0: the host answers the item
};

__global__ void __launch_bounds__(256) k_match_screen(const MatchItemDev* __restrict__ items, const int2* __restrict__ block_map,
                                                      const float* __restrict__ in, int* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) float s_tile[kMatchTile * kMatchMaxStride];
  __shared__ float s_norm[kMatchTile];
  __shared__ float2 s_xy[kMatchTile];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int col = lane & 15, g = lane >> 4;
  const int2 bm = block_map[blockIdx.x];
  const MatchItemDev& it = items[bm.x];
  const int dir = bm.y >= it.blocks1 ? 1 : 0;
  const int strip = dir ? bm.y - it.blocks1 : bm.y;
  // (selects: an index into the record at run time would put a copy of it into scratch memory)
  const int n_own = dir ? it.n[1] : it.n[0], n_walk = dir ? it.n[0] : it.n[1], dim = it.dim;
  const int dimp = (dim + 15) & ~15, stride = dimp + 4, quads = dimp >> 2;
  const float* own_desc = in + (dir ? it.desc[1] : it.desc[0]);
  const float* walk_desc = in + (dir ? it.desc[0] : it.desc[1]);
  const float* own_xy = in + (dir ? it.xy[1] : it.xy[0]);
  const float* walk_xy = in + (dir ? it.xy[0] : it.xy[1]);
  int* nn_out = out + (dir ? it.out[1] : it.out[0]);
  const bool masked = it.masked != 0;
  const double md2 = it.md2;
  const int kp = strip * kMatchStrip + wv * 16 + col;  // the lane's keypoint (the same in the four lane groups)
  const bool kp_ok = kp < n_own;

  // ---- the wave's own keypoints: B operand of every step, and their squared norms ----
  float own[4 * kMatchSteps];
  float own_norm = 0.0f;
#pragma unroll
  for (int s = 0; s < kMatchSteps; ++s) {
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const int k = 16 * s + 4 * g;
    if (kp_ok && k < dim) v = *reinterpret_cast<const float4*>(own_desc + (size_t)kp * dim + k);
    own[4 * s] = v.x; own[4 * s + 1] = v.y; own[4 * s + 2] = v.z; own[4 * s + 3] = v.w;
    own_norm += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
  }
  own_norm += __shfl_xor(own_norm, 16);
  own_norm += __shfl_xor(own_norm, 32);
  float own_x = 0.0f, own_y = 0.0f;
  if (masked && kp_ok) {
    own_x = own_xy[2 * (size_t)kp];
    own_y = own_xy[2 * (size_t)kp + 1];
  }

  float s0 = 0.0f, s1 = 0.0f;  // the lane's two best by (score, index)
  int i0 = -1, i1 = -1;
  for (int base = 0; base < n_walk; base += kMatchTile) {
    __syncthreads();  // (the tile before this one has been read)
    // ---- stage 64 walked descriptors, zero beyond the image and beyond dim ----
    for (int idx = tid; idx < kMatchTile * quads; idx += 256) {
      const int r = idx / quads, c = idx - r * quads;
      float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (base + r < n_walk && 4 * c < dim) v = *reinterpret_cast<const float4*>(walk_desc + (size_t)(base + r) * dim + 4 * c);
      *reinterpret_cast<float4*>(s_tile + r * stride + 4 * c) = v;
    }
    if (masked && tid < kMatchTile) {
      float2 p = make_float2(0.0f, 0.0f);
      if (base + tid < n_walk) p = *reinterpret_cast<const float2*>(walk_xy + 2 * (size_t)(base + tid));
      s_xy[tid] = p;
    }
    __syncthreads();
    {  // the squared norm of every row: four threads per row, quads q, q + 4, ... each, then the four are added
      const int r = tid >> 2, q = tid & 3;
      float p = 0.0f;
      for (int c = q; c < quads; c += 4) {
        const float4 v = *reinterpret_cast<const float4*>(s_tile + r * stride + 4 * c);
        p += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
      }
      p += __shfl_xor(p, 1);
      p += __shfl_xor(p, 2);
      if (q == 0) s_norm[r] = p;
    }
    __syncthreads();

    // ---- 64 rows x 16 keypoints: four accumulators, row block a = rows 16 a .. 16 a + 15 ----
    match_f32x4 acc[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) acc[a] = match_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int s = 0; s < kMatchSteps; ++s) {
      if (16 * s < dimp) {  // (uniform)
        float4 av[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) av[a] = *reinterpret_cast<const float4*>(s_tile + (16 * a + col) * stride + 16 * s + 4 * g);
#pragma unroll
        for (int a = 0; a < 4; ++a) acc[a] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[a].x, own[4 * s], acc[a], 0, 0, 0);
#pragma unroll
        for (int a = 0; a < 4; ++a) acc[a] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[a].y, own[4 * s + 1], acc[a], 0, 0, 0);
#pragma unroll
        for (int a = 0; a < 4; ++a) acc[a] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[a].z, own[4 * s + 2], acc[a], 0, 0, 0);
#pragma unroll
        for (int a = 0; a < 4; ++a) acc[a] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[a].w, own[4 * s + 3], acc[a], 0, 0, 0);
      }
    }
    // ---- the lane's 16 results: column = its keypoint, row 16 a + 4 g + r of the tile, ascending ----
#pragma unroll
    for (int a = 0; a < 4; ++a) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 16 * a + 4 * g + r, j = base + row;
        const float score = (own_norm + s_norm[row]) - 2.0f * acc[a][r];
        bool cand = j < n_walk;
        if (masked) {
          const float2 p = s_xy[row];
          cand = cand && match_candidate(own_x, own_y, p.x, p.y, md2);
        }
        if (cand) match_top2_insert(score, j, s0, i0, s1, i1);
      }
    }
  }

  // ---- the four lane groups of a column: disjoint candidates, merged by (score, index) ----
#pragma unroll
  for (int off = 16; off <= 32; off += 16) {
    const float t0 = __shfl_xor(s0, off), t1 = __shfl_xor(s1, off);
    const int j0 = __shfl_xor(i0, off), j1 = __shfl_xor(i1, off);
    if (j0 >= 0) match_top2_insert(t0, j0, s0, i0, s1, i1);
    if (j1 >= 0) match_top2_insert(t1, j1, s0, i0, s1, i1);
  }

  // ---- rule 2 for the two survivors (lane group 0: the first, lane group 1: the second), rule 3 between them ----
  const int mine = g == 0 ? i0 : i1;
  float e = 0.0f;
  if (g < 2 && kp_ok && mine >= 0) e = match_d2(own_desc + (size_t)kp * dim, walk_desc + (size_t)mine * dim, dim);
  const float e_other = __shfl_xor(e, 16);
  if (g == 0 && kp_ok) {
    float e0 = e, e1 = e_other;
    if (i1 >= 0 && match_before(e1, i1, e0, i0)) {
      const float te = e0; e0 = e1; e1 = te;
      const int ti = i0; i0 = i1; i1 = ti;
    }
    int* nn = nn_out;
    int* dist = nn + 2 * (size_t)n_own;
    nn[2 * (size_t)kp] = i0;
    nn[2 * (size_t)kp + 1] = i1;
    dist[2 * (size_t)kp] = __float_as_int(match_dist(e0, i0));
    dist[2 * (size_t)kp + 1] = __float_as_int(match_dist(e1, i1));
  }
}

// out[q]: the number of matches of item q
__global__ void __launch_bounds__(256) k_match_decide(const MatchItemDev* __restrict__ items, int* out) {
  __shared__ int s_wave[4];
  const MatchItemDev& it = items[blockIdx.x];
  if (it.num_blocks == 0) return;  // (uniform: the host answers this item)
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int n1 = it.n[0], n2 = it.n[1], cap = n1 < n2 ? n1 : n2;
  const int* nn12 = out + it.out[0];
  const float* d12 = reinterpret_cast<const float*>(nn12 + 2 * (size_t)n1);
  const int* nn21 = out + it.out[1];
  const float* d21 = reinterpret_cast<const float*>(nn21 + 2 * (size_t)n2);
  int* matches = out + it.out_matches;
  float* distances = reinterpret_cast<float*>(matches + 2 * (size_t)cap);
  int carry = 0;  // matches of the chunks before this one (the same in every thread)
  for (int base = 0; base < n1; base += 256) {
    const int i = base + tid;
    const bool is = i < n1 && match_is_match(i, nn12, d12, nn21, d21, it.max_ratio);
    const unsigned long long b = __ballot(is);
    if (lane == 0) s_wave[wv] = __popcll(b);
    __syncthreads();
    int before = carry + __popcll(b & ((1ull << lane) - 1ull));
    for (int w = 0; w < wv; ++w) before += s_wave[w];
    carry += s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    if (is && before < cap) {  // (a match owns its i and its j: there are at most min(n1, n2))
      matches[2 * (size_t)before] = i;
      matches[2 * (size_t)before + 1] = nn12[2 * (size_t)i];
      distances[before] = d12[2 * (size_t)i];
    }
    __syncthreads();
  }
  if (tid == 0) out[blockIdx.x] = carry < cap ? carry : cap;
}

// Host side, on the frame of batch_call.h: validate, pack, launch, download, scatter.
void match_descriptors(int count, mavba_match_item* items, int device) {
  // ---- validate: every item is judged before the device is touched ----
  std::vector<MatchItemDev> hd((size_t)count);
  long long blocks = 0, in_floats = 0, out_words = count;
  auto place = [](long long& total, long long len) { const long long at = total; total += (len + 3) & ~3LL; return at; };
  for (int q = 0; q < count; ++q) {
    const mavba_match_item& it = items[q];
    const bool masked = match_masked(it.max_distance);
    check_item(it.n1, !(it.n1 > 0 && (!it.desc1 || (masked && !it.xy1))), "match");
    check_item(it.n2, !(it.n2 > 0 && (!it.desc2 || (masked && !it.xy2))) && match_dim_ok(it.dim) && it.max_ratio == it.max_ratio, "match");
    if (!match_item_runs(it)) continue;  // (such an item owns no work-group and is answered by the host)
    MatchItemDev& d = hd[q];
    const long long n1 = it.n1, n2 = it.n2, cap = std::min(n1, n2);
    d.n[0] = (int)n1; d.n[1] = (int)n2; d.dim = it.dim; d.masked = masked ? 1 : 0;
    d.md2 = it.max_distance * it.max_distance; d.max_ratio = it.max_ratio;
    d.desc[0] = place(in_floats, n1 * it.dim); d.desc[1] = place(in_floats, n2 * it.dim);
    d.xy[0] = d.xy[1] = 0;
    if (masked) { d.xy[0] = place(in_floats, 2 * n1); d.xy[1] = place(in_floats, 2 * n2); }
    d.out[0] = place(out_words, 4 * n1); d.out[1] = place(out_words, 4 * n2); d.out_matches = place(out_words, 3 * cap);
    d.blocks1 = (int)((n1 + kMatchStrip - 1) / kMatchStrip);
    d.first_block = (int)blocks; d.num_blocks = d.blocks1 + (int)((n2 + kMatchStrip - 1) / kMatchStrip);
    blocks += d.num_blocks;
    if (blocks > kBatchMax) throw Failure(MAVBA_ERR_INVALID_ARGUMENT, "more than 2^31 - 1 work-groups in one batch");
  }
  require_device();
  DeviceScope on_device(device);
  double kernel_seconds = 0.0;
  std::vector<int> h_out;
  if (blocks > 0) {
    // ---- pack: records | block map | floats, each part on a 16-byte boundary ----
    const std::vector<int2> map = make_block_map(hd, blocks);
    const size_t items_bytes = ((size_t)count * sizeof(MatchItemDev) + 15) & ~(size_t)15;
    const size_t map_bytes = (map.size() * sizeof(int2) + 15) & ~(size_t)15;
    std::vector<unsigned char> pack(items_bytes + map_bytes + (size_t)in_floats * sizeof(float));
    std::memcpy(pack.data(), hd.data(), (size_t)count * sizeof(MatchItemDev));
    std::memcpy(pack.data() + items_bytes, map.data(), map.size() * sizeof(int2));
    float* fl = reinterpret_cast<float*>(pack.data() + items_bytes + map_bytes);
    for (int q = 0; q < count; ++q) {
      const mavba_match_item& it = items[q];
      const MatchItemDev& d = hd[q];
      if (d.num_blocks == 0) continue;
      std::memcpy(fl + d.desc[0], it.desc1, (size_t)it.n1 * it.dim * sizeof(float));
      std::memcpy(fl + d.desc[1], it.desc2, (size_t)it.n2 * it.dim * sizeof(float));
      if (d.masked) {
        std::memcpy(fl + d.xy[0], it.xy1, 2 * (size_t)it.n1 * sizeof(float));
        std::memcpy(fl + d.xy[1], it.xy2, 2 * (size_t)it.n2 * sizeof(float));
      }
    }
    // ---- launch ----
    StreamScope call;
    hipStream_t st = call.st;
    DevBuf<unsigned char> d_in; DevBuf<int> d_out;
    d_in.upload(pack, st);
    d_out.alloc((size_t)out_words);
    const MatchItemDev* d_items = reinterpret_cast<const MatchItemDev*>(d_in.p);
    const int2* d_map = reinterpret_cast<const int2*>(d_in.p + items_bytes);
    const float* d_fl = reinterpret_cast<const float*>(d_in.p + items_bytes + map_bytes);
    call.begin();
    hipLaunchKernelGGL(k_match_screen, dim3((unsigned)blocks), dim3(256), 0, st, d_items, d_map, d_fl, d_out.p);
    hipLaunchKernelGGL(k_match_decide, dim3((unsigned)count), dim3(256), 0, st, d_items, d_out.p);
    call.end();
    // ---- download ----
    call.download(h_out, d_out.p, (size_t)out_words);
    call.finish();
    kernel_seconds = call.seconds();
  }
  // ---- scatter: nothing of the caller's was written before this point ----
  for (int q = 0; q < count; ++q) {
    mavba_match_item& it = items[q];
    const MatchItemDev& d = hd[q];
    if (d.num_blocks == 0) {
      match_answer_without_run(it);
    } else {
      const size_t n1 = (size_t)it.n1, n2 = (size_t)it.n2, cap = std::min(n1, n2);
      const int* o12 = h_out.data() + d.out[0];
      const int* o21 = h_out.data() + d.out[1];
      const int* om = h_out.data() + d.out_matches;
      const size_t m = (size_t)std::min<long long>(std::max(h_out[(size_t)q], 0), (long long)cap);
      if (it.nn12) std::memcpy(it.nn12, o12, 2 * n1 * sizeof(int));
      if (it.dist12) std::memcpy(it.dist12, o12 + 2 * n1, 2 * n1 * sizeof(float));
      if (it.nn21) std::memcpy(it.nn21, o21, 2 * n2 * sizeof(int));
      if (it.dist21) std::memcpy(it.dist21, o21 + 2 * n2, 2 * n2 * sizeof(float));
      if (it.matches) std::memcpy(it.matches, om, 2 * m * sizeof(int));
      if (it.distances) std::memcpy(it.distances, om + 2 * cap, m * sizeof(float));
      it.num_matches = (int32_t)m;
      it.median_disparity = match_median_disparity(it.xy1, it.xy2, om, (long long)m);
    }
    it.kernel_seconds = kernel_seconds;
  }
}

}  // namespace mavba
