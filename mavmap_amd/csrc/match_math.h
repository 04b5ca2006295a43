// match_math.h — brute-force descriptor matching of an image pair: the direct distance, the order of candidates, the
// spatial mask, the ratio test, the cross-check and the median disparity.
//
// These inline functions are the bodies of the kernels in match.hip. Like h4_math.h they are __host__ __device__, so
// tests/ can compile this header with g++ and check it without a GPU. There is no CPU path in the library:
// match_run_item below is the one-thread run of the g++ harnesses - exhaustive, with no screening, so it IS rules 1-6
// of include/mavba_match.h.
//
// What is evaluated (reference file:line):
//   candidates    max_distance_mask_, src/base2d/feature.cc:23-49
//   two nearest   cv::BFMatcher::knnMatch with k = 2 and NORM_L2, feature.cc:66-78, restated as rules 2 and 3
//   ratio test    ratio_test_, feature.cc:12-20
//   cross-check   feature.cc:85-101
//   median        median_feature_disparity, feature.cc:136-151, and median(), src/util/math.cc:12-26
//
// Everything is evaluated operation for operation as written, without fused multiply-adds (MAVBA_TRI_AS_WRITTEN): it
// needs only + - * / and sqrt, which round the same on the host and on the device.
#ifndef MAVBA_MATCH_MATH_H_
#define MAVBA_MATCH_MATH_H_

#include <stdint.h>

#include <algorithm>
#include <vector>

#include "tri_math.h"

namespace mavba {

constexpr int kMatchMaxDim = 128;

// dim: a multiple of 4 in [4, 128]
MAVBA_HD bool match_dim_ok(int dim) { return dim >= 4 && dim <= kMatchMaxDim && (dim & 3) == 0; }

// Rule 1 with max_distance >= 0: md2 = max_distance * max_distance (feature.cc:29); the coordinates are floats.
MAVBA_HD bool match_candidate(float x1, float y1, float x2, float y2, double md2) {
  MAVBA_TRI_AS_WRITTEN
  const double dx = (double)x1 - (double)x2, dy = (double)y1 - (double)y2;
  const double xx = dx * dx, yy = dy * dy;
  return xx + yy < md2;
}

// Rule 2: the squared distance of two descriptors, a float accumulator over k in order.
MAVBA_HD float match_d2(const float* a, const float* b, int dim) {
  MAVBA_TRI_AS_WRITTEN
  float acc = 0.0f;
  for (int k = 0; k < dim; ++k) {
    const float t = a[k] - b[k];
    const float p = t * t;
    acc = acc + p;
  }
  return acc;
}

// Rule 3: (s, i) comes before (t, j)
MAVBA_HD bool match_before(float s, int i, float t, int j) { return s < t || (s == t && i < j); }

// The running two nearest (s0, i0) <= (s1, i1) of a keypoint, an absent one with index -1, take candidate (s, j).
// A NaN is never a neighbour. The kernel uses this for the screening score and for the merge of its lane groups too.
// Selects, no branches: the four values stay in registers on the device.
MAVBA_HD void match_top2_insert(float s, int j, float& s0, int& i0, float& s1, int& i1) {
  const bool ok = s == s;
  const bool first = ok && (i0 < 0 || match_before(s, j, s0, i0));
  const bool second = ok && !first && (i1 < 0 || match_before(s, j, s1, i1));
  const float t1 = first ? s0 : (second ? s : s1);
  const int j1 = first ? i0 : (second ? j : i1);
  s0 = first ? s : s0; i0 = first ? j : i0;
  s1 = t1; i1 = j1;
}

MAVBA_HD float match_nan() { return __builtin_nanf(""); }

// The distance of a neighbour from its squared distance: the correctly rounded float root; NaN for an absent one.
MAVBA_HD float match_dist(float d2, int index) { return index < 0 ? match_nan() : sqrtf(d2); }

// Rule 4: a keypoint whose neighbours are (nn0, d0) and (nn1, d1) survives the ratio test.
MAVBA_HD bool match_survives(int nn1, float d0, float d1, double max_ratio) {
  if (nn1 < 0) return false;  // fewer than two neighbours: feature.cc:87, :92
  const float q = d0 / d1;
  return !((double)q > max_ratio);
}

// Rule 5: keypoint i of image 1 is a match (with nn12[2 i]).
MAVBA_HD bool match_is_match(int i, const int* nn12, const float* dist12, const int* nn21, const float* dist21, double max_ratio) {
  if (!match_survives(nn12[2 * i + 1], dist12[2 * i], dist12[2 * i + 1], max_ratio)) return false;
  const int j = nn12[2 * i];
  return match_survives(nn21[2 * j + 1], dist21[2 * j], dist21[2 * j + 1], max_ratio) && nn21[2 * j] == i;
}

// ---------------------------------------------------------------------------
// Host only: the median, what the host answers without the device, and one item on one thread (the g++ harnesses)
// ---------------------------------------------------------------------------
// Rule 6, from the matches [m][2]; NaN for m == 0 or NULL coordinates.
inline double match_median_disparity(const float* xy1, const float* xy2, const int32_t* matches, long long m) {
  MAVBA_TRI_AS_WRITTEN
  if (m <= 0 || !xy1 || !xy2) return (double)match_nan();
  std::vector<double> v((size_t)m);
  for (long long q = 0; q < m; ++q) {
    const long long i = matches[2 * q], j = matches[2 * q + 1];
    const double dx = (double)xy1[2 * i] - (double)xy2[2 * j], dy = (double)xy1[2 * i + 1] - (double)xy2[2 * j + 1];
    const double xx = dx * dx, yy = dy * dy;
    v[(size_t)q] = sqrt(xx + yy);
  }
  std::sort(v.begin(), v.end());
  const size_t mid = (size_t)m / 2;
  if (m % 2 == 1) return v[mid];
  return (v[mid - 1] + v[mid]) / 2.0;
}

template <typename Item>
inline bool match_item_runs(const Item& it) { return it.n1 >= 2 && it.n2 >= 2; }

// An item that does not run (n1 < 2 or n2 < 2). Item: mavba_match_item (a template so that this header needs no C header).
template <typename Item>
inline void match_answer_without_run(Item& it) {
  for (long long i = 0; i < 2 * it.n1; ++i) {
    if (it.nn12) it.nn12[i] = -1;
    if (it.dist12) it.dist12[i] = match_nan();
  }
  for (long long j = 0; j < 2 * it.n2; ++j) {
    if (it.nn21) it.nn21[j] = -1;
    if (it.dist21) it.dist21[j] = match_nan();
  }
  it.num_matches = 0;
  it.median_disparity = (double)match_nan();
}

// The mask is on for every max_distance that is not below 0.
MAVBA_HD bool match_masked(double max_distance) { return !(max_distance < 0.0); }

// The two nearest of every keypoint of `a` [na][dim] among `b` [nb][dim], exhaustively: nn [na][2], dist [na][2].
inline void match_two_nearest(const float* a, const float* xya, long long na, const float* b, const float* xyb, long long nb, int dim,
                              double max_distance, int32_t* nn, float* dist) {
  const bool masked = match_masked(max_distance);
  const double md2 = max_distance * max_distance;
  for (long long i = 0; i < na; ++i) {
    float s0 = 0.0f, s1 = 0.0f;
    int i0 = -1, i1 = -1;
    for (long long j = 0; j < nb; ++j) {
      // (dx*dx and dy*dy do not depend on the sign of dx and dy: the mask is the same in both directions)
      if (masked && !match_candidate(xya[2 * i], xya[2 * i + 1], xyb[2 * j], xyb[2 * j + 1], md2)) continue;
      match_top2_insert(match_d2(a + i * dim, b + j * dim, dim), (int)j, s0, i0, s1, i1);
    }
    nn[2 * i] = i0; nn[2 * i + 1] = i1;
    dist[2 * i] = match_dist(s0, i0); dist[2 * i + 1] = match_dist(s1, i1);
  }
}

// One item by rules 1-6, on one thread: the same outputs as the call (kernel_seconds is left alone). The item's
// arguments are taken as valid (the library's entry point judges them).
template <typename Item>
inline void match_run_item(Item& it) {
  if (!match_item_runs(it)) { match_answer_without_run(it); return; }
  const long long n1 = it.n1, n2 = it.n2;
  std::vector<int32_t> nn12(2 * (size_t)n1), nn21(2 * (size_t)n2), matches;
  std::vector<float> d12(2 * (size_t)n1), d21(2 * (size_t)n2), distances;
  match_two_nearest(it.desc1, it.xy1, n1, it.desc2, it.xy2, n2, it.dim, it.max_distance, nn12.data(), d12.data());
  match_two_nearest(it.desc2, it.xy2, n2, it.desc1, it.xy1, n1, it.dim, it.max_distance, nn21.data(), d21.data());
  for (long long i = 0; i < n1; ++i)
    if (match_is_match((int)i, nn12.data(), d12.data(), nn21.data(), d21.data(), it.max_ratio)) {
      matches.push_back((int32_t)i); matches.push_back(nn12[2 * (size_t)i]);
      distances.push_back(d12[2 * (size_t)i]);
    }
  const long long m = (long long)distances.size();
  if (it.nn12) std::copy(nn12.begin(), nn12.end(), it.nn12);
  if (it.dist12) std::copy(d12.begin(), d12.end(), it.dist12);
  if (it.nn21) std::copy(nn21.begin(), nn21.end(), it.nn21);
  if (it.dist21) std::copy(d21.begin(), d21.end(), it.dist21);
  if (it.matches) std::copy(matches.begin(), matches.end(), it.matches);
  if (it.distances) std::copy(distances.begin(), distances.end(), it.distances);
  it.num_matches = (int32_t)m;
  it.median_disparity = match_median_disparity(it.xy1, it.xy2, matches.data(), m);
}

}  // namespace mavba
#endif  // MAVBA_MATCH_MATH_H_
