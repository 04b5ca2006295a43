/*
 * mavba_match.h - brute-force descriptor matching of image pairs: two nearest neighbours in both directions, the ratio
 * test, the cross-check and the median disparity (C ABI, same library as mavba.h).
 *
 * A header of its own, like mavba_homography.h: mavba.h is the interface the drop-in replacement of
 * bundle_adjustment.cc is compiled against. A caller of the call below includes this file (it includes mavba.h for the
 * error codes).
 */
#ifndef MAVBA_MATCH_H_
#define MAVBA_MATCH_H_

#include "mavba.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * The 2D-2D matches of image pairs, any number of pairs in TWO launches: one item is one pair. Replaces
 * match_brute_force() of reference src/base2d/feature.cc:52-102 with ratio_test = true, as
 * SequentialMapper::match_features_ calls it (src/sfm/sequential_mapper.cc:2079-2083), and the median_feature_disparity
 * of feature.cc:136-151 that the mapper gates a pair with (sequential_mapper.cc:100-113). The matches feed
 * mavba_homography_ransac and the pose calls behind it. The ratio_test = false branch of the reference
 * (feature.cc:103-131) is NOT offered: the mapper never takes it.
 *
 * The result is defined by rules 1-6 below, independently of how the kernel sums; rule 7 says where the library may
 * leave them. Everything is evaluated as written, without fused multiply-adds: a float32 loop on any machine gives the
 * same bits.
 *
 * 1. Candidates. Pair (i, j) - keypoint i of image 1, keypoint j of image 2 - is a candidate when max_distance < 0.
 *    Otherwise it is one when dx*dx + dy*dy < max_distance*max_distance, in double from the float coordinates
 *    (dx = (double)x1 - (double)x2), each product rounded, then the sum (feature.cc:29-40).
 * 2. Distance. d2(i, j) is a float accumulator from 0; for k = 0 .. dim-1 in order: t = a[k] - b[k]; p = t*t;
 *    acc = acc + p. d(i, j) is the correctly rounded float square root of d2. d2(i, j) and d2(j, i) are the same bits.
 * 3. Two nearest. A keypoint's candidates are ordered by (d2, index) ascending: of equal distances the lower index
 *    comes first. nn[.][0] and nn[.][1] are the first two; with fewer than two candidates the rest is -1 / NaN.
 * 4. Ratio test (feature.cc:12-20). A keypoint with two neighbours is dropped when (double)(d0 / d1) > max_ratio, the
 *    quotient being the correctly rounded float quotient. 0 / 0 is NaN, which is not greater: the keypoint stays, as in
 *    the reference. A keypoint with fewer than two neighbours is dropped (feature.cc:87, :92).
 * 5. Cross-check (feature.cc:85-101). (i, j) is a match when i survived in direction 1->2 with j = nn12[i][0], j
 *    survived in direction 2->1, and nn21[j][0] == i. The match's distance is d(i, j). Matches are written in
 *    ascending i: the reference's output order.
 * 6. Median disparity (feature.cc:136-151, src/util/math.cc:12-26). Per match sqrt(dx*dx + dy*dy) in double from the
 *    float coordinates; the values are sorted, the median is the middle value of an odd count and the mean of the two
 *    middle values of an even count; NaN for no matches or NULL coordinates. The HOST computes it from the downloaded
 *    matches - at most min(n1, n2) of them - since it needs a full sort. The size_t truncation of the reference's
 *    caller (sequential_mapper.cc:101) is the caller's business and is not reproduced.
 * 7. Screening. The library may find the two nearest by any score whose absolute error against the exact squared
 *    distance is at most eps(i, j) = 2 (dim + 3) 2^-24 (|a_i|^2 + |b_j|^2): the forward bound of the expanded form
 *    |a|^2 + |b|^2 - 2 a.b in float under any summation order. The two candidates that survive screening are
 *    re-evaluated by rule 2 and ordered by rule 3 before anything is decided or returned: returned distances and the
 *    ratio test never see the screening score. The one place the result may differ from rules 1-5: a keypoint whose
 *    second and third nearest exact squared distances lie within 2 eps of each other. For such a keypoint the library
 *    returns two of the candidates whose exact squared distance is at most that of the exact second nearest plus
 *    2 eps, in rule-3 order; which of them is not fixed. Results are bit-reproducible: they do not depend on what else
 *    is in the batch, on the item's position in it, or on which outputs are NULL. Non-finite descriptor entries are
 *    the caller's error and are not validated: the call terminates, indices stay in range or -1, and the matches of
 *    the affected keypoints are unspecified.
 *
 * Items that run: n1 >= 2 and n2 >= 2. Every other item is answered by the host: num_matches 0, median_disparity NaN,
 * nn* all -1, dist* all NaN (the reference likewise yields no match when either side offers fewer than two candidates,
 * feature.cc:87, :92). An item with n1 == 0 and n2 == 0 may leave every pointer NULL.
 *
 * Call errors: MAVBA_ERR_INVALID_ARGUMENT for a negative or >= 2^31 count, a NULL descriptor pointer with a positive
 * count, NULL xy* with max_distance >= 0, a dim that is not a multiple of 4 in [4, 128], a NaN max_ratio;
 * MAVBA_ERR_NO_DEVICE after the argument checks. Arguments are validated before the device is touched, and a failing
 * call writes nothing of the caller's. `device` as in mavba_triangulate_pairs: < 0 is the calling thread's current
 * device, otherwise the call runs on `device` and leaves the thread's current device as it found it.
 */
typedef struct mavba_match_item {
  const float* desc1;       /* [n1][dim] row-major                                                       */
  const float* desc2;       /* [n2][dim]                                                                 */
  const float* xy1;         /* [n1][2] keypoint PIXELS (cv::KeyPoint::pt); may be NULL if max_distance < 0 */
  const float* xy2;         /* [n2][2]                                                                   */
  int64_t n1;               /* below 2^31                                                                */
  int64_t n2;               /* below 2^31                                                                */
  int32_t dim;              /* a multiple of 4, 4 <= dim <= 128 (SURF: 64 or 128)                        */
  double max_ratio;         /* the mapper uses 0.9                                                       */
  double max_distance;      /* pixels; any value below 0: no spatial mask (the reference writes -1)      */
  /* outputs: caller-owned arrays, each may be NULL */
  int32_t* matches;         /* [min(n1, n2)][2]: (index in image 1, index in image 2), ascending in the first */
  float* distances;         /* [min(n1, n2)]: d(i, j) of every match                                     */
  int32_t* nn12;            /* [n1][2]: the two nearest candidates in image 2; absent: -1                */
  float* dist12;            /* [n1][2]: their distances; absent: NaN                                     */
  int32_t* nn21;            /* [n2][2]                                                                   */
  float* dist21;            /* [n2][2]                                                                   */
  /* outputs: scalars */
  int32_t num_matches;      /* rows of matches / distances that were written                             */
  double median_disparity;  /* rule 6; NaN for no matches or NULL coordinates                            */
  double kernel_seconds;    /* device-event time of the batch's launches, the same in every item         */
} mavba_match_item;
int mavba_match_descriptors(int32_t count, mavba_match_item* items, int32_t device);

#ifdef __cplusplus
}
#endif
#endif /* MAVBA_MATCH_H_ */
