/*
 * mavba_homography.h - the view-change test of an image pair: a four-point homography inside RANSAC (C ABI, same
 * library as mavba.h).
 *
 * A header of its own, like mavba_absolute_pose.h: mavba.h is the interface the drop-in replacement of
 * bundle_adjustment.cc is compiled against. A caller of the call below includes this file (it includes mavba.h for the
 * error codes).
 */
#ifndef MAVBA_HOMOGRAPHY_H_
#define MAVBA_HOMOGRAPHY_H_

#include "mavba.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * How much of an image pair's matches ONE homography explains, any number of pairs in ONE launch: one item is one
 * pair. Replaces, per candidate pair, the RANSAC of reference src/sfm/sequential_mapper.cc:116-158 (the initial pair)
 * and :465-503 (every later image) with the estimator of src/base3d/projective_transform.cc:12-74 inside
 * src/util/estimation.cc:15-146. The mapper discards a pair whose inlier share exceeds max_homography_inliers
 * (:153-156): too little parallax, a planar scene or a pure rotation. A pair that passes goes on to
 * mavba_relative_pose_ransac or mavba_absolute_pose_ransac.
 *
 * The result is that of the reference's RANSAC() run on one thread with the same samples.
 *
 * Input. uv1 / uv2 are PIXELS and stay pixels: nothing is lifted and no camera model is involved, the reference runs
 * this test on raw keypoint coordinates. max_reproj_error_px is the threshold as it is (:142).
 *
 * Samples. A trial's four indices are distinct, in [0, n), and used in ASCENDING order (the reference draws into a
 * std::set). `samples` [max_trials][4], when given, are sorted by the library; a row with a repeated or out-of-range
 * index is MAVBA_ERR_INVALID_ARGUMENT. With samples == NULL trial t draws its row with the counter-based generator of
 * mavba_absolute_pose.h (mix(t, d) and index(t, d) exactly as written there, rows of four).
 *
 * Items that run: n > 4 and max_trials > 0. Every other item is answered by the host: status NO_CONSENSUS, H NaN,
 * num_inliers 0, inlier_ratio 0 (also for n == 0), trials_used 0, best_trial -1, an all-zero inlier_mask and the trial
 * arrays filled as invalid trials with samples -1.
 *
 * Hypothesis. ProjectiveTransformEstimator::estimate, projective_transform.cc:18-31, for the four matches
 * (x, y) -> (u, v) of the row: the 8 x 9 system A h = 0 whose rows 0-3 are the x equations
 *     ( x  y  1  0  0  0  -x u  -y u  u )
 * and rows 4-7 the y equations
 *     ( 0  0  0  x  y  1  -x v  -y v  v ),
 * both in sample order. Its null vector h is divided by -h[8], then h[8] = 1 (:35-38); H is h row-major. This is the
 * reference's sign convention - its last column carries +u, not -u - and H maps (x, y, 1) onto a multiple of (u, v, 1).
 * The reference takes the null vector from an SVD of the unscaled system. The library scales every column of A by its
 * largest magnitude, eliminates with complete pivoting (the largest entry of the remaining block; of equal ones the
 * first row, then the first column), back-substitutes from the one free unknown and undoes the scaling: no iteration,
 * and for pixel coordinates, where the columns of A differ by five orders of magnitude, closer to the exact null
 * vector than the SVD (tests/test_homography_host.py measures both against 50 digits).
 * A trial whose H is not finite is INVALID: trial_num_inliers = 0, trial_residual_sum = 0, an all-NaN model, and it
 * never becomes the best.
 * The one place where the result may differ from the reference: a sample whose system has rank below 8 - three of the
 * four points collinear in either image, or a repeated point. There the reference returns an arbitrary member of a
 * null space of dimension two or more; the library returns either some member of that null space or an invalid trial.
 *
 * Score. projective_transform.cc:61-68: H (x, y, 1), divided by the third component, the distance to (u, v). The sign
 * of the third component is not tested, as in the reference. Inlier when residual <= threshold (a NaN is not an
 * inlier); the count, and the sum of the inliers' residuals. The sum has a fixed shape - lane l of one wave adds the
 * matches l, l + 64, ... in order, then the 64 lanes are added by the wave reduction - so results are bit-reproducible
 * and do not depend on what else is in the batch.
 *
 * Selection. estimation.cc:119-133 replayed over the trials in trial order, as in mavba_absolute_pose.h: trial t
 * becomes the best when num_inliers > best, or when the counts are equal and residual_sum < best_sum. After trial t
 * the run ends when best >= stop_num_inliers (<= 0: no stop), or when t >= dynamic_max_trials_(num_inliers of THIS
 * trial, n, 4, probability), tabulated on the host. trials_used = t + 1 of the ending trial (max_trials when none ends
 * it). Later trials are computed, since the launch is parallel, and ignored. The least consensus is 4 inliers
 * (estimation.cc:139-141); the reference has no refit on all inliers and neither has the library.
 */
#define MAVBA_HOMOGRAPHY_OK 0
#define MAVBA_HOMOGRAPHY_NO_CONSENSUS 1 /* n <= 4 (the reference's first domain_error), or best inliers < 4 (its second) */
/*
 * NO_CONSENSUS is an item result, not a call error: the other items are unaffected. Such an item has H NaN,
 * num_inliers 0, inlier_ratio 0, best_trial -1 and an all-zero inlier_mask; trials_used is what the replay used.
 * Call errors: MAVBA_ERR_INVALID_ARGUMENT (NULL or negative arguments, n >= 2^31, a bad sample row),
 * MAVBA_ERR_NO_DEVICE. Arguments are validated before the device is touched, and a failing call writes nothing of the
 * caller's. `device` as in mavba_triangulate_pairs: < 0 is the calling thread's current device, otherwise the call
 * runs on `device` and leaves the thread's current device as it found it.
 * An item with n == 0 may leave every pointer NULL.
 */
typedef struct mavba_homography_item {
  const double* uv1;           /* [n][2] PIXELS in the first image, used as they are                   */
  const double* uv2;           /* [n][2] PIXELS in the second image                                    */
  int64_t n;                   /* below 2^31                                                           */
  double max_reproj_error_px;  /* options.ransac_max_reproj_error: the threshold as it is              */
  int32_t max_trials;          /* the reference uses 100                                               */
  int64_t stop_num_inliers;    /* n * max_homography_inliers, sequential_mapper.cc:131-132; <= 0: none */
  double probability;          /* the reference uses 0.99                                              */
  const int32_t* samples;      /* [max_trials][4] or NULL                                              */
  uint64_t seed;               /* of the generator, used when samples == NULL                          */
  /* outputs: caller-owned arrays, each may be NULL */
  uint8_t* inlier_mask;        /* [n]                                                                  */
  double* trial_models;        /* [max_trials][9] row-major H                                          */
  int32_t* trial_num_inliers;  /* [max_trials]                                                         */
  double* trial_residual_sum;  /* [max_trials]                                                         */
  int32_t* trial_samples;      /* [max_trials][4] ascending                                            */
  /* outputs: scalars */
  double H[9];                 /* row-major: trial_models[best_trial], bit for bit                     */
  int32_t num_inliers;
  double inlier_ratio;         /* num_inliers / n as a double (0 for n == 0): what :153-156 compares   */
  int32_t best_trial;
  int32_t trials_used;
  int32_t status;              /* MAVBA_HOMOGRAPHY_*                                                   */
  double kernel_seconds;       /* device-event time of the batch's launch, the same in every item      */
} mavba_homography_item;
int mavba_homography_ransac(int32_t count, mavba_homography_item* items, int32_t device);

#ifdef __cplusplus
}
#endif
#endif /* MAVBA_HOMOGRAPHY_H_ */
