/*
 * mavba_absolute_pose.h - absolute pose from 2D-3D matches: P3P inside RANSAC (C ABI, same library as mavba.h).
 *
 * A header of its own, like mavba_triangulate.h: mavba.h is the interface the drop-in replacement of
 * bundle_adjustment.cc is compiled against. A caller of the call below includes this file (it includes mavba.h for the
 * error codes and MAVBA_MODEL_*).
 */
#ifndef MAVBA_ABSOLUTE_POSE_H_
#define MAVBA_ABSOLUTE_POSE_H_

#include "mavba.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Absolute pose of an image from its 2D-3D matches, any number of images in ONE launch: one item is one image.
 * Replaces, per registered image, reference src/sfm/sequential_mapper.cc:621-659 (camera_model_image2world, the
 * threshold conversion, RANSAC with the P3P estimator, rvec from the best model) on top of src/base3d/p3p.cc:26-199
 * and src/util/estimation.cc:15-146. The call ends where mavba_pose_refine_item begins: rvec, tvec and inlier_mask
 * are what mavba_pose_refine_batch takes (sequential_mapper.cc:709-732).
 *
 * The result is that of the reference's RANSAC() run on one thread with the same samples.
 *
 * Samples. A trial's four indices are distinct, in [0, n), and used in ASCENDING order (the reference draws into a
 * std::set): the fourth point, the disambiguating point D of p3p.cc:44,59, is the one with the largest index.
 * `samples` [max_trials][4], when given, are sorted by the library; a row with a repeated or out-of-range index is
 * MAVBA_ERR_INVALID_ARGUMENT. With samples == NULL trial t draws its row with a counter-based integer generator.
 * All arithmetic is on unsigned 64-bit integers (wrapping); there is no state between trials and no floating point:
 *     mix(t, d):  z = seed + 0x9E3779B97F4A7C15 * (((uint64)t << 32) + d + 1)
 *                 z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9
 *                 z = (z ^ (z >> 27)) * 0x94D049BB133111EB
 *                 z =  z ^ (z >> 31)
 *     index(t, d) = ((z >> 32) * n) >> 32                      (multiply-high of the upper word by n, n < 2^31)
 *     d = 0, 1, 2, ...: index(t, d) is appended to the row unless the row already holds it, until the row has four
 *     entries. After d = 63 (never met for n >= 5 in practice; it bounds the loop) the row is completed with the
 *     smallest indices it does not hold. Then the row is sorted.
 *
 * Hypothesis. P3PEstimator::estimate: unit bearing vectors, the quartic of Gao et al. in x (roots by the reference's
 * Durand-Kerner iteration, util/math.cc:52, at most 100 sweeps, 1e-10), y = b0 / b1, the three distances, then the rigid
 * fit without scale of the three world points to the three camera points (Eigen::umeyama(..., false)); of the
 * candidates the one with the smallest reprojection error of D. A root is used when imag <= 1e-10 and real >= 0, as
 * in the reference: the test is on imag, not |imag|, so for a complex pair the reference also tries the pair's real
 * part once (through the root of negative imaginary part), and so does this library - that is cheaper to mirror than
 * to explain a mismatch. A trial with no candidate, or whose model is not finite, is INVALID: trial_num_inliers = 0,
 * trial_residual_sum = 0, a NaN model, and it never becomes the best (the reference scores uninitialised memory there).
 *
 * Score. Per point R X + t, divided by z, the distance to the lifted observation; inlier when residual <= threshold
 * (a NaN is not an inlier); the count, and the sum of the inliers' residuals. The sum has a fixed shape - lane l of
 * one wave adds the points l, l + 64, ... in order, then the 64 lanes are added by the wave reduction - so results are
 * bit-reproducible and do not depend on what else is in the batch.
 *
 * Selection. estimation.cc:119-133 replayed over the trials in trial order: trial t becomes the best when
 * num_inliers > best, or when the counts are equal and residual_sum < best_sum (best starts at 0 and DBL_MAX). After
 * trial t the run ends when best >= stop_num_inliers, or when t >= dynamic_max_trials_(num_inliers of THIS trial, n,
 * 4, probability) - the reference passes the current trial's count, not the best one. That limit is formed on the
 * host with the host's log, pow and ceil; a quotient that is not finite (k = 0 divides by log(1)) means no limit, a
 * finite one is clamped to [0, 2^31 - 1]. trials_used = t + 1 of the ending trial (max_trials when none ends it).
 * Later trials are computed, since the launch is parallel, and ignored.
 * rvec is Eigen's AngleAxisd(R) of the best model's rotation, angle times axis (sequential_mapper.cc:710-712).
 */
#define MAVBA_ABSPOSE_OK 0
#define MAVBA_ABSPOSE_NO_CONSENSUS 1 /* n <= 4 (the reference's first domain_error), or best inliers < 4 (its second) */
/*
 * NO_CONSENSUS is an item result, not a call error: the other items are unaffected. Such an item has rvec, tvec and
 * proj_matrix NaN, num_inliers 0, best_trial -1 and an all-zero inlier_mask; trials_used is what the replay used (0
 * for n <= 4 or max_trials == 0, whose trial arrays are filled as invalid trials with samples -1).
 * Call errors: MAVBA_ERR_INVALID_ARGUMENT (NULL or negative arguments, n >= 2^31, a bad sample row),
 * MAVBA_ERR_BAD_MODEL, MAVBA_ERR_NO_DEVICE. Arguments are validated before the device is touched, and a failing call
 * writes nothing of the caller's. `device` as in mavba_triangulate_pairs: < 0 is the calling thread's current
 * device, otherwise the call runs on `device` and leaves the thread's current device as it found it.
 * An item with n == 0 may leave every pointer NULL.
 */
typedef struct mavba_abspose_item {
  const double* intrinsics;    /* first K values of the camera's parameters                            */
  int32_t camera_model;        /* MAVBA_MODEL_*                                                        */
  const double* uv;            /* [n][2] PIXELS; lifted by the library (camera_model_image2world)      */
  const double* xyz;           /* [n][3]                                                               */
  int64_t n;                   /* below 2^31                                                           */
  double max_reproj_error_px;  /* options.max_reproj_error; converted as at sequential_mapper.cc:625   */
  int32_t max_trials;          /* the reference uses 500                                               */
  int64_t stop_num_inliers;    /* rel2abs_threshold already applied; <= 0: none                        */
  double probability;          /* the reference uses 0.99                                              */
  const int32_t* samples;      /* [max_trials][4] or NULL                                              */
  uint64_t seed;               /* of the generator above, used when samples == NULL                    */
  /* outputs: caller-owned arrays, each may be NULL */
  uint8_t* inlier_mask;        /* [n], the layout mavba_pose_refine_item.inlier_mask takes             */
  double* trial_models;        /* [max_trials][12] row-major [R|t]                                     */
  int32_t* trial_num_inliers;  /* [max_trials]                                                         */
  double* trial_residual_sum;  /* [max_trials]                                                         */
  int32_t* trial_samples;      /* [max_trials][4] ascending                                            */
  /* outputs: scalars */
  double rvec[3], tvec[3];
  double proj_matrix[12];      /* row-major [R|t]: trial_models[best_trial], bit for bit               */
  int32_t num_inliers;
  int32_t best_trial;
  int32_t trials_used;
  int32_t status;              /* MAVBA_ABSPOSE_*                                                      */
  double kernel_seconds;       /* device-event time of the batch's launch, the same in every item      */
} mavba_abspose_item;
int mavba_absolute_pose_ransac(int32_t count, mavba_abspose_item* items, int32_t device);

#ifdef __cplusplus
}
#endif
#endif /* MAVBA_ABSOLUTE_POSE_H_ */
