/*
 * mavba_relative_pose.h - relative pose of an image pair from 2D-2D matches: the five-point essential-matrix solver
 * inside RANSAC, then the recovery of (R, t) (C ABI, same library as mavba.h).
 *
 * A header of its own, like mavba_absolute_pose.h: mavba.h is the interface the drop-in replacement of
 * bundle_adjustment.cc is compiled against. A caller of the call below includes this file (it includes mavba.h for the
 * error codes and MAVBA_MODEL_*).
 */
#ifndef MAVBA_RELATIVE_POSE_H_
#define MAVBA_RELATIVE_POSE_H_

#include "mavba.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Relative pose of an image pair from its matches, any number of pairs in ONE launch: one item is one pair.
 * Replaces, per candidate initial pair, reference src/sfm/sequential_mapper.cc:174-216 (the threshold conversion and
 * RANSAC with the five-point estimator) and :269-299 (pose_from_essential_matrix, rvec, the forward-motion figure) on
 * top of src/base3d/essential_matrix.cc:12-269 and src/util/estimation.cc:15-146. The call ends where
 * mavba_triangulate_pairs begins: rvec, tvec and inlier_mask are what the triangulation of the inliers with
 * reject_bits = MAVBA_TRI_DEPTH1 takes (sequential_mapper.cc:302-349).
 *
 * The result is the reference's RANSAC() on one thread with the same samples and each trial's models taken in
 * ascending z.
 *
 * Input. uv1 / uv2 are pixels; the library lifts them with each image's camera_model_image2world. The threshold is the
 * mean of the two cameras' camera_model_image2world_threshold(max_reproj_error_px) (sequential_mapper.cc:187-196).
 *
 * Samples. A trial's five indices are distinct, in [0, n), and used in ASCENDING order (the reference draws into a
 * std::set). `samples` [max_trials][5], when given, are sorted by the library; a row with a repeated or out-of-range
 * index is MAVBA_ERR_INVALID_ARGUMENT. With samples == NULL trial t draws its row with the counter-based generator of
 * mavba_absolute_pose.h (mix(t, d) and index(t, d) exactly as written there): d = 0, 1, 2, ...: index(t, d) is
 * appended to the row unless the row already holds it, until the row has FIVE entries; after d = 63 the row is
 * completed with the smallest indices it does not hold. Then the row is sorted.
 *
 * Hypothesis. EssentialMatrixEstimator::estimate:
 *   1. the 5 x 9 matrix Q of the epipolar constraint x2^T E x1 = 0, columns x1x2 y1x2 x2 x1y2 y1y2 y2 x1 y1 1;
 *   2. an orthonormal basis X, Y, Z, W of Q's null space. The reference takes the last four right singular vectors;
 *      this library takes the last four columns of the product of five Householder reflections that triangularise
 *      Q^T (no iteration). E does not depend on the basis in exact arithmetic;
 *   3. the ten cubic constraints of E = xX + yY + zZ + W over the 20 monomials of degree <= 3: det E = 0 and the nine
 *      entries of 2 E E^T E - tr(E E^T) E = 0. The reference includes generated code for them; this library forms
 *      them by polynomial arithmetic on the four basis matrices;
 *   4. Gauss-Jordan elimination with partial pivoting on the 10 x 20 matrix;
 *   5. the 3 x 3 matrix B(z) with entries of degree 3, 3 and 4 from the rows headed x2z, x2, y2z, y2, xyz, xy:
 *      <x2z> - z <x2>, <y2z> - z <y2>, <xyz> - z <xy>;
 *   6. the degree-10 polynomial det B(z);
 *   7. its roots by the reference's Durand-Kerner rule (util/math.cc:52): starting values (1 + i)^k, at most 100
 *      sweeps, ends when the largest correction is <= 1e-10. The update is the reference's sequential one (each root
 *      uses the roots already updated in the sweep): one thread owns a trial;
 *   8. a root is used when |imag| <= 1e-10;
 *   9. for each root the null vector (X0, X1, X2) of B(z) by a 3 x 3 one-sided Jacobi iteration; the root is skipped
 *      when |X2| < 1e-10;
 *  10. E = (X0 / X2) X + (X1 / X2) Y + z Z + W, divided by its Frobenius norm; row-major, x2^T E x1 = 0.
 * A model that is not finite is dropped. A trial's models are kept in ascending z (the reference's order is whatever
 * its root finder leaves; the order matters only in the trial that ends the run). trial_num_models [T] is the count,
 * trial_models [T][10][9] and trial_z [T][10] are NaN beyond it, trial_num_inliers and trial_residual_sum are 0 there.
 *
 * Score. EssentialMatrixEstimator::residuals: per point the signed Sampson quotient
 *     x2^T E x1 / sqrt((E x1)_0^2 + (E x1)_1^2 + (E^T x2)_0^2 + (E^T x2)_1^2);
 * inlier when fabs(residual) <= threshold (a NaN is never an inlier); the count, and the sum of the inliers' fabs. The
 * sum has a fixed shape - lane l of one wave adds the points l, l + 64, ... in order, then the 64 lanes are added by the
 * wave reduction - so results are bit-reproducible and do not depend on what else is in the batch.
 *
 * Selection. estimation.cc:98-133 replayed over the (trial, model) sequence, trials in order, a trial's models in
 * ascending z: a model becomes the best when num_inliers > best, or when the counts are equal and residual_sum <
 * best_sum (best starts at 0 and DBL_MAX). After EVERY model the run ends when best >= stop_num_inliers, or when
 * trial >= dynamic_max_trials_(num_inliers of THIS model, n, 5, probability); the later models of that trial are
 * ignored (the reference's `if (abort) continue`). A trial with zero models updates nothing and cannot end the run: in
 * the reference the abort test sits inside the model loop. The limit is formed on the host with the host's log, pow
 * and ceil; a quotient that is not finite means no limit, a finite one is clamped to [0, 2^31 - 1]. trials_used =
 * t + 1 of the ending trial (max_trials when none ends it). Later trials are computed, since the launch is parallel,
 * and ignored.
 *
 * Pose recovery. pose_from_essential_matrix over the inliers of the best model: E = U S V^T (3 x 3 one-sided Jacobi),
 * U and V made right-handed, W = [0 1 0; -1 0 0; 0 0 1], R1 = U W V^T, R2 = U W^T V^T, t = U.col(2); the candidates
 * (R1, t), (R2, t), (R1, -t), (R2, -t); for each, every inlier is triangulated by the DLT of mavba_triangulate.h
 * against [I | 0] and counted when 0 < depth < 100 in both views; the first candidate with a strictly larger count is
 * kept. U and V of a matrix with two equal singular values are not unique: the four candidates are the reference's
 * set, their order is the library's (which one is "R1" and the sign of "t" may differ from Eigen's). The four counts
 * are returned so that a caller can see a tie. rvec is Eigen's AngleAxisd(R), angle times axis. forward_z is
 * inv_second_proj_matrix(2, 3) = -(R^T t)_z, which the mapper tests at sequential_mapper.cc:291-299.
 * When every count is zero (the reference then leaves R and t unset) cheirality_best is -1 and R, tvec, rvec and
 * forward_z are NaN; E, the mask and the counts are still returned and status is MAVBA_RELPOSE_OK.
 */
#define MAVBA_RELPOSE_OK 0
#define MAVBA_RELPOSE_NO_CONSENSUS 1 /* n <= 5 (the reference's first domain_error), or best inliers < 5 (its second) */
/*
 * NO_CONSENSUS is an item result, not a call error: the other items are unaffected. Such an item has E, R, tvec, rvec
 * and forward_z NaN, num_inliers 0, cheirality_counts 0, best_trial, best_model and cheirality_best -1 and an all-zero
 * inlier_mask; trials_used is what the replay used (0 for n <= 5 or max_trials == 0, whose trial arrays are filled as
 * trials without a model, with samples -1).
 * Call errors: MAVBA_ERR_INVALID_ARGUMENT (NULL or negative arguments, n >= 2^31, a bad sample row),
 * MAVBA_ERR_BAD_MODEL, MAVBA_ERR_NO_DEVICE. Arguments are validated before the device is touched, and a failing call
 * writes nothing of the caller's. `device` as in mavba_triangulate_pairs: < 0 is the calling thread's current
 * device, otherwise the call runs on `device` and leaves the thread's current device as it found it.
 * MAVBA_ERR_NO_DEVICE comes before every item result: a batch is answered on a machine with a device only, also when
 * all its items have n <= 5 (their camera models are validated like any other item's).
 * An item with n == 0 may leave every pointer NULL.
 */
typedef struct mavba_relpose_item {
  const double* intrinsics1;   /* first K values of each camera's parameters                           */
  const double* intrinsics2;
  int32_t camera_model1;       /* MAVBA_MODEL_*                                                        */
  int32_t camera_model2;
  const double* uv1;           /* [n][2] PIXELS in image 1; lifted by the library                      */
  const double* uv2;           /* [n][2] PIXELS in image 2                                             */
  int64_t n;                   /* below 2^31                                                           */
  double max_reproj_error_px;  /* options.ransac_max_reproj_error                                      */
  int32_t max_trials;          /* the reference uses 1000                                              */
  int64_t stop_num_inliers;    /* <= 0: none (the reference passes n + 1: "run full max_trials")       */
  double probability;          /* the reference uses 0.99                                              */
  const int32_t* samples;      /* [max_trials][5] or NULL                                              */
  uint64_t seed;               /* of the generator, used when samples == NULL                          */
  /* outputs: caller-owned arrays, each may be NULL */
  uint8_t* inlier_mask;        /* [n]                                                                  */
  int32_t* trial_num_models;   /* [max_trials]                                                         */
  double* trial_models;        /* [max_trials][10][9] row-major E, unit Frobenius norm                 */
  double* trial_z;             /* [max_trials][10] ascending                                           */
  int32_t* trial_num_inliers;  /* [max_trials][10]                                                     */
  double* trial_residual_sum;  /* [max_trials][10]                                                     */
  int32_t* trial_samples;      /* [max_trials][5] ascending                                            */
  /* outputs: scalars */
  double E[9];                 /* trial_models[best_trial][best_model], bit for bit                    */
  double R[9];                 /* row-major                                                            */
  double tvec[3], rvec[3];
  int32_t cheirality_counts[4];
  int32_t cheirality_best;
  double forward_z;
  int32_t num_inliers;
  int32_t best_trial;
  int32_t best_model;
  int32_t trials_used;
  int32_t status;              /* MAVBA_RELPOSE_*                                                      */
  double kernel_seconds;       /* device-event time of the batch's launch, the same in every item      */
} mavba_relpose_item;
int mavba_relative_pose_ransac(int32_t count, mavba_relpose_item* items, int32_t device);

#ifdef __cplusplus
}
#endif
#endif /* MAVBA_RELATIVE_POSE_H_ */
