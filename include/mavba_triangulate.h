/*
 * mavba_triangulate.h - two-view triangulation with the mapper's acceptance tests (C ABI, same library as mavba.h).
 *
 * A header of its own: mavba.h is the interface the drop-in replacement of bundle_adjustment.cc is compiled against, and
 * that translation unit needs nothing of this. A caller of the call below includes this file (it includes mavba.h for the
 * error codes and MAVBA_MODEL_*).
 */
#ifndef MAVBA_TRIANGULATE_H_
#define MAVBA_TRIANGULATE_H_

#include "mavba.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Two-view triangulation with the mapper's acceptance tests, many image pairs in ONE launch.
 * Replaces, per image pair: camera_model_image2world of both point sets, the reprojection test of the continued
 * tracks, triangulate_points (DLT), calc_tri_angles, calc_reproj_errors and calc_depth with their thresholds -
 * reference src/sfm/sequential_mapper.cc:755-810 (map extension) and :302-349 (initial pair), on top of
 * src/base3d/triangulation.cc:12-147, src/base3d/projection.cc:107-149, src/base3d/camera_models.cc:24-52.
 *
 * Every item is independent; one thread handles one correspondence, results are in the caller's order.
 * `status` [n] holds, per correspondence, the tests it FAILED (each bit is the negation of the reference's
 * positive test, so a NaN sets the bit exactly where the reference rejects):
 */
#define MAVBA_TRI_REPROJ 1 /* !(reproj_error < max_reproj_error_px / ((fx2 + fy2) / 2))   image 2, normalised */
#define MAVBA_TRI_ANGLE  2 /* !(min_angle_deg in radians < min(angle, pi - angle))                             */
#define MAVBA_TRI_DEPTH2 4 /* !(calc_depth in image 2 > 0)                                                     */
#define MAVBA_TRI_DEPTH1 8 /* !(calc_depth in image 1 > 0)                                                     */
/*
 * A correspondence is accepted when status & mask == 0. For a new point mask = reject_bits. A continued track
 * (has_xyz[i] != 0) keeps its position: xyz = xyz_in, every quantity is evaluated there, and
 * mask = reject_bits & MAVBA_TRI_REPROJ (sequential_mapper.cc:766-777). The reference's map extension is
 * reject_bits = REPROJ | ANGLE | DEPTH2; its initial pair is reject_bits = DEPTH1 plus mean_folded_angle_deg.
 * The sums behind mean_folded_angle_deg and the compaction of `accepted` have a fixed shape: a call gives the same
 * bits twice, and an item gives the same bits alone as inside any batch.
 * Items with n == 0 are valid: num_accepted = 0 and mean_folded_angle_deg = NaN (0 / 0, as in the reference).
 * `device` < 0: the calling thread's current device; otherwise the call runs on `device` and leaves the thread's current
 * device as it found it. An item with n == 0 may leave every pointer NULL.
 */
typedef struct mavba_tri_pair {
  double rvec1[3], tvec1[3];   /* image 1 (the previous image)                                        */
  double rvec2[3], tvec2[3];   /* image 2 (the current image)                                         */
  const double* intrinsics1;   /* first K values of camera 1's parameters                             */
  const double* intrinsics2;
  int32_t camera_model1;       /* MAVBA_MODEL_*; the two images may differ in camera and model        */
  int32_t camera_model2;
  const double* uv1;           /* [n][2] pixels in image 1                                            */
  const double* uv2;           /* [n][2] pixels in image 2                                            */
  int64_t n;                   /* below 2^31                                                          */
  const double* xyz_in;        /* [n][3] or NULL: positions of the continued tracks                   */
  const uint8_t* has_xyz;      /* [n] or NULL (no continued track); needs xyz_in                      */
  double max_reproj_error_px;  /* options.tri_max_reproj_error                                        */
  double min_angle_deg;        /* options.tri_min_angle                                               */
  uint32_t reject_bits;        /* MAVBA_TRI_* that reject                                             */
  /* outputs: caller-owned arrays, each may be NULL */
  double* xyz;                 /* [n][3]                                                              */
  double* angle;               /* [n] radians, unfolded (NaN -> 0)                                    */
  double* reproj_error;        /* [n] image 2, normalised coordinates                                 */
  double* depth;               /* [n][2] calc_depth in image 1, image 2                               */
  int32_t* status;             /* [n] MAVBA_TRI_* bits                                                */
  int32_t* accepted;           /* [n]; the first num_accepted entries: accepted indices, ascending    */
  int64_t num_accepted;        /* out                                                                 */
  double mean_folded_angle_deg; /* out: mean of min(angle, pi - angle) over ALL n, degrees            */
  double kernel_seconds;       /* out: device-event time of the batch's launch, the same in every item: what    */
                               /* mavba_result.solve_seconds is to a solve - a caller sizing its batches, or    */
                               /* choosing between this call and its host code, reads it without a profiler     */
} mavba_tri_pair;
int mavba_triangulate_pairs(int32_t count, mavba_tri_pair* items, int32_t device);

#ifdef __cplusplus
}
#endif
#endif /* MAVBA_TRIANGULATE_H_ */
