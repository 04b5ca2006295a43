/*
 * mavba_obs_math.h - test entry of the per-observation arithmetic of csrc/ba_math.h (C ABI, same library as mavba.h).
 *
 * A header of its own: mavba.h is the interface the drop-in replacement of bundle_adjustment.cc is compiled against, and
 * that translation unit needs nothing of this.
 */
#ifndef MAVBA_OBS_MATH_H_
#define MAVBA_OBS_MATH_H_

#include "mavba.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Test entry: the per-observation functions of csrc/ba_math.h by the host build and by the device build on the same n
 * cases. kind (doubles in per case -> doubles out per case):
 *   0 rcp_obs (x -> 1)   1 rsqrt_obs (x -> 1)   2 log_obs (x -> 1)   3 rot_coeffs (th2 -> a, b, c)
 *   4 cauchy_weight (s, b -> w, half_rho)
 *   5 cam_prepare + obs_jacobian (model, pose[6], cam[9], X[3], uv[2] -> r[2], Jc[12], Jp[6], Jk[18])
 *   6 cam_prepare + obs_residual (as 5 -> r[2])
 *   7 cam_prepare + obs_backsub_term (as 5, then dc[6], dk[9] -> r[2], t[3])
 * out_host is always written; without a device the call then fails with MAVBA_ERR_NO_DEVICE. */
int mavba_debug_obs_math(int32_t kind, int32_t n, const double* in, double* out_host, double* out_device, int32_t device);

#ifdef __cplusplus
}
#endif
#endif
