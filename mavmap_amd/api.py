"""Python binding of the C ABI in include/mavba.h (ctypes; no torch types at the boundary).

Host-side mirror of the reference's bundle-adjustment interface
(reference src/base3d/bundle_adjustment.h:38-114, 212-230):

    BundleAdjustmentOptions      -> options dict / mavmap_amd.BundleAdjustmentOptions
    bundle_adjustment(...)       -> bundle_adjustment(problem, options)   (flat problem instead
                                    of FeatureManager; the C++ shim does the flattening for MAVMAP)
    pose_refinement(...)         -> pose_refinement(rvec, tvec, camera_params, points2D, points3D,
                                    inlier_mask, options)

There is no CPU fallback: without the built HIP library, or without a GPU, every compute call
raises MavbaError.
"""
import ctypes as C
import os
from dataclasses import dataclass

import numpy as np

from . import _abi as A
from .problem import BAProblem

_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libmavba.so")
_lib = None

EXPORTED_SYMBOLS = [
    "mavba_options_init", "mavba_last_error", "mavba_device_count", "mavba_solve", "mavba_pose_refine",
    "mavba_session_create", "mavba_session_destroy", "mavba_session_reset", "mavba_session_iterate",
    "mavba_session_result", "mavba_session_get_params", "mavba_session_point_errors",
    "mavba_session_set_allreduce", "mavba_session_eval_jacobian", "mavba_session_reduced_dim",
    "mavba_session_reduced_system", "mavba_session_linear_step", "mavba_session_time_jacobian", "mavba_session_time_front", "mavba_session_set_profiling",
    "mavba_session_kernel_stats", "mavba_session_get_info", "mavba_dense_spd_solve",
    "mavba_scene_create", "mavba_scene_destroy", "mavba_scene_set_camera", "mavba_scene_set_image", "mavba_scene_add_point2d",
    "mavba_scene_add_points2d", "mavba_scene_set_point3d", "mavba_scene_link", "mavba_scene_delete_point3d", "mavba_scene_get_image", "mavba_scene_get_point3d",
    "mavba_scene_get_camera", "mavba_scene_flatten", "mavba_scene_bundle_adjust",
    "mavba_rccl_unique_id", "mavba_session_set_rccl", "mavba_pose_refine_batch", "mavba_session_set_params", "mavba_session_restart", "mavba_session_filter_points", "mavba_solve_filter_solve",
    "mavba_debug_elimination_tree", "mavba_debug_radix_sort", "mavba_debug_lm_decide", "mavba_debug_chol_schedule",
    "mavba_debug_inproc_comms", "mavba_debug_upload_batch",
]
# include/mavba_triangulate.h (a header of its own: mavba.h is what the drop-in translation unit is compiled against);
# load() resolves them with their argument types, so a library without one does not load
TRIANGULATE_SYMBOLS = ["mavba_triangulate_pairs"]
# include/mavba_absolute_pose.h, likewise
ABSPOSE_SYMBOLS = ["mavba_absolute_pose_ransac"]
# include/mavba_relative_pose.h, likewise
RELPOSE_SYMBOLS = ["mavba_relative_pose_ransac"]
# include/mavba_homography.h, likewise
HOMOGRAPHY_SYMBOLS = ["mavba_homography_ransac"]
# include/mavba_match.h, likewise
MATCH_SYMBOLS = ["mavba_match_descriptors"]
# include/mavba_backsub_tiles.h, likewise
BACKSUB_TILES_SYMBOLS = ["mavba_debug_backsub_tiles"]
# include/mavba_obs_math.h, likewise
OBS_MATH_SYMBOLS = ["mavba_debug_obs_math"]

ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32)


class MavbaError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"mavba error {code}: {msg}")
        self.code = code


def lib_path():
    return _LIB_PATH


def load():
    """Load libmavba.so (raises MavbaError if it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB_PATH):
        raise MavbaError(A.ERR_NO_DEVICE, f"{_LIB_PATH} is missing: run `python -m mavmap_amd.build` "
                                          "(the HIP extension is mandatory, there is no CPU fallback)")
    L = C.CDLL(_LIB_PATH)
    dp, ip, bp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
    pp, op, rp = C.POINTER(A.CProblem), C.POINTER(A.COptions), C.POINTER(A.CResult)
    sp = C.c_void_p
    L.mavba_options_init.argtypes = [op]
    L.mavba_options_init.restype = None
    L.mavba_last_error.restype = C.c_char_p
    L.mavba_device_count.restype = C.c_int
    L.mavba_solve.argtypes = [pp, op, rp, dp]
    L.mavba_pose_refine.argtypes = [dp, dp, dp, C.c_int32, dp, dp, bp, C.c_int64, op, rp]
    L.mavba_session_create.argtypes = [pp, op, C.POINTER(sp)]
    L.mavba_session_destroy.argtypes = [sp]
    L.mavba_session_destroy.restype = None
    L.mavba_session_reset.argtypes = [sp]
    L.mavba_session_iterate.argtypes = [sp, C.c_int32, ip, ip]
    L.mavba_session_result.argtypes = [sp, rp]
    L.mavba_session_get_params.argtypes = [sp, dp, dp, dp]
    L.mavba_session_point_errors.argtypes = [sp, dp]
    L.mavba_session_set_allreduce.argtypes = [sp, ALLREDUCE_FN, C.c_void_p, C.c_int32, C.c_int32]
    L.mavba_session_eval_jacobian.argtypes = [sp, dp, dp, dp, dp, dp]
    L.mavba_session_reduced_dim.argtypes = [sp]
    L.mavba_session_reduced_system.argtypes = [sp, C.c_double, dp, dp]
    L.mavba_session_linear_step.argtypes = [sp, C.c_double, dp, dp, dp, dp]
    L.mavba_session_time_jacobian.argtypes = [sp, C.c_int32, C.POINTER(C.c_float)]
    L.mavba_session_time_front.argtypes = [sp, C.c_double, C.c_int32, C.POINTER(C.c_float)]
    L.mavba_session_set_profiling.argtypes = [sp, C.c_int32]
    L.mavba_session_kernel_stats.argtypes = [sp, C.POINTER(A.CKernelStat), C.c_int32]
    L.mavba_session_get_info.argtypes = [sp, C.POINTER(A.CSessionInfo)]
    L.mavba_dense_spd_solve.argtypes = [C.c_int32, dp, dp, dp, C.c_int32]
    i64p, i64 = C.POINTER(C.c_int64), C.c_int64
    sop = C.POINTER(A.CSceneOptions)
    L.mavba_scene_create.argtypes = [C.POINTER(sp)]
    L.mavba_scene_destroy.argtypes = [sp]
    L.mavba_scene_destroy.restype = None
    L.mavba_scene_set_camera.argtypes = [sp, i64, C.c_int32, dp]
    L.mavba_scene_set_image.argtypes = [sp, i64, i64, dp, dp]
    L.mavba_scene_add_point2d.argtypes = [sp, i64, i64, dp]
    L.mavba_scene_add_points2d.argtypes = [sp, i64, i64, i64p, dp, i64p]
    L.mavba_scene_set_point3d.argtypes = [sp, i64, dp]
    L.mavba_scene_link.argtypes = [sp, i64, i64]
    L.mavba_scene_delete_point3d.argtypes = [sp, i64]
    L.mavba_scene_get_image.argtypes = [sp, i64, dp, dp]
    L.mavba_scene_get_point3d.argtypes = [sp, i64, dp]
    L.mavba_scene_get_camera.argtypes = [sp, i64, ip, dp]
    lists = [i64p, i64, i64p, i64, i64p, i64, i64p, i64, i64p, dp, i64]
    L.mavba_scene_flatten.argtypes = [sp] + lists + [sop, pp, C.POINTER(i64p), C.POINTER(i64p), C.POINTER(i64p)]
    L.mavba_scene_bundle_adjust.argtypes = [sp] + lists + [sop, op, rp, dp, C.POINTER(i64p), C.POINTER(dp), i64p]
    L.mavba_rccl_unique_id.argtypes = [C.c_void_p]
    L.mavba_session_set_rccl.argtypes = [sp, C.c_void_p, C.c_int32, C.c_int32]
    L.mavba_pose_refine_batch.argtypes = [C.c_int32, C.POINTER(A.CPoseRefineItem), op, rp]
    L.mavba_triangulate_pairs.argtypes = [C.c_int32, C.POINTER(A.CTriPair), C.c_int32]
    L.mavba_triangulate_pairs.restype = C.c_int
    L.mavba_absolute_pose_ransac.argtypes = [C.c_int32, C.POINTER(A.CAbsPoseItem), C.c_int32]
    L.mavba_absolute_pose_ransac.restype = C.c_int
    L.mavba_relative_pose_ransac.argtypes = [C.c_int32, C.POINTER(A.CRelPoseItem), C.c_int32]
    L.mavba_relative_pose_ransac.restype = C.c_int
    L.mavba_homography_ransac.argtypes = [C.c_int32, C.POINTER(A.CHomographyItem), C.c_int32]
    L.mavba_homography_ransac.restype = C.c_int
    L.mavba_match_descriptors.argtypes = [C.c_int32, C.POINTER(A.CMatchItem), C.c_int32]
    L.mavba_match_descriptors.restype = C.c_int
    L.mavba_session_set_params.argtypes = [sp, dp, dp, dp]
    L.mavba_session_restart.argtypes = [sp]
    L.mavba_session_filter_points.argtypes = [sp, C.c_double, bp, bp, dp, C.POINTER(C.c_int64)]
    L.mavba_solve_filter_solve.argtypes = [pp, op, C.c_double, bp, rp, rp, dp, bp, C.POINTER(C.c_int64)]
    L.mavba_debug_elimination_tree.argtypes = [C.c_int32, C.c_int32, C.c_int64, ip, ip, C.c_int32, ip, ip, C.c_int32]
    L.mavba_debug_radix_sort.argtypes = [C.c_int32, C.POINTER(C.c_uint32), C.c_int32, ip, C.c_int32]
    L.mavba_debug_lm_decide.argtypes = [C.c_int32, dp, dp, dp, C.c_int32]
    L.mavba_debug_obs_math.argtypes = [C.c_int32, C.c_int32, dp, dp, dp, C.c_int32]
    L.mavba_debug_obs_math.restype = C.c_int
    L.mavba_debug_backsub_tiles.argtypes = [C.c_int32, ip, ip, C.c_int32]
    L.mavba_debug_backsub_tiles.restype = C.c_int
    i32p, i64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    L.mavba_debug_chol_schedule.argtypes = [C.c_int32, C.c_int32, i32p, i32p, i32p, C.c_int64, i32p, i32p, C.c_int32, dp,
                                            i32p, C.c_int64, i64p, i32p, C.c_int64, i64p, i32p]
    for f in EXPORTED_SYMBOLS:
        if f not in ("mavba_options_init", "mavba_last_error", "mavba_session_destroy", "mavba_scene_destroy", "mavba_debug_upload_batch"):
            getattr(L, f).restype = C.c_int
    _lib = L
    return L


def _check(rc):
    if rc != A.OK:
        raise MavbaError(rc, load().mavba_last_error().decode(errors="replace"))


def device_count():
    return int(load().mavba_device_count())


def _d(a):
    return A.ptr(a, C.c_double)


@dataclass
class BundleAdjustmentOptions:
    """Field-for-field mirror of the reference struct (bundle_adjustment.h:38-114)."""
    max_num_iterations: int = 100
    function_tolerance: float = 1e-4
    gradient_tolerance: float = 1e-8
    update_point3D_errors: bool = False
    min_track_len: int = 2
    loss_scale_factor: float = 1.0
    constrain_rotation: bool = False
    constrain_rotation_weight: float = 0.0
    refine_camera_params: bool = False
    print_progress: bool = False
    print_summary: bool = True

    @staticmethod
    def global_ba():
        """The values mapper.cc forces for global BA (reference src/mapper.cc:170-174, 878-881)."""
        return BundleAdjustmentOptions(max_num_iterations=200, function_tolerance=1e-6,
                                       gradient_tolerance=1e-10, update_point3D_errors=True,
                                       refine_camera_params=True, print_summary=False)


def make_options(opts=None, **kw):
    """COptions from a BundleAdjustmentOptions / dict plus overrides of the C-level fields."""
    o = A.COptions()
    load().mavba_options_init(C.byref(o))
    if isinstance(opts, BundleAdjustmentOptions):
        o.max_num_iterations = int(opts.max_num_iterations)
        o.function_tolerance = float(opts.function_tolerance)
        o.gradient_tolerance = float(opts.gradient_tolerance)
        o.loss_scale_factor = float(opts.loss_scale_factor)
        o.update_point_errors = int(bool(opts.update_point3D_errors))
        o.print_progress = int(bool(opts.print_progress))
    elif isinstance(opts, dict):
        kw = {**opts, **kw}
    for k, v in kw.items():
        if not hasattr(o, k):
            raise KeyError(k)
        setattr(o, k, v)
    return o


def print_report(res, title="Bundle Adjustment Report"):
    """stdout report in the reference's format (_print_report, bundle_adjustment.cc:114-136)."""
    n = max(res["num_residuals"], 1)
    print(title)
    print("-" * len(title))
    print(f"{'Residuals : ':>18}{res['num_residuals_reduced']}")
    print(f"{'Parameters : ':>18}{res['num_parameters_reduced']}")
    print(f"{'Iterations : ':>18}{res['num_successful_steps'] + res['num_unsuccessful_steps']}")
    print(f"{'Initial cost : ':>18}{np.sqrt(res['initial_cost'] / n):.6g} [px]")
    print(f"{'Final cost : ':>18}{np.sqrt(res['final_cost'] / n):.6g} [px]")
    print()


def bundle_adjustment(problem: BAProblem, options=None, point3D_errors=None, **kw):
    """Solve IN PLACE on `problem` (the reference mutates FeatureManager in place).

    Returns (final_cost_px, result) where final_cost_px = sqrt(final_cost / num_residuals)
    (the reference's return value, bundle_adjustment.cc:610) and `result` the summary dict.
    `point3D_errors`: optional float64 array [num_points], updated like the reference's map when
    options.update_point3D_errors is set.
    """
    if isinstance(options, BundleAdjustmentOptions):
        if options.min_track_len < 2:
            raise ValueError("Minimum track length must be >= 2 in order build valid bundle adjustment problem.")
    copt = make_options(options, **kw)
    res = A.CResult()
    cp = problem.c_struct()
    perr = None
    if point3D_errors is not None:
        copt.update_point_errors = 1
        perr = _d(point3D_errors)
    _check(load().mavba_solve(C.byref(cp), C.byref(copt), C.byref(res), perr))
    out = res.as_dict()
    if isinstance(options, BundleAdjustmentOptions) and options.print_summary:
        print_report(out)
    return float(np.sqrt(out["final_cost"] / out["num_residuals"])) if out["num_residuals"] else float("nan"), out


def bundle_adjustment_filter_rebundle(problem: BAProblem, filter_max_error, options=None, keep=None, point3D_errors=None, **kw):
    """Global BA, filter_point_cloud, global BA again on one resident session (reference src/mapper.cc:1206,
    1218-1224). Solves IN PLACE; returns (removed mask [num_points] uint8, first result, second result)."""
    copt = make_options(options, **kw)
    first, second = A.CResult(), A.CResult()
    cp = problem.c_struct()
    removed = np.zeros(problem.num_points, np.uint8)
    keep_arr = None if keep is None else np.ascontiguousarray(keep, dtype=np.uint8)
    n = C.c_int64()
    _check(load().mavba_solve_filter_solve(C.byref(cp), C.byref(copt), float(filter_max_error), A.ptr(keep_arr, C.c_uint8),
                                           C.byref(first), C.byref(second),
                                           _d(point3D_errors) if point3D_errors is not None else None,
                                           A.ptr(removed, C.c_uint8), C.byref(n)))
    assert int(removed.sum()) == n.value
    return removed, first.as_dict(), second.as_dict()


def pose_refinement(rvec, tvec, camera_params, points2D, points3D, inlier_mask=None, options=None, **kw):
    """Mirror of pose_refinement() (bundle_adjustment.h:212-218). `camera_params` carries the model
    code as its last element, exactly like FeatureManager.camera_params
    (reference src/sfm/sequential_mapper.cc:958-967). rvec/tvec are updated in place."""
    camera_params = np.asarray(camera_params, float)
    model = int(camera_params[-1])
    intr = A.as_f64(np.pad(camera_params[:-1], (0, 9 - (len(camera_params) - 1))))
    uv, xyz = A.as_f64(points2D, (-1, 2)), A.as_f64(points3D, (-1, 3))
    mask = None if inlier_mask is None else np.ascontiguousarray(inlier_mask, dtype=np.uint8)
    rv, tv = A.as_f64(rvec), A.as_f64(tvec)
    copt = make_options(options, **kw)
    res = A.CResult()
    _check(load().mavba_pose_refine(_d(rv), _d(tv), _d(intr), model, _d(uv), _d(xyz),
                                    A.ptr(mask, C.c_uint8), len(uv), C.byref(copt), C.byref(res)))
    np.asarray(rvec)[...] = rv
    np.asarray(tvec)[...] = tv
    out = res.as_dict()
    return float(np.sqrt(out["final_cost"] / out["num_residuals"])) if out["num_residuals"] else float("nan"), out


def pose_refinement_batch(items, options=None, **kw):
    """Many pose_refinement() problems in one launch (mavba_pose_refine_batch). `items`: list of dicts with rvec, tvec
    (float64 arrays of 3, updated in place), camera_params (model code last), points2D [n,2], points3D [n,3] and an
    optional inlier_mask [n]. Returns the list of (final_cost_px, result) pairs."""
    n = len(items)
    arr = (A.CPoseRefineItem * max(n, 1))()
    hold = []
    for q, it in enumerate(items):
        cp = np.asarray(it["camera_params"], float)
        intr = A.as_f64(np.pad(cp[:-1], (0, 9 - (len(cp) - 1))))
        uv, xyz = A.as_f64(it["points2D"], (-1, 2)), A.as_f64(it["points3D"], (-1, 3))
        mask = None if it.get("inlier_mask") is None else np.ascontiguousarray(it["inlier_mask"], dtype=np.uint8)
        hold.append((intr, uv, xyz, mask))
        for k in range(3):
            arr[q].rvec[k] = float(it["rvec"][k]); arr[q].tvec[k] = float(it["tvec"][k])
        arr[q].intrinsics = _d(intr); arr[q].camera_model = int(cp[-1])
        arr[q].uv = _d(uv); arr[q].xyz = _d(xyz); arr[q].inlier_mask = A.ptr(mask, C.c_uint8); arr[q].n = len(uv)
    res = (A.CResult * max(n, 1))()
    copt = make_options(options, **kw)
    _check(load().mavba_pose_refine_batch(n, arr, C.byref(copt), res))
    out = []
    for q, it in enumerate(items):
        np.asarray(it["rvec"])[...] = list(arr[q].rvec)
        np.asarray(it["tvec"])[...] = list(arr[q].tvec)
        d = res[q].as_dict()
        out.append((float(np.sqrt(d["final_cost"] / d["num_residuals"])) if d["num_residuals"] else float("nan"), d))
    return out


@dataclass
class TriangulationResult:
    """What mavba_triangulate_pairs returns for one image pair (arrays in the caller's order)."""
    xyz: np.ndarray            # [n, 3]; xyz_in for a continued track
    angle: np.ndarray          # [n] radians, unfolded
    reproj_error: np.ndarray   # [n] image 2, normalised coordinates
    depth: np.ndarray          # [n, 2] calc_depth in image 1, image 2
    status: np.ndarray         # [n] int32, TRI_* bits of the failed tests
    accepted: np.ndarray       # [num_accepted] int32, ascending
    mean_folded_angle_deg: float
    kernel_seconds: float

    @property
    def num_accepted(self):
        return len(self.accepted)


def _split_camera_params(camera_params):
    cp = np.asarray(camera_params, float)
    return A.as_f64(np.pad(cp[:-1], (0, 9 - (len(cp) - 1)))), int(cp[-1])


def triangulate_pairs(items, tri_max_reproj_error=4.0, tri_min_angle=2.0, reject=A.TRI_REJECT_EXTEND, device=-1):
    """Two-view triangulation with the mapper's acceptance tests, many image pairs in one launch
    (mavba_triangulate_pairs; reference src/sfm/sequential_mapper.cc:755-810, initial pair :302-349).

    `items`: list of dicts with rvec1, tvec1, rvec2, tvec2, camera_params1, camera_params2 (model code last, like
    FeatureManager.camera_params), points2D1 / points2D2 [n, 2] in pixels and optionally points3D [n, 3] + has_point3D [n]
    (the continued tracks). An item may override tri_max_reproj_error, tri_min_angle and reject. The defaults are the
    reference's SequentialMapperOptions (4 px, 2 degrees) and its map-extension tests; its initial pair is
    reject=TRI_REJECT_INITIAL plus mean_folded_angle_deg. Returns one TriangulationResult per item."""
    count = len(items)
    if count == 0:
        return []
    arr = (A.CTriPair * count)()
    hold, outs = [], []
    for q, it in enumerate(items):
        intr1, model1 = _split_camera_params(it["camera_params1"])
        intr2, model2 = _split_camera_params(it["camera_params2"])
        uv1, uv2 = A.as_f64(it["points2D1"], (-1, 2)), A.as_f64(it["points2D2"], (-1, 2))
        n = len(uv1)
        if len(uv2) != n:
            raise ValueError("points2D1 and points2D2 differ in length")
        has = it.get("has_point3D")
        xin = None
        if has is not None:
            has = np.ascontiguousarray(has, dtype=np.uint8).reshape(n)
            xin = A.as_f64(it["points3D"], (n, 3))
        hold.append((intr1, intr2, uv1, uv2, has, xin))
        c = arr[q]
        for k in range(3):
            c.rvec1[k] = float(it["rvec1"][k]); c.tvec1[k] = float(it["tvec1"][k])
            c.rvec2[k] = float(it["rvec2"][k]); c.tvec2[k] = float(it["tvec2"][k])
        c.intrinsics1 = _d(intr1); c.intrinsics2 = _d(intr2); c.camera_model1 = model1; c.camera_model2 = model2
        c.uv1 = _d(uv1); c.uv2 = _d(uv2); c.n = n
        c.xyz_in = _d(xin); c.has_xyz = A.ptr(has, C.c_uint8)
        c.max_reproj_error_px = float(it.get("tri_max_reproj_error", tri_max_reproj_error))
        c.min_angle_deg = float(it.get("tri_min_angle", tri_min_angle))
        c.reject_bits = int(it.get("reject", reject))
        o = dict(xyz=np.zeros((n, 3)), angle=np.zeros(n), reproj_error=np.zeros(n), depth=np.zeros((n, 2)),
                 status=np.zeros(n, np.int32), accepted=np.zeros(n, np.int32))
        c.xyz = _d(o["xyz"]); c.angle = _d(o["angle"]); c.reproj_error = _d(o["reproj_error"]); c.depth = _d(o["depth"])
        c.status = A.ptr(o["status"], C.c_int32); c.accepted = A.ptr(o["accepted"], C.c_int32)
        outs.append(o)
    _check(load().mavba_triangulate_pairs(count, arr, int(device)))
    return [TriangulationResult(o["xyz"], o["angle"], o["reproj_error"], o["depth"], o["status"],
                                o["accepted"][:int(arr[q].num_accepted)].copy(), float(arr[q].mean_folded_angle_deg),
                                float(arr[q].kernel_seconds)) for q, o in enumerate(outs)]


def _ransac_item(c, it, n, sample_size, defaults, trial_outputs, trial_arrays):
    """What every batched RANSAC call does per item: fills the common fields of the ctypes item `c` (threshold, trial budget,
    stop, probability, supplied samples or seed) from the item's overrides or `defaults`, and allocates inlier_mask [n] and
    - with trial_outputs - the per-trial arrays, trial_arrays = {field: (shape behind the trial axis, dtype)}; without, they
    are empty and their pointers stay NULL. Returns (the samples, to be kept alive, {field: array})."""
    mt = int(it.get("max_trials", defaults["max_trials"]))
    smp = it.get("samples")
    if smp is not None:
        smp = np.ascontiguousarray(smp, dtype=np.int32).reshape(max(mt, 0), sample_size)
    c.max_reproj_error_px = float(it.get("max_reproj_error", defaults["max_reproj_error"]))
    c.max_trials = mt
    c.stop_num_inliers = int(it.get("stop_num_inliers", defaults["stop_num_inliers"]))
    c.probability = float(it.get("probability", defaults["probability"]))
    c.samples = A.ptr(smp, C.c_int32); c.seed = int(it.get("seed", defaults["seed"])) & 0xFFFFFFFFFFFFFFFF
    k = max(mt, 0) if trial_outputs else 0
    o = dict(inlier_mask=np.zeros(n, np.uint8))
    c.inlier_mask = A.ptr(o["inlier_mask"], C.c_uint8)
    for name, (shape, dtype) in trial_arrays.items():
        o[name] = np.zeros((k,) + shape, dtype)
        if trial_outputs:
            setattr(c, name, A.ptr(o[name], C.c_int32) if dtype is np.int32 else _d(o[name]))
    return smp, o


@dataclass
class AbsolutePoseResult:
    """What mavba_absolute_pose_ransac returns for one image."""
    status: int                     # ABSPOSE_OK / ABSPOSE_NO_CONSENSUS
    rvec: np.ndarray                # [3] (NaN without consensus)
    tvec: np.ndarray                # [3]
    proj_matrix: np.ndarray         # [3, 4] = trial_models[best_trial]
    num_inliers: int
    best_trial: int
    trials_used: int
    inlier_mask: np.ndarray         # [n] uint8, the layout pose_refinement_batch takes
    trial_models: np.ndarray        # [max_trials, 3, 4]; NaN for an invalid trial
    trial_num_inliers: np.ndarray   # [max_trials] int32
    trial_residual_sum: np.ndarray  # [max_trials]
    trial_samples: np.ndarray       # [max_trials, 4] int32, ascending
    kernel_seconds: float

    @property
    def ok(self):
        return self.status == A.ABSPOSE_OK


def absolute_pose_ransac(items, max_reproj_error=4.0, max_trials=500, stop_num_inliers=0, probability=0.99, seed=0, device=-1,
                         trial_outputs=True):
    """Absolute pose from 2D-3D matches, P3P inside RANSAC, many images in one launch (mavba_absolute_pose_ransac;
    reference src/sfm/sequential_mapper.cc:621-659). The result of an item is that of the reference's RANSAC() run on
    one thread with the same samples.

    `items`: list of dicts with camera_params (model code last, like FeatureManager.camera_params), points2D [n, 2] in
    pixels and points3D [n, 3]. An item may override max_reproj_error, max_trials, stop_num_inliers (absolute, <= 0:
    none), probability and seed, and may supply samples [max_trials, 4]; otherwise the library draws them from `seed`.
    trial_outputs=False leaves the per-trial arrays out (they come back empty). Returns one AbsolutePoseResult per item."""
    count = len(items)
    if count == 0:
        return []
    arr = (A.CAbsPoseItem * count)()
    hold, outs = [], []
    defaults = dict(max_reproj_error=max_reproj_error, max_trials=max_trials, stop_num_inliers=stop_num_inliers, probability=probability, seed=seed)
    for q, it in enumerate(items):
        intr, model = _split_camera_params(it["camera_params"])
        uv, xyz = A.as_f64(it["points2D"], (-1, 2)), A.as_f64(it["points3D"], (-1, 3))
        n = len(uv)
        if len(xyz) != n:
            raise ValueError("points2D and points3D differ in length")
        c = arr[q]
        c.intrinsics = _d(intr); c.camera_model = model; c.uv = _d(uv); c.xyz = _d(xyz); c.n = n
        smp, o = _ransac_item(c, it, n, 4, defaults, trial_outputs, dict(
            trial_models=((3, 4), float), trial_num_inliers=((), np.int32), trial_residual_sum=((), float), trial_samples=((4,), np.int32)))
        hold.append((intr, uv, xyz, smp))
        outs.append(o)
    _check(load().mavba_absolute_pose_ransac(count, arr, int(device)))
    return [AbsolutePoseResult(int(arr[q].status), np.array(arr[q].rvec), np.array(arr[q].tvec), np.array(arr[q].proj_matrix).reshape(3, 4),
                               int(arr[q].num_inliers), int(arr[q].best_trial), int(arr[q].trials_used), o["inlier_mask"], o["trial_models"],
                               o["trial_num_inliers"], o["trial_residual_sum"], o["trial_samples"], float(arr[q].kernel_seconds))
            for q, o in enumerate(outs)]


def to_pose_refine_items(items, results):
    """The argument of pose_refinement_batch for the images whose RANSAC found a consensus: the chain of
    sequential_mapper.cc:621-732 is absolute_pose_ransac -> to_pose_refine_items -> pose_refinement_batch. Every dict also
    carries `index`, the position of its image in `items` (images without consensus are left out)."""
    out = []
    for q, (it, r) in enumerate(zip(items, results)):
        if r.status != A.ABSPOSE_OK:
            continue
        out.append(dict(index=q, rvec=np.array(r.rvec, float), tvec=np.array(r.tvec, float), camera_params=it["camera_params"],
                        points2D=it["points2D"], points3D=it["points3D"], inlier_mask=np.ascontiguousarray(r.inlier_mask, np.uint8)))
    return out


@dataclass
class RelativePoseResult:
    """What mavba_relative_pose_ransac returns for one image pair."""
    status: int                     # RELPOSE_OK / RELPOSE_NO_CONSENSUS
    E: np.ndarray                   # [3, 3] = trial_models[best_trial, best_model] (NaN without consensus); x2^T E x1 = 0
    R: np.ndarray                   # [3, 3]
    tvec: np.ndarray                # [3]
    rvec: np.ndarray                # [3]
    cheirality_counts: np.ndarray   # [4] int32: (R1, t), (R2, t), (R1, -t), (R2, -t)
    cheirality_best: int
    forward_z: float                # inv_second_proj_matrix(2, 3)
    num_inliers: int
    best_trial: int
    best_model: int
    trials_used: int
    inlier_mask: np.ndarray         # [n] uint8
    trial_num_models: np.ndarray    # [max_trials] int32
    trial_models: np.ndarray        # [max_trials, 10, 3, 3]; NaN beyond a trial's count
    trial_z: np.ndarray             # [max_trials, 10] ascending
    trial_num_inliers: np.ndarray   # [max_trials, 10] int32
    trial_residual_sum: np.ndarray  # [max_trials, 10]
    trial_samples: np.ndarray       # [max_trials, 5] int32, ascending
    kernel_seconds: float

    @property
    def ok(self):
        return self.status == A.RELPOSE_OK


def relative_pose_ransac(items, max_reproj_error=4.0, max_trials=1000, stop_num_inliers=0, probability=0.99, seed=0, device=-1,
                         trial_outputs=True):
    """Relative pose of image pairs from 2D-2D matches: the five-point solver inside RANSAC, then (R, t) by the
    cheirality test, many pairs in one launch (mavba_relative_pose_ransac; reference src/sfm/sequential_mapper.cc:174-216,
    :269-299). The result of an item is the reference's RANSAC() on one thread with the same samples and each trial's
    models taken in ascending z.

    `items`: list of dicts with camera_params1 / camera_params2 (model code last, like FeatureManager.camera_params) and
    points2D1 / points2D2 [n, 2] in pixels. An item may override max_reproj_error, max_trials, stop_num_inliers (absolute,
    <= 0: none), probability and seed, and may supply samples [max_trials, 5]; otherwise the library draws them from
    `seed`. trial_outputs=False leaves the per-trial arrays out (they come back empty). Returns one RelativePoseResult
    per item."""
    count = len(items)
    if count == 0:
        return []
    arr = (A.CRelPoseItem * count)()
    hold, outs = [], []
    defaults = dict(max_reproj_error=max_reproj_error, max_trials=max_trials, stop_num_inliers=stop_num_inliers, probability=probability, seed=seed)
    for q, it in enumerate(items):
        intr1, model1 = _split_camera_params(it["camera_params1"])
        intr2, model2 = _split_camera_params(it["camera_params2"])
        uv1, uv2 = A.as_f64(it["points2D1"], (-1, 2)), A.as_f64(it["points2D2"], (-1, 2))
        n = len(uv1)
        if len(uv2) != n:
            raise ValueError("points2D1 and points2D2 differ in length")
        c = arr[q]
        c.intrinsics1 = _d(intr1); c.intrinsics2 = _d(intr2); c.camera_model1 = model1; c.camera_model2 = model2
        c.uv1 = _d(uv1); c.uv2 = _d(uv2); c.n = n
        smp, o = _ransac_item(c, it, n, 5, defaults, trial_outputs, dict(
            trial_num_models=((), np.int32), trial_models=((10, 3, 3), float), trial_z=((10,), float), trial_num_inliers=((10,), np.int32),
            trial_residual_sum=((10,), float), trial_samples=((5,), np.int32)))
        hold.append((intr1, intr2, uv1, uv2, smp))
        outs.append(o)
    _check(load().mavba_relative_pose_ransac(count, arr, int(device)))
    return [RelativePoseResult(int(arr[q].status), np.array(arr[q].E).reshape(3, 3), np.array(arr[q].R).reshape(3, 3), np.array(arr[q].tvec),
                               np.array(arr[q].rvec), np.array(arr[q].cheirality_counts, np.int32), int(arr[q].cheirality_best),
                               float(arr[q].forward_z), int(arr[q].num_inliers), int(arr[q].best_trial), int(arr[q].best_model),
                               int(arr[q].trials_used), o["inlier_mask"], o["trial_num_models"], o["trial_models"], o["trial_z"],
                               o["trial_num_inliers"], o["trial_residual_sum"], o["trial_samples"], float(arr[q].kernel_seconds))
            for q, o in enumerate(outs)]


def to_triangulate_pairs(items, results, tri_max_reproj_error=4.0, tri_min_angle=2.0):
    """The argument of triangulate_pairs for the pairs whose RANSAC found a consensus and a pose: the chain of
    sequential_mapper.cc:174-349 is relative_pose_ransac -> to_triangulate_pairs -> triangulate_pairs. The first image
    has rvec = tvec = 0, the second the recovered pose; the correspondences are the inliers, in order;
    reject = TRI_REJECT_INITIAL (depth in image 1) and mean_folded_angle_deg of the result is the mapper's angle test.
    Every dict also carries `index`, the position of its pair in `items`, and `inliers`, the positions of its
    correspondences in the pair's matches (pairs without consensus or without a pose are left out)."""
    out = []
    for q, (it, r) in enumerate(zip(items, results)):
        if r.status != A.RELPOSE_OK or r.cheirality_best < 0:
            continue
        inl = np.flatnonzero(np.asarray(r.inlier_mask))
        out.append(dict(index=q, inliers=inl, rvec1=np.zeros(3), tvec1=np.zeros(3), rvec2=np.array(r.rvec, float), tvec2=np.array(r.tvec, float),
                        camera_params1=it["camera_params1"], camera_params2=it["camera_params2"],
                        points2D1=A.as_f64(it["points2D1"], (-1, 2))[inl], points2D2=A.as_f64(it["points2D2"], (-1, 2))[inl],
                        tri_max_reproj_error=tri_max_reproj_error, tri_min_angle=tri_min_angle, reject=A.TRI_REJECT_INITIAL))
    return out


@dataclass
class HomographyResult:
    """What mavba_homography_ransac returns for one image pair."""
    status: int                     # HOMOGRAPHY_OK / HOMOGRAPHY_NO_CONSENSUS
    H: np.ndarray                   # [3, 3] = trial_models[best_trial] (NaN without consensus); H (x, y, 1) ~ (u, v, 1)
    num_inliers: int
    inlier_ratio: float             # num_inliers / n (0 for n == 0)
    best_trial: int
    trials_used: int
    inlier_mask: np.ndarray         # [n] uint8
    trial_models: np.ndarray        # [max_trials, 3, 3]; NaN for an invalid trial
    trial_num_inliers: np.ndarray   # [max_trials] int32
    trial_residual_sum: np.ndarray  # [max_trials]
    trial_samples: np.ndarray       # [max_trials, 4] int32, ascending
    kernel_seconds: float

    @property
    def ok(self):
        return self.status == A.HOMOGRAPHY_OK


def homography_ransac(items, max_reproj_error=4.0, max_trials=100, stop_num_inliers=0, probability=0.99, seed=0, device=-1,
                      trial_outputs=True):
    """The view-change test of image pairs: a four-point homography inside RANSAC, many pairs in one launch
    (mavba_homography_ransac; reference src/sfm/sequential_mapper.cc:116-158 and :465-503). The result of an item is that
    of the reference's RANSAC() run on one thread with the same samples.

    `items`: list of dicts with points2D1 / points2D2 [n, 2] in pixels, as in relative_pose_ransac; they are used as they
    are (no camera model, camera_params* are ignored) and max_reproj_error is the threshold in pixels. An item may
    override max_reproj_error, max_trials, stop_num_inliers (absolute, <= 0: none; see view_change_stop), probability and
    seed, and may supply samples [max_trials, 4]; otherwise the library draws them from `seed`. trial_outputs=False leaves
    the per-trial arrays out (they come back empty). Returns one HomographyResult per item."""
    count = len(items)
    if count == 0:
        return []
    arr = (A.CHomographyItem * count)()
    hold, outs = [], []
    defaults = dict(max_reproj_error=max_reproj_error, max_trials=max_trials, stop_num_inliers=stop_num_inliers, probability=probability, seed=seed)
    for q, it in enumerate(items):
        uv1, uv2 = A.as_f64(it["points2D1"], (-1, 2)), A.as_f64(it["points2D2"], (-1, 2))
        n = len(uv1)
        if len(uv2) != n:
            raise ValueError("points2D1 and points2D2 differ in length")
        c = arr[q]
        c.uv1 = _d(uv1); c.uv2 = _d(uv2); c.n = n
        smp, o = _ransac_item(c, it, n, 4, defaults, trial_outputs, dict(
            trial_models=((3, 3), float), trial_num_inliers=((), np.int32), trial_residual_sum=((), float), trial_samples=((4,), np.int32)))
        hold.append((uv1, uv2, smp))
        outs.append(o)
    _check(load().mavba_homography_ransac(count, arr, int(device)))
    return [HomographyResult(int(arr[q].status), np.array(arr[q].H).reshape(3, 3), int(arr[q].num_inliers), float(arr[q].inlier_ratio),
                             int(arr[q].best_trial), int(arr[q].trials_used), o["inlier_mask"], o["trial_models"],
                             o["trial_num_inliers"], o["trial_residual_sum"], o["trial_samples"], float(arr[q].kernel_seconds))
            for q, o in enumerate(outs)]


def view_change_stop(n, max_homography_inliers):
    """stop_num_inliers of the mapper's view-change test for a pair of n matches: int(n * max_homography_inliers), the
    size_t of sequential_mapper.cc:131-132. A 0 is passed as 1: the library reads 0 as "no stop", where the reference
    would stop at once, after its first trial - as the library does at 1 as soon as a trial has an inlier."""
    return max(int(n * max_homography_inliers), 1)


def view_change_pairs(items, results, max_homography_inliers=0.7):
    """The positions in `items` of the pairs the mapper would keep after homography_ransac: a pair is kept when
    num_inliers / n <= max_homography_inliers, the test of sequential_mapper.cc:153-156 (it discards a pair that one
    homography explains: too little parallax, a planar scene or a pure rotation). A pair without consensus - fewer than
    five matches, or no trial with four inliers - is kept as well: no homography explains it. (The reference does not
    get that far: its RANSAC() throws there.) The positions select the items to hand to relative_pose_ransac."""
    return [q for q, r in enumerate(results) if r.status != A.HOMOGRAPHY_OK or r.inlier_ratio <= max_homography_inliers]


@dataclass
class MatchResult:
    """What mavba_match_descriptors returns for one image pair."""
    matches: np.ndarray           # [num_matches, 2] int32: (index in image 1, index in image 2), ascending in the first
    distances: np.ndarray         # [num_matches] float32: the descriptor distance of every match
    nn12: np.ndarray              # [n1, 2] int32: the two nearest candidates in image 2 (-1: absent)
    dist12: np.ndarray            # [n1, 2] float32 (NaN: absent)
    nn21: np.ndarray              # [n2, 2] int32
    dist21: np.ndarray            # [n2, 2] float32
    median_disparity: float       # NaN without matches or without keypoints
    kernel_seconds: float

    @property
    def num_matches(self):
        return len(self.matches)


def match_descriptors(items, max_ratio=0.9, max_distance=-1.0, device=-1):
    """The 2D-2D matches of image pairs by brute force - two nearest neighbours in both directions, Lowe's ratio test
    on both sides, the mutual-nearest check - many pairs in two launches (mavba_match_descriptors; reference
    src/base2d/feature.cc:52-102 as src/sfm/sequential_mapper.cc:2079-2083 calls it). include/mavba_match.h states the
    rules the result follows.

    `items`: list of dicts with descriptors1 [n1, dim] / descriptors2 [n2, dim] (float32; dim a multiple of 4, at most
    128) and keypoints1 [n1, 2] / keypoints2 [n2, 2] in pixels. The keypoints may be left out when max_distance < 0 (no
    spatial mask); the median disparity is then NaN. An item may override max_ratio and max_distance. Returns one
    MatchResult per item."""
    count = len(items)
    if count == 0:
        return []
    arr = (A.CMatchItem * count)()
    hold, outs = [], []
    f, i32 = C.c_float, C.c_int32
    for q, it in enumerate(items):
        d1, d2 = A.as_f32(it["descriptors1"]), A.as_f32(it["descriptors2"])
        if d1.ndim != 2 or d2.ndim != 2 or d1.shape[1] != d2.shape[1]:
            raise ValueError("descriptors1 and descriptors2 must be [n, dim] with the same dim")
        n1, n2, dim = len(d1), len(d2), d1.shape[1]
        xy1 = None if it.get("keypoints1") is None else A.as_f32(it["keypoints1"], (-1, 2))
        xy2 = None if it.get("keypoints2") is None else A.as_f32(it["keypoints2"], (-1, 2))
        if (xy1 is not None and len(xy1) != n1) or (xy2 is not None and len(xy2) != n2):
            raise ValueError("keypoints and descriptors differ in length")
        m = min(n1, n2)
        o = dict(matches=np.zeros((m, 2), np.int32), distances=np.zeros(m, np.float32),
                 nn12=np.zeros((n1, 2), np.int32), dist12=np.zeros((n1, 2), np.float32),
                 nn21=np.zeros((n2, 2), np.int32), dist21=np.zeros((n2, 2), np.float32))
        c = arr[q]
        c.desc1, c.desc2, c.xy1, c.xy2 = A.ptr(d1, f), A.ptr(d2, f), A.ptr(xy1, f), A.ptr(xy2, f)
        c.n1, c.n2, c.dim = n1, n2, dim
        c.max_ratio, c.max_distance = float(it.get("max_ratio", max_ratio)), float(it.get("max_distance", max_distance))
        c.matches, c.distances = A.ptr(o["matches"], i32), A.ptr(o["distances"], f)
        c.nn12, c.dist12, c.nn21, c.dist21 = A.ptr(o["nn12"], i32), A.ptr(o["dist12"], f), A.ptr(o["nn21"], i32), A.ptr(o["dist21"], f)
        hold.append((d1, d2, xy1, xy2))
        outs.append(o)
    _check(load().mavba_match_descriptors(count, arr, int(device)))
    return [MatchResult(o["matches"][:arr[q].num_matches], o["distances"][:arr[q].num_matches], o["nn12"], o["dist12"], o["nn21"], o["dist21"],
                        float(arr[q].median_disparity), float(arr[q].kernel_seconds)) for q, o in enumerate(outs)]


def to_homography_items(items, results):
    """The items of homography_ransac (and, with camera_params*, of relative_pose_ransac) for the pairs of
    match_descriptors: points2D1 / points2D2 are the keypoints of every match, in the order of the matches. Every other
    key of an item (camera_params1, ...) is passed on."""
    out = []
    for it, r in zip(items, results):
        xy1, xy2 = A.as_f64(it["keypoints1"], (-1, 2)), A.as_f64(it["keypoints2"], (-1, 2))
        keep = {k: v for k, v in it.items() if k not in ("descriptors1", "descriptors2", "keypoints1", "keypoints2", "max_ratio", "max_distance")}
        out.append(dict(keep, points2D1=xy1[r.matches[:, 0]], points2D2=xy2[r.matches[:, 1]]))
    return out


class Scene:
    """Incremental flat mirror of a FeatureManager (mavba_scene_*): deltas in, bundle_adjustment() calls out.
    Ids are the caller's (the FeatureManager's 1-based ids are fine)."""

    def __init__(self):
        self._h = C.c_void_p()
        _check(load().mavba_scene_create(C.byref(self._h)))

    def close(self):
        if self._h:
            load().mavba_scene_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def set_camera(self, camera_id, model, params):
        _check(load().mavba_scene_set_camera(self._h, int(camera_id), int(model), _d(A.as_f64(np.pad(np.asarray(params, float), (0, 9))[:9]))))

    def set_image(self, image_id, camera_id=-1, rvec=None, tvec=None):
        r = None if rvec is None else A.as_f64(rvec)
        t = None if tvec is None else A.as_f64(tvec)
        _check(load().mavba_scene_set_image(self._h, int(image_id), int(camera_id), None if r is None else _d(r), None if t is None else _d(t)))

    def add_point2D(self, image_id, point2D_id, xy):
        _check(load().mavba_scene_add_point2d(self._h, int(image_id), int(point2D_id), _d(A.as_f64(xy))))

    def add_points2D(self, image_id, point2D_ids, xy, point3D_ids=None):
        """Many 2-D points of one image in one call (`point3D_ids`: their links, < 0 = none)."""
        ids = np.ascontiguousarray(point2D_ids, dtype=np.int64)
        uv = A.as_f64(xy, (-1, 2))
        assert len(uv) == len(ids)
        l3 = None if point3D_ids is None else np.ascontiguousarray(point3D_ids, dtype=np.int64)
        _check(load().mavba_scene_add_points2d(self._h, int(image_id), len(ids), A.ptr(ids, C.c_int64), _d(uv),
                                               None if l3 is None else A.ptr(l3, C.c_int64)))

    def set_point3D(self, point3D_id, xyz):
        _check(load().mavba_scene_set_point3d(self._h, int(point3D_id), _d(A.as_f64(xyz))))

    def link(self, point2D_id, point3D_id):
        _check(load().mavba_scene_link(self._h, int(point2D_id), int(point3D_id)))

    def delete_point3D(self, point3D_id):
        _check(load().mavba_scene_delete_point3d(self._h, int(point3D_id)))

    def get_image(self, image_id):
        r, t = np.zeros(3), np.zeros(3)
        _check(load().mavba_scene_get_image(self._h, int(image_id), _d(r), _d(t)))
        return r, t

    def get_point3D(self, point3D_id):
        x = np.zeros(3)
        _check(load().mavba_scene_get_point3d(self._h, int(point3D_id), _d(x)))
        return x

    def get_camera(self, camera_id):
        m, p = C.c_int32(), np.zeros(9)
        _check(load().mavba_scene_get_camera(self._h, int(camera_id), C.byref(m), _d(p)))
        return m.value, p[:A.MODEL_NUM_PARAMS[m.value]]

    @staticmethod
    def _lists(free, fixed, fixed_x, gcp, rot):
        arrs = [np.ascontiguousarray(x, dtype=np.int64) for x in (free, fixed, fixed_x, gcp)]
        rot = rot or {}
        ri = np.ascontiguousarray(list(rot.keys()), dtype=np.int64)
        rv = A.as_f64(np.array([rot[k] for k in rot], float).reshape(-1, 3))
        args = []
        for a in arrs:
            args += [A.ptr(a, C.c_int64), len(a)]
        args += [A.ptr(ri, C.c_int64), _d(rv), len(ri)]
        return args, (arrs, ri, rv)

    @staticmethod
    def _scene_options(min_track_len=2, refine_camera_params=False, constrain_rotation=False, constrain_rotation_weight=0.0):
        return A.CSceneOptions(int(min_track_len), int(bool(refine_camera_params)), int(bool(constrain_rotation)), float(constrain_rotation_weight))

    def flatten(self, free, fixed, fixed_x, gcp=(), rot=None, **scene_opts):
        """The flat problem of a call as a dict of numpy COPIES (+ the flat-index -> id tables)."""
        args, hold = self._lists(free, fixed, fixed_x, gcp, rot)
        so = self._scene_options(**scene_opts)
        P = A.CProblem()
        i64p = C.POINTER(C.c_int64)
        ii, ci, pi = i64p(), i64p(), i64p()
        _check(load().mavba_scene_flatten(self._h, *args, C.byref(so), C.byref(P), C.byref(ii), C.byref(ci), C.byref(pi)))
        g = lambda ptr, n, dt: np.ctypeslib.as_array(ptr, shape=(n,)).astype(dt).copy() if n else np.zeros(0, dt)  # noqa: E731
        ni, nc, npt, no, nr = P.num_images, P.num_cameras, P.num_points, P.num_obs, P.num_rot_priors
        return dict(image_ids=g(ii, ni, np.int64), camera_ids=g(ci, nc, np.int64), point_ids=g(pi, npt, np.int64),
                    poses=g(P.poses, ni * 6, float).reshape(-1, 6), pose_const=g(P.pose_const, ni, np.uint8),
                    image_camera=g(P.image_camera, ni, np.int32), intrinsics=g(P.intrinsics, nc * 9, float).reshape(-1, 9),
                    camera_model=g(P.camera_model, nc, np.int32), intr_const=g(P.intr_const, nc, np.uint8),
                    points=g(P.points, npt * 3, float).reshape(-1, 3), point_const=g(P.point_const, npt, np.uint8),
                    obs_uv=g(P.obs_uv, no * 2, float).reshape(-1, 2), obs_image=g(P.obs_image, no, np.int32),
                    obs_point=g(P.obs_point, no, np.int32), rot_prior_image=g(P.rot_prior_image, nr, np.int32),
                    rot_prior_rvec=g(P.rot_prior_rvec, nr * 3, float).reshape(-1, 3), rot_prior_weight=P.rot_prior_weight)

    def bundle_adjustment(self, free, fixed, fixed_x, options=None, gcp=(), rot=None, point3D_errors=None, **scene_opts):
        """bundle_adjustment() on the scene (results are written back into it). Returns (final_cost_px, result);
        `point3D_errors`: optional dict updated like the reference's map when options.update_point_errors is set."""
        args, hold = self._lists(free, fixed, fixed_x, gcp, rot)
        so = self._scene_options(**scene_opts)
        copt = make_options(options)
        if point3D_errors is not None:
            copt.update_point_errors = 1
        res = A.CResult()
        cost = C.c_double()
        i64p = C.POINTER(C.c_int64)
        eids, evals, n = i64p(), C.POINTER(C.c_double)(), C.c_int64()
        _check(load().mavba_scene_bundle_adjust(self._h, *args, C.byref(so), C.byref(copt), C.byref(res), C.byref(cost),
                                                C.byref(eids), C.byref(evals), C.byref(n)))
        if point3D_errors is not None and n.value:
            ids = np.ctypeslib.as_array(eids, shape=(n.value,))
            vals = np.ctypeslib.as_array(evals, shape=(n.value,))
            point3D_errors.update(zip(ids.tolist(), vals.tolist()))
        return cost.value, res.as_dict()


class Session:
    """Device-resident solver state (mavba_session_*)."""

    def __init__(self, problem: BAProblem, options=None, **kw):
        self.problem = problem
        self.copt = make_options(options, **kw)
        self._cp = problem.c_struct()
        self._h = C.c_void_p()
        self._cb = None
        _check(load().mavba_session_create(C.byref(self._cp), C.byref(self.copt), C.byref(self._h)))

    def close(self):
        if self._h:
            load().mavba_session_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def reset(self):
        _check(load().mavba_session_reset(self._h))

    def iterate(self, max_iters=1):
        done, term = C.c_int32(), C.c_int32()
        _check(load().mavba_session_iterate(self._h, int(max_iters), C.byref(done), C.byref(term)))
        return done.value, term.value

    def solve(self):
        self.iterate(self.copt.max_num_iterations + 1)
        return self.result()

    def result(self):
        r = A.CResult()
        _check(load().mavba_session_result(self._h, C.byref(r)))
        return r.as_dict()

    def get_params(self):
        p = self.problem
        poses, intr, pts = np.zeros((p.num_images, 6)), np.zeros((p.num_cameras, 9)), np.zeros((p.num_points, 3))
        _check(load().mavba_session_get_params(self._h, _d(poses), _d(intr), _d(pts)))
        return poses, intr, pts

    def point_errors(self):
        e = np.full(self.problem.num_points, np.nan)
        _check(load().mavba_session_point_errors(self._h, _d(e)))
        return e

    def set_params(self, poses=None, intrinsics=None, points=None):
        p = self.problem
        arrs = [None if a is None else A.as_f64(a, shape) for a, shape in
                ((poses, (p.num_images, 6)), (intrinsics, (p.num_cameras, 9)), (points, (p.num_points, 3)))]
        _check(load().mavba_session_set_params(self._h, *[None if a is None else _d(a) for a in arrs]))

    def restart(self):
        _check(load().mavba_session_restart(self._h))

    def filter_points(self, max_error, keep=None):
        """filter_point_cloud on the resident session: returns (removed mask, errors the decision used)."""
        n = self.problem.num_points
        removed, errors = np.zeros(n, np.uint8), np.full(n, np.nan)
        keep_arr = None if keep is None else np.ascontiguousarray(keep, dtype=np.uint8)
        cnt = C.c_int64()
        _check(load().mavba_session_filter_points(self._h, float(max_error), A.ptr(keep_arr, C.c_uint8),
                                                  A.ptr(removed, C.c_uint8), _d(errors), C.byref(cnt)))
        return removed, errors

    def set_allreduce(self, fn, rank, world_size):
        """fn(device_ptr:int, count:int, op:int) -> None; must all-reduce in place and return when done."""
        def trampoline(_ctx, ptr, count, op):
            try:
                fn(ptr, count, op)
                return 0
            except Exception as e:  # noqa: BLE001 - must not unwind through C
                print("all-reduce hook raised:", repr(e), flush=True)
                return 1
        self._cb = ALLREDUCE_FN(trampoline)
        _check(load().mavba_session_set_allreduce(self._h, self._cb, None, rank, world_size))

    def set_rccl(self, unique_id, rank, world_size):
        """Native RCCL exchange (mavba_session_set_rccl); `unique_id` = the 128 bytes of rccl_unique_id() from rank 0."""
        buf = C.create_string_buffer(bytes(unique_id), 128)
        _check(load().mavba_session_set_rccl(self._h, buf, rank, world_size))

    def eval_jacobian(self):
        n = self.problem.num_obs
        r, Jc, Jp, Jk = np.zeros((n, 2)), np.zeros((n, 2, 6)), np.zeros((n, 2, 3)), np.zeros((n, 2, 9))
        cost = C.c_double()
        _check(load().mavba_session_eval_jacobian(self._h, C.byref(cost), _d(r), _d(Jc), _d(Jp), _d(Jk)))
        return cost.value, r, Jc, Jp, Jk

    def reduced_system(self, radius):
        n = load().mavba_session_reduced_dim(self._h)
        S, v = np.zeros((n, n)), np.zeros(n)
        _check(load().mavba_session_reduced_system(self._h, float(radius), _d(S), _d(v)))
        return S, v

    def linear_step(self, radius):
        p = self.problem
        dp, di, dx = np.zeros((p.num_images, 6)), np.zeros((p.num_cameras, 9)), np.zeros((p.num_points, 3))
        mcc = C.c_double()
        _check(load().mavba_session_linear_step(self._h, float(radius), _d(dp), _d(di), _d(dx), C.byref(mcc)))
        return dict(d_poses=dp, d_intr=di, d_points=dx, model_cost_change=mcc.value)

    def set_profiling(self, on):
        """Event brackets around the kernels on / off for the iterations that follow."""
        _check(load().mavba_session_set_profiling(self._h, 1 if on else 0))

    def time_front(self, radius=1e4, reps=20):
        """Average milliseconds of one pass of the linear solve's front end (probe)."""
        ms = C.c_float(0)
        _check(load().mavba_session_time_front(self._h, float(radius), int(reps), C.byref(ms)))
        return ms.value

    def time_jacobian(self, reps=20):
        ms = C.c_float()
        _check(load().mavba_session_time_jacobian(self._h, int(reps), C.byref(ms)))
        return float(ms.value)

    def info(self):
        i = A.CSessionInfo()
        _check(load().mavba_session_get_info(self._h, C.byref(i)))
        d = {k: getattr(i, k) for k, _ in i._fields_ if k != "schur_terms"}
        d["schur_terms"] = list(i.schur_terms)
        return d

    def kernel_stats(self):
        buf = (A.CKernelStat * 64)()
        n = load().mavba_session_kernel_stats(self._h, buf, 64)
        return {buf[i].name.decode(): dict(launches=int(buf[i].launches), total_ms=float(buf[i].total_ms))
                for i in range(min(n, 64))}


def elimination_tree(num_images, num_cameras, pairs, max_depth=3):
    """The elimination tree of the reduced camera system for an image graph (`pairs`: [n, 2] coupled images); no GPU
    needed. Returns (node_of_image [num_images], node_parent [num_nodes]); no nodes = no dissection."""
    pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    a, b = np.ascontiguousarray(pairs[:, 0]), np.ascontiguousarray(pairs[:, 1])
    node = np.zeros(max(num_images, 1), np.int32)
    parent = np.zeros(4096, np.int32)
    n = load().mavba_debug_elimination_tree(int(num_images), int(num_cameras), len(a), A.ptr(a, C.c_int32), A.ptr(b, C.c_int32),
                                           int(max_depth), A.ptr(node, C.c_int32), A.ptr(parent, C.c_int32), len(parent))
    if n < 0:
        _check(n)
    return node[:num_images], parent[:n]


def backsub_tiles(pt_start):
    """The wave tiles of the point back-substitution for points with observations [pt_start[q], pt_start[q + 1]); no GPU
    needed. Returns an [n, 4] array: first point, points, first observation, observations of every tile."""
    pt_start = np.ascontiguousarray(pt_start, dtype=np.int32)
    num_points = max(len(pt_start) - 1, 0)
    out = np.zeros((max(num_points, 1), 4), np.int32)
    n = load().mavba_debug_backsub_tiles(num_points, A.ptr(pt_start, C.c_int32), A.ptr(out, C.c_int32), num_points)
    if n < 0:
        _check(n)
    return out[:n].copy()


def radix_sort_order(keys, key_bytes=4, device=-1):
    """Stable ascending order of range(len(keys)) by uint32 keys, computed by the set-up's device radix sort."""
    keys = np.ascontiguousarray(keys, dtype=np.uint32)
    out = np.zeros(len(keys), np.int32)
    _check(load().mavba_debug_radix_sort(len(keys), A.ptr(keys, C.c_uint32), int(key_bytes), A.ptr(out, C.c_int32), device))
    return out


def debug_upload_batch(sizes, arena_bytes=0, device=-1):
    """Wrong bytes after a batch of small uploads / clears of the given sizes (negative: a clear) - 0 = pass."""
    sizes = np.ascontiguousarray(sizes, dtype=np.int64)
    f = load().mavba_debug_upload_batch
    f.restype = C.c_int64   # (wrong bytes, not a status)
    r = f(C.c_int32(len(sizes)), A.ptr(sizes, C.c_int64), C.c_int64(int(arena_bytes)), C.c_int32(device))
    if r < 0:
        raise MavbaError(A.ERR_HIP, load().mavba_last_error().decode(errors="replace"))
    return int(r)


def debug_lm_decide(cases, device=-1):
    """The LM decision function (csrc/lm_decide.h) on rows of 16 scalars + 8 parameters: (host results, device results), 6 columns each."""
    cases = np.ascontiguousarray(cases, dtype=np.float64)
    n = cases.shape[0]
    assert cases.shape[1] == 24
    oh, od = np.zeros((n, 6)), np.zeros((n, 6))
    _check(load().mavba_debug_lm_decide(n, _d(cases), _d(oh), _d(od), device))
    return oh, od


def debug_obs_math(kind, cases, device=-1):
    """One per-observation function of csrc/ba_math.h (kind: _abi.OBS_MATH_*) on the rows of `cases`: (host build's results,
    device build's results), _abi.OBS_MATH_WIDTHS[kind][1] columns each."""
    wi, wo = A.OBS_MATH_WIDTHS[kind]
    cases = np.ascontiguousarray(cases, dtype=np.float64).reshape(-1, wi)
    n = cases.shape[0]
    oh, od = np.zeros((n, wo)), np.zeros((n, wo))
    _check(load().mavba_debug_obs_math(kind, n, _d(cases), _d(oh), _d(od), device))
    return oh, od


def debug_chol_schedule(nb, nodes, pairs, cus=256):
    """Tile structure + persistent schedule of a factorisation on the HOST (no device): `nodes` = [(begin, end, parent)] of the
    elimination tree in tile columns, `pairs` = non-zero lower tiles (row, col). Returns a dict with the modelled times and
    the helpers' / chains' queues: tasks = [(work-group, kind, i, j, [update columns])], kinds 0 TILE 1 PRE_DIAG 2 PRE_SUB 3 CHAIN."""
    nodes = np.ascontiguousarray(nodes, dtype=np.int32).reshape(-1, 3)
    pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    nbg, ne, npar = (np.ascontiguousarray(nodes[:, k]) for k in range(3))
    pr, pc = np.ascontiguousarray(pairs[:, 0]), np.ascontiguousarray(pairs[:, 1])
    i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    out = np.zeros(8)
    nt, nu = C.c_int64(), C.c_int64()
    ci = np.zeros(nb, np.int32)
    L = load()
    _check(L.mavba_debug_chol_schedule(nb, len(nodes), i32(nbg), i32(ne), i32(npar), len(pairs), i32(pr), i32(pc), cus, _d(out),
                                       None, 0, C.byref(nt), None, 0, C.byref(nu), i32(ci)))
    tasks = np.zeros((max(nt.value, 1), 6), np.int32)
    upd = np.zeros(max(nu.value, 1), np.int32)
    _check(L.mavba_debug_chol_schedule(nb, len(nodes), i32(nbg), i32(ne), i32(npar), len(pairs), i32(pr), i32(pc), cus, _d(out),
                                       i32(tasks), nt.value, C.byref(nt), i32(upd), nu.value, C.byref(nu), i32(ci)))
    tl = [(int(t[0]), int(t[1]), int(t[2]), int(t[3]), [int(x) for x in upd[t[4]:t[5]]]) for t in tasks[:nt.value]]
    return dict(ok=bool(out[0]), model_forward_us=float(out[1]), launch_per_panel_us=float(out[2]), grid=int(out[3]),
                chain_wgs=int(out[4]), tiles=int(out[5]), updates=int(out[6]), nodes=int(out[7]), tasks=tl, chain_info=ci.tolist())


def rccl_unique_id():
    """128-byte ncclUniqueId for Session.set_rccl (call on rank 0, distribute to every rank)."""
    buf = C.create_string_buffer(128)
    _check(load().mavba_rccl_unique_id(buf))
    return buf.raw


def dense_spd_solve(Amat, b, device=-1):
    """Solves Amat x = b with the reduced camera system's factorisation. Amat is symmetric positive definite; its LOWER
    triangle is the one that is read. Raises MavbaError if it is not numerically SPD (a NaN in that triangle included)."""
    Amat, b = A.as_f64(Amat), A.as_f64(b)
    x = np.zeros_like(b)
    _check(load().mavba_dense_spd_solve(len(b), _d(Amat), _d(b), _d(x), device))
    return x
