"""Two-view triangulation (mavmap_amd/csrc/tri_math.h) compiled for the HOST by g++ and checked against a numpy
restatement of the reference lines it replaces, plus the C ABI of mavba_triangulate_pairs without a device.

The checker below restates, in numpy and in the reference's order of operations,
  src/base3d/camera_models.h:132-145,195-223,304-338   image2world of the three models
  src/base3d/camera_models.cc:24-52                    division by z, pixel threshold -> normalised threshold
  src/base3d/triangulation.cc:18-48                    DLT (numpy.linalg.svd where the reference has Eigen's JacobiSVD)
  src/base3d/triangulation.cc:101-147                  triangulation angle
  src/base3d/projection.cc:107-149                     reprojection error, calc_depth
  src/sfm/sequential_mapper.cc:755-810, :302-349       the acceptance tests of the map extension and of the initial pair
(the reference's own triangulation.cc needs Eigen and cannot be compiled for these tests). tests/test_gpu_triangulate.py
uses the same checker and the same generator for the kernel.
"""
import ctypes as C
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

from mavmap_amd import _abi as A
from mavmap_amd import synth

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
dp = C.POINTER(C.c_double)
EPS = 2.0 ** -52

# DLT: bound on |h - h_exact| (unit homogeneous vectors, sign fixed) = DLT_K eps sigma1 / (sigma3 - sigma4), the
# perturbation bound of the singular vector of the smallest singular value. DLT_K = 8 x the larger of the two measured
# maxima of that ratio against a 50-digit SVD (see test_dlt_against_a_50_digit_svd, where the figures are recorded).
DLT_K = 8 * 2.999


def d(a):
    return a.ctypes.data_as(dp)


# ---------------------------------------------------------------------------------------------------------------------
# numpy restatement of the reference
# ---------------------------------------------------------------------------------------------------------------------
def ref_distortion(cam, u, v):
    k1, k2, p1, p2 = cam[4:8]
    u2, uy, y2 = u * u, u * v, v * v
    r2 = u2 + y2
    radial = k1 * r2 + k2 * r2 * r2
    return u * radial + 2 * p1 * uy + p2 * (r2 + 2 * u2), v * radial + 2 * p2 * uy + p1 * (r2 + 2 * y2)


def ref_image2world(model, cam, uv):
    """[n, 2] pixels -> [n, 2] normalised coordinates (x / z, y / z)."""
    uv = np.asarray(uv, float).reshape(-1, 2)
    x = (uv[:, 0] - cam[2]) / cam[0]
    y = (uv[:, 1] - cam[3]) / cam[1]
    z = np.ones_like(x)
    if model != A.MODEL_PINHOLE:
        xx, yy = x, y
        for _ in range(10):
            dx, dy = ref_distortion(cam, xx, yy)
            xx, yy = x - dx, y - dy
        x, y = xx, yy
        if model == A.MODEL_CATA:
            xi = cam[8]
            if xi == 1:
                z = (1 - xx * xx - yy * yy) / 2
            else:
                r2 = xx * xx + yy * yy
                z = 1 - xi * (r2 + 1) / (xi + np.sqrt(1 + (1 - xi * xi) * r2))
    return np.stack([x / z, y / z], axis=1)


def ref_threshold(threshold, cam):
    return threshold / ((cam[0] + cam[1]) / 2)


def ref_proj_matrix(rvec, tvec):
    """compose_proj_matrix with the identity calibration: [R(rvec) | t], angle_axis_from_rvec + toRotationMatrix."""
    rvec = np.asarray(rvec, float)
    angle = np.linalg.norm(rvec)
    if angle < np.finfo(float).eps:
        R = np.eye(3)
    else:
        a = rvec / angle
        Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
        R = np.cos(angle) * np.eye(3) + (1 - np.cos(angle)) * np.outer(a, a) + np.sin(angle) * Kx
    return np.concatenate([R, np.asarray(tvec, float).reshape(3, 1)], axis=1)


def ref_dlt_matrices(P1, P2, x1, x2):
    """[n, 6, 4] matrices of triangulate_point."""
    n = len(x1)
    M = np.zeros((n, 6, 4))
    for k in range(4):
        M[:, 0, k] = x1[:, 0] * P1[2, k] - P1[0, k]
        M[:, 1, k] = x1[:, 1] * P1[2, k] - P1[1, k]
        M[:, 2, k] = x1[:, 0] * P1[1, k] - x1[:, 1] * P1[0, k]
        M[:, 3, k] = x2[:, 0] * P2[2, k] - P2[0, k]
        M[:, 4, k] = x2[:, 1] * P2[2, k] - P2[1, k]
        M[:, 5, k] = x2[:, 0] * P2[1, k] - x2[:, 1] * P2[0, k]
    return M


def ref_triangulate(P1, P2, x1, x2):
    """Returns (X [n, 3], h [n, 4] unit homogeneous vectors, sv [n, 4] singular values)."""
    if len(x1) == 0:
        return np.zeros((0, 3)), np.zeros((0, 4)), np.zeros((0, 4))
    M = ref_dlt_matrices(P1, P2, x1, x2)
    _, sv, Vh = np.linalg.svd(M)
    h = Vh[:, 3, :]
    with np.errstate(all="ignore"):
        X = h[:, :3] / h[:, 3:4]
    return X, h, sv


def _dot_rows(P, r, X):
    """Row r of P times (X, 1), summed left to right as written."""
    return P[r, 0] * X[:, 0] + P[r, 1] * X[:, 1] + P[r, 2] * X[:, 2] + P[r, 3]


def ref_centre(P):
    """Camera position: translation column of invert_proj_matrix."""
    M = np.eye(4)
    M[:3] = P
    return np.linalg.inv(M)[:3, 3]


def ref_angles(C1, C2, X):
    """calc_tri_angles with the camera centres given (the library forms them as -R^T t)."""
    b = C1 - C2
    baseline = np.sqrt(b[0] * b[0] + b[1] * b[1] + b[2] * b[2])
    baseline2 = baseline * baseline
    a, c = X - C1, X - C2
    with np.errstate(all="ignore"):
        ray1 = np.sqrt(a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1] + a[:, 2] * a[:, 2])
        ray2 = np.sqrt(c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1] + c[:, 2] * c[:, 2])
        ang = np.arccos((ray1 * ray1 + ray2 * ray2 - baseline2) / (2 * ray1 * ray2))
    return np.where(np.isnan(ang), 0.0, ang)


def ref_fold(angle):
    o = np.pi - angle
    return np.where(o < angle, o, angle)


def ref_reproj_errors(P, X, x):
    with np.errstate(all="ignore"):
        p2 = _dot_rows(P, 2, X)
        p0 = _dot_rows(P, 0, X) / p2
        p1 = _dot_rows(P, 1, X) / p2
        dx, dy = p0 - x[:, 0], p1 - x[:, 1]
        return np.sqrt(dx * dx + dy * dy)


def ref_depth(P, X):
    with np.errstate(all="ignore"):
        return _dot_rows(P, 2, X) * np.sqrt(P[0, 2] * P[0, 2] + P[1, 2] * P[1, 2] + P[2, 2] * P[2, 2])


def ref_status(err, thr_n, folded, min_angle_rad, depth1, depth2):
    with np.errstate(all="ignore"):
        return (np.where(err < thr_n, 0, A.TRI_REPROJ) | np.where(min_angle_rad < folded, 0, A.TRI_ANGLE)
                | np.where(depth2 > 0, 0, A.TRI_DEPTH2) | np.where(depth1 > 0, 0, A.TRI_DEPTH1)).astype(np.int32)


def ref_accept(status, has, reject):
    mask = np.where(has != 0, reject & A.TRI_REPROJ, reject)
    return (status & mask) == 0


def ref_quantities(item, X, rec=None):
    """Angle, error, depths and status by the reference formulas AT the positions X. `rec`: evaluate them with the
    library's own pair record (tri_pair_prepare: projection matrices and camera centres) instead of the reference's."""
    cam2 = np.asarray(item["camera_params2"], float)
    x2 = ref_image2world(int(cam2[-1]), cam2, item["points2D2"])
    if rec is None:
        P1, P2 = ref_proj_matrix(item["rvec1"], item["tvec1"]), ref_proj_matrix(item["rvec2"], item["tvec2"])
        C1, C2 = ref_centre(P1), ref_centre(P2)
    else:
        P1, P2, C1, C2 = rec[:12].reshape(3, 4), rec[12:24].reshape(3, 4), rec[24:27], rec[27:30]
    angle = ref_angles(C1, C2, X)
    err = ref_reproj_errors(P2, X, x2)
    depth = np.stack([ref_depth(P1, X), ref_depth(P2, X)], axis=1)
    thr_n = ref_threshold(item["tri_max_reproj_error"], cam2)
    min_angle_rad = item["tri_min_angle"] * np.pi / 180.0  # options.tri_min_angle * DEG2RAD, DEG2RAD = M_PI / 180.0 unparenthesised
    status = ref_status(err, thr_n, ref_fold(angle), min_angle_rad, depth[:, 0], depth[:, 1])
    return dict(angle=angle, reproj_error=err, depth=depth, status=status, thr_n=thr_n, min_angle_rad=min_angle_rad)


def ref_pair(item):
    """The whole step for one image pair: what the reference computes and which correspondences it keeps."""
    cam1, cam2 = np.asarray(item["camera_params1"], float), np.asarray(item["camera_params2"], float)
    P1, P2 = ref_proj_matrix(item["rvec1"], item["tvec1"]), ref_proj_matrix(item["rvec2"], item["tvec2"])
    x1 = ref_image2world(int(cam1[-1]), cam1, item["points2D1"])
    x2 = ref_image2world(int(cam2[-1]), cam2, item["points2D2"])
    n = len(x1)
    has = np.zeros(n, np.uint8) if item.get("has_point3D") is None else np.asarray(item["has_point3D"], np.uint8)
    X, h, sv = ref_triangulate(P1, P2, x1, x2)
    if has.any():
        X = np.where(has[:, None] != 0, np.asarray(item["points3D"], float), X)
    out = ref_quantities(item, X)
    out.update(xyz=X, h=h, sv=sv, has=has, P1=P1, P2=P2, x1=x1, x2=x2)
    out["accept"] = ref_accept(out["status"], has, item["reject"])
    out["accepted"] = np.flatnonzero(out["accept"]).astype(np.int32)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# generator: synthetic nadir pairs as in mavmap_amd/synth.py
# ---------------------------------------------------------------------------------------------------------------------
CATA_XI1_PARAMS = np.concatenate([synth.CATA_PARAMS[:8], [1.0]])
MODEL_PAIRS = {
    "pinhole_pinhole": ((A.MODEL_PINHOLE, synth.PINHOLE_PARAMS), (A.MODEL_PINHOLE, synth.PINHOLE_PARAMS)),
    "opencv_cata": ((A.MODEL_OPENCV, synth.OPENCV_PARAMS), (A.MODEL_CATA, synth.CATA_PARAMS)),
    "cata1_pinhole": ((A.MODEL_CATA, CATA_XI1_PARAMS), (A.MODEL_PINHOLE, synth.PINHOLE_PARAMS)),
}
# seeded fractions of the kinds of correspondence: chosen so that the reference's status is non-zero for 20-80 % of an item
KINDS = ("good", "outlier", "small_angle", "behind", "track", "track_moved")
KIND_P = (0.40, 0.15, 0.10, 0.10, 0.13, 0.12)
NEAR = 1e-6  # no correspondence within this (relative) of a threshold, by the reference alone


def _camera_params(model, params):
    return np.concatenate([params[:A.MODEL_NUM_PARAMS[model]], [float(model)]])


def _pose(rng, centre):
    R = synth.rodrigues(rng.uniform(-1, 1, 3) * np.deg2rad(5.0) / np.sqrt(3))[0] @ np.diag([1.0, -1.0, -1.0])
    return synth.log_so3(R), -R @ centre, R


def _draw(rng, kind, geo):
    """One correspondence of `kind`: (uv1, uv2, has, xyz_in)."""
    (m1, p1), (m2, p2), (R1, t1), (R2, t2), baseline = geo
    for _ in range(1000):
        if kind == "small_angle":  # far along a central ray of camera 1: angle between 1 and 2 degrees
            ray = np.array([rng.uniform(-0.15, 0.15), rng.uniform(-0.15, 0.15), 1.0])
            depth = baseline / np.tan(np.deg2rad(rng.uniform(1.1, 1.8)))
            X = R1.T @ (ray * depth - t1)
        elif kind == "behind":     # above both cameras: its image is that of the mirrored point in front
            X = np.array([rng.uniform(-10, 10) + baseline / 2, rng.uniform(-10, 10), synth.ALTITUDE + rng.uniform(30, 60)])
        else:                      # ground under the pair, relief sigma 2
            X = np.array([rng.uniform(-15, 15) + baseline / 2, rng.uniform(-15, 15), rng.normal(0, 2.0)])
        Xc1, Xc2 = R1 @ X + t1, R2 @ X + t2
        if kind == "behind":
            Xc1, Xc2 = -Xc1, -Xc2
        uv1 = synth.project(m1, p1, Xc1[None])[0] + rng.normal(0, 0.5, 2)
        uv2 = synth.project(m2, p2, Xc2[None])[0] + rng.normal(0, 0.5, 2)
        if kind == "outlier":      # gross mismatch in image 2
            ang = rng.uniform(0, 2 * np.pi)
            uv2 = uv2 + rng.uniform(25, 80) * np.array([np.cos(ang), np.sin(ang)])
        inside = all(0 <= p[0] <= synth.IMAGE_W and 0 <= p[1] <= synth.IMAGE_H for p in (uv1, uv2))
        if not inside:
            continue
        if kind == "track":
            return uv1, uv2, 1, X + rng.normal(0, 0.02, 3)
        if kind == "track_moved":  # a track whose stored position no longer fits the current image
            return uv1, uv2, 1, X + rng.normal(0, 1.0, 3) + np.array([rng.choice([-3.0, 3.0]), 0, 0])
        return uv1, uv2, 0, np.zeros(3)
    raise RuntimeError("no visible correspondence of kind " + kind)


def near_threshold(ref):
    """Correspondences the reference alone places within NEAR (relative) of a threshold, or at a folded angle below
    one degree (where acos has lost more than the derived-quantity tolerance assumes)."""
    X = ref["xyz"]
    folded = ref_fold(ref["angle"])
    with np.errstate(all="ignore"):
        ray1 = np.linalg.norm(X - ref_centre(ref["P1"]), axis=1)
        ray2 = np.linalg.norm(X - ref_centre(ref["P2"]), axis=1)
        bad = np.abs(ref["reproj_error"] - ref["thr_n"]) <= NEAR * ref["thr_n"]
        bad |= np.abs(folded - ref["min_angle_rad"]) <= NEAR * ref["min_angle_rad"]
        bad |= np.abs(ref["depth"][:, 0]) <= NEAR * ray1
        bad |= np.abs(ref["depth"][:, 1]) <= NEAR * ray2
        bad |= ~(folded >= np.deg2rad(1.0))
        bad |= ~np.isfinite(X).all(axis=1)
    return bad


def make_pair(n, pair="pinhole_pinhole", seed=0, reject=A.TRI_REJECT_EXTEND, tri_max_reproj_error=4.0, tri_min_angle=2.0,
              kinds=KINDS, kind_p=KIND_P):
    """One image pair as the dict mavmap_amd.triangulate_pairs takes: altitude 50, baseline 3-20, 0.5 px noise."""
    rng = np.random.default_rng([seed, n, sorted(MODEL_PAIRS).index(pair)])
    (m1, p1), (m2, p2) = MODEL_PAIRS[pair]
    baseline = rng.uniform(3.0, 20.0)
    c1 = np.array([0.0, 0.0, synth.ALTITUDE]) + rng.normal(0, 0.3, 3)
    c2 = np.array([baseline, 0.0, synth.ALTITUDE]) + rng.normal(0, 0.3, 3)
    rvec1, tvec1, R1 = _pose(rng, c1)
    rvec2, tvec2, R2 = _pose(rng, c2)
    geo = ((m1, p1), (m2, p2), (R1, tvec1), (R2, tvec2), baseline)
    kind = rng.choice(len(kinds), size=n, p=kind_p)
    item = dict(rvec1=rvec1, tvec1=tvec1, rvec2=rvec2, tvec2=tvec2, camera_params1=_camera_params(m1, p1),
                camera_params2=_camera_params(m2, p2), points2D1=np.zeros((n, 2)), points2D2=np.zeros((n, 2)),
                points3D=np.zeros((n, 3)), has_point3D=np.zeros(n, np.uint8), reject=reject,
                tri_max_reproj_error=tri_max_reproj_error, tri_min_angle=tri_min_angle, kind=kind)
    todo = np.arange(n)
    for _ in range(50):
        for i in todo:
            item["points2D1"][i], item["points2D2"][i], item["has_point3D"][i], item["points3D"][i] = _draw(rng, kinds[kind[i]], geo)
        if n == 0:
            break
        todo = np.flatnonzero(near_threshold(ref_pair(item)))
        if len(todo) == 0:
            break
    else:
        raise RuntimeError("generator could not move every correspondence away from the thresholds")
    return item


# ---------------------------------------------------------------------------------------------------------------------
# host build
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host():
    return load_host()


def load_host():
    src = os.path.join(HERE, "host", "tri_math_host.cpp")
    so = os.path.join(HERE, "host", "_tri_math_host.so")
    hdrs = [os.path.join(ROOT, "mavmap_amd", "csrc", h) for h in ("tri_math.h", "ba_math.h")]
    if not os.path.exists(so) or max(os.path.getmtime(f) for f in [src] + hdrs) > os.path.getmtime(so):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
    L = C.CDLL(so)
    L.ht_threshold.restype = C.c_double
    L.ht_threshold.argtypes = [C.c_double, dp]
    L.ht_image2world.argtypes = [C.c_int, dp, C.c_longlong, dp, dp]
    L.ht_dlt.argtypes = [dp, C.c_longlong, dp, dp, dp, dp, C.POINTER(C.c_int)]
    L.ht_pair.restype = C.c_longlong
    L.ht_pair.argtypes = [dp, dp, dp, dp, C.c_int, dp, C.c_int, dp, C.c_longlong, dp, dp, C.POINTER(C.c_uint8), dp, C.c_double, C.c_double,
                          C.c_int, dp, C.POINTER(C.c_int), C.POINTER(C.c_uint8)]
    return L


def _cam9(camera_params):
    cp = np.asarray(camera_params, float)
    return A.as_f64(np.pad(cp[:-1], (0, 9 - (len(cp) - 1)))), int(cp[-1])


def host_pair(host, item):
    """The host build over one item: the same outputs as the kernel."""
    n = len(item["points2D1"])
    cam1, m1 = _cam9(item["camera_params1"])
    cam2, m2 = _cam9(item["camera_params2"])
    uv1, uv2 = A.as_f64(item["points2D1"], (-1, 2)), A.as_f64(item["points2D2"], (-1, 2))
    has = None if item.get("has_point3D") is None else np.ascontiguousarray(item["has_point3D"], np.uint8)
    xin = None if has is None else A.as_f64(item["points3D"], (-1, 3))
    out, status, acc = np.zeros((n, 7)), np.zeros(n, np.int32), np.zeros(n, np.uint8)
    cnt = host.ht_pair(d(A.as_f64(item["rvec1"])), d(A.as_f64(item["tvec1"])), d(A.as_f64(item["rvec2"])), d(A.as_f64(item["tvec2"])),
                       m1, d(cam1), m2, d(cam2), n, d(uv1), d(uv2), A.ptr(has, C.c_uint8), A.ptr(xin, C.c_double),
                       float(item["tri_max_reproj_error"]), float(item["tri_min_angle"]), int(item["reject"]), d(out),
                       A.ptr(status, C.c_int32), A.ptr(acc, C.c_uint8))
    return dict(xyz=out[:, :3].copy(), angle=out[:, 3].copy(), reproj_error=out[:, 4].copy(), depth=out[:, 5:7].copy(), status=status,
                accepted=np.flatnonzero(acc).astype(np.int32), num_accepted=int(cnt))


def pair_record(host, item):
    """tri_pair_prepare of the host build: { P1 | P2 | C1 | C2 | baseline^2 | m1 | m2 }. The library forms the same record
    per pair on the host (csrc/triangulate.hip) and the kernel reads it, so these are the kernel's matrices to the bit."""
    rec = np.zeros(33)
    host.ht_pair_prepare(d(A.as_f64(item["rvec1"])), d(A.as_f64(item["tvec1"])), d(A.as_f64(item["rvec2"])), d(A.as_f64(item["tvec2"])), d(rec))
    # The tie to the reference, per entry and free of the translation's scale. A rotation entry is the sum
    # delta_ij + a [w]x_ij + b (w_i w_j - th^2 delta_ij): either side rounds its coefficients and each term a few times
    # (at most 8 roundings a side), so two correct evaluations differ by at most 16 eps times the sum of the terms'
    # magnitudes - not of the entry, which those terms cancel down to ~0.03 in a nadir attitude. The translation column
    # is a copy. A centre is the three-term product -R^T t: 16 eps times sum_k |R_ki| |t_k|, its condition, likewise.
    for k, (rv, tv) in enumerate(((item["rvec1"], item["tvec1"]), (item["rvec2"], item["tvec2"]))):
        P, L = ref_proj_matrix(rv, tv), rec[12 * k:12 * k + 12].reshape(3, 4)
        w = np.asarray(rv, float)
        th2 = w @ w
        th = np.sqrt(th2)
        a, b = (np.sin(th) / th, (1 - np.cos(th)) / th2) if th > 0 else (1.0, 0.5)
        Kx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
        terms = np.eye(3) + np.abs(a * Kx) + np.abs(b) * (np.abs(np.outer(w, w)) + th2 * np.eye(3))
        assert np.all(np.abs(L[:, :3] - P[:, :3]) <= 16 * EPS * terms), np.max(np.abs(L[:, :3] - P[:, :3]) / (EPS * terms))
        assert np.array_equal(L[:, 3], P[:, 3])
        cond = np.abs(P[:, :3]).T @ np.abs(P[:, 3])
        dc = np.abs(rec[24 + 3 * k:27 + 3 * k] - ref_centre(P))
        assert np.all(dc <= 16 * EPS * cond), np.max(dc / (EPS * cond))
    return rec


# ---------------------------------------------------------------------------------------------------------------------
# checks shared with the GPU test
# ---------------------------------------------------------------------------------------------------------------------
def unit_h(X):
    h = np.concatenate([X, np.ones((len(X), 1))], axis=1)
    return h / np.linalg.norm(h, axis=1, keepdims=True)


def fix_sign(h):
    """Unit homogeneous vectors with the component of the largest magnitude positive."""
    k = np.argmax(np.abs(h), axis=1)
    return h * np.sign(h[np.arange(len(h)), k])[:, None]


def dlt_bound(sv):
    return DLT_K * EPS * sv[:, 0] / (sv[:, 2] - sv[:, 3])


def check_item(got, item, ref, rec, what=""):
    """`got`: the implementation's outputs for `item` (dict or TriangulationResult); `ref`: ref_pair(item); `rec`:
    pair_record(host, item).

    The derived quantities are compared per element at 1e-12 RELATIVE. The reprojection error is a difference of two
    numbers of size 0.1-0.6 and comes out as small as 1e-5, so one rounding of a matrix entry moves it by more than
    that: the reference formulas are therefore evaluated with the library's own projection matrices (`rec`, themselves
    checked against the reference's in pair_record), at the implementation's own positions. The status test below
    uses the reference's own matrices and positions."""
    g = got if isinstance(got, dict) else dict(xyz=got.xyz, angle=got.angle, reproj_error=got.reproj_error, depth=got.depth,
                                               status=got.status, accepted=got.accepted, num_accepted=got.num_accepted)
    n = len(ref["xyz"])
    new = ref["has"] == 0
    # positions: new points within the bound of the numpy SVD, continued tracks are copies
    if new.any():
        dh = np.linalg.norm(fix_sign(unit_h(g["xyz"][new])) - fix_sign(ref["h"][new]), axis=1)
        bound = dlt_bound(ref["sv"][new])
        print(f"{what} xyz: max |dh| / (eps s1 / (s3 - s4)) = {np.max(dh / (bound / DLT_K)):.3g} (allowed {DLT_K})")
        assert np.all(dh <= bound), (what, np.max(dh / bound))
    assert np.array_equal(g["xyz"][~new], np.asarray(item["points3D"], float)[~new]), what
    # derived quantities: the reference formulas at the implementation's own positions
    q = ref_quantities(item, g["xyz"], rec)
    qa = q["angle"]
    rel = lambda a, b: np.abs(a - b) / np.maximum(np.abs(b), 1e-300)
    if n:
        e_ang = np.max(rel(g["angle"], qa) * np.sin(qa))
        e_err, e_dep = np.max(rel(g["reproj_error"], q["reproj_error"])), np.max(rel(g["depth"], q["depth"]))
        print(f"{what} derived: angle {e_ang:.3g} (x sin), error {e_err:.3g}, depth {e_dep:.3g} (allowed 1e-12)")
        assert e_ang <= 1e-12 and e_err <= 1e-12 and e_dep <= 1e-12, (what, e_ang, e_err, e_dep)
    # status: the reference rule on the implementation's own quantities, and the reference's own status
    own = ref_status(g["reproj_error"], q["thr_n"], ref_fold(g["angle"]), q["min_angle_rad"], g["depth"][:, 0], g["depth"][:, 1])
    assert np.array_equal(g["status"], own), what
    assert np.array_equal(g["status"], ref["status"]), (what, np.flatnonzero(g["status"] != ref["status"]))
    acc = np.flatnonzero(ref_accept(g["status"], ref["has"], item["reject"])).astype(np.int32)
    assert np.array_equal(g["accepted"], acc) and g["num_accepted"] == len(acc), what


def check_generator_preconditions(item, ref):
    n = len(ref["xyz"])
    if n == 0:
        return
    assert not near_threshold(ref).any()
    if n >= 63:
        frac = np.count_nonzero(ref["status"]) / n
        assert 0.2 <= frac <= 0.8, frac


# ---------------------------------------------------------------------------------------------------------------------
# tests
# ---------------------------------------------------------------------------------------------------------------------
def _kat_parameter_sets():
    kat = json.load(open(os.path.join(HERE, "golden", "world2image_kat.json")))
    seen = {}
    for v in kat["vectors"]:
        seen[(v["code"], tuple(v["params"]))] = None
    return list(seen)


def test_image2world_matches_the_numpy_restatement_and_round_trips(host):
    """The three inverse models over a pixel grid, for the parameter sets of camera_models_test.cc:60-82 (CATA with
    xi = 0, 0.5 and 1 exactly): 1e-12 on the normalised coordinates, and world2image(image2world(uv)) = uv within the
    reference's own round-trip tolerance (1e-1 px, camera_models_test.cc:34-40). The comparison with numpy runs over
    the whole grid. The round trip runs where the model's distortion is one-to-one (its reference test point (200, 100)
    lies at radius 0.69 of the normalised plane; with k1 = -0.471 the radial map folds over at 0.95): |uv - c| / f <= 0.7."""
    sets = _kat_parameter_sets()
    assert sorted({m for m, _ in sets}) == [1, 2, 3] and {p[8] for m, p in sets if m == 3} == {0, 0.5, 1}
    host.ht_world2image.argtypes = [C.c_int, dp, dp, dp]
    for model, params in sets:
        cam = np.zeros(9)
        cam[:len(params)] = params
        us, vs = np.meshgrid(np.linspace(0, 2 * cam[2], 41), np.linspace(0, 2 * cam[3], 41))
        uv = np.ascontiguousarray(np.stack([us.ravel(), vs.ravel()], axis=1))
        uv = np.concatenate([uv, [[200.0, 100.0], [cam[2], cam[3]]]])
        uv = np.ascontiguousarray(uv)
        got = np.zeros_like(uv)
        host.ht_image2world(model, d(cam), len(uv), d(uv), d(got))
        ref = ref_image2world(model, cam, uv)
        assert np.isfinite(ref).all() and np.abs(got - ref).max() <= 1e-12, (model, params, np.abs(got - ref).max())
        one_to_one = np.ones(len(uv), bool)
        if model != A.MODEL_PINHOLE:
            one_to_one = np.hypot((uv[:, 0] - cam[2]) / cam[0], (uv[:, 1] - cam[3]) / cam[1]) <= 0.7
        assert one_to_one.sum() > 400
        back = np.zeros(2)
        worst = 0.0
        for i in np.flatnonzero(one_to_one):
            host.ht_world2image(model, d(cam), d(np.array([got[i, 0], got[i, 1], 1.0])), d(back))
            worst = max(worst, np.abs(back - uv[i]).max())
        assert worst <= 1e-1, (model, params, worst)
        assert host.ht_threshold(4.0, d(cam)) == ref_threshold(4.0, cam)


def _dlt_inputs():
    """100 new correspondences of every model pair, all kinds but the continued tracks."""
    out = []
    for k, pair in enumerate(sorted(MODEL_PAIRS)):
        item = make_pair(100, pair, seed=11 + k, kinds=KINDS[:4], kind_p=(0.55, 0.2, 0.125, 0.125))
        out.append((item, ref_pair(item)))
    return out


def test_dlt_against_a_50_digit_svd(host):
    """The unit homogeneous vector of the one-sided Jacobi SVD against mpmath.svd_r at 50 digits, per point, on the
    host build's own 6 x 4 matrix inputs: |h - h_mp| <= DLT_K eps sigma1 / (sigma3 - sigma4).

    Measured over these 300 correspondences (three model pairs, good / outlier / small-angle / behind):
      numpy.linalg.svd   max |h - h_mp| / (eps sigma1 / (sigma3 - sigma4)) = 2.999
      host build         max                                               = 0.5335
    so DLT_K = 8 x 2.999 = 23.99. The sweep count of the Jacobi iteration is recorded too: at most 5 sweeps rotate
    anything (kTriMaxSweeps = 12 in tri_math.h)."""
    import mpmath
    worst_np, worst_host, worst_sweeps = 0.0, 0.0, 0
    with mpmath.workdps(50):
        for item, ref in _dlt_inputs():
            n = len(ref["xyz"])
            rec = pair_record(host, item)
            x1, x2 = np.ascontiguousarray(ref["x1"]), np.ascontiguousarray(ref["x2"])
            h, X, sweeps = np.zeros((n, 4)), np.zeros((n, 3)), np.zeros(n, np.int32)
            host.ht_dlt(d(rec), n, d(x1), d(x2), d(h), d(X), sweeps.ctypes.data_as(C.POINTER(C.c_int)))
            M = ref_dlt_matrices(ref["P1"], ref["P2"], x1, x2)
            exact = np.zeros((n, 4))
            for i in range(n):
                _, _, Vh = mpmath.svd_r(mpmath.matrix(M[i].tolist()))
                exact[i] = [float(Vh[3, c]) for c in range(4)]
            exact = fix_sign(exact)
            unit = EPS * ref["sv"][:, 0] / (ref["sv"][:, 2] - ref["sv"][:, 3])
            r_np = np.linalg.norm(fix_sign(ref["h"]) - exact, axis=1) / unit
            r_host = np.linalg.norm(fix_sign(h) - exact, axis=1) / unit
            worst_np, worst_host, worst_sweeps = max(worst_np, r_np.max()), max(worst_host, r_host.max()), max(worst_sweeps, int(sweeps.max()))
            assert np.allclose(X, h[:, :3] / h[:, 3:4], rtol=0, atol=0)
    print(f"DLT ratio: numpy {worst_np:.4g}, host build {worst_host:.4g}, DLT_K {DLT_K}; sweeps {worst_sweeps}")
    assert worst_host <= DLT_K and worst_np <= DLT_K
    assert worst_sweeps < 12


@pytest.mark.parametrize("pair", sorted(MODEL_PAIRS))
@pytest.mark.parametrize("reject", [A.TRI_REJECT_EXTEND, A.TRI_REJECT_INITIAL])
def test_host_pair_matches_the_reference(host, pair, reject):
    """Positions, derived quantities, status, acceptance and the compaction order of the host build for a whole image
    pair (new points, outliers, small angles, points behind the cameras, continued tracks)."""
    item = make_pair(257, pair, seed=3, reject=reject)
    ref = ref_pair(item)
    check_generator_preconditions(item, ref)
    check_item(host_pair(host, item), item, ref, pair_record(host, item), what=f"{pair}/{reject}")


def _degenerate_item(rvec1, tvec1, rvec2, tvec2, x1, x2):
    """Pinhole cameras with unit focal length and zero principal point: pixels ARE normalised coordinates."""
    cp = np.array([1.0, 1.0, 0.0, 0.0, float(A.MODEL_PINHOLE)])
    return dict(rvec1=np.array(rvec1, float), tvec1=np.array(tvec1, float), rvec2=np.array(rvec2, float), tvec2=np.array(tvec2, float),
                camera_params1=cp, camera_params2=cp, points2D1=np.array(x1, float).reshape(-1, 2), points2D2=np.array(x2, float).reshape(-1, 2),
                reject=A.TRI_REJECT_EXTEND | A.TRI_DEPTH1, tri_max_reproj_error=4.0 / 600.0, tri_min_angle=2.0)


def test_degenerate_inputs_terminate_and_classify_as_the_reference_does(host):
    # identical poses: rank-deficient A, the angle is NaN or 0 -> 0, the angle bit is set
    rng = np.random.default_rng(5)
    x = rng.uniform(-0.3, 0.3, (64, 2))
    it = _degenerate_item([0.1, -0.2, 0.05], [1, 2, 3], [0.1, -0.2, 0.05], [1, 2, 3], x, x + rng.normal(0, 1e-3, x.shape))
    got = host_pair(host, it)
    assert np.all(got["angle"] == 0.0) and np.all(got["status"] & A.TRI_ANGLE) and got["num_accepted"] == 0
    it = _degenerate_item([0.1, -0.2, 0.05], [1, 2, 3], [0.1, -0.2, 0.05], [1, 2, 3], x, x)  # and exactly the same points
    got = host_pair(host, it)
    assert np.all(got["angle"] == 0.0) and np.all(got["status"] & A.TRI_ANGLE) and got["num_accepted"] == 0

    # parallel rays: the point is at infinity, xyz is non-finite, the reprojection and depth bits are set
    it = _degenerate_item([0, 0, 0], [0, 0, 0], [0, 0, 0], [-5, 0, 0], [[0, 0]], [[0, 0]])
    got = host_pair(host, it)
    assert not np.isfinite(got["xyz"]).all()
    assert got["status"][0] & A.TRI_REPROJ and got["status"][0] & A.TRI_DEPTH1 and got["status"][0] & A.TRI_DEPTH2
    assert got["num_accepted"] == 0

    # a point in front of camera 1 and behind camera 2 (camera 2 has flown past it), and the other way round
    X = np.array([0.5, -0.3, 10.0])
    for t2, bits in (([-1.0, 0.0, -20.0], A.TRI_DEPTH2), ([-1.0, 0.0, 0.0], 0)):
        Xc2 = X + np.array(t2)
        it = _degenerate_item([0, 0, 0], [0, 0, 0], [0, 0, 0], t2, [X[:2] / X[2]], [Xc2[:2] / Xc2[2]])
        ref, got = ref_pair(it), host_pair(host, it)
        assert np.allclose(got["xyz"], X, rtol=1e-9)
        assert got["status"][0] & (A.TRI_DEPTH1 | A.TRI_DEPTH2) == bits and np.array_equal(got["status"], ref["status"])
        assert got["num_accepted"] == (0 if bits else 1)
    Xc1 = X + np.array([0.0, 0.0, -20.0])
    Xc2 = X + np.array([-1.0, 0.0, 0.0])
    it = _degenerate_item([0, 0, 0], [0, 0, -20.0], [0, 0, 0], [-1.0, 0, 0], [Xc1[:2] / Xc1[2]], [Xc2[:2] / Xc2[2]])
    ref, got = ref_pair(it), host_pair(host, it)
    assert np.allclose(got["xyz"], X, rtol=1e-9)
    assert got["status"][0] & (A.TRI_DEPTH1 | A.TRI_DEPTH2) == A.TRI_DEPTH1 and np.array_equal(got["status"], ref["status"])
    assert got["num_accepted"] == 0
    it["reject"] = A.TRI_REJECT_EXTEND  # the map extension does not look at image 1's depth
    assert host_pair(host, it)["num_accepted"] == 1

    # NaN input ends the iteration too and is rejected by every test
    it = _degenerate_item([0, 0, 0], [0, 0, 0], [0, 0, 0], [-5, 0, 0], [[np.nan, 0]], [[0, 0.1]])
    got = host_pair(host, it)
    assert got["status"][0] == A.TRI_REPROJ | A.TRI_ANGLE | A.TRI_DEPTH1 | A.TRI_DEPTH2


# ---------------------------------------------------------------------------------------------------------------------
# C ABI without a device
# ---------------------------------------------------------------------------------------------------------------------
def test_tri_pair_layout_matches_the_header():
    src = r"""
#include <stdio.h>
#include <stddef.h>
#include "mavba_triangulate.h"
int main(void) {
  printf("%zu %zu %zu %zu %d %d %d %d\n", sizeof(mavba_tri_pair), offsetof(mavba_tri_pair, uv1), offsetof(mavba_tri_pair, reject_bits),
         offsetof(mavba_tri_pair, num_accepted), MAVBA_TRI_REPROJ, MAVBA_TRI_ANGLE, MAVBA_TRI_DEPTH2, MAVBA_TRI_DEPTH1);
  return 0;
}"""
    with tempfile.TemporaryDirectory() as td:
        open(os.path.join(td, "t.c"), "w").write(src)
        exe = os.path.join(td, "t")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(td, "t.c"), "-o", exe])
        out = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    assert out[:4] == [C.sizeof(A.CTriPair), A.CTriPair.uv1.offset, A.CTriPair.reject_bits.offset, A.CTriPair.num_accepted.offset]
    assert out[4:] == [A.TRI_REPROJ, A.TRI_ANGLE, A.TRI_DEPTH2, A.TRI_DEPTH1]


def c_items(items, outputs=("xyz", "angle", "reproj_error", "depth", "status", "accepted")):
    """(ctypes array, output arrays, keep-alive) for a raw mavba_triangulate_pairs call; outputs not named are NULL."""
    arr = (A.CTriPair * max(len(items), 1))()
    outs, hold = [], []
    for q, it in enumerate(items):
        cam1, m1 = _cam9(it["camera_params1"])
        cam2, m2 = _cam9(it["camera_params2"])
        uv1, uv2 = A.as_f64(it["points2D1"], (-1, 2)), A.as_f64(it["points2D2"], (-1, 2))
        n = len(uv1)
        has = None if it.get("has_point3D") is None else np.ascontiguousarray(it["has_point3D"], np.uint8)
        xin = None if has is None else A.as_f64(it["points3D"], (-1, 3))
        hold.append((cam1, cam2, uv1, uv2, has, xin))
        c = arr[q]
        for k in range(3):
            c.rvec1[k], c.tvec1[k], c.rvec2[k], c.tvec2[k] = it["rvec1"][k], it["tvec1"][k], it["rvec2"][k], it["tvec2"][k]
        c.intrinsics1, c.intrinsics2, c.camera_model1, c.camera_model2 = d(cam1), d(cam2), m1, m2
        c.uv1, c.uv2, c.n = d(uv1), d(uv2), n
        c.xyz_in, c.has_xyz = A.ptr(xin, C.c_double), A.ptr(has, C.c_uint8)
        c.max_reproj_error_px, c.min_angle_deg, c.reject_bits = it["tri_max_reproj_error"], it["tri_min_angle"], it["reject"]
        o = dict(xyz=np.full((n, 3), -7.0), angle=np.full(n, -7.0), reproj_error=np.full(n, -7.0), depth=np.full((n, 2), -7.0),
                 status=np.full(n, -7, np.int32), accepted=np.full(n, -7, np.int32))
        for name in outputs:
            setattr(c, name, A.ptr(o[name], C.c_int32 if o[name].dtype == np.int32 else C.c_double))
        c.num_accepted, c.mean_folded_angle_deg = -7, -7.0
        outs.append(o)
    return arr, outs, hold


def test_abi_without_a_device(mavba):
    from mavmap_amd import api
    L = mavba.load()
    # the pin tests/test_abi.py holds on mavba.h, on this header: every function it declares is listed and exported
    import re
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mavba_triangulate.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(mavba_[a-z0-9_]+)\s*\(", header)))
    assert declared == sorted(api.TRIANGULATE_SYMBOLS) == ["mavba_triangulate_pairs"]
    assert all(hasattr(L, name) for name in declared) and not set(declared) & set(api.EXPORTED_SYMBOLS)
    assert mavba.triangulate_pairs([]) == []
    assert L.mavba_triangulate_pairs(0, None, -1) == A.OK
    item = make_pair(65, "opencv_cata", seed=1)
    # invalid arguments give their codes on any machine
    assert L.mavba_triangulate_pairs(-1, None, -1) == A.ERR_INVALID_ARGUMENT
    assert L.mavba_triangulate_pairs(1, None, -1) == A.ERR_INVALID_ARGUMENT
    for field, value, code in (("n", -1, A.ERR_INVALID_ARGUMENT), ("uv1", None, A.ERR_INVALID_ARGUMENT), ("uv2", None, A.ERR_INVALID_ARGUMENT),
                               ("intrinsics2", None, A.ERR_INVALID_ARGUMENT), ("xyz_in", None, A.ERR_INVALID_ARGUMENT),
                               ("camera_model1", 0, A.ERR_BAD_MODEL), ("camera_model2", 4, A.ERR_BAD_MODEL)):
        arr, outs, hold = c_items([item])
        setattr(arr[0], field, C.cast(None, dp) if value is None else value)
        assert L.mavba_triangulate_pairs(1, arr, -1) == code, field
        assert np.all(outs[0]["xyz"] == -7.0) and arr[0].num_accepted == -7
    arr, outs, hold = c_items([make_pair(0, "pinhole_pinhole", seed=1)], outputs=())
    for field in ("intrinsics1", "intrinsics2", "uv1", "uv2"):
        setattr(arr[0], field, C.cast(None, dp))  # an empty item may leave every pointer NULL
    assert L.mavba_triangulate_pairs(1, arr, -1) in (A.OK, A.ERR_NO_DEVICE)
    if mavba.device_count() > 0:
        assert arr[0].num_accepted == 0 and np.isnan(arr[0].mean_folded_angle_deg)
        return  # (the rest is what a machine without a GPU answers)
    arr, outs, hold = c_items([item])
    assert L.mavba_triangulate_pairs(1, arr, -1) == A.ERR_NO_DEVICE
    assert all(np.all(o == -7) for o in outs[0].values()) and arr[0].num_accepted == -7 and arr[0].mean_folded_angle_deg == -7.0
    with pytest.raises(mavba.MavbaError) as ei:
        mavba.triangulate_pairs([item])
    assert ei.value.code == A.ERR_NO_DEVICE and "no CPU path" in str(ei.value)
