"""Absolute pose by P3P inside RANSAC (mavmap_amd/csrc/p3p_math.h) compiled for the HOST by g++ and checked against a
numpy restatement of the reference lines it replaces, plus the C ABI of mavba_absolute_pose_ransac without a device.

The checker below restates, in numpy and in the reference's order of operations,
  src/base3d/p3p.cc:26-169        P3PEstimator::estimate (numpy.roots where the reference has poly_solve,
                                  numpy.linalg.svd inside a restated Eigen::umeyama(..., false))
  src/base3d/p3p.cc:172-199       the residuals
  src/util/estimation.cc:15-21    dynamic_max_trials_ (Python's math.log / pow / ceil)
  src/util/estimation.cc:104-133  the score of a model and the selection among the trials
(the reference's own p3p.cc needs Eigen and cannot be compiled for these tests), and the same hypothesis with mpmath at
50 digits as ground truth. tests/test_gpu_absolute_pose.py uses the same checker and the same generators for the kernel.
"""
import ctypes as C
import functools
import math
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from mavmap_amd import _abi as A
from mavmap_amd import synth

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
dp = C.POINTER(C.c_double)
DBL_MIN, DBL_MAX = sys.float_info.min, sys.float_info.max

# Hypothesis: e_lib <= P3P_K * e_ref per sample, e = max |M - M_50| over the 12 entries of the model, e_ref = the numpy
# restatement's own error at that sample (the largest over the sample and 8 copies with every input moved by +-2^-52
# relative, each against its own 50-digit model). P3P_K = 8 x the largest e_host / e_ref measured on the 300 inputs of
# test_hypothesis_against_50_digits, where the figures are recorded.
P3P_MEASURED_MAX = 1.441
P3P_K = 8 * P3P_MEASURED_MAX

MODELS = {A.MODEL_PINHOLE: synth.PINHOLE_PARAMS, A.MODEL_OPENCV: synth.OPENCV_PARAMS, A.MODEL_CATA: synth.CATA_PARAMS}


def d(a):
    return a.ctypes.data_as(dp)


# ---------------------------------------------------------------------------------------------------------------------
# the generator of include/mavba_absolute_pose.h, restated with Python integers
# ---------------------------------------------------------------------------------------------------------------------
M64 = (1 << 64) - 1


def py_mix(seed, t, draw):
    z = (seed + 0x9E3779B97F4A7C15 * ((t << 32) + draw + 1)) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def py_sample(seed, t, n):
    row = []
    for draw in range(64):
        v = ((py_mix(seed, t, draw) >> 32) * n) >> 32
        if v not in row:
            row.append(v)
        if len(row) == 4:
            break
    v = 0
    while len(row) < 4:
        if v not in row:
            row.append(v)
        v += 1
    return sorted(row)


# ---------------------------------------------------------------------------------------------------------------------
# numpy / mpmath restatement of P3PEstimator::estimate
# ---------------------------------------------------------------------------------------------------------------------
class _NumpyOps:
    one = 1.0
    sqrt = staticmethod(math.sqrt)

    @staticmethod
    def num(v):
        return float(v)

    @staticmethod
    def roots(c4, c3, c2, c1, c0):
        with np.errstate(all="ignore"):
            r = np.roots([c4, c3, c2, c1, c0])
        return [(float(z.real), float(z.imag)) for z in r]

    @staticmethod
    def svd3(S):
        U, _, Vt = np.linalg.svd(np.array(S, float))
        return U.tolist(), Vt.tolist()


class _MpOps:
    def __init__(self):
        import mpmath
        self.mp = mpmath
        self.one = mpmath.mpf(1)
        self.sqrt = mpmath.sqrt

    def num(self, v):
        return self.mp.mpf(float(v))

    def roots(self, c4, c3, c2, c1, c0):
        r = self.mp.polyroots([c4, c3, c2, c1, c0], maxsteps=500, extraprec=400)
        return [(z.real, z.imag) for z in r]

    def svd3(self, S):
        U, _, Vt = self.mp.svd_r(self.mp.matrix(S))
        return [[U[i, j] for j in range(3)] for i in range(3)], [[Vt[i, j] for j in range(3)] for i in range(3)]


def _det3(m):
    return (m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0])
            + m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]))


def _umeyama(ops, src, dst):
    """Eigen::umeyama(src, dst, false) for three points (src[k], dst[k] = point k): the 3 x 4 matrix [R | t]. sigma has
    rank two, so Eigen takes R = U diag(1, 1, det U det V) V^T."""
    third = ops.one / 3
    sm = [(src[0][c] + src[1][c] + src[2][c]) * third for c in range(3)]
    dm = [(dst[0][c] + dst[1][c] + dst[2][c]) * third for c in range(3)]
    sigma = [[third * sum((dst[k][r] - dm[r]) * (src[k][c] - sm[c]) for k in range(3)) for c in range(3)] for r in range(3)]
    U, Vt = ops.svd3(sigma)
    s = 1 if _det3(U) * _det3(Vt) > 0 else -1
    R = [[U[r][0] * Vt[0][c] + U[r][1] * Vt[1][c] + s * U[r][2] * Vt[2][c] for c in range(3)] for r in range(3)]
    t = [dm[r] - (R[r][0] * sm[0] + R[r][1] * sm[1] + R[r][2] * sm[2]) for r in range(3)]
    return [R[r] + [t[r]] for r in range(3)]


def _p3p(ops, x2d, X):
    """P3PEstimator::estimate on four lifted observations x2d [4, 2] and world points X [4, 3] (rows ascending).
    Returns dict(model [12] or None, roots [(re, im)], cands [(error of D, x, model)])."""
    x2d = [[ops.num(v) for v in row] for row in np.asarray(x2d, float).reshape(4, 2)]
    X = [[ops.num(v) for v in row] for row in np.asarray(X, float).reshape(4, 3)]
    sqrt = ops.sqrt
    bear = []
    for k in range(3):
        N = sqrt(x2d[k][0] * x2d[k][0] + x2d[k][1] * x2d[k][1] + 1)
        bear.append([x2d[k][0] / N, x2d[k][1] / N, 1 / N])
    u, v, w = bear
    dot = lambda a, b: a[0] * b[0] + a[1] * b[1] + a[2] * b[2]  # noqa: E731
    dist = lambda a, b: sqrt((a[0] - b[0]) * (a[0] - b[0]) + (a[1] - b[1]) * (a[1] - b[1]) + (a[2] - b[2]) * (a[2] - b[2]))  # noqa: E731
    cos_uv, cos_uw, cos_vw = dot(u, v), dot(u, w), dot(v, w)
    dist_AB, dist_AC, dist_BC = dist(X[0], X[1]), dist(X[0], X[2]), dist(X[1], X[2])
    dist_AB_2 = dist_AB * dist_AB
    a = (dist_BC * dist_BC) / dist_AB_2
    b = (dist_AC * dist_AC) / dist_AB_2
    a2, b2 = a * a, b * b
    p, q, r = 2 * cos_vw, 2 * cos_uw, 2 * cos_uv
    p2 = p * p
    p3 = p2 * p
    q2 = q * q
    r2 = r * r
    r3 = r2 * r
    r4 = r3 * r
    r5 = r4 * r
    c4 = -2 * b + b2 + a2 + 1 + a * b * (2 - r2) - 2 * a
    c3 = -2 * q * a2 - r * p * b2 + 4 * q * a + (2 * q + p * r) * b + (r2 * q - 2 * q + r * p) * a * b - 2 * q
    c2 = (2 + q2) * a2 + (p2 + r2 - 2) * b2 - (4 + 2 * q2) * a - (p * q * r + p2) * b - (p * q * r + r2) * a * b + q2 + 2
    c1 = -2 * q * a2 - r * p * b2 + 4 * q * a + (p * r + q * p2 - 2 * q) * b + (r * p + 2 * q) * a * b - 2 * q
    c0 = a2 + b2 - 2 * a + (2 - p2) * b - 2 * a * b + 1
    roots = ops.roots(c4, c3, c2, c1, c0)
    cands = []
    for x, xi in roots:
        if xi > 1e-10 or x < 0:  # (on imag, not |imag|: of a complex pair the root of negative imaginary part goes on)
            continue
        x2 = x * x
        x3 = x2 * x
        _b1 = (p2 - p * q * r + r2) * a + (p2 - r2) * b - p2 + p * q * r - r2
        b1 = b * _b1 * _b1
        b0 = ((1 - a - b) * x2 + (a - 1) * q * x - a + b + 1) * (
            r3 * (a2 + b2 - 2 * a - 2 * b + (2 - r2) * a * b + 1) * x3
            + r2 * (p + p * a2 - 2 * r * q * a * b + 2 * r * q * b - 2 * r * q - 2 * p * a - 2 * p * b + p * r2 * b + 4 * r * q * a
                    + q * r3 * a * b - 2 * r * q * a2 + 2 * p * a * b + p * b2 - r2 * p * b2) * x2
            + (r5 * (b2 - a * b) - r4 * p * q * b + r3 * (q2 - 4 * a - 2 * q2 * a + q2 * a2 + 2 * a2 - 2 * b2 + 2)
               + r2 * (4 * p * q * a - 2 * p * q * a * b + 2 * p * q * b - 2 * p * q - 2 * p * q * a2)
               + r * (p2 * b2 - 2 * p2 * b + 2 * p2 * a * b - 2 * p2 * a + p2 + p2 * a2)) * x
            + (2 * p * r2 - 2 * r3 * q + p3 - 2 * p2 * q * r + p * q2 * r2) * a2 + (p3 - 2 * p * r2) * b2
            + (4 * q * r3 - 4 * p * r2 - 2 * p3 + 4 * p2 * q * r - 2 * p * q2 * r2) * a
            + (-2 * q * r3 + p * r4 + 2 * p2 * q * r - 2 * p3) * b + (2 * p3 + 2 * q * r3 - 2 * p2 * q * r) * a * b
            + p * q2 * r2 - 2 * p2 * q * r + 2 * p * r2 + p3 - 2 * r3 * q)
        y = b0 / b1
        y2 = y * y
        nu = x2 + y2 - 2 * x * y * cos_uv
        dist_PC = dist_AB / sqrt(nu)
        dist_PB = y * dist_PC
        dist_PA = x * dist_PC
        cam = [[u[k] * dist_PA for k in range(3)], [v[k] * dist_PB for k in range(3)], [w[k] * dist_PC for k in range(3)]]
        M = _umeyama(ops, X[:3], cam)
        zp = [M[r_][0] * X[3][0] + M[r_][1] * X[3][1] + M[r_][2] * X[3][2] + M[r_][3] for r_ in range(3)]
        dx, dy = zp[0] / zp[2] - x2d[3][0], zp[1] / zp[2] - x2d[3][1]
        cands.append((sqrt(dx * dx + dy * dy), x, M))
    best, model = DBL_MAX, None
    for err, _, M in cands:
        if err < best:
            best, model = err, M
    if model is not None:
        model = np.array([[float(v_) for v_ in row] for row in model]).reshape(12)
    return dict(model=model, roots=roots, cands=cands)


def ref_p3p(x2d, X):
    try:
        with np.errstate(all="ignore"):
            return _p3p(_NumpyOps, x2d, X)
    except (ZeroDivisionError, ValueError, np.linalg.LinAlgError):
        return dict(model=None, roots=[], cands=[])


def mp_p3p(x2d, X):
    import mpmath
    with mpmath.workdps(50):
        return _p3p(_MpOps(), x2d, X)


# ---------------------------------------------------------------------------------------------------------------------
# numpy restatement of the score and the selection
# ---------------------------------------------------------------------------------------------------------------------
def ref_residuals(M, xy, xyz):
    """p3p.cc:190-195 for one model [12] or many [T, 12]: residuals [..., n]."""
    M = np.asarray(M, float).reshape(-1, 12)
    X, Y, Z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    with np.errstate(all="ignore"):
        row = lambda k: (M[:, 4 * k, None] * X + M[:, 4 * k + 1, None] * Y + M[:, 4 * k + 2, None] * Z) + M[:, 4 * k + 3, None]  # noqa: E731
        p2 = row(2)
        dx, dy = row(0) / p2 - xy[:, 0], row(1) / p2 - xy[:, 1]
        return np.sqrt(dx * dx + dy * dy)


def py_limit(k, n, probability):
    """dynamic_max_trials_(k, n, 4, probability) with Python's libm; None: no limit (the quotient is not finite)."""
    e = 1 - k / float(n)
    nom = max(DBL_MIN, 1 - probability)
    denom = max(DBL_MIN, 1 - math.pow(1 - e, 4))
    try:
        quot = math.log(nom) / math.log(denom)
    except ZeroDivisionError:
        return None
    if not math.isfinite(quot):
        return None
    return min(max(math.ceil(quot), 0), 2 ** 31 - 1)


def replay_selection(valid, counts, sums, n, stop, probability):
    """estimation.cc:119-133 over the trials in order. Returns dict(best_trial, trials_used, num_inliers, tie_decided)."""
    best, best_sum, best_trial, used, tie = 0, DBL_MAX, -1, 0, False
    for t in range(len(counts)):
        c, s = int(counts[t]), float(sums[t])
        if valid[t] and (c > best or (c == best and s < best_sum)):
            tie |= best_trial >= 0 and c == best and c >= 4
            best, best_sum, best_trial = c, s, t
        used = t + 1
        lim = py_limit(c, n, probability)
        if (stop > 0 and best >= stop) or (lim is not None and t >= lim):
            break
    return dict(best_trial=best_trial, trials_used=used, num_inliers=best, tie_decided=tie)


# ---------------------------------------------------------------------------------------------------------------------
# generators
# ---------------------------------------------------------------------------------------------------------------------
def camera_params(model):
    return np.concatenate([MODELS[model][:A.MODEL_NUM_PARAMS[model]], [float(model)]])


def _cam9(cp):
    cp = np.asarray(cp, float)
    return A.as_f64(np.pad(cp[:-1], (0, 9 - (len(cp) - 1)))), int(cp[-1])


def make_scene(n, model, seed, noise_px=0.0, outlier_frac=0.0, outlier_px=(0.0, 0.0)):
    """n world points in front of a camera of `model`, their pixels with uniform noise in a disc of radius noise_px; a
    fraction moved by outlier_px[0]..outlier_px[1] pixels. Returns dict(camera_params, points2D, points3D, rvec, tvec, outlier)."""
    rng = np.random.default_rng([seed, n, model])
    R = synth.rodrigues(rng.uniform(-0.4, 0.4, 3))[0]
    t = rng.uniform(-1.0, 1.0, 3)
    params = MODELS[model]
    uv, xyz = np.zeros((n, 2)), np.zeros((n, 3))
    outlier = rng.uniform(size=n) < outlier_frac
    for i in range(n):
        while True:
            Xc = np.array([rng.uniform(-4, 4), rng.uniform(-3, 3), rng.uniform(4, 12)])
            p = synth.project(model, params, Xc[None])[0]
            if 20 <= p[0] <= synth.IMAGE_W - 20 and 20 <= p[1] <= synth.IMAGE_H - 20:
                break
        ang, rad = rng.uniform(0, 2 * np.pi), noise_px * np.sqrt(rng.uniform())
        if outlier[i]:
            rad = rng.uniform(*outlier_px)
        uv[i] = p + rad * np.array([np.cos(ang), np.sin(ang)])
        xyz[i] = R.T @ (Xc - t)
    return dict(camera_params=camera_params(model), points2D=uv, points3D=xyz, rvec=synth.log_so3(R), tvec=t, outlier=outlier)


def make_item(n, model=A.MODEL_PINHOLE, seed=0, max_trials=500, stop_frac=None, supplied=False, max_reproj_error=4.0, probability=0.99):
    """One RANSAC item as mavmap_amd.absolute_pose_ransac takes it: 30 % outliers at 3 to 20 thresholds, inlier noise up
    to 0.3 thresholds. stop_frac: stop_num_inliers as a share of n (None: no stop). supplied: the rows are given."""
    it = make_scene(n, model, seed, noise_px=0.3 * max_reproj_error, outlier_frac=0.3 if n > 5 else 0.0,
                    outlier_px=(3 * max_reproj_error, 20 * max_reproj_error))
    it.update(max_trials=max_trials, max_reproj_error=max_reproj_error, probability=probability, seed=1000 + seed,
              stop_num_inliers=0 if stop_frac is None else int(math.ceil(stop_frac * n)))
    if supplied:
        rng = np.random.default_rng([7, seed, n])
        it["samples"] = np.array([rng.permutation(n)[:4] for _ in range(max_trials)], np.int32).reshape(max_trials, 4)
    return it


# ---------------------------------------------------------------------------------------------------------------------
# host build
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host():
    return load_host()


@functools.lru_cache(maxsize=None)
def load_host():
    src = os.path.join(HERE, "host", "p3p_math_host.cpp")
    so = os.path.join(HERE, "host", "_p3p_math_host.so")
    hdrs = [os.path.join(ROOT, "mavmap_amd", "csrc", h) for h in ("p3p_math.h", "ransac_core.h", "tri_math.h", "ba_math.h")]
    hdrs.append(os.path.join(ROOT, "include", "mavba_absolute_pose.h"))
    if not os.path.exists(so) or max(os.path.getmtime(f) for f in [src] + hdrs) > os.path.getmtime(so):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
    L = C.CDLL(so)
    L.hp_draw_samples.argtypes = [C.c_uint64, C.c_longlong, C.c_int, C.POINTER(C.c_int32)]
    L.hp_image2world.argtypes = [C.c_int, dp, C.c_longlong, dp, dp]
    L.hp_estimate.argtypes = [C.c_longlong, dp, dp, dp, C.POINTER(C.c_uint8)]
    L.hp_rvec.argtypes = [dp, dp]
    L.hp_dynamic_limit.argtypes = [C.c_longlong, C.c_longlong, C.c_double]
    L.hp_dynamic_limit.restype = C.c_int
    L.hp_absolute_pose.argtypes = [C.POINTER(A.CAbsPoseItem)]
    L.hp_absolute_pose.restype = None
    return L


def lift(item):
    """The lifted observations [n, 2] (host build of image2world: the library's own packing step) and the threshold."""
    cam, model = _cam9(item["camera_params"])
    uv = A.as_f64(item["points2D"], (-1, 2))
    xy = np.zeros_like(uv)
    if len(uv):
        load_host().hp_image2world(model, d(cam), len(uv), d(uv), d(xy))
    return xy, item.get("max_reproj_error", 4.0) / ((cam[0] + cam[1]) / 2)


OUTPUTS = ("inlier_mask", "trial_models", "trial_num_inliers", "trial_residual_sum", "trial_samples")


def c_items(items, outputs=OUTPUTS, fill=None):
    """(ctypes array, output arrays, keep-alive) for a raw call; outputs not named are NULL. fill: the value every output
    array and scalar starts with (to see what a call leaves untouched)."""
    arr = (A.CAbsPoseItem * max(len(items), 1))()
    outs, hold = [], []
    for q, it in enumerate(items):
        cam, model = _cam9(it["camera_params"])
        uv, xyz = A.as_f64(it["points2D"], (-1, 2)), A.as_f64(it["points3D"], (-1, 3))
        n, mt = len(uv), int(it.get("max_trials", 500))
        smp = None if it.get("samples") is None else np.ascontiguousarray(it["samples"], np.int32)
        hold.append((cam, uv, xyz, smp))
        c = arr[q]
        c.intrinsics, c.camera_model, c.uv, c.xyz, c.n = d(cam), model, d(uv), d(xyz), n
        c.max_reproj_error_px, c.max_trials = it.get("max_reproj_error", 4.0), mt
        c.stop_num_inliers, c.probability = int(it.get("stop_num_inliers", 0)), it.get("probability", 0.99)
        c.samples, c.seed = A.ptr(smp, C.c_int32), int(it.get("seed", 0))
        k = max(mt, 0)
        f = 0 if fill is None else fill
        o = dict(inlier_mask=np.full(n, f % 256, np.uint8), trial_models=np.full((k, 12), float(f)), trial_num_inliers=np.full(k, f, np.int32),
                 trial_residual_sum=np.full(k, float(f)), trial_samples=np.full((k, 4), f, np.int32))
        for name in outputs:
            ct = {np.dtype(np.uint8): C.c_uint8, np.dtype(np.int32): C.c_int32, np.dtype(np.float64): C.c_double}[o[name].dtype]
            setattr(c, name, A.ptr(o[name], ct))
        if fill is not None:
            for k_ in range(3):
                c.rvec[k_] = c.tvec[k_] = float(f)
            c.num_inliers = c.best_trial = c.trials_used = c.status = f
            c.kernel_seconds = float(f)
        outs.append(o)
    return arr, outs, hold


def records(arr, outs):
    """What a call left, one dict per item."""
    return [dict(o, rvec=np.array(arr[q].rvec), tvec=np.array(arr[q].tvec), proj_matrix=np.array(arr[q].proj_matrix),
                 num_inliers=int(arr[q].num_inliers), best_trial=int(arr[q].best_trial), trials_used=int(arr[q].trials_used),
                 status=int(arr[q].status), kernel_seconds=float(arr[q].kernel_seconds)) for q, o in enumerate(outs)]


def host_run(items, outputs=OUTPUTS):
    """The host build over every item (one thread, the kernel's outputs)."""
    L = load_host()
    arr, outs, hold = c_items(items, outputs)
    for q in range(len(items)):
        L.hp_absolute_pose(C.byref(arr[q]))
    return records(arr, outs)


# ---------------------------------------------------------------------------------------------------------------------
# checks shared with the GPU test
# ---------------------------------------------------------------------------------------------------------------------
def check_models(M, what=""):
    """Properties of every valid model [T, 12] that need no yardstick; rvec through hp_rvec composed back into R."""
    L = load_host()
    M = np.asarray(M, float).reshape(-1, 12)
    for m in M[np.isfinite(M).all(axis=1)]:
        R = m.reshape(3, 4)[:, :3]
        assert np.abs(R.T @ R - np.eye(3)).max() <= 1e-12, what
        assert np.linalg.det(R) > 0, what
        rvec = np.zeros(3)
        L.hp_rvec(d(np.ascontiguousarray(m)), d(rvec))
        assert np.abs(synth.rodrigues(rvec)[0] - R).max() <= 1e-12, what


def check_record(rec, item, what="", expect=None):
    """Scoring and selection of one item from the implementation's own trial_models.
    Returns the replay (for the assertions on what a case was built to show)."""
    n, mt = len(item["points2D"]), int(item["max_trials"])
    xy, thr = lift(item)
    xyz = A.as_f64(item["points3D"], (-1, 3))
    M = rec["trial_models"].reshape(mt, 12)
    valid = np.isfinite(M).all(axis=1)
    assert np.array_equal(np.isnan(M).any(axis=1), ~valid) and np.all(np.isnan(M[~valid])), what  # invalid = all NaN
    # the rows: distinct, in range, ascending; the supplied ones sorted, the drawn ones those of the recipe
    rows = rec["trial_samples"]
    assert np.all(rows >= 0) and np.all(rows < n) and np.all(np.diff(rows, axis=1) > 0), what
    if item.get("samples") is not None:
        assert np.array_equal(rows, np.sort(np.asarray(item["samples"]), axis=1)), what
    else:
        assert np.array_equal(rows, np.array([py_sample(int(item["seed"]), t, n) for t in range(mt)], np.int32).reshape(mt, 4)), what
    res = ref_residuals(np.where(valid[:, None], M, 0.0), xy, xyz)
    # precondition, asserted: no residual of any trial lies within 1e-9 relative of the threshold
    with np.errstate(all="ignore"):
        assert not np.any(np.abs(res[valid] - thr) <= 1e-9 * thr), (what, "a residual at the threshold: change the seed")
        inl = (res <= thr) & valid[:, None]
    counts = inl.sum(axis=1)
    sums = np.where(inl, res, 0.0).sum(axis=1)
    assert np.array_equal(rec["trial_num_inliers"], counts), (what, np.flatnonzero(rec["trial_num_inliers"] != counts))
    assert np.all(np.abs(rec["trial_residual_sum"] - sums) <= 1e-12 * np.abs(sums)), what
    assert np.all(rec["trial_residual_sum"][~valid] == 0) and np.all(rec["trial_num_inliers"][~valid] == 0), what
    check_models(M, what)
    # the selection, replayed on the implementation's own counts and sums
    rp = replay_selection(valid, rec["trial_num_inliers"], rec["trial_residual_sum"], n, int(item["stop_num_inliers"]), item["probability"])
    assert rec["trials_used"] == rp["trials_used"], (what, rec["trials_used"], rp)
    if rp["best_trial"] >= 0 and rp["num_inliers"] >= 4:
        assert rec["status"] == A.ABSPOSE_OK and rec["best_trial"] == rp["best_trial"] and rec["num_inliers"] == rp["num_inliers"], (what, rp)
        b = rec["best_trial"]
        assert np.array_equal(rec["inlier_mask"], inl[b].astype(np.uint8)), what
        assert rec["proj_matrix"].tobytes() == M[b].tobytes(), what
        assert np.array_equal(rec["tvec"], M[b][[3, 7, 11]]), what
        assert np.abs(synth.rodrigues(rec["rvec"])[0] - M[b].reshape(3, 4)[:, :3]).max() <= 1e-12, what
    else:
        assert rec["status"] == A.ABSPOSE_NO_CONSENSUS and rec["best_trial"] == -1 and rec["num_inliers"] == 0, what
        assert np.isnan(rec["rvec"]).all() and np.isnan(rec["tvec"]).all() and np.isnan(rec["proj_matrix"]).all(), what
        assert not rec["inlier_mask"].any(), what
    return rp


# ---------------------------------------------------------------------------------------------------------------------
# the 300 hypothesis inputs and their yardstick
# ---------------------------------------------------------------------------------------------------------------------
HYP_SEED = 2


@functools.lru_cache(maxsize=None)
def hypothesis_scenes():
    """300 scenes of four points (100 per camera model): points in front of the camera, 1e-3 normalised noise."""
    return [make_scene(4, model, HYP_SEED * 1000 + k, noise_px=1e-3 * MODELS[model][0]) for model in sorted(MODELS) for k in range(100)]


@functools.lru_cache(maxsize=None)
def hypothesis_inputs():
    """The 300 hypotheses as lifted observations x2d [300, 4, 2] and world points X [300, 4, 3]."""
    sc = hypothesis_scenes()
    return np.ascontiguousarray([lift(s)[0] for s in sc]), np.ascontiguousarray([s["points3D"] for s in sc])


ALL_300 = tuple(range(300))
GPU_SUBSET = tuple((k * 75) // 16 for k in range(64))  # 64 of the 300, evenly over the three models
GOLDEN_YARDSTICK = os.path.join(HERE, "golden", "p3p_yardstick_64.npz")


def golden_yardstick():
    """hypothesis_yardstick(GPU_SUBSET) as recorded (the 50-digit evaluation of 64 inputs and their 8 copies takes twelve
    seconds; test_hypothesis_against_50_digits checks the record against a fresh evaluation)."""
    g = np.load(GOLDEN_YARDSTICK)
    return [int(i) for i in g["idx"]], g["M50"], g["e_ref"], g["keep"].astype(bool)


def _model_error(M, M50):
    return float(np.abs(np.asarray(M, float) - M50).max())


@functools.lru_cache(maxsize=None)
def hypothesis_yardstick(indices=ALL_300):
    """Per input of `indices`: the 50-digit model M50 [12], e_ref, and whether the input meets the preconditions
    (checked on the 50-digit evaluation and the restatement alone)."""
    x2d, X = hypothesis_inputs()
    idx = list(indices)
    M50, e_ref, keep = np.full((len(idx), 12), np.nan), np.full(len(idx), np.inf), np.zeros(len(idx), bool)
    for j, i in enumerate(idx):
        hi = mp_p3p(x2d[i], X[i])
        if hi["model"] is None:
            continue
        M50[j] = hi["model"]
        ok = all(abs(float(im)) < 1e-30 or abs(float(im)) > 1e-6 for _, im in hi["roots"])
        ok &= all(float(x) > 1e-6 for _, x, _ in hi["cands"])
        errs = sorted(float(e) for e, _, _ in hi["cands"])
        ok &= len(errs) == 1 or errs[1] - errs[0] > 1e-6 * errs[1]
        lo = ref_p3p(x2d[i], X[i])
        ok &= lo["model"] is not None
        if not ok:
            continue
        e = _model_error(lo["model"], M50[j])
        rng = np.random.default_rng([HYP_SEED, i])
        for _ in range(8):
            xp = x2d[i] * (1 + rng.choice([-1.0, 1.0], x2d[i].shape) * 2.0 ** -52)
            Xp = X[i] * (1 + rng.choice([-1.0, 1.0], X[i].shape) * 2.0 ** -52)
            lo_p, hi_p = ref_p3p(xp, Xp), mp_p3p(xp, Xp)
            if lo_p["model"] is None or hi_p["model"] is None:
                e = np.inf
                break
            e = max(e, _model_error(lo_p["model"], hi_p["model"]))
        e_ref[j] = e
        keep[j] = e < 1e-6
    return idx, M50, e_ref, keep


def host_models(x2d, X):
    m = len(x2d)
    M, valid = np.zeros((m, 12)), np.zeros(m, np.uint8)
    load_host().hp_estimate(m, d(np.ascontiguousarray(x2d)), d(np.ascontiguousarray(X)), d(M), valid.ctypes.data_as(C.POINTER(C.c_uint8)))
    return M, valid.astype(bool)


def check_hypotheses(M, idx, M50, e_ref, keep, what=""):
    """The bound of the hypothesis test on the models M [len(idx), 12] of the inputs idx. Returns max e / e_ref."""
    assert np.count_nonzero(~keep) <= 0.05 * len(keep), (what, "left out", np.count_nonzero(~keep), len(keep))
    worst = 0.0
    for j in np.flatnonzero(keep):
        e = _model_error(M[j], M50[j])
        worst = max(worst, e / e_ref[j])
        assert np.isfinite(M[j]).all() and e <= P3P_K * e_ref[j], (what, idx[j], e, e_ref[j])
        assert e <= 1e-6, (what, idx[j], e)  # the same root as at 50 digits
    print(f"{what} hypothesis: max e / e_ref = {worst:.4g} (allowed {P3P_K}); left out {np.count_nonzero(~keep)} of {len(keep)}")
    return worst


# ---------------------------------------------------------------------------------------------------------------------
# tests
# ---------------------------------------------------------------------------------------------------------------------
def test_generator_equals_its_restatement(host):
    for n in (5, 6, 64, 1000, 2 ** 31 - 1):
        seed = 0x123456789ABCDEF0 + n
        rows = np.zeros((500, 4), np.int32)
        host.hp_draw_samples(seed, n, 500, rows.ctypes.data_as(C.POINTER(C.c_int32)))
        assert rows.tolist() == [py_sample(seed, t, n) for t in range(500)], n
        assert np.all(rows >= 0) and np.all(rows < n) and np.all(np.diff(rows, axis=1) > 0), n
        if n == 5:
            left_out = {(set(range(5)) - set(r)).pop() for r in rows.tolist()}
            assert left_out == set(range(5))


def test_hypothesis_against_50_digits(host):
    """e_host <= P3P_K e_ref on the 300 inputs (see P3P_K above), preconditions on the 50-digit evaluation and the
    restatement alone.

    Measured on these 300 inputs (HYP_SEED = 2):
      left out by the preconditions     3 of 300 = 1 % (at most 5 % allowed, asserted)
      host build   max e_host / e_ref   1.4405   -> P3P_MEASURED_MAX = 1.441, P3P_K = 8 x 1.441 = 11.53
      device build max e_gpu / e_ref    1.237 on the 64 inputs of tests/test_gpu_absolute_pose.py, bit-equal to the host build there
    (medians: e_ref 3.3e-11, e_host / e_ref 0.32.) The device build evaluates the hypothesis without fused multiply-adds,
    operation for operation as the host build does."""
    x2d, X = hypothesis_inputs()
    idx, M50, e_ref, keep = hypothesis_yardstick()
    M, valid = host_models(x2d, X)
    assert valid[keep].all()
    worst = check_hypotheses(M, idx, M50, e_ref, keep, "host")
    assert worst <= P3P_MEASURED_MAX  # the figure P3P_K was formed from still holds
    check_models(M, "host hypotheses")
    # the record the GPU test reads is this evaluation
    gi, gM, ge, gk = golden_yardstick()
    sub = list(GPU_SUBSET)
    assert gi == sub and np.array_equal(gM[gk], M50[sub][gk]) and np.array_equal(gk, keep[sub])
    assert np.allclose(ge[gk], e_ref[sub][gk], rtol=1e-3, atol=0)


CASES = [(n, mt, stop, supplied) for n in (5, 65, 257) for mt in (1, 3, 64, 500) for stop in (None, 0.8, 1.0) for supplied in (False, True)]


@functools.lru_cache(maxsize=None)
def case_item(n, mt, stop, supplied):
    model = {5: A.MODEL_PINHOLE, 65: A.MODEL_OPENCV, 257: A.MODEL_CATA}[n]
    return make_item(n, model, seed=3, max_trials=mt, stop_frac=stop, supplied=supplied)


def test_scoring_and_selection(host):
    """Counts exactly, sums at 1e-12, then the reference's selection replayed on the implementation's own counts and
    sums: best_trial, trials_used, num_inliers, the mask and the model, for every case of the issue's grid."""
    items = [case_item(*c) for c in CASES]
    recs = host_run(items)
    ties = limited = stopped = 0
    for c, it, rec in zip(CASES, items, recs):
        rp = check_record(rec, it, what=str(c))
        ties += rp["tie_decided"]
        limited += it["stop_num_inliers"] == 0 and rp["trials_used"] < it["max_trials"]
        stopped += it["stop_num_inliers"] > 0 and rp["trials_used"] < it["max_trials"] and rp["num_inliers"] >= it["stop_num_inliers"]
    # what the cases were built to show does happen
    assert ties > 0 and limited > 0 and stopped > 0, (ties, limited, stopped)


def test_a_tie_on_the_count_is_decided_by_the_sum_and_the_dynamic_limit_ends_the_run(host):
    it = case_item(65, 500, None, True)
    rec = host_run([it])[0]
    rp = check_record(rec, it, "tie")
    c, s = rec["trial_num_inliers"], rec["trial_residual_sum"]
    b = rec["best_trial"]
    earlier = [t for t in range(b) if c[t] == c[b]]
    assert earlier and all(s[b] < s[t] for t in earlier) and rp["tie_decided"]   # the same count earlier, the smaller sum won
    lim = py_limit(int(c[rec["trials_used"] - 1]), 65, it["probability"])
    assert rec["trials_used"] < 500 and lim is not None and rec["trials_used"] - 1 >= lim  # ended by THIS trial's count
    assert all(py_limit(int(c[t]), 65, it["probability"]) is None or t < py_limit(int(c[t]), 65, it["probability"])
               for t in range(rec["trials_used"] - 1))
    # the table of the host build is the one of Python's libm
    assert [host.hp_dynamic_limit(k, 65, 0.99) for k in range(66)] == [2 ** 31 - 1 if py_limit(k, 65, 0.99) is None else py_limit(k, 65, 0.99) for k in range(66)]


def _unit_item(uv, xyz, **kw):
    """A pinhole camera with unit focal length and zero principal point: pixels ARE normalised coordinates."""
    it = dict(camera_params=np.array([1.0, 1.0, 0.0, 0.0, float(A.MODEL_PINHOLE)]), points2D=np.array(uv, float).reshape(-1, 2),
              points3D=np.array(xyz, float).reshape(-1, 3), max_trials=8, max_reproj_error=0.01, probability=0.99, seed=5, stop_num_inliers=0)
    it.update(kw)
    return it


def degenerate_items():
    rng = np.random.default_rng(11)
    X = np.stack([rng.uniform(-2, 2, 6), rng.uniform(-2, 2, 6), rng.uniform(4, 9, 6)], axis=1)
    uv = X[:, :2] / X[:, 2:]
    line = np.stack([np.linspace(-2, 2, 6), np.linspace(-1, 1, 6) * 0.5, np.linspace(4, 8, 6)], axis=1)
    out = {}
    out["collinear"] = _unit_item(line[:, :2] / line[:, 2:], line)
    twin = X.copy()
    twin[1] = twin[0]
    out["two_identical"] = _unit_item(uv, twin, samples=np.array([[0, 1, 2, 3]] * 8, np.int32))
    behind = X.copy()
    behind[5, 2] = -6.0
    out["D_behind"] = _unit_item(uv, behind, samples=np.array([[0, 1, 2, 5]] * 8, np.int32))
    out["all_identical"] = _unit_item(np.tile(uv[0], (6, 1)), np.tile(X[0], (6, 1)))
    out["n4"] = _unit_item(uv[:4], X[:4])
    out["n0"] = _unit_item(np.zeros((0, 2)), np.zeros((0, 3)))
    out["no_trials"] = _unit_item(uv, X, max_trials=0)
    out["nan_input"] = _unit_item(np.where(np.arange(6)[:, None] == 2, np.nan, uv), X)
    return out


def check_degenerate(recs):
    """recs: name -> record of degenerate_items(). Every input terminated (we are here); none has a NaN model marked valid."""
    items = degenerate_items()
    for name, rec in recs.items():
        it = items[name]
        n, mt = len(it["points2D"]), it["max_trials"]
        M = rec["trial_models"].reshape(mt, 12)
        valid = np.isfinite(M).all(axis=1)
        assert np.all(np.isnan(M[~valid])) and np.all(rec["trial_num_inliers"][~valid] == 0) and np.all(rec["trial_residual_sum"][~valid] == 0), name
        if n <= 4 or mt == 0:
            assert rec["status"] == A.ABSPOSE_NO_CONSENSUS and rec["trials_used"] == 0 and rec["best_trial"] == -1 and rec["num_inliers"] == 0, name
            assert not valid.any() and np.all(rec["trial_samples"] == -1) and np.isnan(rec["rvec"]).all() and np.isnan(rec["proj_matrix"]).all(), name
            continue
        check_record(rec, it, name)
    assert not np.isfinite(recs["two_identical"]["trial_models"]).any() and recs["two_identical"]["status"] == A.ABSPOSE_NO_CONSENSUS
    assert not np.isfinite(recs["all_identical"]["trial_models"]).any() and recs["all_identical"]["status"] == A.ABSPOSE_NO_CONSENSUS
    assert recs["D_behind"]["num_inliers"] < 6


def test_degenerate_inputs_terminate_and_classify(host):
    items = degenerate_items()
    check_degenerate(dict(zip(items, host_run(list(items.values())))))


# ---------------------------------------------------------------------------------------------------------------------
# C ABI without a device
# ---------------------------------------------------------------------------------------------------------------------
LAYOUT_FIELDS = ("camera_model", "n", "max_trials", "stop_num_inliers", "samples", "seed", "inlier_mask", "trial_samples", "rvec", "proj_matrix",
                 "num_inliers", "status", "kernel_seconds")


def test_item_layout_matches_the_header():
    fields = ", ".join(f"offsetof(mavba_abspose_item, {f})" for f in LAYOUT_FIELDS)
    src = r"""
#include <stdio.h>
#include <stddef.h>
#include "mavba_absolute_pose.h"
int main(void) {
  size_t v[] = {sizeof(mavba_abspose_item), %s};
  for (size_t i = 0; i < sizeof(v) / sizeof(v[0]); ++i) printf("%%zu ", v[i]);
  printf("%%d %%d\n", MAVBA_ABSPOSE_OK, MAVBA_ABSPOSE_NO_CONSENSUS);
  return 0;
}""" % fields
    with tempfile.TemporaryDirectory() as td:
        open(os.path.join(td, "t.c"), "w").write(src)
        exe = os.path.join(td, "t")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(td, "t.c"), "-o", exe])
        out = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    assert out[:-2] == [C.sizeof(A.CAbsPoseItem)] + [getattr(A.CAbsPoseItem, f).offset for f in LAYOUT_FIELDS]
    assert out[-2:] == [A.ABSPOSE_OK, A.ABSPOSE_NO_CONSENSUS]
    assert len(A.CAbsPoseItem._fields_) == 24


def _untouched(arr, outs, q=0, fill=-7):
    return (all(np.all(o == (fill % 256 if o.dtype == np.uint8 else fill)) for o in outs[q].values()) and arr[q].num_inliers == fill
            and arr[q].status == fill and arr[q].rvec[0] == fill and arr[q].kernel_seconds == fill)


def test_abi_without_a_device(mavba):
    from mavmap_amd import api
    L = mavba.load()
    header = open(os.path.join(ROOT, "include", "mavba_absolute_pose.h")).read()
    assert "The result is that of the reference's RANSAC() run on one thread with the same samples." in header
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = sorted(set(re.findall(r"\b(mavba_[a-z0-9_]+)\s*\(", header)))
    assert declared == sorted(api.ABSPOSE_SYMBOLS) == ["mavba_absolute_pose_ransac"]
    assert all(hasattr(L, name) for name in declared)
    assert not set(declared) & set(api.EXPORTED_SYMBOLS) and not set(declared) & set(api.TRIANGULATE_SYMBOLS)
    assert mavba.absolute_pose_ransac([]) == []
    assert L.mavba_absolute_pose_ransac(0, None, -1) == A.OK
    item = make_item(65, A.MODEL_OPENCV, seed=1, max_trials=20, supplied=True)
    # invalid arguments give their codes on any machine, and leave every output as it was
    assert L.mavba_absolute_pose_ransac(-1, None, -1) == A.ERR_INVALID_ARGUMENT
    assert L.mavba_absolute_pose_ransac(1, None, -1) == A.ERR_INVALID_ARGUMENT
    null = object()
    for field, value, code in (("n", -1, A.ERR_INVALID_ARGUMENT), ("n", 2 ** 31, A.ERR_INVALID_ARGUMENT), ("max_trials", -1, A.ERR_INVALID_ARGUMENT),
                               ("uv", null, A.ERR_INVALID_ARGUMENT), ("xyz", null, A.ERR_INVALID_ARGUMENT), ("intrinsics", null, A.ERR_INVALID_ARGUMENT),
                               ("camera_model", 0, A.ERR_BAD_MODEL), ("camera_model", 4, A.ERR_BAD_MODEL)):
        arr, outs, hold = c_items([item], fill=-7)
        setattr(arr[0], field, C.cast(None, dp) if value is null else value)
        assert L.mavba_absolute_pose_ransac(1, arr, -1) == code, field
        assert _untouched(arr, outs), field
    for bad_row in ([3, 9, 3, 1], [0, 1, 2, 65], [-1, 1, 2, 3]):
        bad = dict(item, samples=item["samples"].copy())
        bad["samples"][7] = bad_row
        arr, outs, hold = c_items([item, bad], fill=-7)   # (the second item is the bad one: the first is not written either)
        assert L.mavba_absolute_pose_ransac(2, arr, -1) == A.ERR_INVALID_ARGUMENT, bad_row
        assert _untouched(arr, outs, 0) and _untouched(arr, outs, 1), bad_row
    arr, outs, hold = c_items([_unit_item(np.zeros((0, 2)), np.zeros((0, 3)))], outputs=())
    for field in ("intrinsics", "uv", "xyz"):
        setattr(arr[0], field, C.cast(None, dp))  # an empty item may leave every pointer NULL
    assert L.mavba_absolute_pose_ransac(1, arr, -1) in (A.OK, A.ERR_NO_DEVICE)
    if mavba.device_count() > 0:
        assert arr[0].status == A.ABSPOSE_NO_CONSENSUS and arr[0].trials_used == 0
        return  # (the rest is what a machine without a GPU answers)
    arr, outs, hold = c_items([item], fill=-7)
    assert L.mavba_absolute_pose_ransac(1, arr, -1) == A.ERR_NO_DEVICE
    assert _untouched(arr, outs)
    with pytest.raises(mavba.MavbaError) as ei:
        mavba.absolute_pose_ransac([item])
    assert ei.value.code == A.ERR_NO_DEVICE and "no CPU path" in str(ei.value)
    assert mavba.to_pose_refine_items([], []) == []


if __name__ == "__main__":  # python -m tests.test_absolute_pose_host: writes the record of golden_yardstick() afresh
    i_, M_, e_, k_ = hypothesis_yardstick(GPU_SUBSET)
    np.savez(GOLDEN_YARDSTICK, idx=np.array(i_, np.int32), M50=M_, e_ref=e_, keep=k_)
    print("wrote", GOLDEN_YARDSTICK, "left out", int(np.count_nonzero(~k_)), "of", len(k_))
