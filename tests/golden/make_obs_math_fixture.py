"""Generator of tests/golden/obs_math_hp.npz: inputs and 60-digit reference outputs of the per-observation functions of
csrc/ba_math.h (tests/hp_reference.py, mpmath), for tests/test_gpu_obs_math.py and tests/test_hp_reference.py.

Deterministic (fixed seeds; the inputs are built in double precision, the reference reads those doubles exactly), so
tests/test_hp_reference.py can regenerate every array and compare it with the committed file. The GPU tests read the file
and never import mpmath. Run as  python -m tests.golden.make_obs_math_fixture  from the repository root.

Layout (the scalar grids hold about 4 000 arguments each, so that the file stays under 1 MB). Scalar functions (rcp, rsqrt, log; rot_coeffs; cauchy_weight): `<name>_x` inputs, `<name>_hi` the correctly rounded
result, `<name>_lo` (float32) the remainder in ulps of hi, so the pair is good to about 1e-7 ulp. `<name>_special_*`: the inputs without an ulp
bar. Composed cases (kinds 5-7 of mavba_debug_obs_math): `obs_in` [n, 36] = model, pose[6], cam[9], X[3], uv[2], dc[6], dk[9];
`obs_ref` [n, 41] = r[2], Jc[12], Jp[6], Jk[18], t[3] (nearest doubles; NaN where the projection's denominator is zero);
`obs_family` [n] 1..8; `obs_cin` [n] the amplification factor the bar is scaled with. Stress problems (one per family 2-8,
for the production kernels): `stress<f>_<field of BAProblem>`, `stress<f>_ref` [num_obs, 38] the loss-corrected r, Jc, Jp, Jk,
`stress<f>_cin`, `stress<f>_cost`. Pose refinement: `pose_start` [4, 6], `pose_cam` [4, 10] (model code last), `pose_uv`,
`pose_xyz`, `pose_Rtrue` [4, 3, 3] (pose_items)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "obs_math_hp.npz")

FAMILIES = {1: "benign", 2: "tiny rotation", 3: "large rotation", 4: "depth", 5: "outliers", 6: "far frame", 7: "catadioptric",
            8: "distortion"}
# families in which the oracle's obs_jacobian is expected to meet the bar (tests/test_hp_reference.py checks the pattern):
# every one but the tiny non-zero rotations, where the formula it differentiates loses digits in d / d rvec
ORACLE_OK = [1, 3, 4, 5, 6, 7, 8]
K_OF = {1: 4, 2: 8, 3: 9}


# ---- scalar grids ---------------------------------------------------------------------------------------------------------

def _pow2(exps):
    out = []
    for e in exps:
        x = 2.0 ** e
        out += [np.nextafter(x, 0.0), x, np.nextafter(x, np.inf)]
    return out


def _mantissas(exps):
    lo, hi = 1.0 + 2.0 ** -52, 2.0 - 2.0 ** -52
    return [m * 2.0 ** e for e in exps for m in (lo, hi)]


def rcp_grid():
    rng = np.random.default_rng(9501)
    pos = np.array(_pow2(range(-498, 499, 7)) + _mantissas(range(-498, 498, 7)))
    rnd = 10.0 ** rng.uniform(-150, 150, 2600) * rng.choice([-1.0, 1.0], 2600)
    return np.concatenate([pos, -pos, rnd])


def rsqrt_grid():
    rng = np.random.default_rng(9502)
    edge = np.array(_pow2(range(-498, 997, 5)) + _mantissas(range(-498, 996, 5)))
    return np.concatenate([edge, 10.0 ** rng.uniform(0, 300, 1400), 10.0 ** rng.uniform(-150, 0, 1200)])


def log_grid():
    rng = np.random.default_rng(9503)
    edge = [x for x in _pow2(range(0, 997, 4)) if x >= 1.0] + _mantissas(range(0, 996, 4))
    fold = []
    for m in (2.0 ** 0.5, 0.5 ** 0.5 * 2.0):  # either side of the series' fold m < sqrt(1/2)
        for e in (0, 1, 10, 100, 900):
            x = m * 2.0 ** e
            fold += [np.nextafter(x, 0.0), x, np.nextafter(x, np.inf)]
    low = 1.0 + 10.0 ** rng.uniform(-16, 0, 1500)  # the low end of the Cauchy argument 1 + s / b
    return np.concatenate([[1.0, 1.0 + 2.0 ** -52], edge, fold, low, 10.0 ** rng.uniform(0, 300, 1300)])


SPECIALS = dict(
    rcp=[0.0, -0.0, 5e-324, -5e-324, 1e-310, -1e-310, 1e300, -1e300, 1e-300, -1e-300, np.inf, -np.inf, np.nan],
    rsqrt=[0.0, -0.0, 5e-324, 1e-310, 1e300, 1e-300, np.inf, np.nan, -1e-310, -1.0, -1e300, -np.inf],
    log=[0.0, -0.0, 5e-324, 1e-310, 1e300, 1e-300, np.inf, np.nan, -1e-310, -1.0, -1e300, -np.inf])


def _scalar_ref(name, x, H):
    """The exact value of the function at a double as an mpmath number, or a float inf / nan where it has none."""
    mp = H.mp
    if x != x:
        return float("nan")
    if name == "rcp":
        if x == 0.0:
            return float(np.copysign(np.inf, x))
        return 0.0 if np.isinf(x) else 1 / H.mpf(x)
    if x < 0.0:
        return float("nan")
    if x == 0.0:
        return float("inf") if name == "rsqrt" else float("-inf")
    if np.isinf(x):
        return 0.0 if name == "rsqrt" else float("inf")
    return 1 / mp.sqrt(H.mpf(x)) if name == "rsqrt" else mp.log(H.mpf(x))


def _dd_arrays(vals, H):
    hi, lo = np.zeros(len(vals)), np.zeros(len(vals), np.float32)
    for i, v in enumerate(vals):
        h, l = H.dd(v) if isinstance(v, H.mpf) else (float(v), 0.0)
        hi[i], lo[i] = h, (l / np.spacing(abs(h)) if l != 0.0 else 0.0)
    return hi, lo


def rot_grid():
    rng = np.random.default_rng(9504)
    t = 1e-6
    fixed = [0.0, 1e-300, 1e-24, 1e-12, np.nextafter(t, 0.0), t, np.nextafter(t, 1.0), 1e-5, 1.0, np.pi ** 2, (np.pi + 0.5) ** 2,
             (2 * np.pi) ** 2, 49.0, 1e4]
    # the switch between series and closed form (0.25) with its neighbours, like the 1e-6 it replaced
    fixed += [np.nextafter(0.25, 0.0), 0.25, np.nextafter(0.25, 1.0)]
    # random: angles up to 7 (the largest of the large-rotation family): above it the rounding of sqrt(th2) alone, amplified
    # by th cot th, passes 1e-14 at generic angles; half log-uniform in th2 down to 1e-16, half uniform in th
    rnd = np.concatenate([10.0 ** rng.uniform(-16, np.log10(49.0), 1000), rng.uniform(0.0, 7.0, 1000) ** 2])
    return np.concatenate([fixed, rnd])


def cauchy_grid():
    rng = np.random.default_rng(9505)
    rows = []
    for b in (0.01, 1.0, 9.0, 1e4):
        s = np.concatenate([[0.0, 1e14], 10.0 ** rng.uniform(-20, 14, 380), rng.uniform(0, 100, 20)])
        rows += [(x, b) for x in s]
    # the outlier family's residuals of 1e3, 1e5, 1e7 px, at loss scales a = 1 and a = 0.1
    rows += [(r * r, a * a) for r in (1e3, 1e5, 1e7) for a in (1.0, 0.1)]
    return np.array(rows)


# ---- composed cases ------------------------------------------------------------------------------------------------------

def _R(w):
    """Rotation matrix in double precision (only to place a point: the reference reads the resulting doubles)."""
    th = np.linalg.norm(w)
    if th == 0.0:
        return np.eye(3)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def _direction(rng):
    d = rng.normal(size=3)
    return d / np.linalg.norm(d)


def _cam(rng, model):
    cam = np.zeros(9)
    cam[:4] = [600 + rng.normal(), 610 + rng.normal(), 376, 240]
    if K_OF[model] >= 8:
        cam[4:8] = np.array([-0.1, 0.02, 1e-3, -1e-3]) * (1 + 0.1 * rng.normal(size=4))
    if K_OF[model] == 9:
        cam[8] = rng.uniform(0, 1)
    return cam


def _place(rvec, t, Xc):
    return _R(rvec).T @ (np.asarray(Xc, float) - t)


def _benign(rng, model, scale):
    """The distribution of tests/test_host_math.py's _case."""
    rvec, t = rng.normal(0, 1, 3) * scale, rng.normal(0, 1, 3)
    Xc = np.array([rng.uniform(-2, 2), rng.uniform(-2, 2), rng.uniform(3, 9)])
    return rvec, t, _place(rvec, t, Xc), _cam(rng, model), rng.normal(300, 50, 2)


def _row(rng, model, rvec, t, X, cam, uv):
    dc = rng.normal(0, 1, 6) * np.array([1e-2, 1e-2, 1e-2, 0.1, 0.1, 0.1])
    dk = np.zeros(9)
    dk[:K_OF[model]] = rng.normal(0, 1, K_OF[model]) * 1e-2
    return np.concatenate([[float(model)], rvec, t, cam, X, uv, dc, dk])


def composed_inputs():
    rng = np.random.default_rng(9506)
    rows, fam = [], []

    def add(f, model, rvec, t, X, cam, uv):
        rows.append(_row(rng, model, np.asarray(rvec, float), np.asarray(t, float), np.asarray(X, float), cam, np.asarray(uv, float)))
        fam.append(f)

    for model in (1, 2, 3):
        for it in range(24):  # 1 benign
            add(1, model, *_benign(rng, model, [1e-3, 0.3, 1.5, 3.1][it % 4]))
        mags = [0.0, 1e-12, 1e-9, 1e-4, 1e-3 * (1 - 1e-9), 1e-3 * (1 + 1e-9), 2e-3]
        for it in range(28):  # 2 tiny rotation
            _, t, _, cam, uv = _benign(rng, model, 1.0)
            rvec = _direction(rng) * mags[it % 7]
            add(2, model, rvec, t, _place(rvec, t, [rng.uniform(-2, 2), rng.uniform(-2, 2), rng.uniform(3, 9)]), cam, uv)
        mags = [np.pi - 1e-3, np.pi - 1e-8, np.pi, np.pi + 0.5, 2 * np.pi - 1e-3, 7.0]
        for it in range(24):  # 3 large rotation (an LM update does not renormalise rvec)
            _, t, _, cam, uv = _benign(rng, model, 1.0)
            rvec = _direction(rng) * mags[it % 6]
            add(3, model, rvec, t, _place(rvec, t, [rng.uniform(-2, 2), rng.uniform(-2, 2), rng.uniform(3, 9)]), cam, uv)
        zs = [-5.0, -0.01, 0.01, 1e-6, 1e3, 1e6]
        for it in range(24):  # 4 depth: rotation about the optical axis and t_z = 0, so that Xc_z = X_z is formed without
            # cancellation (a sum of O(1) terms would leave z = 1e-6 with 1e-10 relative; cancellation is family 6's subject)
            cam = _cam(rng, model)
            rvec, t = np.array([0.0, 0.0, rng.normal()]), np.array([rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5), 0.0])
            Xc = np.array([rng.uniform(0.7, 2) * rng.choice([-1, 1]), rng.uniform(0.7, 2) * rng.choice([-1, 1]), zs[it % 6]])
            if model == 3 and Xc[2] < 0:
                cam[8] = rng.uniform(0.1, 0.3)  # keeps z + xi |Xc| away from zero
            X = _place(rvec, t, Xc)
            X[2] = Xc[2]
            add(4, model, rvec, t, X, cam, rng.normal(300, 50, 2))
        for it in range(21):  # 5 outliers: the observation lies 1e3, 1e5, 1e7 px from the projection
            rvec, t, X, cam, _ = _benign(rng, model, 0.3)
            ang = rng.uniform(0, 2 * np.pi)
            add(5, model, rvec, t, X, cam, np.array([376.0, 240.0]) + [1e3, 1e5, 1e7][it % 3] * np.array([np.cos(ang), np.sin(ang)]))
        for it in range(21):  # 6 far frame: the point and the camera centre shifted together
            rvec, t, X, cam, uv = _benign(rng, model, 0.3)
            d = _direction(rng) * [1e3, 1e5, 1e6][it % 3]
            add(6, model, rvec, t - _R(rvec) @ d, X + d, cam, uv)
    for xi in (0.0, 1e-12, 0.5, 1.0, 2.5):  # 7 catadioptric
        for it in range(26):
            rvec, t, _, cam, uv = _benign(rng, 3, 0.3)
            cam[8] = xi
            kind = it % 3 if xi >= 0.5 else (it % 3) * 2 % 4  # small xi: no point with z < 0 < z + xi |Xc|
            if kind == 0:    # in front
                Xc = np.array([rng.uniform(-2, 2), rng.uniform(-2, 2), rng.uniform(3, 9)])
            elif kind == 1:  # behind the image plane, inside the mirror's field: z < 0 < z + xi |Xc|
                f = rng.uniform(0.1, 0.8) * min(xi, 1.0) if xi <= 1.0 else rng.uniform(0.05, 0.38) * xi
                ang, n = rng.uniform(0, 2 * np.pi), rng.uniform(3, 9)
                Xc = n * np.array([np.sqrt(1 - f * f) * np.cos(ang), np.sqrt(1 - f * f) * np.sin(ang), -f])
            else:            # |Xc| = 1e-3, no translation (a translation of order 1 would only repeat family 6)
                Xc, t = _direction(rng) * 1e-3, np.zeros(3)
                Xc[2] = abs(Xc[2])
            add(7, 3, rvec, t, _place(rvec, t, Xc), cam, uv)
    for model in (2, 3):  # 8 distortion: the normalised radius sweeps [0, 2]
        for it in range(30):
            rvec, t, _, cam, uv = _benign(rng, model, 0.3)
            cam[4:8] = [-0.5, 0.3, 0.01 * (1 if it % 2 else -1), 0.01 * (1 if it % 4 < 2 else -1)]
            if model == 3:
                cam[8] = rng.uniform(0, 0.2)
            rho, ang, z = 2.0 * it / 29.0, rng.uniform(0, 2 * np.pi), rng.uniform(3, 9)
            if model == 3:  # un = x / (z + xi |Xc|): solve the radius of the direction for the wanted normalised one
                q = rho
                for _ in range(60):
                    q = rho * (1 + cam[8] * np.sqrt(1 + q * q))
                rho = q
            add(8, model, rvec, t, _place(rvec, t, z * np.array([rho * np.cos(ang), rho * np.sin(ang), 1.0])), cam, uv)
    # the projection's denominator exactly zero: no rotation, no translation, the point in the camera plane
    for model in (1, 2, 3):
        cam = _cam(rng, model)
        cam[8] = 0.0
        add(4, model, np.zeros(3), np.zeros(3), [1.0, -0.5, 0.0], cam, [300.0, 200.0])
    return np.array(rows), np.array(fam, np.int32)


def composed_reference(rows, H):
    ref, cin = np.full((len(rows), 41), np.nan), np.ones(len(rows))
    for i, q in enumerate(rows):
        model, pose, cam, X, uv = int(q[0]), q[1:7], q[7:16], q[16:19], q[19:21]
        out = H.jacobian(model, pose, cam, X, uv)
        if out is None:
            continue
        r, Jc, Jp, Jk = out
        t = H.backsub_term(Jc, Jp, Jk, q[21:27], q[27:36])
        flat = list(r) + [x for row in Jc for x in row] + [x for row in Jp for x in row] + [x for row in Jk for x in row] + list(t)
        ref[i] = [float(x) for x in flat]
        cin[i] = float(H.amplification(model, pose, cam, X))
    return ref, cin


# ---- stress problems for the production kernels (tests/test_gpu_stress_geometry.py) ----------------------------------------

STRESS_FAMILIES = (2, 3, 4, 5, 6, 7, 8)
STRESS_LOSS_SCALE = 1.0


def _project_np(model, cam, Xc):
    """The projection in double precision (only to place an observation near its projection)."""
    zz = Xc[2] + (cam[8] * np.linalg.norm(Xc) if model == 3 else 0.0)
    un, vn = Xc[0] / zz, Xc[1] / zz
    if model != 1:
        k1, k2, p1, p2 = cam[4:8]
        r2 = un * un + vn * vn
        rad = 1 + k1 * r2 + k2 * r2 * r2
        un, vn = un * rad + 2 * p1 * un * vn + p2 * (r2 + 2 * un * un), vn * rad + p1 * (r2 + 2 * vn * vn) + 2 * p2 * un * vn
    return np.array([cam[0] * un + cam[2], cam[1] * vn + cam[3]])


def stress_problem(family):
    """One tiny problem per family, built by hand (synth.make_scene cannot express these scenes): 5 images - image 0
    constant, image 1 with t_x constant, images 2-4 free and carrying the family's rotations -, 3 cameras with free
    intrinsics (pinhole, OpenCV, catadioptric; family 7: three catadioptric ones), 48 points seen by 3 to 5 images each.
    The points lie around the world origin, the cameras 6 in front of it: Xc = R_i X + t_i, t_i = (b_x, b_y, 6 + b_z)."""
    rng = np.random.default_rng(9600 + family)
    NI, NP = 5, 48
    models = [3, 3, 3] if family == 7 else [1, 2, 3]
    intr = np.array([_cam(rng, m) for m in models])
    jitter = lambda: rng.normal(0, 0.03, 3)
    rvecs = [jitter() for _ in range(NI)]
    tvecs = [np.array([rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5), 6.0 + rng.uniform(-0.3, 0.3)]) for _ in range(NI)]
    pts = np.stack([rng.uniform(-2, 2, NP), rng.uniform(-2, 2, NP), rng.uniform(-3, 3, NP)], 1)
    if family == 2:    # a free image at exactly zero, the others on the series branch down to 1e-12
        for i, m in enumerate([1e-3 * (1 + 1e-9), 1e-12, 0.0, 1e-9, 1e-4]):
            rvecs[i] = _direction(rng) * m
    elif family == 3:  # at and beyond pi: an LM update does not renormalise rvec
        for i, m in enumerate([2 * np.pi - 1e-3, np.pi - 1e-3, np.pi - 1e-8, np.pi + 0.5, 7.0]):
            rvecs[i] = _direction(rng) * m
    elif family == 4:  # depths from behind the camera to 1e6: rotations about the optical axis and coplanar cameras, so that
        # Xc_z = X_z without cancellation (see the composed family 4)
        rvecs = [np.array([0.0, 0.0, rng.normal(0, 0.3)]) for _ in range(NI)]
        tvecs = [np.array([rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), 0.0]) for _ in range(NI)]
        zs = [-5.0, -0.01, 0.01, 1e-6, 1e3, 1e6]
        pts = np.stack([rng.uniform(1, 2, NP) * rng.choice([-1, 1], NP), rng.uniform(1, 2, NP) * rng.choice([-1, 1], NP),
                        [zs[j % 6] for j in range(NP)]], 1)
        intr[2, 8] = 0.2
    elif family == 6:  # the world frame far from the cameras
        # (by 1e3, the smallest of the composed family's shifts: the cost's bar of 1e-11 is not scaled with the
        # amplification, and a shift of 1e5 moves every residual of ~1 px by 1e-9 px through the rounding of X alone)
        d = _direction(rng) * 1e3
        pts = pts + d
        tvecs = [t - _R(w) @ d for w, t in zip(rvecs, tvecs)]
    elif family == 7:  # xi = 0.5, 1, 2.5; a field of view beyond 90 degrees: z < 0 < z + xi |Xc| for part of the points
        intr[:, 8] = [0.5, 1.0, 2.5]
        tvecs = [np.array([rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3)]) for _ in range(NI)]
        ang, az, n = rng.uniform(0.1, np.deg2rad(105), NP), rng.uniform(0, 2 * np.pi, NP), rng.uniform(3, 9, NP)
        pts = np.stack([n * np.sin(ang) * np.cos(az), n * np.sin(ang) * np.sin(az), n * np.cos(ang)], 1)
    elif family == 8:  # strong distortion, normalised radii up to 2
        intr[1:, 4:8] = [[-0.5, 0.3, 0.01, -0.01], [-0.5, 0.3, -0.01, 0.01]]
        intr[2, 8] = 0.1
        rho, az, z = 2.0 * np.arange(NP) / (NP - 1), rng.uniform(0, 2 * np.pi, NP), rng.uniform(4, 8, NP)
        pts = np.stack([z * rho * np.cos(az), z * rho * np.sin(az), z - 6.0], 1)
    poses = np.array([np.concatenate([w, t]) for w, t in zip(rvecs, tvecs)])
    img_cam = np.arange(NI) % 3
    oi, op, uv = [], [], []
    for j in range(NP):
        for i in sorted(rng.choice(NI, size=3 + j % 3, replace=False)):
            Xc = _R(poses[i, :3]) @ pts[j] + poses[i, 3:]
            c = img_cam[i]
            # the observation: 0.5 to 1.5 px from the projection in each coordinate - never closer, so that u - u_obs does not
            # cancel (a third data-dependent subtraction, which the amplification factor does not cover) - and, where the
            # projection lies far outside any image (family 4), an ordinary pixel instead
            z = _project_np(models[c], intr[c], Xc)
            z = z + rng.uniform(0.5, 1.5, 2) * rng.choice([-1, 1], 2) if np.abs(z).max() < 1e4 else rng.normal(300, 50, 2)
            if family == 5 and len(oi) % 3 == 0:  # every third observation an outlier of 1e3, 1e5 or 1e7 px
                a = rng.uniform(0, 2 * np.pi)
                z = z + [1e3, 1e5, 1e7][(len(oi) // 3) % 3] * np.array([np.cos(a), np.sin(a)])
            oi.append(i); op.append(j); uv.append(z)
    return dict(poses=poses, pose_const=np.array([15, 2, 0, 0, 0], np.uint8), image_camera=img_cam.astype(np.int32), intrinsics=intr,
                camera_model=np.array(models, np.int32), points=pts, obs_uv=np.array(uv), obs_image=np.array(oi, np.int32),
                obs_point=np.array(op, np.int32))


def stress_reference(P, H):
    """Loss-corrected r[2], Jc[12], Jp[6], Jk[18] per observation, the amplification factors and the cost."""
    n = len(P["obs_image"])
    ref, cin, cost = np.zeros((n, 38)), np.ones(n), H.mpf(0)
    for o in range(n):
        i, j = P["obs_image"][o], P["obs_point"][o]
        c = P["image_camera"][i]
        model, pose, cam, X = int(P["camera_model"][c]), P["poses"][i], P["intrinsics"][c], P["points"][j]
        r, Jc, Jp, Jk = H.jacobian(model, pose, cam, X, P["obs_uv"][o])
        r, (Jc, Jp, Jk), half_rho = H.corrected(r, (Jc, Jp, Jk), STRESS_LOSS_SCALE)
        cost += half_rho
        ref[o] = [float(x) for x in list(r) + [x for B in (Jc, Jp, Jk) for row in B for x in row]]
        cin[o] = float(H.amplification(model, pose, cam, X))
    return ref, cin, float(cost)


# ---- pose refinement from the rotations' hard places -----------------------------------------------------------------------

def pose_items(H):
    """Four pose-refinement problems with 40 clean correspondences each, starting at rvec = 0 exactly, |rvec| = 1e-9, pi - 1e-8
    and pi + 0.5; the true pose lies about 0.01 rad and 0.05 units away. The observations are the 60-digit projections at the
    true pose rounded to double, so the optimum is the true pose: `pose_Rtrue` is its rotation matrix."""
    rng = np.random.default_rng(9700)
    start, cams, uvs, xyzs, Rs = [], [], [], [], []
    for q, mag in enumerate([0.0, 1e-9, np.pi - 1e-8, np.pi + 0.5]):
        model = [1, 2, 3, 2][q]
        rv0 = _direction(rng) * mag
        t0 = np.array([rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5)])
        rv, t = rv0 + rng.normal(0, 0.01, 3), t0 + rng.normal(0, 0.05, 3)
        cam = _cam(rng, model)
        Xc = np.stack([rng.uniform(-2, 2, 40), rng.uniform(-2, 2, 40), rng.uniform(3, 9, 40)], 1)
        X = np.array([_place(rv, t, x) for x in Xc])
        uv = np.zeros((40, 2))
        for k in range(40):
            _, xc = H.transform(H.vec(np.concatenate([rv, t])), H.vec(X[k]))
            uv[k] = [float(v) for v in H.project(model, H.vec(cam), xc)]
        start.append(np.concatenate([rv0, t0])); cams.append(np.concatenate([cam, [float(model)]])); uvs.append(uv); xyzs.append(X)
        Rs.append(np.array([[float(v) for v in row] for row in H.rotation_matrix(rv)]))
    return dict(pose_start=np.array(start), pose_cam=np.array(cams), pose_uv=np.array(uvs), pose_xyz=np.array(xyzs), pose_Rtrue=np.array(Rs))


def build_all(progress=False):
    sys.path.insert(0, ROOT)
    from tests import hp_reference as H
    say = (lambda *a: print(*a, file=sys.stderr)) if progress else (lambda *a: None)
    out = {}
    for name, grid in (("rcp", rcp_grid()), ("rsqrt", rsqrt_grid()), ("log", log_grid())):
        out[name + "_x"] = grid
        out[name + "_hi"], out[name + "_lo"] = _dd_arrays([_scalar_ref(name, float(x), H) for x in grid], H)
        sp = np.array(SPECIALS[name])
        out[name + "_special_x"] = sp
        out[name + "_special_hi"], out[name + "_special_lo"] = _dd_arrays([_scalar_ref(name, float(x), H) for x in sp], H)
        say(name, len(grid))
    th2 = rot_grid()
    abc = [H.rot_coeffs(float(x)) for x in th2]
    out["rot_x"] = th2
    for k, nm in enumerate("abc"):
        out["rot_%s_hi" % nm], out["rot_%s_lo" % nm] = _dd_arrays([v[k] for v in abc], H)
    sb = cauchy_grid()
    wh = [H.cauchy_b(float(s), float(b)) for s, b in sb]
    out["cauchy_x"] = sb
    out["cauchy_w_hi"], out["cauchy_w_lo"] = _dd_arrays([v[0] for v in wh], H)
    out["cauchy_h_hi"], out["cauchy_h_lo"] = _dd_arrays([v[1] for v in wh], H)
    say("rot", len(th2), "cauchy", len(sb))
    rows, fam = composed_inputs()
    out["obs_in"], out["obs_family"] = rows, fam
    out["obs_ref"], out["obs_cin"] = composed_reference(rows, H)
    out["oracle_ok"] = np.array(ORACLE_OK, np.int32)
    say("composed", len(rows))
    for f in STRESS_FAMILIES:
        P = stress_problem(f)
        for k, a in P.items():
            out["stress%d_%s" % (f, k)] = a
        ref, scin, cost = stress_reference(P, H)
        out["stress%d_ref" % f], out["stress%d_cin" % f], out["stress%d_cost" % f] = ref, scin, np.array(cost)
        assert f in (6, 7) or scin.max() <= 4.0, (f, scin.max())
        say("stress", f, len(ref), "observations, c_in up to %.3g" % scin.max())
    out.update(pose_items(H))
    # what the amplification factor may excuse
    cin = out["obs_cin"]
    wide = np.isin(fam, (6, 7))
    assert cin[~wide].max() <= 4.0, cin[~wide].max()
    assert (cin[wide] > 100.0).sum() * 3 <= wide.sum(), ((cin[wide] > 100.0).sum(), wide.sum())
    return out


def main():
    arrays = build_all(progress=True)
    np.savez_compressed(OUT, **arrays)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
