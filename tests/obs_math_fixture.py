"""Loader of tests/golden/obs_math_hp.npz and the bars its users share (tests/test_hp_reference.py on the host build,
tests/test_gpu_obs_math.py on the device build). numpy only: the GPU tests must not need mpmath."""
import os

import numpy as np

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "obs_math_hp.npz")
FAMILIES = {1: "benign", 2: "tiny rotation", 3: "large rotation", 4: "depth", 5: "outliers", 6: "far frame", 7: "catadioptric",
            8: "distortion"}
# blocks of a composed reference row: r[2], Jc[12], Jp[6], Jk[18], t[3]
BLOCKS = dict(r=slice(0, 2), Jc=slice(2, 14), Jp=slice(14, 20), Jk=slice(20, 38), t=slice(38, 41))
COMPOSED_BAR = 1e-11  # the project's single-evaluation bar, times the case's amplification factor obs_cin

_cache = None


def load():
    global _cache
    if _cache is None:
        with np.load(PATH) as z:
            _cache = {k: z[k] for k in z.files}
        for a in _cache.values():
            a.setflags(write=False)
    return _cache


def ulp_error(got, hi, lo):
    """|got - exact| in ulps of the correctly rounded result hi; exact = hi + lo ulp(hi). got - hi is exact in double
    arithmetic wherever got is within a factor 2 of hi, and where it is not the error is huge either way."""
    got, hi = np.asarray(got, float), np.asarray(hi, float)
    u = np.spacing(np.abs(hi))
    with np.errstate(invalid="ignore", over="ignore"):
        return np.abs((got - hi) / u - np.asarray(lo, float))


def classify(x):
    """'nan', '+inf', '-inf', '0' or 'finite' per element."""
    x = np.asarray(x, float)
    return np.where(np.isnan(x), "nan", np.where(np.isposinf(x), "+inf", np.where(np.isneginf(x), "-inf", np.where(x == 0.0, "0", "finite"))))


def special_violations(x, got, hi, lo, bar_ulp):
    """Inputs at which `got` is a FINITE WRONG value: finite although the exact value is not, or finite and further than
    the bar from it. A non-finite result is always acceptable there."""
    bad = []
    for i in range(len(x)):
        if not np.isfinite(got[i]):
            continue
        if not np.isfinite(hi[i]):
            bad.append((float(x[i]), float(got[i]), float(hi[i])))
        elif hi[i] == 0.0:
            if got[i] != 0.0:
                bad.append((float(x[i]), float(got[i]), 0.0))
        elif not ulp_error(got[i], hi[i], lo[i]) <= bar_ulp:
            bad.append((float(x[i]), float(got[i]), float(hi[i])))
    return bad


def rot_bars(th2, ref_a, ref_b):
    """1e-14 relative on each of a, b, c, except where a coefficient passes through a zero: a = sin th / th at every
    multiple of pi and b = (1 - cos th) / th^2 at every multiple of 2 pi; there 1e-14 absolute. 'There' is |sin th| < 0.1
    (and 1 - cos th < 0.01 for b): outside it the rounding of th = sqrt(th2), amplified by th |cot th| <= 70 for
    th <= 7, stays below 8e-15 of a. c = (th - sin th) / th^3 has no zero and keeps the relative bar everywhere."""
    th = np.sqrt(th2)
    near_a = (th > 1.0) & (np.abs(np.sin(th)) < 0.1)
    near_b = (th > 1.0) & (1.0 - np.cos(th) < 0.01)
    return 1e-14 * np.where(near_a, 1.0, np.abs(ref_a)), 1e-14 * np.where(near_b, 1.0, np.abs(ref_b))


def composed_errors(got, ref, blocks):
    """{block: [n] max-norm error of the block relative to the reference block's own maximum (conftest.rel_err per case)}.
    Rows whose reference is NaN come out as NaN."""
    out = {}
    for b in blocks:
        g, r = got[:, BLOCKS[b]], ref[:, BLOCKS[b]]
        with np.errstate(invalid="ignore"):
            out[b] = np.abs(g - r).max(1) / np.maximum(np.abs(r).max(1), 1e-300)
    return out


def composed_failures(got, ref, cin, family, blocks, where=None):
    """(list of failing (case, family, block, error, bar), {family: {block: max error / amplification}})."""
    fin = np.isfinite(ref).all(1)
    errs = composed_errors(got, ref, blocks)
    bad, worst = [], {}
    for i in range(len(ref)):
        if where is not None and not where[i]:
            continue
        if not fin[i]:  # the projection's denominator is zero: nothing finite may come out for the residual
            if np.isfinite(got[i, BLOCKS["r"]]).any():
                bad.append((i, int(family[i]), "r", "finite", "non-finite"))
            continue
        for b in blocks:
            e, bar = errs[b][i], COMPOSED_BAR * cin[i]
            w = worst.setdefault(int(family[i]), {})
            w[b] = max(w.get(b, 0.0), float(e / cin[i]) if np.isfinite(e) else np.inf)
            if not e <= bar:
                bad.append((i, int(family[i]), b, float(e), float(bar)))
    return bad, worst


STRESS_FAMILIES = (2, 3, 4, 5, 6, 7, 8)
STRESS_BLOCKS = dict(r=slice(0, 2), Jc=slice(2, 14), Jp=slice(14, 20), Jk=slice(20, 38))


def stress_problem(family):
    """The hand-built BAProblem of a family (fresh arrays: a solve writes into them)."""
    from mavmap_amd.problem import BAProblem
    z = load()
    g = lambda k: z["stress%d_%s" % (family, k)].copy()
    return BAProblem(poses=g("poses"), pose_const=g("pose_const"), image_camera=g("image_camera"), intrinsics=g("intrinsics"),
                     camera_model=g("camera_model"), intr_const=np.zeros(3, np.uint8), points=g("points"),
                     point_const=np.zeros(len(g("points")), np.uint8), obs_uv=g("obs_uv"), obs_image=g("obs_image"),
                     obs_point=g("obs_point"))


def stress_failures(family, r, Jc, Jp, Jk):
    """Per-observation blocks of an evaluation against the fixture, at the composed bar: (failures, {block: worst error / c_in})."""
    z = load()
    n = len(r)
    got = np.concatenate([np.reshape(r, (n, 2)), np.reshape(Jc, (n, 12)), np.reshape(Jp, (n, 6)), np.reshape(Jk, (n, 18))], 1)
    ref, cin = z["stress%d_ref" % family], z["stress%d_cin" % family]
    bad, worst = [], {}
    for b, sl in STRESS_BLOCKS.items():
        e = np.abs(got[:, sl] - ref[:, sl]).max(1) / np.maximum(np.abs(ref[:, sl]).max(1), 1e-300)
        worst[b] = float((e / cin).max())
        bad += [(int(o), b, float(e[o]), float(COMPOSED_BAR * cin[o])) for o in np.nonzero(~(e <= COMPOSED_BAR * cin))[0]]
    return bad, worst
