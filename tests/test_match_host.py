"""Descriptor matching (include/mavba_match.h) without a GPU: the rules of the header restated in numpy, the host build
of mavmap_amd/csrc/match_math.h against that restatement, and the generators and checkers tests/test_gpu_match.py
reuses.

The reference's match_brute_force() (src/base2d/feature.cc:52-102) needs OpenCV, so there is no reference binary: the
checker is restated_match below, rules 1-6 of the header in numpy with every float operation rounded to float32, and
exact_d2, the same distances in float64. flags() names the keypoints where rule 7 lets the library leave rules 1-5.
"""
import ctypes as C
import functools
import os
import subprocess
import tempfile

import numpy as np
import pytest

from mavmap_amd import _abi as A

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
F32 = np.float32
U = 2.0 ** -24  # the unit roundoff of float32


# ---------------------------------------------------------------------------------------------------------------------
# the generator
# ---------------------------------------------------------------------------------------------------------------------
def _unit_rows(x):
    return x / np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-30)


def make_item(n1, n2, dim, seed, max_ratio=0.9, max_distance=-1.0, with_xy=True):
    """One image pair. Unit-norm Gaussian descriptors; 60 % of the smaller side is copied to random places on the other
    side with noise 0.25 / sqrt(dim) per entry and renormalised; every third copy has noise 2 / sqrt(dim) instead, large
    enough that the ratio test drops some of them; every tenth copied keypoint gets a SECOND copy at that level (a
    candidate for the cross-check to remove). Keypoints are uniform in 752 x 480, a copy's keypoint is displaced by at
    most 3 pixels per axis, so max_distance = 40 keeps it."""
    rng = np.random.default_rng([seed, n1, n2, dim])
    d = [_unit_rows(rng.standard_normal((n1, dim))), _unit_rows(rng.standard_normal((n2, dim)))]
    xy = [rng.uniform(0, 1, (n1, 2)) * [752.0, 480.0], rng.uniform(0, 1, (n2, 2)) * [752.0, 480.0]]
    s, o = (0, 1) if n1 <= n2 else (1, 0)
    ns, no = (n1, n2)[s], (n1, n2)[o]
    k = int(0.6 * ns)
    src = rng.permutation(ns)[:k]
    extra = src[::10][:max(no - k, 0)]
    dst = rng.permutation(no)[:k + len(extra)]
    for c, (a, b) in enumerate(zip(np.concatenate([src, extra]), dst)):
        sigma = (2.0 if c % 3 == 2 or c >= k else 0.25) / np.sqrt(dim)
        d[o][b] = _unit_rows((d[s][a] + sigma * rng.standard_normal(dim))[None])[0]
        xy[o][b] = xy[s][a] + rng.uniform(-3, 3, 2)
    item = dict(descriptors1=d[0].astype(F32), descriptors2=d[1].astype(F32), max_ratio=max_ratio, max_distance=max_distance)
    if with_xy:
        item.update(keypoints1=xy[0].astype(F32), keypoints2=xy[1].astype(F32))
    return item


SIZES = (2, 3, 15, 16, 17, 63, 64, 65, 257)  # the edges of a 16-wide matrix tile and of a wave, one size above a 256 stride
DIMS = (4, 60, 64, 128)
PAIRS = [(2, 2), (2, 3), (3, 2), (3, 15), (15, 16), (16, 16), (16, 17), (17, 17), (17, 65), (65, 17), (63, 64), (64, 63), (64, 64),
         (64, 65), (65, 65), (63, 2), (16, 257), (257, 3), (257, 64), (65, 257)]
# (n1, n2, dim, max_distance): every pair at two dims without and one with the mask, every dim at (17, 65) and (65, 65),
# and the largest item
GRID = []
for _c, (_a, _b) in enumerate(PAIRS):
    GRID += [(_a, _b, DIMS[_c % 4], -1.0), (_a, _b, DIMS[(_c + 1) % 4], 40.0), (_a, _b, DIMS[(_c + 2) % 4], -1.0)]
GRID += [(_a, _b, _d, _m) for (_a, _b) in ((17, 65), (65, 65)) for _d in DIMS for _m in (-1.0, 40.0)]
GRID += [(257, 257, 128, -1.0), (257, 257, 128, 40.0), (257, 257, 64, -1.0)]
GRID = sorted(set(GRID))
assert {n for g in GRID for n in g[:2]} == set(SIZES) and {g[2] for g in GRID} == set(DIMS)
# the seed of a grid item: 1, unless that item then had a flagged keypoint (test_cap_on_the_generated_inputs asserts the result)
GRID_SEEDS = {(63, 64, 64, -1.0): 2}


def grid_item(n1, n2, dim, max_distance):
    return make_item(n1, n2, dim, GRID_SEEDS.get((n1, n2, dim, max_distance), 1), max_distance=max_distance)


def grid_id(g):
    return "%dx%dx%d%s" % (g[0], g[1], g[2], "-masked" if g[3] >= 0 else "")


def integer_item(n1, n2, seed=3):
    """Descriptors of small integers (dim 128, entries in [-8, 8]): all float arithmetic is exact, the screening score
    included. Asymmetric between the images, with repeated rows, and with rows at the SAME distance from a keypoint in
    first, second and third place."""
    rng = np.random.default_rng([seed, n1, n2])
    a = rng.integers(-7, 8, (n1, 128)).astype(np.int64)
    b = rng.integers(-7, 8, (n2, 128)).astype(np.int64)
    b[3] = b[7] = b[11] = a[5]                       # three times distance 0 from a[5]: ties in places 1, 2 and 3
    b[13] = a[2]; b[4] = a[2]; b[4, 0] += 1; b[9] = a[2]; b[9, 77] -= 1   # one exact copy of a[2], then a tie in places 2 and 3
    for r, k in ((1, 5), (6, 40), (14, 127)):       # three rows at squared distance 1 from a[8]: ties in places 1, 2 and 3
        b[r] = a[8]
        b[r, k] += 1
    a[10] = a[12] = b[0]                             # repeated rows in image 1: a tie in direction 2->1
    a[1] = b[2]; a[1, 3] += 1; a[15] = b[2]; a[15, 100] -= 1
    xy = [rng.uniform(0, 400, (n, 2)).astype(F32) for n in (n1, n2)]
    return dict(descriptors1=a.astype(F32), descriptors2=b.astype(F32), keypoints1=xy[0], keypoints2=xy[1], max_ratio=0.9, max_distance=-1.0)


INTEGER_SIZES = ((65, 17), (64, 64))


def near_duplicate_item(n1, n2, dim, seed=5):
    """A third of the smaller side has b = a + a perturbation of length 1e-4 on the other side: the expanded form's
    score there is pure rounding noise and can be negative."""
    it = make_item(n1, n2, dim, seed)
    rng = np.random.default_rng([seed, 77])
    a, b = it["descriptors1"], it["descriptors2"]
    k = min(n1, n2) // 3
    i, j = rng.permutation(n1)[:k], rng.permutation(n2)[:k]
    b[j] = (a[i].astype(float) + 1e-4 * _unit_rows(rng.standard_normal((k, dim)))).astype(F32)
    it["duplicates"] = (i, j)
    return it


NEAR_DUPLICATE_SIZES = ((65, 65, 128, 6), (64, 17, 64, 5), (17, 64, 4, 5))  # (n1, n2, dim, a seed with no flagged keypoint)


# ---------------------------------------------------------------------------------------------------------------------
# the restatement: rules 1-6 of include/mavba_match.h
# ---------------------------------------------------------------------------------------------------------------------
def item_arrays(item):
    d1, d2 = A.as_f32(item["descriptors1"]), A.as_f32(item["descriptors2"])
    xy1 = None if item.get("keypoints1") is None else A.as_f32(item["keypoints1"], (-1, 2))
    xy2 = None if item.get("keypoints2") is None else A.as_f32(item["keypoints2"], (-1, 2))
    return d1, d2, xy1, xy2


def restated_d2(d1, d2):
    """Rule 2: a float32 accumulator over k in order, every operation rounded to float32."""
    acc = np.zeros((len(d1), len(d2)), F32)
    for k in range(d1.shape[1]):
        t = d1[:, k, None] - d2[None, :, k]
        acc = acc + t * t
    assert acc.dtype == F32
    return acc


def restated_mask(item):
    """Rule 1: [n1, n2] bool."""
    d1, d2, xy1, xy2 = item_arrays(item)
    md = float(item.get("max_distance", -1.0))
    if md < 0:
        return np.ones((len(d1), len(d2)), bool)
    x1, x2 = xy1.astype(np.float64), xy2.astype(np.float64)
    dx, dy = x1[:, None, 0] - x2[None, :, 0], x1[:, None, 1] - x2[None, :, 1]
    return dx * dx + dy * dy < md * md


def two_nearest(d2m, mask):
    """Rule 3 for every row: (nn [n, 2] int32, dist [n, 2] float32); candidates by (d2, index), absent: -1 / NaN."""
    n = len(d2m)
    nn, dist = np.full((n, 2), -1, np.int32), np.full((n, 2), np.nan, F32)
    for i in range(n):
        cand = np.flatnonzero(mask[i])
        order = cand[np.argsort(d2m[i, cand], kind="stable")][:2]  # (stable: of equal distances the lower index first)
        nn[i, :len(order)] = order
        dist[i, :len(order)] = np.sqrt(d2m[i, order])
    assert dist.dtype == F32
    return nn, dist


def survives(nn, dist, max_ratio):
    """Rule 4: [n] bool."""
    with np.errstate(divide="ignore", invalid="ignore"):
        q = dist[:, 0] / dist[:, 1]
    assert q.dtype == F32
    return (nn[:, 1] >= 0) & ~(q.astype(np.float64) > float(max_ratio))


def median_disparity(xy1, xy2, matches):
    """Rule 6."""
    if len(matches) == 0 or xy1 is None or xy2 is None:
        return float("nan")
    p, q = xy1[matches[:, 0]].astype(np.float64), xy2[matches[:, 1]].astype(np.float64)
    dx, dy = p[:, 0] - q[:, 0], p[:, 1] - q[:, 1]
    v = np.sort(np.sqrt(dx * dx + dy * dy))
    mid = len(v) // 2
    return float(v[mid]) if len(v) % 2 else float((v[mid - 1] + v[mid]) / 2.0)


def empty_answer(n1, n2):
    return dict(nn12=np.full((n1, 2), -1, np.int32), dist12=np.full((n1, 2), np.nan, F32), nn21=np.full((n2, 2), -1, np.int32),
                dist21=np.full((n2, 2), np.nan, F32), matches=np.zeros((0, 2), np.int32), distances=np.zeros(0, F32), num_matches=0,
                median_disparity=float("nan"))


def restated_match(item):
    """Rules 1-6 in numpy: the outputs of the call, and d2 [n1, n2] (rule 2), mask, keep12 / keep21 (rule 4)."""
    d1, d2, xy1, xy2 = item_arrays(item)
    n1, n2 = len(d1), len(d2)
    if n1 < 2 or n2 < 2:
        return empty_answer(n1, n2)
    d2m, mask = restated_d2(d1, d2), restated_mask(item)
    nn12, dist12 = two_nearest(d2m, mask)
    nn21, dist21 = two_nearest(np.ascontiguousarray(d2m.T), np.ascontiguousarray(mask.T))
    keep12, keep21 = survives(nn12, dist12, item["max_ratio"]), survives(nn21, dist21, item["max_ratio"])
    rows = [(i, nn12[i, 0]) for i in range(n1) if keep12[i] and keep21[nn12[i, 0]] and nn21[nn12[i, 0], 0] == i]
    matches = np.array(rows, np.int32).reshape(-1, 2)
    return dict(nn12=nn12, dist12=dist12, nn21=nn21, dist21=dist21, matches=matches, distances=dist12[matches[:, 0], 0],
                num_matches=len(matches), median_disparity=median_disparity(xy1, xy2, matches), d2=d2m, mask=mask, keep12=keep12, keep21=keep21)


def exact_d2(item):
    """The squared distances [n1, n2] in float64."""
    d1, d2, _, _ = item_arrays(item)
    a, b = d1.astype(np.float64), d2.astype(np.float64)
    return ((a[:, None, :] - b[None, :, :]) ** 2).sum(axis=2)


def epsilon(item):
    """eps(i, j) of rule 7, [n1, n2]."""
    d1, d2, _, _ = item_arrays(item)
    na, nb = (d1.astype(np.float64) ** 2).sum(axis=1), (d2.astype(np.float64) ** 2).sum(axis=1)
    return 2.0 * (d1.shape[1] + 3) * U * (na[:, None] + nb[None, :])


def _flags_one_side(ex, eps, mask, max_ratio, dim):
    n = len(ex)
    out = np.zeros(n, bool)
    for i in range(n):
        cand = np.flatnonzero(mask[i])
        order = cand[np.argsort(ex[i, cand], kind="stable")][:3]
        if len(order) >= 3 and ex[i, order[2]] - ex[i, order[1]] <= 2.0 * eps[i, order].max():
            out[i] = True
        if len(order) >= 2 and ex[i, order[1]] > 0:
            ratio = np.sqrt(ex[i, order[0]] / ex[i, order[1]])
            if abs(ratio - max_ratio) <= (dim + 4) * 2.0 ** -23 * max_ratio:
                out[i] = True
    return out


def flags(item, ex=None):
    """The keypoints where rule 7 leaves the result open, (flag1 [n1], flag2 [n2]): at least three candidates and the
    exact d2 of the third within 2 max(eps) of the second's, or an exact ratio within a relative (dim + 4) 2^-23 of
    max_ratio."""
    ex = exact_d2(item) if ex is None else ex
    eps, mask = epsilon(item), restated_mask(item)
    dim = A.as_f32(item["descriptors1"]).shape[1]
    r = float(item["max_ratio"])
    return _flags_one_side(ex, eps, mask, r, dim), _flags_one_side(ex.T, eps.T, mask.T, r, dim)


# ---------------------------------------------------------------------------------------------------------------------
# host build
# ---------------------------------------------------------------------------------------------------------------------
CSRC_HEADERS = ("match_math.h", "tri_math.h", "ba_math.h")


def _stale(target, deps):
    return not os.path.exists(target) or max(os.path.getmtime(f) for f in deps) > os.path.getmtime(target)


@functools.lru_cache(maxsize=None)
def load_host():
    src = os.path.join(HERE, "host", "match_math_host.cpp")
    so = os.path.join(HERE, "host", "_match_math_host.so")
    hdrs = [os.path.join(ROOT, "mavmap_amd", "csrc", h) for h in CSRC_HEADERS] + [os.path.join(ROOT, "include", "mavba_match.h")]
    if _stale(so, [src] + hdrs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
    L = C.CDLL(so)
    L.mh_d2.argtypes = [fp, C.c_longlong, fp, C.c_longlong, C.c_int, fp]
    L.mh_d2.restype = None
    L.mh_mask.argtypes = [fp, C.c_longlong, fp, C.c_longlong, C.c_double, C.POINTER(C.c_uint8)]
    L.mh_mask.restype = None
    L.mh_match.argtypes = [C.POINTER(A.CMatchItem)]
    L.mh_match.restype = None
    return L


@pytest.fixture(scope="module")
def host():
    return load_host()


OUTPUTS = ("matches", "distances", "nn12", "dist12", "nn21", "dist21")
FILL = -7


def c_items(items, outputs=OUTPUTS, fill=FILL):
    """(ctypes array, output arrays, keep-alive) for a raw call; outputs not named are NULL (their arrays exist all the
    same, to see that they stay untouched). fill: the value every output array and scalar starts with."""
    arr = (A.CMatchItem * max(len(items), 1))()
    outs, hold = [], []
    for q, it in enumerate(items):
        d1, d2, xy1, xy2 = item_arrays(it)
        n1, n2, m = len(d1), len(d2), min(len(d1), len(d2))
        hold.append((d1, d2, xy1, xy2))
        c = arr[q]
        c.desc1, c.desc2, c.xy1, c.xy2 = A.ptr(d1, C.c_float), A.ptr(d2, C.c_float), A.ptr(xy1, C.c_float), A.ptr(xy2, C.c_float)
        c.n1, c.n2, c.dim = n1, n2, d1.shape[1]
        c.max_ratio, c.max_distance = float(it.get("max_ratio", 0.9)), float(it.get("max_distance", -1.0))
        o = dict(matches=np.full((m, 2), fill, np.int32), distances=np.full(m, fill, F32), nn12=np.full((n1, 2), fill, np.int32),
                 dist12=np.full((n1, 2), fill, F32), nn21=np.full((n2, 2), fill, np.int32), dist21=np.full((n2, 2), fill, F32))
        for name in outputs:
            setattr(c, name, A.ptr(o[name], C.c_int32 if o[name].dtype == np.int32 else C.c_float))
        c.num_matches, c.median_disparity, c.kernel_seconds = fill, float(fill), float(fill)
        outs.append(o)
    return arr, outs, hold


def records(arr, outs):
    """What a call left, one dict per item: the arrays as they are (matches and distances in full, with the fill behind
    the rows that were written) and the scalars."""
    return [dict(o, num_matches=int(arr[q].num_matches), median_disparity=float(arr[q].median_disparity),
                 kernel_seconds=float(arr[q].kernel_seconds)) for q, o in enumerate(outs)]


@functools.lru_cache(maxsize=None)
def _host_grid(g):
    return host_run([grid_item(*g)])[0]


def host_run(items, outputs=OUTPUTS):
    """The host build over every item (one thread, exhaustive)."""
    L = load_host()
    arr, outs, hold = c_items(items, outputs)
    for q in range(len(items)):
        L.mh_match(C.byref(arr[q]))
    return records(arr, outs)


# ---------------------------------------------------------------------------------------------------------------------
# checks shared with the GPU test
# ---------------------------------------------------------------------------------------------------------------------
def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def same_scalar(a, b):
    return (np.isnan(a) and np.isnan(b)) or a == b


def check_equal(rec, want, what="", outputs=OUTPUTS):
    """rec (a record of a call) equals want (a record or a restatement) bit for bit in every output named."""
    m = want["num_matches"]
    assert rec["num_matches"] == m, what
    assert same_scalar(rec["median_disparity"], want["median_disparity"]), (what, rec["median_disparity"], want["median_disparity"])
    for name in outputs:
        if name in ("matches", "distances"):
            assert same(rec[name][:m], want[name][:m]), (what, name)
            assert np.all(rec[name][m:] == FILL), (what, name, "rows behind num_matches are left alone")
        else:
            assert same(rec[name], want[name]), (what, name)


def check_empty(rec, what="", outputs=OUTPUTS):
    """An item the host answers: n1 < 2 or n2 < 2."""
    assert rec["num_matches"] == 0 and np.isnan(rec["median_disparity"]), what
    for name in outputs:
        if name.startswith("nn"):
            assert np.all(rec[name] == -1), (what, name)
        elif name.startswith("dist") and name != "distances":
            assert np.isnan(rec[name]).all(), (what, name)
        else:
            assert np.all(rec[name] == FILL), (what, name)


def check_against_host(rec, want, item, what=""):
    """A record of the library against the host build's (or the restatement's) under rule 7: unflagged keypoints bit for
    bit; flagged ones by the rule's set condition; the matches after those that touch a flagged keypoint on either side
    are removed from both lists. Returns the number of flagged keypoints."""
    d1, d2, xy1, xy2 = item_arrays(item)
    n1, n2 = len(d1), len(d2)
    if n1 < 2 or n2 < 2:
        check_empty(rec, what)
        return 0
    ex = exact_d2(item)
    f1, f2 = flags(item, ex)
    if not f1.any() and not f2.any():
        check_equal(rec, want, what)
        return 0
    eps, mask, d2m = epsilon(item), restated_mask(item), restated_d2(d1, d2)
    for nn, dist, wnn, wdist, f, e, ep, mk, dm in ((rec["nn12"], rec["dist12"], want["nn12"], want["dist12"], f1, ex, eps, mask, d2m),
                                                   (rec["nn21"], rec["dist21"], want["nn21"], want["dist21"], f2, ex.T, eps.T, mask.T, d2m.T)):
        assert same(nn[~f], wnn[~f]) and same(dist[~f], wdist[~f]), what
        for i in np.flatnonzero(f):
            cand = np.flatnonzero(mk[i])
            order = cand[np.argsort(e[i, cand], kind="stable")]
            a, b = int(nn[i, 0]), int(nn[i, 1])
            assert a >= 0 and b >= 0 and a != b and mk[i, a] and mk[i, b], (what, i)
            limit = e[i, order[1]] + 2.0 * ep[i, order[:3]].max()
            assert e[i, a] <= limit and e[i, b] <= limit, (what, i)
            assert dm[i, a] < dm[i, b] or (dm[i, a] == dm[i, b] and a < b), (what, i, "rule-3 order")
            assert dist[i, 0] == np.sqrt(dm[i, a]) and dist[i, 1] == np.sqrt(dm[i, b]), (what, i, "rule-2 distances")
    m = rec["num_matches"]
    assert 0 <= m <= min(n1, n2), what
    got, gd = rec["matches"][:m], rec["distances"][:m]
    assert np.all(rec["matches"][m:] == FILL) and np.all(rec["distances"][m:] == FILL), what
    assert np.all(np.diff(got[:, 0]) > 0), what
    assert same_scalar(rec["median_disparity"], median_disparity(xy1, xy2, got)), what
    wm, wd = want["matches"][:want["num_matches"]], want["distances"][:want["num_matches"]]
    kg, kw = ~(f1[got[:, 0]] | f2[got[:, 1]]), ~(f1[wm[:, 0]] | f2[wm[:, 1]])
    # (a match of unflagged i and j needs nn21[j][0] == i and nn12[i][0] == j only: both are unflagged rows)
    assert same(got[kg], wm[kw]) and same(gd[kg], wd[kw]), what
    return int(f1.sum() + f2.sum())


# ---------------------------------------------------------------------------------------------------------------------
# the tests
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def grid_restated(g):
    return restated_match(grid_item(*g))


@functools.lru_cache(maxsize=None)
def grid_flags(g):
    return flags(grid_item(*g))


def test_cap_on_the_generated_inputs():
    """A condition on the INPUTS, on the restatement alone: no grid item with n <= 65 on both sides has a flagged
    keypoint, and no item has more than 2 % of its keypoints flagged."""
    for g in GRID:
        f1, f2 = grid_flags(g)
        count = int(f1.sum() + f2.sum())
        if max(g[0], g[1]) <= 65:
            assert count == 0, (g, count)
        assert count <= 0.02 * (g[0] + g[1]), (g, count)


def test_host_build_equals_the_restatement_bit_for_bit(host):
    for g in GRID:
        item = grid_item(*g)
        check_equal(_host_grid(g), grid_restated(g), grid_id(g))
        d1, d2, xy1, xy2 = item_arrays(item)
        out = np.zeros((g[0], g[1]), F32)
        host.mh_d2(A.ptr(d1, C.c_float), g[0], A.ptr(d2, C.c_float), g[1], g[2], A.ptr(out, C.c_float))
        if min(g[0], g[1]) >= 2:
            assert same(out, grid_restated(g)["d2"]), grid_id(g)
            back = np.zeros((g[1], g[0]), F32)
            host.mh_d2(A.ptr(d2, C.c_float), g[1], A.ptr(d1, C.c_float), g[0], g[2], A.ptr(back, C.c_float))
            assert same(back.T, out), "d2(i, j) and d2(j, i) are the same bits"
            if g[3] >= 0:
                mk = np.zeros((g[0], g[1]), np.uint8)
                host.mh_mask(A.ptr(xy1, C.c_float), g[0], A.ptr(xy2, C.c_float), g[1], g[3], mk.ctypes.data_as(C.POINTER(C.c_uint8)))
                assert same(mk.astype(bool), grid_restated(g)["mask"]), grid_id(g)


def restatement_error_ratio(g):
    """The largest relative error of a restated distance against the exact one, as a share of its bound
    (dim + 2) 2^-24, and whether the indices of the unflagged keypoints are those of exact_d2."""
    item = grid_item(*g)
    if min(g[0], g[1]) < 2:
        return 0.0
    r, ex, (f1, f2) = grid_restated(g), exact_d2(item), grid_flags(g)
    worst = 0.0
    for nn, dist, f, e, mk in ((r["nn12"], r["dist12"], f1, ex, r["mask"]), (r["nn21"], r["dist21"], f2, ex.T, r["mask"].T)):
        for i in range(len(nn)):
            cand = np.flatnonzero(mk[i])
            order = cand[np.argsort(e[i, cand], kind="stable")][:2]
            want = np.full(2, -1)
            want[:len(order)] = order
            # (a first and a second closer than the rounding of rule 2 itself may come in either order)
            close = len(order) == 2 and e[i, order[1]] - e[i, order[0]] <= 2 * (g[2] + 2) * U * e[i, order[1]]
            if not f[i]:
                assert np.array_equal(nn[i], want) or (close and set(nn[i]) == set(want)), (g, i)
            for k in range(2):
                if nn[i, k] >= 0 and e[i, nn[i, k]] > 0:
                    d = np.sqrt(e[i, nn[i, k]])
                    worst = max(worst, abs(float(dist[i, k]) - d) / d / ((g[2] + 2) * U))
    return worst


def test_restatement_against_float64():
    """On unflagged keypoints the restatement's indices are those of the float64 distances under (d2, index) order, and
    every distance is within a relative (dim + 2) 2^-24 of the exact one: the forward bound of the rule-2 sum, halved
    by the root, plus the root's own rounding. Largest observed share of that bound over the grid: 0.33 (at dim 4; the rounding errors of a long sum mostly cancel)."""
    worst = max(restatement_error_ratio(g) for g in GRID)
    print("largest share of the bound: %.4f" % worst)
    assert worst <= 1.0


def test_every_filter_bites():
    """On the (257, 257, 128) item each of the three filters removes a candidate the other two keep (restatement alone)."""
    r = grid_restated((257, 257, 128, -1.0))
    nn12, nn21, k12, k21 = r["nn12"], r["nn21"], r["keep12"], r["keep21"]
    j = nn12[:, 0]
    mutual = nn21[j, 0] == np.arange(257)
    assert np.any(mutual & k21[j] & ~k12), "the ratio test 1->2"
    assert np.any(mutual & k12 & ~k21[j]), "the ratio test 2->1"
    i = nn21[:, 0]
    cross = np.any(k12 & k21[j] & ~mutual) or np.any(k21 & k12[i] & (nn12[i, 0] != np.arange(257)))
    assert cross, "the cross-check"
    assert 0 < r["num_matches"] < int(0.6 * 257)


def integer_brute_force(a, b):
    """(nn [n, 2], d2 [n, 2]) of integer descriptors by (d2, index), in integers."""
    d = ((a[:, None, :] - b[None, :, :]) ** 2).sum(axis=2)
    order = np.argsort(d, axis=1, kind="stable")
    return order[:, :2].astype(np.int32), np.take_along_axis(d, order, axis=1)


def test_exact_integer_data(host):
    for n1, n2 in INTEGER_SIZES:
        item = integer_item(n1, n2)
        a, b = item["descriptors1"].astype(np.int64), item["descriptors2"].astype(np.int64)
        assert not np.array_equal(a[:min(n1, n2)], b[:min(n1, n2)])
        rec, r = host_run([item])[0], restated_match(item)
        check_equal(rec, r, "integers %dx%d" % (n1, n2))
        ties = set()
        for nn, dist, (wnn, wd) in ((rec["nn12"], rec["dist12"], integer_brute_force(a, b)), (rec["nn21"], rec["dist21"], integer_brute_force(b, a))):
            assert np.array_equal(nn, wnn)
            assert same(dist, np.sqrt(wd[:, :2].astype(F32)))  # (the integer is exact in float32, its root correctly rounded)
            ties |= {"first" for row in wd if row[0] == row[1]} | {"second" for row in wd if row[1] == row[2]}
            ties |= {"third" for row in wd if row[0] == row[1] == row[2]}
        assert ties == {"first", "second", "third"}
        # (A tie in second and third place is a flagged keypoint by the letter of rule 7. With exact arithmetic the
        # screening score is exact too and (score, index) is rule 3, so the GPU test asks for equality on this item.)
        assert flags(item)[0].any()


def _edge(d1, d2, xy1=None, xy2=None, **kw):
    it = dict(descriptors1=np.asarray(d1, F32), descriptors2=np.asarray(d2, F32), max_ratio=0.9, max_distance=-1.0)
    if xy1 is not None:
        it.update(keypoints1=np.asarray(xy1, F32), keypoints2=np.asarray(xy2, F32))
    it.update(kw)
    return it


def decision_edge_items():
    """name -> item, the edges of rules 1, 4, 5 and 6."""
    rng = np.random.default_rng(11)
    e = np.eye(8, dtype=F32)
    items = {}
    # image 2 holds a[0] twice: d0 = d1 = 0, the quotient is NaN and the keypoint STAYS (rule 4); the two copies see a[0]
    # as their nearest, but a[0]'s first neighbour is the lower index only
    items["zero_over_zero"] = _edge([e[0], e[1], e[2]], [e[0], e[0], e[3], 2 * e[1]])
    # one duplicate on the far side: d0 = 0 < d1, ratio 0
    items["zero_over_positive"] = _edge([e[0], e[1], e[2]], [e[0], e[3], e[4] + e[1]])
    # the mask leaves keypoint 0 of image 1 no candidate, keypoint 1 one and keypoint 2 two (max_distance = 40)
    xy1 = [[700.0, 400.0], [100.0, 100.0], [300.0, 300.0], [500.0, 100.0]]
    xy2 = [[110.0, 100.0], [310.0, 300.0], [300.0, 320.0], [500.0, 110.0], [500.0, 120.0], [505.0, 100.0]]
    items["mask_0_1_2"] = _edge(_unit_rows(rng.standard_normal((4, 8))), _unit_rows(rng.standard_normal((6, 8))), xy1, xy2, max_distance=40.0)
    # exactly on the circle: dx*dx + dy*dy == max_distance^2 is NOT a candidate (the comparison is <)
    items["mask_on_the_circle"] = _edge(_unit_rows(rng.standard_normal((2, 8))), _unit_rows(rng.standard_normal((3, 8))),
                                        [[0.0, 0.0], [24.0, 32.0]], [[24.0, 32.0], [0.0, 40.0], [-10.0, -10.0]], max_distance=40.0)
    base = make_item(17, 17, 64, 2)
    items["default"] = base
    items["max_ratio_0"] = dict(base, max_ratio=0.0)
    items["max_ratio_1"] = dict(base, max_ratio=1.0)
    items["max_distance_0"] = dict(base, max_distance=0.0)
    items["no_keypoints"] = make_item(17, 16, 64, 2, with_xy=False)
    # an even and an odd number of matches for the median: the second item is the first without the image-1 keypoint of
    # its first match
    full = make_item(17, 17, 64, 3)
    first = int(restated_match(full)["matches"][0, 0])
    items["median_a"] = full
    items["median_b"] = dict(full, descriptors1=np.delete(full["descriptors1"], first, axis=0), keypoints1=np.delete(full["keypoints1"], first, axis=0))
    items["no_matches"] = _edge(_unit_rows(rng.standard_normal((5, 8))), _unit_rows(rng.standard_normal((4, 8))), max_ratio=0.01)
    return items


def check_decision_edges(recs):
    """What the edges are about, on records of the host build or of the library (name -> record)."""
    r = recs["zero_over_zero"]
    assert same(r["nn12"][0], np.array([0, 1], np.int32)) and same(r["dist12"][0], np.zeros(2, F32))
    assert [0, 0] in r["matches"][:r["num_matches"]].tolist()  # 0 / 0 is not greater than max_ratio
    r = recs["zero_over_positive"]
    assert r["nn12"][0, 0] == 0 and r["dist12"][0, 0] == 0 and r["dist12"][0, 1] > 0 and [0, 0] in r["matches"][:r["num_matches"]].tolist()
    r = recs["mask_0_1_2"]
    assert same(r["nn12"][0], np.array([-1, -1], np.int32)) and np.isnan(r["dist12"][0]).all()
    assert r["nn12"][1].tolist() == [0, -1] and not np.isnan(r["dist12"][1, 0]) and np.isnan(r["dist12"][1, 1])
    assert sorted(r["nn12"][2].tolist()) == [1, 2] and sorted(r["nn12"][3].tolist())[0] >= 3
    assert 1 not in r["matches"][:r["num_matches"], 0].tolist()  # one candidate: dropped (feature.cc:87)
    r = recs["mask_on_the_circle"]
    assert r["nn12"][0].tolist() == [2, -1] and sorted(r["nn12"][1].tolist()) == [0, 1]
    assert recs["max_ratio_0"]["num_matches"] == 0 and recs["max_ratio_1"]["num_matches"] > recs["default"]["num_matches"] > 0
    r = recs["max_distance_0"]
    assert r["num_matches"] == 0 and np.all(r["nn12"] == -1) and np.all(r["nn21"] == -1) and np.isnan(r["dist12"]).all() and np.isnan(r["median_disparity"])
    r = recs["no_keypoints"]
    assert r["num_matches"] > 0 and np.isnan(r["median_disparity"])
    a, b = recs["median_a"], recs["median_b"]
    assert {a["num_matches"] % 2, b["num_matches"] % 2} == {0, 1} and min(a["num_matches"], b["num_matches"]) >= 3
    assert a["median_disparity"] > 0 and b["median_disparity"] > 0
    assert recs["no_matches"]["num_matches"] == 0 and np.isnan(recs["no_matches"]["median_disparity"]) and np.all(recs["no_matches"]["nn12"] >= 0)


def test_decision_edges(host):
    items = decision_edge_items()
    recs = dict(zip(items, host_run(list(items.values()))))
    for name, item in items.items():
        check_equal(recs[name], restated_match(item), name)
    check_decision_edges(recs)
    # the items the host answers
    small = [make_item(0, 0, 64, 1, with_xy=False), make_item(1, 64, 64, 1), make_item(64, 1, 128, 1, max_distance=40.0), make_item(0, 5, 4, 1)]
    for rec, item in zip(host_run(small), small):
        check_empty(rec)
        check_equal(rec, restated_match(item))


def check_near_duplicates(rec, item, what=""):
    """The duplicate is the first neighbour on both sides and a match; the returned distances are the direct ones, within
    a relative (dim + 2) 2^-24 of the exact ones."""
    i, j = item["duplicates"]
    ex = exact_d2(item)
    dim = item["descriptors1"].shape[1]
    assert np.array_equal(rec["nn12"][i, 0], j) and np.array_equal(rec["nn21"][j, 0], i), what
    want = np.sqrt(ex[i, j])
    assert np.all(want > 0) and np.all(want < 1e-2)
    for got in (rec["dist12"][i, 0], rec["dist21"][j, 0]):
        assert np.all(np.abs(got.astype(np.float64) - want) <= (dim + 2) * U * want), what
    pairs = set(map(tuple, rec["matches"][:rec["num_matches"]].tolist()))
    assert set(zip(i.tolist(), j.tolist())) <= pairs, what


def test_near_duplicates(host):
    for n1, n2, dim, seed in NEAR_DUPLICATE_SIZES:
        item = near_duplicate_item(n1, n2, dim, seed)
        f1, f2 = flags(item)
        assert not f1.any() and not f2.any()
        rec = host_run([item])[0]
        check_equal(rec, restated_match(item), "near duplicates %dx%dx%d" % (n1, n2, dim))
        check_near_duplicates(rec, item)
        # the expanded form in float32, as a screening would evaluate it, IS rounding noise there
        a, b = item["descriptors1"], item["descriptors2"]
        i, j = item["duplicates"]
        score = ((a[i] * a[i]).sum(axis=1) + (b[j] * b[j]).sum(axis=1)) - F32(2) * (a[i] * b[j]).sum(axis=1)
        assert score.dtype == F32 and np.all(np.abs(score - exact_d2(item)[i, j]) <= epsilon(item)[i, j])
        if dim >= 64:
            assert np.any(np.abs(score - exact_d2(item)[i, j]) > exact_d2(item)[i, j])


def test_null_outputs_on_the_host_build(host):
    item = grid_item(17, 65, 64, 40.0)
    full = host_run([item])[0]
    for leave in OUTPUTS:
        rec = host_run([item], outputs=tuple(o for o in OUTPUTS if o != leave))[0]
        assert np.all(rec[leave] == FILL), leave
        check_equal(rec, full, leave, outputs=tuple(o for o in OUTPUTS if o != leave))
    rec = host_run([item], outputs=())[0]
    assert rec["num_matches"] == full["num_matches"] and rec["median_disparity"] == full["median_disparity"]


# ---------------------------------------------------------------------------------------------------------------------
# the record, the stand-alone sanitizer program
# ---------------------------------------------------------------------------------------------------------------------
LAYOUT_FIELDS = ("desc1", "desc2", "xy1", "xy2", "n1", "n2", "dim", "max_ratio", "max_distance", "matches", "distances", "nn12", "dist12",
                 "nn21", "dist21", "num_matches", "median_disparity", "kernel_seconds")


def test_item_layout_matches_the_header():
    fields = ", ".join(f"offsetof(mavba_match_item, {f})" for f in LAYOUT_FIELDS)
    src = r"""
#include <stdio.h>
#include <stddef.h>
#include "mavba_match.h"
int main(void) {
  size_t v[] = {sizeof(mavba_match_item), %s};
  for (size_t i = 0; i < sizeof(v) / sizeof(v[0]); ++i) printf("%%zu ", v[i]);
  printf("\n");
  return 0;
}""" % fields
    with tempfile.TemporaryDirectory() as td:
        open(os.path.join(td, "t.c"), "w").write(src)
        exe = os.path.join(td, "t")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(td, "t.c"), "-o", exe])
        out = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    assert out == [C.sizeof(A.CMatchItem)] + [getattr(A.CMatchItem, f).offset for f in LAYOUT_FIELDS]
    assert [f[0] for f in A.CMatchItem._fields_] == list(LAYOUT_FIELDS)


def test_the_header_states_the_contract():
    header = " ".join(open(os.path.join(ROOT, "include", "mavba_match.h")).read().replace("*", " ").split())
    for text in ("The ratio_test = false branch of the reference (feature.cc:103-131) is NOT offered", "without fused multiply-adds",
                 "of equal distances the lower index comes first", "0 / 0 is NaN, which is not greater",
                 "The HOST computes it from the downloaded matches", "eps(i, j) = 2 (dim + 3) 2^-24 (|a_i|^2 + |b_j|^2)",
                 "re-evaluated by rule 2 and ordered by rule 3", "Results are bit-reproducible"):
        assert text in header, text


def test_standalone_program_under_the_host_sanitizers():
    src = os.path.join(HERE, "host", "match_math_main.cpp")
    first = open(src).read().split("\n", 3)
    assert "g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tests/host/match_math_main.cpp" in first[1]
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "match_math_main")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", exe])
        run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip().endswith("ok")


def test_python_wrapper_without_a_device(mavba):
    from mavmap_amd import api
    assert api.MATCH_SYMBOLS == ["mavba_match_descriptors"] and hasattr(mavba.load(), "mavba_match_descriptors")
    for other in (api.EXPORTED_SYMBOLS, api.TRIANGULATE_SYMBOLS, api.ABSPOSE_SYMBOLS, api.RELPOSE_SYMBOLS, api.HOMOGRAPHY_SYMBOLS, api.BACKSUB_TILES_SYMBOLS):
        assert not set(api.MATCH_SYMBOLS) & set(other)
    assert mavba.match_descriptors([]) == [] and mavba.to_homography_items([], []) == []
    item = grid_item(17, 65, 64, 40.0)
    r = restated_match(item)
    res = mavba.MatchResult(r["matches"], r["distances"], r["nn12"], r["dist12"], r["nn21"], r["dist21"], r["median_disparity"], 0.0)
    h = mavba.to_homography_items([dict(item, max_trials=50)], [res])[0]
    assert h["max_trials"] == 50 and "descriptors1" not in h and res.num_matches == len(h["points2D1"]) == len(h["points2D2"]) > 0
    assert np.array_equal(h["points2D1"], item["keypoints1"][r["matches"][:, 0]].astype(float)) and h["points2D2"].dtype == np.float64
    if mavba.device_count() > 0:
        return  # (the rest is what a machine without a GPU answers)
    with pytest.raises(mavba.MavbaError) as ei:
        mavba.match_descriptors([item])
    assert ei.value.code == A.ERR_NO_DEVICE and "no CPU path" in str(ei.value)
