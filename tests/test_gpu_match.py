"""mavba_match_descriptors on the GPU (csrc/match.hip) with the generators and checkers of tests/test_match_host.py:
every grid item alone against the host build under rule 7 of include/mavba_match.h, the exact-integer and
near-duplicate items bit for bit, a mixed batch with its reproducibility, NULL outputs, and the chain into
homography_ransac and view_change_pairs.

Sizes: n1, n2 in {2, 3, 15, 16, 17, 63, 64, 65, 257} - the edges of a 16-wide matrix tile, of the 64 keypoints of a
strip and of the 64 descriptors of a staged tile, and one size above the 256 keypoints of a chunk of the decision
kernel; dim in {4, 60, 64, 128} (60 and 4 are padded to the 16 of a block of matrix steps). The largest item is
257 x 257 x 128."""
import numpy as np
import pytest

from mavmap_amd import _abi as A
from tests import test_match_host as T

pytestmark = pytest.mark.gpu


def gpu_run(mavba, items, outputs=T.OUTPUTS):
    arr, outs, hold = T.c_items(items, outputs)
    rc = mavba.load().mavba_match_descriptors(len(items), arr, -1)
    assert rc == A.OK, mavba.load().mavba_last_error()
    return T.records(arr, outs)


def same_bits(a, b, skip=("kernel_seconds",)):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a if k not in skip)


@pytest.mark.parametrize("g", T.GRID, ids=T.grid_id)
def test_single_item(mavba, g):
    item = T.grid_item(*g)
    rec, = gpu_run(mavba, [item])
    if min(g[0], g[1]) < 2:
        T.check_empty(rec, T.grid_id(g))
    else:
        flagged = T.check_against_host(rec, T._host_grid(g), item, T.grid_id(g))
        assert flagged == sum(int(f.sum()) for f in T.grid_flags(g))
        assert rec["kernel_seconds"] > 0


def test_flagged_keypoints_are_exercised():
    """(What test_single_item's rule-7 branch runs on: some items of the grid do have flagged keypoints.)"""
    assert sum(int(f.sum()) for g in T.GRID for f in T.grid_flags(g)) > 0


def test_integer_and_near_duplicate_items_equal_the_host_build(mavba):
    """Everything bit for bit: with integer data every float operation is exact, the screening score included, so
    (score, index) IS rule 3; the near-duplicate items have no flagged keypoint. What a swapped row / column map, a
    wrong k order or a tile-edge mask would break."""
    items = [T.integer_item(n1, n2) for n1, n2 in T.INTEGER_SIZES] + [T.near_duplicate_item(*s) for s in T.NEAR_DUPLICATE_SIZES]
    want = T.host_run(items)
    recs = gpu_run(mavba, items)
    for q, (rec, w, item) in enumerate(zip(recs, want, items)):
        T.check_equal(rec, w, "item %d" % q)
        if "duplicates" in item:
            T.check_near_duplicates(rec, item, "item %d" % q)


def test_decision_edges(mavba):
    items = T.decision_edge_items()
    recs = dict(zip(items, gpu_run(mavba, list(items.values()))))
    want = dict(zip(items, T.host_run(list(items.values()))))
    for name, item in items.items():
        T.check_against_host(recs[name], want[name], item, name)
    T.check_decision_edges(recs)


def mixed_batch():
    order = [(257, 257, 128, 40.0), (2, 3, 60, -1.0), (17, 65, 64, -1.0), "0x0", (65, 17, 64, 40.0), (16, 257, 64, -1.0), "1x64", (63, 64, 64, -1.0),
             (64, 65, 128, -1.0), (257, 3, 60, -1.0), (65, 65, 60, 40.0), (15, 16, 4, -1.0)]
    small = {"0x0": T.make_item(0, 0, 64, 1, with_xy=False), "1x64": T.make_item(1, 64, 64, 1)}
    assert all(isinstance(o, str) or o in T.GRID for o in order)
    return [(o, small[o] if isinstance(o, str) else T.grid_item(*o)) for o in order]


def test_mixed_batch_alone_reversed_and_twice(mavba):
    batch = mixed_batch()
    items = [it for _, it in batch]
    recs = gpu_run(mavba, items)
    for (o, it), rec in zip(batch, recs):
        if isinstance(o, str):
            T.check_empty(rec, o)
        else:
            T.check_against_host(rec, T._host_grid(o), it, "batch " + T.grid_id(o))
    again = gpu_run(mavba, items)
    assert all(same_bits(a, b) for a, b in zip(recs, again))                      # a call gives the same bits twice
    rev = gpu_run(mavba, items[::-1])[::-1]
    assert all(same_bits(a, b) for a, b in zip(recs, rev))                        # ... in the reversed batch
    for q in (0, 2, 5, 7, 10):
        alone, = gpu_run(mavba, [items[q]])
        assert same_bits(recs[q], alone), q                                       # ... and alone


def test_null_outputs_leave_the_others_unchanged(mavba):
    items = [T.grid_item(257, 257, 128, 40.0), T.grid_item(17, 65, 64, -1.0), T.make_item(1, 64, 64, 1)]
    full = gpu_run(mavba, items)
    for name in T.OUTPUTS:
        part = gpu_run(mavba, items, outputs=tuple(o for o in T.OUTPUTS if o != name))
        for f, p in zip(full, part):
            assert same_bits({k: v for k, v in f.items() if k != name}, {k: v for k, v in p.items() if k != name}), name
            assert np.all(p[name] == T.FILL), name   # (not handed over: not written)
    none = gpu_run(mavba, items, outputs=())
    for f, p in zip(full, none):
        assert f["num_matches"] == p["num_matches"] and T.same_scalar(f["median_disparity"], p["median_disparity"])
        assert all(np.all(p[name] == T.FILL) for name in T.OUTPUTS)


CHAIN_SEED = 7  # chosen on the CPU (restatement alone): no flagged keypoint in either pair, 138 matches each


def chain_pairs():
    """Two pairs of 257 keypoints with the descriptors of a grid item: in the first the keypoints of image 2 are a
    homography of their partners in image 1, in the second they have parallax (a shift that depends on a depth drawn
    per keypoint). A keypoint of image 2 that is no copy lies anywhere."""
    pairs = []
    for kind in ("planar", "parallax"):
        it = T.make_item(257, 257, 128, CHAIN_SEED)
        r = T.restated_match(it)
        rng = np.random.default_rng([CHAIN_SEED, len(pairs)])
        xy1 = it["keypoints1"].astype(float)
        xy2 = rng.uniform(0, 1, (257, 2)) * [752.0, 480.0]
        i, j = r["matches"][:, 0], r["matches"][:, 1]
        if kind == "planar":
            w = 1 + 2e-5 * xy1[i, 0] - 1e-5 * xy1[i, 1]
            xy2[j] = np.stack([(1.02 * xy1[i, 0] + 0.01 * xy1[i, 1] + 5) / w, (-0.02 * xy1[i, 0] + 0.97 * xy1[i, 1] - 8) / w], axis=1)
        else:
            xy2[j] = xy1[i] + np.stack([90.0 / rng.uniform(1.0, 6.0, len(i)), rng.uniform(-1, 1, len(i))], axis=1)
        xy2[j] += rng.uniform(-0.5, 0.5, (len(i), 2))
        pairs.append(dict(it, keypoints2=xy2.astype(np.float32)))
    return pairs


def _homography_share(uv1, uv2, rng, trials=200, thr=4.0):
    """The largest inlier share of a homography through four of the matches, over `trials` draws (numpy, DLT)."""
    best = 0.0
    n = len(uv1)
    for _ in range(trials):
        s = rng.permutation(n)[:4]
        rows = []
        for (x, y), (u, v) in zip(uv1[s], uv2[s]):
            rows += [[x, y, 1, 0, 0, 0, -x * u, -y * u, -u], [0, 0, 0, x, y, 1, -x * v, -y * v, -v]]
        h = np.linalg.svd(np.array(rows))[2][-1].reshape(3, 3)
        p = np.concatenate([uv1, np.ones((n, 1))], axis=1) @ h.T
        with np.errstate(divide="ignore", invalid="ignore"):
            err = np.linalg.norm(p[:, :2] / p[:, 2:] - uv2, axis=1)
        best = max(best, float(np.mean(err <= thr)))
    return best


def test_the_chain_from_descriptors_to_the_view_change_gate(mavba):
    """match_descriptors -> to_homography_items -> homography_ransac with the mapper's stop -> view_change_pairs keeps
    exactly the parallax pair."""
    pairs = chain_pairs()
    # the restatements alone, before the library's numbers are read
    restated = [T.restated_match(p) for p in pairs]
    rng = np.random.default_rng(CHAIN_SEED)
    shares = []
    for p, r in zip(pairs, restated):
        assert r["num_matches"] >= 60
        f1, f2 = T.flags(p)
        assert not (f1[r["matches"][:, 0]] | f2[r["matches"][:, 1]]).any()
        shares.append(_homography_share(p["keypoints1"][r["matches"][:, 0]].astype(float), p["keypoints2"][r["matches"][:, 1]].astype(float), rng))
    assert shares[0] >= 0.9 and shares[1] <= 0.5, shares
    results = mavba.match_descriptors(pairs)
    for res, r in zip(results, restated):
        assert T.same(res.matches, r["matches"]) and T.same(res.distances, r["distances"]) and res.median_disparity == r["median_disparity"]
    items = mavba.to_homography_items(pairs, results)
    for it, res in zip(items, results):
        it["max_trials"], it["stop_num_inliers"] = 100, mavba.view_change_stop(len(res.matches), 0.7)
    hres = mavba.homography_ransac(items)
    assert hres[0].ok and hres[0].inlier_ratio > 0.7 and hres[1].inlier_ratio <= 0.5  # (the stop ends the first pair's run above 0.7)
    assert mavba.view_change_pairs(items, hres, 0.7) == [1]
