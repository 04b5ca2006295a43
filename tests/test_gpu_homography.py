"""mavba_homography_ransac on the GPU (csrc/homography.hip) with the checker and the generators of
tests/test_homography_host.py: the hypothesis bound on 64 of the 300 inputs, counts, sums and the replayed selection per
item, bit-reproducibility, NULL outputs, degenerate inputs, and the gate with the chain into relative_pose_ransac.

Sizes: n in {5, 63, 64, 65, 255, 256, 257, 513} - the edges of a wave (64) and of the last work-group's stride (256);
max_trials in {1, 3, 100} and 15, 16, 17 around the 16 trials one work-group takes - alone, and mixed in one batch
with an n = 0 and an n = 4 item in the middle."""

import numpy as np
import pytest

from mavmap_amd import _abi as A
from tests import test_homography_host as T

pytestmark = pytest.mark.gpu

SIZES = (5, 63, 64, 65, 255, 256, 257, 513)
TRIALS = (1, 3, 15, 16, 17, 100)
_cache = {}


def case(n, mt):
    """One item - generated once, shared by the tests, never modified. Drawn and supplied rows, the stops and the kind of
    pair alternate over the grid."""
    key = (n, mt)
    if key not in _cache:
        k = SIZES.index(n) + TRIALS.index(mt)
        _cache[key] = T.make_item(n, seed=31, kind=("planar", "planar", "parallax")[k % 3], max_trials=mt, stop_frac=(None, 0.7, None, 1.0)[k % 4],
                                  supplied=k % 2 == 1)
    return _cache[key]


def gpu_run(mavba, items, outputs=T.OUTPUTS, fill=None):
    arr, outs, hold = T.c_items(items, outputs, fill)
    rc = mavba.load().mavba_homography_ransac(len(items), arr, -1)
    assert rc == A.OK, mavba.load().mavba_last_error()
    return T.records(arr, outs)


def same_bits(a, b, skip=("kernel_seconds",)):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a if k not in skip)


def mixed_batch():
    order = [(513, 100), (5, 3), (64, 17), (255, 1), "n0", (257, 16), "n4", (63, 100), (256, 15), (65, 100), (5, 100)]
    deg = T.degenerate_items()
    return [deg[o] if isinstance(o, str) else case(*o) for o in order]


@pytest.mark.parametrize("mt", TRIALS)
@pytest.mark.parametrize("n", SIZES)
def test_single_item(mavba, n, mt):
    item = case(n, mt)
    rec, = gpu_run(mavba, [item])
    T.check_record(rec, item, what=f"n={n} trials={mt}")
    assert rec["kernel_seconds"] > 0


def test_mixed_batch_alone_reversed_and_twice(mavba):
    items = mixed_batch()
    recs = gpu_run(mavba, items)
    for it, rec in zip(items, recs):
        if len(it["points2D1"]) > 4:
            T.check_record(rec, it, what=f"batch n={len(it['points2D1'])} trials={it['max_trials']}")
        else:
            T.check_empty(rec, what=f"batch n={len(it['points2D1'])}")
    again = gpu_run(mavba, items)
    assert all(same_bits(a, b) for a, b in zip(recs, again))                      # a call gives the same bits twice
    rev = gpu_run(mavba, items[::-1])[::-1]
    assert all(same_bits(a, b) for a, b in zip(recs, rev))                        # ... in the reversed batch
    for q in (0, 2, 5, 7, 9):
        alone, = gpu_run(mavba, [items[q]])
        assert same_bits(recs[q], alone), q                                       # ... and alone


def test_null_outputs_leave_the_others_unchanged(mavba):
    items = [case(257, 17), case(65, 100), T.degenerate_items()["n4"]]
    full = gpu_run(mavba, items)
    for name in T.OUTPUTS:
        part = gpu_run(mavba, items, outputs=tuple(o for o in T.OUTPUTS if o != name), fill=-7)
        for f, p in zip(full, part):
            assert same_bits({k: v for k, v in f.items() if k != name}, {k: v for k, v in p.items() if k != name}), name
            assert np.all(p[name] == (-7 % 256 if p[name].dtype == np.uint8 else -7)), name   # (not handed over: not written)
    none = gpu_run(mavba, items, outputs=())
    for f, p in zip(full, none):
        assert all(np.asarray(f[k]).tobytes() == np.asarray(p[k]).tobytes() for k in T.SCALARS)


def test_hypothesis_bound_on_64_of_the_300_inputs(mavba):
    """The kernel's model of 64 of the 300 inputs of T.test_hypothesis_against_50_digits against the same H4_K and the
    same 1e-6 px: every input is an item of its four matches plus one more, one trial, the row (0, 1, 2, 3). Measured on
    the MI355X: max e_gpu / e_ref = 0.003827 over these 64, and every model equal to the host build's bit for bit (the
    hypothesis is evaluated operation for operation as written on both; the host build's maximum over the 300 is 0.006158)."""
    idx, H50, e_ref, keep = T.golden_yardstick()
    m = T.hypothesis_inputs()
    items = []
    for i in idx:
        five = np.concatenate([m[i], m[i][:1]])
        items.append(dict(points2D1=five[:, :2], points2D2=five[:, 2:], max_trials=1, samples=np.array([[0, 1, 2, 3]], np.int32),
                          max_reproj_error=4.0, probability=0.99, stop_num_inliers=0, seed=0))
    recs = gpu_run(mavba, items)
    Hs = np.array([r["trial_models"].reshape(9) for r in recs])
    T.check_hypotheses(Hs, idx, H50, e_ref, keep, "gpu")
    # the device build evaluates the hypothesis operation for operation as the host build does
    Hh, _ = T.host_models(m[idx])
    assert Hs.tobytes() == Hh.tobytes()


def test_degenerate_inputs_terminate_and_classify(mavba):
    items = T.degenerate_items()
    T.check_degenerate(dict(zip(items, gpu_run(mavba, list(items.values())))))


GATE_SEED = 42  # chosen on the CPU (host build and restatement): the planar pair's share is 0.942, the parallax pair's 0.097


def test_the_gate_keeps_the_parallax_pair_and_the_chain_goes_on(mavba):
    """One planar and one parallax pair of 257 matches in one batch, with the mapper's stop: the numpy restatement of the
    whole run on the library's rows gives the same best trial, trials used and mask; view_change_pairs keeps exactly the
    parallax pair, and relative_pose_ransac finds its pose. (The planar pair has 5 % outliers, not the generator's 30 %:
    with 30 % moved by at least three thresholds no homography explains 90 % of a pair.)"""
    stop = mavba.view_change_stop(257, 0.7)
    keys = ("points2D1", "points2D2", "camera_params1", "camera_params2", "max_reproj_error", "probability", "seed")
    pairs = [T.make_item(257, seed=GATE_SEED, kind="planar", outlier_frac=0.05), T.make_item(257, seed=GATE_SEED, kind="parallax")]
    items = [dict({k: p[k] for k in keys}, max_trials=100, stop_num_inliers=stop) for p in pairs]
    rows = [np.array([T.py_sample(int(it["seed"]), t, 257) for t in range(100)]) for it in items]  # the rows the library draws
    restated = [T.restated_ransac(it, r) for it, r in zip(items, rows)]
    for rs in restated:
        assert not np.any(np.abs(rs["residuals"] - 4.0) <= 1e-6 * 4.0)  # (no match of the best model at the threshold)
    # the restatement alone, before the library's numbers are read
    assert restated[0]["replay"]["num_inliers"] / 257 >= 0.9 and restated[1]["replay"]["num_inliers"] / 257 <= 0.5
    results = mavba.homography_ransac(items)
    for res, rs, r in zip(results, restated, rows):
        assert res.ok and np.array_equal(res.trial_samples, r)
        assert res.best_trial == rs["replay"]["best_trial"] and res.trials_used == rs["replay"]["trials_used"]
        assert np.array_equal(res.inlier_mask, rs["mask"]) and res.num_inliers == rs["replay"]["num_inliers"]
        assert res.inlier_ratio == res.num_inliers / 257.0
    assert results[0].trials_used < 100  # (the stop ended the planar pair's run)
    kept = mavba.view_change_pairs(items, results, 0.7)
    assert kept == [1]
    rel, = mavba.relative_pose_ransac([{k: v for k, v in items[q].items() if k != "max_trials" and k != "stop_num_inliers"} for q in kept])
    assert rel.ok and rel.cheirality_best >= 0 and np.isfinite(rel.rvec).all() and np.isfinite(rel.tvec).all()
    assert abs(rel.tvec[0]) >= 0.9 * np.linalg.norm(rel.tvec)  # a sideways baseline
