"""mavba_relative_pose_ransac on the GPU (csrc/relative_pose.hip) with the checker and the generators of
tests/test_relative_pose_host.py: the hypothesis bound on 64 of the 300 inputs, the properties of every model, counts,
sums and the replayed selection per item, the pose, bit-reproducibility, NULL outputs, degenerate inputs, and the chain
into mavba_triangulate_pairs.

Sizes: n in {6, 63, 64, 65, 257} - the smallest item, the edges of a wave (64) and of the last work-group's stride
(256); max_trials in {1, 15, 16, 17, 64} around the 16 trials one work-group takes - alone, and mixed in one batch with
an n = 0 and an n = 5 item in the middle; two items of 1000 trials: one that uses them all (four passes of the selection
replay's 256 trials) and one whose run ends in the third pass."""

import numpy as np
import pytest

from mavmap_amd import _abi as A
from mavmap_amd import synth
from tests import test_relative_pose_host as T

pytestmark = pytest.mark.gpu

SIZES = (6, 63, 64, 65, 257)
TRIALS = (1, 15, 16, 17, 64)
MODEL_OF = ((A.MODEL_PINHOLE, A.MODEL_PINHOLE), (A.MODEL_OPENCV, A.MODEL_PINHOLE), (A.MODEL_CATA, A.MODEL_OPENCV))
_cache = {}


def case(n, mt):
    """One item - generated once, shared by the tests, never modified. Supplied rows and a stop alternate over the grid."""
    key = (n, mt)
    if key not in _cache:
        k = SIZES.index(n) + TRIALS.index(mt)
        _cache[key] = T.make_item(n, *MODEL_OF[k % 3], seed=31, max_trials=mt, stop_frac=(None, 0.6, None, 1.0)[k % 4], supplied=k % 2 == 1)
    return _cache[key]


def gpu_run(mavba, items, outputs=T.OUTPUTS, fill=None):
    arr, outs, hold = T.c_items(items, outputs, fill)
    rc = mavba.load().mavba_relative_pose_ransac(len(items), arr, -1)
    assert rc == A.OK, mavba.load().mavba_last_error()
    return T.records(arr, outs)


def same_bits(a, b, skip=("kernel_seconds", "rvec")):
    """(rvec goes through atan2, which the host's and the device's libraries may round differently)"""
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a if k not in skip)


def proper(n, mt):
    """A consensus and an unambiguous pose are expected of a real scene once there are matches and trials to find them."""
    return n >= 63 and mt >= 15


@pytest.mark.parametrize("mt", TRIALS)
@pytest.mark.parametrize("n", SIZES)
def test_single_item(mavba, n, mt):
    item = case(n, mt)
    rec, = gpu_run(mavba, [item])
    T.check_record(rec, item, what=f"n={n} trials={mt}", proper=proper(n, mt))
    assert rec["kernel_seconds"] > 0
    host, = T.host_run([item])
    assert same_bits(rec, host)  # the host build of the same header, operation for operation


def thousand_trials_full_run():
    """The reference's 1000 trials, none ending the run: probability = 1 puts the dynamic limit of every count these models
    reach (at most ~ 0.75 n) above 3000, and stop_num_inliers = n + 1 never stops. The replay walks all four chunks of 256."""
    item = T.make_item(257, A.MODEL_OPENCV, A.MODEL_OPENCV, seed=34, max_trials=1000, probability=1.0)
    item["stop_num_inliers"] = 258
    return item


def thousand_trials_ending_in_the_third_chunk():
    """1000 supplied rows: the first 600 of mismatched pairs only (counts of a few matches, limits in the millions), the others
    of true matches only: the first of those at or past the dynamic limit of its count (~ 25) ends the run, in the replay's
    third chunk."""
    item = T.make_item(257, A.MODEL_PINHOLE, A.MODEL_OPENCV, seed=36, max_trials=1000)   # (seed 35 has a residual at the threshold)
    bad, good = np.flatnonzero(item["outlier"]), np.flatnonzero(~item["outlier"])
    rng = np.random.default_rng(36)
    item["samples"] = np.array([rng.permutation(bad if t < 600 else good)[:5] for t in range(1000)], np.int32)
    return item


def test_thousand_trials_full_run(mavba):
    """All 1000 trials are used: the vectorised property, score and replay checks, the best (trial, model) against the replay."""
    item = thousand_trials_full_run()
    rec, = gpu_run(mavba, [item])
    rp = T.check_record(rec, item, what="1000 trials, full run")
    assert rec["status"] == A.RELPOSE_OK and rec["num_inliers"] >= 0.6 * 257
    assert rp["end"] is None and rec["trials_used"] == 1000
    assert np.count_nonzero(rec["trial_num_inliers"].max(axis=1) == rec["num_inliers"]) >= 1 and rec["best_trial"] == rp["best_trial"]


def test_thousand_trials_ending_in_the_third_chunk(mavba):
    """The run ends at a trial between 600 and 640, and the best model so far comes from no earlier than trial 600."""
    item = thousand_trials_ending_in_the_third_chunk()
    rec, = gpu_run(mavba, [item])
    rp = T.check_record(rec, item, what="1000 trials, ending in the third chunk")
    assert rp["end"] is not None and 600 < rec["trials_used"] == rp["end"][0] + 1 <= 640
    assert rec["status"] == A.RELPOSE_OK and rec["best_trial"] >= 600 and rec["num_inliers"] >= 0.6 * 257
    host, = T.host_run([item])
    assert same_bits(rec, host)


def mixed_batch():
    order = [(257, 64), (6, 17), (64, 17), (63, 1), "n0", (257, 16), "n5", (63, 64), (65, 15), (65, 64), (6, 1)]
    deg = T.degenerate_items()
    return [deg[o] if isinstance(o, str) else case(*o) for o in order]


def test_mixed_batch_alone_reversed_and_twice(mavba):
    items = mixed_batch()
    recs = gpu_run(mavba, items)
    for it, rec in zip(items, recs):
        n, mt = len(it["points2D1"]), it["max_trials"]
        if n > 5:
            T.check_record(rec, it, what=f"batch n={n} trials={mt}", proper=proper(n, mt))
        else:
            T.check_empty(rec, f"batch n={n}")
    again = gpu_run(mavba, items)
    assert all(same_bits(a, b) for a, b in zip(recs, again))                      # a call gives the same bits twice
    rev = gpu_run(mavba, items[::-1])[::-1]
    assert all(same_bits(a, b) for a, b in zip(recs, rev))                        # ... in the reversed batch
    for q in (0, 2, 5, 7, 9):
        alone, = gpu_run(mavba, [items[q]])
        assert same_bits(recs[q], alone), q                                       # ... and alone


def test_null_outputs_leave_the_others_unchanged(mavba):
    items = [case(257, 17), case(65, 64), T.degenerate_items()["n5"]]
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
    """The kernel's models of 64 of the 300 inputs of T.test_hypothesis_against_50_digits against the same E5_K: every
    input is an item of its five correspondences plus one more under a unit pinhole camera, one trial, the row
    (0, 1, 2, 3, 4). Every model equals the host build's bit for bit (the hypothesis is evaluated operation for operation
    as written on both). Measured on the MI355X: max e_gpu / e_ref = 2.224 over these 64 (the host build's maximum over the
    300 is 2.2636), none left out."""
    idx, M50, n50, e_ref, why = T.golden_yardstick()
    x1, x2 = T.hypothesis_inputs()
    items = [T._unit_item(np.concatenate([x1[i], x1[i][:1]]), np.concatenate([x2[i], x2[i][:1]]), max_trials=1,
                          samples=np.array([[0, 1, 2, 3, 4]], np.int32)) for i in idx]
    recs = gpu_run(mavba, items)
    M = np.array([r["trial_models"].reshape(10, 9) for r in recs])
    z = np.array([r["trial_z"].reshape(10) for r in recs])
    nm = np.array([r["trial_num_models"][0] for r in recs])
    T.check_hypotheses(M, nm, idx, M50, n50, e_ref, why, "gpu")
    T.check_model_arrays(M, z, nm, "gpu hypotheses")
    T.check_model_properties(M, nm, x1[idx], x2[idx], "gpu hypotheses")
    # the device build evaluates the hypothesis operation for operation as the host build does
    Mh, zh, nmh, _ = T.host_models(x1[idx], x2[idx])
    assert np.array_equal(nm, nmh) and M.tobytes() == Mh.tobytes() and z.tobytes() == zh.tobytes()


def test_degenerate_inputs_terminate_and_classify(mavba):
    items = T.degenerate_items()
    T.check_degenerate(dict(zip(items, gpu_run(mavba, list(items.values())))))


def test_a_trial_without_a_model_cannot_end_the_run(mavba):
    """A trial without a model at the dynamic limit does not end the run; the outputs equal the host build's bit for bit."""
    it, limit = T.zero_model_item()
    rec, = gpu_run(mavba, [it])
    T.check_zero_model_run(rec, it, limit)
    host, = T.host_run([it])
    assert same_bits(rec, host)


def test_the_second_of_three_models_ends_the_run_and_stop_num_inliers(mavba):
    T.check_second_of_three(lambda items: gpu_run(mavba, items))


def test_reference_fixture(mavba):
    it = T.reference_fixture_item()
    rec, = gpu_run(mavba, [it])
    T.check_reference_fixture(rec, it)


def _restated_ransac(item, rows):
    """The numpy restatement of the whole run on the given rows (no run ends early: see the test): (E, mask, R, t)."""
    p1, p2, thr = T.lift(item)
    best, best_sum, Eb = 0, T.DBL_MAX, None
    for r in rows:
        for E in T.ref_e5(p1[r], p2[r])["models"]:
            res = np.abs(T.ref_residuals(E, p1, p2))
            inl = res <= thr
            c, s = int(inl.sum()), float(res[inl].sum())
            if c > best or (c == best and s < best_sum):
                best, best_sum, Eb = c, s, E
    res = np.abs(T.ref_residuals(Eb, p1, p2))
    assert not np.any(np.abs(res - thr) <= 1e-6 * thr)  # (no match of the best model at the threshold)
    mask = res <= thr
    R, t, _ = T.ref_pose(Eb, p1[mask], p2[mask])
    return Eb, mask.astype(np.uint8), R, t


@pytest.mark.parametrize("models", [(A.MODEL_PINHOLE, A.MODEL_PINHOLE), (A.MODEL_OPENCV, A.MODEL_CATA)])
def test_chain_into_triangulation(mavba, models):
    """relative_pose_ransac -> to_triangulate_pairs -> triangulate_pairs against the same chain started from the numpy
    restatement's pose: the masks equal, mean_folded_angle_deg and num_accepted within 1e-6 relative. probability = 1 leaves
    no dynamic limit within 64 trials, so no run ends early and the order of a trial's models (ascending z in each solver's
    own basis) does not matter."""
    item = T.make_item(257, *models, seed=41, max_trials=64, probability=1.0)
    item = {k: v for k, v in item.items() if k in ("camera_params1", "camera_params2", "points2D1", "points2D2", "max_trials", "max_reproj_error",
                                                   "probability", "stop_num_inliers", "seed")}
    res, = mavba.relative_pose_ransac([item])
    assert res.ok and res.num_inliers >= 0.6 * 257 and res.trials_used == 64
    Eb, mask, R, t = _restated_ransac(item, res.trial_samples)
    assert np.array_equal(res.inlier_mask, mask)
    assert min(np.abs(res.E.reshape(9) - s * Eb).max() for s in (1, -1)) < 1e-6
    chain = mavba.to_triangulate_pairs([item], [res])
    assert len(chain) == 1 and chain[0]["index"] == 0 and np.array_equal(chain[0]["inliers"], np.flatnonzero(mask))
    assert chain[0]["reject"] == A.TRI_REJECT_INITIAL and not np.any(chain[0]["rvec1"]) and not np.any(chain[0]["tvec1"])
    ref = [dict(chain[0], rvec2=synth.log_so3(R), tvec2=np.array(t, float))]
    t1, = mavba.triangulate_pairs(chain)
    t2, = mavba.triangulate_pairs(ref)
    assert np.array_equal(t1.accepted, t2.accepted) and t1.num_accepted == t2.num_accepted > 0.9 * mask.sum()
    assert abs(t1.mean_folded_angle_deg - t2.mean_folded_angle_deg) <= 1e-6 * t2.mean_folded_angle_deg
    assert abs(res.forward_z) < 0.99 and t1.mean_folded_angle_deg > 2.0  # (the mapper's two tests on this pair)
