"""mavba_absolute_pose_ransac on the GPU (csrc/absolute_pose.hip) with the checker and the generators of
tests/test_absolute_pose_host.py: the hypothesis bound on 64 of the 300 inputs, the properties of every model, counts,
sums and the replayed selection per item, bit-reproducibility, NULL outputs, degenerate inputs, and the chain into
mavba_pose_refine_batch.

Sizes: n in {5, 63, 64, 65, 255, 256, 257, 513} - the edges of a wave (64) and of the last work-group's stride (256);
max_trials in {1, 3, 500} and 15, 16, 17 around the 16 trials one work-group takes - alone, and mixed in one batch
with an n = 0 and an n = 4 item in the middle."""

import numpy as np
import pytest

from mavmap_amd import _abi as A
from mavmap_amd import synth
from tests import test_absolute_pose_host as T

pytestmark = pytest.mark.gpu

SIZES = (5, 63, 64, 65, 255, 256, 257, 513)
TRIALS = (1, 3, 15, 16, 17, 500)
MODEL_OF = (A.MODEL_PINHOLE, A.MODEL_OPENCV, A.MODEL_CATA)
_cache = {}


def case(n, mt):
    """One item - generated once, shared by the tests, never modified. Supplied rows and a stop alternate over the grid."""
    key = (n, mt)
    if key not in _cache:
        k = SIZES.index(n) + TRIALS.index(mt)
        _cache[key] = T.make_item(n, MODEL_OF[k % 3], seed=31, max_trials=mt, stop_frac=(None, 0.8, None, 1.0)[k % 4], supplied=k % 2 == 1)
    return _cache[key]


def gpu_run(mavba, items, outputs=T.OUTPUTS, fill=None):
    arr, outs, hold = T.c_items(items, outputs, fill)
    rc = mavba.load().mavba_absolute_pose_ransac(len(items), arr, -1)
    assert rc == A.OK, mavba.load().mavba_last_error()
    return T.records(arr, outs)


def same_bits(a, b, skip=("kernel_seconds",)):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a if k not in skip)


def mixed_batch():
    order = [(513, 500), (5, 3), (64, 17), (255, 1), "n0", (257, 16), "n4", (63, 500), (256, 15), (65, 500), (5, 500)]
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
        if len(it["points2D"]) > 4:
            T.check_record(rec, it, what=f"batch n={len(it['points2D'])} trials={it['max_trials']}")
        else:
            assert rec["status"] == A.ABSPOSE_NO_CONSENSUS and rec["trials_used"] == 0 and np.isnan(rec["proj_matrix"]).all()
    again = gpu_run(mavba, items)
    assert all(same_bits(a, b) for a, b in zip(recs, again))                      # a call gives the same bits twice
    rev = gpu_run(mavba, items[::-1])[::-1]
    assert all(same_bits(a, b) for a, b in zip(recs, rev))                        # ... in the reversed batch
    for q in (0, 2, 5, 7, 9):
        alone, = gpu_run(mavba, [items[q]])
        assert same_bits(recs[q], alone), q                                       # ... and alone


def test_null_outputs_leave_the_others_unchanged(mavba):
    items = [case(257, 17), case(65, 500), T.degenerate_items()["n4"]]
    full = gpu_run(mavba, items)
    for name in T.OUTPUTS:
        part = gpu_run(mavba, items, outputs=tuple(o for o in T.OUTPUTS if o != name), fill=-7)
        for f, p in zip(full, part):
            assert same_bits({k: v for k, v in f.items() if k != name}, {k: v for k, v in p.items() if k != name}), name
            assert np.all(p[name] == (-7 % 256 if p[name].dtype == np.uint8 else -7)), name   # (not handed over: not written)
    none = gpu_run(mavba, items, outputs=())
    for f, p in zip(full, none):
        assert all(np.asarray(f[k]).tobytes() == np.asarray(p[k]).tobytes() for k in ("rvec", "tvec", "proj_matrix", "num_inliers", "best_trial", "trials_used", "status"))


def test_hypothesis_bound_on_64_of_the_300_inputs(mavba):
    """The kernel's model of 64 of the 300 inputs of T.test_hypothesis_against_50_digits against the same P3P_K: every
    input is an item of its four points plus one more, one trial, the row (0, 1, 2, 3). Measured on the MI355X:
    max e_gpu / e_ref = 1.237 over these 64, and every model equal to the host build's bit for bit (the hypothesis is
    evaluated operation for operation as written on both; the host build's maximum over the 300 is 1.4405)."""
    idx, M50, e_ref, keep = T.golden_yardstick()
    scenes = T.hypothesis_scenes()
    items = []
    for i in idx:
        sc = scenes[i]
        items.append(dict(camera_params=sc["camera_params"], points2D=np.concatenate([sc["points2D"], sc["points2D"][:1]]),
                          points3D=np.concatenate([sc["points3D"], sc["points3D"][:1]]), max_trials=1, samples=np.array([[0, 1, 2, 3]], np.int32),
                          max_reproj_error=4.0, probability=0.99, stop_num_inliers=0, seed=0))
    recs = gpu_run(mavba, items)
    M = np.array([r["trial_models"].reshape(12) for r in recs])
    T.check_hypotheses(M, idx, M50, e_ref, keep, "gpu")
    T.check_models(M, "gpu hypotheses")
    # the device build evaluates the hypothesis operation for operation as the host build does
    x2d, X = T.hypothesis_inputs()
    Mh, _ = T.host_models(x2d[idx], X[idx])
    assert M.tobytes() == Mh.tobytes()


def test_degenerate_inputs_terminate_and_classify(mavba):
    items = T.degenerate_items()
    T.check_degenerate(dict(zip(items, gpu_run(mavba, list(items.values())))))


def _restated_ransac(item, rows):
    """The numpy restatement of the whole run on the given rows: (best model [12], mask, trials used)."""
    n = len(item["points2D"])
    xy, thr = T.lift(item)
    xyz = A.as_f64(item["points3D"], (-1, 3))
    models = [T.ref_p3p(xy[r], xyz[r])["model"] for r in rows]
    valid = np.array([m is not None and np.isfinite(m).all() for m in models])
    M = np.array([m if v else np.zeros(12) for m, v in zip(models, valid)])
    res = T.ref_residuals(M, xy, xyz)
    inl = (res <= thr) & valid[:, None]
    rp = T.replay_selection(valid, inl.sum(axis=1), np.where(inl, res, 0.0).sum(axis=1), n, int(item["stop_num_inliers"]), item["probability"])
    b = rp["best_trial"]
    assert not np.any(np.abs(res[b] - thr) <= 1e-6 * thr)  # (no match of the best model at the threshold)
    return M[b], inl[b].astype(np.uint8), rp


@pytest.mark.parametrize("model", [A.MODEL_PINHOLE, A.MODEL_OPENCV])
def test_chain_into_pose_refinement(mavba, model):
    """absolute_pose_ransac -> to_pose_refine_items -> pose_refinement_batch against pose_refinement_batch started from the
    numpy restatement's best model with the restatement's mask: the masks equal, the refined poses within the tolerance
    tests/test_gpu_parity.py uses for pose refinement (1e-6 relative on the pose and on the final cost)."""
    from tests.conftest import rel_err
    item = T.make_item(257, model, seed=41, max_trials=500)
    item = {k: v for k, v in item.items() if k in ("camera_params", "points2D", "points3D", "max_trials", "max_reproj_error", "probability",
                                                   "stop_num_inliers", "seed")}
    res, = mavba.absolute_pose_ransac([item])
    assert res.ok and res.num_inliers >= 0.6 * 257
    Mb, mask, rp = _restated_ransac(item, res.trial_samples)
    assert rp["best_trial"] == res.best_trial and rp["trials_used"] == res.trials_used
    assert np.array_equal(res.inlier_mask, mask)
    chain = mavba.to_pose_refine_items([item], [res])
    assert len(chain) == 1 and chain[0]["index"] == 0 and np.array_equal(chain[0]["inlier_mask"], mask)
    ref = [dict(chain[0], rvec=synth.log_so3(Mb.reshape(3, 4)[:, :3]), tvec=Mb[[3, 7, 11]].copy())]
    (c1, r1), = mavba.pose_refinement_batch(chain)
    (c2, r2), = mavba.pose_refinement_batch(ref)
    assert r1["termination"] == r2["termination"]
    assert abs(r1["final_cost"] - r2["final_cost"]) <= 1e-6 * r2["final_cost"]
    assert rel_err(np.concatenate([chain[0]["rvec"], chain[0]["tvec"]]), np.concatenate([ref[0]["rvec"], ref[0]["tvec"]])) < 1e-6
    assert abs(c1 - c2) < 1e-6 * c2
