"""The camera sweep riding in the cluster launch (k_schur_rows<.., SWEEP>) beyond local windows, at every problem size.

Every case solves the same problem twice in one process - MAVBA_SWEEP_RIDE_MAX_OBS=0 (local windows only: the sweep keeps its
own launch) and the variable unset (the sweep rides) - and asks for the same bits: the sweep's work-groups run the same body
on the same chunks and write the same per-chunk partials, so nothing downstream may differ. The shapes are the smallest beyond
the one-work-group route of local windows (more than 64 images or more than 8 192 points) at which each route of the
evaluation is taken; the full-size configurations ride by default in tests/test_gpu_fullsize.py."""
import numpy as np
import pytest

from mavmap_amd import _abi as A
from mavmap_amd import synth
from tests.conftest import global_opts

pytestmark = pytest.mark.gpu

RESULT_KEYS = ("final_cost", "final_gradient_max_norm", "final_trust_region_radius", "num_successful_steps", "num_unsuccessful_steps",
               "termination")
FILTER_MAX_ERROR = 4.0  # (pixels: the generator's gross outliers, +-50 px on 1 % of the observations, lie beyond it)


def _case(name):
    if name in ("gram", "filter", "profiled"):   # 60 images, two cameras, PINHOLE + OPENCV: Gram form of width 8, k_eval_head / k_eval_tail
        return synth.make_config("C3", scale=0.12, seed=33)
    if name == "four_launch_tail":               # more than 160 images: four-launch tail with the partial ride; priors; constant points
        p = synth.make_scene(num_images=170, num_points=9000, track_len=6, models=[A.MODEL_PINHOLE, A.MODEL_OPENCV], seed=34, rot_priors=True)
        p.point_const[::11] = 1
        return p
    if name == "vector":                         # constant intrinsics: the vector form of the sweep
        return synth.make_scene(num_images=70, num_points=9000, track_len=5, models=[A.MODEL_CATA], seed=35, refine_camera_params=False)
    if name == "tail_tiles":                     # a few tracks longer than 16: points behind the clusters (k_point_front beside k_schur_rows)
        return synth.make_scene(num_images=70, num_points=9000, track_len=5, models=[A.MODEL_PINHOLE, A.MODEL_OPENCV], seed=36,
                                long_track_frac=0.004, long_track_len=24)
    if name == "rough":                          # the first case's shape from a rough start: 7 of 32 steps rejected (oracle run of the same scene)
        p = synth.make_config("C3", scale=0.12, seed=33, outlier_frac=0.1)
        rng = np.random.default_rng(5)
        p.poses[2:, :3] += rng.normal(0, 0.15, p.poses[2:, :3].shape)
        p.poses[2:, 3:] += rng.normal(0, 3.0, p.poses[2:, 3:].shape)
        p.points += rng.normal(0, 3.0, p.points.shape)
        return p
    raise KeyError(name)


def _opts(name):
    o = global_opts(initial_trust_region_radius=1e14) if name == "rough" else global_opts()
    if name in ("profiled", "tail_tiles"):
        o["profile_kernels"] = 1
    return o


def _run(mavba, name, p0):
    """linear_step at two radii (the second re-runs the front end without the evaluation), a solve and - `filter` - a
    filter_points pass with a second solve. Returns every array / scalar to compare and the kernel timers."""
    p = p0.copy()
    out = []
    with mavba.Session(p, _opts(name)) as s:
        a = s.linear_step(1e4)
        b = s.linear_step(3e2)
        out += [a["d_poses"], a["d_intr"], a["d_points"], b["d_poses"], b["d_intr"], b["d_points"]]
        r = s.solve()
        out += list(s.get_params()) + [r[k] for k in RESULT_KEYS]
        rejected = r["num_unsuccessful_steps"]
        if name == "filter":
            removed, errors = s.filter_points(FILTER_MAX_ERROR)
            assert 0 < removed.sum() < p.num_points
            r = s.solve()   # (restart(): the first evaluation has no scales and launches the sweep on its own; pt_active form after it)
            out += [removed, errors] + list(s.get_params()) + [r[k] for k in RESULT_KEYS]
            rejected += r["num_unsuccessful_steps"]
        stats = s.kernel_stats()
        info = s.info()
    return out, stats, info, rejected


def _both_ways(mavba, monkeypatch, name):
    p0 = _case(name)
    assert p0.num_images > 64 or p0.num_points > 8192   # (beyond the one-work-group route of local windows)
    runs = {}
    for ride in (False, True):
        if ride:
            monkeypatch.delenv("MAVBA_SWEEP_RIDE_MAX_OBS", raising=False)
        else:
            monkeypatch.setenv("MAVBA_SWEEP_RIDE_MAX_OBS", "0")
        runs[ride] = _run(mavba, name, p0)
    print(name, "images", p0.num_images, "points", p0.num_points, "obs", p0.num_obs, "steps (accepted, rejected)",
          runs[True][0][-3], runs[True][3], "termination", runs[True][0][-1])
    assert len(runs[False][0]) == len(runs[True][0])
    for u, v in zip(runs[False][0], runs[True][0]):
        assert np.array_equal(np.asarray(u), np.asarray(v), equal_nan=True)
    return p0, runs


def test_gram_form_of_width_8(mavba, monkeypatch):
    """60 images, free intrinsics of two models: the Gram form of width 8 rides, the evaluation's tail is k_eval_head /
    k_eval_tail."""
    _both_ways(mavba, monkeypatch, "gram")


def test_rejected_steps(mavba, monkeypatch):
    """The same shape from a rough start and a trust region of 1e14: steps are rejected. Their speculative evaluation - the
    riding sweep included - never ran, the front end runs again for the smaller radius without a sweep, and the books must
    say so."""
    _, runs = _both_ways(mavba, monkeypatch, "rough")
    assert runs[True][3] > 0 and runs[False][3] > 0   # rejected steps did occur


def test_four_launch_tail_with_priors_and_constant_points(mavba, monkeypatch):
    p0, _ = _both_ways(mavba, monkeypatch, "four_launch_tail")
    assert p0.num_images > 160


def test_vector_form_with_constant_intrinsics(mavba, monkeypatch):
    _both_ways(mavba, monkeypatch, "vector")


def test_points_behind_the_clusters(mavba, monkeypatch):
    """Tracks longer than 16 stay behind the clusters: their cost partials sit behind the clusters' ones and the sweep's
    work-groups - appended to the same launch - must not disturb the rows the cost is summed over."""
    p0, runs = _both_ways(mavba, monkeypatch, "tail_tiles")
    for ride in (False, True):
        _, stats, info, _ = runs[ride]
        assert 0 < info["clustered_points"] < p0.num_points
        assert "schur_fused" in stats and "point_front" in stats, stats.keys()   # the fused kernel AND the tail's front end ran


def test_filtered_points_and_a_second_solve(mavba, monkeypatch):
    _both_ways(mavba, monkeypatch, "filter")


def test_profiled_pass_of_a_small_problem_rides(mavba, monkeypatch):
    """Up to 1 000 000 observations the event-timed pass rides like the plain loop. The camera_sweep timer sees the two
    evaluations that have no radius yet, and so no cluster launch to ride in - the one in front of the first linear_step (no
    Jacobi scales either) and the first of the solve (start()) - and nothing after them; with the ride off, every evaluation."""
    _, runs = _both_ways(mavba, monkeypatch, "profiled")
    off, on = runs[False][1], runs[True][1]
    evaluations = lambda st: st.get("camera_reduce", dict(launches=0))["launches"] + st.get("eval_tail", dict(launches=0))["launches"]
    assert evaluations(off) == evaluations(on) > 2
    assert off["camera_sweep"]["launches"] == evaluations(off)
    assert on["scales"]["launches"] == 1
    assert on["camera_sweep"]["launches"] == 2
