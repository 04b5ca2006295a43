"""The point back-substitution on wave tiles (k_backsub_points_tiles, candidate cost folded in) against the CPU oracle and against
the block kernel (MAVBA_BACKSUB_BLOCKS=1) on identical inputs.

A tile holds at most 64 observations and at most 64 points; a point with more is a tile of its own, walked in chunks of 64 with
the sum carried by lane 0. The scene is the long-track scene of tests/test_gpu_limits.py (320 images, 600 points) with the
longest tracks trimmed to exactly 63, 64 (fills a tile alone), 65 (ONE lane in the second chunk), 128 (two full chunks) and 129
views; the other 595 points have six views. Points of more than 16 views sort behind all the others in the session's point
order: the 595 six-view points make 59 tiles of ten points and one of five, and the last five tiles are single points.

Tolerances are the suite's (tests/test_gpu_limits.py): S, v and the model cost change 1e-9, LM step 1e-8 per parameter group and
per long point, a 3-iteration solve 1e-6; every step test measures the oracle's own floor (dense against sparse solver, Jets
against the analytic Jacobian) and asserts that it is at most a tenth of the tolerance it applies.
"""
import functools

import numpy as np
import pytest

from mavmap_amd import _abi as A
from tests.conftest import assert_params_close, global_opts, rel_err
from tests.test_gpu_limits import RADII, _gpu_step, _tolerance, long_track_scene, step_errors

pytestmark = pytest.mark.gpu

LENGTHS = (63, 64, 65, 128, 129)
VARIANTS = {
    "mixed": dict(),
    "fixed_intr": dict(refine_camera_params=False),
    "not_free": dict(),  # points 130 .. 149 constant: the 65-view point (142) among them
}


@functools.lru_cache(maxsize=None)
def _scene(key):
    """(problem, {track length: point}); shared between the tests: nobody writes into it."""
    p, ids = long_track_scene(LENGTHS, models=[A.MODEL_PINHOLE, A.MODEL_OPENCV], seed=101, **VARIANTS[key])
    if key == "not_free":
        p.point_const[130:150] = 1
        assert 130 <= ids[65] < 150
    return p, ids


@functools.lru_cache(maxsize=None)
def _oracle_step(oracle, key, radius):
    p, ids = _scene(key)
    ref = oracle.linear_step(p, radius)
    with oracle.linear_solver(oracle.SPARSE):
        sparse = oracle.linear_step(p, radius)
    analytic = oracle.linear_step(p, radius, jac_mode=1)
    a, b = step_errors(sparse, ref, p, ids), step_errors(analytic, ref, p, ids)
    return ref, {k: max(a[k], b[k]) for k in a}


@functools.lru_cache(maxsize=None)
def _oracle_solve(oracle, key, radius0):
    """Three LM iterations of the oracle from the scene's parameters."""
    p, _ = _scene(key)
    po = p.copy()
    ro, eo = oracle.solve(po, oracle.options(**_opts(radius0)), want_point_errors=True)
    return po, ro, eo


@pytest.fixture(scope="module", autouse=True)
def _release_shared_references():
    yield
    _oracle_step.cache_clear()
    _oracle_solve.cache_clear()
    _scene.cache_clear()


def _opts(radius0):
    kw = dict(max_num_iterations=3)
    if radius0:
        kw["initial_trust_region_radius"] = radius0
    return global_opts(**kw)


def test_scene_and_its_tiles():
    from mavmap_amd import api
    p, ids = _scene("mixed")
    cnt = np.bincount(p.obs_point, minlength=p.num_points)
    assert sorted(ids) == sorted(LENGTHS) and all(cnt[ids[n]] == n for n in LENGTHS)
    assert p.num_points == 600 and (cnt == 6).sum() == 595
    # the session's order: the points of at most 16 views (here: all of six), then the long ones
    order = np.concatenate([np.full(595, 6), sorted(LENGTHS)])
    tiles = api.backsub_tiles(np.concatenate([[0], np.cumsum(order)]))
    assert len(tiles) == 65 and (tiles[:59, 1] == 10).all() and tiles[59, 1] == 5 and (tiles[60:, 1] == 1).all()
    assert tuple(tiles[-1, [1, 3]]) == (1, 129)


@pytest.mark.parametrize("key", sorted(VARIANTS))
def test_linear_step_matches_oracle_and_the_block_kernel(mavba, oracle, key, monkeypatch):
    p, ids = _scene(key)
    for radius in RADII:
        ref, floor = _oracle_step(oracle, key, radius)
        high = {k: v for k, v in floor.items() if not v <= 0.1 * _tolerance(k)}
        assert not high, ("the oracle's own floor is too near the tolerance: change the scene", key, radius, high)
        monkeypatch.delenv("MAVBA_BACKSUB_BLOCKS", raising=False)
        st, info, timers = _gpu_step(mavba, p, radius)
        assert "backsub_points" in timers and "cost_only" not in timers, timers  # the cost rides in the tile kernel
        errs = step_errors(st, ref, p, ids)
        print(f"{key} radius {radius:g}: " + ", ".join(f"{k} {v:.1e} (floor {floor[k]:.1e})" for k, v in errs.items()))
        bad = {k: v for k, v in errs.items() if not (v == 0.0 if _tolerance(k) == 0.0 else v < _tolerance(k))}
        assert not bad, (key, radius, bad)
        if key == "fixed_intr":
            assert not st["d_intr"].any()
        if key == "not_free":
            assert not st["d_points"][130:150].any()
        # route equality: per-point results are the same sequence of operations on both routes
        monkeypatch.setenv("MAVBA_BACKSUB_BLOCKS", "1")
        blocks, _, _ = _gpu_step(mavba, p, radius)
        for name in ("d_points", "d_poses", "d_intr"):
            assert np.array_equal(st[name], blocks[name]), (key, radius, name, np.abs(st[name] - blocks[name]).max())
        # the scalar sums only regroup (rows of the tile kernel against rows of the block kernel): two orders of summing
        # n <= 1000 terms t differ by at most 2 n eps sum|t| = 2.2e-13 sum|t|; the bound allows sum|t| = 50 |sum t|
        assert abs(st["model_cost_change"] - blocks["model_cost_change"]) <= 1e-11 * abs(blocks["model_cost_change"])


def _assert_solve(rg, pg, eg, po, ro, eo, ids, live=None):
    assert ro["num_unsuccessful_steps"] == 0, ro  # (a rejected step's acceptance test compares nearly equal numbers)
    assert rg["termination"] == ro["termination"], (rg["termination_name"], ro["termination_name"])
    assert rg["num_successful_steps"] == ro["num_successful_steps"] and rg["num_unsuccessful_steps"] == ro["num_unsuccessful_steps"]
    for k in ("num_residuals", "num_residuals_reduced", "num_parameters_reduced"):
        assert rg[k] == ro[k], k
    assert abs(rg["initial_cost"] - ro["initial_cost"]) <= 1e-10 * ro["initial_cost"]
    assert abs(rg["final_cost"] - ro["final_cost"]) <= 1e-6 * ro["final_cost"]
    assert abs(rg["final_trust_region_radius"] - ro["final_trust_region_radius"]) <= 1e-6 * ro["final_trust_region_radius"]
    live = np.ones(len(po.points), bool) if live is None else live
    assert_params_close(dict(poses=pg["poses"], intrinsics=pg["intrinsics"], points=pg["points"][live]),
                        dict(poses=po.poses, intrinsics=po.intrinsics, points=po.points[live]))
    m = ~np.isnan(eo)
    assert np.array_equal(m, ~np.isnan(eg)) and rel_err(eg[m], eo[m]) < 1e-6
    for n, q in ids.items():
        if live[q]:
            assert m[q] and abs(eg[q] - eo[q]) < 1e-6 * eo[q], (n, eg[q], eo[q])
            assert rel_err(pg["points"][q], po.points[q]) < 1e-6, n


@pytest.mark.parametrize("blocks", [False, True], ids=["tiles", "blocks"])
@pytest.mark.parametrize("key", ["mixed", "not_free"])
def test_three_lm_iterations_match_oracle(mavba, oracle, key, blocks, monkeypatch):
    """From radius 1e5 the oracle's final radius is 9.35e5 (mixed) / 13.4e5 (not_free): not one of the fixed factors 3, 9, 27 but
    a smooth function of the last candidate's cost (tests/test_gpu_limits.py) - one observation left out or counted twice
    moves it by about 1e-4."""
    p, ids = _scene(key)
    if blocks:
        monkeypatch.setenv("MAVBA_BACKSUB_BLOCKS", "1")
    else:
        monkeypatch.delenv("MAVBA_BACKSUB_BLOCKS", raising=False)
    for radius0 in (None, 1e5):
        po, ro, eo = _oracle_solve(oracle, key, radius0)
        assert ro["num_successful_steps"] == 3
        pg = p.copy()
        eg = np.full(p.num_points, np.nan)
        _, rg = mavba.bundle_adjustment(pg, dict(_opts(radius0)), point3D_errors=eg)
        _assert_solve(rg, dict(poses=pg.poses, intrinsics=pg.intrinsics, points=pg.points), eg, po, ro, eo, ids)
        if radius0:
            ratio = ro["final_trust_region_radius"] / radius0  # (not one of the fixed factors 3^k: the cost decides)
            assert 1.0 < ratio < 27.0 and min(abs(ratio - f) for f in (3.0, 9.0, 27.0)) > 0.05, ratio


def test_filter_of_the_longest_point_on_the_resident_session_matches_oracle(mavba, oracle, monkeypatch):
    """The 129-view point leaves the resident session (its residual blocks get zero weight: the chunked tile still walks its
    three chunks, its cost lanes add nothing); the oracle solves a fresh problem without it."""
    from tests.test_gpu_filter import _drop_points
    monkeypatch.delenv("MAVBA_BACKSUB_BLOCKS", raising=False)
    p, ids = _scene("mixed")
    opts = _opts(None)
    keep = np.ones(p.num_points, np.uint8)
    keep[ids[129]] = 0
    with mavba.Session(p, opts) as s:
        s.solve()
        removed, _ = s.filter_points(0.0, keep)  # every point's error exceeds 0: all that `keep` does not hold go
        assert list(np.nonzero(removed)[0]) == [ids[129]]
        cur = p.copy()
        cur.poses, cur.intrinsics, cur.points = s.get_params()
        q = _drop_points(cur, removed)
        ro, eo = oracle.solve(q, oracle.options(**opts), want_point_errors=True)
        rg = s.solve()
        poses, intr, pts = s.get_params()
        eg = s.point_errors()
    live = removed == 0
    _assert_solve(rg, dict(poses=poses, intrinsics=intr, points=pts), eg, q, ro, eo, ids, live=live)
    assert rel_err(pts[~live], cur.points[~live]) < 1e-6  # nothing references it any more
    assert not (~np.isnan(eo))[~live].any()
