"""Invalid LM steps and NUMERICAL_FAILURE: the path "the linear solve failed" against the oracle.

How a step is made invalid, on both sides and without a rounding deciding it:

  whole solves   initial_trust_region_radius = 1, min_lm_diagonal = max_lm_diagonal = -4. Neither side validates options and
                 both clamp the LM diagonal as written, min(max(x, min), max) = -4. With Jacobi scaling every scaled diagonal
                 entry is s / (1 + sqrt(s))^2 < 1, so every damped diagonal entry - of the point blocks and of the reduced
                 system - is <= 1 - 4 / r <= -3 at every radius <= 1: the device's first pivot is negative by a wide margin.
                 The oracle forms sqrt(diag / radius) = NaN and its Cholesky refuses. Different mechanisms, same verdict.
                 Points free: the front end fails first (SC_FAIL_FRONT). All points constant: there is no point block, the
                 failure arises inside the reduced factorisation (SC_FAIL alone) - k_chol_small, k_chol_persist or the
                 launch-per-panel kernels, whichever the session runs.
  single steps   default options and a negative radius, Session.linear_step(-0.5): damped diagonals become -diag. The oracle
                 refuses that radius too; it is only the trigger, never the comparison.

Counts, terminations, radii (only ever divided by powers of two) and untouched parameters are exact; everything else uses
the bar the neighbouring test applies to the same quantity (initial cost 1e-11, steps 1e-8, reduced system 1e-9, point
errors and complete solves 1e-6, the stand-alone factorisation 1e-10)."""
import numpy as np
import pytest

from mavmap_amd import _abi as A
from mavmap_amd import synth
from tests.conftest import assert_params_close, global_opts, rel_err

pytestmark = pytest.mark.gpu

BAD = dict(initial_trust_region_radius=1.0, min_lm_diagonal=-4.0, max_lm_diagonal=-4.0)
# (extra options, termination, unsuccessful steps, final radius): tests/test_oracle.py pins the oracle's side of these
VARIANTS = {"limit_10": (dict(), A.TERM_NUMERICAL_FAILURE, 9, 2.0 ** -45),
            "limit_3": (dict(max_num_consecutive_invalid_steps=3), A.TERM_NUMERICAL_FAILURE, 2, 0.125),
            "min_radius": (dict(min_trust_region_radius=1e-3), A.TERM_PARAMETER_TOLERANCE, 4, 2.0 ** -10)}
RESULT_KEYS = ("termination", "num_successful_steps", "num_unsuccessful_steps", "final_trust_region_radius", "initial_cost", "final_cost",
               "final_gradient_max_norm", "num_residuals", "num_residuals_reduced", "num_parameters_reduced")


def bad_opts(variant="limit_10"):
    return global_opts(**BAD, **VARIANTS[variant][0])


_scenes, _oracle_cache = {}, {}


def _scene(name, constant_points=False):
    """window: reduced system n <= 128, the merged one-work-group loop (k_chol_small<true>). mid: beyond k_chol_small - the
    persistent factorisation, the speculative loop, k_eval_head / k_eval_tail. large: more than 160 images - the four-launch
    evaluation tail."""
    if name not in _scenes:
        _scenes[name] = {
            "window": lambda: synth.make_scene(num_images=6, num_points=120, track_len=3, models=[A.MODEL_PINHOLE, A.MODEL_OPENCV], seed=31),
            "mid": lambda: synth.make_scene(num_images=40, num_points=800, track_len=4, models=[A.MODEL_OPENCV], seed=5),
            "large": lambda: synth.make_scene(num_images=170, num_points=2000, track_len=4, models=[A.MODEL_PINHOLE, A.MODEL_OPENCV], seed=9),
        }[name]()
    p = _scenes[name].copy()
    if constant_points:
        p.point_const[:] = 1
    return p


def _oracle_solve(oracle, name, constant_points, opts_key, opts):
    """(result, point errors, solved problem) of the oracle, computed once per scene and option set."""
    key = (name, constant_points, opts_key)
    if key not in _oracle_cache:
        q = _scene(name, constant_points)
        r, e = oracle.solve(q, oracle.options(**opts), want_point_errors=True)
        _oracle_cache[key] = (r, e, q)
    return _oracle_cache[key]


def _bits_equal(got, ref, what=""):
    for name in ("poses", "intrinsics", "points"):
        a = got[name] if isinstance(got, dict) else getattr(got, name)
        assert np.array_equal(np.asarray(a), getattr(ref, name)), (what, name)


def _assert_failed_like_oracle(rg, ro, variant, what=""):
    _, termination, unsuccessful, radius = VARIANTS[variant]
    print(what, variant, "device", {k: rg[k] for k in RESULT_KEYS[:6]}, "oracle", {k: ro[k] for k in RESULT_KEYS[:6]})
    assert ro["termination"] == termination and ro["num_unsuccessful_steps"] == unsuccessful and ro["final_trust_region_radius"] == radius
    assert rg["termination"] == ro["termination"], (what, rg["termination_name"], ro["termination_name"])
    assert rg["num_successful_steps"] == ro["num_successful_steps"] == 0, what
    assert rg["num_unsuccessful_steps"] == ro["num_unsuccessful_steps"], (what, rg["num_unsuccessful_steps"], ro["num_unsuccessful_steps"])
    for k in ("num_residuals", "num_residuals_reduced", "num_parameters_reduced"):
        assert rg[k] == ro[k], (what, k)
    assert rg["final_trust_region_radius"] == ro["final_trust_region_radius"], (what, rg["final_trust_region_radius"])
    assert abs(rg["initial_cost"] - ro["initial_cost"]) <= 1e-11 * ro["initial_cost"], what
    assert rg["final_cost"] == rg["initial_cost"], what


def _route(mavba, p, opts):
    """The kernel timers and the set-up's figures of a solve of `p` on a profiled session, and its result."""
    with mavba.Session(p.copy(), dict(opts, profile_kernels=1)) as s:
        r = s.solve()
        return set(s.kernel_stats()), s.info(), r


def _assert_route(name, switch, constant_points, num_points, timers, info):
    """Every case must run the route it is there for; a case that silently runs another one fails here. (No evaluation
    with Jacobi scales ever completes in a failed solve: the size route of the evaluation's tail shows in the speculative
    evaluation, which is enqueued and returns at once.)"""
    planes = switch == "MAVBA_FRONT_PLANES"
    small = name == "window"
    merged = switch != "MAVBA_MERGE"
    assert (info["matrix_dim"] <= 128) == small, info["matrix_dim"]            # k_chol_small: at most two tile columns
    if not small:
        assert info["chol_model_forward_us"] > 0.0                              # the persistent schedule exists for this structure
    # k_chol_small<true> applies the camera update itself: no launch of its own in the merged loop of a window
    assert ("update_cameras" not in timers) == (small and merged), timers
    # constant points sit in no cluster: their front end is k_point_front + k_schur_clusters, and that loop does not speculate
    fused = not planes and not constant_points
    assert info["clustered_points"] == (0 if constant_points else num_points)
    assert ("entries_pose" in timers) == planes and ("schur_fused" in timers) == fused, timers
    assert ("point_front" in timers) == (constant_points and not planes), timers
    speculated = fused and switch != "MAVBA_SPECULATE"
    assert ("lm_tail" in timers) == (speculated and merged), timers
    assert ("lm_snapshot" in timers) == (speculated and not merged), timers
    assert ("eval_small" in timers) == (speculated and small and merged), timers
    assert ("eval_tail" in timers) == (speculated and name == "mid" and merged), timers   # (large: the four launches)
    assert "chol_factor" in timers and "backsub_points" in timers, timers


# ---- 2. whole solves end like the oracle's ------------------------------------------------------------------------------

# (the value each switch takes is the one the existing tests give it; all four are read per solve or per session)
SWITCHES = {"MAVBA_SPECULATE": "0", "MAVBA_MERGE": "0", "MAVBA_FRONT_PLANES": "1", "MAVBA_BACKSUB_BLOCKS": "1"}
# (a window's back-substitution is the block kernel anyway: that switch goes to the scenes it changes something for)
CASES = ([("window", None), ("mid", None), ("large", None)] + [(n, s) for s in list(SWITCHES)[:3] for n in ("window", "mid")] +
         [("mid", "MAVBA_BACKSUB_BLOCKS"), ("large", "MAVBA_BACKSUB_BLOCKS")])


@pytest.mark.parametrize("constant_points", [False, True], ids=["points_free", "points_constant"])
@pytest.mark.parametrize("name,switch", CASES, ids=[f"{n}-{s or 'default'}" for n, s in CASES])
def test_failed_solves_end_like_the_oracle(mavba, oracle, monkeypatch, capfd, name, switch, constant_points):
    """mavba_solve with the bad options: termination, step counts, radius and sizes are the oracle's, the cost is the initial
    one, poses / intrinsics / points come back with the bits they went in with (both write-back branches: NUMERICAL_FAILURE
    skips it, PARAMETER_TOLERANCE after invalid steps writes what the session holds), the point errors are those at the
    input. A bad pivot is not a time-out: nothing is said about falling back. A default-options solve of the same scene in
    the same process then matches the oracle: no state outlives the failure."""
    if switch:
        monkeypatch.setenv(switch, SWITCHES[switch])
    p0 = _scene(name, constant_points)
    what = f"{name} {switch} constant_points={constant_points}"
    timers, info, r_session = _route(mavba, p0, bad_opts())
    _assert_route(name, switch, constant_points, p0.num_points, timers, info)
    for variant in VARIANTS:
        ro, eo, _ = _oracle_solve(oracle, name, constant_points, variant, bad_opts(variant))
        pg, eg = p0.copy(), np.full(p0.num_points, np.nan)
        _, rg = mavba.bundle_adjustment(pg, bad_opts(variant), point3D_errors=eg)
        _assert_failed_like_oracle(rg, ro, variant, what)
        _bits_equal(pg, p0, what)
        m = ~np.isnan(eo)
        assert np.array_equal(m, ~np.isnan(eg)) and rel_err(eg[m], eo[m]) < 1e-6, what
        if variant == "limit_10":   # the profiled session walked the same path
            for k in RESULT_KEYS:
                assert r_session[k] == rg[k], (what, k)
    err = capfd.readouterr().err
    assert "falling back" not in err and "timed out" not in err, err[-2000:]
    # afterwards, in the same process: a solve with the default options, like test_full_solve_matches_oracle
    ro, eo, po = _oracle_solve(oracle, name, constant_points, "global", global_opts())
    pg, eg = p0.copy(), np.full(p0.num_points, np.nan)
    _, rg = mavba.bundle_adjustment(pg, global_opts(), point3D_errors=eg)
    assert rg["termination"] == ro["termination"], (what, rg["termination_name"], ro["termination_name"])
    assert rg["num_successful_steps"] == ro["num_successful_steps"] and rg["num_unsuccessful_steps"] == ro["num_unsuccessful_steps"], what
    assert abs(rg["initial_cost"] - ro["initial_cost"]) <= 1e-10 * ro["initial_cost"]
    assert abs(rg["final_cost"] - ro["final_cost"]) <= 1e-6 * ro["final_cost"]
    assert_params_close(pg, po, what=what)
    m = ~np.isnan(eo)
    assert np.array_equal(m, ~np.isnan(eg)) and rel_err(eg[m], eo[m]) < 1e-6
    err = capfd.readouterr().err
    assert "falling back" not in err and "timed out" not in err, err[-2000:]


# ---- 3. the session's books across a failed solve -----------------------------------------------------------------------

BOOKS = [("window", None, False), ("mid", None, False), ("large", None, False), ("window", "MAVBA_FRONT_PLANES", False),
         ("mid", "MAVBA_FRONT_PLANES", False), ("window", None, True), ("mid", None, True), ("large", None, True)]


def _assert_step_close(st, ref, what):
    for k in ("d_poses", "d_intr", "d_points"):
        assert rel_err(st[k], ref[k]) < 1e-8, (what, k, rel_err(st[k], ref[k]))
    assert abs(st["model_cost_change"] - ref["model_cost_change"]) < 1e-9 * abs(ref["model_cost_change"]), what


@pytest.mark.parametrize("name,switch,constant_points", BOOKS,
                         ids=[f"{n}-{s or 'default'}-{'points_constant' if c else 'points_free'}" for n, s, c in BOOKS])
def test_a_failed_linear_step_leaves_the_session_as_it_was(mavba, oracle, monkeypatch, name, switch, constant_points):
    """linear_step / reduced_system at a negative radius in between good ones: the failure is reported, the next good call
    gives the bits of the one before the failure (the failure slots are cleared, the front end's entries of the failed radius
    are not taken for the good one's), another radius gives the oracle's step, and a solve on that session is a fresh
    session's solve to the last bit."""
    if switch:
        monkeypatch.setenv(switch, SWITCHES[switch])
    p = _scene(name, constant_points)
    what = f"{name} {switch} constant_points={constant_points}"
    ref4, ref3 = oracle.linear_step(p, 1e4), oracle.linear_step(p, 1e3)
    with mavba.Session(p, global_opts()) as s:
        a = s.linear_step(1e4)
        _assert_step_close(a, ref4, what)
        with pytest.raises(mavba.MavbaError):
            s.linear_step(-0.5)
        b = s.linear_step(1e4)
        for k in a:
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), (what, k)
        _assert_step_close(s.linear_step(1e3), ref3, what)
        S, v = s.reduced_system(1e4)
        assert rel_err(S, ref4["S"]) < 1e-9 and rel_err(v, ref4["v"]) < 1e-9, what
        try:   # (assembly only: no factorisation runs, and a front end that fails is free to say so here or not)
            s.reduced_system(-0.5)
        except mavba.MavbaError:
            pass
        with pytest.raises(mavba.MavbaError):
            s.linear_step(-0.5)
        S2, v2 = s.reduced_system(1e4)
        assert np.array_equal(S, S2) and np.array_equal(v, v2), what
        S3, v3 = s.reduced_system(1e3)
        assert rel_err(S3, ref3["S"]) < 1e-9 and rel_err(v3, ref3["v"]) < 1e-9, what
        r = s.solve()
        x = s.get_params()
    with mavba.Session(p, global_opts()) as f:
        r_fresh = f.solve()
        x_fresh = f.get_params()
    for k in RESULT_KEYS:
        assert r[k] == r_fresh[k], (what, k, r[k], r_fresh[k])
    for u, w in zip(x, x_fresh):
        assert np.array_equal(u, w), what
    assert r["num_successful_steps"] > 0


@pytest.mark.parametrize("constant_points", [False, True], ids=["points_free", "points_constant"])
@pytest.mark.parametrize("name", ["window", "mid", "large"])
def test_a_failed_solve_step_by_step_restarted_and_reset(mavba, name, constant_points):
    """On a session with the bad options: iterate(1) until it terminates is one solve() call, restart() and reset() give the
    identical run again, get_params() returns the input bits every time."""
    p = _scene(name, constant_points)
    for variant in VARIANTS:
        _, termination, unsuccessful, radius = VARIANTS[variant]
        with mavba.Session(p, bad_opts(variant)) as s:
            whole = s.solve()
            assert (whole["termination"], whole["num_successful_steps"], whole["num_unsuccessful_steps"], whole["final_trust_region_radius"]) == \
                (termination, 0, unsuccessful, radius), (name, variant, whole)
            runs = []
            for again in (s.reset, s.restart, s.reset):
                again()
                calls = 0
                while True:
                    done, term = s.iterate(1)
                    calls += 1
                    assert done <= 1 and calls <= 12
                    if term != A.TERM_RUNNING:
                        break
                runs.append(s.result())
                _bits_equal(dict(zip(("poses", "intrinsics", "points"), s.get_params())), p, (name, variant))
            for r in runs:
                for k in RESULT_KEYS:
                    assert r[k] == whole[k], (name, variant, k, r[k], whole[k])


# ---- 4. the other entry points ------------------------------------------------------------------------------------------

def _pose_items():
    """Three pose-refinement problems: three camera models, 200 / 256 / 300 inliers (the block is 256 threads wide)."""
    items = []
    for model, inliers, seed in ((A.MODEL_PINHOLE, 200, 3), (A.MODEL_OPENCV, 256, 4), (A.MODEL_CATA, 300, 5)):
        g = synth.make_scene(num_images=4, num_points=600, track_len=3, models=[model], seed=seed)
        img = int(np.argmax(np.bincount(g.obs_image)))
        sel = g.obs_image == img
        uv, xyz = g.obs_uv[sel], g.truth["points"][g.obs_point[sel]]
        assert len(uv) > inliers + 10
        mask = np.zeros(len(uv), np.uint8)
        mask[np.random.default_rng(seed).permutation(len(uv))[:inliers]] = 1
        K = A.MODEL_NUM_PARAMS[model]
        cam = np.concatenate([g.truth["intrinsics"][g.image_camera[img]][:K], [float(model)]])
        items.append(dict(rvec=g.poses[img, :3].copy(), tvec=g.poses[img, 3:].copy(), camera_params=cam, points2D=uv, points3D=xyz, inlier_mask=mask))
    return items


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_pose_refinement_fails_like_the_oracle(mavba, oracle, monkeypatch, variant):
    """The in-kernel trust-region loop of k_pose_refine_batch, the single call and the session path
    (MAVBA_POSE_REFINE_SESSION, read per call) against the oracle's flat one-image problem."""
    from tests.test_gpu_parity import _oracle_pose
    items = _pose_items()
    opts = bad_opts(variant)
    ref = [_oracle_pose(oracle, it, **opts) for it in items]
    copies = lambda: [dict(it, rvec=it["rvec"].copy(), tvec=it["tvec"].copy()) for it in items]  # noqa: E731

    def check(results, got, what):
        for it, g, (cost, res), (pose_o, ro) in zip(items, got, results, ref):
            assert res["num_residuals"] == 2 * int(it["inlier_mask"].sum())
            _assert_failed_like_oracle(res, ro, variant, what)
            assert np.array_equal(g["rvec"], it["rvec"]) and np.array_equal(g["tvec"], it["tvec"]), what
            assert np.array_equal(pose_o, np.concatenate([it["rvec"], it["tvec"]]))   # (the oracle left them alone too)
            assert cost == np.sqrt(res["initial_cost"] / res["num_residuals"])

    batch = copies()
    check(mavba.pose_refinement_batch(batch, opts), batch, "batch")
    for env in (None, "1"):
        if env:
            monkeypatch.setenv("MAVBA_POSE_REFINE_SESSION", env)
        single = copies()
        out = [mavba.pose_refinement(s["rvec"], s["tvec"], s["camera_params"], s["points2D"], s["points3D"], s["inlier_mask"], opts) for s in single]
        check(out, single, f"single, session path {env}")


def test_filter_and_rebundle_after_a_failed_solve(mavba, oracle):
    """mavba_solve_filter_solve with the bad options: both solves end in NUMERICAL_FAILURE with the oracle's counts, the filter
    decides on the errors at the INPUT parameters (what the reference's second call would see), nothing is written back."""
    from tests.test_gpu_filter import _oracle_flow
    p = _scene("window")
    _, e_in, _ = _oracle_solve(oracle, "window", False, "limit_10", bad_opts())
    srt = np.sort(e_in[~np.isnan(e_in)])
    gaps = srt[1:] - srt[:-1]
    lo, hi = len(srt) // 4, 3 * len(srt) // 4
    at = lo + int(np.argmax(gaps[lo:hi]))
    max_error = 0.5 * (srt[at] + srt[at + 1])   # in the widest gap of the middle half: no error is near the threshold
    assert gaps[at] > 1e-3 * max_error
    a, b, removed_o, r1o, r2o, e1o, e2o = _oracle_flow(oracle, p, max_error, **bad_opts())
    assert 0 < removed_o.sum() < p.num_points and np.array_equal(e1o, e_in, equal_nan=True)
    g, eg = p.copy(), np.full(p.num_points, np.nan)
    removed_g, r1g, r2g = mavba.bundle_adjustment_filter_rebundle(g, max_error, bad_opts(), point3D_errors=eg)
    assert np.array_equal(removed_g, removed_o)
    _assert_failed_like_oracle(r1g, r1o, "limit_10", "first solve")
    _assert_failed_like_oracle(r2g, r2o, "limit_10", "second solve")
    assert r2g["num_residuals"] < r1g["num_residuals"]
    _bits_equal(g, p)
    m = ~np.isnan(e2o)
    assert np.array_equal(m, ~np.isnan(eg)) and not m[removed_o == 1].any()
    assert rel_err(eg[m], e2o[m]) < 1e-6


@pytest.mark.parametrize("constant_points", [False, True], ids=["points_free", "points_constant"])
def test_sharded_solve_fails_like_one_rank(mavba, oracle, monkeypatch, capfd, constant_points):
    """MAVBA_GPUS=2 through mavba_solve (ranks as host threads sharing the device): every rank takes the same decisions, the
    call returns, and the outcome is the single rank's and the oracle's (multi_gpu.hip's own untouched write-back and
    point errors at the input)."""
    p = _scene("mid", constant_points)
    monkeypatch.setenv("MAVBA_GPUS", "2")
    monkeypatch.setenv("MAVBA_GPUS_SAME_DEVICE", "1")
    monkeypatch.setenv("MAVBA_GPUS_MIN_OBS", "0")
    for variant in VARIANTS:
        ro, eo, _ = _oracle_solve(oracle, "mid", constant_points, variant, bad_opts(variant))
        pg, eg = p.copy(), np.full(p.num_points, np.nan)
        _, rg = mavba.bundle_adjustment(pg, bad_opts(variant), point3D_errors=eg)
        _assert_failed_like_oracle(rg, ro, variant, f"two ranks, constant_points={constant_points}")
        _bits_equal(pg, p)
        m = ~np.isnan(eo)
        assert np.array_equal(m, ~np.isnan(eg)) and rel_err(eg[m], eo[m]) < 1e-6
    err = capfd.readouterr().err
    assert "falling back" not in err and "timed out" not in err, err[-2000:]


@pytest.mark.parametrize("route", ["host", "device"])
def test_scene_bundle_adjustment_fails_and_keeps_the_scene(mavba, oracle, monkeypatch, route):
    """Scene.bundle_adjustment with the bad options, on the host and on the device-resident route: NUMERICAL_FAILURE with the
    oracle's counts, the scene keeps the parameters it had, point3D_errors are those at these parameters."""
    from tests.test_scene import _fm_from, _fresh_problem, ids, mirror
    monkeypatch.setenv("MAVBA_SCENE", route)
    fm = _fm_from(_scene("window"))
    with mirror(fm) as sc:
        free, fixed, fixed_x = ids(range(2, 6)), ids([0]), ids([1])
        f0 = sc.flatten(free, fixed, fixed_x, refine_camera_params=1)
        q = _fresh_problem(f0)
        ro, eo = oracle.solve(q, oracle.options(**bad_opts()), want_point_errors=True)
        errs = {}
        cost, res = sc.bundle_adjustment(free, fixed, fixed_x, bad_opts(), point3D_errors=errs, refine_camera_params=1)
        _assert_failed_like_oracle(res, ro, "limit_10", f"scene, {route} route")
        assert cost == np.sqrt(res["initial_cost"] / res["num_residuals"])
        f1 = sc.flatten(free, fixed, fixed_x, refine_camera_params=1)
        for k in ("poses", "intrinsics", "points", "image_ids", "camera_ids", "point_ids"):
            assert np.array_equal(f0[k], f1[k]), k
        assert sorted(errs) == sorted(f0["point_ids"].tolist())
        eg = np.array([errs[int(i)] for i in f0["point_ids"]])
        assert not np.isnan(eo).any() and rel_err(eg, eo) < 1e-6
        # and the scene solves like the oracle afterwards
        qo = _fresh_problem(f1)
        ro, _ = oracle.solve(qo, oracle.options(**global_opts()))
        cost, res = sc.bundle_adjustment(free, fixed, fixed_x, global_opts(), refine_camera_params=1)
        assert res["termination"] == ro["termination"] and res["num_successful_steps"] == ro["num_successful_steps"]
        assert abs(res["final_cost"] - ro["final_cost"]) <= 1e-6 * ro["final_cost"]


# ---- 5. stand-alone factorisation: pivots that go bad only through elimination ------------------------------------------

def spd_matrix(n, seed=None):
    """The matrix and right-hand side of test_dense_spd_solve (tests/test_gpu_parity.py)."""
    rng = np.random.default_rng(n if seed is None else seed)
    B = rng.normal(size=(n, n))
    Amat = B @ B.T + n * np.eye(n)
    Amat[np.arange(n), np.arange(n)] += np.arange(n) * 0.5
    return Amat, rng.normal(size=n)


def elimination_pairs(n):
    """(j, k): pivot k on both sides of every step of the block structure (4-pivot steps, 16-pivot blocks, 64-wide tiles, the
    last row), made bad by column j inside the same 4-pivot step, in an earlier step of the same 16-block, and in another
    tile column (only the trailing update carries the failure there)."""
    return [(k - d, k) for k in sorted({3, 4, 15, 16, 63, 64, n - 1}) if k < n for d in (1, 5, 64) if k - d >= 0]


def bad_pivot_matrix(Amat, j, k):
    """Every diagonal entry positive, pivot k = 1 - 2^2 = -3 whatever the order of the sums: rows and columns j and k hold
    nothing but A[j, j] = A[k, k] = 1 and A[k, j] = A[j, k] = 2."""
    Bad = Amat.copy()
    for i in (j, k):
        Bad[i, :] = 0.0
        Bad[:, i] = 0.0
        Bad[i, i] = 1.0
    Bad[j, k] = Bad[k, j] = 2.0
    assert (np.diag(Bad) > 0).all()
    return Bad


def nan_entries(n):
    """Strictly lower entries, and only those (the mirror entry stays a number): first column, last row, beside the diagonal,
    the corner of a diagonal 16 x 16 block, across a tile boundary. The tiled kernels read a diagonal 16 x 16 block right of
    its diagonal; the entry point hands them the caller's lower triangle mirrored, so none of these may go unread."""
    return sorted({(1, 0), (15, 0), (n - 1, 0), (n - 1, n - 2), (n // 2, n // 2 - 1)} | ({(64, 63), (n - 1, 63)} if n > 64 else set()) |
                  ({(79, 64)} if n > 79 else set()))


def failures_reported(mavba, n, Amat, b):
    """Runs every bad matrix of size n and a good solve after each: (failures reported, failures tried, worst error of the
    good solves against numpy)."""
    x0 = np.linalg.solve(Amat, b)
    tried = reported = 0
    worst = 0.0
    bad = [bad_pivot_matrix(Amat, j, k) for j, k in elimination_pairs(n)]
    for i, j in nan_entries(n):
        M = Amat.copy()
        M[i, j] = np.nan
        bad.append(M)
    for M in bad:
        tried += 1
        try:
            mavba.dense_spd_solve(M, b)
        except mavba.MavbaError:
            reported += 1
        worst = max(worst, rel_err(mavba.dense_spd_solve(Amat, b), x0))
    return reported, tried, worst


_PANEL_SNIPPET = r"""
import sys, numpy as np
sys.path.insert(0, {root!r})
import mavmap_amd
from tests import test_gpu_failure_paths as T
reported = tried = 0
after = 0.0
for n in (200, 777):
    A, b = T.spd_matrix(n)
    r, t, w = T.failures_reported(mavmap_amd, n, A, b)
    reported += r; tried += t; after = max(after, w)
print("REPORTED", reported, "OF", tried, "AFTER", after)
for constant_points in (False, True):
    p0 = T._scene("mid", constant_points)
    with mavmap_amd.Session(p0.copy(), T.bad_opts()) as s:
        print("PERSISTENT_MODEL_US", s.info()["chol_model_forward_us"])
    for variant in sorted(T.VARIANTS):
        p = p0.copy()
        _, r = mavmap_amd.bundle_adjustment(p, T.bad_opts(variant))
        same = all(np.array_equal(getattr(p, k), getattr(p0, k)) for k in ("poses", "intrinsics", "points"))
        print("SOLVE", variant, r["termination"], r["num_successful_steps"], r["num_unsuccessful_steps"], repr(r["final_trust_region_radius"]),
              int(r["final_cost"] == r["initial_cost"]), int(same))
"""


def test_the_launch_per_panel_schedule_reports_bad_pivots_too(mavba):
    """MAVBA_CHOL_PERSIST=0 (read once per process, hence the child): no persistent launch, the launch-per-panel kernels
    factorise - stand-alone on the matrices below and inside the sessions of the 40-image scene. The expected counts and
    radii are the oracle's (VARIANTS; tests/test_oracle.py holds the oracle to them)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", _PANEL_SNIPPET.format(root=root)], env=dict(os.environ, MAVBA_CHOL_PERSIST="0"),
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    print(out.stdout)
    words = out.stdout.split("REPORTED")[1].split()
    assert int(words[0]) == int(words[2]) > 40 and float(words[4]) < 1e-10, out.stdout
    models = [float(l.split()[1]) for l in out.stdout.splitlines() if l.startswith("PERSISTENT_MODEL_US")]
    assert models == [0.0, 0.0], models   # no persistent schedule was built: the sessions ran the launch-per-panel kernels
    solves = [l.split()[1:] for l in out.stdout.splitlines() if l.startswith("SOLVE")]
    assert len(solves) == 2 * len(VARIANTS)
    for variant, termination, good, bad, radius, cost_kept, params_kept in solves:
        _, t, n_bad, r = VARIANTS[variant]
        assert (int(termination), int(good), int(bad), float(radius), cost_kept, params_kept) == (t, 0, n_bad, r, "1", "1"), (variant, out.stdout)
    assert "falling back" not in out.stderr and "timed out" not in out.stderr, out.stderr[-2000:]


@pytest.mark.parametrize("n", [65, 128, 200, 777])
def test_dense_spd_solve_reports_pivots_that_elimination_makes_bad(mavba, n):
    """No zero pivot here: the hardware reciprocal square root is not correctly rounded and a sign there is not defined."""
    Amat, b = spd_matrix(n)
    pairs = elimination_pairs(n)
    assert {k for _, k in pairs} >= {3, 4, 15, 16, 63, 64, n - 1} and {k - j for j, k in pairs} == {1, 5, 64}
    for j, k in pairs:   # one by one, so that a miss names its pair
        with pytest.raises(mavba.MavbaError):
            mavba.dense_spd_solve(bad_pivot_matrix(Amat, j, k), b)
            pytest.fail(f"n = {n}: pivot {k} made -3 by column {j} was not reported")
    reported, tried, worst = failures_reported(mavba, n, Amat, b)
    assert reported == tried == len(pairs) + len(nan_entries(n)), (reported, tried)
    assert worst < 1e-10, worst
