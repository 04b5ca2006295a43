"""GPU parity at the sizes where a kernel changes its code path: the HIP path against the CPU oracle on identical inputs.

Every other GPU scene has at most four cameras and tracks of at most 40 views. The limits this module crosses, each through
the public API with valid input:

  kFrontObs = 256 observations of one point   k_point_front walks the point in windows (Jacobians evaluated a second time for
                                              the entry records, sums carried from window to window); tracks of exactly 17,
                                              255, 256, 257 (ONE active lane in the second window) and 300 views
  256 observations of one point               the owner lane of k_backsub_points_packed adds its point over several chunks,
                                              and the candidate's cost walks the same chunks
  kBsCamsLds = 16 cameras                     the back-substitution reads the intrinsics tables from memory, not from LDS
  kFrontQ = 96 refined cameras on one point   the session drops to the plane kernels on its own
  more than 3 cameras on every point          no clusters at all: k_point_front + the generic term lists
  3 camera slots in a cluster                 k_schur_rows<K, GENERIC = true>
  256 inliers                                 the per-lane loops of k_pose_refine_batch make a second trip
  more than 8 cameras in a small window       the window leaves the merged one-work-group LM loop

Tolerances are the suite's (tests/test_gpu_parity.py): cost and Jacobian 1e-11, S and v 1e-9, LM step 1e-8, a 3-iteration
solve 1e-6 per kind of parameter block. Step entries are compared per GROUP - rvec, t, (fx fy cx cy), (k1 k2), (p1 p2), xi of
the cameras that have them, the points, each long point on its own - against the largest reference magnitude of that group.

The oracle's own floor, measured on the host for exactly these scenes as the disagreement of its dense solver with its sparse
one and of its Jets with its analytic Jacobian (largest over the scenes of this module; every step test measures it again and
asserts that it is at most a tenth of the tolerance it then applies):

                                      radius 1e4    radius 30
  S, v                                  <= 3e-14      <= 3e-14
  step, worst group                     <= 1e-10      <= 3e-12     (xi of per_image_track3; k1 k2 of the long-track scene)
  d_points of one long point            <= 5e-12      <= 3e-14
"""
import functools

import numpy as np
import pytest

from mavmap_amd import _abi as A
from mavmap_amd import synth
from mavmap_amd.problem import BAProblem
from tests.conftest import assert_params_close, global_opts, rel_err

pytestmark = pytest.mark.gpu

RADII = (1e4, 30.0)
LONG_LENGTHS = (17, 255, 256, 257, 300)
STEP_TOL = 1e-8
SYSTEM_TOL = 1e-9


# ---- scenes ----------------------------------------------------------------------------------------------------------------

def long_track_scene(lengths, models, seed, short_len=6, **kw):
    """320 images in a dense grid, 600 points of 6 views and some twenty loop-closure tracks of 200 to 316 views: the longest
    are trimmed to exactly `lengths` observations, the other long ones to `short_len`. Returns (problem, {length: point})."""
    p = synth.make_scene(num_images=320, num_points=600, track_len=short_len, long_track_frac=0.03, long_track_len=320,
                         spacing=2.0, models=models, seed=seed, **kw)
    cnt = np.bincount(p.obs_point, minlength=p.num_points)
    long_pts = [int(q) for q in np.argsort(-cnt, kind="stable") if cnt[q] > short_len]
    want = sorted(lengths, reverse=True)
    assert len(long_pts) >= len(want) and all(cnt[q] >= n for q, n in zip(long_pts, want)), (np.sort(cnt)[::-1][:8], want)
    target = {q: short_len for q in long_pts}
    target.update(zip(long_pts, want))
    keep = np.ones(p.num_obs, bool)
    for q, n in target.items():
        idx = np.nonzero(p.obs_point == q)[0]
        chosen = idx[np.linspace(0, len(idx) - 1, n).astype(int)]  # (spread over the track: the views stay far apart)
        keep[idx] = False
        keep[chosen] = True
    p.obs_uv, p.obs_image, p.obs_point = (np.ascontiguousarray(p.obs_uv[keep]), np.ascontiguousarray(p.obs_image[keep]),
                                          np.ascontiguousarray(p.obs_point[keep]))
    del p.truth["uv_clean"]  # (per observation of the untrimmed scene)
    ids = {n: q for q, n in zip(long_pts, want)}
    cnt = np.bincount(p.obs_point, minlength=p.num_points)
    assert all(cnt[q] == n for n, q in ids.items())
    rest = np.delete(cnt, list(ids.values()))
    assert rest.min() == short_len == rest.max()
    return p, ids


def many_camera_scene(kind):
    if kind == "nc17":  # more cameras than the back-substitution keeps in LDS
        models = ([A.MODEL_PINHOLE, A.MODEL_OPENCV, A.MODEL_CATA] * 6)[:17]
        return synth.make_scene(num_images=40, num_points=1500, track_len=4, models=models, seed=71, spacing=5.0,
                                image_camera=np.arange(40) % 17)
    if kind == "per_image_track3":  # one camera per image, three views per point: every cluster has three camera slots
        return synth.make_scene(num_images=40, num_points=1500, track_len=3, models=[1, 2, 3, 2] * 10, seed=76, spacing=5.0,
                                image_camera=np.arange(40))
    if kind == "per_image_120":  # five cameras on every point: no clusters; the longest track has more refined cameras than a tile holds
        return synth.make_scene(num_images=120, num_points=3000, track_len=5, models=[1, 2, 3] * 40, seed=73, spacing=2.0,
                                long_track_frac=0.004, long_track_len=110, image_camera=np.arange(120))
    raise KeyError(kind)


LONG_SCENES = {
    "mixed": dict(models=[A.MODEL_PINHOLE, A.MODEL_OPENCV], seed=101),
    "fixed_intr": dict(models=[A.MODEL_PINHOLE, A.MODEL_OPENCV], seed=101, refine_camera_params=False),  # KMAX = 0
    "cata": dict(models=[A.MODEL_CATA], seed=102),                                                         # K = 9
}


@functools.lru_cache(maxsize=None)
def _scene(key):
    """(problem, {track length: long point}); shared between the tests: nobody writes into it."""
    if key in LONG_SCENES:
        return long_track_scene(LONG_LENGTHS, **LONG_SCENES[key])
    if key == "window9":
        # a local window [FIXED, FIXED, FREE x 10] with nine constant cameras: 60 free columns, one tile column to factorise
        p = synth.make_scene(num_images=12, num_points=900, track_len=4, models=[A.MODEL_OPENCV, A.MODEL_PINHOLE, A.MODEL_CATA] * 3,
                             seed=74, image_camera=np.arange(12) % 9)
        p.pose_const[:] = 0
        p.pose_const[:2] = A.CONST_POSE
        p.intr_const[:] = 1
        return p, {}
    return many_camera_scene(key), {}


@pytest.fixture(scope="module", autouse=True)
def _release_shared_references():
    """The scenes and the oracle's steps (a 1938 x 1938 system each) are computed once for the module, and let go after it."""
    yield
    _oracle_step.cache_clear()
    _scene.cache_clear()


# ---- comparison of a linear step, group by group -----------------------------------------------------------------------------

INTR_GROUPS = (("fxfycxcy", slice(0, 4), (A.MODEL_PINHOLE, A.MODEL_OPENCV, A.MODEL_CATA)), ("k1k2", slice(4, 6), (A.MODEL_OPENCV, A.MODEL_CATA)),
               ("p1p2", slice(6, 8), (A.MODEL_OPENCV, A.MODEL_CATA)), ("xi", slice(8, 9), (A.MODEL_CATA,)))


def step_errors(got, ref, p, long_ids):
    """{quantity: relative error}, every group against the largest reference magnitude of ITS OWN entries."""
    e = {"S": rel_err(got["S"], ref["S"]), "v": rel_err(got["v"], ref["v"]),
         "d_rvec": rel_err(got["d_poses"][:, :3], ref["d_poses"][:, :3]), "d_t": rel_err(got["d_poses"][:, 3:], ref["d_poses"][:, 3:])}
    covered = np.zeros(ref["d_intr"].shape, bool)
    for name, cols, models in INTR_GROUPS:
        cams = np.isin(p.camera_model, models) & (np.asarray(p.intr_const) == 0)
        if cams.any():
            covered[np.ix_(cams, np.arange(9)[cols])] = True
            e["d_" + name] = rel_err(got["d_intr"][cams][:, cols], ref["d_intr"][cams][:, cols])
    # constant cameras and the padding of the smaller models do not move
    e["d_intr_padding"] = float(np.abs(got["d_intr"][~covered]).max()) if (~covered).any() else 0.0
    rest = np.ones(p.num_points, bool)
    rest[list(long_ids.values())] = False
    e["d_points"] = rel_err(got["d_points"][rest], ref["d_points"][rest])
    for n, q in long_ids.items():  # a whole-array maximum would hide them
        e[f"d_point_of_{n}_views"] = rel_err(got["d_points"][q], ref["d_points"][q])
    e["model_cost_change"] = abs(got["model_cost_change"] - ref["model_cost_change"]) / abs(ref["model_cost_change"])
    return e


def _tolerance(quantity):
    return 0.0 if quantity == "d_intr_padding" else SYSTEM_TOL if quantity in ("S", "v", "model_cost_change") else STEP_TOL


@functools.lru_cache(maxsize=None)
def _oracle_step(oracle, key, radius):
    """(the oracle's dense step with Jets, its own floor): the floor is the disagreement of the sparse solver and of the
    analytic Jacobian with that step, quantity by quantity."""
    p, long_ids = _scene(key)
    ref = oracle.linear_step(p, radius)
    with oracle.linear_solver(oracle.SPARSE):
        sparse = oracle.linear_step(p, radius)
    analytic = oracle.linear_step(p, radius, jac_mode=1)
    a, b = step_errors(sparse, ref, p, long_ids), step_errors(analytic, ref, p, long_ids)
    return ref, {k: max(a[k], b[k]) for k in a}


def assert_step(got, oracle, key, radius, what=""):
    p, long_ids = _scene(key)
    ref, floor = _oracle_step(oracle, key, radius)
    high = {k: v for k, v in floor.items() if not v <= 0.1 * _tolerance(k)}
    assert not high, ("the oracle's own floor is too near the tolerance: change the scene", key, radius, high)
    errs = step_errors(got, ref, p, long_ids)
    print(f"{key} {what} radius {radius:g}: " + ", ".join(f"{k} {v:.1e} (floor {floor[k]:.1e})" for k, v in errs.items()))
    bad = {k: v for k, v in errs.items() if not (v == 0.0 if _tolerance(k) == 0.0 else v < _tolerance(k))}
    assert not bad, (key, what, radius, bad)
    return errs


def _gpu_step(mavba, p, radius):
    with mavba.Session(p, dict(profile_kernels=1)) as s:
        info = s.info()
        S, v = s.reduced_system(radius)
        st = s.linear_step(radius)
        timers = set(s.kernel_stats())
    assert np.abs(S - S.T).max() == 0.0
    st.update(S=S, v=v)
    return st, info, timers


def _solve_both(mavba, oracle, p, **optkw):
    po, pg = p.copy(), p.copy()
    ro, eo = oracle.solve(po, oracle.options(**optkw), want_point_errors=True)
    eg = np.full(p.num_points, np.nan)
    _, rg = mavba.bundle_adjustment(pg, dict(optkw), point3D_errors=eg)
    return po, ro, eo, pg, rg, eg


def assert_short_solve(mavba, oracle, p, long_ids=(), **optkw):
    """Three LM iterations on both sides; the oracle must not reject a step (a rejected step's acceptance test is a
    comparison of nearly equal numbers: not what these tests are about)."""
    po, ro, eo, pg, rg, eg = _solve_both(mavba, oracle, p, **global_opts(max_num_iterations=3, **optkw))
    assert ro["num_unsuccessful_steps"] == 0 and ro["num_successful_steps"] == 3, ro
    assert rg["termination"] == ro["termination"], (rg["termination_name"], ro["termination_name"])
    assert rg["num_successful_steps"] == ro["num_successful_steps"] and rg["num_unsuccessful_steps"] == ro["num_unsuccessful_steps"]
    for k in ("num_residuals", "num_residuals_reduced", "num_parameters_reduced"):
        assert rg[k] == ro[k], k
    assert abs(rg["initial_cost"] - ro["initial_cost"]) <= 1e-10 * ro["initial_cost"]
    assert abs(rg["final_cost"] - ro["final_cost"]) <= 1e-6 * ro["final_cost"]
    assert abs(rg["final_trust_region_radius"] - ro["final_trust_region_radius"]) <= 1e-6 * ro["final_trust_region_radius"]
    assert_params_close(pg, po)
    m = ~np.isnan(eo)
    assert np.array_equal(m, ~np.isnan(eg)) and rel_err(eg[m], eo[m]) < 1e-6
    for n, q in dict(long_ids).items():
        assert m[q] and abs(eg[q] - eo[q]) < 1e-6 * eo[q], (n, eg[q], eo[q])
        assert rel_err(pg.points[q], po.points[q]) < 1e-6, n
    return pg, rg


# ---- 1, 2: tracks of more than 256 views through every front end -------------------------------------------------------------

def test_long_track_scene_has_the_exact_lengths():
    p, ids = _scene("mixed")
    cnt = np.bincount(p.obs_point, minlength=p.num_points)
    assert sorted(ids) == sorted(LONG_LENGTHS) and [cnt[ids[n]] for n in LONG_LENGTHS] == list(LONG_LENGTHS)
    assert sorted(cnt)[-5:] == sorted(LONG_LENGTHS) and sorted(cnt)[-6] == 6
    assert p.num_obs <= 16000


def test_long_tracks_default_route_matches_oracle(mavba, oracle):
    """Clusters for the points of six views, the windowed k_point_front + the generic term lists for the five long tracks."""
    p, ids = _scene("mixed")
    c0, r0, Jc0, Jp0, Jk0 = oracle.eval_jacobian(p, jac_mode=0)
    c1 = oracle.eval_jacobian(p, jac_mode=1)[0]
    assert abs(c1 - c0) <= 1e-12 * abs(c0)
    with mavba.Session(p) as s:
        c, r, Jc, Jp, Jk = s.eval_jacobian()
    assert abs(c - c0) <= 1e-11 * abs(c0)
    for name, a, b in (("r", r, r0), ("Jc", Jc, Jc0), ("Jp", Jp, Jp0), ("Jk", Jk, Jk0)):
        assert rel_err(a, b) < 1e-11, (name, rel_err(a, b))
    for radius in RADII:
        st, info, timers = _gpu_step(mavba, p, radius)
        assert info["num_clusters"] > 0 and 0 < info["clustered_points"] < p.num_points and sum(info["schur_terms"]) > 0
        assert "schur_fused" in timers and "point_front" in timers, timers  # the tail took the windowed kernel
        assert_step(st, oracle, "mixed", radius)


@pytest.mark.parametrize("key", sorted(LONG_SCENES))
def test_long_tracks_through_every_front_end(mavba, oracle, key, monkeypatch):
    """The default route, k_point_front for every point with the entry records on (MAVBA_NO_FUSE) and the plane kernels
    (MAVBA_FRONT_PLANES), with free intrinsics of two models, constant intrinsics (KMAX = 0) and CATA cameras only (K = 9):
    each route gives the oracle's step, and the routes give the same system up to the order of their sums."""
    p, ids = _scene(key)
    radius = RADII[1]
    out = {}
    for env in (None, "MAVBA_NO_FUSE", "MAVBA_FRONT_PLANES"):
        if env:
            monkeypatch.setenv(env, "1")
        out[env] = _gpu_step(mavba, p, radius)
        assert_step(out[env][0], oracle, key, radius, what=str(env))
    # the routes really differ
    assert "point_front" in out[None][2]
    assert "schur_fused" not in out["MAVBA_NO_FUSE"][2] and "point_front" in out["MAVBA_NO_FUSE"][2]
    assert "point_front" not in out["MAVBA_FRONT_PLANES"][2] and "entries_pose" in out["MAVBA_FRONT_PLANES"][2]
    S0, v0 = out[None][0]["S"], out[None][0]["v"]
    for env in ("MAVBA_NO_FUSE", "MAVBA_FRONT_PLANES"):
        assert rel_err(out[env][0]["S"], S0) < 1e-11 and rel_err(out[env][0]["v"], v0) < 1e-11, env
    if key == "fixed_intr":
        assert not out[None][0]["d_intr"].any()
    # the other radius on the route every point takes through k_point_front (the mixed scene's default route: the test above)
    if key != "mixed":
        monkeypatch.delenv("MAVBA_FRONT_PLANES")
        assert_step(_gpu_step(mavba, p, RADII[0])[0], oracle, key, RADII[0], what="MAVBA_NO_FUSE")


# ---- 3, 4: the LM loop and the filter over a multi-window point ----------------------------------------------------------------

def test_three_lm_iterations_with_long_tracks_match_oracle(mavba, oracle):
    """The candidate's cost inside the back-substitution walks the chunks of a long point too."""
    p, ids = _scene("mixed")
    assert_short_solve(mavba, oracle, p, ids)
    # From the default radius every step is so good that the radius grows by its largest factor, 3, whatever the candidate's
    # cost is exactly. From 1e8 the third step's quality is about 0.74 (oracle): the final radius is a smooth function of the
    # candidate's cost, and has to agree too.
    pg, rg = assert_short_solve(mavba, oracle, p, ids, initial_trust_region_radius=1e8)
    assert 9.5e8 < rg["final_trust_region_radius"] < 11e8, rg["final_trust_region_radius"]


def test_filter_of_a_long_point_on_the_resident_session_matches_oracle(mavba, oracle):
    """One long and one ordinary point leave the resident session (their residual blocks get zero weight: the MASK
    instantiations walk the windows of the other long points); the oracle solves a fresh problem without them."""
    from tests.test_gpu_filter import _drop_points
    p, ids = _scene("mixed")
    opts = global_opts(max_num_iterations=3)
    cnt = np.bincount(p.obs_point, minlength=p.num_points)
    ordinary = int(np.nonzero(cnt == 6)[0][7])
    gone = [ids[256], ordinary]
    keep = np.ones(p.num_points, np.uint8)
    keep[gone] = 0
    with mavba.Session(p, opts) as s:
        s.solve()
        removed, errs = s.filter_points(0.0, keep)  # every point's error exceeds 0: all that `keep` does not hold go
        assert sorted(np.nonzero(removed)[0]) == sorted(gone)
        cur = p.copy()
        cur.poses, cur.intrinsics, cur.points = s.get_params()
        q = _drop_points(cur, removed)
        ro, eo = oracle.solve(q, oracle.options(**opts), want_point_errors=True)
        rg = s.solve()
        poses, intr, pts = s.get_params()
        eg = s.point_errors()
    assert rg["termination"] == ro["termination"]
    assert rg["num_successful_steps"] == ro["num_successful_steps"] and rg["num_unsuccessful_steps"] == ro["num_unsuccessful_steps"]
    for k in ("num_residuals", "num_residuals_reduced", "num_parameters_reduced"):
        assert rg[k] == ro[k], k
    assert abs(rg["initial_cost"] - ro["initial_cost"]) <= 1e-10 * ro["initial_cost"]
    assert abs(rg["final_cost"] - ro["final_cost"]) <= 1e-6 * ro["final_cost"]
    live = removed == 0
    assert_params_close(dict(poses=poses, intrinsics=intr, points=pts[live]), dict(poses=q.poses, intrinsics=q.intrinsics, points=q.points[live]))
    assert rel_err(pts[~live], cur.points[~live]) < 1e-6  # nothing references them any more
    m = ~np.isnan(eo)
    assert np.array_equal(m, ~np.isnan(eg)) and not m[~live].any() and rel_err(eg[m], eo[m]) < 1e-6
    for n in (17, 255, 257, 300):
        assert abs(eg[ids[n]] - eo[ids[n]]) < 1e-6 * eo[ids[n]] and rel_err(pts[ids[n]], q.points[ids[n]]) < 1e-6, n


# ---- 5: many cameras -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["nc17", "per_image_track3", "per_image_120"])
def test_many_cameras_match_oracle(mavba, oracle, kind):
    p, _ = _scene(kind)
    for radius in RADII:
        st, info, timers = _gpu_step(mavba, p, radius)
        assert_step(st, oracle, kind, radius)
    if kind == "nc17":
        assert p.num_cameras == 17 and set(p.camera_model) == {1, 2, 3}
    if kind == "per_image_track3":
        assert info["num_clusters"] > 0 and info["clustered_points"] > 0
    if kind == "per_image_120":
        imgs = p.obs_image[p.obs_point == np.argmax(np.bincount(p.obs_point))]
        assert len(np.unique(p.image_camera[imgs])) == 110  # more refined cameras on one point than a tile of k_point_front holds
        assert info["num_clusters"] == 0 and sum(info["schur_terms"]) > 0
        assert "entries_pose" in timers and "point_front" not in timers  # the automatic fallback to the plane kernels
    assert_short_solve(mavba, oracle, p)


# ---- 6: a small window with nine cameras ---------------------------------------------------------------------------------------

def test_small_window_with_nine_cameras_matches_oracle(mavba, oracle, monkeypatch):
    """Nine cameras: one more than the merged one-work-group LM loop of a local window takes. The system is still solved by
    k_chol_small (one active tile column); the launch-per-step loop gives the oracle's step and solve, and MAVBA_MERGE = 0
    changes no bit of it."""
    p, _ = _scene("window9")
    assert p.num_cameras == 9 and int((p.pose_const == 0).sum()) == 10
    for radius in RADII:
        st, info, timers = _gpu_step(mavba, p, radius)
        assert info["matrix_dim"] == 64 * ((6 * 12 + 9 * 9 + 63) // 64)
        assert_step(st, oracle, "window9", radius)
        assert not st["d_poses"][:2].any()
    outs = []
    for merge in ("1", "0"):
        monkeypatch.setenv("MAVBA_MERGE", merge)
        q = p.copy()
        e = np.full(p.num_points, np.nan)
        with mavba.Session(q, dict(profile_kernels=1)) as s:
            r = s.solve()
            x = s.get_params()
            e = s.point_errors()
            timers = set(s.kernel_stats())
        assert "eval_small" not in timers, timers  # not the merged one-work-group loop
        outs.append((x[0], x[1], x[2], e, r["final_cost"], r["num_successful_steps"], r["num_unsuccessful_steps"], r["termination"],
                     r["final_gradient_max_norm"], r["final_trust_region_radius"]))
    for a, b in zip(*outs):
        assert np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)
    monkeypatch.delenv("MAVBA_MERGE")
    po, ro, eo, pg, rg, eg = _solve_both(mavba, oracle, p)  # BundleAdjustmentOptions defaults, like a local window
    assert rg["termination"] == ro["termination"]
    assert rg["num_successful_steps"] == ro["num_successful_steps"] and rg["num_unsuccessful_steps"] == ro["num_unsuccessful_steps"]
    assert abs(rg["final_cost"] - ro["final_cost"]) <= 1e-6 * ro["final_cost"]
    assert_params_close(pg, po)
    assert np.array_equal(pg.poses[:2], p.poses[:2]) and np.array_equal(pg.intrinsics, p.intrinsics)


# ---- 7: pose refinement around 256 inliers -------------------------------------------------------------------------------------

POSE_INLIERS = (0, 6, 255, 256, 257, 700)
POSE_SEED = 81


def _pose_size_items(seed=POSE_SEED):
    """One batch, all three camera models in it, inlier sets of exactly POSE_INLIERS observations."""
    g = synth.make_scene(num_images=6, num_points=1500, track_len=3, models=[A.MODEL_PINHOLE, A.MODEL_OPENCV, A.MODEL_CATA], seed=seed)
    rng = np.random.default_rng(seed)
    items = []
    for q, n_in in enumerate(POSE_INLIERS):
        img = 1 + q % (g.num_images - 1)
        model = int(g.camera_model[g.image_camera[img]])
        sel = g.obs_image == img
        uv, xyz = g.obs_uv[sel], g.truth["points"][g.obs_point[sel]]
        assert len(uv) >= n_in, (img, len(uv))
        mask = np.zeros(len(uv), np.uint8)
        mask[rng.choice(len(uv), n_in, replace=False)] = 1
        assert int(mask.sum()) == n_in
        cam = np.concatenate([g.truth["intrinsics"][g.image_camera[img]][:A.MODEL_NUM_PARAMS[model]], [float(model)]])
        pose = g.truth["poses"][img] + rng.normal(0, [0.01] * 3 + [0.3] * 3)
        items.append(dict(rvec=pose[:3].copy(), tvec=pose[3:].copy(), camera_params=cam, points2D=uv, points3D=xyz, inlier_mask=mask))
    assert {int(it["camera_params"][-1]) for it in items} == {1, 2, 3}
    return items


def _oracle_pose(oracle, it, jac_mode=0):
    keep = np.asarray(it["inlier_mask"], bool)
    cam = np.asarray(it["camera_params"], float)
    n = int(keep.sum())
    q = BAProblem(poses=np.concatenate([it["rvec"], it["tvec"]])[None].copy(), pose_const=[0], image_camera=[0],
                  intrinsics=np.pad(cam[:-1], (0, 9 - (len(cam) - 1)))[None].copy(), camera_model=[int(cam[-1])], intr_const=[1],
                  points=it["points3D"][keep].copy(), point_const=np.ones(n, np.uint8), obs_uv=it["points2D"][keep].copy(),
                  obs_image=np.zeros(n, np.int32), obs_point=np.arange(n, dtype=np.int32))
    ro, _ = oracle.solve(q, oracle.options(), jac_mode=jac_mode)  # BundleAdjustmentOptions defaults, like the reference call
    return q.poses[0], ro


def test_pose_refinement_batch_around_256_inliers_matches_oracle(mavba, oracle):
    items = _pose_size_items()
    start = [np.concatenate([it["rvec"], it["tvec"]]) for it in items]
    ref = [_oracle_pose(oracle, it) for it in items]
    # six inliers are twelve residuals for six parameters: the oracle's two Jacobian modes must walk the same path there
    ro6, ra6 = ref[1][1], _oracle_pose(oracle, items[1], jac_mode=1)[1]
    assert (ro6["num_successful_steps"], ro6["num_unsuccessful_steps"], ro6["termination"]) == \
           (ra6["num_successful_steps"], ra6["num_unsuccessful_steps"], ra6["termination"])
    singles = [dict(it, rvec=it["rvec"].copy(), tvec=it["tvec"].copy()) for it in items]
    out = mavba.pose_refinement_batch(items)
    for n_in, it, x0, (cost, res), (pose_o, ro) in zip(POSE_INLIERS, items, start, out, ref):
        assert res["num_residuals"] == 2 * n_in == ro["num_residuals"]
        got = np.concatenate([it["rvec"], it["tvec"]])
        if n_in == 0:  # nothing to refine: the pose stays, the reference's return value is sqrt(0 / 0)
            assert np.isnan(cost) and res["final_cost"] == 0.0 and np.array_equal(got, x0) and np.array_equal(pose_o, x0)
            continue
        assert res["termination"] == ro["termination"], (n_in, res["termination_name"], ro["termination_name"])
        assert res["num_successful_steps"] == ro["num_successful_steps"] and res["num_unsuccessful_steps"] == ro["num_unsuccessful_steps"], n_in
        assert res["num_parameters_reduced"] == ro["num_parameters_reduced"]
        assert abs(res["initial_cost"] - ro["initial_cost"]) <= 1e-10 * ro["initial_cost"], n_in
        assert abs(res["final_cost"] - ro["final_cost"]) <= 1e-6 * ro["final_cost"], n_in
        assert rel_err(got, pose_o) < 1e-6, n_in
        assert abs(cost - np.sqrt(ro["final_cost"] / ro["num_residuals"])) < 1e-6 * cost, n_in
    # the batch equals single calls bit for bit
    for n_in, it, s, (cost, res) in zip(POSE_INLIERS, items, singles, out):
        c1, r1 = mavba.pose_refinement(s["rvec"], s["tvec"], s["camera_params"], s["points2D"], s["points3D"], s["inlier_mask"])
        assert (c1 == cost or (np.isnan(c1) and np.isnan(cost))) and r1["final_cost"] == res["final_cost"], n_in
        assert np.array_equal(s["rvec"], it["rvec"]) and np.array_equal(s["tvec"], it["tvec"]), n_in
        assert r1["num_successful_steps"] == res["num_successful_steps"] and r1["termination"] == res["termination"], n_in
