"""The production kernels on the geometry no synth.make_scene problem has: free images on the series branch of the rotation
and at or beyond pi, points behind and next to the camera plane, outliers of 1e7 px, a world frame far from the cameras, wide
catadioptric fields of view, strong distortion. tests/test_gpu_obs_math.py proves the functions of csrc/ba_math.h; this proves
each kernel's inlined copy of them, with its own register and LDS plumbing.

One tiny hand-built problem per family 2-8 (tests/golden/make_obs_math_fixture.py, stress_problem: 5 images, 3 cameras with
free intrinsics, 48 points in 3 to 5 images each), stored in tests/golden/obs_math_hp.npz with its 60-digit evaluation. The
oracle referees only where tests/test_hp_reference.py found it fit to (the fixture's oracle_ok: not the tiny rotations)."""
import numpy as np
import pytest

from tests import obs_math_fixture as F
from tests.conftest import rel_err

pytestmark = pytest.mark.gpu

RADII = (3.0, 1e4)  # tests/test_hp_reference.py: the oracle's S has a condition number below 1e6 at both, in every family


@pytest.mark.parametrize("family", F.STRESS_FAMILIES)
def test_eval_jacobian_against_the_60_digit_evaluation(mavba, family):
    """Session.eval_jacobian(): the loss-corrected r, Jc, Jp, Jk of every observation within 1e-11 times its amplification
    factor (each block in the max norm relative to its own maximum), the cost within 1e-11."""
    p = F.stress_problem(family)
    with mavba.Session(p) as s:
        cost, r, Jc, Jp, Jk = s.eval_jacobian()
    bad, worst = F.stress_failures(family, r, Jc, Jp, Jk)
    ref_cost = float(F.load()["stress%d_cost" % family])
    print("family %d %-15s worst error / c_in %s, cost %.3e relative" % (family, F.FAMILIES[family], {b: "%.1e" % e for b, e in worst.items()},
                                                                        abs(cost - ref_cost) / ref_cost))
    assert not bad, bad[:5]
    assert abs(cost - ref_cost) <= 1e-11 * ref_cost


@pytest.mark.parametrize("family", F.STRESS_FAMILIES)
def test_the_three_front_ends_on_stress_geometry(mavba, oracle, monkeypatch, family):
    """The default route, MAVBA_NO_FUSE and MAVBA_FRONT_PLANES (set as test_the_three_front_ends_give_the_same_system_and_solve
    sets them): S exactly symmetric, the routes within 1e-12 of each other on S in every family - the tiny rotations too, where
    no oracle can referee -, and, in the families of oracle_ok, S and v within 1e-9, the step within 1e-8 and
    model_cost_change within 1e-9 of the oracle's, at both radii."""
    p = F.stress_problem(family)
    use_oracle = family in F.load()["oracle_ok"].tolist()
    refs = {rad: oracle.linear_step(p, rad) for rad in RADII} if use_oracle else {}
    systems, timers = [], []
    for env in (None, "MAVBA_NO_FUSE", "MAVBA_FRONT_PLANES"):
        if env:
            monkeypatch.setenv(env, "1")
        with mavba.Session(p, dict(profile_kernels=1)) as s:
            for rad in RADII:
                S, v = s.reduced_system(rad)
                st = s.linear_step(rad)
                assert np.array_equal(S, S.T), (env, rad)
                systems.append((env, rad, S, v))
                if use_oracle:
                    ref = refs[rad]
                    assert rel_err(S, ref["S"]) < 1e-9 and rel_err(v, ref["v"]) < 1e-9, (env, rad, rel_err(S, ref["S"]), rel_err(v, ref["v"]))
                    for k in ("d_poses", "d_intr", "d_points"):
                        assert rel_err(st[k], ref[k]) < 1e-8, (env, rad, k, rel_err(st[k], ref[k]))
                    assert abs(st["model_cost_change"] - ref["model_cost_change"]) < 1e-9 * abs(ref["model_cost_change"]), (env, rad)
            timers.append(set(s.kernel_stats()))
    print("family %d kernels: default %s | no_fuse adds %s | planes adds %s" % (family, sorted(timers[0]), sorted(timers[1] - timers[0]),
                                                                                 sorted(timers[2] - timers[0])))
    assert timers[1] != timers[0] and timers[2] != timers[0] and timers[2] != timers[1]  # the routes really differ
    for env, rad, S, v in systems[2:]:
        S0, v0 = next((a, b) for e, r_, a, b in systems if e is None and r_ == rad)
        assert rel_err(S, S0) < 1e-12, (env, rad, rel_err(S, S0))


@pytest.mark.parametrize("family", F.STRESS_FAMILIES)
def test_initial_cost_and_first_step_of_a_solve(mavba, oracle, family):
    """One LM iteration: the initial cost (the evaluation kernels, not the Jacobian probe) within 1e-11 of the 60-digit cost,
    no error, and the first step accepted, rejected or invalid as the oracle's is."""
    p, po = F.stress_problem(family), F.stress_problem(family)
    ro, _ = oracle.solve(po, oracle.options(max_num_iterations=1))
    _, rg = mavba.bundle_adjustment(p, dict(max_num_iterations=1))
    ref_cost = float(F.load()["stress%d_cost" % family])
    print("family %d initial cost %.3e relative, steps %d / %d" % (family, abs(rg["initial_cost"] - ref_cost) / ref_cost,
                                                                   rg["num_successful_steps"], rg["num_unsuccessful_steps"]))
    assert abs(rg["initial_cost"] - ref_cost) <= 1e-11 * ref_cost
    assert rg["termination"] == ro["termination"]
    assert (rg["num_successful_steps"], rg["num_unsuccessful_steps"]) == (ro["num_successful_steps"], ro["num_unsuccessful_steps"])


def _rotation(w):
    th = np.linalg.norm(w)
    if th == 0.0:
        return np.eye(3)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def pose_refine_items():
    z = F.load()
    return [dict(rvec=z["pose_start"][q, :3].copy(), tvec=z["pose_start"][q, 3:].copy(), camera_params=z["pose_cam"][q].copy(),
                 points2D=z["pose_uv"][q].copy(), points3D=z["pose_xyz"][q].copy(), inlier_mask=np.ones(40, np.uint8)) for q in range(4)]


def test_pose_refinement_from_zero_tiny_and_beyond_pi(mavba, oracle):
    """pose_refine_batch (the loop of pose_refine.hip) from rvec = 0 exactly, |rvec| = 1e-9, pi - 1e-8 and pi + 0.5, 40 clean
    correspondences each: the oracle's optimum within the existing 1e-6, and the rotation MATRIX of the 60-digit ground truth
    within 1e-6 (an rvec beyond pi is another vector for the same rotation)."""
    from tests.test_gpu_parity import _oracle_pose
    items = pose_refine_items()
    ref = [_oracle_pose(oracle, it) for it in items]
    out = mavba.pose_refinement_batch(items)
    Rtrue = F.load()["pose_Rtrue"]
    for q, (it, (cost, res), (pose_o, ro)) in enumerate(zip(items, out, ref)):
        dR = np.abs(_rotation(it["rvec"]) - Rtrue[q]).max()
        print("item %d: |rvec| start %.3g, end %.6g, %s, rotation matrix off by %.1e" % (q, np.linalg.norm(F.load()["pose_start"][q, :3]),
                                                                                       np.linalg.norm(it["rvec"]), res["termination_name"], dR))
        assert rel_err(np.concatenate([it["rvec"], it["tvec"]]), pose_o) < 1e-6, q
        assert dR < 1e-6, (q, dR)
