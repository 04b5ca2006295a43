"""The 60-digit reference of the per-observation maths (tests/hp_reference.py) and its committed fixture
(tests/golden/obs_math_hp.npz): the reference against the reference project's own known answers, the fixture against its
generator, and the two CPU parties - the host build of csrc/ba_math.h and the oracle - against the fixture, at the bars
tests/test_gpu_obs_math.py holds the device build to. A failure here and there says the formula is wrong; a failure there
alone says the device build is."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from mavmap_amd import _abi as A
from tests import obs_math_fixture as F

HERE = os.path.dirname(os.path.abspath(__file__))
dp = C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def host():
    src = os.path.join(HERE, "host", "ba_math_host.cpp")
    so = os.path.join(HERE, "host", "_ba_math_host.so")
    hdr = os.path.join(HERE, "..", "mavmap_amd", "csrc", "ba_math.h")
    if not os.path.exists(so) or max(os.path.getmtime(src), os.path.getmtime(hdr)) > os.path.getmtime(so):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
    L = C.CDLL(so)
    if not hasattr(L, "hm_obs_math"):  # a library from before the export
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
        L = C.CDLL(so)
    L.hm_obs_math.argtypes = [C.c_int, C.c_int, dp, dp]
    L.hm_obs_math.restype = None
    return L


def host_obs_math(host, kind, cases):
    wi, wo = A.OBS_MATH_WIDTHS[kind]
    cases = np.ascontiguousarray(cases, dtype=np.float64).reshape(-1, wi)
    out = np.zeros((len(cases), wo))
    host.hm_obs_math(kind, len(cases), cases.ctypes.data_as(dp), out.ctypes.data_as(dp))
    return out


def test_reference_reproduces_the_reference_projects_known_answers():
    """world2image_kat.json / world2image_jet_kat.json: values and derivatives of the reference's own templates, at the bars
    tests/test_host_math.py uses for them (1e-12 values, 1e-11 derivatives)."""
    from tests import hp_reference as H
    kat = json.load(open(os.path.join(HERE, "golden", "world2image_kat.json")))
    for c in kat["vectors"]:
        cam = np.zeros(9); cam[:len(c["params"])] = c["params"]
        uv = [float(x) for x in H.residual(c["code"], np.zeros(6), cam, c["Xc"], np.zeros(2))]
        assert np.abs(np.array(uv) - c["uv"]).max() <= 1e-12 * np.abs(c["uv"]).max(), c
    jet = json.load(open(os.path.join(HERE, "golden", "world2image_jet_kat.json")))
    for c in jet["vectors"]:
        K = A.MODEL_NUM_PARAMS[c["code"]]
        cam = np.zeros(9); cam[:K] = c["params"]
        r, Jc, Jp, Jk = H.jacobian(c["code"], np.zeros(6), cam, c["Xc"], np.zeros(2))
        r, Jp, Jk = np.array(r, float), np.array(Jp, float), np.array(Jk, float)
        assert np.abs(r - c["uv"]).max() <= 1e-12 * np.abs(c["uv"]).max()
        ref_p, ref_k = np.array([c["du"][:3], c["dv"][:3]]), np.array([c["du"][3:], c["dv"][3:]])
        assert np.abs(Jp - ref_p).max() <= 1e-11 * np.abs(ref_p).max(), c["model"]
        assert np.abs(Jk[:, :K] - ref_k).max() <= 1e-11 * np.abs(ref_k).max(), c["model"]
        assert not Jk[:, K:].any()
        # with no rotation d r / d t = d r / d Xc
        assert np.abs(np.array(Jc, float)[:, 3:] - ref_p).max() <= 1e-11 * np.abs(ref_p).max()


def test_regenerating_the_fixture_gives_the_committed_arrays():
    pytest.importorskip("mpmath")
    from tests.golden import make_obs_math_fixture as G
    fresh, kept = G.build_all(), F.load()
    assert sorted(fresh) == sorted(kept)
    for k in kept:
        assert fresh[k].dtype == kept[k].dtype and fresh[k].shape == kept[k].shape, k
        assert fresh[k].tobytes() == kept[k].tobytes(), k
    assert os.path.getsize(F.PATH) < 1000000


def test_fixture_holds_what_the_amplification_factor_may_excuse():
    """c_in <= 4 outside the far-frame and catadioptric families; inside them at most a third of the cases above 100; every
    family is there, with every model it is meant for."""
    z = F.load()
    fam, cin, model = z["obs_family"], z["obs_cin"], z["obs_in"][:, 0].astype(int)
    wide = np.isin(fam, (6, 7))
    assert cin[~wide].max() <= 4.0 and cin.min() >= 1.0
    assert (cin[wide] > 100.0).sum() * 3 <= wide.sum()
    for f in F.FAMILIES:
        want = {7: {3}, 8: {2, 3}}.get(f, {1, 2, 3})
        for m in want:
            assert ((fam == f) & (model == m)).sum() >= 20, (f, m)
    assert (~np.isfinite(z["obs_ref"]).all(1)).sum() == 3  # the three zero-denominator cases


def test_host_build_meets_the_bars_on_the_composed_cases(host):
    z = F.load()
    rows, ref, cin, fam = z["obs_in"], z["obs_ref"], z["obs_cin"], z["obs_family"]
    got = np.full_like(ref, np.nan)
    got[:, :38] = host_obs_math(host, A.OBS_MATH_JACOBIAN, rows[:, :21])
    bs = host_obs_math(host, A.OBS_MATH_BACKSUB, rows)
    got[:, 38:] = bs[:, 2:]
    bad, worst = F.composed_failures(got, ref, cin, fam, ("r", "Jc", "Jp", "Jk", "t"))
    print({F.FAMILIES[f]: {b: "%.1e" % e for b, e in w.items()} for f, w in sorted(worst.items())})
    assert not bad, bad[:10]
    # the residual of the other two entries is the same arithmetic: identical, not merely close
    res = host_obs_math(host, A.OBS_MATH_RESIDUAL, rows[:, :21])
    fin = np.isfinite(ref).all(1)
    assert np.array_equal(res[fin], got[fin, :2]) and np.array_equal(bs[fin, :2], got[fin, :2])


def test_host_build_of_rot_coeffs_and_cauchy_weight_meets_the_bars(host):
    z = F.load()
    th2 = z["rot_x"]
    got = host_obs_math(host, A.OBS_MATH_ROT_COEFFS, th2)
    bar_a, bar_b = F.rot_bars(th2, z["rot_a_hi"], z["rot_b_hi"])
    for k, (nm, bar) in enumerate((("a", bar_a), ("b", bar_b), ("c", 1e-14 * np.abs(z["rot_c_hi"])))):
        err = np.abs(got[:, k] - z["rot_%s_hi" % nm])
        i = int(np.argmax(err / bar))
        assert (err <= bar).all(), (nm, th2[i], got[i, k], z["rot_%s_hi" % nm][i])
    sb = z["cauchy_x"]
    got = host_obs_math(host, A.OBS_MATH_CAUCHY, sb)
    ew = F.ulp_error(got[:, 0], z["cauchy_w_hi"], z["cauchy_w_lo"])
    assert ew.max() <= 4.0, (ew.max(), sb[int(np.argmax(ew))])
    h = z["cauchy_h_hi"]
    eh = np.abs(got[:, 1] - h)
    ok = (eh <= 1e-15 * np.abs(h)) | (eh <= 1e-300)
    assert ok.all(), (sb[~ok][:5], got[~ok, 1][:5], h[~ok][:5])


def test_oracle_agrees_with_the_reference_except_at_tiny_rotations(oracle):
    """The oracle's obs_jacobian on the composed cases: within the bar in every family but the tiny rotations, where the
    formula it differentiates (like the reference project's) loses digits in d / d rvec for 0 < |rvec| << 1. The fixture's
    oracle_ok records the pattern; it is what lets a GPU test use the oracle as the referee for a family."""
    z = F.load()
    rows, ref, cin, fam = z["obs_in"], z["obs_ref"], z["obs_cin"], z["obs_family"]
    got = np.full((len(rows), 41), np.nan)
    for i, q in enumerate(rows):
        r, Jc, Jp, Jk = oracle.obs_jacobian(0, int(q[0]), q[1:7], q[16:19], q[7:16], q[19:21])
        got[i, :38] = np.concatenate([r, Jc.ravel(), Jp.ravel(), Jk.ravel()])
    bad, worst = F.composed_failures(got, ref, cin, fam, ("r", "Jc", "Jp", "Jk"))
    print({F.FAMILIES[f]: {b: "%.1e" % e for b, e in w.items()} for f, w in sorted(worst.items())})
    failing = sorted({f for _, f, *_ in bad})
    assert sorted(set(F.FAMILIES) - set(failing)) == sorted(z["oracle_ok"].tolist()), bad[:10]
    # and inside the failing family it is d / d rvec of the non-zero tiny rotations, nothing else
    for i, f, b, *_ in bad:
        th = np.linalg.norm(rows[i, 1:4])
        assert f == 2 and b == "Jc" and 0.0 < th < 1e-3, (i, f, b, th)


@pytest.mark.parametrize("family", F.STRESS_FAMILIES)
def test_stress_problems_are_well_conditioned_and_the_oracle_evaluates_them(oracle, family):
    """tests/test_gpu_stress_geometry.py compares steps with the oracle's at 1e-8, which presumes a well-conditioned reduced
    system: cond(S) <= 1e6 at the radii it uses. And the oracle's own evaluation of the problem meets the bars in exactly
    the families of oracle_ok (elsewhere only d / d rvec may miss)."""
    p = F.stress_problem(family)
    for radius in (3.0, 1e4):
        S = oracle.linear_step(p, radius)["S"]
        assert np.linalg.cond(S) <= 1e6, (radius, np.linalg.cond(S))
    cost, r, Jc, Jp, Jk = oracle.eval_jacobian(p)
    bad, worst = F.stress_failures(family, r, Jc, Jp, Jk)
    ref_cost = float(F.load()["stress%d_cost" % family])
    assert abs(cost - ref_cost) <= 1e-11 * ref_cost
    if family in F.load()["oracle_ok"].tolist():
        assert not bad, bad[:5]
    else:
        assert bad and {b for _, b, *_ in bad} == {"Jc"}, bad[:5]


def test_the_test_entry_is_declared_exported_and_listed(mavba):
    """include/mavba_obs_math.h (a header of its own, like the other test entries outside mavba.h): what it declares is what
    api.OBS_MATH_SYMBOLS lists and the library exports."""
    import re
    from mavmap_amd import api
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(HERE, "..", "include", "mavba_obs_math.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(mavba_[a-z0-9_]+)\s*\(", header)))
    assert declared == sorted(api.OBS_MATH_SYMBOLS) and all(hasattr(mavba.load(), n) for n in declared)
    assert not set(declared) & set(api.EXPORTED_SYMBOLS)
