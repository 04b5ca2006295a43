"""The per-observation arithmetic of csrc/ba_math.h as the DEVICE builds it - hardware reciprocal and reciprocal-square-root
seeds with Newton steps, the short log series, FMA contraction - against the 60-digit reference of
tests/golden/obs_math_hp.npz (tests/hp_reference.py; generator tests/golden/make_obs_math_fixture.py), through the test entry
mavba_debug_obs_math, which calls the very functions the kernels inline. One launch per test. tests/test_hp_reference.py
holds the host build to the same bars, so a failure here alone is the device build's.

Measured on an MI355X (the printed maxima): see the comment block above rcp_obs in csrc/ba_math.h."""
import numpy as np
import pytest

from mavmap_amd import _abi as A
from tests import obs_math_fixture as F

pytestmark = pytest.mark.gpu

ULP_BAR = 2.0  # the claim of csrc/ba_math.h for rcp_obs, rsqrt_obs and log_obs


def _both(mavba, kind, cases):
    return mavba.api.debug_obs_math(kind, cases)


@pytest.mark.parametrize("name,kind", [("rcp", A.OBS_MATH_RCP), ("rsqrt", A.OBS_MATH_RSQRT), ("log", A.OBS_MATH_LOG)])
def test_scalar_function_is_within_its_claimed_ulps(mavba, name, kind):
    """rcp_obs over 1e-150 <= |x| <= 1e150, rsqrt_obs over [1e-150, 1e300], log_obs over [1, 1e300]: log-uniform values, the
    powers of two with their neighbours, the extreme mantissas, and for the log the low end 1 + 10^u of the Cauchy argument
    and both sides of the series' fold at sqrt(2)."""
    z = F.load()
    x, hi, lo = z[name + "_x"], z[name + "_hi"], z[name + "_lo"]
    host, dev = _both(mavba, kind, x)
    eh, ed = F.ulp_error(host[:, 0], hi, lo), F.ulp_error(dev[:, 0], hi, lo)
    i = int(np.argmax(np.where(np.isnan(ed), np.inf, ed)))
    print("%s_obs: max error device %.3f ulp (x = %r, device %r, host %r, exact %r), host %.3f ulp, %d cases"
          % (name, ed[i], x[i], dev[i, 0], host[i, 0], hi[i], np.nanmax(eh), len(x)))
    assert np.isfinite(dev).all()
    assert ed.max() <= ULP_BAR, (x[i], dev[i, 0], host[i, 0], hi[i], ed[i])
    if name == "log":
        assert x[0] == 1.0 and dev[0, 0] == 0.0 and np.signbit(dev[0, 0]) == np.signbit(0.0)


@pytest.mark.parametrize("name,kind", [("rcp", A.OBS_MATH_RCP), ("rsqrt", A.OBS_MATH_RSQRT), ("log", A.OBS_MATH_LOG)])
def test_special_values_are_never_a_finite_wrong_value(mavba, name, kind):
    """Zeros, denormals, 1e300, 1e-300, infinities, NaN, and negative arguments of the root and the log: no ulp bar, but the
    device result is either within the bar of the exact value or not finite. The printed table (host class / device class) is
    the one in csrc/ba_math.h."""
    z = F.load()
    x, hi, lo = z[name + "_special_x"], z[name + "_special_hi"], z[name + "_special_lo"]
    host, dev = _both(mavba, kind, x)
    ch, cd = F.classify(host[:, 0]), F.classify(dev[:, 0])
    print("%s_obs   x: host -> device" % name)
    for i in range(len(x)):
        print("  %-8r %-7s %-7s%s" % (float(x[i]), ch[i], cd[i], "  (%r)" % float(dev[i, 0]) if cd[i] == "finite" else ""))
    bad = F.special_violations(x, dev[:, 0], hi, lo, ULP_BAR)
    assert not bad, bad


def test_rot_coeffs_on_both_branches_and_through_the_zeros_of_sin(mavba):
    """a, b, c of Rodrigues' formula and its left Jacobian: th2 = 0, far inside the series, either side of 1e-6 (the switch
    this test found wanting) and of 0.25 (the switch now), pi, beyond pi, 2 pi, 7, 100, and 2 000 random values."""
    z = F.load()
    th2 = z["rot_x"]
    host, dev = _both(mavba, A.OBS_MATH_ROT_COEFFS, th2)
    bar_a, bar_b = F.rot_bars(th2, z["rot_a_hi"], z["rot_b_hi"])
    assert np.array_equal(dev[0], [1.0, 0.5, 1.0 / 6.0]) and th2[0] == 0.0
    for k, (nm, bar) in enumerate((("a", bar_a), ("b", bar_b), ("c", 1e-14 * np.abs(z["rot_c_hi"])))):
        ref = z["rot_%s_hi" % nm]
        err = np.abs(dev[:, k] - ref)
        i = int(np.argmax(err / bar))
        print("rot_coeffs %s: worst error / bar %.3f at th2 = %r (device %r, host %r, exact %r)"
              % (nm, err[i] / bar[i], th2[i], dev[i, k], host[i, k], ref[i]))
        assert (err <= bar).all(), (nm, th2[i], dev[i, k], host[i, k], ref[i])


def test_cauchy_weight_from_zero_to_1e14(mavba):
    """w = sqrt(rho') within 4 ulp, rho / 2 within 1e-15 relative (or 1e-300 absolute), for s = |r|^2 from 0 and 1e-20 to
    1e14 - the outlier family's 1e3, 1e5, 1e7 px included - and b = a^2 in {0.01, 1, 9, 1e4}."""
    z = F.load()
    sb = z["cauchy_x"]
    host, dev = _both(mavba, A.OBS_MATH_CAUCHY, sb)
    ew = F.ulp_error(dev[:, 0], z["cauchy_w_hi"], z["cauchy_w_lo"])
    h = z["cauchy_h_hi"]
    eh = np.abs(dev[:, 1] - h)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(h > 0, eh / h, 0.0)
    i, j = int(np.argmax(ew)), int(np.argmax(np.where(eh <= 1e-300, 0.0, rel)))
    print("cauchy_weight: w max %.3f ulp at (s, b) = %r; half_rho max %.2e relative at %r (device %r, host %r, exact %r)"
          % (ew[i], tuple(sb[i]), rel[j], tuple(sb[j]), dev[j, 1], host[j, 1], h[j]))
    assert ew.max() <= 4.0, (tuple(sb[i]), dev[i, 0], host[i, 0], z["cauchy_w_hi"][i])
    ok = (eh <= 1e-15 * np.abs(h)) | (eh <= 1e-300)
    assert ok.all(), (sb[~ok][:5], dev[~ok, 1][:5], host[~ok, 1][:5], h[~ok][:5])


def _composed(mavba):
    z = F.load()
    rows = z["obs_in"]
    hj, dj = _both(mavba, A.OBS_MATH_JACOBIAN, rows[:, :21])
    hb, db = _both(mavba, A.OBS_MATH_BACKSUB, rows)
    hr, dr = _both(mavba, A.OBS_MATH_RESIDUAL, rows[:, :21])
    return z, (hj, hb, hr), (dj, db, dr)


def test_composed_cases_through_the_three_observation_functions(mavba):
    """cam_prepare + obs_jacobian, obs_residual and obs_backsub_term on the eight families of the fixture (benign, tiny and
    large rotations, depth, outliers, far frame, catadioptric, distortion): every block (r, Jc, Jp, Jk, t) in the max norm
    relative to its own maximum, within 1e-11 times the case's amplification factor; where the projection's denominator is
    exactly zero nothing finite comes out."""
    z, (hj, hb, hr), (dj, db, dr) = _composed(mavba)
    ref, cin, fam = z["obs_ref"], z["obs_cin"], z["obs_family"]
    got, goth = np.concatenate([dj, db[:, 2:]], 1), np.concatenate([hj, hb[:, 2:]], 1)
    bad, worst = F.composed_failures(got, ref, cin, fam, ("r", "Jc", "Jp", "Jk", "t"))
    _, worst_h = F.composed_failures(goth, ref, cin, fam, ("r", "Jc", "Jp", "Jk", "t"))
    for f in sorted(worst):
        print("family %d %-15s device %s | host %s" % (f, F.FAMILIES[f], {b: "%.1e" % e for b, e in worst[f].items()},
                                                         {b: "%.1e" % e for b, e in worst_h[f].items()}))
    assert not bad, [(b, z["obs_in"][b[0], :21].tolist(), got[b[0], F.BLOCKS[b[2]]].tolist(), goth[b[0], F.BLOCKS[b[2]]].tolist()) for b in bad[:3]]
    # the residual of obs_residual and of obs_backsub_term: the same bar (the compiler may contract them differently)
    for name, r in (("obs_residual", dr), ("obs_backsub_term", db[:, :2])):
        g = got.copy()
        g[:, :2] = r
        bad, _ = F.composed_failures(g, ref, cin, fam, ("r",))
        assert not bad, (name, bad[:5])
