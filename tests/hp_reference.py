"""A plain high-precision reference of the per-observation maths, in mpmath at 60 digits. TEST INFRASTRUCTURE.

Written from the model definitions, not from csrc/ba_math.h: the rotation is Rodrigues' formula in its exact form (no
series branch: 60 digits do not need one), the derivatives are central differences at 80 digits with a step of 1e-30, whose
truncation error (step^2 ~ 1e-60) and rounding error (1e-80 / 1e-30) are both far below 1e-40 - no hand-derived derivative
that could share a mistake with the kernels'.

  pose  = (rvec[3], t[3]),  Xc = R(rvec) X + t
  cam   = (fx, fy, cx, cy, k1, k2, p1, p2, xi); PINHOLE reads 4 of them, OPENCV 8, CATA all 9
  r     = project(model, cam, Xc) - uv
  loss  = Cauchy with scale a: rho(s) = a^2 log(1 + s / a^2), s = |r|^2; the corrected residual and every Jacobian row are
          the raw ones times sqrt(rho') (the rho'' <= 0 branch of the Ceres corrector: what tests/test_oracle.py pins for the
          oracle and include/mavba.h documents for mavba_session_eval_jacobian); the block's cost is rho / 2.

Only tests/golden/make_obs_math_fixture.py and tests/test_hp_reference.py import this; GPU tests read the fixture."""
import mpmath as mp
from mpmath import mpf

DPS = 60
DIFF_DPS = 80
DIFF_STEP = mpf(10) ** -30
PINHOLE, OPENCV, CATA = 1, 2, 3
NUM_PARAMS = {PINHOLE: 4, OPENCV: 8, CATA: 9}

mp.mp.dps = DPS


def vec(a):
    """Doubles (or mpf) -> list of mpf, exactly."""
    return [x if isinstance(x, mpf) else mpf(float(x)) for x in a]


def cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def norm(a):
    return mp.sqrt(dot(a, a))


def rotate(rvec, X):
    """R(rvec) X by Rodrigues' formula: X cos th + (k x X) sin th + k (k . X)(1 - cos th), k = rvec / th; 1 - cos th is
    formed as 2 sin^2(th / 2), which has no cancellation."""
    th2 = dot(rvec, rvec)
    if th2 == 0:
        return list(X)
    th = mp.sqrt(th2)
    k = [w / th for w in rvec]
    s, c = mp.sin(th), mp.cos(th)
    omc = 2 * mp.sin(th / 2) ** 2
    kx, kd = cross(k, X), dot(k, X)
    return [X[i] * c + kx[i] * s + k[i] * kd * omc for i in range(3)]


def rotation_matrix(rvec):
    """3 x 3 list of rows."""
    w = vec(rvec)
    cols = [rotate(w, [mpf(i == j) for i in range(3)]) for j in range(3)]
    return [[cols[j][i] for j in range(3)] for i in range(3)]


def rot_coeffs(th2):
    """a = sin th / th, b = (1 - cos th) / th^2, c = (th - sin th) / th^3 with their limits at 0. The working precision is
    raised by the digits that th - sin th cancels."""
    th2 = mpf(th2)
    if th2 == 0:
        return mpf(1), mpf(1) / 2, mpf(1) / 6
    with mp.workdps(DPS + 40 + max(0, int(-1.5 * mp.log10(th2)))):
        th = mp.sqrt(th2)
        out = mp.sin(th) / th, 2 * mp.sin(th / 2) ** 2 / th2, (th - mp.sin(th)) / (th2 * th)
    return tuple(+x for x in out)


def transform(pose, X):
    Xr = rotate(pose[:3], X)
    return Xr, [Xr[i] + pose[3 + i] for i in range(3)]


def project(model, cam, Xc):
    """(u, v). mpmath raises ZeroDivisionError where the denominator is exactly zero."""
    fx, fy, cx, cy = cam[:4]
    zz = Xc[2]
    if model == CATA:
        zz = Xc[2] + cam[8] * norm(Xc)
    un, vn = Xc[0] / zz, Xc[1] / zz
    if model != PINHOLE:
        k1, k2, p1, p2 = cam[4:8]
        r2 = un * un + vn * vn
        radial = 1 + k1 * r2 + k2 * r2 * r2
        un, vn = (un * radial + 2 * p1 * un * vn + p2 * (r2 + 2 * un * un),
                  vn * radial + p1 * (r2 + 2 * vn * vn) + 2 * p2 * un * vn)
    return [fx * un + cx, fy * vn + cy]


def _residual(model, params):
    """params = pose[6] + X[3] + cam[9] + uv[2], all mpf."""
    _, Xc = transform(params[:6], params[6:9])
    u, v = project(model, params[9:18], Xc)
    return [u - params[18], v - params[19]]


def residual(model, pose, cam, X, uv):
    return _residual(model, vec(pose) + vec(X) + vec(cam) + vec(uv))


def cauchy(s, a):
    """(sqrt(rho'), rho / 2) of the Cauchy loss with scale a at s = |r|^2."""
    s, b = mpf(s), mpf(a) * mpf(a)
    x = 1 + s / b
    return 1 / mp.sqrt(x), b * mp.log(x) / 2


def cauchy_b(s, b):
    """The same with b = a^2 given (what cauchy_weight takes)."""
    s, b = mpf(s), mpf(b)
    x = 1 + s / b
    return 1 / mp.sqrt(x), b * mp.log(x) / 2


def jacobian(model, pose, cam, X, uv):
    """Raw residual r[2] and Jc[2][6] = d r / d (rvec, t), Jp[2][3] = d r / d X, Jk[2][9] = d r / d cam (columns the model
    does not read are zero) by central differences. None instead of every block where the projection's denominator is zero."""
    p0 = vec(pose) + vec(X) + vec(cam) + vec(uv)
    try:
        r = _residual(model, p0)
    except ZeroDivisionError:
        return None
    K = NUM_PARAMS[model]
    cols = {}
    with mp.workdps(DIFF_DPS):
        for j in list(range(9)) + list(range(9, 9 + K)):
            h = DIFF_STEP * max(1, abs(p0[j]))
            hi, lo = list(p0), list(p0)
            hi[j], lo[j] = p0[j] + h, p0[j] - h
            rp, rm = _residual(model, hi), _residual(model, lo)
            cols[j] = [(rp[0] - rm[0]) / (2 * h), (rp[1] - rm[1]) / (2 * h)]
    zero = [mpf(0), mpf(0)]
    J = [[+cols.get(j, zero)[i] for j in range(18)] for i in range(2)]
    return r, [row[:6] for row in J], [row[6:9] for row in J], [row[9:18] for row in J]


def corrected(r, blocks, a):
    """Loss-corrected residual and Jacobian blocks, and the block's cost rho / 2."""
    w, half_rho = cauchy(r[0] * r[0] + r[1] * r[1], a)
    return [w * x for x in r], [[[w * x for x in row] for row in B] for B in blocks], half_rho


def backsub_term(Jc, Jp, Jk, dc, dk):
    """t = Jp^T (Jc dc + Jk dk), unweighted."""
    dc, dk = vec(dc), vec(dk)
    tau = [sum(Jc[i][j] * dc[j] for j in range(6)) + sum(Jk[i][j] * dk[j] for j in range(9)) for i in range(2)]
    return [Jp[0][j] * tau[0] + Jp[1][j] * tau[1] for j in range(3)]


def amplification(model, pose, cam, X):
    """c_in: by how much the two data-dependent subtractions of the formula amplify the rounding of their operands:
    Xc = R X + t, max(1, (|R X| + |t|) / |Xc|), times, for the catadioptric model, the same for z + xi |Xc|."""
    pose, cam, X = vec(pose), vec(cam), vec(X)
    Xr, Xc = transform(pose, X)
    c = max(mpf(1), (norm(Xr) + norm(pose[3:])) / norm(Xc))
    if model == CATA:
        n = norm(Xc)
        den = abs(Xc[2] + cam[8] * n)
        c *= max(mpf(1), (abs(Xc[2]) + abs(cam[8]) * n) / den) if den != 0 else mpf(1)
    return c


def dd(x):
    """mpf -> (hi, lo): the nearest double and the nearest double of the remainder."""
    hi = float(x)
    if hi != hi or hi in (float("inf"), float("-inf")):
        return hi, 0.0
    return hi, float(x - mpf(hi))
