"""Restatements of the two sky backgrounds, shared by tests/test_sky_host.py and tests/test_gpu_sky.py.

GradientBackground::eval (background_gradient.cc:40-59) is float32 arithmetic alone.  SunSkyBackground (background_sunsky.cc) mixes double
arithmetic with the reference's float helpers: its constructor (:37-76) runs in double on the host, getSkyCol (:116-169) on the device.
Which overload each unqualified call takes there was read off the reference's headers: acos, atan2, cos and tan are the double ones
(the float arguments widen), fExp__ / fSin__ / fCos__ / fAcos__ take and return float (their double arguments narrow at the call)."""
import math

import numpy as np

from tests.test_gpu_ibl import M_1_PI, M_PI, MAXU, NV, ROW, inv_spheremap, np_fcos, np_fsin, pdf1d, row_counts

F = np.float32
f64 = np.float64
KIND_GRADIENT, KIND_SUNSKY = 4, 5

# the (from, turbidity) cases whose tables have energy in every row, and the one that has not (a sun well below the horizon)
SUNSKY_CASES = [((1.0, 1.0, 1.0), 4.0), ((1.0, 0.2, 0.15), 2.5), ((0.3, -1.0, 0.02), 6.0), ((1.0, 1.0, -0.1), 3.0)]
SUNSKY_EMPTY = ((1.0, 1.0, -0.5), 3.0)


def normalize32(v):
    """Vec3::normalize (vector.h:227-238) on rows of float32 vectors: a zero vector stays zero"""
    v = np.array(v, np.float32).reshape(-1, 3)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    ln = x * x + y * y + z * z
    with np.errstate(all="ignore"):
        inv = np.where(ln != 0, F(1) / np.sqrt(ln), F(1)).astype(np.float32)
    return np.stack([x * inv, y * inv, z * inv], axis=1).astype(np.float32)


# ---- gradientback ---------------------------------------------------------------------------------------------------
def gradient_eval(sky, dirs):
    """GradientBackground::eval: blends on dir.z as given; sky: the record's four float32 colours"""
    d = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
    z = d[:, 2]
    up = z >= 0
    blend = np.where(up, z, -z).astype(np.float32)[:, None]
    zen = np.where(up[:, None], sky["zenith"][None, :], sky["zenith_ground"][None, :]).astype(np.float32)
    hor = np.where(up[:, None], sky["horizon"][None, :], sky["horizon_ground"][None, :]).astype(np.float32)
    col = (blend * zen + (F(1) - blend) * hor).astype(np.float32)
    low = np.minimum(col[:, 0], np.minimum(col[:, 1], col[:, 2])) < F(1e-6)
    return np.where(low[:, None], F(1e-5), col).astype(np.float32)


# ---- sunsky: the constructor, in double -----------------------------------------------------------------------------
PEREZ_Y = ((0.17872, -1.46303), (-0.35540, 0.42749), (-0.02266, 5.32505), (0.12064, -2.57705), (-0.06696, 0.37027))
PEREZ_x = ((-0.01925, -0.25922), (-0.06651, 0.00081), (-0.00041, 0.21247), (-0.06409, -0.89887), (-0.00325, 0.04517))
PEREZ_y = ((-0.01669, -0.26078), (-0.09495, 0.00921), (-0.00792, 0.21023), (-0.04405, -1.65369), (-0.01092, 0.05291))


def sunsky_constants(frm, turbidity=4.0, var=(1.0, 1.0, 1.0, 1.0, 1.0), power=1.0):
    """SunSkyBackground's constructor with Python floats (IEEE doubles) and the C library's acos / atan2 / tan (the math module calls
    them).  Also returns `scale`: per value, the sum of the magnitudes of the terms it is added up from, for the test's bound."""
    d = normalize32(frm)[0]
    z = float(d[2])
    theta_f = F(M_PI) if z <= -1.0 else F(0) if z >= 1.0 else F(math.acos(z))      # fAcos__
    ts = float(theta_f); t2 = ts * ts; t3 = t2 * ts
    turb = F(turbidity)
    t, tt = float(turb), float(turb * turb)          # t_2_ = turb * turb is a float product
    chi = (4.0 / 9.0 - t / 120.0) * (M_PI - 2.0 * ts)
    tan_chi = math.tan(chi)
    zY = (4.0453 * t - 4.9710) * tan_chi - 0.2155 * t + 2.4192
    zY *= 1000
    zx = ((0.00165 * t3 - 0.00375 * t2 + 0.00209 * ts) * tt + (-0.02903 * t3 + 0.06377 * t2 - 0.03202 * ts + 0.00394) * t
          + (0.11693 * t3 - 0.21196 * t2 + 0.06052 * ts + 0.25886))
    zy = ((0.00275 * t3 - 0.00610 * t2 + 0.00317 * ts) * tt + (-0.04214 * t3 + 0.08970 * t2 - 0.04153 * ts + 0.00516) * t
          + (0.15346 * t3 - 0.26756 * t2 + 0.06670 * ts + 0.26688))
    v = [float(F(a)) for a in var]
    k = {"theta_s": ts, "phi_s": math.atan2(float(d[1]), float(d[0])), "zenith_x": zx, "zenith_y": zy, "zenith_Y": zY,
         "perez_Y": np.array([(a * t + b) * v[j] for j, (a, b) in enumerate(PEREZ_Y)]),
         "perez_x": np.array([(a * t + b) * v[j] for j, (a, b) in enumerate(PEREZ_x)]),
         "perez_y": np.array([(a * t + b) * v[j] for j, (a, b) in enumerate(PEREZ_y)]),
         "power": F(power), "turbidity": turb, "from": np.array(frm, np.float32)}
    zsum = lambda c: (abs(c[0]) * t3 + abs(c[1]) * t2 + abs(c[2]) * ts + (abs(c[3]) if len(c) > 3 else 0.0))
    scale = {"theta_s": 0.0, "phi_s": abs(k["phi_s"]),
             "zenith_Y": 1000 * (abs((4.0453 * t - 4.9710) * tan_chi) + 0.2155 * t + 2.4192),
             "zenith_x": zsum((0.00165, 0.00375, 0.00209)) * tt + zsum((0.02903, 0.06377, 0.03202, 0.00394)) * t + zsum((0.11693, 0.21196, 0.06052, 0.25886)),
             "zenith_y": zsum((0.00275, 0.00610, 0.00317)) * tt + zsum((0.04214, 0.08970, 0.04153, 0.00516)) * t + zsum((0.15346, 0.26756, 0.06670, 0.26688)),
             "perez_Y": np.array([(abs(a) * t + abs(b)) * abs(v[j]) for j, (a, b) in enumerate(PEREZ_Y)]),
             "perez_x": np.array([(abs(a) * t + abs(b)) * abs(v[j]) for j, (a, b) in enumerate(PEREZ_x)]),
             "perez_y": np.array([(abs(a) * t + abs(b)) * abs(v[j]) for j, (a, b) in enumerate(PEREZ_y)])}
    return k, scale


# ---- sunsky: getSkyCol, in the reference's precision mix -------------------------------------------------------------
def _nudged(x, n):
    """a double library result moved n ulps (n in -1, 0, 1)"""
    return x if n == 0 else np.nextafter(x, np.inf if n > 0 else -np.inf)


def _facos(x, n=0):
    """fAcos__ (util_math_optimizations.h:255-261) of float32 values: the double acos, nudged, narrowed"""
    x = np.asarray(x, np.float32).astype(f64)
    with np.errstate(invalid="ignore"):
        a = _nudged(np.arccos(np.clip(x, -1.0, 1.0)), n).astype(np.float32)
    return np.where(x <= -1.0, F(M_PI), np.where(x >= 1.0, F(0), a)).astype(np.float32)


def _fexp(a):
    """fExp__ = fExp2__((float) M_LOG2E * a), util_math_optimizations.h:116-129, :194-201"""
    x = F(1.4426950408889634074) * np.asarray(a, np.float32)
    x = np.where(F(129.0) < x, F(129.0), x)
    x = np.where(x < F(-126.99999), F(-126.99999), x).astype(np.float32)
    ip = (x - F(0.5)).astype(np.int32)
    p = (x - ip.astype(np.float32)).astype(np.float32)
    e = ((ip + 127) << 23).astype(np.int32).view(np.float32)
    poly = (p * (p * (p * (p * (p * F(1.8775767e-3) + F(8.9893397e-3)) + F(5.5826318e-2)) + F(2.4015361e-1)) + F(6.9315308e-1)) + F(9.9999994e-1))
    return (e * poly).astype(np.float32)


def _exp_or_cap(v):
    with np.errstate(all="ignore"):
        return np.where(v <= 230.0, _fexp(np.asarray(v, f64).astype(np.float32)).astype(f64), 7.7220185e99)


def _perez(lam, theta_s, cos_theta, gamma, lvz):
    """perezFunction, background_sunsky.cc:83-105"""
    e_1 = _exp_or_cap(np.full_like(gamma, lam[1]))
    e_2 = _exp_or_cap(np.full_like(gamma, lam[3] * theta_s))
    with np.errstate(all="ignore"):
        e_3 = _exp_or_cap(lam[1] / cos_theta)
    e_4 = _exp_or_cap(lam[3] * gamma)
    cs = f64(np_fcos(F(theta_s)))
    cg = np_fcos(gamma.astype(np.float32)).astype(f64)
    den = (1 + lam[0] * e_1) * (1 + lam[2] * e_2 + lam[4] * cs * cs)
    num = (1 + lam[0] * e_3) * (1 + lam[2] * e_4 + lam[4] * cg * cg)
    return lvz * num / den


NUDGES = ("acos_theta", "atan2", "cos", "acos_gamma")      # the double library results of getSkyCol


def sunsky_eval(k, dirs, nudge=None):
    """power_ * getSkyCol(dir), :116-179; k: the sky record as the device has it.  nudge: {name of NUDGES: +-1}, which moves that double
    library result by one ulp before it is used"""
    nudge = nudge or {}
    iw = normalize32(dirs)
    ts = f64(k["theta_s"]); ps = f64(k["phi_s"])
    theta = _facos(iw[:, 2], nudge.get("acos_theta", 0)).astype(f64)
    below = theta > (0.5 * M_PI)
    hfade = 1.0 - (theta * M_1_PI - 0.5) * 2.0
    hfade = np.where(below, hfade * hfade * (3.0 - 2.0 * hfade), 1.0)
    theta = np.where(below, 0.5 * M_PI, theta)
    nfade = np.ones_like(theta)
    if ts > (0.5 * M_PI):
        n = 1.0 - (0.5 - theta * M_1_PI) * 2.0
        n = n * (1.0 - (ts * M_1_PI - 0.5) * 2.0)
        nfade = np.where(theta <= 0.5 * M_PI, n * n * (3.0 - 2.0 * n), 1.0)
    pole = (iw[:, 1] == 0) & (iw[:, 0] == 0)
    phi = np.where(pole, M_PI * 0.5, _nudged(np.arctan2(iw[:, 1].astype(f64), iw[:, 0].astype(f64)), nudge.get("atan2", 0)))
    # angleBetween: the sum of products is float
    cospsi = (np_fsin(theta.astype(np.float32)) * np_fsin(F(ts)) * np_fcos((ps - phi).astype(np.float32))
              + np_fcos(theta.astype(np.float32)) * np_fcos(F(ts))).astype(np.float32).astype(f64)
    gamma = np.where(cospsi > 1, 0.0, np.where(cospsi < -1, M_PI, _facos(cospsi.astype(np.float32), nudge.get("acos_gamma", 0)).astype(f64)))
    cos_theta = _nudged(np.cos(theta), nudge.get("cos", 0))
    x = _perez(k["perez_x"], ts, cos_theta, gamma, f64(k["zenith_x"]))
    y = _perez(k["perez_y"], ts, cos_theta, gamma, f64(k["zenith_y"]))
    Y = 6.666666667e-5 * nfade * hfade * _perez(k["perez_Y"], ts, cos_theta, gamma, f64(k["zenith_Y"]))
    with np.errstate(all="ignore"):
        X = (x / y) * Y
        z = ((1.0 - x - y) / y) * Y
        rgb = np.stack([3.240479 * X - 1.537150 * Y - 0.498535 * z, -0.969256 * X + 1.875992 * Y + 0.041556 * z,
                        0.055648 * X - 0.204043 * Y + 1.057311 * z], axis=1).astype(np.float32)
    rgb = np.where(rgb < 0, F(0), np.where(rgb > 1, F(1), rgb)).astype(np.float32)      # clampRgb01
    rgb = np.where((y == 0)[:, None], F(0), rgb).astype(np.float32)
    return (rgb * F(k["power"])).astype(np.float32)


def sky_eval(kind, sky, dirs, nudge=None):
    return gradient_eval(sky, dirs) if kind == KIND_GRADIENT else sunsky_eval(sky, dirs, nudge)


# ---- the background light's tables over a sky ------------------------------------------------------------------------
def table_dirs():
    """the directions BackgroundLight::init evaluates (light_background.cc:78-120), row after row, and each one's row"""
    fy, sintheta, nu = row_counts()
    fx = np.concatenate([(np.arange(n, dtype=np.float32) + F(0.5)) * (F(1) / F(n)) for n in nu])
    yy = np.repeat(np.arange(NV), nu)
    return inv_spheremap(fx, fy[yy]), yy, sintheta, nu


def sky_func(col, yy, sintheta):
    """func_ of the rows from the colours at table_dirs(): Rgb::energy times the row's sine"""
    return (((col[:, 0] + col[:, 1] + col[:, 2]) * F(0.333333)) * sintheta[yy]).astype(np.float32)


def sky_tables(col, yy, sintheta, nu):
    """the tables in the device's layout (tests/test_gpu_ibl.py: tables) from the colours at table_dirs()"""
    fu = sky_func(col, yy, sintheta)
    tab = np.zeros((NV + 1, ROW), np.float32)
    start = np.concatenate([[0], np.cumsum(nu)])
    with np.errstate(all="ignore"):
        for y in range(NV):
            tab[y] = pdf1d(fu[start[y]:start[y + 1]])
        tab[NV] = pdf1d(tab[:NV, 1].copy())
    return tab
