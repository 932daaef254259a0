"""TEST SUPPORT: the IES photometric files the IES tests read, written by the tests themselves (a few lines of text each), and the float32
restatement of what the reference does with such a file: the parser's results (IesData::parseIesFile, util_ies.h:135-376), getRadiance
(:65-131) and IesLight's getAngles, illuminate and illumSample (light_ies.cc:51-121), operation for operation, in numpy float32 on top of
the fSin__ / fCos__ / fSqrt__ / createCs__ / sampleCone__ restatements of tests/test_lights_host.py and np_facos of tests/test_gpu_ibl.py.
Shared by tests/test_ies_host.py and tests/test_gpu_ies.py."""
import os

import numpy as np

from tests.test_gpu_ibl import np_facos
from tests.test_lights_host import F, create_cs, dot, fcos, fsqrt, normalize, sample_cone

D2R = 0.01745329251994329576922          # DEG_TO_RAD, util_math_optimizations.h:94
R2D = 57.29577951308232087684636         # RAD_TO_DEG, :95
M_PI_2 = 1.57079632679489661923

# name -> type, horizontal angles, vertical angles, table rows (one per horizontal angle), tilt block
SPECS = {
    # one horizontal angle: the parser adds a second one at 180 with the same column
    "C1": (1, [0], [0, 22.5, 45, 67.5, 90], [[100, 90, 60, 30, 5]], None),
    # unequal steps, distinct values
    "C5x7": (1, [0, 70, 180, 250, 360], [0, 10, 35, 60, 90, 130, 180],
             [[310, 300, 250, 190, 120, 60, 20], [305, 290, 241, 181, 111, 52, 18], [295, 280, 230, 170, 100, 45, 12],
              [301, 285, 236, 177, 108, 49, 15], [310, 300, 250, 190, 120, 60, 20]], None),
    # horizontal angles up to 90: the quadrant fold
    "C90": (1, [0, 30, 90], [0, 30, 60, 90], [[50, 40, 30, 10], [45, 36, 22, 8], [40, 31, 17, 4]], None),
    # vertical angles that start above 0: the shift
    "Cup": (1, [0, 90, 180], [90, 120, 150, 180], [[5, 20, 40, 70], [6, 24, 44, 75], [8, 27, 49, 81]], None),
    "B": (2, [-90, -30, 0, 45, 90], [0, 30, 60, 90],
          [[10, 12, 9, 3], [30, 33, 21, 6], [60, 55, 34, 9], [41, 37, 20, 5], [14, 11, 7, 2]], None),
    "TILT": (1, [0, 90, 180], [0, 45, 90], [[9, 7, 2], [8, 6, 1.5], [7, 5, 1]], (1, [0, 15, 30, 45], [1, 0.95, 0.9, 0.85])),
    "FLAT": (1, [0], [0, 30, 60, 90], [[1, 1, 1, 1]], None),
}


def text(name):
    t, hor, vert, table, tilt = SPECS[name]
    num = lambda xs: " ".join(repr(float(x)) if float(x) != int(x) else str(int(x)) for x in xs)
    lines = ["IESNA:LM-63-1995", "[TEST] " + name, "[MANUFAC] written by tests/ies_fixture.py"]
    if tilt:
        lines += ["TILT=INCLUDE", str(tilt[0]), str(len(tilt[1])), num(tilt[1]), num(tilt[2])]
    else:
        lines += ["TILT=NONE"]
    lines += ["1 1000 1 %d %d %d 2 0 0 0" % (len(vert), len(hor), t), "1 1 100", num(vert), num(hor)]
    lines += [num(row) for row in table]
    return "\n".join(lines) + "\n"


def write(directory, name, body=None):
    path = os.path.join(str(directory), name + ".ies")
    with open(path, "w") as f:
        f.write(text(name) if body is None else body)
    return path


# ---- the restatement ------------------------------------------------------------------------------------------------
def parsed(name):
    """what parseIesFile leaves: type, hor, vert, table (n_hor, n_vert), max_rad, max_v_angle (radians), all float32"""
    t, hor, vert, table, _ = SPECS[name]
    hor = np.array(hor, np.float32); vert = np.array(vert, np.float32); table = np.array(table, np.float32)
    max_v = max(F(0), vert.max())
    if vert[0] > 0:
        minus = vert[0]
        max_v = F(max_v - minus)
        vert = vert - minus
    max_v_angle = np.float32(np.float64(max_v) * D2R)
    if t == 1 and hor.size == 1:
        hor = np.array([hor[0], 180], np.float32)
        table = np.vstack([table, table])
    return {"type": t, "hor": hor, "vert": vert, "table": table, "max_rad": F(1) / max(F(0), table.max()), "max_v_angle": max_v_angle}


def _cell(m, a):
    """the scans of getRadiance (:93-108) without their read of map[n]: the interval that holds the angle, 0 where none does"""
    x = np.zeros(a.shape, np.int64)
    for i in range(m.size - 1):
        x = np.where((m[i] <= a) & (m[i + 1] > a), i, x)
    return x


def radiance(ies, h_ang, v_ang):
    """IesData::getRadiance, util_ies.h:65-131"""
    h = np.asarray(h_ang, np.float32); v = np.asarray(v_ang, np.float32)
    hm, vm, tab = ies["hor"], ies["vert"], ies["table"]
    if ies["type"] == 1:
        a1, a2 = h, v
    else:
        a1, a2 = v, h
        if ies["type"] == 2:
            a1 = a1 + F(90)
            a1 = np.where(a1 > F(360), a1 - F(360), a1)
    if hm[-1] <= F(180):
        a1 = np.where(a1 > F(180), F(360) - a1, a1)
    if hm[-1] <= F(90):
        a1 = np.where(a1 > F(90), a1 - F(90), a1)
    if vm[-1] <= F(90):
        a2 = np.where(a2 > F(90), a2 - F(90), a2)
    x, y = _cell(hm, a1), _cell(vm, a2)
    exact = (a1 == hm[x]) & (a2 == vm[y])
    with np.errstate(all="ignore"):
        d_x = (a1 - hm[x]) / (hm[x + 1] - hm[x])
        d_y = (a2 - vm[y]) / (vm[y + 1] - vm[y])
        rx_1 = ((F(1) - d_x) * tab[x, y]) + (d_x * tab[x + 1, y])
        rx_2 = ((F(1) - d_x) * tab[x, y + 1]) + (d_x * tab[x + 1, y + 1])
        rad = ((F(1) - d_y) * rx_1) + (d_y * rx_2)
    return (np.where(exact, tab[x, y], rad) * ies["max_rad"]).astype(np.float32)


def angles(d, costheta):
    """IesLight::getAngles, light_ies.cc:51-61: the world z and y of the direction"""
    z = d[..., 2]
    u = np.where(z >= F(1), F(0), (np_facos(z).astype(np.float64) * R2D).astype(np.float32))
    u = np.where(d[..., 1] < 0, F(360) - u, u).astype(np.float32)
    v = np.where(costheta >= F(1), F(0), (np_facos(costheta).astype(np.float64) * R2D).astype(np.float32)).astype(np.float32)
    return u, v


def consts(ies, frm, to, color, power):
    """IesLight's constructor, light_ies.cc:30-49"""
    ndir = normalize(np.array(frm, np.float32) - np.array(to, np.float32))
    du, dv = create_cs(-ndir)
    return {"position": np.array(frm, np.float32), "ndir": ndir, "du": du[0], "dv": dv[0],
            "cos_end": fcos(ies["max_v_angle"])[()],
            "color": np.array(color, np.float32) * F(power)}


def _to_light(c, p):
    ldir = c["position"] - p
    dist_sqr = dot(ldir, ldir)
    with np.errstate(all="ignore"):
        dist = fsqrt(dist_sqr)
        idist_sqr = F(1) / dist_sqr
        ldir = ldir * (F(1) / dist)[:, None]
        cosa = dot(np.broadcast_to(c["ndir"], ldir.shape), ldir)
        ok = ~(dist == 0) & ~(cosa < c["cos_end"])
    return ldir.astype(np.float32), dist, idist_sqr, cosa, ok


def illuminate(ies, c, p):
    """IesLight::illuminate, :63-89 -> (n, 8): ok, wi.dir_, wi.tmax_, colour (zeros where it refuses)"""
    ldir, dist, idist_sqr, cosa, ok = _to_light(c, p)
    with np.errstate(all="ignore"):
        u, v = angles(ldir, cosa)
        rad = radiance(ies, u, v)
        col = (c["color"][None, :] * rad[:, None]) * idist_sqr[:, None]
    out = np.zeros((p.shape[0], 8), np.float32)
    out[:, 0] = ok; out[ok, 1:4] = ldir[ok]; out[ok, 4] = dist[ok]; out[ok, 5:8] = col[ok]
    return out


def illum_sample(ies, c, p, s_1, s_2):
    """IesLight::illumSample, :91-121 -> (n, 9): ok, wi.dir_, wi.tmax_, pdf, ls.col (zeros where it refuses)"""
    ldir, dist, idist_sqr, cosa, ok = _to_light(c, p)
    n = p.shape[0]
    with np.errstate(all="ignore"):
        wdir = sample_cone(ldir, np.broadcast_to(c["du"], (n, 3)), np.broadcast_to(c["dv"], (n, 3)), cosa, s_1, s_2).astype(np.float32)
        u, v = angles(wdir, cosa)
        rad = radiance(ies, u, v)
        ok = ok & ~(rad == 0)
        col = c["color"][None, :] * idist_sqr[:, None]
        pdf = F(1) / rad
    out = np.zeros((n, 9), np.float32)
    out[:, 0] = ok; out[ok, 1:4] = wdir[ok]; out[ok, 4] = dist[ok]; out[ok, 5] = pdf[ok]; out[ok, 6:9] = col[ok]
    return out
