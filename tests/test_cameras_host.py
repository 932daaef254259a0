"""The architect, angular and equirectangular cameras on the HOST: factories, refusals, XML — and the float32 restatement of the three
classes (src/camera/camera_architect.cc, camera_angular.cc, camera_equirectangular.cc over camera.cc and camera_perspective.cc) that
tests/test_gpu_cameras.py holds the device to.

The restatement is written operation for operation in numpy float32.  fSin__ / fCos__ / fSqrt__ are the oracle library's (through
tests/test_lights_host.py); the four libm calls of the angular camera (tan in the constructor; atan2, asin, atan in shootRay) are the
np.float64 functions narrowed, as the reference's unqualified calls resolve to the double C functions.  These cameras are held to this
restatement, not to the reference's compiled sources."""
import numpy as np
import pytest

from libyafaray_amd import Interface
from tests.test_lights_host import cross, dot, fcos, fsin, fsqrt, normalize

F = np.float32
D = np.float64
M_PI, M_PI_2, M_2PI = 3.14159265358979323846, 1.57079632679489661923, 6.28318530717958647692
D2R = 0.01745329251994329576922          # DEG_TO_RAD, util_math_optimizations.h:94
PERSPECTIVE, ARCHITECT, ANGULAR, EQUIRECTANGULAR = 0, 1, 2, 3
PROJECTIONS = {"equidistant": 0, "orthographic": 1, "stereographic": 2, "equisolid_angle": 3, "rectilinear": 4}
BOKEH = {"disk1": 0, "disk2": 1, "triangle": 3, "square": 4, "pentagon": 5, "hexagon": 6, "ring": 7}
BIAS = {"uniform": 0, "center": 1, "edge": 2}


def v3(p):
    return np.array(p, dtype=F)


# ---- the factories and constructors, restated as record builders -----------------------------------------------------
def base_record(p, far_default):
    """Camera::Camera, camera.cc:46-66"""
    frm, to, up = v3(p.get("from", (0, 1, 0))), v3(p.get("to", (0, 0, 0))), v3(p.get("up", (0, 1, 1)))
    resx, resy = int(p.get("resx", 320)), int(p.get("resy", 200))
    near, far = F(p.get("nearClip", 0.0)), F(p.get("farClip", far_default))
    aspect_ratio = F(F(F(p.get("aspect_ratio", 1.0)) * F(resy)) / F(resx))
    cy, cz = up - frm, to - frm
    cx = cross(cz, cy)
    cy = cross(cz, cx)
    cx, cy, cz = normalize(cx), normalize(cy), normalize(cz)
    z3 = np.zeros(3, F)
    return {"position": frm, "near_n": cz.copy(), "near_p": frm + cz * near, "far_n": cz.copy(), "far_p": frm + cz * far,
            "resx": resx, "resy": resy, "cam_x": cx, "cam_y": cy, "cam_z": cz, "aspect_ratio": aspect_ratio,
            "aperture": F(0), "dof_distance": F(0), "bokeh_type": 0, "bokeh_bias": 0, "bokeh_rotation": F(0), "dof_rt": z3.copy(), "dof_up": z3.copy(),
            "focal_distance": F(0), "type": PERSPECTIVE, "focal_length": F(0), "max_radius": F(0), "circular": 0, "projection": 0}


def perspective_record(p):
    """PerspectiveCamera::factory, ctor, setAxis: camera_perspective.cc:198-243, :29-54, :60-74"""
    r = base_record(p, -1.0)
    focal, apt = F(p.get("focal", 1.0)), F(p.get("aperture", 0.0))
    vright = r["cam_x"].copy()
    vup = r["aspect_ratio"] * r["cam_y"]
    r["vto"] = focal * r["cam_z"] - F(0.5) * (vup + vright)
    r["vup"], r["vright"] = vup / F(r["resy"]), vright / F(r["resx"])
    r.update(focal_distance=focal, aperture=apt, dof_distance=F(p.get("dof_distance", 0.0)), bokeh_rotation=F(p.get("bokeh_rotation", 0.0)),
             bokeh_type=BOKEH.get(p.get("bokeh_type", "disk1"), 0), bokeh_bias=BIAS.get(p.get("bokeh_bias", "uniform"), 0),
             dof_rt=apt * r["cam_x"], dof_up=apt * r["cam_y"])
    return r


def architect_record(p):
    """ArchitectCamera: PerspectiveCamera's factory parameters and ctor, then its own setAxis (camera_architect.cc:52-66):
    vup_ = aspect_ratio_ * Vec3(0, 0, -1), vto_ from that vup_; dof_up_ still follows cam_y_"""
    r = perspective_record(p)
    vright = r["cam_x"].copy()
    vup = r["aspect_ratio"] * v3((0, 0, -1))
    r["vto"] = r["cam_z"] * r["focal_distance"] - F(0.5) * (vup + vright)
    r["vup"] = vup / F(r["resy"])
    r["type"] = ARCHITECT
    return r


def equirectangular_record(p):
    """EquirectangularCamera::factory, ctor, setAxis: camera_equirectangular.cc:67-90, :29-47"""
    r = base_record(p, -1.0e38)
    r.update(vright=r["cam_x"].copy(), vup=r["cam_y"].copy(), vto=r["cam_z"].copy(), type=EQUIRECTANGULAR)
    return r


def angular_record(p):
    """AngularCamera::factory, ctor, setAxis: camera_angular.cc:82-121, :29-53.  An `aperture` in the ParamMap is not even read."""
    r = base_record(p, -1.0e38)
    angle_degrees = float(p.get("angle", 90.0))
    max_angle_degrees = float(p.get("max_angle", angle_degrees))
    angle, max_angle = F(angle_degrees * M_PI / 180.0), F(max_angle_degrees * M_PI / 180.0)
    proj = PROJECTIONS.get(p.get("projection", ""), 0)
    if proj == 1:
        focal = F(1) / fsin(angle)
    elif proj == 2:
        focal = F(D(F(1) / F(2)) / np.tan(D(angle / F(2))))          # the double tan(), narrowed
    elif proj == 3:
        focal = F(1) / F(2) / fsin(angle / F(2))
    elif proj == 4:
        focal = F(D(1.0) / np.tan(D(angle)))
    else:
        focal = F(1) / angle
    vright = r["cam_x"].copy()
    if p.get("mirrored", False):
        vright = vright * F(-1.0)                                       # :116, after the ctor: cam_x_ stays
    r.update(vright=vright, vup=r["cam_y"].copy(), vto=r["cam_z"].copy(), type=ANGULAR, focal_length=F(focal), max_radius=F(max_angle / angle),
             circular=int(bool(p.get("circular", True))), projection=proj)
    return r


RECORD = {"perspective": perspective_record, "architect": architect_record, "angular": angular_record, "equirectangular": equirectangular_record}


def bokeh_table(r):
    """the corner table of the polygonal bokeh shapes (camera_perspective.cc:41-53 = camera_architect.cc:37-49)"""
    ls = np.zeros(16, F)
    ns = r["bokeh_type"]
    if 3 <= ns <= 6:
        w, wi = F(float(r["bokeh_rotation"]) * D2R), F(M_2PI / float(F(ns)))
        for i in range(0, (ns + 2) * 2, 2):
            ls[i], ls[i + 1] = fcos(w), fsin(w)
            w = F(w + wi)
    return ls


# ---- shootRay --------------------------------------------------------------------------------------------------------
def col(x):
    return np.asarray(x, F)[:, None]


def plane_t(r, which, frm, dr):
    """rayPlaneIntersection__, util_geometry.h:34-37 (per row: the origin moves with the lens sample)"""
    with np.errstate(all="ignore"):
        return (dot(r[which + "_n"][None, :], r[which + "_p"][None, :] - frm) / dot(dr, r[which + "_n"][None, :])).astype(F)


def shirley_disk(r_1, r_2):
    """shirleyDisk__, vector.cc:155-190, row by row (the angle is formed in double and narrowed)"""
    u, v = np.zeros_like(r_1), np.zeros_like(r_1)
    k = M_PI / 4
    for i, (x, y) in enumerate(zip(r_1, r_2)):
        a, b = F(F(2) * x - F(1)), F(F(2) * y - F(1))
        if a > -b:
            rad, phi = (a, F(k * D(b / a))) if a > b else (b, F(k * D(F(2) - a / b)))
        elif a < b:
            rad, phi = -a, F(k * D(F(4) + b / a))
        else:
            rad, phi = -b, (F(k * D(F(6) - a / b)) if b != 0 else F(0))
        u[i], v[i] = rad * fcos(phi), rad * fsin(phi)
    return u, v


def lens_uv(r, lu, lv):
    """PerspectiveCamera::getLensUv / sampleTsd with bias `uniform` (camera_perspective.cc:91-129): disk1 and the polygons"""
    assert r["bokeh_bias"] == 0
    bt = r["bokeh_type"]
    if bt == 0:
        return shirley_disk(lu, lv)
    assert 3 <= bt <= 6
    ls, fn = bokeh_table(r), F(bt)
    idx = (lu * fn).astype(np.int32)
    r_1 = fsqrt((lu - idx.astype(F) / fn) * fn)
    b_1 = r_1 * lv
    b_0 = r_1 - b_1
    idx = idx << 1
    return ls[idx] * b_0 + ls[idx + 2] * b_1, ls[idx + 1] * b_0 + ls[idx + 3] * b_1


def shoot(r, px, py, lu=None, lv=None):
    """Camera::shootRay of the record's type over rows -> from (n,3), dir (n,3), tmin, tmax, wt.  Rows with wt == 0 carry no ray:
    their other columns are zero."""
    px, py = np.asarray(px, F), np.asarray(py, F)
    n = len(px)
    frm = np.repeat(r["position"][None, :], n, axis=0)
    wt = np.ones(n, F)
    if r["type"] in (PERSPECTIVE, ARCHITECT):                              # PerspectiveCamera::shootRay, camera_perspective.cc:133-156
        dr = normalize((r["vright"][None, :] * col(px) + r["vup"][None, :] * col(py)) + r["vto"][None, :])
        tmin, tmax = plane_t(r, "near", frm, dr), plane_t(r, "far", frm, dr)
        if r["aperture"] != 0:
            u, v = lens_uv(r, np.asarray(lu, F), np.asarray(lv, F))
            li = r["dof_rt"][None, :] * col(u) + r["dof_up"][None, :] * col(v)
            frm = frm + li
            dr = normalize(dr * r["dof_distance"] - li)
        return frm, dr, tmin, tmax, wt
    if r["type"] == EQUIRECTANGULAR:                                       # camera_equirectangular.cc:49-65
        u = F(2) * px / F(r["resx"]) - F(1)
        v = F(2) * py / F(r["resy"]) - F(1)
        phi, theta = (M_PI * u.astype(D)).astype(F), (M_PI_2 * v.astype(D)).astype(F)
        dr = col(fcos(theta)) * (col(fcos(phi)) * r["vto"][None, :] + col(fsin(phi)) * r["vright"][None, :]) + col(fsin(theta)) * r["vup"][None, :]
    else:                                                                  # camera_angular.cc:55-80
        u = F(1) - F(2) * (px / F(r["resx"]))
        v = (F(2) * (py / F(r["resy"])) - F(1)) * r["aspect_ratio"]
        radius = fsqrt(u * u + v * v)
        dead = (radius > r["max_radius"]) if r["circular"] else np.zeros(n, bool)
        wt[dead] = 0
        u, v, radius = np.where(dead, F(0), u), np.where(dead, F(0), v), np.where(dead, F(0), radius)
        theta = np.where((u == 0) & (v == 0), F(0), np.arctan2(v.astype(D), u.astype(D)).astype(F))
        fl, proj = r["focal_length"], r["projection"]
        with np.errstate(all="ignore"):
            if proj == 1:
                phi = np.arcsin((radius / fl).astype(D)).astype(F)
            elif proj == 2:
                phi = (2.0 * np.arctan((radius / (F(2) * fl)).astype(D))).astype(F)
            elif proj == 3:
                phi = (2.0 * np.arcsin((radius / (F(2) * fl)).astype(D))).astype(F)
            elif proj == 4:
                phi = np.arctan((radius / fl).astype(D)).astype(F)
            else:
                phi = radius / fl
        dr = col(fsin(phi)) * (col(fcos(theta)) * r["vright"][None, :] + col(fsin(theta)) * r["vup"][None, :]) + col(fcos(phi)) * r["vto"][None, :]
    tmin, tmax = plane_t(r, "near", frm, dr), plane_t(r, "far", frm, dr)
    tmin = np.where(np.isnan(tmin), F(0), tmin)       # the one deviation (DESIGN, "Cameras"): a 0 / 0 near distance is 0
    live = wt != 0
    return np.where(live[:, None], frm, F(0)), np.where(live[:, None], dr, F(0)), np.where(live, tmin, F(0)), np.where(live, tmax, F(0)), wt


# ---- screenproject ---------------------------------------------------------------------------------------------------
def screenproject(r, p):
    """Camera::screenproject of the record's type over rows of points -> (n, 3)"""
    p = np.asarray(p, F).reshape(-1, 3)
    z = np.zeros(len(p), F)
    with np.errstate(all="ignore"):
        if r["type"] == PERSPECTIVE:                                       # camera_perspective.cc:158-173
            d = p - r["position"][None, :]
            dx, dy, dz = dot(d, r["cam_x"][None, :]), dot(d, r["cam_y"][None, :]), dot(d, r["cam_z"][None, :])
            return np.stack([F(2) * dx * r["focal_distance"] / dz, F(-2) * dy * r["focal_distance"] / (dz * r["aspect_ratio"]), z], axis=-1)
        if r["type"] == ARCHITECT:                                         # camera_architect.cc:68-90
            d = p - r["position"][None, :]
            camy = v3((0, 0, 1))
            camz = cross(camy, r["cam_x"])
            camx = cross(camz, camy)
            dx, dy, dz = dot(d, camx[None, :]), dot(d, r["cam_y"][None, :]), dot(d, camz[None, :])
            fod = dot(r["focal_distance"] * camy, r["cam_y"]) / dot(camx, r["cam_x"])
            return np.stack([F(2) * dx * fod / dz, F(2) * dy * r["focal_distance"] / (dz * r["aspect_ratio"]), z], axis=-1)
        d = normalize(p - r["position"][None, :])                          # camera_angular.cc:123-140 = camera_equirectangular.cc:92-109
        dx, dy, dz = dot(r["cam_x"][None, :], d), dot(r["cam_y"][None, :], d), dot(r["cam_z"][None, :], d)
        den = (4.0 * M_PI) * dz.astype(D)
        return np.stack([((-dx).astype(D) / den).astype(F), ((-dy).astype(D) / den).astype(F), z], axis=-1)


# ---- through the C API -----------------------------------------------------------------------------------------------
def camera_of(params, name="cam"):
    yi = Interface(strict=False)
    yi.startScene(0)
    yi.paramsClearAll()
    yi.paramsSet(params)
    return yi, yi.createCamera(name)


def same_bits(a, b):
    return np.array_equal(np.atleast_1d(np.asarray(a, F)).view(np.uint32), np.atleast_1d(np.asarray(b, F)).view(np.uint32))


def assert_record(params):
    yi, h = camera_of(params)
    assert h, yi.getLastError()
    got, want = yi.getCamera("cam"), RECORD[params["type"]](params)
    for field, value in want.items():
        if field in Interface.CAMERA_INT_FIELDS:
            assert got[field] == value, (field, got[field], value)
        else:
            assert same_bits(got[field], value), (field, got[field], value)
    assert not got["ls"].any()         # the corner table is the device scene's to fill
    return got


TILTED = {"from": (0.3, -2.0, 1.6), "to": (0.0, 0.1, 0.2), "up": (0.4, -2.1, 2.6), "resx": 24, "resy": 16}


@pytest.mark.parametrize("t", ["architect", "angular", "equirectangular"])
def test_defaults_alone(t):
    got = assert_record({"type": t})
    assert got["type"] == {"architect": 1, "angular": 2, "equirectangular": 3}[t]
    assert got["resx"] == 320 and got["resy"] == 200
    assert same_bits(got["far_p"], got["position"] + got["cam_z"] * F(-1.0 if t == "architect" else -1.0e38))


def test_perspective_record_is_what_it_was():
    got = assert_record(dict(TILTED, type="perspective", focal=1.3, aperture=0.05, dof_distance=2.0, bokeh_type="pentagon"))
    assert got["type"] == 0 and got["focal_length"] == 0 and got["max_radius"] == 0 and got["circular"] == 0 and got["projection"] == 0


def test_tilted_architect_with_aperture_and_hexagon_bokeh():
    p = dict(TILTED, type="architect", focal=1.3, aperture=0.05, dof_distance=2.5, bokeh_type="hexagon", bokeh_rotation=10.0, aspect_ratio=1.1,
             nearClip=0.1, farClip=50.0)
    got = assert_record(p)
    per = perspective_record(p)
    assert got["bokeh_type"] == 6 and got["aperture"] == F(0.05)
    assert not same_bits(got["vup"], per["vup"]) and not same_bits(got["vto"], per["vto"])      # the camera is tilted: the verticals differ
    assert same_bits(got["vup"][:2], [0, 0]) and got["vup"][2] < 0
    assert same_bits(got["dof_up"], per["dof_up"]) and same_bits(got["vright"], per["vright"])


@pytest.mark.parametrize("projection", list(PROJECTIONS) + ["no such word"])
def test_angular_projections(projection):
    got = assert_record(dict(TILTED, type="angular", angle=80.0, max_angle=50.0, projection=projection, aspect_ratio=1.2))
    assert got["projection"] == PROJECTIONS.get(projection, 0)
    assert got["circular"] == 1 and got["max_radius"] == F(F(50.0 * M_PI / 180.0) / F(80.0 * M_PI / 180.0))


def test_angular_max_angle_defaults_to_angle():
    got = assert_record(dict(TILTED, type="angular", angle=70.0))
    assert got["max_radius"] == 1
    got = assert_record(dict(TILTED, type="angular", angle=70.0, max_angle=35.0, circular=False))
    assert got["max_radius"] == F(0.5) and got["circular"] == 0


def test_angular_mirrored_flips_vright_and_not_cam_x():
    plain = assert_record(dict(TILTED, type="angular", angle=70.0))
    mirrored = assert_record(dict(TILTED, type="angular", angle=70.0, mirrored=True))
    assert same_bits(mirrored["vright"], -plain["vright"]) and same_bits(mirrored["cam_x"], plain["cam_x"])
    assert same_bits(plain["vright"], plain["cam_x"])
    assert same_bits(mirrored["vup"], plain["vup"]) and same_bits(mirrored["vto"], plain["vto"])


@pytest.mark.parametrize("t", ["angular", "equirectangular"])
def test_aperture_stays_zero_without_a_lens(t):
    got = assert_record(dict(TILTED, type=t, aperture=0.3, dof_distance=2.0, bokeh_type="hexagon", focal=1.5))
    assert got["aperture"] == 0 and got["dof_distance"] == 0 and got["bokeh_type"] == 0 and not got["dof_rt"].any() and not got["dof_up"].any()


def test_equirectangular_every_parameter():
    got = assert_record(dict(TILTED, type="equirectangular", aspect_ratio=0.9, nearClip=0.2, farClip=30.0))
    assert same_bits(got["vto"], got["cam_z"]) and same_bits(got["vup"], got["cam_y"]) and same_bits(got["vright"], got["cam_x"])


# ---- refusals --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("angle", [0.0, -30.0])
def test_angle_must_be_positive(angle):
    yi, h = camera_of({"type": "angular", "angle": angle})
    assert not h
    assert "angle" in yi.getLastError()


@pytest.mark.parametrize("projection,params", [
    ("orthographic", {"angle": 90.0, "circular": False}),                       # the frame's corners lie past radius 1 = focal_length
    ("orthographic", {"angle": 60.0, "max_angle": 90.0}),                      # the circle is larger than the projection's domain
    ("equisolid_angle", {"angle": 40.0, "circular": False, "resx": 16, "resy": 64}),
])
def test_asin_domain_is_refused_at_the_boundary(projection, params):
    yi, h = camera_of(dict(params, type="angular", projection=projection))
    assert not h
    msg = yi.getLastError()
    assert "projection" in msg and projection in msg and "max_angle" in msg, msg


def test_asin_domain_reached_exactly_is_accepted():
    for projection in ("orthographic", "equisolid_angle"):
        yi, h = camera_of({"type": "angular", "projection": projection, "angle": 60.0, "max_angle": 45.0})
        assert h, yi.getLastError()


def test_orthographic_and_unknown_types_stay_out_of_scope():
    for t in ("orthographic", "fisheye", ""):
        yi, h = camera_of({"type": t})
        assert not h
        msg = yi.getLastError()
        assert "scope" in msg, msg
        for accepted in ("perspective", "architect", "angular", "equirectangular"):
            assert accepted in msg, msg


def test_get_camera_of_an_unknown_name_fails():
    yi, h = camera_of({"type": "architect"})
    assert h
    with pytest.raises(Exception):
        Interface.getCamera(_strict(yi), "no such camera")


def _strict(yi):
    yi.strict = True
    return yi


# ---- the restatement itself ------------------------------------------------------------------------------------------
def test_restated_rays_behave():
    """what the GPU tests lean on: unit-length directions where the axes are orthonormal, the circle, the centre, the seam"""
    r = angular_record(dict(TILTED, type="angular", angle=90.0, max_angle=60.0))
    px, py = np.meshgrid(np.arange(24, dtype=F) + F(0.5), np.arange(16, dtype=F) + F(0.5))
    frm, dr, tmin, tmax, wt = shoot(r, px.ravel(), py.ravel())
    assert 0.1 < (wt == 0).mean() < 0.9
    live = wt != 0
    assert np.allclose(np.linalg.norm(dr[live], axis=1), 1.0, atol=2e-3) and not dr[~live].any()
    assert (tmin[live] == 0).all() and not np.isnan(tmax).any()
    _, centre, _, _, w = shoot(r, [12.0], [8.0])
    assert w[0] == 1 and np.allclose(centre[0], r["cam_z"], atol=1e-3)
    e = equirectangular_record(dict(TILTED, type="equirectangular"))
    _, d, _, _, w = shoot(e, [0.0, 24.0, 12.0], [8.0, 8.0, 8.0])
    assert (w == 1).all()
    assert np.allclose(d[0], -e["cam_z"], atol=2e-3) and np.allclose(d[1], -e["cam_z"], atol=2e-3) and np.allclose(d[2], e["cam_z"], atol=2e-3)


def test_level_architect_restates_to_the_perspective_camera():
    p = {"from": (0, -3, 0), "to": (0, 0, 0), "up": (0, -3, 1), "resx": 24, "resy": 16, "focal": 1.2, "aperture": 0.1, "dof_distance": 3.0}
    a, b = architect_record(dict(p, type="architect")), perspective_record(dict(p, type="perspective"))
    assert same_bits(b["cam_y"], [0, 0, -1])
    for k in ("vto", "vup", "vright", "dof_rt", "dof_up"):
        assert same_bits(a[k], b[k]), k


# ---- XML -------------------------------------------------------------------------------------------------------------
XML = """<?xml version="1.0"?>
<scene type="triangle">
<material name="lamp"><type sval="light_mat"/><color r="1" g="0.5" b="0.25" a="1"/><power fval="1"/><double_sided bval="true"/></material>
<camera name="cam">%s</camera>
<integrator name="default"><type sval="directlighting"/><caustic_type sval="none"/></integrator>
<integrator name="volintegr"><type sval="none"/></integrator>
<mesh id="1" vertices="4" faces="2" has_orco="false" has_uv="false" type="0">
  <p x="-1" y="1" z="-1"/><p x="1" y="1" z="-1"/><p x="1" y="1" z="1"/><p x="-1" y="1" z="1"/>
  <set_material sval="lamp"/><f a="0" b="1" c="2"/><f a="0" b="2" c="3"/>
</mesh>
<render><camera_name sval="cam"/><integrator_name sval="default"/><volintegrator_name sval="volintegr"/>
  <width ival="24"/><height ival="16"/><AA_passes ival="1"/><AA_minsamples ival="1"/>
  <AA_pixelwidth fval="1"/><filter_type sval="box"/><tile_size ival="7"/></render>
</scene>
"""
COMMON = '<from x="0" y="-3" z="0.5"/><to x="0" y="0" z="0"/><up x="0" y="-3" z="1.5"/><resx ival="24"/><resy ival="16"/>'
XML_CAMERAS = {
    "architect": '<type sval="architect"/>' + COMMON + '<focal fval="1.2"/><aperture fval="0.05"/><dof_distance fval="3"/><bokeh_type sval="hexagon"/>',
    "angular": '<type sval="angular"/>' + COMMON + '<angle fval="90"/><max_angle fval="60"/><circular bval="true"/><mirrored bval="true"/>'
               '<projection sval="stereographic"/>',
    "equirectangular": '<type sval="equirectangular"/>' + COMMON,
}


@pytest.mark.parametrize("t", list(XML_CAMERAS))
def test_xml_scene_with_the_camera_loads(tmp_path, t):
    path = tmp_path / f"{t}.xml"
    path.write_text(XML % XML_CAMERAS[t])
    yi = Interface(strict=False)
    assert yi.loadXml(str(path)), yi.getLastError()
    got = yi.getCamera("cam")
    assert got["type"] == {"architect": 1, "angular": 2, "equirectangular": 3}[t] and got["resx"] == 24 and got["resy"] == 16
    if t == "angular":
        assert got["projection"] == 2 and got["circular"] == 1 and same_bits(got["vright"], -got["cam_x"])
    if t == "architect":
        assert got["bokeh_type"] == 6 and got["aperture"] == F(0.05)


def prepare_only(yi):
    """prepareRender flattens the scene and creates the device scene: without a device it must fail there and nowhere earlier"""
    ok = yi.prepareRender()
    return ok, yi.getLastError()


@pytest.mark.parametrize("t", list(XML_CAMERAS))
def test_prepare_render_accepts_the_camera(tmp_path, t):
    path = tmp_path / f"{t}.xml"
    path.write_text(XML % XML_CAMERAS[t])
    yi = Interface(strict=False)
    assert yi.loadXml(str(path)), yi.getLastError()
    ok, msg = prepare_only(yi)
    assert ok or ("camera" not in msg.lower() and "scope" not in msg), msg


# ---- the reference's compiled cameras ----------------------------------------------------------------------------------
# tests/golden/ref_cameras_{ieee,fast}.json.gz: ArchitectCamera, AngularCamera and EquirectangularCamera made by their factories in the
# reference harness (oracle/ref_harness/ref_cameras.cc), the 26 configurations of tests/test_gpu_cameras.py::RAY_CONFIGS
from tests import pin_fixture as pin                                   # noqa: E402
from tests.test_oracle_golden import FAST_ATOL, FAST_RTOL              # noqa: E402

PINNED = pin.load("cameras", "ieee")["sets"]


def pinned_camera(doc, name):
    return pin.params(doc, name)


def rays_against(rec, inp, want, what, angular):
    """shoot() against fixture rows (n, 9) as bit patterns -> the share of live rows that are not bit-exact.  wt bit for bit on every row;
    the other words bit for bit too, but that an angular row may differ where a double libm result narrows to the neighbouring float: at
    most 0.1 % of the live rows, each within 1e-6 per direction component, origins exact (the rule of
    tests/test_gpu_cameras.py::test_rays_bit_for_bit)"""
    frm, dr, tmin, tmax, wt = shoot(rec, inp[:, 0], inp[:, 1], inp[:, 2], inp[:, 3])
    assert np.array_equal(wt.view(np.uint32), want[:, 8]), f"{what}: wt"
    live = wt != 0
    got = np.column_stack([frm, dr, tmin, tmax]).astype(F)
    assert not got[~live].any() and not want[~live, :8].any()
    g, w = got[live].view(np.uint32), want[live, :8]
    differ = ((g != w) & ~(((g | w) & 0x7fffffff) == 0)).any(axis=1)
    if not angular:
        assert not differ.any(), f"{what}: {int(differ.sum())} rows differ, first {inp[live][differ][0]}: {got[live][differ][0]} vs {w[differ][0].view(F)}"
        return 0.0
    share = float(differ.mean())
    worst = float(np.abs(got[live][differ, 3:6].astype(D) - w[differ, 3:6].view(F)).max()) if differ.any() else 0.0
    assert share <= 0.001 and worst <= 1e-6, (what, share, worst)
    assert np.array_equal(g[differ, :3], w[differ, :3])
    return share


def test_fixture_configurations_are_the_gpu_tests_configurations():
    from tests.test_gpu_cameras import RAY_CONFIGS
    doc = pin.load("cameras", "ieee")
    assert [doc[n + "_label"] for n in doc["sets"]] == [what for what, _ in RAY_CONFIGS]
    for name, (_, cam) in zip(doc["sets"], RAY_CONFIGS):
        want = {k: (tuple(float(F(x)) for x in v) if isinstance(v, tuple) else (float(F(v)) if isinstance(v, float) else v)) for k, v in cam.items()}
        got = {k: (float(F(v)) if isinstance(v, float) else v) for k, v in pinned_camera(doc, name).items()}
        assert got == want, name


@pytest.mark.parametrize("name", PINNED)
def test_restatement_reproduces_the_reference(name):
    """shoot() and screenproject() of the restated record against the IEEE fixture, the C ABI's record against the restated one (so its
    words are held to the reference's factory and constructor through the rays), the rows the fixture promises, and the circle's radius
    between the radii of the rows the reference took and refused"""
    doc = pin.load("cameras", "ieee")
    cam = pinned_camera(doc, name)
    rec = assert_record(cam)
    rec = {k: (np.asarray(v, F) if np.ndim(v) else v) for k, v in rec.items()}
    inp, want, _ = pin.leaf(doc, name, "shoot")
    angular = cam["type"] == "angular"
    assert rays_against(RECORD[cam["type"]](cam), inp, want, doc[name + "_label"], angular) == rays_against(rec, inp, want, "the C ABI's record", angular)
    # the 81 pixel-boundary rows (a 0 / 0 near distance moves a row a few float steps, ref_cameras.cc), the four corners, the exact centre
    gx, gy = np.meshgrid(np.arange(0, 25, 3, dtype=F), np.arange(0, 17, 2, dtype=F))
    assert np.abs(inp[:81, 0] - gx.ravel()).max() < 1e-5 and np.abs(inp[:81, 1] - gy.ravel()).max() < 1e-5
    assert all(((inp[:81, 0] == a) & (inp[:81, 1] == b)).any() for a in (0, 24) for b in (0, 16))
    assert np.array_equal(inp[81], np.array([12, 8, 0.5, 0.5], F))
    out = want.view(F)
    dead = out[:, 8] == 0
    assert not np.isnan(out).any()
    if angular and cam["circular"]:
        assert 0.1 <= dead.mean() <= 0.9
        r = RECORD["angular"](cam)
        u = F(1) - F(2) * (inp[:, 0] / F(r["resx"]))
        v = (F(2) * (inp[:, 1] / F(r["resy"])) - F(1)) * r["aspect_ratio"]
        radius = fsqrt(u * u + v * v)
        assert radius[~dead].max() <= rec["max_radius"] < radius[dead].min()
        circle = slice(82, 82 + 16 * 7)
        assert dead[circle].sum() >= 16 and (~dead[circle]).sum() >= 16
        assert radius[dead].min() - radius[~dead].max() <= 2.0 ** -23, "rows within a float step either side of the circle"
    else:
        assert not dead.any()
    p, want, _ = pin.leaf(doc, name, "project")
    s = screenproject(rec, p)
    pin.same(s, want, f"{name} screenproject")
    assert np.isfinite(s).all() and len(np.unique(s[:, 0])) == len(p)


def test_release_flag_build_of_the_reference_agrees():
    """the two builds of the reference against each other (a sample without a ray in one and with one in the other: below 1 % per
    configuration), then the restatement against the release-flag one with the tolerances every release-flag fixture is compared with"""
    ieee, fast = pin.load("cameras", "ieee"), pin.load("cameras", "fast")
    worst = 0.0
    for name in ieee["sets"]:
        cam = pinned_camera(ieee, name)
        rec = RECORD[cam["type"]](cam)
        inp, a, _ = pin.leaf(ieee, name, "shoot")
        inp_f, b, _ = pin.leaf(fast, name, "shoot")
        # the same questions, the rows moved off a 0 / 0 near distance included (both builds meet it at the same floats), and no NaN in either
        assert np.array_equal(inp.view(np.uint32), inp_f.view(np.uint32)), name
        assert not np.isnan(a.view(F)).any() and not np.isnan(b.view(F)).any(), name
        a, b = a.view(F).astype(D), b.view(F).astype(D)
        differ = a[:, 8] != b[:, 8]
        assert differ.mean() < 0.01, (name, differ.mean())
        frm, dr, tmin, tmax, wt = shoot(rec, inp_f[:, 0], inp_f[:, 1], inp_f[:, 2], inp_f[:, 3])
        got = np.column_stack([frm, dr, tmin, tmax, wt]).astype(D)
        agree = ~differ
        with np.errstate(invalid="ignore"):
            between = np.abs(a - b)[agree]
            worst = max(worst, float(np.nanmax(between / np.maximum(np.abs(b[agree]), 1.0))))
        close = np.isclose(got[agree], b[agree], rtol=FAST_RTOL, atol=FAST_ATOL)
        assert close.all(), (name, inp_f[agree][~close.all(axis=1)][:3], got[agree][~close.all(axis=1)][:3], b[agree][~close.all(axis=1)][:3])
        p, a, _ = pin.leaf(ieee, name, "project")
        p_f, b, _ = pin.leaf(fast, name, "project")
        assert np.array_equal(p.view(np.uint32), p_f.view(np.uint32))
        assert np.isclose(screenproject(rec, p_f).astype(D), b.view(F).astype(D), rtol=FAST_RTOL, atol=FAST_ATOL).all(), name
    print(f"largest difference between the two builds of the reference (relative, absolute below 1): {worst:.3g}")
