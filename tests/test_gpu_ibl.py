"""Image-based lighting on the DEVICE: the background light's Pdf1D tables and its leaf functions bit for bit against a float32
restatement in the reference's operation order (light_background.cc, background_texture.cc, texture.h:83-140, util_sample.h:89-141;
probe ops 22-25), escaping rays against the background evaluated per camera ray, the texture path against the constant path, ray
counts, occlusion and transparent shadows on the light's infinite rays, the estimator's mean against a quadrature of
doLightEstimation's two halves, importance sampling, caustic paths that escape, the serial-state replay with sharding and pass
pipelining."""
import ctypes as C
import os

import numpy as np
import pytest

from libyafaray_amd import Interface, scenes
from oracle import pyoracle as po
from tests.test_gpu_components import exact
from tests.test_gpu_lights import K_MIS_FLAGS, RHO, occluder, plane_points, plane_scene, render
from tests.test_lights_host import F, fcos, fsin, fsqrt

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "tests", "golden", "test01_tex.hdr")
M_PI, M_2PI, M_1_PI, M_1_2PI, M_PI_2 = 3.14159265358979323846, 6.28318530717958647692, 0.31830988618379067154, 0.15915494309189533577, 1.57079632679489661923
NV, MAXU, MINU = 360, 720, 16            # MAX_VSAMPLES, MAX_USAMPLES, MIN_SAMPLES (light_background.cc:33-35)
ROW = 4 + MAXU + MAXU + 1                # count, integral, 1 / integral, 1 / count, func_, cdf_
f64 = np.float64


@pytest.fixture(scope="module", autouse=True)
def torch_first():
    """the emulated shard exchange hands device memory to torch: let torch open the GPU before the library does"""
    import torch
    torch.cuda.init()


# ---- float32 restatements, vectorised ------------------------------------------------------------------------------
def np_fsin(x):
    """fSin__ with FAST_TRIG (util_math_optimizations.h:222-244) on arrays; test_restatements_agree holds it to the oracle library's"""
    x = np.array(x, dtype=np.float32)
    big = (x.astype(f64) > M_2PI) | (x.astype(f64) < -M_2PI)
    with np.errstate(invalid="ignore"):
        x = np.where(big, x - (x * F(M_1_2PI)).astype(np.int32).astype(np.float32) * F(M_2PI), x)
    x = np.where(x.astype(f64) < -M_PI, x + F(M_2PI), np.where(x.astype(f64) > M_PI, x - F(M_2PI), x))
    x = (F(1.27323954473516268615) * x) - (F(0.40528473456935108578) * x * np.abs(x))
    r = F(0.225) * (x * np.abs(x) - x) + x
    return np.where(r <= F(-1), F(-1), np.where(r >= F(1), F(1), r)).astype(np.float32)


def np_fcos(x):
    return np_fsin(np.array(x, dtype=np.float32) + F(M_PI_2))


def np_facos(x):
    """fAcos__, util_math_optimizations.h:255-261"""
    x = np.array(x, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        a = np.arccos(np.clip(x.astype(f64), -1.0, 1.0)).astype(np.float32)
    return np.where(x.astype(f64) <= -1.0, F(M_PI), np.where(x.astype(f64) >= 1.0, F(0), a)).astype(np.float32)


def spheremap(p):
    """spheremap__, texture.h:111-128: the double constants make those sums and products double, narrowed once"""
    x, y, z = (np.ascontiguousarray(p[:, k], np.float32) for k in range(3))
    r_phi = x * x + y * y
    r_theta = r_phi + z * z
    with np.errstate(all="ignore"):
        a = np_facos(x / np.sqrt(r_phi)).astype(f64)
        ratio = np.where(y < 0, (M_2PI - a) * M_1_2PI, a * M_1_2PI).astype(np.float32)
        u = np.where(r_phi > 0, F(1) - ratio, F(0)).astype(np.float32)
        v = (1.0 - np_facos(z / np.sqrt(r_theta)).astype(f64) * M_1_PI).astype(np.float32)
    return u, v


def inv_spheremap(u, v):
    """invSpheremap__, texture.h:131-140"""
    theta = (np.asarray(v, np.float32).astype(f64) * M_PI).astype(np.float32)
    phi = (-(np.asarray(u, np.float32).astype(f64) * M_2PI)).astype(np.float32)
    ct, st, cp, sp = np_fcos(theta), np_fsin(theta), np_fcos(phi), np_fsin(phi)
    return np.stack([st * cp, st * sp, -ct], axis=-1).astype(np.float32)


def angmap(p):
    """angmap__, texture.h:83-94"""
    x, y, z = (np.ascontiguousarray(p[:, k], np.float32) for k in range(3))
    r = x * x + z * z
    with np.errstate(all="ignore"):
        ratio = (M_1_PI * np_facos(y).astype(f64)).astype(np.float32)
        q = ratio / np.sqrt(r)
        return np.where(r > 0, x * q, F(0)).astype(np.float32), np.where(r > 0, z * q, F(0)).astype(np.float32)


def bg_uv(bg, dirs):
    """the texture coordinates TextureBackground::eval looks up (background_texture.cc:55-70) and whether u wrapped"""
    dirs = np.ascontiguousarray(dirs, np.float32)
    if bg["projection"] == 1:
        d = dirs.copy()
        d[:, 0] = dirs[:, 0] * bg["cos_r"] + dirs[:, 1] * bg["sin_r"]
        d[:, 1] = dirs[:, 0] * -bg["sin_r"] + dirs[:, 1] * bg["cos_r"]
        u, v = angmap(d)
        return u, v, np.zeros(len(u), bool)
    u, v = spheremap(dirs)
    u = F(2) * u - F(1)
    v = F(2) * v - F(1)
    u = u + bg["rotation"]
    wrapped = u > 1
    return np.where(wrapped, u - F(2), u).astype(np.float32), v, wrapped


def bg_eval(yi, bg, dirs, info=None):
    """Background::eval; the texture's colour comes from the pinned lookup (probe op 13, tests/test_gpu_textures.py)"""
    dirs = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
    if bg["kind"] == 1:
        return np.broadcast_to(bg["color"], dirs.shape).astype(np.float32)
    u, v, wrapped = bg_uv(bg, dirs)
    ti = np.full(len(u), np.uint32(bg["texture"])).view(np.float32)
    c = yi.probe(13, np.stack([u, v, np.zeros_like(u), ti], axis=1), 5)[:, :3]
    floored = c < F(1.0e-5)
    if info is not None:
        info["wrapped"] = wrapped; info["floored"] = floored.any(axis=1)
    return (np.where(floored, F(1.0e-5), c).astype(np.float32) * bg["power"]).astype(np.float32)


def row_counts():
    fy = (np.arange(NV, dtype=np.float32) + F(0.5)) * (F(1) / F(NV))
    sintheta = np_fsin((fy.astype(f64) * M_PI).astype(np.float32))
    return fy, sintheta, MINU + (sintheta * F(MAXU - MINU)).astype(np.int32)


def pdf1d(f):
    """Pdf1D's constructor (util_sample.h:89-122): the running sum in double, in index order; stored as float; divided by the float integral"""
    n = len(f)
    c = np.cumsum(f.astype(f64) * (1.0 / f64(n)))
    integral = np.float32(c[-1])
    row = np.zeros(ROW, np.float32)
    row[0] = n; row[1] = integral; row[2] = F(1) / integral; row[3] = F(1) / F(n)
    row[4:4 + n] = f
    row[4 + MAXU + 1:4 + MAXU + 1 + n] = c.astype(np.float32) / integral
    return row


def tables(yi, bg):
    """BackgroundLight::init (light_background.cc:78-120) in the device's layout: rows 0..359 = u_dist_, row 360 = v_dist_"""
    fy, sintheta, nu = row_counts()
    fx = np.concatenate([(np.arange(n, dtype=np.float32) + F(0.5)) * (F(1) / F(n)) for n in nu])
    yy = np.repeat(np.arange(NV), nu)
    col = bg_eval(yi, bg, inv_spheremap(fx, fy[yy]))
    fu = ((col[:, 0] + col[:, 1] + col[:, 2]) * F(0.333333)) * sintheta[yy]
    tab = np.zeros((NV + 1, ROW), np.float32)
    start = np.concatenate([[0], np.cumsum(nu)])
    for y in range(NV):
        tab[y] = pdf1d(fu[start[y]:start[y + 1]])
    tab[NV] = pdf1d(tab[:NV, 1].copy())
    return tab


def pdf1d_sample(row, u):
    """Pdf1D::sample (util_sample.h:127-141); also returns lower_bound's position"""
    n = int(row[0])
    cdf, func = row[4 + MAXU:4 + MAXU + n + 1], row[4:4 + n]
    pos = np.searchsorted(cdf, u, side="left")
    idx = np.minimum(np.maximum(pos - 1, 0), n - 1)
    delta = (u - cdf[idx]) / (cdf[idx + 1] - cdf[idx])
    return idx.astype(np.float32) + delta, func[idx] * row[2], pos


def clamp_zero(x):
    with np.errstate(divide="ignore"):
        return np.where(x > 0, F(1) / x, F(0)).astype(np.float32)


def sin_sample(s):
    return np_fsin((np.asarray(s, np.float32).astype(f64) * M_PI).astype(np.float32))


def calc_from_sample(tab, s1, s2, info=None):
    """BackgroundLight::calcFromSample, light_background.cc:122-133 (inv = false)"""
    s1, s2 = np.asarray(s1, np.float32), np.asarray(s2, np.float32)
    v, pdf2, pos_v = pdf1d_sample(tab[NV], s2)
    iv = np.clip((v + F(0.4999)).astype(np.int32), 0, NV - 1)
    u = np.zeros_like(v); pdf1 = np.zeros_like(v); pos_u = np.zeros(len(v), np.int64)
    for y in np.unique(iv):
        m = iv == y
        u[m], pdf1[m], pos_u[m] = pdf1d_sample(tab[y], s1[m])
    u = u * tab[iv, 3]
    v = v * tab[NV, 3]
    if info is not None:
        info["pos_u"] = pos_u; info["pos_v"] = pos_v; info["iv"] = iv
    return np.maximum(F(0.000001), ((pdf1 * pdf2) * F(M_1_2PI)) * clamp_zero(sin_sample(v))).astype(np.float32), u, v


def calc_from_dir(tab, dirs):
    """BackgroundLight::calcFromDir, :135-146 (inv = true)"""
    u, v = spheremap(dirs)
    iv = np.clip((v * F(NV) + F(0.4999)).astype(np.int32), 0, NV - 1)
    nu = tab[iv, 0].astype(np.int32)
    iu = np.clip((u * nu.astype(np.float32) + F(0.4999)).astype(np.int32), 0, nu - 1)
    pdf1 = tab[iv, 4 + iu] * tab[iv, 2]
    pdf2 = tab[NV, 4 + iv] * tab[NV, 2]
    return np.maximum(F(0.000001), (F(M_2PI) * sin_sample(v)) * clamp_zero(pdf1 * pdf2)).astype(np.float32), u, v


def illum_sample(yi, bg, tab, s1, s2, info=None):
    """BackgroundLight::illumSample, :162-171 -> direction, pdf, colour"""
    pdf, u, v = calc_from_sample(tab, s1, s2, info)
    d = inv_spheremap(u, v)
    return d, pdf, bg_eval(yi, bg, d)


def clamp_proportional(col, max_value):
    """Rgb::clampProportionalRgb, color.h:412-445; also returns which rows it changed"""
    col = np.array(col, np.float32)
    if not max_value > 0:
        return col, np.zeros(len(col), bool)
    mx = np.maximum(col[:, 0], np.maximum(col[:, 1], col[:, 2]))
    adj = F(max_value) / mx
    hit = mx > F(max_value)
    first = np.where(col[:, 0] >= mx, 0, np.where(col[:, 1] >= mx, 1, 2))
    out = col.copy()
    for k in range(3):
        out[:, k] = np.where(hit, np.where(first == k, F(max_value), col[:, k] * adj), col[:, k])
    return out, hit


def intersect(yi, bg, tab, dirs, clamp):
    """BackgroundLight::intersect, :173-184 -> inverse pdf, colour (evaluated where (u, v) maps back to), clamped rows"""
    ipdf, u, v = calc_from_dir(tab, np.ascontiguousarray(dirs, np.float32))
    col, hit = clamp_proportional(bg_eval(yi, bg, inv_spheremap(u, v)), clamp)
    return ipdf, col, hit


# ---- scenes ----------------------------------------------------------------------------------------------------
def block_texels():
    """a dark environment (zero: the 1e-5 floor of TextureBackground::eval) with one bright block of texels; 36 rows: ten table rows each"""
    t = np.zeros((36, 72, 4), np.float32)
    t[..., 3] = 1
    t[6:9, 20:26, :3] = (2.0e-3, 1.5e-3, 1.0e-3)
    return t


def prepared(bg, textures=(), lights=(), res=8):
    sc = plane_scene(list(lights), res=res)
    sc["textures"] = list(textures)
    yi = Interface()
    scenes.load_scene(yi, sc, scenes.render_settings(res, res, 1, integrator="directlighting", background=bg))
    yi.prepareRender()
    return yi


SKY = dict(name="sky", filename=HDR)


@pytest.fixture(scope="module")
def cases():
    """the scenes tests 1, 2 and 8 share: name -> (interface, background record, restated tables, clamp_intersect)"""
    out = {}

    def add(name, bg, textures=(), clamp=0.0):
        yi = prepared(bg, textures)
        rec = yi.getBackground("world_background")
        out[name] = (yi, rec, tables(yi, rec), clamp)

    add("constant", {"type": "constant", "color": (0.3, 0.9, 0.6), "power": 1.7, "ibl": True})
    add("spherical", {"type": "textureback", "texture": "sky", "rotation": 37.0, "power": 1.3, "ibl": True, "ibl_samples": 4}, [SKY])
    # a clamp between the environment's dark and bright parts (four fifths of the image are black, the rest is near 1): half of its
    # largest component, times the power
    img = out["spherical"][0].getTextureImage("sky")
    clamp = 0.5 * float(img[..., :3].max()) * 0.8
    assert clamp > 0
    add("angular", {"type": "textureback", "texture": "sky", "mapping": "angular", "rotation": 37.0, "power": 0.8, "ibl": True,
                    "ibl_clamp_sampling": clamp}, [SKY], clamp)
    add("block", {"type": "textureback", "texture": "env", "ibl": True}, [dict(name="env", texels=block_texels(), interpolate="none")])
    return out


def test_restatements_agree():
    """the vectorised fSin__ / fCos__ above against the oracle library's (which tests/test_oracle_golden.py holds to the reference)"""
    x = np.concatenate([np.random.default_rng(3).uniform(-20, 20, 4000), [0.0, M_PI, -M_PI, M_2PI, 7.0, -7.0, 1e-30]]).astype(np.float32)
    assert np.array_equal(np_fsin(x).view(np.uint32), fsin(x).view(np.uint32))
    assert np.array_equal(np_fcos(x).view(np.uint32), fcos(x).view(np.uint32))
    assert np.array_equal(np.sqrt(np.abs(x)).view(np.uint32), fsqrt(np.abs(x)).view(np.uint32))


# ---- 1. the tables, bit for bit ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["constant", "spherical", "angular"])
def test_tables_bit_for_bit(cases, name):
    yi, bg, tab, _ = cases[name]
    got = yi.probe(25, np.arange(NV + 1, dtype=np.uint32).view(np.float32).reshape(-1, 1), ROW)
    _, sintheta, nu = row_counts()
    assert np.array_equal(got[:NV, 0].astype(np.int32), nu) and MINU <= nu.min() < 2 * MINU and MAXU - 2 <= nu.max() <= MAXU and got[NV, 0] == NV
    assert np.array_equal(nu, [MINU + int(s * F(MAXU - MINU)) for s in sintheta])
    assert (tab[:, 1] > 0).all() and np.isfinite(tab).all()
    exact(got[:, :4], tab[:, :4].view(np.uint32), f"{name}: row headers")
    exact(got[:, 4:4 + MAXU], tab[:, 4:4 + MAXU].view(np.uint32), f"{name}: func_")
    exact(got[:, 4 + MAXU:], tab[:, 4 + MAXU:].view(np.uint32), f"{name}: cdf_")
    assert (tab[np.arange(NV), 4 + MAXU + nu] == 1).all()          # cdf_[n] = integral / integral


# ---- 2. the leaf functions, bit for bit -----------------------------------------------------------------------------------
def unit_dirs(rng, n):
    d = rng.normal(0, 1, (n, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    # the poles of spheremap__ (x = y = 0), of angmap__ (x = z = 0), and a zero in each component
    d[:8] = [(0, 0, 1), (0, 0, -1), (0, 1, 0), (0, -1, 0), (1, 0, 0), (-1, 0, 0), (0, 0.6, 0.8), (0.6, 0, -0.8)]
    return d


@pytest.mark.parametrize("name", ["constant", "spherical", "angular", "block"])
def test_leaf_functions_bit_for_bit(cases, name):
    yi, bg, tab, clamp = cases[name]
    rng = np.random.default_rng(11)
    N = 10000
    # Background::eval
    dirs = unit_dirs(rng, N)
    info = {}
    want = bg_eval(yi, bg, dirs, info)
    exact(yi.probe(22, dirs, 3), want.view(np.uint32), f"{name}: bg_eval")
    if name == "spherical":
        assert 0.05 < info["wrapped"].mean() < 0.95           # rotation 37 degrees: u + 0.2056 wraps for a tenth of the directions
    if name == "block":
        assert 0.1 < info["floored"].mean() < 1.0 and not info["floored"].all()
    # BackgroundLight::illumSample: random samples, s = 0 (lower_bound at 0: the index clamp), s equal to a cdf entry
    s = rng.random((N, 2)).astype(np.float32)
    s[:40, 0] = 0; s[20:60, 1] = 0
    nv_cdf = tab[NV, 4 + MAXU:4 + MAXU + NV + 1]
    s[100:300, 1] = nv_cdf[rng.integers(1, NV + 1, 200)]
    _, _, pos_v = pdf1d_sample(tab[NV], s[:, 1])
    v0, _, _ = pdf1d_sample(tab[NV], s[:, 1])
    iv0 = np.clip((v0 + F(0.4999)).astype(np.int32), 0, NV - 1)
    for k in range(300, 500):                                # s_1 on a cdf entry of the row s_2 picks
        n = int(tab[iv0[k], 0])
        s[k, 0] = tab[iv0[k], 4 + MAXU + rng.integers(1, n + 1)]
    info = {}
    d, pdf, col = illum_sample(yi, bg, tab, s[:, 0], s[:, 1], info)
    assert (info["pos_u"] == 0).sum() >= 40 and (info["pos_v"] == 0).sum() >= 40 and (info["pos_u"] > 0).sum() > N // 2
    on_u = tab[info["iv"], 4 + MAXU + np.minimum(info["pos_u"], MAXU)] == s[:, 0]
    on_v = tab[NV, 4 + MAXU + np.minimum(info["pos_v"], NV)] == s[:, 1]
    assert on_u.sum() >= 200 and on_v.sum() >= 200 and (~on_u).sum() > N // 2 and (~on_v).sum() > N // 2
    want = np.zeros((N, 9), np.float32)
    want[:, 0] = 1; want[:, 1:4] = d; want[:, 4] = -1; want[:, 5] = pdf; want[:, 6:9] = col
    assert np.isfinite(want).all()
    exact(yi.probe(23, s, 9), want.view(np.uint32), f"{name}: illumSample")
    # BackgroundLight::intersect
    ipdf, col, hit = intersect(yi, bg, tab, dirs, clamp)
    if name == "angular":
        assert clamp > 0 and 0.1 < hit.mean() < 0.9
    else:
        assert clamp == 0 and not hit.any()
    want = np.zeros((N, 6), np.float32)
    want[:, 0] = 1; want[:, 1] = -1; want[:, 2] = ipdf; want[:, 3:6] = col
    assert np.isfinite(want).all()
    exact(yi.probe(24, dirs, 6), want.view(np.uint32), f"{name}: intersect")
    assert not (ipdf == F(0.000001)).all()                   # (the floor of CALC_INV_PDF is not all there is)


# ---- 3. escaping rays --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mapping, rotation", [("sphere", 0.0), ("sphere", 143.0), ("angular", 0.0), ("angular", 143.0)])
def test_escaping_rays_pick_up_the_background_of_their_direction(mapping, rotation):
    res = 24
    tri = np.array([[(-1, -1, -50), (1, -1, -50), (0, 1, -50)]], np.float32)           # far behind the camera
    sc = {"verts": tri, "tri_mat": np.array([0], np.int32), "vnormals": None, "materials": [{"type": "shinydiffusemat", "color": RHO}],
          "lights": [], "textures": [SKY],
          "camera": {"type": "perspective", "from": (0.0, 0.0, 0.0), "to": (0.3, 1.0, 0.5), "up": (0.3, 1.0, 1.5), "resx": res, "resy": res, "focal": 0.6}}
    bgp = {"type": "textureback", "texture": "sky", "mapping": mapping, "rotation": rotation, "power": 1.25}
    for integrator in ("directlighting", "pathtracing"):
        yi = Interface()
        scenes.load_scene(yi, sc, scenes.render_settings(res, res, 1, integrator=integrator, background=bgp))
        yi.render()
        film = yi.getFilm(res, res)
        assert (film[..., 4] == 1).all() and yi.getRenderStats().rays_shadow == 0
        px = np.stack(np.meshgrid(np.arange(res) + 0.5, np.arange(res) + 0.5), axis=-1).reshape(-1, 2).astype(np.float32)
        dirs = yi.probe(7, px, 9)[:, 3:6]
        bg = yi.getBackground("world_background")
        want = bg_eval(yi, bg, dirs)
        exact(yi.probe(22, dirs, 3), want.view(np.uint32), "bg_eval of the camera rays")
        exact(film[..., :3].reshape(-1, 3), want.view(np.uint32), f"{integrator}: the film of an empty view")
        assert len(np.unique(want[:, 0])) > res                     # (the view is not one colour)


# ---- 4. the texture path is the constant path ------------------------------------------------------------------------------
OPAQUE = {"type": "shinydiffusemat", "color": (0.5, 0.5, 0.5)}


def render_bg(sc, bg, spp=1, integrator="directlighting", res=48, **kw):
    rd = scenes.render_settings(res, res, spp, integrator=integrator, background=bg, **kw)
    yi = Interface()
    scenes.load_scene(yi, sc, rd)
    yi.render()
    return yi.getFilm(res, res).copy(), yi


def low_occluder():
    """a quad over the plane, out of the camera's sight lines' way only in part: it shadows and is seen"""
    return scenes._quad((1.0, -2.0, 1.5), (4.0, -2.0, 1.5), (4.0, 2.0, 1.5), (1.0, 2.0, 1.5))


@pytest.mark.parametrize("integrator, kw", [("directlighting", {}), ("pathtracing", {"bounces": 3})])
def test_texture_path_equals_constant_path(integrator, kw):
    col, power = (0.5, 0.25, 0.75), 1.5
    texels = np.zeros((5, 7, 4), np.float32)
    texels[..., :3] = col; texels[..., 3] = 1
    sc = plane_scene([], extra=[(low_occluder(), OPAQUE)], res=48)
    sc["textures"] = [dict(name="flat", texels=texels, interpolate="none")]
    a, ya = render_bg(sc, {"type": "textureback", "texture": "flat", "power": power, "ibl": True, "ibl_samples": 3}, spp=2, integrator=integrator, **kw)
    b, yb = render_bg(sc, {"type": "constant", "color": col, "power": power, "ibl": True, "ibl_samples": 3}, spp=2, integrator=integrator, **kw)
    sa, sb = ya.getRenderStats(), yb.getRenderStats()
    assert (sa.rays_closest, sa.rays_shadow, sa.camera_samples) == (sb.rays_closest, sb.rays_shadow, sb.camera_samples)
    assert a[..., :3].sum() > 0 and len(np.unique(a[..., 0])) > 100
    assert np.array_equal(a, b)


# ---- 5. ray counts -------------------------------------------------------------------------------------------------------
def test_ray_counts_and_cast_shadows():
    n = 3
    bg = {"type": "constant", "color": (1.0, 0.9, 0.8), "ibl": True, "ibl_samples": n}
    sc = plane_scene([], extra=[(occluder(), OPAQUE)], res=64)
    _, yi = render_bg(sc, bg, spp=2, res=64)
    st = yi.getRenderStats()
    # illumSample and intersect never fail: both halves of every pair send a ray (the BSDF half unless its sample's pdf is below 1e-6)
    assert st.camera_samples == 64 * 64 * 2
    assert 0.999 * 2 * n * st.camera_samples < st.rays_shadow <= 2 * n * st.camera_samples
    off = dict(bg, cast_shadows=False)
    a, ya = render_bg(sc, off, spp=2, res=64)
    b, yb = render_bg(plane_scene([], res=64), off, spp=2, res=64)
    assert ya.getRenderStats().rays_shadow == 0 and yb.getRenderStats().rays_shadow == 0
    assert a[..., :3].sum() > 0 and np.array_equal(a, b)


# ---- 6. occlusion -----------------------------------------------------------------------------------------------------------
def box_walls(h=8.0, r=10.0, m=1.0):
    """four walls around the plane, oversized so that they overlap at the corners and reach below the plane and above the lid"""
    q = scenes._quad
    return np.concatenate([q((-r, -r - m, -m), (-r, r + m, -m), (-r, r + m, h + m), (-r, -r - m, h + m)),
                           q((r, -r - m, -m), (r, r + m, -m), (r, r + m, h + m), (r, -r - m, h + m)),
                           q((-r - m, -r, -m), (r + m, -r, -m), (r + m, -r, h + m), (-r - m, -r, h + m)),
                           q((-r - m, r, -m), (r + m, r, -m), (r + m, r, h + m), (-r - m, r, h + m))])


def lid(h=8.0):
    """ONE triangle over the whole box (a quad's diagonal would filter a transparent-shadow ray through it twice)"""
    return np.array([[(-60.0, -40.0, h), (60.0, -40.0, h), (0.0, 80.0, h)]], np.float32)


def test_occlusion_and_transparent_shadows():
    bg = {"type": "constant", "color": (1.0, 0.9, 0.8), "power": 2.0, "ibl": True, "ibl_samples": 4}
    closed = plane_scene([], extra=[(box_walls(), OPAQUE), (lid(), OPAQUE)], res=32)
    film, yi = render_bg(closed, bg, spp=2, res=32)
    assert yi.getRenderStats().rays_shadow > 0 and (film[..., :3] == 0).all(), "inside a closed box the direct term is exactly zero"
    filt = (0.3, 0.6, 0.9)
    sheet = {"type": "shinydiffusemat", "color": filt, "transparency": 1.0, "transmit_filter": 1.0}
    opened = plane_scene([], extra=[(box_walls(), OPAQUE)], res=32)
    lidded = plane_scene([], extra=[(box_walls(), OPAQUE), (lid(), sheet)], res=32)
    a, _ = render_bg(opened, bg, spp=2, res=32, transpShad=True, shadowDepth=4)
    b, _ = render_bg(lidded, bg, spp=2, res=32, transpShad=True, shadowDepth=4)
    a, b = po.film_to_rgb(a)[..., :3].astype(f64), po.film_to_rgb(b)[..., :3].astype(f64)
    assert (a > 0).all()
    # ShinyDiffuseMaterial::getTransparency: transmit_filter * colour + (1 - transmit_filter), transparency 1 (material_shiny_diffuse.cc:541-563)
    np.testing.assert_allclose(b, a * np.array(filt), rtol=1e-5)


# ---- 7. the estimator's mean -------------------------------------------------------------------------------------------------
def estimate_moments(yi, bg, tab, mat, wo, G, n=(0.0, 0.0, 1.0)):
    """First and second moment, per channel, of ONE term of doLightEstimation's sampled branch for the background light at a surface
    point with normal n seen from wo: the light half (integrator_montecarlo.cc:161-262) plus the BSDF half (:273-333) of the pair that
    shares (s_1, s_2), integrated by G x G midpoint quadrature over the sample square with the material's eval / pdf / sample from the
    oracle (yor_material_probe) and the light's restated calcFromSample / calcFromDir.  Also the BSDF half's mean alone."""
    L = po.lib()
    md = po.material_desc(mat)
    g = ((np.arange(G) + 0.5) / G).astype(np.float32)
    s1, s2 = [a.ravel() for a in np.meshgrid(g, g)]
    N = s1.size
    wi, pdf_l, lcol = illum_sample(yi, bg, tab, s1, s2)
    n = np.array(n, np.float32)
    inp = np.zeros(14, np.float32); e = np.zeros(3, np.float32); s8 = np.zeros(8, np.float32)
    bf, pdf, so = C.c_int32(), C.c_float(), C.c_int32()
    ev = np.zeros((N, 3)); mp = np.zeros(N); smp = np.zeros((N, 8))
    for i in range(N):
        inp[:] = [*n, *n, *wo, *wi[i], s1[i], s2[i]]
        L.yor_material_probe(C.byref(md), po.fptr(inp), K_MIS_FLAGS, C.byref(bf), po.fptr(e), C.byref(pdf), C.byref(so), po.fptr(s8))
        ev[i] = e; mp[i] = pdf.value; smp[i] = s8
    pl = pdf_l.astype(f64)
    w = np.where(mp > 1e-6, pl * pl / (pl * pl + mp * mp), 1.0)
    light = np.where((pl > 1e-6)[:, None], ev * lcol.astype(f64) * np.abs(wi.astype(f64) @ n.astype(f64))[:, None] * (w / pl)[:, None], 0.0)
    with np.errstate(all="ignore"):                          # (a sample that took no lobe leaves a zero direction: masked below)
        ipdf, icol, _ = intersect(yi, bg, tab, smp[:, 3:6].astype(np.float32), 0.0)
    spdf, W = smp[:, 6], smp[:, 7]
    lp = 1.0 / ipdf.astype(f64)
    wb = spdf * spdf / (lp * lp + spdf * spdf)
    bsdf = np.where(((spdf > 1e-6) & (ipdf > 1e-6))[:, None], smp[:, :3] * icol.astype(f64) * (wb * W)[:, None], 0.0)
    x = light + bsdf
    return x.mean(axis=0), (x * x).mean(axis=0), bsdf.mean(axis=0)


def check_mean(img, yi, mat, wos, n_samples, spp, G, what):
    bg = yi.getBackground("world_background")
    tab = tables(yi, bg)
    m1, m2, b1, m1_2g = [], [], [], []
    for wo in wos:
        a, b, c = estimate_moments(yi, bg, tab, mat, wo, G)
        m1.append(a); m2.append(b); b1.append(c)
        m1_2g.append(estimate_moments(yi, bg, tab, mat, wo, 2 * G)[0])
    m1, m2, b1, m1_2g = (np.mean(v, axis=0) for v in (m1, m2, b1, m1_2g))
    n_terms = img.shape[0] * img.shape[1] * spp * n_samples
    # six standard errors of the frame mean (the second moment over pixels x spp x light samples) plus what the quadrature itself is
    # unsure of (G against 2 G): neither depends on the device
    tol = 6.0 * np.sqrt(np.maximum(m2 - m1 * m1, 0.0) / n_terms) + np.abs(m1_2g - m1)
    got = img.reshape(-1, 3).mean(axis=0)
    print(f"{what}: frame mean {got}, expectation (2G) {m1_2g}, deviation {np.abs(got - m1_2g)}, tolerance {tol}, BSDF share {b1 / m1}")
    assert (np.abs(got - m1_2g) <= tol).all(), (what, got, m1_2g, tol)
    return b1 / m1


def test_estimator_mean_on_a_diffuse_plane():
    """Constant IBL over the diffuse plane: the lobe's eval, pdf and sample do not depend on wo, so every pixel has one expectation.
    The deviation the run observes is printed next to the tolerance (no figure recorded yet: DESIGN.md §8)."""
    n, spp, res = 4, 16, 64
    mat = {"type": "shinydiffusemat", "color": RHO, "diffuse_reflect": 1.0}
    bgp = {"type": "constant", "color": (0.9, 1.0, 1.1), "power": 1.5, "ibl": True, "ibl_samples": n}
    img, yi = render(dict(plane_scene([], res=res), textures=[]), spp=spp, res=res, background=bgp)
    check_mean(img, yi, mat, [(0.0, 0.0, 1.0)], n, spp, 64, "diffuse plane")


def test_estimator_mean_on_a_glossy_plane_pins_the_bsdf_half():
    """The exponent-200 Blinn lobe of test_sun_on_a_glossy_plane_pins_the_bsdf_half under a constant environment: the BSDF half carries a
    large share, so intersect's colour, its inverse pdf and the weight m^2 / (l^2 + m^2) show in the frame mean.  The camera is far away
    (wo within 0.7 degrees of the normal); the expectation is taken at a 2 x 2 grid of pixel centres and averaged."""
    n, spp, res = 4, 16, 64
    glossy = {"type": "glossy", "color": (0.9, 0.8, 0.7), "diffuse_reflect": 0.0, "glossy_reflect": 1.0, "exponent": 200.0, "as_diffuse": True}
    bgp = {"type": "constant", "color": (0.9, 1.0, 1.1), "power": 1.5, "ibl": True, "ibl_samples": n}
    sc = plane_scene([], res=res, plane_mat=glossy)
    sc["camera"] = dict(sc["camera"], **{"from": (0.0, 0.0, 200.0), "up": (0.0, 1.0, 200.0), "focal": 40.0})
    img, yi = render(sc, spp=spp, res=res, background=bgp)
    pts = plane_points(yi, res)[16::32, 16::32].reshape(-1, 3)
    wos = [((np.array([0.0, 0.0, 200.0]) - p) / np.linalg.norm(np.array([0.0, 0.0, 200.0]) - p)).astype(np.float32) for p in pts]
    share = check_mean(img, yi, glossy, wos, n, spp, 64, "glossy plane")
    assert (share > 0.2).all(), "the BSDF half should carry a large share here"


# ---- 8. importance -------------------------------------------------------------------------------------------------------------
def test_samples_follow_the_environment(cases):
    yi, bg, tab, _ = cases["block"]
    got = yi.probe(25, np.arange(NV + 1, dtype=np.uint32).view(np.float32).reshape(-1, 1), ROW)      # the device's own tables
    nu = got[:NV, 0].astype(np.int64)
    _, sintheta, _ = row_counts()
    func = got[:NV, 4:4 + MAXU].astype(f64)
    bright = func > 10 * (1.0e-5 * sintheta.astype(f64))[:, None]          # cells whose centre saw the block (dark cells hold the floor)
    assert 50 < bright.sum() < 0.05 * nu.sum()
    share = ((func * bright).sum(axis=1) / nu).sum() / NV / f64(got[NV, 1])
    assert 0.2 < share < 0.8, share
    K = 100
    rng = np.random.default_rng(5)
    gx, gy = np.meshgrid(np.arange(K), np.arange(K))
    s = ((np.stack([gx.ravel(), gy.ravel()], axis=1) + rng.random((K * K, 2))) / K).astype(np.float32)
    o = yi.probe(23, s, 9)
    u, v = spheremap(o[:, 1:4])
    iv = np.clip(np.floor(v.astype(f64) * NV).astype(np.int64), 0, NV - 1)
    iu = np.clip(np.floor(u.astype(f64) * nu[iv]).astype(np.int64), 0, nu[iv] - 1)
    landed = bright[iv, iu].mean()
    se = np.sqrt(share * (1 - share) / (K * K))
    assert abs(landed - share) <= 3 * se, (landed, share, se)


# ---- 9. caustic paths that escape -----------------------------------------------------------------------------------------------
def test_escaping_caustic_paths_pick_up_an_ibl_background():
    glass = {"type": "glass", "IOR": 1.5, "filter_color": (1.0, 1.0, 1.0), "transmit_filter": 0.0, "mirror_color": (1.0, 1.0, 1.0)}
    sheet = scenes._quad((-12.0, -12.0, 1.0), (12.0, -12.0, 1.0), (12.0, 12.0, 1.0), (-12.0, 12.0, 1.0))
    sc = plane_scene([], extra=[(sheet, glass)], res=32)
    sc["textures"] = [SKY]
    kw = dict(spp=2, integrator="pathtracing", res=32, bounces=4, caustic_type="path")
    films = {}
    for kind, p in (("texture", {"type": "textureback", "texture": "sky", "power": 2.0}), ("constant", {"type": "constant", "color": (0.5, 0.6, 0.7)})):
        for wc in (True, False):
            films[kind, wc], _ = render_bg(sc, dict(p, ibl=True, ibl_samples=2, with_caustic=wc), **kw)
    assert np.isfinite(films["texture", True]).all()
    d = films["texture", True][..., :3].astype(f64) - films["texture", False][..., :3].astype(f64)
    assert (d >= 0).all() and (d > 0).mean() > 0.5, "with_caustic on a texture background adds the escaped caustic paths"
    assert np.array_equal(films["constant", True], films["constant", False]), "a constant background always shoots caustics"
    none, _ = render_bg(sc, {"type": "textureback", "texture": "sky", "power": 2.0, "ibl": True, "ibl_samples": 2}, **dict(kw, caustic_type="none"))
    assert np.array_equal(none, films["texture", False])


# ---- 10. serial state --------------------------------------------------------------------------------------------------------------
def test_replay_shards_and_pipelining_with_the_background_light():
    import torch
    from libyafaray_amd.parallel import _DeviceFloats
    W = H = 96; T = 32; WORLD = 2
    sc = scenes.cornell_soup(1500, seed=41, res=(W, H))
    sc["lights"] = sc["lights"] + [{"type": "pointlight", "from": (0.3, -0.5, 0.2), "color": (1.0, 0.9, 0.8), "power": 1.5}]
    sc["camera"] = dict(sc["camera"], resx=W, resy=H)
    sc["textures"] = [SKY]
    bgp = {"type": "textureback", "texture": "sky", "rotation": 20.0, "ibl": True, "ibl_samples": 2}
    rd = scenes.render_settings(W, H, 4, bounces=4, tile_size=T, russian_roulette_min_bounces=1, background=bgp)
    yi = Interface()
    scenes.load_scene(yi, sc, rd)
    assert [int(t) for t in yi.getLights()[:, 0].view(np.int32)] == [0, 1, 5]
    yi.setSerialReplay(True)
    yi.render()
    full, st_full = yi.getFilm(W, H).copy(), yi.getRenderStats()
    assert np.isfinite(full).all() and full[..., :3].sum() > 0
    contrib = {}
    state = {"rank": 0, "k": 0, "phase": 0}

    def exchange(ptr, n):
        t = torch.as_tensor(_DeviceFloats(ptr, n), device=torch.device("cuda", 0))
        key = state["k"]; state["k"] += 1
        if state["phase"] == 0:
            contrib[(state["rank"], key)] = t.clone()
        else:
            t.copy_(sum(contrib[(r, key)] for r in range(WORLD)))
        torch.cuda.synchronize()

    yi.setPlaneExchange(exchange)
    parts = []
    for phase in (0, 1):
        state["phase"] = phase
        for r in range(WORLD):
            state["rank"], state["k"] = r, 0
            yi.setShard(r, WORLD)
            yi.render()
            if phase == 1:
                parts.append((yi.getFilm(W, H).copy(), yi.getRenderStats()))
    assert contrib, "the light-counter exchange never ran"
    assert (sum(p[1].rays_closest for p in parts), sum(p[1].rays_shadow for p in parts)) == (st_full.rays_closest, st_full.rays_shadow)
    total = sum(p[0] for p in parts)
    interior = np.ones((H, W), bool)
    interior[::T, :] = False; interior[:, ::T] = False
    assert np.array_equal(total[..., 4], full[..., 4])
    assert np.array_equal(total[interior], full[interior]), "two shards do not sum to the single-GPU film"
    np.testing.assert_allclose(total, full, rtol=2.5e-7, atol=1e-7)
    films = []
    for mode in (0, 1):
        y2 = Interface()
        scenes.load_scene(y2, sc, dict(rd, AA_passes=3, AA_inc_samples=2, AA_threshold=0.0))
        y2.setSerialReplay(False)
        y2.setPassPipelining(mode)
        y2.render()
        films.append(y2.getFilm(W, H).copy())
    assert np.array_equal(films[0], films[1])
