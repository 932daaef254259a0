"""The directional, sun and sphere lights on the DEVICE: their leaf functions bit for bit against the reference's own light sources
(tests/golden/ref_lights_ieee, probe ops 17-20) and against a float32 restatement in the reference's operation order (probe ops 17-21:
the static sphereIntersect__ has no fixture), a scene with all five light types against the oracle, renders against closed forms (a diffuse plane under each light,
infinite and finite directional shadows, transparent shadows on infinite rays, the sun's cone, the sphere's cap), the light-sampling
half only for the sphere (no BSDF-half rays), the serial-state replay with sharding and pass pipelining."""
import ctypes as C

import numpy as np
import pytest

from libyafaray_amd import Interface, scenes
from oracle import pyoracle as po
from tests import lights_fixture
from tests.test_gpu_components import exact
from tests.test_lights_host import (F, W_COLOR, W_COLPDF, W_COS, W_DIR, W_DU, W_DV, W_INVPDF, W_PDF, W_POS, W_RAD, W_RAD2, W_RAD2EPS,
                                    create_cs, cross, dot, fsqrt, sample_cone, sphere_consts, sphere_intersect, sun_consts)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def torch_first():
    """the emulated shard exchange hands device memory to torch: let torch open the GPU before the library does"""
    import torch
    torch.cuda.init()


RHO = (0.8, 0.6, 0.4)
COS30 = float(np.cos(np.radians(30.0)))
DIR30 = (0.5, 0.0, COS30)                # 30 degrees from the plane's normal +z
RES = 100


def plane_scene(lights, extra=(), res=RES, plane_mat=None):
    """a 20 x 20 plane at z = 0 facing +z, seen from straight above: every pixel is on it"""
    quad = scenes._quad((-10, -10, 0), (10, -10, 0), (10, 10, 0), (-10, 10, 0))
    verts = [quad]; mats = [0, 0]
    materials = [plane_mat or {"type": "shinydiffusemat", "color": RHO, "diffuse_reflect": 1.0}]
    for (v, m) in extra:
        verts.append(v); mats += [len(materials)] * len(v); materials.append(m)
    cam = {"type": "perspective", "from": (0.0, 0.0, 5.0), "to": (0.0, 0.0, 0.0), "up": (0.0, 1.0, 5.0), "resx": res, "resy": res, "focal": 1.0}
    return {"verts": np.concatenate(verts).astype(np.float32), "tri_mat": np.array(mats, np.int32), "vnormals": None,
            "materials": materials, "lights": list(lights), "camera": cam}


def render(sc, spp=1, integrator="directlighting", res=RES, **kw):
    rd = scenes.render_settings(res, res, spp, integrator=integrator, **kw)
    yi = Interface()
    scenes.load_scene(yi, sc, rd)
    yi.render()
    return po.film_to_rgb(yi.getFilm(res, res))[..., :3].astype(np.float64), yi


def sun(**kw):
    return dict({"type": "sunlight", "direction": DIR30, "color": (1.0, 1.0, 1.0), "power": 2.0, "samples": 4}, **kw)


def directional(**kw):
    return dict({"type": "directionallight", "direction": DIR30, "color": (1.0, 1.0, 1.0), "power": 2.0}, **kw)


def lambert_value(power=2.0, cos=COS30):
    """ShinyDiffuseMaterial::eval with only the diffuse lobe (material_shiny_diffuse.cc:275-287): diffuse colour * diffuse strength, no
    1 / pi (the reference keeps pi in its lights: the area light's colour is col * power * pi), times the light colour and |n . wi|
    (doLightEstimation's Dirac branch, integrator_montecarlo.cc:121-145)"""
    return np.array(RHO) * power * cos


def plane_points(yi, res=RES):
    """where each pixel centre's camera ray meets the plane (probe op 7: PerspectiveCamera::shootRay)"""
    px = np.stack(np.meshgrid(np.arange(res) + 0.5, np.arange(res) + 0.5), axis=-1).reshape(-1, 2).astype(np.float32)
    o = yi.probe(7, px, 9)
    t = -o[:, 2] / o[:, 5]
    return (o[:, :3] + o[:, 3:6] * t[:, None]).reshape(res, res, 3)


def stable(mask):
    """pixels whose 3x3 neighbourhood has one value of the mask (the one-pixel band at an edge is left out)"""
    m = np.pad(mask, 1, mode="edge")
    win = np.stack([m[1 + dy:1 + dy + mask.shape[0], 1 + dx:1 + dx + mask.shape[1]] for dy in (-1, 0, 1) for dx in (-1, 0, 1)])
    return win.all(axis=0) | (~win).all(axis=0)


# ---- 1. leaf functions, bit for bit --------------------------------------------------------------------------------
def test_leaf_functions_bit_for_bit():
    lights = [directional(direction=(0.3, -0.4, 1.2), color=(0.9, 0.5, 0.3)),
              directional(direction=(-0.2, 0.5, 1.0), infinite=False, **{"from": (0.5, -0.5, 4.0)}, radius=2.5),
              sun(direction=(0.6, 0.2, 0.9), angle=12.0, color=(1.0, 0.8, 0.6)),
              {"type": "spherelight", "from": (0.3, -0.2, 1.5), "radius": 0.4, "color": (0.7, 0.8, 0.9), "power": 5.0, "samples": 2}]
    sc = plane_scene(lights, res=8)
    yi = Interface()
    scenes.load_scene(yi, sc, scenes.render_settings(8, 8, 1, integrator="directlighting"))
    yi.prepareRender()
    rec = yi.getLights()
    rng = np.random.default_rng(7)
    N = 10000
    k_bits = lambda k: np.full((N, 1), np.uint32(k)).view(np.float32)

    # DirectionalLight::illuminate, infinite (light 0) and finite (light 1)
    p = rng.uniform(-5, 5, (N, 3)).astype(np.float32)
    for k in (0, 1):
        L = rec[k]
        o = yi.probe(17, np.hstack([p, k_bits(k)]), 8)
        d = L[W_DIR:W_DIR + 3]
        if k == 0:
            ok = np.ones(N, bool); tmax = np.full(N, -1, np.float32)
        else:
            vec = L[W_POS:W_POS + 3] - p
            dist = fsqrt(dot(cross(np.broadcast_to(d, vec.shape), vec), cross(np.broadcast_to(d, vec.shape), vec)))
            tmax = dot(vec, np.broadcast_to(d, vec.shape))
            ok = ~(dist > L[W_RAD]) & ~(tmax <= 0)
            assert 0.1 < ok.mean() < 0.9
        want = np.zeros((N, 8), np.float32)
        want[:, 0] = ok
        want[ok, 1:4] = d; want[ok, 4] = tmax[ok]; want[ok, 5:8] = L[W_COLOR:W_COLOR + 3]
        exact(o, want.view(np.uint32), f"directional illuminate, light {k}")

    # SunLight::illumSample and ::intersect (light 2)
    L = rec[2]
    d, du, dv = (np.broadcast_to(L[w:w + 3], (N, 3)) for w in (W_DIR, W_DU, W_DV))
    s = rng.random((N, 2)).astype(np.float32)
    o = yi.probe(18, np.hstack([s, k_bits(2)]), 9)
    want = np.zeros((N, 9), np.float32)
    want[:, 0] = 1; want[:, 1:4] = sample_cone(d, du, dv, np.full(N, L[W_COS], np.float32), s[:, 0], s[:, 1])
    want[:, 4] = -1; want[:, 5] = L[W_PDF]; want[:, 6:9] = L[W_COLPDF:W_COLPDF + 3]
    exact(o, want.view(np.uint32), "sun illumSample")
    dirs = (d + rng.normal(0, 0.2, (N, 3))).astype(np.float32)
    dirs = (dirs / np.linalg.norm(dirs, axis=1, keepdims=True)).astype(np.float32)
    o = yi.probe(19, np.hstack([dirs, k_bits(2)]), 6)
    ok = ~(dot(dirs, d) < L[W_COS])
    assert 0.1 < ok.mean() < 0.9
    want = np.zeros((N, 6), np.float32)
    want[:, 0] = ok; want[ok, 1] = -1; want[ok, 2] = L[W_INVPDF]; want[ok, 3:6] = L[W_COLPDF:W_COLPDF + 3]
    exact(o, want.view(np.uint32), "sun intersect")

    # SphereLight::illumSample with sphereIntersect__ (light 3); a few points inside the sphere
    L = rec[3]
    c = L[W_POS:W_POS + 3]
    p = rng.uniform(-3, 3, (N, 3)).astype(np.float32)
    p[:200] = (c + rng.uniform(-0.2, 0.2, (200, 3))).astype(np.float32)
    o = yi.probe(20, np.hstack([p, s, k_bits(3)]), 9)
    cdir = c - p
    dist_sqr = dot(cdir, cdir)
    outside = ~(dist_sqr <= L[W_RAD2])
    with np.errstate(all="ignore"):
        dist = fsqrt(dist_sqr)
        cos_alpha = fsqrt(F(1) - L[W_RAD2] * (F(1) / dist_sqr))
        cdir = cdir * (F(1) / dist)[:, None]
        cu, cv = create_cs(cdir)
        wdir = sample_cone(cdir, cu, cv, cos_alpha, s[:, 0], s[:, 1])
        hit, d1, _ = sphere_intersect(p, wdir, c, L[W_RAD2EPS])
        pdf = F(1) / (F(2) * (F(1) - cos_alpha))
    ok = outside & hit
    assert ok.sum() > N - 400
    want = np.zeros((N, 9), np.float32)
    want[:, 0] = ok; want[ok, 1:4] = wdir[ok]; want[ok, 4] = d1[ok]; want[ok, 5] = pdf[ok]; want[ok, 6:9] = L[W_COLOR:W_COLOR + 3]
    exact(o, want.view(np.uint32), "sphere illumSample")
    # sphereIntersect__ alone, hits, misses and the tangential branch (d_1 = fSqrt__(ec / ea))
    dirs = rng.normal(0, 1, (N, 3)).astype(np.float32)
    o = yi.probe(21, np.hstack([p, dirs, k_bits(3)]), 3)
    with np.errstate(all="ignore"):
        hit, d1, d2 = sphere_intersect(p, dirs, c, L[W_RAD2])
    assert 0.02 < hit.mean() < 0.98
    want = np.stack([hit.astype(np.float32), d1, np.where(hit, d2, F(0))], axis=1).astype(np.float32)
    exact(o, want.view(np.uint32), "sphereIntersect__")


@pytest.fixture(scope="module")
def gold():
    return lights_fixture.load("ieee")


def test_leaf_functions_match_the_reference(gold):
    """Probe ops 17-20 on the inputs of tests/golden/ref_lights_ieee (the reference's own light sources, every light made by its factory):
    each parameter set goes through the C ABI as a light of one scene, the outputs are compared bit for bit.  The getLights() records
    hold what the constructors compute: checked against the fixture's outputs where those carry the value (direction, colour, pdf,
    inverse pdf, colour times pdf) and against the restated constructors otherwise (cosine, squared radius and its epsilon —
    tests/test_lights_host.py holds those restatements to the same fixture), the cosine also against the directions SunLight::intersect
    took and refused."""
    doc = gold
    names = doc["sets"]
    sc = plane_scene([lights_fixture.light(doc, n) for n in names], res=8)
    yi = Interface()
    scenes.load_scene(yi, sc, scenes.render_settings(8, 8, 1, integrator="directlighting"))
    yi.prepareRender()
    rec = yi.getLights()
    assert rec.shape[0] == len(names)
    bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
    for k, name in enumerate(names):
        p = lights_fixture.light(doc, name)
        L = rec[k]
        kb = lambda n: np.full((n, 1), np.uint32(k)).view(np.float32)
        dirac, can_intersect, n_samples = doc[name + "_flags3"]
        if p["type"] == "directionallight":
            inp, want = lights_fixture.leaf(doc, name, "illuminate")
            exact(yi.probe(17, np.hstack([inp, kb(len(inp))]), 8), want, f"{name} illuminate")
            ok = want[:, 0] != 0
            assert dirac == 1 and int(L[:4].view(np.int32)[3]) == int(p.get("infinite", True))
            assert np.array_equal(bits(L[W_DIR:W_DIR + 3]), want[ok][0, 1:4]) and np.array_equal(bits(L[W_COLOR:W_COLOR + 3]), want[ok][0, 5:8])
        elif p["type"] == "sunlight":
            inp, want = lights_fixture.leaf(doc, name, "illum_sample")
            exact(yi.probe(18, np.hstack([inp, kb(len(inp))]), 9), want, f"{name} illumSample")
            assert bits(L[W_PDF]) == want[0, 5] and np.array_equal(bits(L[W_COLPDF:W_COLPDF + 3]), want[0, 6:9])
            inp, want = lights_fixture.leaf(doc, name, "intersect")
            exact(yi.probe(19, np.hstack([inp, kb(len(inp))]), 6), want, f"{name} intersect")
            ok = want[:, 0] != 0
            assert bits(L[W_INVPDF]) == want[ok][0, 2] and np.array_equal(bits(L[W_COLPDF:W_COLPDF + 3]), want[ok][0, 3:6])
            c = sun_consts(p["direction"], p["color"], p["power"], p["angle"])
            cosine = dot(inp, np.broadcast_to(c["direction"], inp.shape))
            assert cosine[~ok].max() < L[W_COS] <= cosine[ok].min()
            assert bits(L[W_COS]) == bits(c["cos_angle"])
            for w, key in ((W_DIR, "direction"), (W_DU, "du"), (W_DV, "dv")):
                assert np.array_equal(bits(L[w:w + 3]), bits(c[key])), (name, key)
            assert (dirac, can_intersect) == (0, 1) and int(L[:4].view(np.int32)[1]) == n_samples
        else:
            inp, want = lights_fixture.leaf(doc, name, "illum_sample")
            exact(yi.probe(20, np.hstack([inp, kb(len(inp))]), 9), want, f"{name} illumSample")
            ok = want[:, 0] != 0
            assert np.array_equal(bits(L[W_COLOR:W_COLOR + 3]), want[ok][0, 6:9])
            r2, r2eps = sphere_consts(p["radius"])
            assert bits(L[W_RAD2]) == bits(r2) and bits(L[W_RAD2EPS]) == bits(r2eps)
            assert (dirac, can_intersect) == (0, 0) and int(L[:4].view(np.int32)[1]) == n_samples


# ---- 2.-4. directional lights --------------------------------------------------------------------------------------
def test_directional_plane_matches_the_closed_form():
    img, _ = render(plane_scene([directional()]))
    np.testing.assert_allclose(img, np.broadcast_to(lambert_value(), img.shape), rtol=1e-5)


def occluder(h=20.0, half=1.5, shift=(0.0, 0.0)):
    """a horizontal quad at height h, centred on the line from the origin along DIR30: far away along the light's direction"""
    t = h / DIR30[2]
    cx, cy = DIR30[0] * t + shift[0], DIR30[1] * t + shift[1]
    return scenes._quad((cx - half, cy - half, h), (cx + half, cy - half, h), (cx + half, cy + half, h), (cx - half, cy + half, h))


def occluder_coords(pts, h=20.0, shift=(0.0, 0.0)):
    """where the ray from each plane point along DIR30 crosses the occluder's plane, relative to the occluder's centre"""
    t = (h - pts[..., 2]) / DIR30[2]
    x, y = pts[..., 0] + DIR30[0] * t, pts[..., 1] + DIR30[1] * t
    return x - (DIR30[0] * h / DIR30[2] + shift[0]), y - (DIR30[1] * h / DIR30[2] + shift[1])


def shadow_mask(pts, h=20.0, half=1.5, shift=(0.0, 0.0)):
    x, y = occluder_coords(pts, h, shift)
    return (np.abs(x) < half) & (np.abs(y) < half)


def test_directional_shadows_infinite_and_finite():
    opaque = {"type": "shinydiffusemat", "color": (0.5, 0.5, 0.5)}
    v = lambert_value()
    img, yi = render(plane_scene([directional()], extra=[(occluder(), opaque)]))
    m = shadow_mask(plane_points(yi))
    keep = stable(m)
    assert m[keep].sum() > 200 and (~m[keep]).sum() > 2000
    assert (img[m & keep] == 0).all(), "an infinite directional light's shadow ray must reach the far occluder"
    np.testing.assert_allclose(img[~m & keep], np.broadcast_to(v, img[~m & keep].shape), rtol=1e-5)
    # finite: the cylinder of `radius` around `from` along the direction; the occluder lies beyond `from` (tmax <= 0 side): no shadow
    frm = tuple(10.0 * c for c in DIR30)
    img, yi = render(plane_scene([directional(infinite=False, radius=1.5, **{"from": frm})], extra=[(occluder(), opaque)]))
    pts = plane_points(yi)
    vec = np.array(frm) - pts
    inside = np.linalg.norm(np.cross(np.array(DIR30), vec), axis=-1) <= 1.5
    keep = stable(inside)
    assert inside[keep].sum() > 500 and (~inside[keep]).sum() > 500
    assert (img[~inside & keep] == 0).all()
    np.testing.assert_allclose(img[inside & keep], np.broadcast_to(v, img[inside & keep].shape), rtol=1e-5)


def test_transparent_shadows_on_infinite_rays():
    filt = (0.3, 0.6, 0.9)
    glass = {"type": "shinydiffusemat", "color": filt, "transparency": 1.0, "transmit_filter": 1.0}
    img, yi = render(plane_scene([directional()], extra=[(occluder(), glass)]), transpShad=True, shadowDepth=4)
    pts = plane_points(yi)
    m = shadow_mask(pts)
    # a shadow ray through the quad's shared diagonal meets both of its triangles and is filtered by each (intersectTs keeps a set of
    # triangles, kdtree_triangle.cc:983-1162): leave out the pixels whose footprint (0.05 units wide here) reaches the diagonal
    x, y = occluder_coords(pts)
    keep = stable(m) & (np.abs(x - y) > 0.15)
    v = lambert_value()
    assert m[keep].sum() > 200
    # ShinyDiffuseMaterial::getTransparency (material_shiny_diffuse.cc:541-563): transmit_filter * colour + (1 - transmit_filter), times
    # transparency^1 without a mirror lobe
    np.testing.assert_allclose(img[m & keep], np.broadcast_to(v * np.array(filt), img[m & keep].shape), rtol=1e-5)
    np.testing.assert_allclose(img[~m & keep], np.broadcast_to(v, img[~m & keep].shape), rtol=1e-5)


# ---- 5. sun ------------------------------------------------------------------------------------------------------
K_MIS_FLAGS = 0x3e          # BsdfGlossy | BsdfDiffuse | BsdfDispersive | BsdfReflect | BsdfTransmit (integrator_montecarlo.cc:214, :298)


def sun_estimate_mean(mat, rec, wo, n=(0.0, 0.0, 1.0), G=128):
    """What doLightEstimation's sampled branch returns ON AVERAGE for sun light `rec` (a getLights() row) at a surface point with normal n
    seen from wo: both halves of the MIS pair (integrator_montecarlo.cc:161-262, :273-333) integrated by G x G midpoint quadrature over
    their sample square, with the material's eval / pdf / sample from the oracle (yor_material_probe, pinned against the reference's own
    material sources).  This is the estimator's exact expectation in the reference's conventions — its BSDF half weighs a hit with the
    sampler's W, and for the diffuse lobe the reference's pdf is cos, not cos / pi, so the sum is NOT the ideal cone integral
    rho * colour * <cos>: 0.45 % below it on the diffuse plane at 10 degrees, where the BSDF half has 0.2 % of the weight."""
    L = po.lib()
    md = po.material_desc(mat)
    d, du, dv = (np.ascontiguousarray(rec[w:w + 3], np.float32) for w in (W_DIR, W_DU, W_DV))
    cos_a, pdf_l, lp = rec[W_COS], float(rec[W_PDF]), 1.0 / float(rec[W_INVPDF])
    lcol = rec[W_COLPDF:W_COLPDF + 3].astype(np.float64)
    g = ((np.arange(G) + 0.5) / G).astype(np.float32)
    s1, s2 = [a.ravel() for a in np.meshgrid(g, g)]
    N = s1.size
    cone = sample_cone(np.broadcast_to(d, (N, 3)), np.broadcast_to(du, (N, 3)), np.broadcast_to(dv, (N, 3)), np.full(N, cos_a, np.float32), s1, s2)
    n = np.array(n, np.float32)
    inp = np.zeros(14, np.float32); e = np.zeros(3, np.float32); s8 = np.zeros(8, np.float32)
    bf, pdf, so = C.c_int32(), C.c_float(), C.c_int32()
    light_half = np.zeros(3); bsdf_half = np.zeros(3)
    for i in range(N):
        inp[:] = [*n, *n, *wo, *cone[i], s1[i], s2[i]]
        L.yor_material_probe(C.byref(md), po.fptr(inp), K_MIS_FLAGS, C.byref(bf), po.fptr(e), C.byref(pdf), C.byref(so), po.fptr(s8))
        m = pdf.value                                            # light half: ls.col_ = col_pdf, weight l^2 / (l^2 + m^2)
        w = pdf_l * pdf_l / (pdf_l * pdf_l + m * m) if m > 1e-6 else 1.0
        light_half += e.astype(np.float64) * lcol * abs(float(np.dot(n, cone[i]))) * w / pdf_l
        spdf, W = float(s8[6]), float(s8[7])                     # BSDF half: the sampled direction, if SunLight::intersect takes it
        if spdf > 1e-6 and float(np.dot(s8[3:6], d)) >= cos_a:
            bsdf_half += s8[:3].astype(np.float64) * lcol * (spdf * spdf / (lp * lp + spdf * spdf)) * W
    return light_half / N, bsdf_half / N


def test_sun():
    ref, _ = render(plane_scene([directional()]))
    img, _ = render(plane_scene([sun(angle=0.05)]))
    np.testing.assert_allclose(img, ref, rtol=1e-3)
    # 10 degrees: the diffuse lobe's eval, pdf and sample do not depend on wo, so every pixel has the same expectation
    img, yi = render(plane_scene([sun(angle=10.0)]), spp=64)
    lh, bh = sun_estimate_mean({"type": "shinydiffusemat", "color": RHO, "diffuse_reflect": 1.0}, yi.getLights()[0], (0.0, 0.0, 1.0))
    # the frame mean (10^4 pixels x 64 spp x 4 Halton samples) was measured 3e-6 from the expectation; the bound leaves 60 times that
    np.testing.assert_allclose(img.reshape(-1, 3).mean(axis=0), lh + bh, rtol=2e-4)


def test_sun_on_a_glossy_plane_pins_the_bsdf_half():
    """A sharp Blinn lobe (exponent 200) facing a sun straight above: the BSDF half of the MIS pair carries 23 % of the estimate, so the
    colour SunLight::intersect returns (col_pdf), its inverse pdf and the weight m^2 / (l^2 + m^2) all show in the frame mean.  The
    camera is far away (wo within 0.7 degrees of the normal); the expectation is taken at a 4 x 4 grid of pixel centres and averaged."""
    res, spp = 64, 64
    glossy = {"type": "glossy", "color": (0.9, 0.8, 0.7), "diffuse_reflect": 0.0, "glossy_reflect": 1.0, "exponent": 200.0, "as_diffuse": True}
    sc = plane_scene([sun(direction=(0.0, 0.0, 1.0), angle=10.0)], res=res, plane_mat=glossy)
    sc["camera"] = dict(sc["camera"], **{"from": (0.0, 0.0, 200.0), "up": (0.0, 1.0, 200.0), "focal": 40.0})
    img, yi = render(sc, spp=spp, res=res)
    rec = yi.getLights()[0]
    pts = plane_points(yi, res)[8::16, 8::16].reshape(-1, 3)
    halves = []
    for p in pts:
        wo = np.array([0.0, 0.0, 200.0]) - p
        halves.append(sun_estimate_mean(glossy, rec, (wo / np.linalg.norm(wo)).astype(np.float32)))
    lh = np.mean([h[0] for h in halves], axis=0); bh = np.mean([h[1] for h in halves], axis=0)
    assert (bh / (lh + bh) > 0.2).all(), "the BSDF half should carry a large share here"
    # measured 4.5e-5 from the expectation at 64 and at 256 spp alike (what is left is the quadrature over wo, not sampling noise); the
    # bound leaves 20 times that, and a wrong colour or weight in the BSDF half moves the mean by percents
    np.testing.assert_allclose(img.reshape(-1, 3).mean(axis=0), lh + bh, rtol=1e-3)


# ---- 6. sphere -----------------------------------------------------------------------------------------------------
def test_sphere_light_takes_the_light_half_only():
    r, h = 0.3, 2.0
    c = (0.0, 0.0, h)
    img, yi = render(plane_scene([{"type": "spherelight", "from": c, "radius": r, "color": (1.0, 1.0, 1.0), "power": 3.0, "samples": 4}]), spp=64)
    st = yi.getRenderStats()
    # per (camera hit, light sample) at most one shadow ray: the light-sampling half only (canIntersect() is false)
    assert st.rays_shadow <= st.camera_samples * 4
    assert st.rays_shadow > 0.99 * st.camera_samples * 4
    # E[f L cos / pdf] over the cone, with the reference's pdf 1 / (2 (1 - cos alpha)) (no pi, light_sphere.cc:96) = f L (1 / pi) x (the
    # sphere's projected solid angle, pi (r/d)^2 cos(theta)) = f L (r/d)^2 cos(theta): a point light at the centre of power r^2 x power
    # gives the same mean
    pt, _ = render(plane_scene([{"type": "pointlight", "from": c, "color": (1.0, 1.0, 1.0), "power": float(np.float32(r) * np.float32(r) * 3.0)}]))
    assert abs(img.mean() / pt.mean() - 1) < 5e-3
    np.testing.assert_allclose(img, pt, rtol=0.05)
    # the sun takes both halves: per (camera hit, light sample) one light-half ray (its illumSample never fails) and one BSDF-half ray when
    # the diffuse sample falls in the cone — at most two.  With an 80 degree cone that is 1 + P, P = the cosine-weighted share of the
    # hemisphere inside the cone, by quadrature (0.86)
    _, ys = render(plane_scene([sun(angle=80.0)]))
    ss = ys.getRenderStats()
    rec = ys.getLights()[0]
    u = (np.arange(1000) + 0.5) / 1000
    a, b = np.meshgrid(u, u)
    sin_t, cos_t, ph = np.sqrt(a), np.sqrt(1 - a), 2 * np.pi * b
    d = rec[W_DIR:W_DIR + 3].astype(np.float64)
    P = ((sin_t * np.cos(ph) * d[0] + sin_t * np.sin(ph) * d[1] + cos_t * d[2]) >= rec[W_COS]).mean()
    ratio = ss.rays_shadow / (ss.camera_samples * 4)
    assert ratio <= 2.0 and abs(ratio - (1 + P)) < 0.02, (ratio, 1 + P)


# ---- 7. serial-state replay, sharding, pass pipelining -------------------------------------------------------------
def three_light_scene(res=96):
    sc = scenes.cornell_soup(1500, seed=41, res=(res, res))
    sc["lights"] = sc["lights"] + [sun(direction=(0.2, -0.9, 0.4), angle=5.0, samples=2),
                                   {"type": "spherelight", "from": (0.3, -0.3, 0.3), "radius": 0.1, "color": (1.0, 0.9, 0.8), "power": 8.0, "samples": 3}]
    sc["camera"] = dict(sc["camera"], resx=res, resy=res)
    return sc


def test_replay_shards_and_pipelining_with_three_light_types():
    import torch
    from libyafaray_amd.parallel import _DeviceFloats
    W = H = 96; T = 32; WORLD = 2
    sc = three_light_scene(W)
    rd = scenes.render_settings(W, H, 4, bounces=4, tile_size=T, russian_roulette_min_bounces=1)
    yi = Interface()
    scenes.load_scene(yi, sc, rd)
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
    # pass pipelining on and off (independent passes: no replay, so that consecutive passes may overlap)
    films = []
    for mode in (0, 1):
        y2 = Interface()
        scenes.load_scene(y2, sc, dict(rd, AA_passes=3, AA_inc_samples=2, AA_threshold=0.0))
        y2.setSerialReplay(False)
        y2.setPassPipelining(mode)
        y2.render()
        films.append(y2.getFilm(W, H).copy())
    assert np.array_equal(films[0], films[1])



# ---- 8. every light type in one scene, against the oracle --------------------------------------------------------------
@pytest.mark.parametrize("mode", ["directlighting", "pathtracing", "pathtracing_three_passes"])
def test_render_matches_oracle_with_every_light_type(mode):
    """One light of each of the five types in the soup's room, against the oracle (which tests/test_integrator_golden.py holds to the
    reference's own integrators on these light types): every pixel within the parity tolerance, no outliers, the oracle's ray counts.
    With five lights the path tracer's light choice is the reference's serial counter: the device replays it, the oracle renders
    single-threaded from the same libc state."""
    from tests.test_gpu_parity import _render_with_rand_state, compare_films, render_both
    W, H = 48, 40
    sc = lights_fixture.five_light_scene(800, seed=43, res=(W, H))
    if mode == "directlighting":
        rd = scenes.render_settings(W, H, 2, integrator="directlighting", raydepth=2, tile_size=16)
        film, st, ofilm, ost = render_both(sc, rd)
    else:
        aa = dict(AA_passes=3, AA_inc_samples=2, AA_threshold=0.02, AA_light_sample_multiplier_factor=1.5) if mode.endswith("passes") else {}
        rd = scenes.render_settings(W, H, 4, bounces=3, tile_size=16, **aa)          # roulette off (render_settings' default)
        # (adaptive passes: the oracle walks the product's tree — a camera ray on a pixel's diagonal can run into the edge two walls share,
        # a tie that the tree's topology resolves: see tests.test_gpu_parity._render_with_rand_state)
        film, st, ofilm, ost = _render_with_rand_state(sc, rd, same_tree=bool(aa))
    assert film[..., :3].sum() > 0
    assert (st.camera_samples, st.rays_closest, st.rays_shadow) == (ost.camera_samples, ost.rays_closest, ost.rays_shadow)
    compare_films(film, ofilm, f"five light types, {mode}")
