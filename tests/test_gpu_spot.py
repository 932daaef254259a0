"""Spot lights on the DEVICE: SpotLight::illuminate, ::illumSample and ::intersect bit for bit against the float32 restatement of
tests/spot_fixture.py (probe ops 41-43), a Dirac render against a point light and the restatement's smoothstep pixel by pixel, shadows,
the soft mode's mean against a quadrature of its estimator (the light half WITH its MIS weight: a soft spot is intersectable, and darker
for it), the serial-state replay with sharding and pass pipelining beside an area and a mesh light, the shading kernel a scene with a
spot light takes, and an XML scene end to end.

Every test here fails without the feature: createLight refused every spotlight."""
import re

import numpy as np
import pytest

from libyafaray_amd import Interface, render_xml, scenes
from tests import spot_fixture as spf
from tests import xml_writer
from tests.test_gpu_components import exact
from tests.test_gpu_ibl import np_fcos, np_fsin
from tests.test_gpu_lights import RES, RHO, plane_points, plane_scene, render
from tests.test_lights_host import F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def torch_first():
    """the emulated shard exchange hands device memory to torch: let torch open the GPU before the library does"""
    import torch
    torch.cuda.init()


def spot(**kw):
    return dict({"type": "spotlight", "from": (0.0, 0.0, 3.0), "to": (0.0, 0.0, 0.0), "color": (1.0, 1.0, 1.0), "power": 9.0}, **kw)


def kbits(n, k):
    return np.full((n, 1), np.uint32(k)).view(np.float32)


FROM, TO, COL, POWER = (0.25, -0.5, 2.0), (0.75, 0.25, 0.0), (0.9, 0.7, 0.3), 5.0
# cone_angle, blend, shadowFuzzyness, soft_shadows: blends 0 / 0.15 / 1, cone angles 5 / 45 / 120, fuzzyness 0 / 0.5 / 1, both kinds
LEAF = [(45.0, 0.15, 1.0, False), (45.0, 0.0, 1.0, False), (45.0, 1.0, 0.5, True), (5.0, 0.15, 1.0, True),
        (5.0, 1.0, 0.0, False), (120.0, 0.15, 0.5, True), (120.0, 0.0, 0.0, True), (120.0, 1.0, 1.0, False)]


def leaf_consts(k):
    a, b, f, _ = LEAF[k]
    return spf.consts(FROM, TO, COL, POWER, a, b, f)


@pytest.fixture(scope="module")
def leaf():
    """one scene with eight spot lights at one place, on a skew axis"""
    lights = [spot(**{"from": FROM, "to": TO, "color": COL, "power": POWER, "cone_angle": a, "blend": b, "shadowFuzzyness": f,
                      "soft_shadows": s, "samples": 2}) for a, b, f, s in LEAF]
    yi = Interface()
    scenes.load_scene(yi, plane_scene(lights, res=8), scenes.render_settings(8, 8, 1, integrator="directlighting"))
    yi.prepareRender()
    assert [int(t) for t in yi.getLights()[:, 0].view(np.int32)] == [12 if s else 11 for _, _, _, s in LEAF]
    return yi


def points(c, rng, n=2048):
    """2048 points: a box around the light, the light's own position (refused), 64 on the plane through the light across its axis, 64 on
    each of the two cones (cos_end_, cos_start_) together with the cosine's float neighbours, 64 along the axis before the light and 64
    behind it.  The special points lie 0.2 to 3 from the light, half of them nearer than 1 (the pdf correction of illumSample)."""
    p = (c["position"] + rng.uniform(-3, 3, (n, 3))).astype(np.float32)
    p[0] = c["position"]
    t = rng.uniform(-2, 2, (64, 2)).astype(np.float32)
    p[1:65] = c["position"] + t[:, :1] * c["du"] + t[:, 1:] * c["dv"]
    at = 65

    def radii(m):
        return np.where(np.arange(m) % 2 == 0, rng.uniform(0.2, 1.0, m), rng.uniform(1.0, 3.0, m))[:, None]

    for cos in (c["cos_end"], c["cos_start"]):
        for cc in (cos, np.nextafter(cos, F(2)), np.nextafter(cos, F(-2))):
            cc = np.float64(min(max(cc, F(-1)), F(1)))
            phi = rng.uniform(0, 2 * np.pi, (64, 1))
            # the direction TO the light makes the angle with ndir_: the point lies at position - r * that direction
            d = c["ndir"].astype(np.float64) * cc + (c["du"] * np.cos(phi) + c["dv"] * np.sin(phi)) * np.sqrt(max(1.0 - cc * cc, 0.0))
            p[at:at + 64] = (c["position"] - radii(64) * d).astype(np.float32)
            at += 64
    p[at:at + 64] = c["position"] - radii(64).astype(np.float32) * c["ndir"]; at += 64        # in front: on the axis, lit
    p[at:at + 64] = c["position"] + radii(64).astype(np.float32) * c["ndir"]; at += 64        # behind the light
    assert at == 577
    return p


# ---- 1 .. 3: the light's functions, bit for bit ------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(LEAF)))
def test_illuminate_bit_for_bit(leaf, k):
    c = leaf_consts(k)
    pts = points(c, np.random.default_rng(31 + k))
    want = spf.illuminate(c, pts)
    ok = want[:, 0] == 1
    _, _, _, cosa, _ = spf._to_light(c, pts)
    plain = ok & (cosa >= c["cos_start"])
    print(f"light {k} {LEAF[k]}: accepted {ok.mean():.3f}, plain {plain.sum()}, falloff {(ok & ~plain).sum()}")
    assert want[0, 0] == 0 and 0.05 <= ok.mean() <= 1
    assert plain.any() and ((ok & ~plain).any() or LEAF[k][1] == 0.0), "both colour branches (blend 0 has no falloff to reach)"
    o = leaf.probe(41, np.hstack([pts, kbits(len(pts), k)]), 8)
    exact(o, want.view(np.uint32), f"illuminate, light {k}")


def test_illum_sample_bit_for_bit(leaf):
    near = far = 0
    for k in range(len(LEAF)):
        c = leaf_consts(k)
        rng = np.random.default_rng(31 + k)
        pts = points(c, rng)
        s = rng.random((len(pts), 2)).astype(np.float32)
        one = np.nextafter(F(1), F(0))
        s[450:458] = [(0, 0), (0, one), (one, 0), (one, one), (0, 0.5), (0.5, 0), (one, 0.5), (0.5, one)]      # (points 449 .. 512 lie on the axis in front: accepted)
        want = spf.illum_sample(c, pts, s[:, 0], s[:, 1])
        ok = want[:, 0] == 1
        assert want[0, 0] == 0 and 0.05 <= ok.mean() <= 1 and ok[450:458].all()
        d2 = ((c["position"] - pts) ** 2).sum(axis=1)
        near += int((ok & (want[:, 5] == 1) & (d2 < 0.999)).sum()); far += int((ok & (want[:, 5] > 1)).sum())
        o = leaf.probe(42, np.hstack([pts, s, kbits(len(pts), k)]), 9)
        exact(o, want.view(np.uint32), f"illumSample, light {k}")
    print(f"illumSample: {near} accepted points with dist_sqr < 1, {far} above it")
    assert near >= 200 and far >= 200


ORIGIN_LIGHTS = [((0.0, 0.0, 0.0), (0.0, 0.0, -1.0)), ((0.0, 0.0, 0.0), (0.0, 0.0, 1.0)), ((0.0, 0.0, 0.0), (-1.0, 0.0, 0.0)),
                 ((0.0, 0.0, 0.0), (1.0, 0.0, 0.0)), ((0.05, 0.0, 0.0), (0.05, 0.0, -1.0)), ((0.05, 0.0, 0.0), (0.05, 0.0, 1.0)),
                 ((0.05, 0.0, 0.0), (-1.0, 0.0, 0.0)), ((0.05, 0.0, 0.0), (1.0, 0.0, 0.0))]


def test_intersect_bit_for_bit():
    """SpotLight::intersect answers true only for a ray that meets the plane through the light in a point whose offset along the axis is
    EXACTLY zero and that lies within 0.1 of the world origin: lights at the origin and at (0.05, 0, 0), axes along +-z and +-x; rays
    from origins on a grid of dyadic offsets aimed through the light (along and against the axis, inside the falloff, outside the
    cone), which can meet the exact-zero test, and random rays, which meet it by luck alone (with the light's plane at z = 0 the product
    t * dir.z often rounds back to -from.z, but the hit point then still has to fall within 0.1 of the origin and inside the cone: one
    ray in a thousand).  With the light at x = 0.05 and the axis along x no ray from these origins meets it: 0.05f has more low bits than
    a sum of magnitude 0.5 to 2 keeps, so those two lights answer false throughout, which is held bit for bit as well"""
    lights = [spot(**{"from": f, "to": t, "color": COL, "power": POWER, "cone_angle": 45.0, "blend": 0.5, "soft_shadows": True, "samples": 2})
              for f, t in ORIGIN_LIGHTS]
    yi = Interface()
    scenes.load_scene(yi, plane_scene(lights, res=8), scenes.render_settings(8, 8, 1, integrator="directlighting"))
    yi.prepareRender()
    g = np.array([-2.0, -1.0, -0.5, 0.0, 0.5, 1.0, 2.0], np.float32)
    offs = np.stack(np.meshgrid(g, g, g), axis=-1).reshape(-1, 3)
    offs = offs[(offs != 0).any(axis=1)]
    n_true = n_false = n_plain = n_fall = 0
    for k, (f, t) in enumerate(ORIGIN_LIGHTS):
        c = spf.consts(f, t, COL, POWER, 45.0, 0.5, 1.0)
        rng = np.random.default_rng(7 + k)
        frm = (c["position"] + offs).astype(np.float32)
        d = spf.normalize(c["position"] - frm).astype(np.float32)
        rf = rng.uniform(-2, 2, (1024, 3)).astype(np.float32)
        rd = rng.normal(size=(1024, 3)); rd = (rd / np.linalg.norm(rd, axis=1, keepdims=True)).astype(np.float32)
        frm = np.concatenate([frm, rf]); d = np.concatenate([d, rd])
        want = spf.intersect(c, frm, d)
        ok = want[:, 0] == 1
        plain = ok & (want[:, 3] == c["color"][0])
        print(f"light {k}: {ok.sum()} rays answered true ({plain.sum()} plain, {(ok & ~plain).sum()} in the falloff), {(~ok).sum()} false")
        n_true += int(ok.sum()); n_false += int((~ok).sum()); n_plain += int(plain.sum()); n_fall += int((ok & ~plain).sum())
        o = yi.probe(43, np.hstack([frm, d, kbits(len(frm), k)]), 6)
        exact(o, want.view(np.uint32), f"intersect, light {k}")
    assert n_true >= 16 and n_false >= 1000 and n_plain > 0 and n_fall > 0


# ---- 4. the Dirac render ----------------------------------------------------------------------------------------------------
CONE = {"cone_angle": 40.0, "blend": 0.5}
POINT = {"type": "pointlight", "from": (0.0, 0.0, 3.0), "color": (1.0, 1.0, 1.0), "power": 9.0}
EDGE_BAND = 1e-5            # on the cosine to the axis: pixels this close to cos_end_ or cos_start_ may fall on either side
# pointlight_illuminate and spotlight_illuminate (yafgpu_shading.h, yafgpu_wavefront.h) share their arithmetic up to the colour: both form
# dist_sqr, dist, 1 / dist_sqr, the direction, and inside the inner cone both return color * idist_sqr.  There the two films are equal
# bit for bit.  In the falloff the spot returns color * (v * idist_sqr) where the point light returns color * idist_sqr.  Roundings, each at
# most 2^-24 relative: v * idist_sqr, its product with the colour, (eval * lcol), * angle and the film's weight on the spot's side (5); the
# product with the colour, (eval * lcol), * angle and the film on the point light's (4).  Nine, below the 16 that 2^-20 leaves room for.
ROUND_BAND = 2.0 ** -20
# The smoothstep itself is taken at the restatement's surface point, which is the pixel's camera ray (the device's own, probe op 7) cut with
# z = 0 in numpy, while the device's is the same ray at the distance its triangle test found.  Both distances (below 6.2, one float32 step
# there is 4.8e-7) carry a handful of roundings: allowing each four steps and the point's own three roundings (2.4e-7 each), the two surface
# points lie within 5e-6 of each other, and the cosine to the axis of a light at least 3 away within DCOS = 5e-6 / 3.  The smoothstep's
# slope in v is at most 1.5, v's slope in the cosine is icos_diff_.
DCOS = 5e-6 / 3.0


def classes(c, yi):
    pts = plane_points(yi).reshape(-1, 3).astype(np.float32)
    _, _, _, cosa, _ = spf._to_light(c, pts)
    edge = (np.abs(cosa - c["cos_end"]) < EDGE_BAND) | (np.abs(cosa - c["cos_start"]) < EDGE_BAND)
    inner, fall, outside = (cosa > c["cos_start"]) & ~edge, (cosa < c["cos_start"]) & (cosa > c["cos_end"]) & ~edge, (cosa < c["cos_end"]) & ~edge
    return pts, cosa, edge, inner, fall, outside


def test_dirac_render_pixel_by_pixel():
    a, ya = render(plane_scene([spot(**CONE)]))
    b, _ = render(plane_scene([POINT]))
    c = spf.consts((0, 0, 3), (0, 0, 0), (1, 1, 1), 9.0, 40.0, 0.5)
    _, cosa, edge, inner, fall, outside = (x.reshape(RES, RES) if x.ndim == 1 else x for x in classes(c, ya))
    print(f"{inner.sum()} pixels in the inner cone, {fall.sum()} in the falloff, {outside.sum()} outside, {edge.sum()} within {EDGE_BAND} of a cone")
    assert edge.mean() <= 0.02 and inner.sum() > 1000 and fall.sum() > 1000 and outside.sum() > 1000
    assert (b > 0).all() and (a[outside] == 0).all()
    assert np.array_equal(a[inner], b[inner]), "inside the inner cone the spot light is the point light, bit for bit"
    sm = spf.falloff(c, cosa[fall]).astype(np.float64)
    ratio = a[fall] / b[fall]
    band = ROUND_BAND * sm + 1.5 * float(c["icos_diff"]) * DCOS
    dev = np.abs(ratio - sm[:, None]).max(axis=1)
    print(f"falloff: largest |image / point light's - smoothstep| {dev.max():.3g}, largest share of its band {np.max(dev / band):.3g}")
    assert sm.min() < 0.05 and sm.max() > 0.95 and (dev <= band).all()


# ---- 5. shadows -------------------------------------------------------------------------------------------------------------
def test_shadows():
    occ = scenes._quad((-1.0, -0.5, 1.5), (0.5, -0.5, 1.5), (0.5, 0.8, 1.5), (-1.0, 0.8, 1.5))
    grey = {"type": "shinydiffusemat", "color": (0.5, 0.5, 0.5)}
    frm = (0.4, 0.2, 3.0)
    aim = {"from": frm, "to": (0.4, 0.2, 0.0), "cone_angle": 60.0, "blend": 0.3}
    a, ya = render(plane_scene([spot(**aim)], extra=[(occ, grey)]))
    b, _ = render(plane_scene([dict(POINT, **{"from": frm})], extra=[(occ, grey)]))
    free, _ = render(plane_scene([spot(**aim)]))
    # the quad hides part of the plane from the camera: only pixels that show the plane count (where the quad-less render's surface point
    # is the plane's too, which is everywhere, and the quad's own pixels are lit from above)
    dark_b = (b == 0).all(axis=-1)
    assert 300 < dark_b.sum() < RES * RES - 300
    assert (a[dark_b] == 0).all(), "the point light's umbra is exactly black under the spot light"
    lit = (free > 0).all(axis=-1)
    assert np.array_equal((a == 0).all(axis=-1) & lit, dark_b & lit)
    off, _ = render(plane_scene([spot(**dict(aim, cast_shadows=False))], extra=[(occ, grey)]))
    on_plane = dark_b                                                  # (a black pixel shows the plane: the quad's top is lit)
    assert np.array_equal(off[on_plane], free[on_plane]), "without cast_shadows the umbra is the render without the quad"
    assert (off[on_plane & lit] > 0).all()


# ---- 6. the soft mode ---------------------------------------------------------------------------------------------------------
def soft_expectation(c, pts, G=32):
    """mean and variance, over the sample square, of one sample of doLightEstimation's light half for a light that CAN be intersected
    (integrator_montecarlo.cc:191-213): eval * ls.col * |n . wi| * w / ls.pdf, w = ls.pdf^2 / (ls.pdf^2 + m_pdf^2), with the
    restatement's illumSample, by G x G midpoint quadrature, in units of RHO * colour.  The plane's ShinyDiffuseMaterial::eval is RHO for
    a direction above the plane and black below it; its pdf for the one diffuse lobe is |n . wi| (material_shiny_diffuse.cc:450-459,
    matb_pdf on the device), and a pdf of 1e-6 or less takes no weight (:194, :229)."""
    g = ((np.arange(G) + 0.5) / G).astype(np.float32)
    s1, s2 = [a.ravel()[None, :] * c["fuzzy"] for a in np.meshgrid(g, g)]
    ldir, dist_sqr, _, cosa, ok = spf._to_light(c, pts)
    cos_ang = F(1) - (F(1) - c["cos_end"]) * s2
    sin_ang = np.sqrt(np.maximum(F(1) - cos_ang * cos_ang, F(0)))
    t1 = (6.28318530717958647692 * s1.astype(np.float64)).astype(np.float32)
    w = ((c["du"][None, None, :] * np_fcos(t1)[..., None] + c["dv"][None, None, :] * np_fsin(t1)[..., None]) * sin_ang[..., None]
         + ldir[:, None, :] * cos_ang[..., None]).astype(np.float32)
    col = np.where(cosa >= c["cos_start"], F(1), spf.falloff(c, cosa)).astype(np.float64)
    assert (dist_sqr >= 1).all()                                       # (no pdf correction on this plane: the light is 3 away)
    pdf = dist_sqr.astype(np.float64)[:, None]
    m = np.abs(w[..., 2]).astype(np.float64)
    weight = np.where(m > 1e-6, pdf * pdf / (pdf * pdf + m * m), 1.0)
    f = np.where(ok[:, None] & (w[..., 2] > 0), col[:, None] * m * weight / pdf, 0.0)
    return f.mean(axis=1), f.var(axis=1)


def test_soft_mode_matches_its_expectation():
    """soft_shadows with 4 samples over 16 camera samples: 64 light samples per pixel, each pixel against the expectation of its
    estimator, as tests/test_gpu_ies.py::test_soft_mode_matches_its_expectation does: six standard deviations of the mean of 64
    independent samples from the estimator's own variance, the footprint term (a 24th of the second differences, added to the
    expectation and, where the falloff bends, to the band), and 1e-4 for the midpoint rule: on these points the 32 x 32 and the 128 x 128
    grids differ by 1.5e-7 of the mean at most and 9.2e-4 of the variance (the estimator is linear in s_2 up to its MIS weight).
    The BSDF half is asked for every sample and never answers: SpotLight::intersect wants its hit point within 0.1 of the world origin,
    the light is 3 away.  So the MIS weight of the light half is lost, and with the cosine of the sampled direction the soft image is
    darker than the Dirac image of the same light: asserted, so that nobody repairs it."""
    light = spot(**dict(CONE, soft_shadows=True, samples=4, shadowFuzzyness=1.0))
    img, yi = render(plane_scene([light]), spp=16)
    c = spf.consts((0, 0, 3), (0, 0, 0), (1, 1, 1), 9.0, 40.0, 0.5, 1.0)
    pts = plane_points(yi).reshape(-1, 3).astype(np.float32)
    mean, var = soft_expectation(c, pts)
    m = mean.reshape(RES, RES)
    d2 = np.zeros_like(m)
    for ax in (0, 1):
        t = np.moveaxis(m, ax, 0)
        dd = np.empty_like(t)
        dd[1:-1] = t[2:] + t[:-2] - 2.0 * t[1:-1]
        dd[0], dd[-1] = dd[1], dd[-2]
        d2 += np.moveaxis(dd, 0, ax)
    footprint = (d2 / 24.0).ravel()
    mean = mean + footprint
    n = 64
    got = img.reshape(-1, 3) / (np.array(RHO)[None, :] * 9.0)
    band = 6.0 * np.sqrt(var / n) + 1e-4 * np.abs(mean) + np.abs(footprint)
    dev = np.abs(got - mean[:, None]).max(axis=1)
    lit = var > 0                                                      # (a pixel outside the cone has only its neighbours' footprint term: 0 against a band of that size)
    print(f"soft mode: worst lit pixel's deviation / band {np.max(dev[lit] / band[lit]):.3g}; frame mean {got[:, 0].mean():.6g} against {mean.mean():.6g}")
    assert mean.max() > 0 and (dev <= band).all()
    assert abs(got[:, 0].mean() - mean.mean()) <= 6.0 * np.sqrt(var.sum() / n) / var.size + 1e-4 * mean.mean()
    st = yi.getRenderStats()
    assert st.rays_shadow <= st.camera_samples * 4, "the BSDF half is asked, intersect never answers, no ray is sent for it"
    dirac, _ = render(plane_scene([spot(**CONE)]), spp=16)             # (the same camera samples: the same footprint)
    on = (dirac > 0).all(axis=-1)
    assert on.sum() > 5000 and (img[on] < dirac[on]).all(), "a soft spot light is darker than the Dirac one (light_spot.cc's own behaviour)"
    print(f"soft / Dirac over the lit pixels: {np.mean(img[on] / dirac[on]):.4f}")


def test_soft_mode_without_fuzzyness_is_deterministic():
    """shadowFuzzyness 0 makes every sample the direction to the light (sampleCone__ with s_1 = s_2 = 0: cos_ang 1, sin_ang 0), so all
    four samples of the one camera sample are the same: eval * (colour * v) * |n . wi| * w / dist_sqr.  Over the point light's image
    (eval * colour / dist_sqr * |n . wi| at the same surface point) that is v * w.  Roundings on this side: colour * v, eval * ls.col,
    * angle, l_2, m_2, their sum and the quotient w, * w, / pdf, two in the sum of four equal samples (3x and none for 4x), * 1/4 exact,
    the film: 12; the point light's 4: 16 roundings of 2^-24, ROUND_BAND, with the surface point's share of test 4 on the smoothstep."""
    light = spot(**dict(CONE, soft_shadows=True, samples=4, shadowFuzzyness=0.0))
    a, ya = render(plane_scene([light]))
    b, _ = render(plane_scene([POINT]))
    c = spf.consts((0, 0, 3), (0, 0, 0), (1, 1, 1), 9.0, 40.0, 0.5, 0.0)
    pts, cosa, edge, inner, fall, outside = classes(c, ya)
    ldir, dist_sqr, _, _, _ = spf._to_light(c, pts)
    sm = np.where(inner, 1.0, spf.falloff(c, cosa).astype(np.float64))
    l2 = dist_sqr.astype(np.float64) ** 2
    w = l2 / (l2 + ldir[:, 2].astype(np.float64) ** 2)
    a = a.reshape(-1, 3); b = b.reshape(-1, 3)
    assert (a[outside] == 0).all()
    keep = inner | fall
    ratio = a[keep] / b[keep]
    want = (sm * w)[keep]
    band = ROUND_BAND * want + np.where(fall[keep], 1.5 * float(c["icos_diff"]) * DCOS, 0.0)
    dev = np.abs(ratio - want[:, None]).max(axis=1)
    print(f"fuzzyness 0: largest share of the band {np.max(dev / band):.3g} over {keep.sum()} pixels")
    assert keep.sum() > 7000 and (dev <= band).all()


# ---- 7. serial-state replay, shards, pass pipelining ---------------------------------------------------------------------------
def test_replay_shards_and_pipelining_with_a_spot_light():
    """tests.test_gpu_ies.test_replay_shards_and_pipelining_with_an_ies_light with a spot light of each kind in place of the IES lights"""
    import torch
    from libyafaray_amd.parallel import _DeviceFloats
    from tests.test_gpu_meshlight import soup_with_a_box_light
    W = H = 96; T = 32; WORLD = 2
    sc = soup_with_a_box_light(W)
    sc["lights"] = sc["lights"] + [spot(**{"from": (0.3, -0.4, 0.9), "to": (0.0, 0.0, -1.0), "power": 2.0, "cone_angle": 50.0, "blend": 0.4}),
                                   spot(**{"from": (-0.5, 0.2, 0.8), "to": (-0.2, 0.0, -1.0), "power": 1.5, "cone_angle": 35.0,
                                           "soft_shadows": True, "samples": 2})]
    rd = scenes.render_settings(W, H, 4, bounces=4, tile_size=T, russian_roulette_min_bounces=1)
    yi = Interface()
    scenes.load_scene(yi, sc, rd)
    assert [int(t) for t in yi.getLights()[:, 0].view(np.int32)] == [0, 7, 11, 12]
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
    assert np.array_equal(total, full), "two shards do not sum to the single-GPU film"
    films = []
    for mode in (0, 1):
        y2 = Interface()
        scenes.load_scene(y2, sc, dict(rd, AA_passes=3, AA_inc_samples=2, AA_threshold=0.0))
        y2.setSerialReplay(False)      # (a pass that replays is never pipelined: the three passes run with the per-sample streams)
        y2.setPassPipelining(mode)
        y2.render()
        films.append(y2.getFilm(W, H).copy())
    assert np.array_equal(films[0], films[1])


# ---- 8. the kernel a scene takes -----------------------------------------------------------------------------------------------
def test_variant_choice(tmp_path, monkeypatch, capfd):
    from tests import ies_fixture as ief
    monkeypatch.setenv("YAFGPU_VERBOSE", "1")
    kernel = lambda: re.findall(r"shading kernel: (\S+) \(", capfd.readouterr().err)
    capfd.readouterr()
    render(plane_scene([POINT]), res=16)
    without = kernel()
    for soft in (False, True):
        render(plane_scene([POINT, spot(soft_shadows=soft)]), res=16)
        assert set(kernel()) == {"spot"}
    # a blend material in use: two carrier triangles under the plane, one of them on a blend of the plane's material and the other's
    under = np.array([[[0.0, 0.0, -5.0], [0.01, 0.0, -5.0], [0.0, 0.01, -5.0]]], np.float32)
    grey = {"type": "shinydiffusemat", "color": (0.5, 0.5, 0.5)}
    blend = {"type": "blend_mat", "material1": "mat0", "material2": "mat1", "blend_value": 0.5}
    render(plane_scene([POINT, spot()], extra=[(under, grey), (under + np.float32(0.5), blend)]), res=16)
    assert set(kernel()) == {"blend_spot"}
    ies = {"type": "ieslight", "file": ief.write(tmp_path, "C1"), "from": (0.0, 0.0, 3.0), "to": (0.0, 0.0, 0.0), "color": (1.0, 1.0, 1.0), "power": 9.0}
    render(plane_scene([ies, spot()]), res=16)
    assert set(kernel()) == {"spot"}, "an IES light beside the spot light: still the spot light's kernel, which has both"
    render(plane_scene([ies]), res=16)
    assert set(kernel()) == {"ies"}
    assert without and not {"spot", "blend_spot"} & set(without)
    render(plane_scene([POINT]), res=16)
    assert kernel() == without, "a scene without a spot light keeps the kernel it had"


# ---- 9. XML end to end ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("soft", [False, True], ids=["dirac", "soft"])
def test_xml_scene_renders_the_film_of_the_api_scene(tmp_path, soft):
    res = 16
    light = spot(**dict(CONE, **{"from": (0.3, -0.2, 3.0), "to": (0.1, 0.2, 0.0), "soft_shadows": soft, "samples": 3, "shadowFuzzyness": 0.75}))
    sc = plane_scene([light], res=res)
    rd = scenes.render_settings(res, res, 2, integrator="directlighting")
    xml = tmp_path / "spot.xml"
    xml_writer.write(xml, sc, rd)
    yx = render_xml.render_xml(xml, tmp_path / "spot.hdr")
    ya = Interface()
    scenes.load_scene(ya, sc, rd)
    ya.render()
    assert np.array_equal(yx.getLights().view(np.uint32), ya.getLights().view(np.uint32))
    fx, fa = yx.getFilm(res, res), ya.getFilm(res, res)
    assert fa[..., :3].max() > 0 and np.array_equal(fx, fa)


# ---- 10. the reference's compiled SpotLight ------------------------------------------------------------------------------------
def test_leaf_functions_match_the_reference():
    """tests/golden/ref_spot_ies_ieee: what the reference's own SpotLight, made by its factory from the parameters stored there (the
    eight lights of LEAF and the eight of ORIGIN_LIGHTS, as tests/test_spot_host.py asserts), gave.  All sixteen are the lights of one
    scene; illuminate, illumSample and intersect (probe ops 41, 42, 43) bit for bit on every row; diracLight() and canIntersect() against
    what light_is_dirac / light_can_intersect (yafgpu_shading.h) make of the type word getLights() shows, nSamples() against its word"""
    from tests import pin_fixture as pin
    doc = pin.load("spot_ies", "ieee")
    names = doc["spot_sets"] + doc["intersect_sets"]
    yi = Interface()
    scenes.load_scene(yi, plane_scene([pin.params(doc, n) for n in names], res=8), scenes.render_settings(8, 8, 1, integrator="directlighting"))
    yi.prepareRender()
    rec = yi.getLights()
    assert rec.shape[0] == len(names) == 16
    rows = 0
    for k, name in enumerate(names):
        dirac, can_intersect, n_samples = doc[name + "_flags3"]
        t, n = (int(x) for x in rec[k, :2].view(np.int32))
        assert t in (spf.TYPE_SPOT, spf.TYPE_SPOT_SOFT)
        assert (dirac, can_intersect) == (int(t == spf.TYPE_SPOT), int(t == spf.TYPE_SPOT_SOFT)), name      # light_is_dirac, light_can_intersect
        assert n == (1 if dirac else n_samples), name
        for fn, op in (("illuminate", 41), ("illum_sample", 42)) if name in doc["spot_sets"] else (("intersect", 43),):
            inp, want, _ = pin.leaf(doc, name, fn)
            exact(yi.probe(op, np.hstack([inp, kbits(len(inp), k)]), want.shape[1]), want, f"{name} {fn}")
            assert 0.02 <= (want[:, 0] != 0).mean() <= 0.98 or fn == "intersect"
            rows += len(inp)
    print(f"{rows} rows against the reference")
    assert rows >= 10000
