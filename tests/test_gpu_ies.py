"""IES photometric lights on the DEVICE: the table lookup, IesLight::illuminate and ::illumSample bit for bit against the float32
restatement of tests/ies_fixture.py (probe ops 38-40), a flat table against a point light, a measured table against the restatement
pixel by pixel, shadows, the soft mode's mean against a quadrature of its estimator, the serial-state replay with sharding and pass
pipelining beside an area and a mesh light, and the shading kernel a scene with an IES light takes."""
import re

import numpy as np
import pytest

from libyafaray_amd import Interface, scenes
from tests import ies_fixture as ief
from tests.test_gpu_components import exact
from tests.test_gpu_ibl import np_fcos, np_fsin
from tests.test_gpu_lights import RES, RHO, plane_points, plane_scene, render
from tests.test_lights_host import F

pytestmark = pytest.mark.gpu
NAMES = sorted(ief.SPECS)


@pytest.fixture(scope="module", autouse=True)
def torch_first():
    """the emulated shard exchange hands device memory to torch: let torch open the GPU before the library does"""
    import torch
    torch.cuda.init()


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("ies")
    return {n: ief.write(d, n) for n in NAMES}


def ies(path, **kw):
    return dict({"type": "ieslight", "file": path, "from": (0.0, 0.0, 3.0), "to": (0.0, 0.0, 0.0), "color": (1.0, 1.0, 1.0), "power": 9.0}, **kw)


def kbits(n, k):
    return np.full((n, 1), np.uint32(k)).view(np.float32)


FROM, TO, COL, POWER = (0.25, -0.5, 2.0), (0.75, 0.25, 0.0), (0.9, 0.7, 0.3), 5.0


@pytest.fixture(scope="module")
def leaf(files):
    """one scene with every fixture file as a Dirac IES light, at the same place"""
    lights = [ies(files[n], **{"from": FROM, "to": TO, "color": COL, "power": POWER}) for n in NAMES]
    yi = Interface()
    scenes.load_scene(yi, plane_scene(lights, res=8), scenes.render_settings(8, 8, 1, integrator="directlighting"))
    yi.prepareRender()
    return yi


def angle_pairs(p, rng, n=4096):
    """every node of both maps paired with every other, both ends, the fold boundaries 90 / 180 / 360 and their float neighbours, angles
    below and beyond the maps, and random ones"""
    special = np.array([0, 90, 180, 270, 360, -90, -0.0], np.float32)
    nodes = np.unique(np.concatenate([p["hor"], p["vert"], p["hor"] - F(90), special]))
    beside = np.concatenate([nodes, np.nextafter(nodes, F(1e9)), np.nextafter(nodes, F(-1e9))])
    g = np.stack(np.meshgrid(beside, beside), axis=-1).reshape(-1, 2)
    if g.shape[0] > n // 2:
        g = np.concatenate([np.stack(np.meshgrid(nodes, nodes), axis=-1).reshape(-1, 2), g[rng.choice(g.shape[0], n // 2, replace=False)]])[:n // 2]
    r = rng.uniform(-20, 380, (n - g.shape[0], 2)).astype(np.float32)
    return np.concatenate([g, r]).astype(np.float32)


@pytest.mark.parametrize("k", range(len(NAMES)))
def test_radiance_bit_for_bit(leaf, k):
    p = ief.parsed(NAMES[k])
    a = angle_pairs(p, np.random.default_rng(11 + k))
    assert a.shape == (4096, 2)
    o = leaf.probe(38, np.hstack([a, kbits(4096, k)]), 2)
    want = np.stack([np.ones(4096, np.float32), ief.radiance(p, a[:, 0], a[:, 1])], axis=1)
    exact(o, want.view(np.uint32), f"getRadiance, {NAMES[k]}")


def points(c, rng, n=2048):
    """points in a box around the light, the light's own position, points on the cone's edge (the plane through the light across its
    axis, where the cosine to the axis is about 0: the edge for a file that reaches 90 degrees) and straight along the axis"""
    p = (c["position"] + rng.uniform(-3, 3, (n, 3))).astype(np.float32)
    p[0] = c["position"]
    t = rng.uniform(-2, 2, (64, 2)).astype(np.float32)
    p[1:65] = c["position"] + t[:, :1] * c["du"] + t[:, 1:] * c["dv"]
    p[65:97] = c["position"] - rng.uniform(0.1, 3, (32, 1)).astype(np.float32) * c["ndir"]
    p[97:129] = c["position"] + rng.uniform(0.1, 3, (32, 1)).astype(np.float32) * c["ndir"]
    return p


@pytest.mark.parametrize("k", range(len(NAMES)))
def test_illuminate_bit_for_bit(leaf, k):
    p = ief.parsed(NAMES[k])
    c = ief.consts(p, FROM, TO, COL, POWER)
    pts = points(c, np.random.default_rng(31 + k))
    o = leaf.probe(39, np.hstack([pts, kbits(len(pts), k)]), 8)
    want = ief.illuminate(p, c, pts)
    assert want[0, 0] == 0 and 0.05 < want[:, 0].mean() <= 1
    exact(o, want.view(np.uint32), f"illuminate, {NAMES[k]}")


@pytest.mark.parametrize("k", range(len(NAMES)))
def test_illum_sample_bit_for_bit(leaf, k):
    p = ief.parsed(NAMES[k])
    c = ief.consts(p, FROM, TO, COL, POWER)
    rng = np.random.default_rng(31 + k)
    pts = points(c, rng)
    s = rng.random((len(pts), 2)).astype(np.float32)
    one = np.nextafter(F(1), F(0))
    s[200:208] = [(0, 0), (0, one), (one, 0), (one, one), (0, 0.5), (0.5, 0), (one, 0.5), (0.5, one)]
    o = leaf.probe(40, np.hstack([pts, s, kbits(len(pts), k)]), 9)
    want = ief.illum_sample(p, c, pts, s[:, 0], s[:, 1])
    assert want[0, 0] == 0 and 0.05 < want[:, 0].mean() <= 1
    exact(o, want.view(np.uint32), f"illumSample, {NAMES[k]}")


# ---- renders --------------------------------------------------------------------------------------------------------
TILTED = {"from": (0.0, 0.0, 3.0), "to": (3.0, 0.0, 1.5)}      # the cone's edge crosses the plane at x = -1.5, inside the frame
# (a) the flat table against a point light.  The table's values and max_rad_ are 1, so getRadiance differs from 1 only by rounding: with
# d in [0, 1], 1 - d rounds by at most 2^-25 and (1 - d) + d by at most 2^-24 more, so rx_1 and rx_2 lie within 2^-24 + 2^-25 of 1; the
# third lerp multiplies them by 1 - d and d (2^-24 relative each), and adds (2^-24): |rad - 1| < 2^-21.  color * rad rounds once more
# (2^-24).  What follows is the point light's arithmetic on a colour that differs by that much: three more roundings, (eval * lcol) * angle
# and the film's weight, which may fall differently for the two inputs, 2^-23 each.  Sum: 2^-21 + 2^-24 + 3 * 2^-23 < 2^-20.
FLAT_BAND = 2.0 ** -20
EDGE_BAND = 1e-5            # on the cosine to the axis: pixels this close to cos_end_ may fall on either side


def test_flat_table_is_a_point_light_inside_the_cone(files):
    a, ya = render(plane_scene([ies(files["FLAT"], **TILTED)]))
    b, _ = render(plane_scene([{"type": "pointlight", "from": TILTED["from"], "color": (1.0, 1.0, 1.0), "power": 9.0}]))
    p = ief.parsed("FLAT")
    c = ief.consts(p, TILTED["from"], TILTED["to"], (1.0, 1.0, 1.0), 9.0)
    pts = plane_points(ya).reshape(-1, 3).astype(np.float32)
    _, _, _, cosa, _ = ief._to_light(c, pts)
    cosa = cosa.reshape(RES, RES)
    edge = np.abs(cosa - c["cos_end"]) < EDGE_BAND
    inside, outside = (cosa > c["cos_end"]) & ~edge, (cosa < c["cos_end"]) & ~edge
    print(f"flat table: {inside.sum()} pixels inside the cone, {outside.sum()} outside, {edge.sum()} within {EDGE_BAND} of its edge")
    assert edge.mean() <= 0.02 and inside.sum() > 1000 and outside.sum() > 1000
    assert (a[outside] == 0).all() and (b > 0).all()
    dev = np.abs(a[inside] / b[inside] - 1).max()
    print(f"largest relative difference from the point light inside the cone: {dev:.3g} (band {FLAT_BAND:.3g})")
    assert dev <= FLAT_BAND


def test_measured_table_pixel_by_pixel(files):
    """C5x7 as a Dirac light off the axis: every pixel is eval * lcol * |n . wi| (doLightEstimation's Dirac branch) with the restatement's
    illuminate at the pixel's surface point; the band is the closed-form tests' of tests/test_gpu_lights.py, rtol 1e-5"""
    light = ies(files["C5x7"], **{"from": (0.5, -0.3, 3.0), "to": (0.0, 0.2, 0.0), "color": (1.0, 0.9, 0.8)})
    img, yi = render(plane_scene([light]))
    p = ief.parsed("C5x7")
    c = ief.consts(p, light["from"], light["to"], light["color"], light["power"])
    pts = plane_points(yi).reshape(-1, 3).astype(np.float32)
    o = ief.illuminate(p, c, pts)
    assert (o[:, 0] == 1).all()
    want = (np.array(RHO)[None, :] * o[:, 5:8].astype(np.float64) * np.abs(o[:, 3:4].astype(np.float64))).reshape(RES, RES, 3)
    assert want.min() > 0 and want.max() / want.min() > 3, "the table should show in the frame"
    np.testing.assert_allclose(img, want, rtol=1e-5)


def test_shadows_are_the_point_lights(files):
    """an occluder between the light and the plane: the shadow rays are the point light's, so the black pixels are the same ones"""
    occ = scenes._quad((-1.0, -0.5, 1.5), (0.5, -0.5, 1.5), (0.5, 0.8, 1.5), (-1.0, 0.8, 1.5))
    grey = {"type": "shinydiffusemat", "color": (0.5, 0.5, 0.5)}
    frm = (0.4, 0.2, 3.0)
    a, _ = render(plane_scene([ies(files["C5x7"], **{"from": frm})], extra=[(occ, grey)]))
    b, _ = render(plane_scene([{"type": "pointlight", "from": frm, "color": (1.0, 1.0, 1.0), "power": 9.0}], extra=[(occ, grey)]))
    dark_a, dark_b = (a == 0).all(axis=-1), (b == 0).all(axis=-1)
    assert 300 < dark_b.sum() < RES * RES - 300
    assert np.array_equal(dark_a, dark_b)
    off, _ = render(plane_scene([ies(files["C5x7"], **{"from": frm, "cast_shadows": False})], extra=[(occ, grey)]))
    lit = off[dark_a]
    assert (lit[lit.sum(axis=-1) > 0] > 0).all() and (off >= a).all()


def soft_expectation(p, c, pts, G=32):
    """mean and variance, over the sample square, of one sample of doLightEstimation's sampled branch for a light that cannot be
    intersected (integrator_montecarlo.cc:244-258): eval * ls.col * |n . wi| / ls.pdf with the restatement's illumSample, by G x G
    midpoint quadrature; vectorised (np_fsin / np_fcos of tests/test_gpu_ibl.py in place of the per-value calls).  The plane's
    ShinyDiffuseMaterial::eval is RHO for a direction above the plane and black below it."""
    g = ((np.arange(G) + 0.5) / G).astype(np.float32)
    s1, s2 = [a.ravel()[None, :] for a in np.meshgrid(g, g)]
    ldir, dist, idist_sqr, cosa, ok = ief._to_light(c, pts)
    cos_ang = F(1) - (F(1) - cosa[:, None]) * s2
    sin_ang = np.sqrt(np.maximum(F(1) - cos_ang * cos_ang, F(0)))
    t1 = (6.28318530717958647692 * s1.astype(np.float64)).astype(np.float32)
    w = ((c["du"][None, None, :] * np_fcos(t1)[..., None] + c["dv"][None, None, :] * np_fsin(t1)[..., None]) * sin_ang[..., None]
         + ldir[:, None, :] * cos_ang[..., None]).astype(np.float32)
    u, v = ief.angles(w, np.broadcast_to(cosa[:, None], cos_ang.shape))
    rad = ief.radiance(p, u, v).astype(np.float64)
    f = np.where(ok[:, None] & (w[..., 2] > 0), rad * idist_sqr[:, None] * np.abs(w[..., 2]), 0.0)
    return f.mean(axis=1), f.var(axis=1)


def test_soft_mode_matches_its_expectation(files):
    """soft_shadows with 4 samples over 16 passes of one camera sample: 64 light samples per pixel.  Each pixel against the expectation
    of its estimator; the band is six standard deviations of the mean of 64 independent samples, from the estimator's own variance by
    the same quadrature (the Halton pairs the integrator uses spread more evenly than independent ones would), plus 1e-4 for the
    midpoint rule: on these points the restatement's 32 x 32 and 128 x 128 grids differ by 7.3e-6 in the mean and 1.4e-3 in the variance.
    The frame mean is held the same way: six standard deviations of the mean of all pixels' samples, plus 1e-4.
    A pixel's 16 camera samples spread over its footprint, so what it shows is the expectation's mean over the footprint, not its value
    at the centre: for a footprint of one pixel that is the centre's value plus a 24th of the second differences to the neighbours'
    values along both axes (the midpoint rule's error term).  The expectation is corrected by that term, and where it is not smooth (the
    table's lookup has a kink on the light's axis, in the middle of the frame) the term is as uncertain as it is large, so its size
    joins the band."""
    light = ies(files["C5x7"], soft_shadows=True, samples=4, color=(1.0, 1.0, 1.0))
    img, yi = render(plane_scene([light]), spp=16)
    p = ief.parsed("C5x7")
    c = ief.consts(p, light["from"], light["to"], light["color"], light["power"])
    pts = plane_points(yi).reshape(-1, 3).astype(np.float32)
    mean, var = soft_expectation(p, c, pts)
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
    band = 6.0 * np.sqrt(var / n) + 1e-4 * mean + np.abs(footprint)
    dev = np.abs(got - mean[:, None]).max(axis=1)
    print(f"soft mode: worst pixel deviation / band {np.max(dev / band):.3g}; frame mean {got[:, 0].mean():.6g} against {mean.mean():.6g}")
    assert mean.min() > 0 and (dev <= band).all()
    print(f"largest footprint term {np.abs(footprint / mean).max():.3g} of the expectation")
    assert abs(got[:, 0].mean() - mean.mean()) <= 6.0 * np.sqrt(var.sum() / n) / var.size + 1e-4 * mean.mean()
    st = yi.getRenderStats()
    assert st.rays_shadow <= st.camera_samples * 4, "the light half only: a light that cannot be intersected sends no BSDF-half ray"


# ---- serial-state replay, shards, pass pipelining -------------------------------------------------------------------------
def test_replay_shards_and_pipelining_with_an_ies_light(files):
    """tests.test_gpu_meshlight.test_replay_shards_and_pipelining_with_a_mesh_light with an IES light of each kind beside the soup's area
    light and the box's mesh light: four lights, so the path tracer's light choice is the reference's serial counter, carried across the
    shards.  Box filter of width 1: no sample reaches into another tile, so the two shards' films sum to the whole film bit for bit."""
    import torch
    from libyafaray_amd.parallel import _DeviceFloats
    from tests.test_gpu_meshlight import soup_with_a_box_light
    W = H = 96; T = 32; WORLD = 2
    sc = soup_with_a_box_light(W)
    sc["lights"] = sc["lights"] + [ies(files["C5x7"], **{"from": (0.3, -0.4, 0.9), "to": (0.0, 0.0, -1.0), "power": 2.0}),
                                   ies(files["C1"], **{"from": (-0.5, 0.2, 0.8), "to": (-0.2, 0.0, -1.0), "power": 1.5, "soft_shadows": True, "samples": 2})]
    rd = scenes.render_settings(W, H, 4, bounces=4, tile_size=T, russian_roulette_min_bounces=1)
    yi = Interface()
    scenes.load_scene(yi, sc, rd)
    assert [int(t) for t in yi.getLights()[:, 0].view(np.int32)] == [0, 7, 9, 10]
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


def test_variant_choice(files, monkeypatch, capfd):
    monkeypatch.setenv("YAFGPU_VERBOSE", "1")
    kernel = lambda: re.findall(r"shading kernel: (\S+) \(", capfd.readouterr().err)
    capfd.readouterr()
    point = {"type": "pointlight", "from": (0.0, 0.0, 3.0), "color": (1.0, 1.0, 1.0), "power": 9.0}
    render(plane_scene([point]), res=16)
    without = kernel()
    for soft in (False, True):
        render(plane_scene([point, ies(files["C1"], soft_shadows=soft)]), res=16)
        assert set(kernel()) == {"ies"}
    assert without and "ies" not in without and "blend_ies" not in without
    render(plane_scene([point]), res=16)
    assert kernel() == without, "a scene without an IES light keeps the kernel it had"


# ---- the reference's compiled IesLight and IesData -----------------------------------------------------------------------
def test_leaf_functions_match_the_reference(files):
    """tests/golden/ref_spot_ies_ieee: what the reference's own IesData (parseIesFile, then getRadiance) and IesLight, made by its factory
    from the parameters stored there, gave on the seven files, each as a Dirac light and with soft_shadows.  All fourteen are the lights
    of one scene; getRadiance, illuminate and illumSample (probe ops 38, 39, 40) bit for bit on every row without a mark (a marked row's
    lookup lies at or beyond the last entry of an angle map, where the reference reads past its array: no fixture value); the flags
    against what light_is_dirac / light_can_intersect (yafgpu_shading.h) make of the type word getLights() shows"""
    import os
    from tests import pin_fixture as pin
    doc = pin.load("spot_ies", "ieee")
    names = doc["ies_sets"]
    d = os.path.dirname(files[NAMES[0]])
    yi = Interface()
    scenes.load_scene(yi, plane_scene([pin.params(doc, n, d) for n in names], res=8), scenes.render_settings(8, 8, 1, integrator="directlighting"))
    yi.prepareRender()
    rec = yi.getLights()
    assert rec.shape[0] == len(names) == 2 * len(NAMES)
    rows = 0

    def held(got, want, keep, what):
        assert keep.mean() >= 0.95, what
        exact(got[keep], want[keep], what)
        return int(keep.sum())

    for k, name in enumerate(names):
        dirac, can_intersect, n_samples = doc[name + "_flags3"]
        t, n = (int(x) for x in rec[k, :2].view(np.int32))
        assert t in (9, 10) and (dirac, can_intersect) == (int(t == 9), 0), name          # light_is_dirac; neither kind can be intersected
        assert n == (1 if dirac else n_samples), name
        file = os.path.splitext(doc[name + "_params"]["file"])[0]
        inp, want, keep = pin.leaf(doc, f"file_{file}", "radiance")
        o = yi.probe(38, np.hstack([inp, kbits(len(inp), k)]), 2)
        assert (o[:, 0] == 1).all()
        rows += held(o[:, 1:], want, keep, f"{name} getRadiance")
        for fn, op in (("illuminate", 39), ("illum_sample", 40)):
            inp, want, keep = pin.leaf(doc, name, fn)
            rows += held(yi.probe(op, np.hstack([inp, kbits(len(inp), k)]), want.shape[1]), want, keep, f"{name} {fn}")
    print(f"{rows} rows against the reference")
    assert rows >= 10000
