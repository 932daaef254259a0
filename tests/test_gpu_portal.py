"""The background portal light on the DEVICE: the row, area, triangle records and normals that scene set-up computes for its hidden mesh
and the two leaf functions (probe ops 35-37) bit for bit against the float32 restatements of tests/test_portal_host.py, which follow
light_background_portal.cc operation for operation, over a constant and over a texture background; renders against the estimator's
expectation by quadrature, against the same quad as a mesh light, with the power moved into the background, from behind the portal, with
shadows, beside a mesh light and a blend material; the serial-state replay with shards and pass pipelining; the film-preserving switches."""
import numpy as np
import pytest

from libyafaray_amd import Interface, scenes
from oracle import pyoracle as po
from tests.test_gpu_components import exact
from tests.test_gpu_ibl import bg_eval
from tests.test_gpu_lights import plane_points, plane_scene, render, stable
from tests.test_gpu_meshlight import (BOX, DIFFUSE, FAN_ZERO, MEASURED_EQUIVALENCE, MEASURED_EXPECTATION, N_FAN, QUAD2, RHO, SWITCHES, TRI, box, fan,
                                      kbits, mirror_quad, sample_points)
from tests.test_lights_host import F, W_COLOR, cross, dot
from tests.test_meshlight_host import W_AREA, W_COUNT, d_sample, iw, meshlight, pdf1d, total_area, tri_areas
from tests.test_meshlight_host import scene_with as meshlight_scene
from tests.test_portal_host import INVISIBLE, LAMP, TYPE_PORTAL, W_POWER, illum_sample, intersect, portal, scene_with

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def torch_first():
    """the emulated shard exchange hands device memory to torch: let torch open the GPU before the library does"""
    import torch
    torch.cuda.init()


# ---- the four meshes of the leaf tests: those of tests/test_gpu_meshlight.py, hidden ----
MESHES = [TRI, QUAD2, BOX, fan()]
GHOST = {"type": "shinydiffusemat", "color": (0.5, 0.5, 0.5), "visibility": "invisible"}
GHOST_TRI = 3                 # the box's triangle with the invisible material: intersect skips it, illumSample samples it
MAT_LAMP, MAT_GHOST = 1, 2    # material indices: the plane's is 0
VIS_INVISIBLE = 3


def texels_4x3():
    t = np.ones((3, 4, 4), np.float32)
    t[..., :3] = np.array([[(0.9, 0.2, 0.1), (0.1, 0.8, 0.3), (0.2, 0.3, 0.9), (0.7, 0.7, 0.1)],
                           [(0.05, 0.4, 0.6), (1.5, 1.2, 0.9), (0.3, 0.0, 0.5), (0.6, 0.1, 0.8)],
                           [(0.4, 0.9, 0.2), (0.0, 0.0, 0.0), (0.8, 0.5, 0.3), (0.2, 0.6, 0.7)]], np.float32)      # one black texel: the 1e-5 floor
    return t


BACKGROUNDS = {"constant": ({"type": "constant", "color": (0.3, 0.9, 0.6), "power": 1.7}, []),
               "texture": ({"type": "textureback", "texture": "env", "rotation": 37.0, "power": 1.3},
                           [dict(name="env", texels=texels_4x3(), interpolate="none")])}


def records(verts):
    """updateIntersectionCachedValues (triangle.h:197-207) and recNormal (:295-302) for (n, 3, 3) corners -> e1, e2, eps, normal"""
    a, b, c = verts[:, 0], verts[:, 1], verts[:, 2]
    e1, e2 = b - a, c - a
    longest = np.maximum(np.sqrt(dot(e1, e1)), np.sqrt(dot(e2, e2)))
    eps = (np.float64(F(0.1)) * 0.00005 * longest.astype(np.float64)).astype(np.float32)
    n = cross(e1, e2)
    ln = dot(n, n)
    with np.errstate(all="ignore"):
        inv = (F(1) / np.sqrt(ln)).astype(np.float32)
        n = np.where((ln != 0)[:, None], n * inv[:, None], n).astype(np.float32)      # (a triangle without area keeps its zero normal)
    return e1, e2, eps, n


@pytest.fixture(scope="module", params=sorted(BACKGROUNDS))
def leaf(request):
    """one scene with the four portals over one of the two backgrounds, prepared; per light the restatement's inputs, none of them read
    from the device: corners, records, normals, func_, cdf_, area_ all restated here"""
    bg, textures = BACKGROUNDS[request.param]
    lights = [portal(2 + k, power=1.5 + k) for k in range(len(MESHES))]
    sc = scene_with(MESHES, lights)
    sc["materials"] = sc["materials"] + [GHOST]
    sc["extra_meshes"][2]["material"] = [MAT_GHOST if t == GHOST_TRI else MAT_LAMP for t in range(len(BOX))]
    sc["textures"] = textures
    yi = Interface()
    scenes.load_scene(yi, sc, scenes.render_settings(8, 8, 1, integrator="directlighting", background=bg))
    yi.prepareRender()
    assert yi.getRenderStats().n_triangles == 2, "the portals' meshes add no triangle to the scene"
    rec = yi.getLights()
    bgrec = yi.getBackground("world_background")
    out = []
    for k, v in enumerate(MESHES):
        e1, e2, eps, n = records(v)
        mat = np.full(len(v), MAT_LAMP, np.uint32)
        if k == 2:
            mat[GHOST_TRI] = MAT_GHOST | (VIS_INVISIBLE << 30)
        func = tri_areas(v)
        out.append({"k": k, "rec": rec[k], "verts": v, "normals": n, "rows": [(v[t, 0], eps[t], e1[t], e2[t]) for t in range(len(v))],
                    "e1": e1, "e2": e2, "eps": eps, "mat": mat, "visible": (mat >> 30) < 2, "power": F(1.5 + k),
                    "func": func, "cdf": pdf1d(func)[0], "integral": pdf1d(func)[1], "area": total_area(func)})
    return yi, out, (lambda d: bg_eval(yi, bgrec, d))


def test_rows_records_and_areas(leaf):
    """BackgroundPortalLight::initIs on the device: func_ (Triangle::surfaceArea), cdf_ and integral_ (Pdf1D's constructor), area_; and the
    triangles' normals and records, which for this light exist nowhere else"""
    yi, lights, _ = leaf
    for L in lights:
        n = L["verts"].shape[0]
        assert (int(L["rec"][0].view(np.int32)), iw(L["rec"], W_COUNT)) == (TYPE_PORTAL, n) and L["rec"][W_POWER] == L["power"]
        o = yi.probe(37, kbits(1, L["k"]), 4 + 2 * n + 1 + 16 * n)[0]
        func, cdf, integral, area = L["func"], L["cdf"], L["integral"], L["area"]
        assert int(o[0].view(np.uint32)) == n
        with np.errstate(divide="ignore"):
            exact(o[1:4], np.array([area, integral, F(1) / integral], np.float32).view(np.uint32), f"light {L['k']}: area_, integral_, inv_integral_")
        exact(o[4:4 + n], func.view(np.uint32), f"light {L['k']}: func_")
        exact(o[4 + n:4 + 2 * n + 1], cdf.view(np.uint32), f"light {L['k']}: cdf_")
        assert L["rec"][W_AREA].view(np.uint32) == area.view(np.uint32), "getLights shows area_"
        ng = o[5 + 2 * n:5 + 6 * n].reshape(n, 4)
        exact(ng[:, :3], L["normals"].view(np.uint32), f"light {L['k']}: normals")
        assert not ng[:, 3].view(np.uint32).any()
        r = o[5 + 6 * n:].reshape(n, 12)
        want = np.zeros((n, 12), np.uint32)
        want[:, 0:3] = L["verts"][:, 0].view(np.uint32); want[:, 3] = L["eps"].view(np.uint32)
        want[:, 4:7] = L["e1"].view(np.uint32); want[:, 7] = L["mat"]
        want[:, 8:11] = L["e2"].view(np.uint32)
        exact(r, want, f"light {L['k']}: records")
    f = lights[3]["func"]
    assert f[FAN_ZERO[0]] == 0 and f[FAN_ZERO[1]] == 0 and f[f > 0].max() / f[f > 0].min() > 1e5
    c = lights[3]["cdf"]
    assert c[FAN_ZERO[0]] == c[FAN_ZERO[0] + 1] == c[FAN_ZERO[1] + 1] and c[-1] == 1


def test_illum_sample_bit_for_bit(leaf):
    yi, lights, sky = leaf
    rng = np.random.default_rng(11)
    N = 10000
    for L in lights:
        n, cdf = L["verts"].shape[0], L["cdf"]
        p = sample_points(rng, L, N)                                       # the first sixteen lie on the light
        s = rng.random((N, 2)).astype(np.float32)
        s[16:24, 0] = 0; s[24:32, 0] = 1
        s[32:232, 0] = cdf[rng.integers(0, n + 1, 200)]                    # s_1 exactly on entries of cdf_, the equal ones among them
        if n == N_FAN:
            s[232:240, 0] = cdf[FAN_ZERO[0]]; s[240:248, 0] = np.nextafter(cdf[FAN_ZERO[0]], F(2))
        s[248:256, 0] = np.nextafter(cdf[1], F(0)); s[256:264, 0] = min(np.nextafter(cdf[1], F(2)), F(1))      # both branches of the ss_1 remap, at their border
        want, prim = illum_sample(L["verts"], L["normals"], cdf, L["area"], L["power"], sky, p, s[:, 0], s[:, 1])
        got = yi.probe(35, np.hstack([p, s, kbits(N, L["k"])]), 9)
        exact(got, want.view(np.uint32), f"illumSample, light {L['k']}")
        share = want[:, 0].mean()
        print(f"light {L['k']}: {share:.3f} of the samples accepted")
        assert 0.1 < share < 0.9
        assert (prim < n).all() and (prim == 0).any() and (n == 1 or (prim > 0).any())
        if n == N_FAN:
            assert not np.isin(prim, FAN_ZERO).any(), "a triangle of zero area was chosen"
            assert len(np.unique(prim)) > 100
        if n == len(BOX):
            assert (want[prim == GHOST_TRI, 0] != 0).any(), "illumSample samples the triangle whose material is invisible, as the reference does"


def test_intersect_bit_for_bit(leaf):
    yi, lights, sky = leaf
    rng = np.random.default_rng(13)
    N = 10000
    for L in lights:
        v = L["verts"]
        frm = rng.uniform((-4, -4, 0), (4, 4, 5), (N, 3)).astype(np.float32)
        # aimed at and around the light: at the centroid of a triangle picked by area, off by a good part of the triangle's own size
        k = np.minimum(d_sample(L["cdf"], rng.random(N).astype(np.float32)), len(L["func"]) - 1)
        target = (v[k].mean(axis=1) + rng.normal(0, 1, (N, 3)) * (0.35 * np.sqrt(L["func"][k]))[:, None]).astype(np.float32)
        # rays through shared edges of coplanar neighbours: at a point of an edge of the triangle picked (in the quad and the fan that edge
        # is shared), and straight at corners
        w = rng.random(300).astype(np.float32)[:, None]
        target[:300] = v[k[:300], 0] * w + v[k[:300], 2] * (F(1) - w)
        target[300:400] = v[k[300:400], 1]
        d = target - frm
        d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
        tmin = np.full(N, 1e-4, np.float32)
        first, _, _ = intersect(L["rows"], L["visible"], L["normals"], L["area"], L["power"], sky, frm, d, tmin)
        # a third of the rays that hit start beyond the first face they met
        beyond = (first[:, 0] != 0) & (rng.random(N) < 0.33)
        tmin[beyond] = first[beyond, 1] + F(0.01)
        want, hit, brute = intersect(L["rows"], L["visible"], L["normals"], L["area"], L["power"], sky, frm, d, tmin)
        got = yi.probe(36, np.hstack([frm, d, tmin[:, None], kbits(N, L["k"])]), 6)
        exact(got, want.view(np.uint32), f"intersect, light {L['k']}")
        found = hit >= 0
        assert np.array_equal(np.where(found, brute, 0).view(np.uint32)[want[:, 0] != 0], got[:, 1].view(np.uint32)[want[:, 0] != 0]), "not the closest hit"
        share = found.mean()
        print(f"light {L['k']}: {share:.3f} of the rays hit, {want[:, 0].mean():.3f} accepted")
        assert 0.1 < share < 0.9
        if len(v) == len(BOX):
            assert not (hit == GHOST_TRI).any(), "the triangle whose material is invisible was hit"
            # ... and it would have been: with every triangle visible a good number of these rays meet it first
            _, hit_all, _ = intersect(L["rows"], np.ones(len(v), bool), L["normals"], L["area"], L["power"], sky, frm, d, tmin)
            assert (hit_all == GHOST_TRI).sum() > 50
            outside = (np.abs(frm - np.array([1.5, 1.5, 1.5], np.float32)) > 0.4).any(axis=1)
            back = found & outside & beyond & (dot(d, L["normals"][np.maximum(hit, 0)]) > 0)
            assert back.sum() > 100 and (want[back, 0] == 0).all(), "back faces refuse"


def test_sample_limit_still_holds():
    yi = Interface(strict=False)
    scenes.load_scene(yi, scene_with([TRI], [portal(2, samples=5000)]), scenes.render_settings(8, 8, 1, integrator="directlighting"))
    assert not yi.render() and "4095" in yi.getLastError()


# ---- renders ----
SIN30, COS30 = 0.5, float(np.cos(np.radians(30.0)))
SMOOTH_SKY = ({"type": "textureback", "texture": "env", "rotation": 37.0, "power": 1.3}, [dict(name="env", texels=texels_4x3(), interpolate="bilinear")])


def render_portal(sc, bg, textures=(), spp=1, res=64, **kw):
    sc["textures"] = list(textures)
    return render(sc, spp=spp, res=res, background=bg, **kw)


def expectation(yi, bgrec, quad, power, p, n=(0.0, 0.0, 1.0), G=384):
    """What one light sample returns ON AVERAGE at the diffuse point p with normal n, in float64: the area form of the direct-lighting
    integral over the quad, rho / pi * int bg_eval(w) * power * cos * cos' / d^2 dA, by G x G midpoint quadrature.  The MIS weights of the
    two halves sum to one wherever both are defined, so the pair's expectation is this integral.  Nothing here comes from the code under
    test but the texture lookup that tests/test_gpu_textures.py pins (through tests.test_gpu_ibl.bg_eval)"""
    corners = np.unique(quad.reshape(-1, 3).astype(np.float64), axis=0)
    assert len(corners) == 4
    a = corners[0]
    rest = sorted(corners[1:], key=lambda q: np.linalg.norm(q - a))
    b, d, c = rest                                   # the farthest from a is the opposite corner
    g = (np.arange(G) + 0.5) / G
    s, t = [x.ravel() for x in np.meshgrid(g, g)]
    ex, ey = b - a, d - a
    assert np.allclose(a + ex + ey, c), "a parallelogram"
    pts = a + s[:, None] * ex + t[:, None] * ey
    nl = np.cross(quad[0, 1] - quad[0, 0], quad[0, 2] - quad[0, 0]).astype(np.float64); area = np.linalg.norm(np.cross(ex, ey)); nl /= np.linalg.norm(nl)
    w = pts - np.asarray(p, np.float64)
    d2 = (w * w).sum(axis=1); w /= np.sqrt(d2)[:, None]
    cos_s = np.maximum(w @ np.asarray(n, np.float64), 0); cos_l = np.maximum(-(w @ nl), 0)
    L = bg_eval(yi, bgrec, w.astype(np.float32)).astype(np.float64) * float(power)
    return np.array(RHO) / np.pi * (L * (cos_s * cos_l / d2)[:, None]).mean(axis=0) * area


def test_frame_mean_matches_the_expectation_over_a_texture_background():
    """The mesh light's expectation test (64 x 64 pixels, 64 spp, 4 light samples, the quad 30 degrees off the plane's normal, a patch 0.01
    wide) with the quad as a portal over a bilinear 4 x 3 texture background, whose colour varies across the quad.  The margin is that
    test's, 20 * 1.26e-4.  Measured on the MI355X: see DESIGN.md, the portal's section."""
    res, spp, power = 64, 64, 3.0
    quad = mirror_quad()
    sc = scene_with([quad], [portal(2, power=power)], res=res, plane_mat=DIFFUSE)
    cam_from = tuple(200.0 * c for c in (-SIN30, 0.0, COS30))
    sc["camera"] = dict(sc["camera"], **{"from": cam_from, "up": (cam_from[0], 1.0, cam_from[2]), "focal": 20000.0})
    img, yi = render_portal(sc, *SMOOTH_SKY, spp=spp, res=res)
    bgrec = yi.getBackground("world_background")
    pp = plane_points(yi, res)
    assert np.abs(pp).max() < 0.01
    pts = (0.5 * (pp[15::32, 15::32] + pp[16::32, 16::32])).reshape(-1, 3)
    want = np.mean([expectation(yi, bgrec, quad, power, p) for p in pts], axis=0)
    coarse = np.mean([expectation(yi, bgrec, quad, power, p, G=192) for p in pts], axis=0)
    mean = img.reshape(-1, 3).mean(axis=0)
    dev = np.abs(mean / want - 1).max()
    print(f"frame mean {mean}, expectation {want}, largest relative deviation {dev:.3g}; quadrature at half the grid differs by {np.abs(coarse / want - 1).max():.3g}")
    spread = bg_eval(yi, bgrec, (quad.reshape(-1, 3) / np.linalg.norm(quad.reshape(-1, 3), axis=1, keepdims=True)).astype(np.float32))
    assert (spread.max(axis=0) / spread.min(axis=0)).max() > 1.05, "the background should vary across the quad"
    assert np.abs(coarse / want - 1).max() < 1e-5, "the quadrature has not converged"
    st = yi.getRenderStats()
    assert st.camera_samples * 4 <= st.rays_shadow <= st.camera_samples * 4 * 2
    assert dev < 20 * MEASURED_EXPECTATION["diffuse"]


def test_the_same_quad_as_a_one_sided_mesh_light_has_the_same_mean():
    """a constant background whose colour words are the getLights colour of a one-sided mesh light on the same quad, and power 1: every leaf
    operation of the portal then equals the mesh light's (the pdf differs only in the mesh light's guard against area * cos == 0).  Margin:
    that of tests.test_gpu_meshlight.test_the_same_quad_as_an_area_light_has_the_same_mean"""
    z = 8.0
    quad = scenes._quad((-0.5, -0.5, z), (-0.5, 0.5, z), (0.5, 0.5, z), (0.5, -0.5, z))                  # faces -z
    m, ym = render(meshlight_scene([quad], [meshlight(2, power=40.0)], res=100), spp=64, res=100)
    col = ym.getLights()[0][W_COLOR:W_COLOR + 3]
    p, yp = render_portal(scene_with([quad], [portal(2, power=1.0)], res=100), {"type": "constant", "color": tuple(float(c) for c in col), "power": 1.0},
                          spp=64, res=100)
    assert np.array_equal(yp.getBackground("world_background")["color"].view(np.uint32), col.view(np.uint32))
    assert ym.getLights()[0][W_AREA].view(np.uint32) == yp.getLights()[0][W_AREA].view(np.uint32)
    dev = abs(p.mean() / m.mean() - 1)
    equal = (p == m).all(axis=-1).mean()
    print(f"mesh light mean {m.mean():.8g}, portal mean {p.mean():.8g}, relative difference {dev:.3g}; {100 * equal:.2f} % of the pixels are bit-equal")
    assert m.mean() > 0.01
    assert dev < 20 * MEASURED_EQUIVALENCE


def film_of(sc, bg, textures=(), spp=2, res=32, **kw):
    sc["textures"] = list(textures)
    yi = Interface()
    scenes.load_scene(yi, sc, scenes.render_settings(res, res, spp, integrator="directlighting", background=bg, **kw))
    yi.render()
    return yi.getFilm(res, res).copy(), yi


def test_power_scales_like_the_background():
    """background (0.5, 0.25, 1) under power 2 is background (1, 0.5, 2) under power 1, exactly; the view never sees the background"""
    quad = scenes._quad((-0.5, -0.5, 8.0), (-0.5, 0.5, 8.0), (0.5, 0.5, 8.0), (0.5, -0.5, 8.0))
    a, _ = film_of(scene_with([quad], [portal(2, power=2.0)], res=32), {"type": "constant", "color": (0.5, 0.25, 1.0)})
    b, _ = film_of(scene_with([quad], [portal(2, power=1.0)], res=32), {"type": "constant", "color": (1.0, 0.5, 2.0)})
    assert a[..., :3].min() > 0
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_a_camera_behind_the_portal_sees_through_it():
    """from the room through the window, with nothing outside: the film of the scene without the light and its mesh, because the mesh is
    not there"""
    quad = scenes._quad((-0.5, -0.5, 2.0), (-0.5, 0.5, 2.0), (0.5, 0.5, 2.0), (0.5, -0.5, 2.0))
    up = {"from": (0.0, 0.0, 1.0), "to": (0.0, 0.0, 5.0), "up": (0.0, 1.0, 1.0)}
    bg, textures = BACKGROUNDS["texture"]
    with_ = scene_with([quad], [portal(2)], res=32)
    with_["camera"] = dict(with_["camera"], **up)
    without = plane_scene([], res=32)
    without["camera"] = dict(without["camera"], **up)
    a, ya = film_of(with_, bg, textures)
    b, yb = film_of(without, bg, textures)
    assert ya.getRenderStats().n_triangles == yb.getRenderStats().n_triangles == 2
    assert a[..., :3].min() > 0 and len(np.unique(a[..., 0])) > 1, "the background, more than one texel of it"
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_shadows():
    """the mesh light's shadow test with the quad as a portal: the light off to the side at (6, 0, 8), an occluder half way on the line to
    the origin, whose umbra on the plane is |x|, |y| < 1.5"""
    quad = scenes._quad((5.5, -0.5, 8.0), (5.5, 0.5, 8.0), (6.5, 0.5, 8.0), (6.5, -0.5, 8.0))             # faces -z
    occ = scenes._quad((2.0, -1.0, 4.0), (4.0, -1.0, 4.0), (4.0, 1.0, 4.0), (2.0, 1.0, 4.0))
    grey = {"type": "shinydiffusemat", "color": (0.5, 0.5, 0.5)}
    sky = {"type": "constant", "color": (100.0, 90.0, 80.0)}
    open_, _ = render_portal(scene_with([quad], [portal(2)], res=64), sky, spp=4)
    shad, ys = render_portal(scene_with([quad], [portal(2)], res=64, extra=[(occ, grey)]), sky, spp=4)
    pts = plane_points(ys, 64)
    umbra = (np.abs(pts[..., 0]) < 1.5) & (np.abs(pts[..., 1]) < 1.5)
    keep = stable(umbra)
    assert (umbra & keep).sum() > 500 and (open_ > 0).all()
    assert (shad[umbra & keep] == 0).all(), "the umbra must be exactly black"
    off, _ = render_portal(scene_with([quad], [portal(2, cast_shadows=False)], res=64, extra=[(occ, grey)]), sky, spp=4)
    assert np.array_equal(off, open_), "cast_shadows = false gives the unoccluded film"


def test_a_portal_beside_a_mesh_light_and_a_blend_material():
    """a scene with both lights and a blend material in use picks a kernel that has all three, and each light shows in the film"""
    window = scenes._quad((-2.5, -0.5, 6.0), (-2.5, 0.5, 6.0), (-1.5, 0.5, 6.0), (-1.5, -0.5, 6.0))
    lamp = scenes._quad((1.5, -0.5, 6.0), (1.5, 0.5, 6.0), (2.5, 0.5, 6.0), (2.5, -0.5, 6.0))
    sky = {"type": "constant", "color": (30.0, 40.0, 60.0)}

    def film(lights):
        sc = plane_scene(lights, res=32)
        # (a blend's two materials exist before it: load_scene creates materials in list order, as mat0, mat1, ...)
        sc["materials"] = [{"type": "shinydiffusemat", "color": (0.8, 0.15, 0.1), "diffuse_reflect": 0.9},
                           {"type": "glossy", "color": (0.9, 0.85, 0.8), "diffuse_color": (0.5, 0.4, 0.6), "diffuse_reflect": 0.4, "glossy_reflect": 0.6,
                            "exponent": 40.0, "as_diffuse": False},
                           {"type": "blend_mat", "material1": "mat0", "material2": "mat1", "blend_value": 0.3}, LAMP]
        sc["tri_mat"] = np.full_like(sc["tri_mat"], 2)
        sc["extra_meshes"] = [{"verts": window, "material": 3, "type": INVISIBLE}, {"verts": lamp, "material": 3}]
        return film_of(sc, sky, spp=4)

    both, yi = film([portal(2, power=1.0), meshlight(3, power=30.0)])
    assert sorted(int(t) for t in yi.getLights()[:, 0].view(np.int32)) == [7, TYPE_PORTAL]
    assert np.isfinite(both).all() and both[..., :3].min() > 0
    only_lamp, _ = film([meshlight(3, power=30.0)])
    only_window, _ = film([portal(2, power=1.0)])
    assert not np.array_equal(both, only_lamp) and not np.array_equal(both, only_window)
    left, right = both[:, :8, :3].mean(), both[:, -8:, :3].mean()
    assert only_lamp[:, :8, :3].mean() < left and only_window[:, -8:, :3].mean() < right, "each light adds to the side it hangs over"


# ---- serial-state replay, shards, pass pipelining; the switches: the mesh light file's scene at its size, the box hidden as a portal ----
SOUP_SKY = {"type": "constant", "color": (6.0, 5.4, 4.8)}


def soup_with_a_box_portal(res=96):
    sc = scenes.cornell_soup(1500, seed=41, res=(res, res))
    sc["materials"] = sc["materials"] + [LAMP]
    sc["extra_meshes"] = [{"verts": box((0.4, -0.2, 0.2), 0.12), "material": len(sc["materials"]) - 1, "type": INVISIBLE}]
    sc["lights"] = sc["lights"] + [portal(2, power=1.0, samples=2)]
    sc["camera"] = dict(sc["camera"], resx=res, resy=res)
    return sc


def test_replay_shards_and_pipelining_with_a_portal():
    """tests.test_gpu_meshlight.test_replay_shards_and_pipelining_with_a_mesh_light with the box as a portal: two lights, so the path
    tracer's light choice is the reference's serial counter, carried across the shards"""
    import torch
    from libyafaray_amd.parallel import _DeviceFloats
    W = H = 96; T = 32; WORLD = 2
    sc = soup_with_a_box_portal(W)
    rd = scenes.render_settings(W, H, 4, bounces=4, tile_size=T, russian_roulette_min_bounces=1, background=SOUP_SKY)
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
    films = []
    for mode in (0, 1):
        y2 = Interface()
        scenes.load_scene(y2, sc, dict(rd, AA_passes=3, AA_inc_samples=2, AA_threshold=0.0))
        y2.setSerialReplay(False)
        y2.setPassPipelining(mode)
        y2.render()
        films.append(y2.getFilm(W, H).copy())
    assert np.array_equal(films[0], films[1])
    # the portal shows: without it the film is another
    y3 = Interface()
    scenes.load_scene(y3, dict(sc, lights=sc["lights"][:-1], extra_meshes=[]), rd)
    y3.setSerialReplay(True)
    y3.render()
    assert not np.array_equal(y3.getFilm(W, H), full)


@pytest.fixture(scope="module")
def switch_scene():
    W = 48
    yi = Interface()
    scenes.load_scene(yi, soup_with_a_box_portal(W), scenes.render_settings(W, W, 2, bounces=3, tile_size=16, russian_roulette_min_bounces=1, background=SOUP_SKY))
    yi.setSerialReplay(True)
    yi.render()
    st = yi.getRenderStats()
    return yi, yi.getFilm(W, W).copy(), (st.rays_closest, st.rays_shadow)


@pytest.mark.parametrize("switch", SWITCHES)
def test_film_preserving_switches(switch_scene, switch, monkeypatch):
    yi, film, rays = switch_scene
    monkeypatch.setenv(switch, "0")
    yi.render()
    st = yi.getRenderStats()
    assert (st.rays_closest, st.rays_shadow) == rays
    assert np.array_equal(yi.getFilm(48, 48).view(np.uint32), film.view(np.uint32)), f"{switch}=0 renders another film"
