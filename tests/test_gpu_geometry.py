"""The two functions every ray goes through, held to float64 references written from their definitions (tests/geometry_fixture.py):
Triangle::intersect — tri_test and tri_test_flat through probe op 29, and as wf_trace runs it under intersectRays / shadowRays, on the
trees of both builders — and Triangle::getSurface — get_surface, tex_point and tex_point_derivatives through probe op 30.

Nothing here is compared with the oracle: the float64 reference decides where it can (a verdict whose margin exceeds the derived band
K U S), the band marks what float32 cannot decide, and tests/test_geometry_host.py holds, without a GPU, the caps that keep the band
from hiding a failure, the floors on decided hits and misses, and the list of misreadings these inputs catch."""
import numpy as np
import pytest

from libyafaray_amd import Interface, scenes
from tests import geometry_fixture as gf
from tests.test_geometry_host import CASES, IDS, check_pairs, check_rays, check_surface

pytestmark = pytest.mark.gpu

F = np.float32


def bits(i):
    return np.asarray(i, np.uint32).view(F)


def device_scene(monkeypatch, verts, builder):
    monkeypatch.setenv("YAFGPU_BUILD", builder)
    yi = Interface()
    scenes.load_scene(yi, gf.scene_of(verts), scenes.render_settings(8, 8, 1))
    yi.prepareRender()
    assert yi.getRenderStats().kd_nodes >= 1
    return yi


@pytest.mark.parametrize("ci", CASES, ids=IDS)
def test_triangle_test_pairs(monkeypatch, ci):
    """op 29, every ray against the triangle it was placed at: tri_test and tri_test_flat answer alike bit for bit, meet every decided
    float64 verdict, and keep t, u, v inside the bands"""
    case = gf.all_cases()[ci]
    yi = device_scene(monkeypatch, case.verts, "host")
    out = yi.probe(29, np.column_stack([bits(case.target), case.rays[:, :6]]), 8)
    ok, ok_flat = out[:, 0] == 1, out[:, 4] == 1
    assert np.isin(out[:, [0, 4]], (0, 1)).all() and np.array_equal(ok, ok_flat), "tri_test and tri_test_flat: another verdict"
    assert np.array_equal(out[ok, 1:4].view(np.uint32), out[ok, 5:8].view(np.uint32)), "tri_test and tri_test_flat: t, u, v of an accepted pair differ"
    assert not out[~ok, 1:4].any()
    assert ok.any() and ((~ok).any() or case.name == "ranges")      # (the ranges' pairs are hits by construction: the range is the ray's)
    check_pairs("tri_test", case, gf.decided_pairs(ci), ok, out[:, 1], out[:, 2], out[:, 3])
    none = yi.probe(29, np.column_stack([bits([len(case.verts), 0xffffffff]), case.rays[:2, :6]]), 8)
    assert not none.any(), "an index outside the scene leaves zeros"


@pytest.mark.parametrize("builder", ["host", "device"])
@pytest.mark.parametrize("ci", CASES, ids=IDS)
def test_rays_through_wf_trace(monkeypatch, ci, builder):
    """intersectRays and shadowRays: every decided closest ray returns the float64 triangle with t and barycentrics in band, every
    decided miss -1, every decided shadow verdict the float64 one"""
    case = gf.all_cases()[ci]
    yi = device_scene(monkeypatch, case.verts, builder)
    tri, t, bary = yi.intersectRays(case.rays)
    shadow_rows = np.nonzero(case.rays[:, 6] == 0)[0]
    occluded = np.zeros(len(case.rays), bool)
    occluded[shadow_rows] = yi.shadowRays(case.rays[shadow_rows]) != 0
    assert ((tri >= -1) & (tri < len(case.verts))).all()
    hit = tri >= 0
    assert not t[~hit].any() and not bary[~hit].any()
    assert np.allclose(bary[hit].sum(axis=1), 1, rtol=0, atol=8 * gf.U), "b_0 = 1 - u - v: two roundings, and two more to add them up here"
    check_rays(f"wf_trace, {builder} tree", case, gf.decided(ci), tri, t, bary[:, 1], bary[:, 2], occluded)


# ---- the surface point -----------------------------------------------------------------------------------------------
TEXEL = (0.5, 0.25, 0.75, 1.0)
_layer = dict(type="layer", mode=0, def_val=1.0, upper_value=0.0)
PLAIN = {"type": "shinydiffusemat", "color": (0.7, 0.7, 0.7), "diffuse_reflect": 1.0}
BUMPED = {"type": "shinydiffusemat", "color": (0.8, 0.8, 0.8), "diffuse_reflect": 0.9, "diffuse_shader": "diff", "bump_shader": "bmp",
          "nodes": [dict(_layer, name="diff", input="map", colfac=1.0, def_col=(1.0, 0.0, 1.0, 1.0), do_color=True, do_scalar=False, color_input=True,
                         upper_color=(0.8, 0.8, 0.8, 1.0)),
                    dict(name="map", type="texture_mapper", texture="t_flat", texco="uv", mapping="plain"),
                    dict(_layer, name="bmp", input="bmap", valfac=1.0, do_color=False, do_scalar=True, color_input=False),
                    dict(name="bmap", type="texture_mapper", texture="t_flat", texco="uv", mapping="plain", bump_strength=2.0)]}
FLAT_TEXTURE = dict(name="t_flat", texels=np.broadcast_to(np.array(TEXEL, F), (4, 4, 4)).copy(), interpolate="none", clipping="repeat", color_space="LinearRGB")


def surface_device_scene():
    """the fixture's three meshes through the Interface, in object order: the smooth mesh (addNormal at the corners that have a normal),
    the mesh with UVs and orco under the bump-mapped material, the plain mesh"""
    sc, _ = gf.surface_scene()
    (s0, e0), (s1, e1), (s2, e2) = sc["meshes"]
    first = dict(gf.scene_of(sc["verts"][s0:e0]), vnormals=sc["vn"][s0:e0], materials=[dict(PLAIN), BUMPED, dict(PLAIN, color=(0.2, 0.3, 0.8))], textures=[FLAT_TEXTURE])
    rd = scenes.render_settings(8, 8, 1)
    yi = Interface()
    handles = scenes.load_scene(yi, first, rd)
    fl = lambda row: [float(x) for x in row]
    yi.startGeometry()
    yi.startTriMesh(yi.getNextFreeId(), 3 * (e1 - s1), e1 - s1, True, True, 0)
    for k in range(s1, e1):
        base = 3 * (k - s1)
        for c in range(3):
            yi.addVertexWithOrco(*fl(sc["verts"][k, c]), *fl(sc["orco"][k, c]))
            yi.addUv(*fl(sc["uv"][k, c]))
        yi.addTriangleWithUv(base, base + 1, base + 2, base, base + 1, base + 2, handles[1])
    yi.endTriMesh()
    yi.startTriMesh(yi.getNextFreeId(), 3 * (e2 - s2), e2 - s2, False, False, 0)
    for k in range(s2, e2):
        for c in range(3):
            yi.addVertex(*fl(sc["verts"][k, c]))
        yi.addTriangle(3 * (k - s2), 3 * (k - s2) + 1, 3 * (k - s2) + 2, handles[2])
    yi.endTriMesh()
    yi.endGeometry()
    scenes.set_render_params(yi, rd)
    yi.prepareRender()
    return yi


def test_surface_points():
    """op 30 at the corners, the edge midpoints, on bu + bv = 1 and inside every triangle of three meshes: every output within its band of
    the float64 surface point, exact where the answer is exact, has_uv and the material index equal"""
    sc, (tri, bu, bv, p) = gf.surface_scene()
    yi = surface_device_scene()
    rows = yi.probe(28, bits(np.arange(len(sc["verts"])))[:, None], 44)
    assert np.array_equal(rows[:, :3], sc["verts"][:, 0]) and (rows[:, 43].view(np.uint32) == 7).all(), "the device holds the fixture's triangles in the fixture's order, with normals, UVs and orco arrays"
    out = yi.probe(30, np.column_stack([bits(tri), bu, bv, p]), 28)
    got = dict(n=out[:, 0:3], ng=out[:, 3:6], nu=out[:, 6:9], nv=out[:, 9:12], mat=out[:, 12].view(np.uint32), orco_p=out[:, 13:16], orco_ng=out[:, 16:19],
               uv=out[:, 19:21], has_uv=out[:, 21] != 0, ds_du=out[:, 22:25], ds_dv=out[:, 25:28])
    assert np.isin(out[:, 21], (0, 1)).all()
    check_surface("device", got)
    mid = (tri == gf.OPPOSED) & (bu == 0.5) & (bv == 0.5)
    assert not got["n"][mid].any() and np.array_equal(got["nu"][mid][0], [1, 0, 0]) and np.array_equal(got["nv"][mid][0], [0, 1, 0])
    none = yi.probe(30, np.column_stack([bits([len(sc["verts"]), 0xffffffff]), bu[:2], bv[:2], p[:2]]), 28)
    assert not none.any(), "an index outside the scene leaves zeros"


def test_surface_point_without_bump_data():
    """a scene without a bump shader has no dPdU / dPdV data: op 30 leaves those six words zero, and everything else as it is"""
    case = gf.all_cases()[3]
    yi = Interface()
    scenes.load_scene(yi, gf.scene_of(case.verts), scenes.render_settings(8, 8, 1))
    yi.prepareRender()
    n = len(case.verts)
    p = case.verts[:, 0]
    out = yi.probe(30, np.column_stack([bits(np.arange(n)), np.full(n, 0.25, F), np.full(n, 0.5, F), p]), 28)
    assert not out[:, 22:].any() and not out[:, 19:22].any() and np.array_equal(out[:, 13:16], p) and np.array_equal(out[:, 16:19], out[:, 3:6])
    assert np.array_equal(out[:, 0:3], out[:, 3:6]) and (out[:, 12].view(np.uint32) == 0).all()
