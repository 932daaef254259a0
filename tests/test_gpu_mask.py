"""The mask material on the DEVICE (MaskMaterial, material_mask.cc): a shader node's scalar picks one of two materials at every hit.

The oracle does not know mask_mat, so the material is held to equivalences and to a float32 restatement of its selection, not to the
reference's compiled material_mask.cc: a masked scene must give the film of a plain scene whose triangles (or pixels) carry the
material the mask picks there.  Paired renders run in one process with the libc stream pinned (setRandState), the same number of
materials created in the same order, and a node material in the plain scene too, so that both take the general shading kernel: the
arithmetic per path is then the same, "equal" means np.array_equal of the films, and the ray counts agree."""
import re

import numpy as np
import pytest

from libyafaray_amd import Interface, scenes
from oracle import pyoracle as po
from tests.test_gpu_ao import CLAY, FLAT_TEXTURE, NODE_MATERIAL, POINT, clay_scene, settings
from tests.test_gpu_components import exact

pytestmark = pytest.mark.gpu

F = np.float32
W = Interface.MATERIAL_FIELDS
RES = (24, 16)


@pytest.fixture(scope="module", autouse=True)
def torch_first():
    """(as in the other GPU modules: let torch open the GPU before the library does)"""
    import torch
    torch.cuda.init()


# ---- scenes ----------------------------------------------------------------------------------------------------------
RED = {"type": "shinydiffusemat", "color": (0.8, 0.15, 0.1), "diffuse_reflect": 1.0}
BLUE = {"type": "shinydiffusemat", "color": (0.1, 0.2, 0.8), "diffuse_reflect": 0.8}
MIRROR = {"type": "mirror", "color": (0.9, 0.9, 1.0), "reflect": 0.8}
GLASS = {"type": "glass", "IOR": 1.45, "filter_color": (0.8, 1.0, 0.85), "transmit_filter": 0.9, "mirror_color": (1.0, 1.0, 1.0)}
TINTED = {"type": "shinydiffusemat", "color": (0.2, 0.8, 0.3), "diffuse_reflect": 1.0, "transparency": 0.7, "transmit_filter": 1.0}
# what stands where the mask stands, in a plain scene: a material with a node of its own that no triangle uses
SPARE = {"type": "shinydiffusemat", "color": (0.5, 0.5, 0.5), "diffuse_reflect": 1.0, "diffuse_shader": "c",
         "nodes": [dict(name="c", type="value", color=(0.3, 0.6, 0.9, 1.0))]}
TWO_TEXELS = dict(name="t_mask", texels=np.array([[[0.2, 0.2, 0.2, 1.0], [0.9, 0.9, 0.9, 1.0]]], F), interpolate="none", clipping="repeat", color_space="LinearRGB")
MAPPER = dict(name="mk", type="texture_mapper", texture="t_mask", texco="uv", mapping="plain")
PICK = np.array([0, 1, 1, 0, 1, 0, 0, 1, 1, 0, 1, 0], np.int32)      # which material the mask picks on each of the clay scene's 12 triangles


def mask_mat(nodes=(MAPPER,), mask="mk", material1="mat0", material2="mat1", **kw):
    return dict({"type": "mask_mat", "material1": material1, "material2": material2, "mask": mask, "nodes": list(nodes)}, **kw)


def value_mask(v, **kw):
    return mask_mat(nodes=(dict(name="mk", type="value", scalar=float(v)),), **kw)


def texel_uv(pick):
    """UVs that put every corner of triangle k at the centre of texel pick[k] of a two-texel row"""
    uv = np.zeros((len(pick), 3, 2), F)
    uv[..., 0] = (0.25 + 0.5 * np.asarray(pick, F))[:, None]
    uv[..., 1] = 0.5
    return uv


def scene(materials, tri_mat, uv=None, textures=(), extra=(), **kw):
    g = clay_scene(lights=[POINT], extra=[(v, CLAY) for v in extra], **kw)
    sc = dict(g, materials=list(materials), tri_mat=np.asarray(tri_mat, np.int32))
    assert len(sc["tri_mat"]) == len(sc["verts"])
    if uv is not None:
        sc["uv"] = uv
    if textures:
        sc["textures"] = list(textures)
    return sc


def pair(sub1, sub2, plain1=None, plain2=None, pick=PICK, textures=(TWO_TEXELS,), **mask_kw):
    """(masked scene, plain scene): every triangle on a mask of sub1 / sub2 that the texel under it decides, against the triangles on
    the materials themselves (plain1 / plain2 where the plain scene's differ)"""
    uv = texel_uv(pick)
    masked = scene([sub1, sub2, mask_mat(**mask_kw)], np.full(len(pick), 2), uv, textures)
    plain = scene([plain1 or sub1, plain2 or sub2, SPARE], pick, uv, textures)
    return masked, plain


def device(sc, rd, shard=None, replay=None):
    yi = Interface()
    scenes.load_scene(yi, sc, rd)
    yi.setRandState(20240, 3)
    if replay is not None:
        yi.setSerialReplay(replay)
    if shard:
        yi.setShard(*shard)
    yi.render()
    return yi.getFilm(rd["width"], rd["height"]), yi


def same(a, b, what, rays=True):
    (fa, ya), (fb, yb) = a, b
    assert fa[..., 4].all() and fa[..., :3].any()
    diff = float(np.abs(fa - fb).max())
    print(f"{what}: largest film difference {diff:.3g}")
    assert np.array_equal(fa, fb), f"{what}: films differ by up to {diff}"
    if rays:
        sa, sb = ya.getRenderStats(), yb.getRenderStats()
        assert (sa.rays_closest, sa.rays_shadow) == (sb.rays_closest, sb.rays_shadow), what


def primary_hits(sc, rd):
    """the camera ray through every pixel centre (one sample per pixel) and what it hits, from the oracle on the CPU:
    (h, w) triangle index or -1, (h, w, 3) barycentrics b_0 b_1 b_2, (h, w, 3) hit point"""
    import ctypes as C
    bare = {k: v for k, v in sc.items() if k not in ("uv", "textures")}      # geometry and camera are all that is asked of the oracle here
    osc, cam = po.OracleScene(dict(bare, materials=[CLAY] * len(sc["materials"]))), po.camera_desc(sc["camera"])
    h, w = rd["height"], rd["width"]
    tri, bary, pt = np.full((h, w), -1, np.int32), np.zeros((h, w, 3), F), np.zeros((h, w, 3), F)
    out9 = np.zeros(9, F)
    for y in range(h):
        for x in range(w):
            po.lib().yor_camera_shoot(C.byref(cam), F(F(x) + F(0.5)), F(F(y) + F(0.5)), po.fptr(out9))
            hit, k, t, b = osc.intersect(out9[0:3], out9[3:6], float(out9[6]), float(out9[7]), use_tree=False)
            if hit:
                tri[y, x], bary[y, x], pt[y, x] = k, b, (out9[0:3] + (out9[3:6] * F(t)).astype(F)).astype(F)
    return tri, bary, pt


def probe27(yi, mat, tri, bu, bv, p, n):
    """-> mask scalar, choice under threshold_, choice under 0.5, the material index the vertex gets"""
    k = len(tri)
    x = np.hstack([np.full((k, 1), np.uint32(mat)).view(F), np.asarray(tri, np.uint32).reshape(k, 1).view(F), np.asarray(bu, F).reshape(k, 1),
                   np.asarray(bv, F).reshape(k, 1), np.asarray(p, F).reshape(k, 3), np.asarray(n, F).reshape(k, 3), np.asarray(n, F).reshape(k, 3)])
    o = yi.probe(27, x, 4)
    return o[:, 0], o[:, 1], o[:, 2], o[:, 3].view(np.uint32)


# ---- 1. the selection, bit for bit -------------------------------------------------------------------------------------
@pytest.mark.parametrize("interpolate", ["bilinear", "none"])
def test_probe_selection_bit_for_bit(interpolate):
    """probe 27 on 2000 points of a triangle under a random 16 x 12 texture: the scalar is the node probe's (op 14) for the same graph
    at the same point, both choices are float comparisons of it, and the vertex gets the clone that goes with the first"""
    N, THRESHOLD = 2000, 0.62
    rng = np.random.default_rng(27)
    tex = dict(name="t_mask", texels=np.concatenate([rng.random((12, 16, 3)), np.ones((12, 16, 1))], axis=2).astype(F), interpolate=interpolate,
               clipping="repeat", color_space="LinearRGB")
    nodes = (dict(type="layer", name="top", input="mk", mode=0, do_color=False, do_scalar=True, color_input=False, def_val=1.0, upper_value=0.0, valfac=1.0), MAPPER)
    tri = np.array([[[0, 0, 0], [1.5, 0.1, 0], [0.2, 1.2, 0]]], F)
    uv = np.array([[[0.07, 0.11], [1.31, 0.23], [0.19, 0.93]]], F)          # reaches past 1: the repeat is part of the graph
    sc = {"verts": tri, "tri_mat": np.array([2], np.int32), "vnormals": None, "materials": [RED, BLUE, mask_mat(nodes=nodes, mask="top", threshold=THRESHOLD)],
          "uv": uv, "textures": [tex], "lights": [], "camera": {"type": "perspective", "from": (0.5, 0.5, 5.0), "to": (0.5, 0.5, 0.0), "up": (0.5, 1.5, 5.0), "resx": 8, "resy": 8}}
    yi = Interface()
    scenes.load_scene(yi, sc, settings((8, 8)))
    yi.prepareRender()
    table = yi.getMaterialTable()
    first, count, slot = (int(table[2, W[k]]) for k in ("node_first", "n_nodes", "sh_diffuse"))
    clones = table[2, W["c_index"]:W["c_index"] + 2]
    assert (count, slot, list(clones)) == (2, 1, [3, 4])
    b = rng.random((N, 2)).astype(F)
    b[b.sum(axis=1) > 1] = (F(1) - b[b.sum(axis=1) > 1]).astype(F)
    bu, bv = b[:, 0], b[:, 1]
    w0 = ((F(1) - bu).astype(F) - bv).astype(F)                              # Triangle::getSurface, triangle.cc:34, :66-67
    p = (w0[:, None] * tri[0, 0] + bu[:, None] * tri[0, 1] + bv[:, None] * tri[0, 2]).astype(F)
    n = np.broadcast_to(np.array([0, 0, 1], F), (N, 3))
    u = (((w0 * uv[0, 0, 0]).astype(F) + (bu * uv[0, 1, 0]).astype(F)).astype(F) + (bv * uv[0, 2, 0]).astype(F)).astype(F)
    v = (((w0 * uv[0, 0, 1]).astype(F) + (bu * uv[0, 1, 1]).astype(F)).astype(F) + (bv * uv[0, 2, 1]).astype(F)).astype(F)
    val, by_threshold, by_half, index = probe27(yi, 2, np.zeros(N, np.uint32), bu, bv, p, n)
    x14 = np.hstack([p, n, n, p, n, u[:, None], v[:, None], np.zeros((N, 1), F), np.full((N, 1), np.uint32(first)).view(F), np.full((N, 1), np.uint32(count)).view(F)])
    want = yi.probe(14, x14, 5 * count)[:, 5 * slot + 4]
    assert 0.05 < want.min() < 0.3 and 0.8 < want.max() < 1.0 and len(np.unique(want)) > (N // 2 if interpolate == "bilinear" else 50)
    exact(val, want.view(np.uint32), f"mask scalar, {interpolate}")
    assert np.array_equal(by_threshold, (want > F(THRESHOLD)).astype(F)) and np.array_equal(by_half, (want > F(0.5)).astype(F))
    assert np.array_equal(index, clones[(want > F(THRESHOLD)).astype(int)].astype(np.uint32))
    both = np.stack([by_threshold, by_half], axis=1)
    for case in ([0, 0], [0, 1], [1, 1]):                                      # below both, between 0.5 and the threshold, above both
        assert (both == case).all(axis=1).sum() >= 60, case
    # a material that is no mask keeps its index and leaves the other three outputs at zero
    o = yi.probe(27, np.hstack([np.zeros((4, 2), F), b[:4], p[:4], n[:4], n[:4]]), 4)
    assert (o[:, :3] == 0).all() and (o[:, 3].view(np.uint32) == 0).all()


# ---- 2. constant per triangle ------------------------------------------------------------------------------------------
CASES = {
    "directlighting, 2 spp": dict(spp=2),
    "pathtracing, 3 bounces, roulette, serial replay": dict(spp=2, integrator="pathtracing", bounces=3, russian_roulette_min_bounces=1),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_constant_per_triangle_equals_the_plain_scene(case):
    masked, plain = pair(RED, BLUE)
    rd = settings(RES, **CASES[case])
    replay = True if "replay" in case else None
    same(device(masked, rd, replay=replay), device(plain, rd, replay=replay), case)


def test_constant_per_triangle_with_vertex_records_in_memory(monkeypatch):
    monkeypatch.setenv("YAFGPU_VERTEX_LDS", "0")
    masked, plain = pair(RED, BLUE)
    rd = settings(RES, spp=2, integrator="pathtracing", bounces=3, russian_roulette_min_bounces=1)
    same(device(masked, rd, replay=True), device(plain, rd, replay=True), "YAFGPU_VERTEX_LDS=0")


def test_the_mask_really_picks():
    """the equalities above are not those of a mask that always picks one side: swapping material1 and material2 changes the film"""
    masked, _ = pair(RED, BLUE)
    swapped, _ = pair(RED, BLUE, material1="mat1", material2="mat0")
    rd = settings(RES)
    a, b = device(masked, rd)[0], device(swapped, rd)[0]
    assert (np.abs(a - b)[..., :3].max(axis=-1) > 1e-3).mean() > 0.3


# ---- 3. varying inside triangles ---------------------------------------------------------------------------------------
def test_varying_inside_triangles_pixel_by_pixel():
    """an 8 x 8 checker of the values 0.2 and 0.9 over the plane, one sample per pixel: every pixel is film A's (all material1) or
    film B's (all material2), by the mask value at the camera ray's hit — the hit from the oracle's intersect, the value from probe 27"""
    T = 8
    checker = np.where((np.add.outer(np.arange(T), np.arange(T)) % 2 == 0)[..., None], F(0.2), F(0.9)) * np.ones(4, F)
    checker[..., 3] = 1
    tex = dict(name="t_mask", texels=checker.astype(F), interpolate="none", clipping="repeat", color_space="LinearRGB")
    g = clay_scene(lights=[POINT])
    xy = np.asarray(g["verts"], F).reshape(-1, 3, 3)[..., :2]
    uv = ((xy + F(2)) / F(4) * np.array([0.913, 0.877], F) + np.array([0.0437, 0.0611], F)).astype(F)      # the plane spans 7.3 x 7.0 texels, off the texel grid
    on_plane = [2, 2] + [0] * 10
    masked = scene([RED, BLUE, mask_mat()], on_plane, uv, [tex])
    film_a = scene([RED, BLUE, SPARE], [0, 0] + [0] * 10, uv, [tex])
    film_b = scene([RED, BLUE, SPARE], [1, 1] + [0] * 10, uv, [tex])
    rd = settings(RES)
    (fm, yi), (fa, _), (fb, _) = device(masked, rd), device(film_a, rd), device(film_b, rd)
    tri, bary, pt = primary_hits(film_a, rd)
    hit = (tri == 0) | (tri == 1)
    assert hit.mean() > 0.5
    ys, xs = np.nonzero(hit)
    k, b = tri[ys, xs], bary[ys, xs]
    val, by_threshold, _, _ = probe27(yi, 2, k, b[:, 1], b[:, 2], pt[ys, xs], np.broadcast_to(np.array([0, 0, 1], F), (len(k), 3)))
    assert set(np.unique(val)) == {F(0.2), F(0.9)} and np.array_equal(by_threshold, (val > F(0.5)).astype(F))
    # pixels whose hit lies within 1e-4 texel of a texel edge may go either way: left out, at most 1 % of the hit pixels
    tuv = np.einsum("kc,kcd->kd", b.astype(np.float64), uv[k].astype(np.float64)) * T
    near_edge = (np.abs(tuv - np.round(tuv)) < 1e-4).any(axis=1)
    assert near_edge.mean() <= 0.01
    picks_b = val > F(0.5)
    assert picks_b[~near_edge].mean() >= 0.2 and (~picks_b)[~near_edge].mean() >= 0.2
    want = np.where(picks_b[:, None], fb[ys, xs], fa[ys, xs])
    differ = np.abs(fa[ys, xs] - fb[ys, xs])[:, :3].max(axis=1) > 1e-3      # (not in the box's shadow, where both are black)
    assert differ.mean() > 0.7 and (differ & picks_b).sum() >= 30 and (differ & ~picks_b).sum() >= 30, "films A and B must differ where the plane is lit"
    wrong = (fm[ys, xs] != want).any(axis=1) & ~near_edge
    print(f"plane pixels {len(k)}, left out {int(near_edge.sum())}, material2 on {float(picks_b.mean()):.2f}, wrong {int(wrong.sum())}")
    assert not wrong.any()
    assert np.array_equal(fm[~hit], fa[~hit]) and np.array_equal(fa[~hit], fb[~hit])


# ---- 4. getTransparency compares with 0.5, not with the threshold -------------------------------------------------------
SHEET = scenes._quad((-0.9, -0.9, 0.8), (0.9, -0.9, 0.8), (0.9, 0.9, 0.8), (-0.9, 0.9, 0.8))


def sheet_scenes(value, **mask_kw):
    """a sheet over the clay scene: on a mask of an opaque and a tinted transparent material (threshold 0.8), on either material alone"""
    tri_mat = lambda k: [0] * 2 + [0] * 10 + [k] * 2
    mats = lambda last: [CLAY, RED, TINTED, last]
    kw = dict({"threshold": 0.8, "material1": "mat1", "material2": "mat2"}, **mask_kw)
    return (scene(mats(value_mask(value, **kw)), tri_mat(3), extra=[SHEET]), scene(mats(SPARE), tri_mat(1), extra=[SHEET]), scene(mats(SPARE), tri_mat(2), extra=[SHEET]))


def test_transparent_shadows_use_one_half_whatever_the_threshold():
    """mask value 0.6 under threshold 0.8: initBsdf picks material1 (material_mask.cc:45), getTransparency material2 (:96).  The camera
    sees the opaque sheet, the floor the shadow of the tinted one.  Mask value 0.4: both pick material1, and the sheet blocks"""
    rd = settings(RES, transpShad=True, shadowDepth=4)      # one sample per pixel, at its centre: primary_hits tells what every pixel sees
    masked, opaque, tinted = sheet_scenes(0.6)
    (fm, _), (fo, _), (ft, _) = device(masked, rd), device(opaque, rd), device(tinted, rd)
    tri, _, _ = primary_hits(opaque, rd)
    sheet = tri >= 12
    assert 0.1 < sheet.mean() < 0.7
    lit_through = (np.abs(ft - fo)[..., :3].max(axis=-1) > 1e-3) & ~sheet
    assert lit_through.sum() >= 10, "the tinted sheet's shadow must differ from the opaque one's on the floor"
    assert np.array_equal(fm[sheet], fo[sheet]), "to the camera the sheet is material1"
    assert np.array_equal(fm[~sheet], ft[~sheet]), "its shadow is material2's"
    assert not np.array_equal(fm[~sheet], fo[~sheet])
    blocked, _, _ = sheet_scenes(0.4)
    fb = device(blocked, rd)[0]
    assert np.array_equal(fb[sheet], fo[sheet]) and np.array_equal(fb[~sheet], fo[~sheet]), "mask value 0.4: an opaque sheet"


# ---- 5. recursion ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sub", ["mirror", "glass with absorption"])
def test_recursion_levels_pick_too(sub):
    """raydepth 3: the reflected and refracted rays of a level hit masked triangles again.  getVolumeHandler() is read off the mask,
    which has none (integrator_montecarlo.cc:991, :1016): glass under a mask equals glass WITHOUT absorption"""
    if sub == "mirror":
        masked, plain = pair(MIRROR, BLUE)
    else:
        masked, plain = pair(dict(GLASS, absorption=(0.3, 0.6, 0.9), absorption_dist=0.2), BLUE, plain1=GLASS)
    rd = settings(RES, spp=2, raydepth=3)
    same(device(masked, rd), device(plain, rd), sub)
    if sub != "mirror":      # and the absorption would have shown
        absorbing = scene([dict(GLASS, absorption=(0.3, 0.6, 0.9), absorption_dist=0.2), BLUE, SPARE], PICK, texel_uv(PICK), [TWO_TEXELS])
        assert not np.array_equal(device(absorbing, rd)[0], device(plain, rd)[0])


# ---- 6. material-level fields ------------------------------------------------------------------------------------------
def test_receive_shadows_is_the_masks():
    masked, plain = pair(RED, BLUE, plain1=dict(RED, receive_shadows=False), plain2=dict(BLUE, receive_shadows=False), receive_shadows=False)
    rd = settings(RES, spp=2)
    same(device(masked, rd), device(plain, rd), "receive_shadows false on the mask")
    shadowed, _ = pair(RED, BLUE)
    assert not np.array_equal(device(shadowed, rd)[0], device(plain, rd)[0])
    # ... and a sub-material's own receive_shadows = false does not count under a mask that receives them
    masked, plain = pair(dict(RED, receive_shadows=False), BLUE, plain1=RED)
    same(device(masked, rd), device(plain, rd), "receive_shadows false on a sub-material")


def test_flat_material_under_a_mask_is_not_flat_to_the_integrator():
    """isFlat() is read off the mask (integrator_montecarlo.cc:105, :189): the cosine stays"""
    masked, plain = pair(dict(RED, flat_material=True), BLUE, plain1=RED)
    rd = settings(RES, spp=2)
    same(device(masked, rd), device(plain, rd), "flat_material on a sub-material")
    flat = scene([dict(RED, flat_material=True), BLUE, SPARE], PICK, texel_uv(PICK), [TWO_TEXELS])
    assert not np.array_equal(device(flat, rd)[0], device(plain, rd)[0])


def test_shadow_only_mask_hides_and_keeps_its_shadow():
    rd = settings(RES)
    masked, _, _ = sheet_scenes(0.6, visibility="shadow_only")
    hidden = scene([CLAY, dict(RED, visibility="shadow_only"), TINTED, SPARE], [0] * 12 + [1] * 2, extra=[SHEET])
    same(device(masked, rd), device(hidden, rd), "visibility shadow_only on the mask")
    _, opaque, _ = sheet_scenes(0.6)
    fm, fo = device(masked, rd)[0], device(opaque, rd)[0]
    tri, _, _ = primary_hits(opaque, rd)
    behind = primary_hits(scene([CLAY, RED, TINTED, SPARE], [0] * 12), rd)[0]
    sheet = tri >= 12
    floor_only = ~sheet & (behind >= 0)
    assert np.array_equal(fm[floor_only], fo[floor_only]), "the shadow stays"
    assert (np.abs(fm - fo)[sheet][:, :3].max(axis=1) > 1e-3).mean() > 0.5, "the sheet itself is gone"


# ---- 7. the chosen material's own nodes and bump run ---------------------------------------------------------------------
def test_sub_material_with_nodes_and_bump():
    masked, plain = pair(NODE_MATERIAL, BLUE, textures=(TWO_TEXELS, FLAT_TEXTURE))
    rd = settings(RES, spp=2)
    same(device(masked, rd), device(plain, rd), "a node material with bump under a mask")
    # (NODE_MATERIAL's colour comes from its texture, not from its `color`: had its nodes not run the film would be another)
    undone, _ = pair(dict({k: v for k, v in NODE_MATERIAL.items() if k not in ("nodes", "diffuse_shader", "bump_shader")}), BLUE, textures=(TWO_TEXELS, FLAT_TEXTURE))
    assert not np.array_equal(device(undone, rd)[0], device(plain, rd)[0])


# ---- 8. switches -------------------------------------------------------------------------------------------------------
def test_shards_and_serial_replay():
    """two tile shards add up to the unsharded film; with one light and no roulette no serial state is consumed, and the replay switch
    changes nothing"""
    masked, _ = pair(RED, BLUE)
    rd = settings(RES, spp=2)
    full, yi = device(masked, rd)
    parts = [device(masked, rd, shard=(r, 2)) for r in range(2)]
    assert all(p[0][..., 4].any() for p in parts)
    assert np.array_equal(parts[0][0] + parts[1][0], full)
    assert sum(p[1].getRenderStats().rays_shadow for p in parts) == yi.getRenderStats().rays_shadow
    for replay in (True, False):
        assert np.array_equal(device(masked, rd, replay=replay)[0], full)


def test_ambient_occlusion_on_a_masked_scene():
    masked, plain = pair(RED, BLUE)
    rd = settings(RES, spp=2, do_AO=True, AO_samples=4, AO_distance=0.6, AO_color=(0.9, 0.8, 0.7))
    same(device(masked, rd), device(plain, rd), "do_AO")


def test_an_unused_mask_sizes_nothing(monkeypatch, capfd):
    """a mask no triangle refers to changes neither the film nor the shading kernel the pass picks"""
    monkeypatch.setenv("YAFGPU_VERBOSE", "1")
    rd = settings(RES, spp=2, integrator="pathtracing", bounces=3)
    kernel = lambda: re.findall(r"shading kernel: (\S+) \(materials (0x[0-9a-f]+), frames (\d+)\)", capfd.readouterr().err)
    with_mask = device(scene([CLAY, BLUE, mask_mat(material2="mat0", material1="mat1", nodes=(dict(name="mk", type="value", scalar=0.9),))], [0, 0] + [1] * 10), rd)
    k_mask = kernel()
    without = device(scene([CLAY, BLUE, RED], [0, 0] + [1] * 10), rd)
    k_plain = kernel()
    same(with_mask, without, "an unused mask")
    assert k_mask and k_mask == k_plain and k_mask[0][0] != "general", (k_mask, k_plain)
    # in use, it takes the general kernel and counts its sub-materials' types, not its own
    used = device(scene([CLAY, BLUE, mask_mat(material2="mat0", material1="mat1", nodes=(dict(name="mk", type="value", scalar=0.9),))], [2, 2] + [1] * 10), rd)
    k_used = kernel()
    assert k_used[0][0] == "general" and k_used[0][1:] == k_plain[0][1:], (k_used, k_plain)
    # (another kernel than `without` ran: the project's 1e-4 on normalized pixels, not bits)
    assert np.abs(used[0][..., :3] / used[0][..., 4:5] - without[0][..., :3] / without[0][..., 4:5]).max() <= 1e-4
