"""The blend material on the DEVICE (BlendMaterial, material_blend.cc): every material function runs on two sub-materials and mixes the
results by val and ival = min(1, max(0, 1 - val)).

The oracle does not know blend_mat, so the material is held to its parts and to identities, not to the reference's compiled
material_blend.cc:
  1. its leaf functions (probe ops 11 and 12 on a blend's record) against the oracle's outputs for the two sub-materials — those are
     pinned to the reference's compiled sources — combined in float32 by the reference's expressions, one rounding per operation;
  2. blend_value 0 and 1 are the plain materials, bit for bit;   3. a node that is 0 or 1 everywhere is the mask material at 0.5;
  4. where the integrator is linear in the material the film is the weighted sum of the plain films;
  5. transparent shadows mix the two filters, alpha is the smaller one;   6. `sample` inside a path;   7. textured sub-materials.
Films that are compared bit for bit come from the same shading kernel: a scene takes the kernel with the blend's code when some triangle
uses a blend_mat, so the plain scene of such a pair carries one too, on a tiny triangle under the floor that no ray reaches (CARRIER).
Paired renders run with the libc stream pinned and the same materials created in the same order."""
import ctypes as C

import numpy as np
import pytest

from libyafaray_amd import Interface, scenes
from oracle import pyoracle as po
from tests.test_gpu_ao import CLAY, POINT, clay_scene, settings
from tests.test_gpu_components import exact
from tests.test_gpu_mask import device, primary_hits, probe27, same

pytestmark = pytest.mark.gpu

F = np.float32
W = Interface.MATERIAL_FIELDS


@pytest.fixture(scope="module", autouse=True)
def torch_first():
    """(as in the other GPU modules: let torch open the GPU before the library does)"""
    import torch
    torch.cuda.init()


def blend_mat(value=0.5, material1="mat1", material2="mat2", nodes=(), **kw):
    return dict({"type": "blend_mat", "material1": material1, "material2": material2, "blend_value": float(value), "nodes": list(nodes)}, **kw)


def weights(value):
    """getBlendVal, material_blend.cc:57-75: val as it is, ival = min(1, max(0, 1 - val)), in float32"""
    val = np.asarray(value, F)
    return val, np.minimum(F(1), np.maximum(F(0), (F(1) - val).astype(F))).astype(F)


# ---- 1. leaf functions against pinned parts ----------------------------------------------------------------------------
D1 = {"type": "shinydiffusemat", "color": (0.8, 0.15, 0.1), "diffuse_reflect": 0.9}
D2 = {"type": "shinydiffusemat", "color": (0.2, 0.7, 0.3), "diffuse_reflect": 0.8, "specular_reflect": 0.3, "transparency": 0.4, "transmit_filter": 0.7,
      "mirror_color": (0.9, 0.8, 0.7), "fresnel_effect": True, "IOR": 1.5}
GLOSSY = {"type": "glossy", "color": (0.9, 0.85, 0.8), "diffuse_color": (0.5, 0.4, 0.6), "diffuse_reflect": 0.4, "glossy_reflect": 0.6, "exponent": 40.0, "as_diffuse": False}
COATED = {"type": "coated_glossy", "color": (0.8, 0.9, 0.7), "diffuse_color": (0.3, 0.5, 0.6), "diffuse_reflect": 0.5, "glossy_reflect": 0.7, "exponent": 80.0,
          "as_diffuse": True, "IOR": 1.6, "mirror_color": (0.9, 0.9, 1.0), "specular_reflect": 0.8}
MIRROR = {"type": "mirror", "color": (0.9, 0.9, 1.0), "reflect": 0.8}
GLASS = {"type": "glass", "IOR": 1.45, "filter_color": (0.8, 1.0, 0.85), "transmit_filter": 0.9, "mirror_color": (1.0, 0.95, 0.9), "fake_shadows": True}
LIGHT = {"type": "light_mat", "color": (1.0, 0.9, 0.8), "power": 3.0}
PAIRS = {"diffuse + diffuse": (D1, D2), "diffuse + glossy": (D1, GLOSSY), "glossy + coated glossy": (GLOSSY, COATED), "mirror + diffuse": (MIRROR, D1),
         "glass + diffuse": (GLASS, D2), "light + diffuse": (LIGHT, D1), "diffuse + glass": (D1, GLASS)}
VALUES = (0.0, 0.3, 1.0, 1.4, -0.2)          # the last two: ival is clamped, val is not
N_ROWS = 2000
INCLUDE_LIGHTS = 0x40000000                   # op 11 takes include_lights from `flag word != 0.f`: a bit no lobe has makes the word a normal float
FLAG_WORDS = [0x7f, 0x3e, 0x34, 0x14, 0x12, 0x31, 0x11, 0x1, 0x2, 0x4, 0x24, 0x60, 0x84]      # all, MIS, path, diffuse, glossy, specular ..., single bits: words that reach one sub-material only


def leaf_rows(seed):
    rng = np.random.default_rng(seed)
    unit = lambda a: (a / np.linalg.norm(a, axis=1, keepdims=True)).astype(F)
    n = unit(rng.normal(size=(N_ROWS, 3)))
    ng = n.copy()
    ng[N_ROWS // 2:] = unit(n[N_ROWS // 2:] + rng.normal(0, 0.2, (N_ROWS - N_ROWS // 2, 3)))
    wo = unit(n + rng.normal(0, 0.7, (N_ROWS, 3)))      # mostly above the surface, some below
    wl = unit(n + rng.normal(0, 0.7, (N_ROWS, 3)))
    s = rng.random((N_ROWS, 2)).astype(F)
    flags = rng.choice(np.array(FLAG_WORDS, np.uint32), N_ROWS) | np.uint32(INCLUDE_LIGHTS)
    flags[:8] = 0                                       # no lobe asked for, include_lights false
    return np.hstack([n, ng, wo, wl, s]).astype(F), flags.astype(np.uint32)


def oracle_parts(mat, inp, flags):
    """the oracle's outputs for one sub-material at every row: what ops 11 and 12 give for a plain record"""
    L, md, n = po.lib(), po.material_desc(mat), len(inp)
    o = dict(eval=np.zeros((n, 3), F), pdf=np.zeros(n, F), sampled=np.zeros(n, np.uint32), s8=np.zeros((n, 8), F), spec=np.zeros(n, np.uint32), o12=np.zeros((n, 12), F),
             alpha=np.zeros(n, F), transp=np.zeros((n, 3), F), emit=np.zeros((n, 3), F))
    bf, pdf, so, fl, al = C.c_int32(), C.c_float(), C.c_int32(), C.c_int32(), C.c_float()
    for i in range(n):
        row = np.ascontiguousarray(inp[i])
        L.yor_material_probe(C.byref(md), po.fptr(row), int(flags[i]), C.byref(bf), po.fptr(o["eval"][i]), C.byref(pdf), C.byref(so), po.fptr(o["s8"][i]))
        o["pdf"][i], o["sampled"][i] = pdf.value, np.uint32(so.value & 0xffffffff)
        L.yor_material_specular(C.byref(md), po.fptr(row), 1, C.byref(fl), po.fptr(o["o12"][i]), C.byref(al))
        o["spec"][i], o["alpha"][i] = fl.value, al.value
        L.yor_material_transparency(C.byref(md), po.fptr(row), po.fptr(o["transp"][i]))
        L.yor_lightmat_emit(C.byref(md), po.fptr(row[0:3].copy()), po.fptr(row[6:9].copy()), int(flags[i] != 0), po.fptr(o["emit"][i]))
    o["flags"] = np.uint32(bf.value)
    return o


def mix(c1, c2, ival, val):
    """ADD_COLORS / ADD_PDF (material_blend.cc:33-36): c1 * ival + c2 * val, three float32 operations"""
    return ((c1 * ival).astype(F) + (c2 * val).astype(F)).astype(F)


def normalize(v):
    """Vec3::normalize, vector.h:227-238"""
    l = ((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]).astype(F) + v[:, 2] * v[:, 2]).astype(F)
    inv = (F(1) / np.sqrt(np.where(l != 0, l, F(1)))).astype(F)
    return np.where((l != 0)[:, None], (v * inv[:, None]).astype(F), v).astype(F)


def blend_expected(a, b, flags, value, transparent):
    """BlendMaterial's functions (eval :106-129, pdf :239-257, sample :131-214, emit :397-420, getSpecular :259-325, getAlpha :363-395,
    getTransparency :337-361) on the two sub-materials' outputs -> op 11's 17 words, op 12's 17 words"""
    val, ival = weights(value)
    n = len(flags)
    o11, o12 = np.zeros((n, 17), F), np.zeros((n, 17), F)
    o11[:, 0] = np.full(n, a["flags"] | b["flags"], np.uint32).view(F)
    o11[:, 1:4] = mix(a["eval"], b["eval"], ival, val)
    o11[:, 4] = mix(a["pdf"], b["pdf"], ival, val)
    m1, m2 = (flags & a["flags"]) != 0, (flags & b["flags"]) != 0
    zero8 = np.zeros((n, 8), F)                                          # a sub-material that is not sampled: colour, direction, pdf and weight stay 0
    s1, s2 = np.where(m1[:, None], a["s8"], zero8), np.where(m2[:, None], b["s8"], zero8)
    f1, f2 = np.where(m1, a["sampled"], 0).astype(np.uint32), np.where(m2, b["sampled"], 0).astype(np.uint32)
    both, only1 = m1 & m2, m1 & ~m2
    col_both = mix((s1[:, 0:3] * s1[:, 7:8]).astype(F), (s2[:, 0:3] * s2[:, 7:8]).astype(F), ival, val)
    wi_both = normalize((s2[:, 3:6] + s1[:, 3:6]).astype(F))
    pdf_both = mix(s1[:, 6], s2[:, 6], ival, val)
    pick = lambda x_both, x1, x2: np.where(both.reshape((n,) + (1,) * (x1.ndim - 1)), x_both, np.where(only1.reshape((n,) + (1,) * (x1.ndim - 1)), x1, x2))
    o11[:, 5] = pick(f1 | f2, f1, f2).astype(np.uint32).view(F)          # neither sampled: f2 is 0 there, Sample's initial sampled_flags_
    o11[:, 6:9] = pick(col_both, s1[:, 0:3], s2[:, 0:3])
    o11[:, 9:12] = pick(wi_both, s1[:, 3:6], s2[:, 3:6])
    o11[:, 12] = pick(pdf_both, s1[:, 6], s2[:, 6])
    o11[:, 13] = pick(np.ones(n, F), s1[:, 7], s2[:, 7])
    o11[:, 14:17] = mix(a["emit"], b["emit"], ival, val)
    o12[:, 0] = (a["spec"] | b["spec"]).astype(np.uint32).view(F)
    for bit, lo in ((1, 0), (2, 6)):                                     # reflection: words 0..5 of the oracle's twelve, refraction: 6..11
        r1, r2 = (a["spec"] & bit) != 0, (b["spec"] & bit) != 0
        d1, c1, d2, c2 = a["o12"][:, lo:lo + 3], a["o12"][:, lo + 3:lo + 6], b["o12"][:, lo:lo + 3], b["o12"][:, lo + 3:lo + 6]
        both_r, only_1 = (r1 & r2)[:, None], (r1 & ~r2)[:, None]
        # :290-303 (and :305-318): mixed where both; material1's * ival where only it; else whatever material2 left, * val
        o12[:, 1 + lo:4 + lo] = np.where(both_r, normalize((d2 + d1).astype(F)), np.where(only_1, d1, d2))
        o12[:, 4 + lo:7 + lo] = np.where(both_r, mix(c1, c2, ival, val), np.where(only_1, (c1 * ival).astype(F), (c2 * val).astype(F)))
    o12[:, 13] = np.minimum(a["alpha"], b["alpha"]) if transparent else F(1)
    o12[:, 14:17] = mix(a["transp"], b["transp"], ival, val)
    return o11, o12


@pytest.mark.parametrize("pair", sorted(PAIRS))
def test_leaf_functions_against_pinned_parts(pair):
    """Measured on gfx950: every row of every pair and value bit-exact (share 1.0000 of 7 x 5 x 2000 rows, ops 11 and 12): no operation of
    the blend's own differs, and the sub-materials here have no anisotropic lobe (whose tanf is the one known last-bit difference)."""
    m1, m2 = PAIRS[pair]
    tri = np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0]]], F)
    sc = {"verts": tri, "tri_mat": np.array([1], np.int32), "vnormals": None, "materials": [m1, m2] + [blend_mat(v, "mat0", "mat1") for v in VALUES], "lights": [],
          "camera": {"type": "perspective", "from": (0.5, 0.5, 5.0), "to": (0.5, 0.5, 0.0), "up": (0.5, 1.5, 5.0), "resx": 8, "resy": 8}}
    yi = Interface()
    scenes.load_scene(yi, sc, settings((8, 8)))
    yi.prepareRender()
    table = yi.getMaterialTable()
    inp, flags = leaf_rows(sorted(PAIRS).index(pair) + 11)
    a, b = oracle_parts(m1, inp, flags), oracle_parts(m2, inp, flags)
    assert a["flags"] == np.uint32(table[0, W["bsdf_flags"]]) and b["flags"] == np.uint32(table[1, W["bsdf_flags"]])
    reach_one = ((flags & a["flags"]) != 0) != ((flags & b["flags"]) != 0)
    assert reach_one.sum() >= 50 or a["flags"] == b["flags"], "some flag words must reach only one of the two sub-materials"
    transparent = bool(table[2, W["is_transparent"]])
    assert transparent == (pair in ("diffuse + diffuse", "glass + diffuse", "diffuse + glass"))
    exact_rows = []
    for k, value in enumerate(VALUES):
        assert table[2 + k, W["type"]] == 8
        want11, want12 = blend_expected(a, b, flags, value, transparent)
        idx = np.full((N_ROWS, 1), np.uint32(2 + k)).view(F)
        x11 = np.hstack([idx, inp, flags.reshape(-1, 1).view(F)])
        got11 = yi.probe(11, x11, 17)
        got12 = yi.probe(12, np.hstack([x11[:, :10], np.ones((N_ROWS, 1), F)]), 17)
        for got, want in ((got11, want11), (got12, want12)):
            ok = (got.view(np.uint32) == want.view(np.uint32)) | ((got == 0) & (want == 0)) | (np.isnan(got) & np.isnan(want))
            exact_rows.append(ok.all(axis=1).mean())
        print(f"{pair}, blend_value {value}: rows bit-exact, op 11 {exact_rows[-2]:.4f}, op 12 {exact_rows[-1]:.4f}")
        with np.errstate(all="ignore"):
            assert np.array_equal(got11[:, 0].view(np.uint32), want11[:, 0].view(np.uint32)), "initBsdf: the union of flags"
            exact(got11[:, 1:4], want11[:, 1:4].view(np.uint32), f"{pair} {value} eval")
            exact(got11[:, 4], want11[:, 4].view(np.uint32), f"{pair} {value} pdf")
            assert np.array_equal(got11[:, 5].view(np.uint32), want11[:, 5].view(np.uint32)), "sampled flags"
            exact(got11[:, 6:14], want11[:, 6:14].view(np.uint32), f"{pair} {value} sample")
            exact(got11[:, 14:17], want11[:, 14:17].view(np.uint32), f"{pair} {value} emit")
            assert np.array_equal(got12[:, 0].view(np.uint32), want12[:, 0].view(np.uint32)), "getSpecular flags"
            exact(got12[:, 1:13], want12[:, 1:13].view(np.uint32), f"{pair} {value} getSpecular")
            exact(got12[:, 13], want12[:, 13].view(np.uint32), f"{pair} {value} getAlpha")
            exact(got12[:, 14:17], want12[:, 14:17].view(np.uint32), f"{pair} {value} getTransparency")
    assert min(exact_rows) == 1.0


def test_the_frame_initbsdf_leaves():
    """BlendMaterial::initBsdf ends with sp = blendSurfacePoints__(sp_0, sp_1, inv_alpha) (:98, surface.cc:137-151); without bump both copies
    are the vertex's own frame, and lerp__(v, v, alpha) = v * alpha + v * (1.0 - alpha) (util_interpolation.h:31-36, alpha a double narrowed by
    Vec3 * float) gives n_, nu_ and nv_ back only up to roundings: probe op 31 (blend_lerp_frame with the record's ival) against that
    expression in float32, bit for bit: the frame is not renormalised, leaving the lerp out shows at 0.3, and a lerp by val instead of the
    clamped ival shows at 1.4 and -0.2 (at 0.3 the two weights only trade places, which the sum does not see)"""
    tri = np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0]]], F)
    sc = {"verts": tri, "tri_mat": np.array([0], np.int32), "vnormals": None, "materials": [D1, GLOSSY] + [blend_mat(v, "mat0", "mat1") for v in VALUES], "lights": [],
          "camera": {"type": "perspective", "from": (0.5, 0.5, 5.0), "to": (0.5, 0.5, 0.0), "up": (0.5, 1.5, 5.0), "resx": 8, "resy": 8}}
    yi = Interface()
    scenes.load_scene(yi, sc, settings((8, 8)))
    yi.prepareRender()
    rng = np.random.default_rng(31)
    n = rng.normal(size=(N_ROWS, 3))
    n = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(F)
    n[:3] = np.array([[0, 0, 1], [0, 0, -1], [1, 0, 0]], F)
    changed = []
    for k, value in enumerate(VALUES):
        o = yi.probe(31, np.hstack([np.full((N_ROWS, 1), np.uint32(2 + k)).view(F), n]), 17)
        val, ival = weights(value)
        assert np.array_equal(o[:, 15].view(np.uint32), np.full(N_ROWS, val, F).view(np.uint32)) and np.array_equal(o[:, 16].view(np.uint32), np.full(N_ROWS, ival, F).view(np.uint32))
        other = F(1.0 - np.float64(ival))                                   # (1.0 - alpha) in double, narrowed by Vec3 * float
        frame = np.hstack([n, o[:, 9:15]])                                   # n and create_cs's nu, nv
        want = ((frame * ival).astype(F) + (frame * other).astype(F)).astype(F)
        exact(o[:, 0:9], want.view(np.uint32), f"frame after initBsdf, blend_value {value}")
        changed.append(float((want != frame).any(axis=1).mean()))
        if value in (0.0, 1.0, 1.4, -0.2):                                   # ival 1, 0, 0, 1: v * 1 + v * 0 is v
            assert changed[-1] == 0.0
        if value in (1.4, -0.2):                                             # here a lerp by val instead of ival would not be the identity
            wrong = ((frame * val).astype(F) + (frame * F(1.0 - np.float64(val))).astype(F)).astype(F)
            assert (wrong != want).any(axis=1).mean() > 0.2, "val for ival must show"
    print(f"rows whose frame the lerp changes, per blend_value {VALUES}: {changed}")
    assert changed[1] > 0.2, "at 0.3 the lerp is not the identity: leaving it out must show"


# ---- scenes of the render tests ------------------------------------------------------------------------------------------
RES = (32, 32)
RED = {"type": "shinydiffusemat", "color": (0.8, 0.15, 0.1), "diffuse_reflect": 1.0}
BLUE = {"type": "shinydiffusemat", "color": (0.1, 0.2, 0.8), "diffuse_reflect": 0.8}
SHEEN = {"type": "glossy", "color": (0.9, 0.9, 0.8), "diffuse_color": (0.2, 0.6, 0.7), "diffuse_reflect": 0.5, "glossy_reflect": 0.5, "exponent": 30.0, "as_diffuse": True}
# a blend in use makes a scene take the kernel built with the blend's code: this triangle carries one in the scenes that have no other.
# 1 cm wide, 5 below the middle of the floor: every ray of these scenes starts above the floor's plane, inside the floor's outline
CARRIER = np.array([[[0.0, 0.0, -5.0], [0.01, 0.0, -5.0], [0.0, 0.01, -5.0]]], F)
CARRIER_BLEND = blend_mat(0.5)


def box_scene(materials, box_mat, plane_mat=0, uv=False, textures=(), res=RES):
    """the clay scene (a floor and a box on it, one point light) with the box's ten triangles on materials[box_mat], and the carrier
    triangle on the last material"""
    g = clay_scene(res=res, lights=[POINT], extra=[(CARRIER, CLAY)])
    sc = dict(g, materials=list(materials), tri_mat=np.array([plane_mat] * 2 + [box_mat] * 10 + [len(materials) - 1], np.int32))
    if uv:
        v = np.asarray(sc["verts"], F).reshape(-1, 3, 3)
        sc["uv"] = np.stack([v[..., 0] * F(0.913) + v[..., 2] * F(1.31) + F(0.537), v[..., 1] * F(0.877) + v[..., 2] * F(0.71) + F(0.561)], axis=-1).astype(F) / F(2)
    if textures:
        sc["textures"] = list(textures)
    return sc


# ---- 2. endpoints are the plain materials --------------------------------------------------------------------------------
@pytest.mark.parametrize("value", [0.0, 1.0])
def test_endpoints_are_the_plain_materials(value):
    """c * 1 + d * 0 is exact for finite values, lerp__(v, v, 1) and lerp__(v, v, 0) return v, and direct lighting reads eval alone: the
    film and the ray counts are those of material1 (blend_value 0) or material2 (1) alone.  Both sub-materials have the lobes Diffuse |
    Reflect, so the union sends the vertex the same way"""
    mats = [CLAY, RED, SHEEN, blend_mat(value), CARRIER_BLEND]
    rd = settings(RES, spp=4)
    blended, plain, other = (device(box_scene(mats, k), rd) for k in (3, 1 if value == 0.0 else 2, 2 if value == 0.0 else 1))
    same(blended, plain, f"blend_value {value}")
    assert (np.abs(plain[0] - other[0])[..., :3].max(axis=-1) > 1e-3).mean() > 0.05, "the two plain films must differ"


def test_plain_materials_shade_alike_in_the_blend_kernel_and_outside_it():
    """the bit-equalities of this file compare films of the kernel with the blend's code with each other.  This holds that kernel's shading
    of PLAIN materials to the kernels every other scene takes: the same scene with the carrier triangle on a blend (the blend kernel runs)
    and on a diffuse material (a kernel without the blend's code runs), direct lighting and path tracing, to the project's 1e-4 on
    normalized pixels and far inside it — the arithmetic per path is the same source"""
    for kw in (dict(spp=4), dict(spp=4, integrator="pathtracing", bounces=3)):
        rd = settings(RES, **kw)
        with_blend = device(box_scene([CLAY, RED, SHEEN, BLUE, CARRIER_BLEND], 2), rd)
        without = device(box_scene([CLAY, RED, SHEEN, BLUE, dict(BLUE)], 2), rd)
        (fa, ya), (fb, yb) = with_blend, without
        assert fa[..., 4].all() and np.array_equal(fa[..., 4], fb[..., 4])
        a, b = fa[..., :3] / fa[..., 4:5], fb[..., :3] / fb[..., 4:5]
        dev = float(np.abs(a - b).max())
        print(f"{kw}: blend kernel against the scene's usual kernel on plain materials: largest deviation {dev:.3g}, bit-equal pixels {float((fa == fb).all(axis=-1).mean()):.4f}")
        assert a.max() > 0.1 and dev <= 1e-5
        sa, sb = ya.getRenderStats(), yb.getRenderStats()
        assert (sa.rays_closest, sa.rays_shadow) == (sb.rays_closest, sb.rays_shadow)


# ---- 3. a binary node-driven blend is the mask ---------------------------------------------------------------------------
def exact_one():
    """a green level g with 0.7152f * g == 1 in float32: Texture::getFloat is col2Bri, 0.2126f r + 0.7152f g + 0.0722f b"""
    g = F(1) / F(0.7152)
    for _ in range(8):
        for cand in (g, np.nextafter(g, F(2)), np.nextafter(g, F(0))):
            if F(0.7152) * cand == F(1):
                return cand
        g = np.nextafter(g, F(2))
    raise AssertionError("no float32 green level gives a node scalar of exactly 1")


def test_a_binary_node_driven_blend_is_the_mask():
    g1 = exact_one()
    assert ((F(0.2126) * F(0) + F(0.7152) * g1).astype(F) + F(0.0722) * F(0)) == F(1)
    rng = np.random.default_rng(3)
    on = rng.integers(0, 2, (4, 4)).astype(bool)
    assert on.any() and (~on).any()
    texels = np.zeros((4, 4, 4), F)
    texels[..., 1] = np.where(on, g1, F(0)); texels[..., 3] = 1
    tex = dict(name="t_bin", texels=texels, interpolate="none", clipping="repeat", color_space="LinearRGB")
    mapper = dict(name="mk", type="texture_mapper", texture="t_bin", texco="uv", mapping="plain")
    driven = blend_mat(0.5, mask="mk", nodes=(mapper,))
    masked = {"type": "mask_mat", "material1": "mat1", "material2": "mat2", "mask": "mk", "threshold": 0.5, "nodes": [mapper]}
    rd = settings(RES, spp=4)
    as_blend = device(box_scene([CLAY, RED, SHEEN, driven, CARRIER_BLEND], 3, uv=True, textures=[tex]), rd)
    as_mask = device(box_scene([CLAY, RED, SHEEN, masked, CARRIER_BLEND], 3, uv=True, textures=[tex]), rd)
    same(as_blend, as_mask, "a blend driven by a node that is 0 or 1 against mask_mat at 0.5")
    one = device(box_scene([CLAY, RED, SHEEN, driven, CARRIER_BLEND], 1, uv=True, textures=[tex]), rd)[0]
    two = device(box_scene([CLAY, RED, SHEEN, driven, CARRIER_BLEND], 2, uv=True, textures=[tex]), rd)[0]
    f = as_blend[0]
    differs = lambda p, q: np.abs(p - q)[..., :3].max(axis=-1) > 1e-3
    assert differs(f, one).mean() > 0.02 and differs(f, two).mean() > 0.02, "both materials must show on the box"


# ---- 4. linearity where the integrator is linear -------------------------------------------------------------------------
LINEAR = {"diffuse A + diffuse B": (RED, BLUE), "mirror + diffuse": (MIRROR, BLUE), "light + diffuse": (LIGHT, BLUE)}


@pytest.mark.parametrize("pair", sorted(LINEAR))
def test_linear_in_the_blend_value(pair):
    """direct lighting, raydepth 2, blend_value 0.3: emission, the light estimate (eval) and getSpecular's colours are linear in the
    material, so film(blend) = ival * film(material1) + val * film(material2) up to a handful of float32 roundings per sample"""
    m1, m2 = LINEAR[pair]
    mats = [CLAY, m1, m2, blend_mat(0.3), CARRIER_BLEND]
    rd = settings(RES, spp=4, raydepth=2)
    (fb, yb), (f1, y1), (f2, y2) = (device(box_scene(mats, k), rd) for k in (3, 1, 2))
    val, ival = weights(0.3)
    want = float(ival) * f1.astype(np.float64) + float(val) * f2.astype(np.float64)
    assert np.array_equal(fb[..., 4], f1[..., 4]) and fb[..., 4].all()
    box = np.abs(f1 - f2)[..., :3].max(axis=-1) > 1e-3
    assert box.mean() > 0.05, "the plain films must differ on the box"
    err = np.abs(fb[..., :3] - want[..., :3]) / np.maximum(np.abs(want[..., :3]), 1e-30)
    print(f"{pair}: largest relative deviation from the weighted sum {float(err[want[..., :3] != 0].max()):.3g}, box pixels {int(box.sum())}")
    np.testing.assert_allclose(fb[..., :3], want[..., :3], rtol=1e-5, atol=0)
    sb, s1, s2 = yb.getRenderStats(), y1.getRenderStats(), y2.getRenderStats()
    if pair == "mirror + diffuse":
        # both branches run at a vertex on the blend: the union of flags sends it through the light estimate (as the diffuse material
        # alone) AND the specular branch (as the mirror alone).  n_box camera samples hit the box: each sends a reflected ray
        total = RES[0] * RES[1] * 4
        n_box = s1.rays_closest - total
        assert n_box > 0 and s2.rays_closest == total
        assert sb.rays_closest == s1.rays_closest, "a reflected ray per camera sample on the box, as for the mirror alone"
        assert sb.rays_shadow == s1.rays_shadow + n_box, "and a shadow ray there, as for the diffuse material alone"
        assert s2.rays_shadow < sb.rays_shadow


# ---- 5. transparent shadows and alpha ------------------------------------------------------------------------------------
def test_transparent_shadows_mix_the_filters():
    """a sheet on a blend of a transparent and an opaque shinydiffuse material over a floor, under an infinite directional light: the
    floor under it is the lit floor times t1 * ival + t2 * val (getTransparency, :337-361; t2 = 0), in the closed form and with the
    tolerance of test_transparent_shadows_on_infinite_rays"""
    from tests.test_gpu_lights import directional, lambert_value, occluder, occluder_coords, plane_points, plane_scene, render, shadow_mask, stable
    filt = (0.3, 0.6, 0.9)
    clear = {"type": "shinydiffusemat", "color": filt, "transparency": 1.0, "transmit_filter": 1.0}
    opaque = {"type": "shinydiffusemat", "color": (0.5, 0.5, 0.5)}
    val, ival = weights(0.3)
    for first, second, t_mix in ((clear, opaque, np.array(filt) * float(ival)), (opaque, clear, np.array(filt) * float(val))):
        sc = plane_scene([directional()], extra=[(occluder(), first)])
        sc["materials"] = [sc["materials"][0], first, second, blend_mat(0.3)]
        sc["tri_mat"] = np.array([0, 0, 3, 3], np.int32)
        img, yi = render(sc, transpShad=True, shadowDepth=4)
        pts = plane_points(yi)
        m = shadow_mask(pts)
        x, y = occluder_coords(pts)
        keep = stable(m) & (np.abs(x - y) > 0.15)          # (not where a shadow ray meets both triangles of the quad: see that test)
        v = lambert_value()
        assert m[keep].sum() > 200
        np.testing.assert_allclose(img[m & keep], np.broadcast_to(v * t_mix, img[m & keep].shape), rtol=1e-5)
        np.testing.assert_allclose(img[~m & keep], np.broadcast_to(v, img[~m & keep].shape), rtol=1e-5)


def test_alpha_is_the_smaller_one():
    """getAlpha, :363-395: min(al_1, al_2) where the blend is transparent.  A sheet before an empty, transparent background
    (bg_transp_refract): the film's alpha is the sheet's — 1 - transparency for a shinydiffuse material without a mirror lobe"""
    from tests.test_gpu_lights import directional
    thin = {"type": "shinydiffusemat", "color": (0.3, 0.6, 0.9), "transparency": 0.6, "transmit_filter": 1.0}
    thick = {"type": "shinydiffusemat", "color": (0.9, 0.6, 0.3), "transparency": 0.25, "transmit_filter": 1.0}
    opaque = {"type": "shinydiffusemat", "color": (0.5, 0.5, 0.5)}
    quad = scenes._quad((-10, -10, 0), (10, -10, 0), (10, 10, 0), (-10, 10, 0))
    cam = {"type": "perspective", "from": (0.0, 0.0, 5.0), "to": (0.0, 0.0, 0.0), "up": (0.0, 1.0, 5.0), "resx": 16, "resy": 16, "focal": 1.0}
    rd = scenes.render_settings(16, 16, 1, integrator="directlighting", bg_transp=True, bg_transp_refract=True, raydepth=2, tile_size=8)

    def alpha(materials, k):
        sc = {"verts": quad, "tri_mat": np.array([k, k], np.int32), "vnormals": None, "materials": materials, "lights": [directional()], "camera": cam}
        film = device(sc, rd)[0]
        assert film[..., 4].all()
        return film[..., 3] / film[..., 4]

    mats = [thin, thick, opaque, blend_mat(0.3, "mat0", "mat1"), blend_mat(0.3, "mat2", "mat0"), blend_mat(0.3, "mat2", "mat2")]
    a_thin, a_thick, a_opaque = (alpha(mats, k) for k in (0, 1, 2))
    np.testing.assert_allclose(a_thin, 0.4, rtol=1e-6); np.testing.assert_allclose(a_thick, 0.75, rtol=1e-6); assert (a_opaque == 1).all()
    assert np.array_equal(alpha(mats, 3), a_thin), "two transparent materials: the smaller alpha"
    assert np.array_equal(alpha(mats, 4), a_thin), "an opaque material's alpha is 1: the transparent one's"
    assert (alpha(mats, 5) == 1).all(), "a blend of opaque materials is not transparent: 1"


# ---- 6. `sample` inside a path -------------------------------------------------------------------------------------------
MEAN_MEASURED = 1.17e-8      # relative difference of the frame means, blend against plain, measured on an MI355X (no pixel outside rtol 1e-4, 68 % of them bit-equal)
MEAN_BOUND = 10 * MEAN_MEASURED


def test_sample_inside_a_path():
    """path tracing in a closed box, one area light, 2 bounces, 16 spp: the floor on a blend (0.3) of a glossy material with a second
    material of the same parameters, against the floor on the material itself.  The blend's sample then differs from the material's by
    roundings alone — normalize(wi + wi), c * ival + c * val, the pdf likewise, w = 1 on a colour already times w — and a rounding can flip a
    grazing ray: at most 1 % of the pixels may lie outside rtol 1e-4, and the frame means agree within MEAN_BOUND, ten times the measured
    difference MEAN_MEASURED.  A wrong w, pdf mix or direction moves the mean by percents."""
    sc = scenes.cornell_soup(14, seed=5, n_lights=1, res=RES, open_front=False)
    sc["camera"] = {"type": "perspective", "from": (0.0, -0.9, 0.1), "to": (0.0, 0.2, -0.5), "up": (0.0, -0.9, 1.1), "resx": RES[0], "resy": RES[1], "focal": 0.7}      # inside the box
    gloss = dict(SHEEN)
    sc["materials"] = sc["materials"][:4] + [gloss, dict(gloss), blend_mat(0.3, "mat4", "mat5")]
    rd = scenes.render_settings(RES[0], RES[1], 16, bounces=2, integrator="pathtracing", tile_size=8)
    films = []
    for floor in (6, 4):
        s = dict(sc, tri_mat=np.array([floor, floor] + list(sc["tri_mat"][2:]), np.int32))
        films.append(device(s, rd)[0])
    fb, fp = films
    assert np.array_equal(fb[..., 4], fp[..., 4]) and fp[..., 4].all()
    rgb_b, rgb_p = fb[..., :3].astype(np.float64), fp[..., :3].astype(np.float64)
    outside = (np.abs(rgb_b - rgb_p) > 1e-4 * np.abs(rgb_p)).any(axis=-1)
    mean_diff = abs(rgb_b.mean() - rgb_p.mean()) / rgb_p.mean()
    print(f"pixels outside rtol 1e-4: {float(outside.mean()):.4f}; frame means differ by {mean_diff:.3g} (relative); bit-equal pixels {float((fb == fp).all(axis=-1).mean()):.4f}")
    assert rgb_p.mean() > 0.05
    assert outside.mean() <= 0.01
    assert mean_diff <= MEAN_BOUND


# ---- 7. textured sub-materials -------------------------------------------------------------------------------------------
def test_textured_sub_materials_under_a_node_driven_blend():
    """both sub-materials carry a colour node and the blend is driven by a bilinear texture: two resolved records and the blend's own
    node at every vertex.  One sample per pixel at its centre: the pixel is ival * film(material1) + val * film(material2) with the
    blend's scalar at the camera ray's hit — the hit from the oracle's intersect, the scalar from probe 27 on a mask_mat with the same
    nodes that no triangle uses"""
    res = (24, 24)
    rng = np.random.default_rng(7)
    rand_tex = lambda name, lo, hi: dict(name=name, texels=np.concatenate([rng.uniform(lo, hi, (8, 8, 3)), np.ones((8, 8, 1))], axis=2).astype(F),
                                         interpolate="bilinear", clipping="repeat", color_space="LinearRGB")
    textures = [rand_tex("t_a", 0.2, 0.9), rand_tex("t_b", 0.1, 0.8), rand_tex("t_w", 0.05, 0.95)]
    mapper = lambda name, tex: dict(name=name, type="texture_mapper", texture=tex, texco="uv", mapping="plain")
    m1 = dict(RED, diffuse_shader="ca", nodes=[mapper("ca", "t_a")])
    m2 = dict(SHEEN, diffuse_shader="cb", nodes=[mapper("cb", "t_b")])
    driven = blend_mat(0.5, mask="mk", nodes=(mapper("mk", "t_w"),))
    spare_mask = {"type": "mask_mat", "material1": "mat1", "material2": "mat2", "mask": "mk", "nodes": [mapper("mk", "t_w")]}
    mats = [CLAY, m1, m2, driven, spare_mask, CARRIER_BLEND]
    rd = settings(res)

    def sc(plane_mat):
        s = box_scene(mats, 0, plane_mat=plane_mat, uv=True, textures=textures, res=res)
        return s

    (fb, yi), (f1, _), (f2, _) = (device(sc(k), rd) for k in (3, 1, 2))
    tri, bary, pt = primary_hits(sc(1), rd)
    hit = (tri == 0) | (tri == 1)
    assert hit.mean() > 0.5
    ys, xs = np.nonzero(hit)
    k, b = tri[ys, xs], bary[ys, xs]
    scalar, _, _, _ = probe27(yi, 4, k, b[:, 1], b[:, 2], pt[ys, xs], np.broadcast_to(np.array([0, 0, 1], F), (len(k), 3)))
    assert scalar.min() < 0.3 and scalar.max() > 0.7 and len(np.unique(scalar)) > len(k) // 2
    val, ival = weights(scalar)
    want = ival.astype(np.float64)[:, None] * f1[ys, xs].astype(np.float64) + val.astype(np.float64)[:, None] * f2[ys, xs].astype(np.float64)
    lit = np.abs(f1[ys, xs] - f2[ys, xs])[:, :3].max(axis=1) > 1e-3
    assert lit.mean() > 0.5, "films 1 and 2 must differ where the plane is lit"
    got = fb[ys, xs]
    err = np.abs(got[:, :3] - want[:, :3]) / np.maximum(np.abs(want[:, :3]), 1e-30)
    print(f"plane pixels {len(k)}, lit {int(lit.sum())}: largest relative deviation from the weighted sum {float(err[want[:, :3] != 0].max()):.3g}")
    np.testing.assert_allclose(got[:, :3], want[:, :3], rtol=1e-5, atol=0)
    assert np.array_equal(fb[~hit], f1[~hit]) and np.array_equal(f1[~hit], f2[~hit])
