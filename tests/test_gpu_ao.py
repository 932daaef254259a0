"""Ambient occlusion of the direct lighting integrator on the DEVICE (DirectLightIntegrator::integrate, integrator_direct_light.cc:130-146;
MonteCarloIntegrator::sampleAmbientOcclusion, integrator_montecarlo.cc:1030-1088).

The expected values are a float32 restatement of sampleAmbientOcclusion written here on top of the oracle's leaf functions, which other
tests hold bit for bit to the reference's golden vectors: Material::sample with a flag set (yor_material_probe), Material::emit
(yor_lightmat_emit), the Halton sequences (yor_halton_seq, yor_scr_halton), fnv32a, the camera (yor_camera_shoot) and the closest hit
(yor_intersect).  Shadow verdicts are the device's own ray batches (shadowRays: the same wf_trace, pinned against brute force in
tests/test_gpu_parity.py), so no pixel has to be left out for a grazing ray: every comparison covers all pixels.

A sample whose contribution is exactly zero goes without a shadow ray on the device ("Ambient occlusion"); the ray counts
below are the restatement's under that rule."""
import ctypes as C

import numpy as np
import pytest

from libyafaray_amd import Interface, scenes
from oracle import pyoracle as po
from tests.test_gpu_components import exact

pytestmark = pytest.mark.gpu

F = np.float32
M32 = 0xffffffff
K_AO_FLAGS = 0x16           # BsdfGlossy | BsdfDiffuse | BsdfReflect (integrator_montecarlo.cc:1069)
K_GLOSSY_FLAGS = 0x12       # BsdfGlossy | BsdfReflect (recursiveRaytrace's glossy branch, :890)
BSDF_DIFFUSE, BSDF_GLOSSY, BSDF_EMIT = 0x4, 0x2, 0x80
ATOL = 1e-4                 # the project's parity tolerance, device against oracle (README)


@pytest.fixture(scope="module", autouse=True)
def torch_first():
    """(as in the other GPU modules: let torch open the GPU before the library does)"""
    import torch
    torch.cuda.init()


# ---- float32 helpers in the reference's operation order --------------------------------------------------------------
def dot(a, b):
    return F(F(F(a[0] * b[0]) + F(a[1] * b[1])) + F(a[2] * b[2]))       # vector.h:154


def length(v):
    return F(po.lib().yor_fsqrt(float(dot(v, v))))                        # vector.h:222


def add_mod_1(x, y):
    t = F(F(x) + F(y))                                                    # util_sample.h:183-187
    return F(t - F(1)) if t > 1 else t


def halton(base, start, count):
    out = np.zeros(count, F)
    po.lib().yor_halton_seq(base, start & M32, count, po.fptr(out))
    return out


def fnv(v):
    return int(po.lib().yor_fnv32a(v & M32))


def sampling_offs(px, py):
    return fnv((py * fnv(px)) & M32)                                      # integrator_tiled.cc:386


# ---- the restatement -------------------------------------------------------------------------------------------------
def ao_leaf(md, p, n, ng, wo, s_1, s_2, bias_auto, bias, dist, col):
    """One turn of sampleAmbientOcclusion's loop (:1053-1084) up to the shadow test: the ray, what it adds if it is not shadowed
    (ao_col * surf_col * cos * w, left to right, :1081-1083), emit() * pdf (:1072-1075).  -> wanted, dir, tmin, tmax, contribution, emission"""
    L = po.lib()
    tmin = F(F(bias) * max(F(1), length(p))) if bias_auto else F(bias)   # :1062-1063
    inp = np.array([*n, *ng, *wo, 0, 0, 0, s_1, s_2], F)
    e = np.zeros(3, F); s8 = np.zeros(8, F)
    bf, pdf, so = C.c_int32(), C.c_float(), C.c_int32()
    L.yor_material_probe(C.byref(md), po.fptr(inp), K_AO_FLAGS, C.byref(bf), po.fptr(e), C.byref(pdf), C.byref(so), po.fptr(s8))
    surf, d, spdf, w = s8[0:3].copy(), s8[3:6].copy(), F(s8[6]), F(s8[7])
    emit = np.zeros(3, F)
    if bf.value & BSDF_EMIT:
        em = np.zeros(3, F)
        L.yor_lightmat_emit(C.byref(md), po.fptr(np.array(n, F)), po.fptr(np.array(wo, F)), 1, po.fptr(em))
        emit = (em * spdf).astype(F)
    cos = F(abs(dot(n, d)))
    with np.errstate(all="ignore"):
        contrib = (((np.asarray(col, F) * surf).astype(F) * cos).astype(F) * w).astype(F)
    wanted = not (contrib == 0).all()
    return wanted, d, tmin, F(dist), contrib, emit, bf.value


class Restatement:
    """sampleAmbientOcclusion at the vertices of one scene / render description; `yi` is the device interface of the same scene
    (prepared), asked for the shadow verdicts and for the settings createIntegrator parsed"""

    def __init__(self, sc, rd, yi):
        self.sc, self.rd, self.yi = sc, rd, yi
        self.osc = po.OracleScene(sc)
        self.cam = po.camera_desc(sc["camera"])
        self.md = [po.material_desc(m) for m in sc["materials"]]
        v = np.asarray(sc["verts"], F).reshape(-1, 3, 3)
        ng = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]).astype(F)
        ng /= np.linalg.norm(ng, axis=1, keepdims=True).astype(F)
        assert (np.sort(np.abs(ng), axis=1)[:, :2] == 0).all(), "the scenes of this module are axis-aligned: their normals are exact"
        self.ng = ng.astype(F)
        ao = yi.getIntegratorAO("default")
        self.ao_n, self.ao_dist, self.ao_col = ao["AO_samples"], F(ao["AO_distance"]), ao["AO_color"]
        self.bias_auto = bool(rd.get("adv_auto_shadow_bias_enabled", True))
        self.bias = F(0.0005) if self.bias_auto else F(rd.get("adv_shadow_bias_value", 0.0005))
        self.base = int(rd.get("adv_base_sampling_offset", 0)) + 100000 * int(rd.get("adv_computer_node", 0))
        self.n_rays = 0

    # -- the camera samples of a render: [(film pixels it is added to, pixel_sample, sampling_offs, from, dir, tmin, tmax)], pixel by pixel
    def camera_samples(self):
        L = po.lib()
        rd = self.rd
        spp, passes = int(rd.get("AA_minsamples", 1)), int(rd.get("AA_passes", 1))
        inc = int(rd.get("AA_inc_samples", spp))
        schedule = [(0, spp)] + [(spp + k * inc, inc) for k in range(passes - 1)]          # (pass_offset, samples): every pixel again (AA_threshold 0)
        assert passes == 1 or rd.get("AA_threshold") == 0.0
        out9 = np.zeros(9, F)
        for py in range(rd.get("ystart", 0), rd.get("ystart", 0) + rd["height"]):
            for px in range(rd.get("xstart", 0), rd.get("xstart", 0) + rd["width"]):
                so = sampling_offs(px, py)
                for pass_offset, n in schedule:
                    for s in range(n):
                        pixel_sample = (self.base + pass_offset + s) & M32                 # integrator_tiled.cc:389
                        if passes > 1:                                                     # :394-398
                            dx, dy = F(L.yor_ri_vdc(pixel_sample, so)), F(L.yor_ri_s(pixel_sample, so))
                        elif n > 1:                                                        # :399-403
                            d_1 = F(1.0 / float(F(n)))
                            dx, dy = F((0.5 + float(F(s))) * float(d_1)), F(L.yor_ri_lp((s + so) & M32, 0))
                        else:
                            dx, dy = F(0.5), F(0.5)
                        L.yor_camera_shoot(C.byref(self.cam), F(F(px) + dx), F(F(py) + dy), po.fptr(out9))
                        # ImageFilm::addSample with the box filter of half-width 0.501 (imagefilm.cc:925-1015): the pixel itself, and the
                        # right / lower neighbour too when the sample lies within 0.001 of that edge
                        edge = lambda d: int(float(d) + float(F(0.501)) - 1.0 + (0.5 - 1.4e-11)) >= 1
                        pixels = [(py + j, px + i) for j in range(1 + edge(dy)) for i in range(1 + edge(dx))]
                        pixels = [(y - rd.get("ystart", 0), x - rd.get("xstart", 0)) for y, x in pixels]
                        pixels = [(y, x) for y, x in pixels if y < rd["height"] and x < rd["width"]]
                        yield pixels, pixel_sample, so, out9[0:3].copy(), out9[3:6].copy(), float(out9[6]), float(out9[7])

    def vertex(self, frm, dr, t, tri):
        return dict(p=(frm + (dr * F(t)).astype(F)).astype(F), n=self.ng[tri], ng=self.ng[tri], wo=(-dr).astype(F), mat=int(self.sc["tri_mat"][tri]))

    def hit(self, frm, dr, tmin, tmax):
        h, tri, t, _ = self.osc.intersect(frm, dr, tmin, tmax, use_tree=False)
        return self.vertex(frm, dr, t, tri) if h else None

    def candidates(self, v, pixel_sample, so, division=1, dc=(F(0), F(0))):
        """the samples of one sampleAmbientOcclusion call (:1040-1060): None where the material has no diffuse component
        (integrator_direct_light.cc:130), else (n, [(wanted, ray8, contribution, emission)])"""
        n = self.ao_n
        if division > 1:
            n = max(1, n // division)
        offs = (n * pixel_sample + so) & M32
        h_2, h_3 = halton(2, offs - 1, n), halton(3, offs - 1, n)
        out = []
        for i in range(n):
            s_1, s_2 = h_2[i], h_3[i]
            if division > 1:
                s_1, s_2 = add_mod_1(s_1, dc[0]), add_mod_1(s_2, dc[1])
            wanted, d, tmin, tmax, contrib, emit, bsdfs = ao_leaf(self.md[v["mat"]], v["p"], v["n"], v["ng"], v["wo"], s_1, s_2,
                                                                 self.bias_auto, self.bias, self.ao_dist, self.ao_col)
            if not bsdfs & BSDF_DIFFUSE:
                return None
            out.append((wanted, np.array([*v["p"], *d, tmin, tmax], F), contrib, emit))
        return n, out

    def evaluate(self, calls):
        """calls: a list of candidates() results -> the value of each call (col / (float)n, :1087; zeros for None); one shadow batch"""
        rays = [c[1] for call in calls if call for c in call[1] if c[0]]
        self.n_rays += len(rays)
        sh = iter(self.yi.shadowRays(np.array(rays, F)) if rays else [])
        vals = []
        for call in calls:
            acc = np.zeros(3, F)
            if call:
                for wanted, _, contrib, emit in call[1]:
                    acc = (acc + emit).astype(F)
                    if wanted and not next(sh):
                        acc = (acc + contrib).astype(F)
                acc = (acc / F(call[0])).astype(F)
            vals.append(acc)
        return vals

    def primary_film(self):
        """sum of the AO term of every camera sample per pixel (level 0 only: scenes without recursion), as the film adds them"""
        rd = self.rd
        keys, calls = [], []
        for pixels, ps, so, frm, dr, tmin, tmax in self.camera_samples():
            v = self.hit(frm, dr, tmin, tmax)
            keys.append(pixels)
            calls.append(self.candidates(v, ps, so) if v else None)
        film = np.zeros((rd["height"], rd["width"], 3), F)
        for pixels, val in zip(keys, self.evaluate(calls)):
            for y, x in pixels:
                film[y, x] = (film[y, x] + val).astype(F)
        return film


# ---- scenes ----------------------------------------------------------------------------------------------------------
CLAY = {"type": "shinydiffusemat", "color": (0.8, 0.8, 0.8), "diffuse_reflect": 1.0}


def box(x0, y0, z0, x1, y1, z1, bottom=False):
    """the faces of an axis-aligned box, outward normals: 10 triangles (12 with the bottom)"""
    q = scenes._quad
    f = [q((x0, y0, z1), (x1, y0, z1), (x1, y1, z1), (x0, y1, z1)), q((x0, y0, z0), (x1, y0, z0), (x1, y0, z1), (x0, y0, z1)),
         q((x1, y0, z0), (x1, y1, z0), (x1, y1, z1), (x1, y0, z1)), q((x1, y1, z0), (x0, y1, z0), (x0, y1, z1), (x1, y1, z1)),
         q((x0, y1, z0), (x0, y0, z0), (x0, y0, z1), (x0, y1, z1))]
    if bottom:
        f.append(q((x0, y0, z0), (x0, y1, z0), (x1, y1, z0), (x1, y0, z0)))
    return np.concatenate(f)


def clay_scene(res=(24, 16), lights=(), extra=(), plane_mat=None, box_mat=None, with_box=True, cam=None):
    """a 4 x 4 plane at z = 0 and a small box resting on it, seen from above at an angle: 12 triangles, every normal along an axis"""
    verts = [scenes._quad((-2, -2, 0), (2, -2, 0), (2, 2, 0), (-2, 2, 0))]
    mats, materials = [0, 0], [plane_mat or CLAY]
    if with_box:
        verts.append(box(-0.3, -0.2, 0.0, 0.35, 0.3, 0.4)); mats += [1] * 10; materials.append(box_mat or dict(CLAY, color=(0.7, 0.5, 0.3)))
    for v, m in extra:
        verts.append(np.asarray(v, F).reshape(-1, 3, 3)); mats += [len(materials)] * len(verts[-1]); materials.append(m)
    camera = dict({"type": "perspective", "from": (0.3, -2.0, 1.6), "to": (0.0, 0.0, 0.1), "up": (0.3, -2.0, 2.6), "resx": res[0], "resy": res[1], "focal": 1.1},
                  **(cam or {}))
    return {"verts": np.concatenate(verts).astype(F), "tri_mat": np.array(mats, np.int32), "vnormals": None, "materials": materials,
            "lights": list(lights), "camera": camera}


def settings(res=(24, 16), spp=1, integrator="directlighting", **kw):
    return scenes.render_settings(res[0], res[1], spp, integrator=integrator, tile_size=8, **kw)


def device(sc, rd, shard=None, replay=None):
    yi = Interface()
    scenes.load_scene(yi, sc, rd)
    if replay is not None:
        yi.setSerialReplay(replay)
    if shard:
        yi.setShard(*shard)
    yi.render()
    return yi.getFilm(rd["width"], rd["height"]), yi


def check(film, want_sum, what):
    """film: the device's (h, w, 5) sums; want_sum: the expected colour sums.  Pixel::normalized of both, 1e-4 absolute, all pixels"""
    w = film[..., 4:5]
    assert (w > 0).all()
    dev = float(np.abs(film[..., :3] / w - want_sum / w).max())
    print(f"{what}: largest deviation {dev:.3g} (bit-exact pixels {float((film[..., :3] == want_sum).all(axis=-1).mean()):.4f})")
    assert dev <= ATOL, f"{what}: {dev}"
    return dev


# ---- 1. the leaf, bit for bit ----------------------------------------------------------------------------------------
LEAF_MATERIALS = [
    ("shinydiffuse", {"type": "shinydiffusemat", "color": (0.8, 0.6, 0.4), "diffuse_reflect": 0.9}),
    ("shinydiffuse, emitting", {"type": "shinydiffusemat", "color": (0.8, 0.6, 0.4), "diffuse_reflect": 0.9, "emit": 0.5}),
    ("Oren-Nayar", {"type": "shinydiffusemat", "color": (0.5, 0.7, 0.9), "diffuse_reflect": 1.0, "diffuse_brdf": "oren_nayar", "sigma": 0.3}),
    ("glossy", {"type": "glossy", "color": (0.9, 0.8, 0.7), "diffuse_color": (0.6, 0.6, 0.7), "diffuse_reflect": 0.4, "glossy_reflect": 0.6,
                "exponent": 40.0, "as_diffuse": False}),
    ("coated glossy", {"type": "coated_glossy", "color": (0.9, 0.8, 0.7), "diffuse_color": (0.3, 0.6, 0.4), "mirror_color": (0.9, 0.9, 1.0),
                       "diffuse_reflect": 0.5, "glossy_reflect": 0.5, "exponent": 60.0, "IOR": 1.5, "as_diffuse": False}),
]


# a material with shader nodes and bump.  Its texture is one colour all over, so what the nodes resolve to is known without restating them:
# the diffuse shader gives that colour wherever the point lies, and the bump shader's derivative is zero, which sends the frame through
# Material::applyBump and leaves it where it was on a triangle whose normal lies along an axis.  The restatement is therefore that of
# NODE_PLAIN; the device has to get there through the triangle's texture coordinates, evalBump, applyBump and the node stack.
NODE_TEXEL = (0.5, 0.25, 0.75, 1.0)
_layer = dict(type="layer", mode=0, def_val=1.0, upper_value=0.0)
NODE_MATERIAL = {"type": "shinydiffusemat", "color": (0.8, 0.8, 0.8), "diffuse_reflect": 0.9, "diffuse_shader": "diff", "bump_shader": "bmp",
                 "nodes": [dict(_layer, name="diff", input="map", colfac=1.0, def_col=(1.0, 0.0, 1.0, 1.0), do_color=True, do_scalar=False, color_input=True,
                                upper_color=(0.8, 0.8, 0.8, 1.0)),
                           dict(name="map", type="texture_mapper", texture="t_flat", texco="uv", mapping="plain"),
                           dict(_layer, name="bmp", input="bmap", valfac=1.0, do_color=False, do_scalar=True, color_input=False),
                           dict(name="bmap", type="texture_mapper", texture="t_flat", texco="uv", mapping="plain", bump_strength=2.0)]}
NODE_PLAIN = {"type": "shinydiffusemat", "color": NODE_TEXEL[:3], "diffuse_reflect": 0.9}
FLAT_TEXTURE = dict(name="t_flat", texels=np.broadcast_to(np.array(NODE_TEXEL, F), (4, 4, 4)).copy(), interpolate="none", clipping="repeat", color_space="LinearRGB")


def leaf_inputs(N, seed):
    rng = np.random.default_rng(seed)
    unit = lambda a: (a / np.linalg.norm(a, axis=1, keepdims=True)).astype(F)
    p = rng.uniform(-5, 5, (N, 3)).astype(F)
    p[::2] *= F(0.1)                                           # |p| < 1: the automatic bias takes max(1, |p|)
    n = unit(rng.normal(size=(N, 3)))
    ng = n.copy()
    ng[N // 2:] = unit(n[N // 2:] + rng.normal(0, 0.2, (N - N // 2, 3)))
    wo = unit(rng.normal(size=(N, 3)))
    wo[:N // 4] = unit(n[:N // 4] + rng.normal(0, 0.6, (N // 4, 3)))      # mostly above the surface, some below
    s = rng.random((N, 2)).astype(F)
    s[:20, 0] = 0
    return p, n, ng, wo, s


@pytest.mark.parametrize("bias_auto", [True, False])
def test_leaf_bit_for_bit(bias_auto):
    N = 2000
    tris = np.stack([np.array([[k, 0, 0], [k + 0.5, 0, 0], [k, 0.5, 0]], F) for k in range(len(LEAF_MATERIALS))])
    K_NODE = len(LEAF_MATERIALS)                          # the sixth material and its triangle
    tris = np.concatenate([tris, np.array([[[K_NODE, 0, 0], [K_NODE + 0.5, 0, 0], [K_NODE, 0.5, 0]]], F)])
    sc = {"verts": tris, "tri_mat": np.arange(K_NODE + 1, dtype=np.int32), "vnormals": None, "materials": [m for _, m in LEAF_MATERIALS] + [NODE_MATERIAL],
          "uv": np.random.default_rng(3).uniform(0, 1, (K_NODE + 1, 3, 2)).astype(F), "textures": [FLAT_TEXTURE],
          "lights": [], "camera": {"type": "perspective", "from": (0.0, 0.0, 5.0), "to": (0.0, 0.0, 0.0), "up": (0.0, 1.0, 5.0), "resx": 8, "resy": 8}}
    yi = Interface()
    scenes.load_scene(yi, sc, settings((8, 8)))
    yi.prepareRender()
    bias = F(0.0005) if bias_auto else F(0.003)
    dist, col = F(0.7), np.array([0.9, 0.5, 0.25], F)
    for k, (name, m) in enumerate(LEAF_MATERIALS):
        md = po.material_desc(m)
        p, n, ng, wo, s = leaf_inputs(N, 100 + k)
        assert 0.05 < (np.einsum("ij,ij->i", ng, wo) < 0).mean() < 0.95
        tail = np.broadcast_to(np.array([1.0 if bias_auto else 0.0, bias, dist, *col], F), (N, 6))
        got = yi.probe(26, np.hstack([np.full((N, 1), np.uint32(k)).view(F), p, n, ng, wo, s, tail]), 12)
        want = np.zeros((N, 12), F)
        for i in range(N):
            wanted, d, tmin, tmax, contrib, emit, _ = ao_leaf(md, p[i], n[i], ng[i], wo[i], s[i, 0], s[i, 1], bias_auto, bias, dist, col)
            want[i] = [wanted, *d, tmin, tmax, *contrib, *emit]
        assert 0.2 < want[:, 0].mean(), name
        if "emit" in m:
            assert (want[:, 9:] > 0).any(), "the emission quirk is not exercised"
        else:
            assert (want[:, 9:] == 0).all()
        exact(got, want.view(np.uint32), f"ao_candidate, {name}, {'automatic' if bias_auto else 'fixed'} bias")
    # the material with shader nodes and bump, at points of its own triangle (normal +z): the probe's triangle path
    md = po.material_desc(NODE_PLAIN)
    p, _, _, wo, s = leaf_inputs(N, 100 + K_NODE)
    n = np.broadcast_to(np.array([0, 0, 1], F), (N, 3))
    bary = np.random.default_rng(9).dirichlet((1, 1, 1), N).astype(F)
    tail = np.broadcast_to(np.array([1.0 if bias_auto else 0.0, bias, dist, *col], F), (N, 6))
    where = np.hstack([np.full((N, 1), np.uint32(K_NODE)).view(F), bary[:, 1:3]])
    got = yi.probe(26, np.hstack([np.full((N, 1), np.uint32(K_NODE)).view(F), p, n, n, wo, s, tail, where]), 12)
    want = np.zeros((N, 12), F)
    for i in range(N):
        wanted, d, tmin, tmax, contrib, emit, _ = ao_leaf(md, p[i], n[i], n[i], wo[i], s[i, 0], s[i, 1], bias_auto, bias, dist, col)
        want[i] = [wanted, *d, tmin, tmax, *contrib, *emit]
    assert 0.2 < want[:, 0].mean()
    exact(got, want.view(np.uint32), f"ao_candidate, shader nodes and bump, {'automatic' if bias_auto else 'fixed'} bias")
    # ... and without the triangle the same material index gives the unresolved material (its own colour): the path above is the one that ran
    base = yi.probe(26, np.hstack([np.full((N, 1), np.uint32(K_NODE)).view(F), p, n, n, wo, s, tail]), 12)
    assert not np.array_equal(base[:, 6:9], got[:, 6:9])


# ---- 2. clay render without lights, 9. ray counts -----------------------------------------------------------------------
@pytest.mark.parametrize("n_samples", [1, 3, 32])
def test_clay_render_without_lights(n_samples):
    """measured on the MI355X: see DESIGN.md "Ambient occlusion" (the largest deviation over the three cases)"""
    sc = clay_scene()
    rd = settings(do_AO=True, AO_samples=n_samples, AO_distance=0.6, AO_color=(0.9, 0.8, 0.7))
    film, yi = device(sc, rd)
    r = Restatement(sc, rd, yi)
    want = r.primary_film()
    assert want.max() > 0.3 and (want.reshape(-1, 3).max(axis=1) == 0).any()       # lit clay, and shadowed or empty pixels
    check(film, want, f"clay, AO_samples {n_samples}")
    # every sample with a contribution sent one shadow ray, and nothing else did
    st = yi.getRenderStats()
    assert st.rays_shadow == r.n_rays and r.n_rays >= (want.reshape(-1, 3).max(axis=1) > 0).sum()
    assert st.rays_closest == st.camera_samples == 24 * 16
    # the occlusion shows: without the box the film is brighter next to where it stood
    open_film, _ = device(clay_scene(with_box=False), rd)
    assert (open_film[..., :3] - film[..., :3]).max() > 0.05


# ---- 3. invariants, bit for bit ----------------------------------------------------------------------------------------
POINT = {"type": "pointlight", "from": (0.8, -0.9, 1.5), "color": (1.0, 0.9, 0.8), "power": 4.0}


def test_black_ao_color_is_no_ao():
    sc = clay_scene(lights=[POINT])
    off, _ = device(sc, settings(spp=2))
    black, _ = device(sc, settings(spp=2, do_AO=True, AO_samples=5, AO_distance=0.6, AO_color=(0.0, 0.0, 0.0)))
    assert off[..., :3].max() > 0.1 and np.array_equal(off, black)


def test_occluder_beyond_the_distance_changes_nothing():
    rd = settings(do_AO=True, AO_samples=8, AO_distance=0.6)
    lid = scenes._quad((-3, -3, 3.0), (-3, 3, 3.0), (3, 3, 3.0), (3, -3, 3.0))          # above the camera, 2.6 above the box's top
    plain, _ = device(clay_scene(), rd)
    far, _ = device(clay_scene(extra=[(lid, CLAY)]), rd)
    assert plain[..., :3].max() > 0.3 and np.array_equal(plain, far)


def test_a_closed_room_nearer_than_the_distance_leaves_no_ao():
    """the plane is the floor of a closed room around the camera: every AO ray ends on a wall within AO_distance"""
    room = box(-2.5, -2.5, 0, 2.5, 2.5, 3)[:, ::-1, :]                                   # facing inward
    sc = clay_scene(lights=[POINT], extra=[(room, dict(CLAY, color=(0.5, 0.5, 0.6)))], with_box=False)
    off, _ = device(sc, settings())
    on, yi = device(sc, settings(do_AO=True, AO_samples=8, AO_distance=100.0))
    assert off[..., :3].max() > 0.1 and yi.getRenderStats().rays_shadow > 8 * 0.9 * 24 * 16
    assert np.array_equal(off, on)


def test_doubling_the_ao_color_doubles_the_film():
    sc = clay_scene()
    one, _ = device(sc, settings(do_AO=True, AO_samples=6, AO_distance=0.6, AO_color=(0.4, 0.3, 0.2)))
    two, _ = device(sc, settings(do_AO=True, AO_samples=6, AO_distance=0.6, AO_color=(0.8, 0.6, 0.4)))
    assert one[..., :3].max() > 0.1 and np.array_equal(one[..., :3] * F(2), two[..., :3]) and np.array_equal(one[..., 3:], two[..., 3:])


# ---- 4. with lights ------------------------------------------------------------------------------------------------------
def test_ao_follows_the_lights():
    """an area light and a point light, then AO: the oracle's film of the scene WITHOUT AO plus the composed AO term — (col + direct) + ao,
    integrator_direct_light.cc:132-145.  The point light casts no shadows and the plane receives none: AO is occluded all the same (:1077)"""
    z = 1.9
    lamp = scenes._quad((-0.3, -0.3, z), (-0.3, 0.3, z), (0.3, 0.3, z), (0.3, -0.3, z))
    lights = [{"type": "arealight", "corner": (-0.3, -0.3, z), "point1": (-0.3, 0.3, z), "point2": (0.3, -0.3, z), "color": (1.0, 1.0, 1.0), "power": 6.0, "samples": 2},
              dict(POINT, cast_shadows=False)]
    sc = clay_scene(lights=lights, plane_mat=dict(CLAY, receive_shadows=False), extra=[(lamp, {"type": "light_mat", "color": (1.0, 1.0, 1.0), "power": 6.0})])
    rd_off = settings(spp=2)
    rd = dict(rd_off, do_AO=True, AO_samples=4, AO_distance=0.6, AO_color=(0.5, 0.6, 0.7))
    film, yi = device(sc, rd)
    ofilm, ost = po.OracleScene(sc).render(rd_off)
    assert np.array_equal(film[..., 4], ofilm[..., 4])
    r = Restatement(sc, rd, yi)
    ao = r.primary_film()
    check(film, ofilm[..., :3] + ao, "area + point light + AO")
    st = yi.getRenderStats()
    assert st.rays_shadow == ost.rays_shadow + r.n_rays
    # what the comparison holds: leaving AO's occlusion out, or AO itself, misses the tolerance by far
    assert np.abs(ao / ofilm[..., 4:5]).max() > 100 * ATOL


# ---- 7. schedules ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["two passes", "crop window", "sampling offset"])
def test_schedules(case):
    res, kw, cam = (24, 16), {}, None
    if case == "two passes":
        kw = dict(AA_passes=2, AA_inc_samples=2, AA_threshold=0.0)
    elif case == "crop window":
        res, kw, cam = (14, 9), dict(xstart=7, ystart=4), dict(resx=24, resy=16)
    else:
        kw = dict(adv_base_sampling_offset=7, adv_computer_node=1)
    sc = clay_scene(cam=cam)
    rd = settings(res, spp=2, do_AO=True, AO_samples=3, AO_distance=0.6, **kw)
    film, yi = device(sc, rd)
    assert film[..., 4].sum() >= (4 if case == "two passes" else 2) * res[0] * res[1]
    check(film, Restatement(sc, rd, yi).primary_film(), f"clay, {case}")


def test_shards_and_serial_replay_are_bit_for_bit():
    """AO has no serial state: two tile shards add up to the unsharded film, and the serial-state replay switch changes nothing"""
    sc = clay_scene(lights=[POINT])
    rd = settings(spp=2, do_AO=True, AO_samples=5, AO_distance=0.6)
    full, yi = device(sc, rd)
    parts = [device(sc, rd, shard=(r, 2)) for r in range(2)]
    assert all(p[0][..., 4].any() for p in parts)
    assert np.array_equal(parts[0][0] + parts[1][0], full)
    assert sum(p[1].getRenderStats().rays_shadow for p in parts) == yi.getRenderStats().rays_shadow
    for replay in (True, False):
        assert np.array_equal(device(sc, rd, replay=replay)[0], full)


# ---- 8. path tracing ignores it ----------------------------------------------------------------------------------------------
def test_path_tracing_ignores_do_ao():
    sc = clay_scene(lights=[POINT])
    rd = settings(spp=2, integrator="pathtracing", bounces=3)
    off, y0 = device(sc, rd)
    on, y1 = device(sc, dict(rd, do_AO=True, AO_samples=4, AO_distance=0.6))
    assert off[..., :3].max() > 0.1 and off.tobytes() == on.tobytes()
    assert y0.getRenderStats().rays_shadow == y1.getRenderStats().rays_shadow


# ---- 5. recursion and trajectory splitting ----------------------------------------------------------------------------------
def traced_queries(sc, rd_off):
    """the oracle's render of the scene WITHOUT AO, with every closest-hit query it made: film, stats, {(px, py): [query rows]} in call order
    (depth first, as recursiveRaytrace walks its calls); 1 spp"""
    n_px = rd_off["width"] * rd_off["height"]
    ofilm, ost, _, rays, total = po.OracleScene(sc).render_traced(rd_off, n_px, 16 * n_px)
    assert total == len(rays)
    per = {}
    for q in rays:
        per.setdefault((int(q[10]), int(q[11])), []).append(q)
    return ofilm, ost, per


def query_vertex(r, q):
    tri = int(q[9:10].view(np.int32)[0])
    return r.vertex(q[0:3].copy(), q[3:6].copy(), q[8], tri) if q[8] >= 0 else None


def test_mirror_gives_ao_at_level_one():
    """a mirror behind the box, facing the camera: where the camera sees the mirror, AO runs at the reflected ray's hit only (the mirror has
    no diffuse component) and comes back scaled by the mirror's colour (recursiveRaytrace, integrator_montecarlo.cc:980-990)"""
    L = po.lib()
    mirror = scenes._quad((-1.2, 1.0, 0.0), (1.2, 1.0, 0.0), (1.2, 1.0, 1.2), (-1.2, 1.0, 1.2))
    sc = clay_scene(lights=[POINT], extra=[(mirror, {"type": "mirror", "color": (0.9, 0.8, 0.7), "reflect": 0.8})])
    i_mirror = len(sc["materials"]) - 1
    rd_off = settings(raydepth=2)
    rd = dict(rd_off, do_AO=True, AO_samples=4, AO_distance=0.6)
    film, yi = device(sc, rd)
    ofilm, ost, per = traced_queries(sc, rd_off)
    r = Restatement(sc, rd, yi)
    keys, calls, scale = [], [], []
    for (px, py), qs in per.items():
        ps, so = r.base & M32, sampling_offs(px, py)
        v0 = query_vertex(r, qs[0])
        if v0 is None:
            continue
        v, mcol = v0, np.ones(3, F)
        if v0["mat"] == i_mirror:
            assert len(qs) == 2
            flags, out12, alpha = C.c_int32(), np.zeros(12, F), C.c_float()
            L.yor_material_specular(C.byref(r.md[i_mirror]), po.fptr(np.array([*v0["n"], *v0["ng"], *v0["wo"], 0, 0, 0, 0, 0], F)), 1,
                                    C.byref(flags), po.fptr(out12), C.byref(alpha))
            assert flags.value & 1 and np.array_equal(out12[0:3], qs[1][3:6])              # the reflected ray is the one the oracle traced
            v, mcol = query_vertex(r, qs[1]), out12[3:6].copy()
        else:
            assert len(qs) == 1
        if v is not None:
            keys.append((py, px)); calls.append(r.candidates(v, ps, so)); scale.append(mcol)
    assert sum(1 for m in scale if not (m == 1).all()) > 20, "the camera should see the mirror"
    want = ofilm[..., :3].copy()
    for (y, x), val, m in zip(keys, r.evaluate(calls), scale):
        want[y, x] = (want[y, x] + (val * m).astype(F)).astype(F)
    check(film, want, "mirror: AO at level 1")
    assert yi.getRenderStats().rays_shadow == ost.rays_shadow + r.n_rays
    assert np.abs(want - ofilm[..., :3]).max() > 100 * ATOL


def test_trajectory_splitting_divides_the_samples():
    """a glossy floor whose recursion splits the trajectory eight ways (recursiveRaytrace's glossy branch, :861-918): below it
    ray_division_ is 8, so AO_samples = 3 becomes max(1, 3 / 8) = 1 (:1041) and its sample is rotated by dc_1_ / dc_2_ (:1056-1060)"""
    L = po.lib()
    floor = {"type": "glossy", "color": (0.9, 0.9, 0.9), "diffuse_color": (0.6, 0.6, 0.7), "diffuse_reflect": 0.5, "glossy_reflect": 0.5,
             "exponent": 30.0, "as_diffuse": False}
    sc = clay_scene(lights=[POINT], plane_mat=floor)
    rd_off = settings(raydepth=1)
    rd = dict(rd_off, do_AO=True, AO_samples=3, AO_distance=0.6)
    film, yi = device(sc, rd)
    ofilm, ost, per = traced_queries(sc, rd_off)
    r = Restatement(sc, rd, yi)
    keys, calls, scale = [], [], []                       # one entry per AO call: its pixel, its samples, what its value is multiplied by
    n_split = 0
    for (px, py), qs in per.items():
        ps, so = r.base & M32, sampling_offs(px, py)
        v0 = query_vertex(r, qs[0])
        if v0 is None:
            continue
        keys.append((py, px)); calls.append(r.candidates(v0, ps, so)); scale.append((np.ones(3, F), F(1), F(1)))
        if v0["mat"] != 0:
            assert len(qs) == 1
            continue
        assert len(qs) == 9
        offs = (8 * ps + so) & M32                                                         # :875 (gsam = 8, started at offs)
        h_2, h_3 = halton(2, offs, 8), halton(3, offs, 8)
        for ns in range(8):
            s8, e = np.zeros(8, F), np.zeros(3, F)
            bf, pdf, sf = C.c_int32(), C.c_float(), C.c_int32()
            L.yor_material_probe(C.byref(r.md[0]), po.fptr(np.array([*v0["n"], *v0["ng"], *v0["wo"], 0, 0, 0, h_2[ns], h_3[ns]], F)), K_GLOSSY_FLAGS,
                                 C.byref(bf), po.fptr(e), C.byref(pdf), C.byref(sf), po.fptr(s8))
            assert np.array_equal(s8[3:6], qs[1 + ns][3:6])                                # the trajectory the oracle traced
            v1 = query_vertex(r, qs[1 + ns])
            if v1 is None:
                continue
            dc = (F(L.yor_scr_halton(3, (ns + so) & M32)), F(L.yor_scr_halton(4, (ns + so) & M32)))      # :886-887 at raylevel 1, branch = ns
            call = r.candidates(v1, ps, so, division=8, dc=dc)
            if call:
                assert call[0] == 1
                n_split += 1
                keys.append((py, px)); calls.append(call); scale.append((s8[0:3].copy(), F(s8[7]), F(1.0) / F(8)))
    assert n_split > 50, "the trajectories should reach the box and the floor"
    want = ofilm[..., :3].copy()
    for (y, x), val, (mcol, w, g) in zip(keys, r.evaluate(calls), scale):
        want[y, x] = (want[y, x] + (((val * mcol).astype(F) * w).astype(F) * g).astype(F)).astype(F)      # gcol += integ * mcol * w; col += gcol / gsam
    check(film, want, "trajectory splitting")
    assert yi.getRenderStats().rays_shadow == ost.rays_shadow + r.n_rays


# ---- 6. transparent shadows -----------------------------------------------------------------------------------------------
def fin_scene(room_mat=None):
    """the plane, a thin wall standing on it and, with room_mat, a closed room of that material around all of it and the camera: convex,
    so every ray that leaves the plane or the wall without meeting the other crosses the room exactly once"""
    fin = scenes._quad((-0.2, 0.1, 0.0), (0.4, 0.1, 0.0), (0.4, 0.1, 0.5), (-0.2, 0.1, 0.5))
    extra = [(fin, dict(CLAY, color=(0.7, 0.5, 0.3)))]
    if room_mat:
        extra.append((box(-2, -2, 0, 2, 2, 1.5)[:, ::-1, :], room_mat))
    return clay_scene(extra=extra, with_box=False, cam={"from": (0.0, -1.5, 1.2), "to": (0.0, 0.0, 0.0), "up": (0.0, -1.5, 2.2)})


def glass_sheet(color):
    return {"type": "shinydiffusemat", "color": color, "transparency": 1.0, "diffuse_reflect": 0.0, "transmit_filter": 1.0}


def test_transparent_shadows_filter_ao():
    rd = settings(do_AO=True, AO_samples=6, AO_distance=10.0, transpShad=True, shadowDepth=3)
    bare, _ = device(fin_scene(), rd)
    assert bare[..., :3].max() > 0.3 and (bare[..., 4] == 1).all() and (bare[..., 3] == 1).all()       # the camera sees the plane and the wall only
    white, yi = device(fin_scene(glass_sheet((1.0, 1.0, 1.0))), rd)
    assert yi.getRenderStats().rays_shadow > 0
    assert np.array_equal(white[..., :3], bare[..., :3]), "a white filter must leave AO as it is, bit for bit"
    c = np.array([0.9, 0.5, 0.25], F)
    tinted, _ = device(fin_scene(glass_sheet(tuple(float(x) for x in c))), rd)
    check(tinted, bare[..., :3] * c, "AO through a tinted sheet")
    # one surface crossed, none allowed: the sheet blocks every ray that the scene itself let pass
    blocked, _ = device(fin_scene(glass_sheet((0.9, 0.5, 0.25))), dict(rd, shadowDepth=0))
    off, _ = device(fin_scene(glass_sheet((0.9, 0.5, 0.25))), settings(transpShad=True, shadowDepth=0))
    assert np.array_equal(blocked, off) and not blocked[..., :3].any()


# ---- the state machine honours the parked frame and the node-resolved material; the emission quirk in a film ------------------------------
def test_bumped_textured_receiver_matches_the_probe():
    """A plane with a really varying texture on its diffuse shader and a really bumping bump shader, no lights.  The expectation is composed
    from probe op 26 at every AO sample — through the triangle and its barycentrics: wf_bump_hit, wf_mat_hit, then ao_candidate — so the
    film holds what st_dl_eval makes of the PARKED frame and material (wf_frame_parked, wf_mat_parked, records 22 and 24) against the
    direct evaluation.  (Bump and node evaluation themselves are held to the reference in tests/test_gpu_textures.py.)"""
    rng = np.random.default_rng(17)
    tex = dict(name="t_rgb", texels=rng.uniform(0.1, 1, (12, 16, 4)).astype(F), interpolate="bilinear", clipping="repeat", color_space="LinearRGB")
    mat = dict(NODE_MATERIAL, nodes=[dict(nd, texture="t_rgb") if "texture" in nd else nd for nd in NODE_MATERIAL["nodes"]])
    sc = clay_scene(plane_mat=mat)
    sc["uv"] = rng.uniform(0, 3, (sc["verts"].shape[0], 3, 2)).astype(F)
    sc["textures"] = [tex]
    rd = settings(do_AO=True, AO_samples=4, AO_distance=0.6, AO_color=(0.9, 0.8, 0.7))
    film, yi = device(sc, rd)
    flat, _ = device(dict(sc, materials=[dict(NODE_PLAIN, color=(0.8, 0.8, 0.8))] + sc["materials"][1:]), rd)
    assert np.abs(film[..., :3] - flat[..., :3]).max() > 0.05, "texture and bump should show"
    r = Restatement(sc, rd, yi)
    keys, rows, n_of = [], [], []
    for pixels, ps, so, frm, dr, tmin, tmax in r.camera_samples():
        h, tri, t, bary = r.osc.intersect(frm, dr, tmin, tmax, use_tree=False)
        if not h:
            continue
        v = r.vertex(frm, dr, t, tri)
        n = r.ao_n
        offs = (n * ps + so) & M32
        h_2, h_3 = halton(2, offs - 1, n), halton(3, offs - 1, n)
        for i in range(n):
            rows.append([np.array([v["mat"]], np.uint32).view(F)[0], *v["p"], *v["n"], *v["ng"], *v["wo"], h_2[i], h_3[i], 1.0, F(0.0005), r.ao_dist, *r.ao_col,
                         np.array([tri], np.uint32).view(F)[0], bary[1], bary[2]])
        keys.append(pixels); n_of.append(n)
    out = yi.probe(26, np.array(rows, F), 12)
    rows = np.array(rows, F)
    go = out[:, 0] != 0
    rays = np.hstack([rows[:, 1:4], out[:, 1:4], out[:, 4:6]])[go]
    sh = np.zeros(len(out), bool); sh[go] = yi.shadowRays(rays) != 0
    want = np.zeros((rd["height"], rd["width"], 3), F)
    k = 0
    for pixels, n in zip(keys, n_of):
        acc = np.zeros(3, F)
        for i in range(k, k + n):
            if go[i] and not sh[i]:
                acc = (acc + out[i, 6:9]).astype(F)
        k += n
        for y, x in pixels:
            want[y, x] = (want[y, x] + (acc / F(n)).astype(F)).astype(F)
    check(film, want, "bumped, textured receiver")
    assert yi.getRenderStats().rays_shadow == int(go.sum())


def test_emitting_receiver():
    """the emission quirk in a film: an emitting box adds emit() * pdf per sample whatever the shadow ray says (:1072-1075), before that
    sample's own contribution; on top of the oracle's film without AO (which holds the box's own emission, integrator_direct_light.cc:125-128)"""
    sc = clay_scene(box_mat={"type": "shinydiffusemat", "color": (0.7, 0.5, 0.3), "diffuse_reflect": 0.9, "emit": 0.4})
    rd_off = settings()
    rd = dict(rd_off, do_AO=True, AO_samples=5, AO_distance=0.6)
    film, yi = device(sc, rd)
    ofilm, ost = po.OracleScene(sc).render(rd_off)
    r = Restatement(sc, rd, yi)
    ao = r.primary_film()
    check(film, ofilm[..., :3] + ao, "emitting box")
    assert yi.getRenderStats().rays_shadow == r.n_rays
    # the quirk shows: the same film with the emission term left out of AO misses by far
    plain = Restatement(clay_scene(), rd, yi).primary_film()
    assert np.abs(ao - plain).max() > 100 * ATOL
