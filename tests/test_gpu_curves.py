"""Curve meshes on the DEVICE: Scene::endCurveMesh (scene.cc:154-281) expanded at scene set-up by the kernel of
libyafaray_amd/csrc/yafgpu_assemble.hip into rows of the triangle, shading and texture-coordinate arrays.

What the rows are held to is the float32 restatement of tests/curves_fixture.py (one rounding per operation, doubles where the source
has them), with the records, normals and instance rows restated here as the host loop of yafgpu_scene_create and the reference's
TriangleInstance make them.  The device unit is built without contraction and with IEEE square root and division, so the comparisons
are np.array_equal on bit patterns.  Beside the rows: twin scenes (the same strands handed over as plain UV meshes, whose rows the host
loop makes) must give the same film and ray counts, and ray batches must match brute force over the restated triangles under both tree
builders.  Nothing here is compared with the reference's compiled Scene: its sources need the generated build header."""

import numpy as np
import pytest

from libyafaray_amd import Interface, scenes
from oracle import pyoracle as po
from tests import curves_fixture as cf

pytestmark = pytest.mark.gpu

F = np.float32
U = np.uint32
BASEMESH = 0x0200
NAN_BITS = 0x7fc00000


@pytest.fixture(scope="module", autouse=True)
def torch_first():
    """(as in the other GPU modules: let torch open the GPU before the library does)"""
    import torch
    torch.cuda.init()


# ---- the restatement of the rows ----------------------------------------------------------------------------------------------------
sq3, cross, normalize = cf.sq3, cf.cross, cf.normalize


def mul_point(m, p):
    """Matrix4 * Point3, matrix4.h:89-94"""
    return np.stack([((m[r, 0] * p[..., 0] + m[r, 1] * p[..., 1]) + m[r, 2] * p[..., 2]) + m[r, 3] for r in range(3)], -1)


def mul_vec(m, v):
    """Matrix4 * Vec3, matrix4.h:82-87"""
    return np.stack([(m[r, 0] * v[..., 0] + m[r, 1] * v[..., 1]) + m[r, 2] * v[..., 2] for r in range(3)], -1)


def records(va, vb, vc, n):
    """updateIntersectionCachedValues, triangle.h:197-220; recNormal, :295-302"""
    e1, e2 = vb - va, vc - va
    longest = np.maximum(np.sqrt(sq3(e1)), np.sqrt(sq3(e2)))
    eps = (np.float64(F(0.1)) * 0.00005 * longest.astype(np.float64)).astype(F)
    if n is None:
        n = normalize(cross(e1, e2))
    return e1, e2, eps, n


def pack(verts, mat, n, cn, uv, have_vn, have_tc):
    """the 44 words probe op 28 returns per triangle: three records, (normal, smooth), three corner normals, UVs, orcos, what is there"""
    va, vb, vc = (np.ascontiguousarray(verts[:, c]) for c in range(3))
    e1, e2, eps, n = records(va, vb, vc, n)
    t = len(va)
    o = np.zeros((t, 44), U)
    o[:, 0:3] = va.view(U); o[:, 3] = eps.view(U)
    o[:, 4:7] = e1.view(U); o[:, 7] = np.asarray(mat).astype(U)
    o[:, 8:11] = e2.view(U)
    o[:, 12:15] = n.view(U)
    if cn is not None:
        has = np.abs(cn).sum(-1) != 0
        o[:, 15] = has.any(-1).astype(U)
        cn = np.where(has[..., None], cn, n[:, None, :])
    else:
        cn = np.repeat(n[:, None, :], 3, 1)
    if have_vn:
        for c in range(3):
            o[:, 16 + 4 * c:19 + 4 * c] = np.ascontiguousarray(cn[:, c]).view(U)
    if have_tc:
        o[:, 28] = NAN_BITS
        o[:, 34] = NAN_BITS             # none of the objects here has orco
        if uv is not None:
            o[:, 28:34] = np.ascontiguousarray(uv, F).reshape(t, 6).view(U)
    o[:, 43] = (1 if have_vn else 0) | (6 if have_tc else 0)
    return o


def mesh_corners(mesh):
    v, tris = np.asarray(mesh["verts"], F), np.asarray(mesh["tris"], np.int64)
    uv = None if mesh.get("uv") is None else np.asarray(mesh["uv"][0], F)[np.asarray(mesh["uv"][1], np.int64)]
    vn = None if mesh.get("normals") is None else np.asarray(mesh["normals"], F)[tris]
    return v[tris], uv, vn


def plain_rows(mesh, have_vn, have_tc):
    """what the host loop of yafgpu_scene_create gives, and the kernel for a plain segment"""
    verts, uv, vn = mesh_corners(mesh)
    return pack(verts, mesh["mat"], None, vn, uv, have_vn, have_tc), verts


def instance_rows(mesh, m, have_vn, have_tc):
    """a TriangleObjectInstance of a base without normals or texture coordinates: M * vertex, the normal M * base normal, normalised
    (TriangleInstance::getNormal, triangle.h:376-379)"""
    m = np.asarray(m, F).reshape(4, 4)
    v, _, _ = mesh_corners(mesh)
    n = normalize(mul_vec(m, normalize(cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]))))
    verts = np.stack([mul_point(m, v[:, c]) for c in range(3)], 1)
    return pack(verts, mesh["mat"], n, None, None, have_vn, have_tc), verts


def curve_rows(c, have_vn, have_tc):
    """a strand: the restated triangles, one material, UVs along the strand, no orco, no vertex normals"""
    verts, uv = cf.triangles(c["points"], c["start"], c["end"], c["shape"])
    return pack(verts, np.full(len(verts), c["mat"]), None, None, uv, have_vn, have_tc), verts


# ---- building a scene through the Interface ---------------------------------------------------------------------------------------
CLAY = {"type": "shinydiffusemat", "color": (0.8, 0.8, 0.8), "diffuse_reflect": 1.0}
RUST = {"type": "shinydiffusemat", "color": (0.7, 0.3, 0.2), "diffuse_reflect": 0.9}
VALUE = {"type": "shinydiffusemat", "color": (0.5, 0.5, 0.5), "diffuse_reflect": 1.0, "diffuse_shader": "c",
         "nodes": [dict(name="c", type="value", color=(0.3, 0.6, 0.9, 1.0))]}      # a node of its own: the scene then carries texture coordinates
POINT = {"type": "pointlight", "from": (0.5, -4.0, 3.0), "color": (1.0, 1.0, 1.0), "power": 20.0}
RES = 48
CAMERA = {"type": "perspective", "from": (0.0, -6.0, 1.5), "to": (0.0, 0.0, 1.0), "up": (0.0, -6.0, 2.5), "resx": RES, "resy": RES, "focal": 1.2}


class Scene:
    """drives an Interface and keeps what it was given, in order to restate the flattened scene: objects by id"""

    def __init__(self, materials, rd=None, lights=(POINT,), camera=CAMERA, textures=(), strict=True):
        self.yi = Interface(strict=strict)
        self.rd = rd or scenes.render_settings(RES, RES, 1, integrator="directlighting")
        empty = {"verts": np.zeros((0, 3, 3), F), "tri_mat": np.zeros(0, np.int32), "vnormals": None, "materials": list(materials),
                 "lights": list(lights), "camera": camera, "textures": list(textures)}
        self.handles = scenes.load_scene(self.yi, empty, self.rd)      # (its one mesh is empty: no rows)
        self.have_tc = any(m.get("nodes") for m in materials)
        self.meshes, self.objects = {}, {}

    def mesh(self, mesh, mid=None, type_=0):
        yi = self.yi
        mid = yi.getNextFreeId() if mid is None else mid
        v, tris = np.asarray(mesh["verts"], F), np.asarray(mesh["tris"])
        yi.startGeometry()
        yi.startTriMesh(mid, len(v), len(tris), False, mesh.get("uv") is not None, type_)
        for k in range(len(v)):
            yi.addVertex(*[float(x) for x in v[k]])
            if mesh.get("normals") is not None:
                yi.addNormal(*[float(x) for x in mesh["normals"][k]])
        if mesh.get("uv") is not None:
            for u in mesh["uv"][0]:
                yi.addUv(float(u[0]), float(u[1]))
        for t in range(len(tris)):
            a, b, c = (int(x) for x in tris[t])
            h = self.handles[int(mesh["mat"][t])]
            if mesh.get("uv") is not None:
                ua, ub, uc = (int(x) for x in mesh["uv"][1][t])
                assert yi.addTriangleWithUv(a, b, c, ua, ub, uc, h)
            else:
                assert yi.addTriangle(a, b, c, h)
        yi.endTriMesh()
        yi.endGeometry()
        self.meshes[mid] = mesh
        if not (type_ & BASEMESH):
            self.objects[mid] = ("mesh", mid)
        return mid

    def instance(self, base, matrix):
        before = {g["id"] for g in self.yi.getInstances()}
        assert self.yi.addInstance(base, matrix), self.yi.getLastError()
        (new,) = [g for g in self.yi.getInstances() if g["id"] not in before]
        self.objects[new["id"]] = ("instance", base, np.asarray(matrix, F).reshape(4, 4))
        return new["id"]

    def curve(self, points, mat, start, end, shape, cid=None):
        yi = self.yi
        cid = yi.getNextFreeId() if cid is None else cid
        pts = np.ascontiguousarray(points, F).reshape(-1, 3)
        yi.startGeometry()
        yi.startCurveMesh(cid, len(pts))
        for p in pts:
            yi.addVertex(*[float(x) for x in p])
        yi.endCurveMesh(self.handles[mat], start, end, shape)
        yi.endGeometry()
        self.objects[cid] = ("curve", {"points": pts, "mat": mat, "start": start, "end": end, "shape": shape})
        return cid

    def expected(self):
        """(rows (n, 44) uint32, corner vertices (n, 3, 3), the object id of every row) of the flattened scene, in object-id order"""
        have_vn = any(m.get("normals") is not None for m in self.meshes.values())
        rows, verts, owner = [np.zeros((0, 44), U)], [np.zeros((0, 3, 3), F)], []
        for oid in sorted(self.objects):
            ob = self.objects[oid]
            if ob[0] == "mesh":
                r, v = plain_rows(self.meshes[ob[1]], have_vn, self.have_tc)
            elif ob[0] == "instance":
                r, v = instance_rows(self.meshes[ob[1]], ob[2], have_vn, self.have_tc)
            else:
                r, v = curve_rows(ob[1], have_vn, self.have_tc)
            rows.append(r); verts.append(v); owner += [oid] * len(r)
        return np.concatenate(rows), np.concatenate(verts), np.array(owner)

    def device_rows(self, n):
        x = np.arange(n, dtype=U).reshape(n, 1).view(F)
        return self.yi.probe(28, x, 44).view(U)


def strip(n_tris, seed, mat=0, lo=-1.0, hi=1.0):
    """a strip of n_tris random triangles over n_tris + 2 vertices"""
    rng = np.random.default_rng(seed)
    v = rng.uniform(lo, hi, (n_tris + 2, 3)).astype(F)
    tris = np.array([(k, k + 1, k + 2) for k in range(n_tris)], np.int64)
    return {"verts": v, "tris": tris, "mat": np.full(n_tris, mat, np.int64)}


def with_uv_and_normals(mesh, seed):
    rng = np.random.default_rng(seed)
    nv, nt = len(mesh["verts"]), len(mesh["tris"])
    n = rng.normal(size=(nv, 3))
    return dict(mesh, uv=(rng.uniform(0, 1, (nv + 3, 2)).astype(F), rng.integers(0, nv + 3, (nt, 3))), normals=(n / np.linalg.norm(n, axis=1, keepdims=True)).astype(F))


ROTATE = np.array([[0.8, -0.6, 0.0, 0.2], [0.6, 0.8, 0.0, 0.1], [0.0, 0.0, 1.0, -0.4], [0.0, 0.0, 0.0, 1.0]], F)


@pytest.fixture(scope="module")
def rows_scene():
    """strands of 2, 3 and 17 points (8, 14 and 98 rows: no multiple of 64, waves straddle the segment boundaries) with a plain mesh and an
    instance between them by object id"""
    s = Scene([CLAY, RUST, VALUE])
    base = s.mesh(strip(7, 1, mat=1), 1001, BASEMESH)
    tags = {}
    tags["2 points, +z, shape 0"] = s.curve([(0, 0, 0), (0, 0, 1)], 0, 0.05, 0.0125, 0.0)
    tags["3 points, -z then coincident"] = s.curve([(1, 0, 2), (1, 0, 1), (1, 0, 1)], 1, 0.04, 0.02, -0.5)
    tags["plain a"] = s.mesh(strip(5, 2, mat=1))
    tags["17 points, tip 0, shape 0.7"] = s.curve(cf.strand(17, 3, 2.0, (-1, 0, 0)), 2, 0.06, 0.0, 0.7)
    tags["instance"] = s.instance(base, ROTATE)
    tags["3 points, coincident first, tip 0"] = s.curve([(0.5, 0.5, 0), (0.5, 0.5, 0), (0.75, 0.5, 1)], 0, 0.03, 0.0, -0.5)
    tags["plain b"] = s.mesh(with_uv_and_normals(strip(3, 4, mat=2), 5))
    tags["17 points, start = end, shape -0.5"] = s.curve(cf.strand(17, 6, 1.5, (1, 1, 0)), 1, 0.03, 0.03, -0.5)
    tags["2 points, -z"] = s.curve([(0, 1, 1), (0, 1, 0.25)], 2, 0.02, 0.01, 0.7)
    for k in range(4):
        tags[f"17 points, {k}"] = s.curve(cf.strand(17, 10 + k, 1.0 + k, (k - 2, -1, 0)), k % 3, 0.05, 0.01 * k, (-0.5, 0.0, 0.7, -0.25)[k])
    tags["plain c"] = s.mesh(strip(2, 7))
    s.tags = tags
    s.yi.prepareRender()
    return s


# ---- 1. rows, bit for bit -----------------------------------------------------------------------------------------------------------
def test_rows_bit_for_bit(rows_scene):
    s = rows_scene
    want, verts, owner = s.expected()
    n = len(want)
    assert s.yi.getRenderStats().n_triangles == n and n > 2 * 256, "the flattened triangles, over more than one block"
    got = s.device_rows(n)
    bad = np.flatnonzero((got != want).any(1))
    names = {v: k for k, v in s.tags.items()}
    print(f"{n} rows, {len(set(owner))} objects; rows that differ: {len(bad)}")
    assert len(bad) == 0, [(int(i), names[int(owner[i])], int(i - np.flatnonzero(owner == owner[i])[0]), np.flatnonzero(got[i] != want[i]).tolist()) for i in bad[:8]]
    assert np.array_equal(got, want)
    # what the cases were meant to cover is there
    sizes = {k: int((owner == oid).sum()) for k, oid in s.tags.items()}
    assert {8, 14, 98} <= set(sizes.values()) and sizes["instance"] == 7
    kinds = [s.objects[oid][0] for oid in sorted(s.objects)]
    assert all(any(kinds[k] == a and kinds[k + 1] == b for k in range(len(kinds) - 1)) for a, b in
               [("curve", "mesh"), ("mesh", "curve"), ("curve", "instance"), ("instance", "curve"), ("curve", "curve")]), "the segment search crosses all three kinds"
    firsts = [int(np.flatnonzero(owner == oid)[0]) for oid in sorted(s.objects)]
    assert sum(1 for f in firsts if f % 64) >= 8, "segment boundaries inside waves"
    # both branches of createCs__, and the zero tangent of coincident points, which takes the z branch too (u = +x)
    up, down = verts[owner == s.tags["2 points, +z, shape 0"]], verts[owner == s.tags["2 points, -z"]]
    assert up[0, 1, 0] > 0 > down[0, 1, 0], "b0 = o + s * u - h * v: u = +x for a tangent along +z, -x along -z"
    coincident = verts[owner == s.tags["3 points, coincident first, tip 0"]]
    assert coincident[0, 1, 0] > coincident[0, 0, 0] and coincident[0, 1, 2] == 0
    # a tip radius of 0 makes degenerate triangles: the top cap is one point, its normal stays the zero vector
    tip = want[owner == s.tags["17 points, tip 0, shape 0.7"]]
    assert not tip[-1, 4:7].view(F).any() and not tip[-1, 8:11].view(F).any() and not tip[-1, 12:15].view(F).any() and tip[-1, 3] == 0
    # UVs run 0 -> 1 along the strand; no orco; no vertex normals
    assert tip[0, 28:34].view(F).max() == 0 and tip[-1, 28:34].view(F).min() > 0.999 and (tip[:, 34] == NAN_BITS).all() and not tip[:, 15].any()
    assert (want[owner == s.tags["plain b"]][:, 15] == 1).all(), "the scene carries vertex normals: a curve's corners take the geometric normal"
    assert np.array_equal(tip[:, 16:19], tip[:, 12:15]) and np.array_equal(tip[:, 24:27], tip[:, 12:15])


def test_plain_and_instance_rows_are_what_they_are_without_curves():
    """the rows of the plain meshes and of the instance do not depend on the curves between them"""
    def build(with_curves):
        s = Scene([CLAY, RUST, VALUE])
        base = s.mesh(strip(7, 1, mat=1), 1001, BASEMESH)
        ids = []
        if with_curves:
            s.curve(cf.strand(3, 20), 0, 0.05, 0.0, 0.0)
        ids.append(s.mesh(strip(70, 22, mat=1)))
        if with_curves:
            s.curve(cf.strand(17, 21), 1, 0.05, 0.02, -0.5)
        ids.append(s.instance(base, ROTATE))
        ids.append(s.mesh(with_uv_and_normals(strip(33, 23, mat=2), 24)))
        if with_curves:
            s.curve(cf.strand(2, 22), 2, 0.05, 0.02, 0.7)
        s.yi.prepareRender()
        want, _, owner = s.expected()
        got = s.device_rows(len(want))
        assert np.array_equal(got, want)
        return got, owner, ids
    got1, owner1, ids1 = build(True)
    got0, owner0, ids0 = build(False)
    assert len(got1) == len(got0) + 14 + 98 + 8
    for a, b in zip(ids1, ids0):
        assert np.array_equal(got1[owner1 == a], got0[owner0 == b])


# ---- 2. twin scenes: the same strands as plain UV meshes ----------------------------------------------------------------------------
def quad(a, b, c, d):
    return [a, b, c, d], [(0, 1, 2), (0, 2, 3)]


def room():
    """an axis-aligned room, open towards the camera"""
    x0, x1, y0, y1, z0, z1 = -2.0, 2.0, -2.0, 2.0, 0.0, 3.0
    faces = [quad((x0, y0, z0), (x1, y0, z0), (x1, y1, z0), (x0, y1, z0)), quad((x0, y0, z1), (x0, y1, z1), (x1, y1, z1), (x1, y0, z1)),
             quad((x0, y1, z0), (x1, y1, z0), (x1, y1, z1), (x0, y1, z1)), quad((x0, y0, z0), (x0, y1, z0), (x0, y1, z1), (x0, y0, z1)),
             quad((x1, y0, z0), (x1, y0, z1), (x1, y1, z1), (x1, y1, z0))]
    v, t = [], []
    for fv, ft in faces:
        t += [tuple(len(v) + k for k in tri) for tri in ft]
        v += fv
    return {"verts": np.array(v, F), "tris": np.array(t, np.int64), "mat": np.zeros(len(t), np.int64)}


AREA = {"type": "arealight", "corner": (-0.5, -0.5, 2.875), "point1": (-0.5, 0.5, 2.875), "point2": (0.5, -0.5, 2.875), "color": (1.0, 1.0, 1.0), "power": 25.0,
        "samples": 2}
# a gradient along u: the strand's UVs (t, t) read it from root to tip
GRADIENT = dict(name="t_strand", texels=np.repeat(np.linspace(0.05, 0.95, 16, dtype=F)[None, :, None], 4, 0).repeat(4, 2).copy(), interpolate="none",
                clipping="repeat", color_space="LinearRGB")
_layer = dict(type="layer", mode=0, def_val=1.0, upper_value=0.0, colfac=1.0, def_col=(1.0, 0.0, 1.0, 1.0), do_color=True, do_scalar=False, color_input=True,
              upper_color=(0.8, 0.8, 0.8, 1.0))
MAPPED_UV = {"type": "shinydiffusemat", "color": (0.8, 0.8, 0.8), "diffuse_reflect": 0.9, "diffuse_shader": "diff",
             "nodes": [dict(_layer, name="diff", input="map"), dict(name="map", type="texture_mapper", texture="t_strand", texco="uv", mapping="plain")]}

FILM_CASES = {
    "directlighting": dict(rd=dict(integrator="directlighting"), materials=[CLAY, RUST]),
    "pathtracing, two bounces": dict(rd=dict(integrator="pathtracing", bounces=2), materials=[CLAY, RUST]),
    "node material reading UV": dict(rd=dict(integrator="directlighting"), materials=[CLAY, MAPPED_UV], textures=[GRADIENT]),
}


def tuft():
    """30 strands on the room's floor, of 2 to 9 points, both signs of the shape, every third with a tip radius of 0"""
    rng = np.random.default_rng(77)
    out = []
    for k in range(30):
        n = (2, 3, 5, 9)[k % 4]
        origin = (rng.uniform(-1.5, 1.5), rng.uniform(-1.0, 1.5), 0.0)
        out.append(dict(points=cf.strand(n, 200 + k, rng.uniform(0.8, 2.2), origin), mat=1, start=0.09, end=0.0 if k % 3 == 0 else 0.03, shape=(-0.5, 0.0, 0.7)[k % 3]))
    return out


@pytest.mark.parametrize("case", list(FILM_CASES))
def test_twin_scene_films_bit_for_bit(case):
    c = FILM_CASES[case]
    rd = scenes.render_settings(RES, RES, 4, **c["rd"])
    strands = tuft()
    films, stats = [], []
    for as_curves in (True, False):
        s = Scene(c["materials"], rd=rd, lights=[AREA], textures=c.get("textures", ()))
        s.mesh(room(), 2)
        for k, st in enumerate(strands):          # the same object ids, one object per strand in both scenes: the libc stream agrees
            if as_curves:
                s.curve(st["points"], st["mat"], st["start"], st["end"], st["shape"], 10 + k)
            else:
                verts, uv = cf.triangles(st["points"], st["start"], st["end"], st["shape"])
                t = len(verts)
                s.mesh({"verts": verts.reshape(-1, 3), "tris": np.arange(3 * t).reshape(t, 3), "mat": np.full(t, st["mat"]),
                        "uv": (uv.reshape(-1, 2), np.arange(3 * t).reshape(t, 3))}, 10 + k)
        s.yi.setRandState(20240, 3)
        s.yi.render()
        films.append(s.yi.getFilm(RES, RES))
        stats.append(s.yi.getRenderStats())
        assert stats[-1].n_triangles == 10 + sum(6 * (len(st["points"]) - 1) + 2 for st in strands)
        assert len(s.yi.getCurves()) == (30 if as_curves else 0)
    a, b = films
    assert a[..., 4].all() and a[..., :3].any()
    print(f"{case}: largest film difference {float(np.abs(a - b).max()):.3g}; rays {stats[0].rays_closest} + {stats[0].rays_shadow}")
    assert np.array_equal(a, b), f"{case}: films differ by up to {float(np.abs(a - b).max())}"
    for k in ("rays_closest", "rays_shadow", "camera_samples"):
        assert getattr(stats[0], k) == getattr(stats[1], k), k


# ---- 3. traversal -----------------------------------------------------------------------------------------------------------------
def ray_batch_report():
    """a patch of 200 strands set up through addCurves beside a plain mesh, under the tree builder YAFGPU_BUILD names: closest-hit and
    shadow answers for 2000 rays against brute force over the restated triangles"""
    s = Scene([CLAY, RUST])
    rng = np.random.default_rng(9)
    s.mesh(strip(20, 41, mat=1, lo=-2.0, hi=2.0))
    n_points, pts = [], []
    for k in range(200):
        n_points.append(4)
        pts.append(cf.strand(4, 300 + k, rng.uniform(0.5, 1.5), (rng.uniform(-2, 2), rng.uniform(-2, 2), rng.uniform(-1.0, 0.0))))
    s.yi.startGeometry()
    ids = s.yi.addCurves(n_points, np.concatenate(pts), s.handles[0], 0.08, 0.02, -0.5)
    s.yi.endGeometry()
    for cid, p in zip(ids, pts):
        s.objects[int(cid)] = ("curve", {"points": p, "mat": 0, "start": 0.08, "end": 0.02, "shape": -0.5})
    s.yi.prepareRender()
    want, verts, _ = s.expected()
    report = {"n_triangles": int(s.yi.getRenderStats().n_triangles), "n_restated": len(verts), "rows_equal": bool(np.array_equal(s.device_rows(len(want)), want))}
    osc = po.OracleScene({"verts": verts, "tri_mat": want[:, 7].astype(np.int32), "vnormals": None, "materials": [CLAY, RUST], "lights": [POINT], "camera": CAMERA})
    n = 2000
    o = rng.uniform(-2.5, 2.5, size=(n, 3)).astype(F)
    d = rng.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.concatenate([o, d.astype(F), np.full((n, 1), 5e-5, F), np.full((n, 1), -1.0, F)], axis=1)
    rays[::7, 7] = rng.uniform(0.05, 2.0, size=rays[::7].shape[0])      # bounded rays too
    tri, t, bary = s.yi.intersectRays(rays)
    sh = s.yi.shadowRays(rays)
    mism, hits = 0, 0
    for i in range(n):
        h, oti, ot, ob = osc.intersect(rays[i, :3], rays[i, 3:6], float(rays[i, 6]), float(rays[i, 7]), use_tree=False)
        hits += bool(h)
        if (tri[i] >= 0) != bool(h) or (h and (tri[i] != oti or t[i] != ot or not np.array_equal(bary[i], ob))):
            mism += 1
        if bool(osc.is_shadowed(rays[i, :3], rays[i, 3:6], float(rays[i, 6]), float(rays[i, 7]), use_tree=False)) != bool(sh[i]):
            mism += 1
    report.update(rays=n, hits=hits, mismatches=mism)
    return report


@pytest.mark.parametrize("builder", ["host", "device"])
def test_ray_batches_match_brute_force(builder):
    """each builder in a fresh child process: the child sees YAFGPU_BUILD from its first scene on"""
    import json, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    child = "import json; from tests import test_gpu_curves as t; print('REPORT ' + json.dumps(t.ray_batch_report()))"
    r = subprocess.run([sys.executable, "-c", child], cwd=root, env=dict(os.environ, YAFGPU_BUILD=builder), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rep = json.loads([l for l in r.stdout.splitlines() if l.startswith("REPORT ")][-1][7:])
    print(f"{builder} builder: {rep['hits']} of {rep['rays']} rays hit; {rep['mismatches']} results differ")
    assert rep["n_triangles"] == rep["n_restated"] == 20 + 200 * 20 and rep["rows_equal"]
    assert rep["hits"] > rep["rays"] // 20
    assert rep["mismatches"] == 0, f"{rep['mismatches']} ray results differ from the brute force over the restated triangles"


# ---- 4. cache invalidation ----------------------------------------------------------------------------------------------------------
def test_one_more_curve_rebuilds_the_scene():
    s = Scene([CLAY])
    s.mesh(strip(4, 62))
    s.curve(cf.strand(3, 63), 0, 0.05, 0.01, 0.0)
    s.yi.prepareRender()
    assert s.yi.getRenderStats().n_triangles == 4 + 14
    s.curve(cf.strand(2, 64), 0, 0.05, 0.01, 0.0)
    s.yi.prepareRender()
    assert s.yi.getRenderStats().n_triangles == 4 + 14 + 8
    want, _, _ = s.expected()
    assert np.array_equal(s.device_rows(len(want)), want)
