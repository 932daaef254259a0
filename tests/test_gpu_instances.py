"""Mesh instances on the DEVICE: Scene::addInstance (scene.cc:1105-1130) expanded at scene set-up by the kernel of
libyafaray_amd/csrc/yafgpu_assemble.hip into rows of the triangle, shading and texture-coordinate arrays.

What the rows are held to is a float32 restatement written here, one rounding per operation in the order the reference's expressions
give (Matrix4 * Point3, matrix4.h:89-94; updateIntersectionCachedValues, triangle.h:210-220; TriangleInstance::getNormal, :376-379;
TriangleInstance::getSurface's vertex normals with its `index > 0` test, triangle.cc:210-222).  The device unit is built without
contraction and with IEEE square root and division, so the same operations in the same order give the same bits: the comparisons are
np.array_equal on the bit patterns and need no tolerance.  The rows are read back through probe op 28."""

import numpy as np
import pytest

from libyafaray_amd import Interface, scenes
from oracle import pyoracle as po

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


# ---- the restatement -------------------------------------------------------------------------------------------------------------
def sq3(v):
    return (v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def normalize(v):
    """Vec3::normalize, vector.h:227-238"""
    l = sq3(v)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = F(1.0) / np.sqrt(l)
    out = v * inv[..., None]
    return np.where((l != 0)[..., None], out, v)


def mul_point(m, p):
    """Matrix4 * Point3, matrix4.h:89-94"""
    return np.stack([((m[r, 0] * p[..., 0] + m[r, 1] * p[..., 1]) + m[r, 2] * p[..., 2]) + m[r, 3] for r in range(3)], -1)


def mul_vec(m, v):
    """Matrix4 * Vec3, matrix4.h:82-87"""
    return np.stack([(m[r, 0] * v[..., 0] + m[r, 1] * v[..., 1]) + m[r, 2] * v[..., 2] for r in range(3)], -1)


def mesh_rows(mesh):
    """per triangle of a mesh description: corner vertices, materials, corner normals (zeros: none) with the index-0 marks, UVs, orcos"""
    v = np.asarray(mesh["verts"], F)
    tris = np.asarray(mesh["tris"], np.int64)
    rows = {"verts": v[tris], "mat": np.asarray(mesh["mat"], np.int64), "vn": np.zeros((len(tris), 3, 3), F), "index0": np.zeros((len(tris), 3), bool),
            "uv": None, "orco": None}
    if mesh.get("corner_normals") is not None:      # what smoothMesh computed, read back from the host side
        rows["vn"] = np.asarray(mesh["corner_normals"], F)
        if mesh["smooth"] >= 180:                     # the loop of scene.cc:420-448: the corner's normal index is its vertex index
            rows["index0"] = tris == 0
    elif mesh.get("normals") is not None:             # exported: the index is the vertex index
        rows["vn"] = np.asarray(mesh["normals"], F)[tris]
        rows["index0"] = tris == 0
    if mesh.get("uv") is not None:
        rows["uv"] = np.asarray(mesh["uv"][0], F)[np.asarray(mesh["uv"][1], np.int64)]
    if mesh.get("orco") is not None:
        rows["orco"] = np.asarray(mesh["orco"], F)[tris]
    return rows


def has_normals(mesh):
    return mesh.get("corner_normals") is not None or mesh.get("normals") is not None


def records(va, vb, vc, n):
    e1, e2 = vb - va, vc - va
    longest = np.maximum(np.sqrt(sq3(e1)), np.sqrt(sq3(e2)))
    eps = (np.float64(F(0.1)) * 0.00005 * longest.astype(np.float64)).astype(F)
    if n is None:
        n = normalize(cross(e1, e2))      # recNormal, triangle.h:295-302
    return e1, e2, eps, n


def pack(va, e1, e2, eps, mat, n, smooth, cn, uv, orco, have_vn, have_tc):
    """the 44 words probe op 28 returns per triangle"""
    t = len(va)
    o = np.zeros((t, 44), U)
    o[:, 0:3] = va.view(U); o[:, 3] = eps.view(U)
    o[:, 4:7] = e1.view(U); o[:, 7] = mat.astype(U)
    o[:, 8:11] = e2.view(U)
    o[:, 12:15] = n.view(U); o[:, 15] = smooth.astype(U)
    if have_vn:
        for c in range(3):
            o[:, 16 + 4 * c:19 + 4 * c] = np.ascontiguousarray(cn[:, c]).view(U)
    if have_tc:
        o[:, 28] = NAN_BITS
        o[:, 34] = NAN_BITS
        if uv is not None:
            o[:, 28:34] = np.ascontiguousarray(uv, F).reshape(t, 6).view(U)
        if orco is not None:
            o[:, 34:43] = np.ascontiguousarray(orco, F).reshape(t, 9).view(U)
    o[:, 43] = (1 if have_vn else 0) | (6 if have_tc else 0)
    return o


def plain_rows(mesh, have_vn, have_tc):
    """what the host loop of yafgpu_scene_create gives, and the kernel for a plain segment"""
    r = mesh_rows(mesh)
    va, vb, vc = (np.ascontiguousarray(r["verts"][:, c]) for c in range(3))
    e1, e2, eps, n = records(va, vb, vc, None)
    has = np.abs(r["vn"]).sum(-1) != 0
    cn = np.where(has[..., None], r["vn"], n[:, None, :])
    return pack(va, e1, e2, eps, r["mat"], n, has.any(-1), cn, r["uv"], r["orco"], have_vn, have_tc), np.stack([va, vb, vc], 1)


def instance_rows(mesh, m, flags, have_vn, have_tc):
    """a TriangleObjectInstance of `mesh` under m, with the flags it copied when it was made"""
    m = np.asarray(m, F).reshape(4, 4)
    r = mesh_rows(mesh)
    a, b, c = (np.ascontiguousarray(r["verts"][:, k]) for k in range(3))
    n_base = normalize(cross(b - a, c - a))
    n = normalize(mul_vec(m, n_base))              # TriangleInstance::getNormal: not recomputed from the transformed edges
    va, vb, vc = mul_point(m, a), mul_point(m, b), mul_point(m, c)
    e1, e2, eps, _ = records(va, vb, vc, n)
    has = np.zeros((len(a), 3), bool)
    cn = np.repeat(n[:, None, :], 3, 1)
    if flags["smooth"] and has_normals(mesh):
        has = (np.abs(r["vn"]).sum(-1) != 0) & ~r["index0"]      # `index > 0`, triangle.cc:215-217
        cn = np.where(has[..., None], mul_vec(m, r["vn"]), cn)   # Vec3(M * normals_[index]), not normalised
    uv = r["uv"] if flags["has_uv"] else None
    orco = r["orco"] if flags["has_orco"] else None
    return pack(va, e1, e2, eps, r["mat"], n, has.any(-1), cn, uv, orco, have_vn, have_tc), np.stack([va, vb, vc], 1)


# ---- building a scene through the Interface ---------------------------------------------------------------------------------------
CLAY = {"type": "shinydiffusemat", "color": (0.8, 0.8, 0.8), "diffuse_reflect": 1.0}
RUST = {"type": "shinydiffusemat", "color": (0.7, 0.3, 0.2), "diffuse_reflect": 0.9}
# a material with a node of its own: the scene then carries texture coordinates
VALUE = {"type": "shinydiffusemat", "color": (0.5, 0.5, 0.5), "diffuse_reflect": 1.0, "diffuse_shader": "c",
         "nodes": [dict(name="c", type="value", color=(0.3, 0.6, 0.9, 1.0))]}
POINT = {"type": "pointlight", "from": (0.5, -4.0, 3.0), "color": (1.0, 1.0, 1.0), "power": 20.0}
CAMERA = {"type": "perspective", "from": (0.0, -6.0, 1.5), "to": (0.0, 0.0, 1.0), "up": (0.0, -6.0, 2.5), "resx": 32, "resy": 32, "focal": 1.2}


class Scene:
    """drives an Interface and keeps what it was given, in order to restate the flattened scene: objects by id"""

    def __init__(self, materials, rd=None, lights=(POINT,), camera=CAMERA, textures=(), strict=True):
        self.yi = Interface(strict=strict)
        self.rd = rd or scenes.render_settings(32, 32, 1, integrator="directlighting")
        empty = {"verts": np.zeros((0, 3, 3), F), "tri_mat": np.zeros(0, np.int32), "vnormals": None, "materials": list(materials),
                 "lights": list(lights), "camera": camera, "textures": list(textures)}
        self.handles = scenes.load_scene(self.yi, empty, self.rd)      # (its one mesh is empty: no rows)
        self.have_tc = any(m.get("nodes") for m in materials)
        self.meshes, self.objects = {}, {}

    def mesh(self, mesh, mid=None, type_=0):
        yi = self.yi
        mid = yi.getNextFreeId() if mid is None else mid
        mesh = dict(mesh)
        v, tris = np.asarray(mesh["verts"], F), np.asarray(mesh["tris"])
        yi.startGeometry()
        yi.startTriMesh(mid, len(v), len(tris), mesh.get("orco") is not None, mesh.get("uv") is not None, type_)
        for k in range(len(v)):
            if mesh.get("orco") is not None:
                yi.addVertexWithOrco(*[float(x) for x in v[k]], *[float(x) for x in mesh["orco"][k]])
            else:
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
        mesh["smooth"] = None
        self.meshes[mid] = mesh
        if not (type_ & BASEMESH):
            self.objects[mid] = ("mesh", mid)
        return mid

    def smooth(self, mid, angle):
        yi = self.yi
        yi.startGeometry()
        yi.smoothMesh(mid, angle)
        yi.endGeometry()
        m = self.meshes[mid]
        m["smooth"] = angle
        if m.get("normals") is None:
            m["corner_normals"] = yi.getMeshCornerNormals(mid, len(m["tris"]))

    def instance(self, base, matrix):
        before = {g["id"] for g in self.yi.getInstances()}
        assert self.yi.addInstance(base, matrix), self.yi.getLastError()
        new = [g for g in self.yi.getInstances() if g["id"] not in before]
        assert len(new) == 1
        m = self.meshes[base]
        flags = {"smooth": m["smooth"] is not None or m.get("normals") is not None, "has_uv": m.get("uv") is not None, "has_orco": m.get("orco") is not None}
        got = new[0]
        assert ((got["is_smooth"] or got["normals_exported"]), got["has_uv"], got["has_orco"]) == (flags["smooth"], flags["has_uv"], flags["has_orco"])
        self.objects[got["id"]] = ("instance", base, np.asarray(matrix, F).reshape(4, 4), flags)
        return got["id"]

    def expected(self):
        """(rows (n, 44) uint32, corner vertices (n, 3, 3), the object id of every row) of the flattened scene, in object-id order"""
        have_vn = any(has_normals(m) for m in self.meshes.values())
        rows, verts, owner = [np.zeros((0, 44), U)], [np.zeros((0, 3, 3), F)], []
        for oid in sorted(self.objects):
            ob = self.objects[oid]
            r, v = plain_rows(self.meshes[ob[1]], have_vn, self.have_tc) if ob[0] == "mesh" else instance_rows(self.meshes[ob[1]], ob[2], ob[3], have_vn, self.have_tc)
            rows.append(r); verts.append(v); owner += [oid] * len(r)
        return np.concatenate(rows), np.concatenate(verts), np.array(owner)

    def device_rows(self, n):
        x = np.arange(n, dtype=U).reshape(n, 1).view(F)
        return self.yi.probe(28, x, 44).view(U)


def strip(n_tris, seed, mat=0, lo=-1.0, hi=1.0):
    """a strip of n_tris random triangles over n_tris + 2 vertices; triangle 0 uses vertex 0"""
    rng = np.random.default_rng(seed)
    v = rng.uniform(lo, hi, (n_tris + 2, 3)).astype(F)
    tris = np.array([(k, k + 1, k + 2) for k in range(n_tris)], np.int64)
    return {"verts": v, "tris": tris, "mat": np.full(n_tris, mat, np.int64)}


def with_texcoords(mesh, seed):
    rng = np.random.default_rng(seed)
    nv, nt = len(mesh["verts"]), len(mesh["tris"])
    uvs = rng.uniform(0, 1, (nv + 3, 2)).astype(F)
    return dict(mesh, orco=rng.uniform(-1, 1, (nv, 3)).astype(F), uv=(uvs, rng.integers(0, nv + 3, (nt, 3))))


def with_normals(mesh, seed):
    rng = np.random.default_rng(seed)
    n = rng.normal(size=(len(mesh["verts"]), 3))
    return dict(mesh, normals=(n / np.linalg.norm(n, axis=1, keepdims=True)).astype(F))


def rotation(axis, degrees):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    t = np.radians(degrees)
    k = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    m = np.eye(4)
    m[:3, :3] = np.eye(3) + np.sin(t) * k + (1 - np.cos(t)) * (k @ k)
    return m.astype(F)


def translation(x, y, z):
    m = np.eye(4, dtype=F)
    m[:3, 3] = (x, y, z)
    return m


IDENTITY = np.eye(4, dtype=F)
TRANSLATE = translation(0.37, -1.3, 2.11)
ROTATE = rotation((1.0, 2.0, 0.5), 37.0) + translation(0.2, 0.1, -0.4) - IDENTITY
SCALE = np.diag([1.7, 0.3, 2.9, 1.0]).astype(F) + translation(-0.6, 0.0, 0.3) - IDENTITY
MIRROR = np.diag([-1.0, 1.0, 1.0, 1.0]).astype(F) + translation(1.1, 0.2, 0.0) - IDENTITY
SHEAR = np.array([[1.0, 0.4, -0.3, 0.1], [0.0, 1.0, 0.7, -0.2], [0.2, 0.0, 1.0, 0.5], [0.0, 0.0, 0.0, 1.0]], F)
MATRICES = {"identity": IDENTITY, "translation": TRANSLATE, "rotation": ROTATE, "scale": SCALE, "mirror": MIRROR, "shear": SHEAR}


@pytest.fixture(scope="module")
def rows_scene():
    """bases of 1, 63, 65 and 100 triangles and small ones for the smoothing cases, instanced under every matrix, with plain meshes
    between the instances by id"""
    s = Scene([CLAY, RUST, VALUE])
    b1 = s.mesh(strip(1, 1), 1001, BASEMESH)
    b63 = s.mesh(with_texcoords(strip(63, 2, mat=1), 3), 1002, BASEMESH)
    b65 = s.mesh(with_normals(strip(65, 4, mat=2), 5), 1003, BASEMESH)         # exported normals; triangle 0 uses vertex 0
    b100 = s.mesh(strip(100, 6), 1004, BASEMESH)
    late = s.mesh(strip(7, 7, mat=1), 1005, BASEMESH)
    by_angle = s.mesh(with_texcoords(strip(9, 8, lo=0.0), 9), 1006, BASEMESH)
    s.smooth(b100, 181.0)                                                         # smoothed before every call on it
    s.smooth(by_angle, 60.0)                                                      # the angle-dependent loop: no normal has index 0
    tags = {}
    tags["1 identity"] = s.instance(b1, IDENTITY)
    plain_a = s.mesh(strip(5, 10, mat=1))
    tags["63 translation"] = s.instance(b63, TRANSLATE)
    tags["flat: smoothed after the call"] = s.instance(late, ROTATE)
    s.smooth(late, 181.0)
    tags["smooth: smoothed before the call"] = s.instance(late, ROTATE)
    plain_b = s.mesh(with_normals(with_texcoords(strip(3, 11, mat=2), 12), 13))
    tags["65 rotation"] = s.instance(b65, ROTATE)
    tags["100 scale"] = s.instance(b100, SCALE)
    plain_c = s.mesh(strip(2, 14))
    s.smooth(plain_c, 181.0)
    for base, what in ((b1, "1"), (b63, "63"), (b65, "65"), (b100, "100"), (by_angle, "angle")):      # every kind of base under every matrix
        for name, m in MATRICES.items():
            tags[f"{what} {name} (all)"] = s.instance(base, m)
    tags["65 mirror"] = s.instance(b65, MIRROR)
    tags["100 mirror"] = s.instance(b100, MIRROR)
    tags["angle scale"] = s.instance(by_angle, SCALE)
    tags["of a visible mesh"] = s.instance(plain_a, TRANSLATE)                    # any mesh can be a base; it renders itself too
    s.tags, s.plain = tags, (plain_a, plain_b, plain_c)
    s.yi.prepareRender()
    return s


# ---- 1. rows, bit for bit -----------------------------------------------------------------------------------------------------------
def test_rows_bit_for_bit(rows_scene):
    s = rows_scene
    want, _, owner = s.expected()
    n = len(want)
    assert s.yi.getRenderStats().n_triangles == n and n > 2 * 256, "the flattened triangles, over more than one block"
    got = s.device_rows(n)
    bad = np.flatnonzero((got != want).any(1))
    names = {v: k for k, v in s.tags.items()}
    print(f"{n} rows, {len(set(owner))} objects; rows that differ: {len(bad)}")
    assert len(bad) == 0, [(int(i), names.get(int(owner[i]), "plain mesh"), np.flatnonzero(got[i] != want[i]).tolist()) for i in bad[:8]]
    assert np.array_equal(got, want)
    # what the cases were meant to cover is there
    sizes = [int((owner == oid).sum()) for oid in sorted(set(owner))]
    assert {1, 63, 65, 100} <= set(sizes)
    kinds = [s.objects[oid][0] for oid in sorted(s.objects)]
    assert any(kinds[k] == "instance" and kinds[k + 1] == "mesh" and "instance" in kinds[k + 2:] for k in range(len(kinds) - 2)), "plain meshes between instances"
    flat, smooth = want[owner == s.tags["flat: smoothed after the call"]], want[owner == s.tags["smooth: smoothed before the call"]]
    assert not flat[:, 15].any() and smooth[:, 15].all(), "the flags as they stood at the call"
    assert np.array_equal(flat[:, 0:15], smooth[:, 0:15]), "same base, same matrix: only the vertex normals differ"
    # exported normals: the corner at vertex 0 takes the geometric normal, every other corner M * its normal
    r65 = want[owner == s.tags["65 rotation"]]
    assert np.array_equal(r65[0, 16:19], r65[0, 12:15]) and not np.array_equal(r65[0, 20:23], r65[0, 12:15]) and r65[:, 15].all()
    # the angle-dependent loop gives no normal the index 0, and it smoothed some corners of this base
    angled = mesh_rows(s.meshes[s.objects[s.tags["angle scale"]][1]])
    assert not angled["index0"].any() and want[owner == s.tags["angle scale"]][:, 15].any()


def test_mirror_keeps_the_transformed_base_normal(rows_scene):
    """TriangleInstance::getNormal under a mirroring matrix: M * n normalised, the other way than recNormal of the transformed vertices"""
    s = rows_scene
    want, verts, owner = s.expected()
    got = s.device_rows(len(want))
    for tag in ("65 mirror", "100 mirror"):
        sel = owner == s.tags[tag]
        base = mesh_rows(s.meshes[s.objects[s.tags[tag]][1]])["verts"]
        n_base = normalize(cross(base[:, 1] - base[:, 0], base[:, 2] - base[:, 0]))
        ng = np.ascontiguousarray(got[sel][:, 12:15]).view(F)
        assert np.array_equal(ng.view(U), normalize(mul_vec(MIRROR, n_base)).view(U))
        v = verts[sel]
        recomputed = normalize(cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]))
        d = (ng.astype(np.float64) * recomputed.astype(np.float64)).sum(-1)
        assert (d < -0.999).all(), "it differs in sign from the recomputed normal"


# ---- 2. plain rows are unchanged ------------------------------------------------------------------------------------------------
def test_plain_rows_are_what_the_host_path_makes():
    def build(with_instance):
        s = Scene([CLAY, RUST, VALUE])
        base = s.mesh(strip(4, 21), 1001, BASEMESH)
        ids = [s.mesh(strip(70, 22, mat=1))]
        if with_instance:
            s.instance(base, ROTATE)
        ids.append(s.mesh(with_normals(with_texcoords(strip(33, 23, mat=2), 24), 25)))
        ids.append(s.mesh(strip(6, 26)))
        s.smooth(ids[-1], 181.0)
        s.yi.prepareRender()
        want, _, owner = s.expected()
        return s, s.device_rows(len(want)), want, owner, ids
    s1, got1, want1, owner1, ids1 = build(True)
    s0, got0, want0, owner0, ids0 = build(False)
    assert s0.yi.getInstances() == [] and len(s1.yi.getInstances()) == 1
    assert len(got1) == len(got0) + 4
    assert np.array_equal(got0, want0), "the host path, by the restatement"
    for a, b in zip(ids1, ids0):
        assert np.array_equal(got1[owner1 == a], got0[owner0 == b])
    assert sum(int((owner0 == b).sum()) for b in ids0) == len(got0)


# ---- 3. films, bit for bit, on exact transforms -----------------------------------------------------------------------------------
def quad(a, b, c, d):
    return [a, b, c, d], [(0, 1, 2), (0, 2, 3)]


def assemble(faces, mats):
    v, t, m = [], [], []
    for (fv, ft), mat in zip(faces, mats):
        t += [tuple(len(v) + k for k in tri) for tri in ft]
        v += fv
        m += [mat] * len(ft)
    return {"verts": np.array(v, F), "tris": np.array(t, np.int64), "mat": np.array(m, np.int64)}


def room(mat_floor=0, mat_walls=0):
    """an axis-aligned room, open towards the camera; every vertex a multiple of 1/8"""
    x0, x1, y0, y1, z0, z1 = -2.0, 2.0, -2.0, 2.0, 0.0, 3.0
    faces = [quad((x0, y0, z0), (x1, y0, z0), (x1, y1, z0), (x0, y1, z0)), quad((x0, y0, z1), (x0, y1, z1), (x1, y1, z1), (x1, y0, z1)),
             quad((x0, y1, z0), (x1, y1, z0), (x1, y1, z1), (x0, y1, z1)), quad((x0, y0, z0), (x0, y1, z0), (x0, y1, z1), (x0, y0, z1)),
             quad((x1, y0, z0), (x1, y0, z1), (x1, y1, z1), (x1, y1, z0))]
    return assemble(faces, [mat_floor, mat_walls, mat_walls, mat_walls, mat_walls])


def base_box(mats):
    """0.5 x 0.5 x 0.25, outward normals, 12 triangles: edge products are powers of two, so every normal is a unit vector exactly"""
    x0, y0, z0, x1, y1, z1 = 0.0, 0.0, 0.0, 0.5, 0.5, 0.25
    faces = [quad((x0, y0, z1), (x1, y0, z1), (x1, y1, z1), (x0, y1, z1)), quad((x0, y0, z0), (x1, y0, z0), (x1, y0, z1), (x0, y0, z1)),
             quad((x1, y0, z0), (x1, y1, z0), (x1, y1, z1), (x1, y0, z1)), quad((x1, y1, z0), (x0, y1, z0), (x0, y1, z1), (x1, y1, z1)),
             quad((x0, y1, z0), (x0, y0, z0), (x0, y0, z1), (x0, y1, z1)), quad((x0, y0, z0), (x0, y1, z0), (x1, y1, z0), (x1, y0, z0))]
    return assemble(faces, [mats[k % len(mats)] for k in range(6)])


def box_texcoords(mesh):
    v = mesh["verts"]
    orco = ((v - F((0.25, 0.25, 0.125))) / F((0.25, 0.25, 0.125))).astype(F)      # the box in [-1, 1]^3
    uvs = np.array([(0.125, 0.125), (0.875, 0.125), (0.875, 0.875), (0.125, 0.875)], F)
    return dict(mesh, orco=orco, uv=(uvs, np.array([(0, 1, 2), (0, 2, 3)] * 6, np.int64)))


QUARTER = np.array([[0, -1, 0, 0], [1, 0, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], F)      # a quarter turn about z: entries 0 and +-1
BOX_MATRICES = [translation(-1.25, 0.25, 0.25), QUARTER + translation(1.5, -0.5, 0.5) - IDENTITY,
                (QUARTER @ QUARTER) + translation(0.25, 1.0, 1.25) - IDENTITY]
AREA = {"type": "arealight", "corner": (-0.5, -0.5, 2.875), "point1": (-0.5, 0.5, 2.875), "point2": (0.5, -0.5, 2.875), "color": (1.0, 1.0, 1.0), "power": 25.0,
        "samples": 2}
EMIT = {"type": "light_mat", "color": (1.0, 0.9, 0.7), "power": 6.0}
TEXELS = dict(name="t_box", texels=np.random.default_rng(31).uniform(0.05, 0.95, (4, 4, 4)).astype(F), interpolate="none", clipping="repeat", color_space="LinearRGB")
_layer = dict(type="layer", mode=0, def_val=1.0, upper_value=0.0, colfac=1.0, def_col=(1.0, 0.0, 1.0, 1.0), do_color=True, do_scalar=False, color_input=True,
              upper_color=(0.8, 0.8, 0.8, 1.0))


def mapped(texco):
    return {"type": "shinydiffusemat", "color": (0.8, 0.8, 0.8), "diffuse_reflect": 0.9, "diffuse_shader": "diff",
            "nodes": [dict(_layer, name="diff", input="map"), dict(name="map", type="texture_mapper", texture="t_box", texco=texco, mapping="plain")]}


FILM_CASES = {
    "directlighting, area light": dict(rd=dict(integrator="directlighting"), materials=[CLAY, RUST], box=[1], lights=[AREA]),
    "pathtracing, two bounces": dict(rd=dict(integrator="pathtracing", bounces=2), materials=[CLAY, RUST], box=[1], lights=[AREA]),
    "emitting light_mat on the boxes": dict(rd=dict(integrator="pathtracing", bounces=2), materials=[CLAY, EMIT], box=[1], lights=[AREA]),
    "node material reading orco and UV": dict(rd=dict(integrator="directlighting"), materials=[CLAY, mapped("orco"), mapped("uv")], box=[1, 2], lights=[AREA],
                                              textures=[TEXELS], texcoords=True),
}


def test_exact_transforms_are_exact_on_the_cpu():
    """the film cases rest on this: under translations by multiples of 1/4 and quarter turns, a box with vertices on multiples of 1/8
    and power-of-two edges has the rows of the plain triangles at the transformed vertices, normals included"""
    box = box_texcoords(base_box([1, 2]))
    flags = {"smooth": False, "has_uv": True, "has_orco": True}
    for m in BOX_MATRICES:
        inst, verts = instance_rows(box, m, flags, False, True)
        exact = mul_point(m.astype(np.float64), np.asarray(box["verts"], np.float64)[box["tris"]])
        assert np.array_equal(verts.astype(np.float64), exact), "every transformed coordinate is exact"
        moved = dict(box, verts=verts.reshape(-1, 3), tris=np.arange(36).reshape(12, 3), orco=box["orco"][box["tris"]].reshape(-1, 3))
        plain, _ = plain_rows(moved, False, True)
        assert np.array_equal(inst.view(F), plain.view(F)), "same values (a zero may differ in sign)"
        n = np.ascontiguousarray(inst[:, 12:15]).view(F)
        assert np.array_equal(np.abs(n).sum(-1), np.ones(12, F)) and np.array_equal(np.abs(n).max(-1), np.ones(12, F)), "unit normals along an axis, exactly"


@pytest.mark.parametrize("case", list(FILM_CASES))
def test_films_bit_for_bit(case):
    c = FILM_CASES[case]
    rd = scenes.render_settings(32, 32, 4, **c["rd"])
    box = base_box(c["box"])
    if c.get("texcoords"):
        box = box_texcoords(box)
    films, stats = [], []
    for instanced in (True, False):
        s = Scene(c["materials"], rd=rd, lights=c["lights"], textures=c.get("textures", ()))
        base = s.mesh(box, 1001, BASEMESH)                      # in both scenes: the same objects are made in the same order
        s.mesh(room())
        for m in BOX_MATRICES:
            if instanced:
                s.instance(base, m)
            else:
                _, verts = instance_rows(box, m, {"smooth": False, "has_uv": False, "has_orco": False}, False, False)
                moved = dict(box, verts=verts.reshape(-1, 3), tris=np.arange(36).reshape(12, 3))
                if c.get("texcoords"):                          # the plain scene carries the base's orcos explicitly
                    moved["orco"] = box["orco"][box["tris"]].reshape(-1, 3)
                s.mesh(moved)
        s.yi.setRandState(20240, 3)
        s.yi.render()
        films.append(s.yi.getFilm(32, 32))
        stats.append(s.yi.getRenderStats())
        assert stats[-1].n_triangles == 10 + 3 * 12
        assert len(s.yi.getInstances()) == (3 if instanced else 0)
    a, b = films
    assert a[..., 4].all() and a[..., :3].any()
    print(f"{case}: largest film difference {float(np.abs(a - b).max()):.3g}; rays {stats[0].rays_closest} + {stats[0].rays_shadow}")
    assert np.array_equal(a, b), f"{case}: films differ by up to {float(np.abs(a - b).max())}"
    for k in ("rays_closest", "rays_shadow", "camera_samples"):
        assert getattr(stats[0], k) == getattr(stats[1], k), k


# ---- 4. traversal -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("builder", ["host", "device"])
def test_ray_batches_match_brute_force(builder, monkeypatch):
    monkeypatch.setenv("YAFGPU_BUILD", builder)
    s = Scene([CLAY, RUST])
    base = s.mesh(strip(40, 41, lo=-0.5, hi=0.5), 1001, BASEMESH)
    s.mesh(strip(30, 42, mat=1))
    for m in (ROTATE, SCALE, MIRROR, SHEAR, TRANSLATE):
        s.instance(base, m)
    s.mesh(strip(20, 43))
    s.yi.prepareRender()
    want, verts, _ = s.expected()
    assert s.yi.getRenderStats().n_triangles == len(verts) == 250
    osc = po.OracleScene({"verts": verts, "tri_mat": want[:, 7].astype(np.int32), "vnormals": None, "materials": [CLAY, RUST], "lights": [POINT], "camera": CAMERA})
    rng = np.random.default_rng(5)
    n = 3000
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
    print(f"{builder} builder: {hits} of {n} rays hit; {mism} results differ")
    assert hits > n // 20
    assert mism == 0, f"{mism} ray results differ from the brute force over the restated triangles"


# ---- 5. refusals on the device path -------------------------------------------------------------------------------------------------
def test_a_matrix_that_overflows_a_coordinate_is_refused():
    s = Scene([CLAY], strict=False)
    base = s.mesh(strip(3, 51, lo=1.0, hi=2.0), 1001, BASEMESH)
    s.mesh(strip(2, 52))
    big = np.diag([3e38, 1.0, 1.0, 1.0]).astype(F)              # finite, and 3e38 * x overflows for x > 1.14
    assert np.isfinite(big).all()
    s.instance(base, big)
    assert not s.yi.prepareRender()
    assert "non-finite vertex coordinate" in s.yi.getLastError(), s.yi.getLastError()


# ---- 6. cache invalidation ----------------------------------------------------------------------------------------------------------
def test_one_more_instance_rebuilds_the_scene():
    s = Scene([CLAY])
    base = s.mesh(strip(9, 61), 1001, BASEMESH)
    s.mesh(strip(4, 62))
    s.instance(base, TRANSLATE)
    s.yi.prepareRender()
    assert s.yi.getRenderStats().n_triangles == 13
    s.yi.prepareRender()                                           # nothing changed: the scene is kept
    assert s.yi.getRenderStats().n_triangles == 13
    s.instance(base, ROTATE)
    s.yi.prepareRender()
    assert s.yi.getRenderStats().n_triangles == 22
    want, _, _ = s.expected()
    assert np.array_equal(s.device_rows(22), want)
