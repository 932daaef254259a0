"""wf_trace's own copy of the triangle records, in kd-leaf order (YAFGPU_TRI_ORDER=leaf, the default) and in id order
(YAFGPU_TRI_ORDER=id, the layout the scene's other arrays keep).  The kernel walks positions in that copy and takes a hit's triangle
id from the record's spare word, so every answer must be the same in both orders, bit for bit, and the oracle's walking the same
tree: ray batches (intersectRays / shadowRays run wf_trace) on soups whose ids are shuffled, with leaves inline and through the
escape array, and with the four material visibilities (the flag travels in the copied record); and renders of the scenes where a
triangle id is used after the hit: a mesh light, smooth vertex normals, uv-mapped textures, instanced geometry (rows made on the
device), and a single triangle whose tree is one leaf."""
import numpy as np
import pytest

from libyafaray_amd import Interface, interface, scenes
from oracle import pyoracle as po
from tests.test_gpu_trace_refill import DEVICE_TREE, VISIBILITIES, Pair, oracle_answers, with_visibilities
from tests.test_gpu_treelets import batch_rays
from tests.test_tri_order_host import shuffled_soup

pytestmark = pytest.mark.gpu

ORDERS = ["leaf", "id"]
LENGTHS = [1, 64, 65, 513]
SCENES = {
    "soup_600": lambda: shuffled_soup(600, 5),
    "soup_3000": lambda: shuffled_soup(3000, 21),
    "visibilities": lambda: with_visibilities(shuffled_soup(600, 5), VISIBILITIES),
}

_SCENES, _PAIRS, _BATCH = {}, {}, {}


def scene(name):
    if name not in _SCENES:
        _SCENES[name] = SCENES[name]()
    return _SCENES[name]


def pair(monkeypatch, name, order, inline=True):
    """the scene on the device with its walk copy in `order`, and the oracle on the same tree (the switches are read at scene creation)"""
    key = (name, order, inline)
    if key not in _PAIRS:
        monkeypatch.setenv("YAFGPU_TRI_ORDER", order)
        monkeypatch.setenv("YAFGPU_TREELET_INLINE", "1" if inline else "0")
        _PAIRS[key] = Pair(scene(name))
    return _PAIRS[key]


def batch(monkeypatch, name):
    """the longest batch of a scene and the oracle's answers to it, computed once; the shorter batches are its prefixes"""
    if name not in _BATCH:
        p = pair(monkeypatch, name, "leaf")
        rays = batch_rays(p.sc, max(LENGTHS), seed=len(name))
        _BATCH[name] = (rays, p.oracle(rays))
    return _BATCH[name]


def positions(sc):
    nodes, refs, bound, info = interface.build_kdtree(sc["verts"], device=DEVICE_TREE)
    return interface.tri_order(refs, len(sc["verts"])), refs


@pytest.mark.parametrize("name", sorted(SCENES))
def test_most_triangles_move(name):
    """otherwise an answer that returned the position instead of the id would go unseen; and the box's wall quads are the triangles
    that many leaves reference"""
    sc = scene(name)
    pos, refs = positions(sc)
    n = len(pos)
    assert (pos != np.arange(n)).sum() >= n // 2
    counts = np.bincount(refs, minlength=n)
    big = np.flatnonzero(np.abs(sc["verts"]).max(axis=(1, 2)) == 1.0)      # walls and lights touch the box
    assert len(big) >= 10 and counts[big].max() > 4 * np.median(counts)


def both_orders(monkeypatch, name, n, inline):
    rays, want = batch(monkeypatch, name)
    rays, want = rays[:n], tuple(w[:n] for w in want)
    got = {}
    for order in ORDERS:
        p = pair(monkeypatch, name, order, inline)
        bad = p.differences(rays, want)
        assert not bad, f"{name}, {n} rays, order {order}, inline {inline}: {len(bad)} answers differ from the oracle, first {bad[:3]}"
        tri, t, bary = p.yi.intersectRays(rays)
        got[order] = (tri.tobytes(), t.tobytes(), bary.tobytes(), p.yi.shadowRays(rays).tobytes())
    assert got["leaf"] == got["id"], f"{name}, {n} rays, inline {inline}: leaf order and id order answer differently"
    return want


@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("name", ["soup_600", "soup_3000"])
def test_batches_in_both_orders_match_the_oracle(monkeypatch, name, n):
    want = both_orders(monkeypatch, name, n, True)
    if n == max(LENGTHS):
        pos, _ = positions(scene(name))
        hit = want[0][want[0] >= 0]
        assert len(hit) > n // 10 and (pos[hit] != hit).sum() > len(hit) // 2, "the hit triangles' positions are not their ids"
        assert want[3].any() and not want[3].all()


@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("name", ["soup_600", "soup_3000"])
def test_batches_through_the_escape_array(monkeypatch, name, n):
    both_orders(monkeypatch, name, n, False)


def test_visibility_travels_in_the_copied_record(monkeypatch):
    sc = scene("visibilities")
    p = pair(monkeypatch, "visibilities", "leaf")
    rng = np.random.default_rng(11)
    n = 513
    tris = sc["verts"].reshape(-1, 3, 3).astype(np.float64)
    o = rng.uniform(-0.95, 0.95, size=(n, 3))
    target = np.einsum("nk,nkj->nj", rng.dirichlet(np.ones(3), size=n), tris[rng.integers(0, len(tris), size=n)])
    d = target - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.concatenate([o, d, np.full((n, 1), 5e-5), np.full((n, 1), -1.0)], axis=1).astype(np.float32)
    want = p.oracle(rays)
    for order in ORDERS:
        bad = pair(monkeypatch, "visibilities", order).differences(rays, want)
        assert not bad, f"order {order}: {len(bad)} answers differ from the oracle, first {bad[:3]}"
    # ... and the flags did decide: the same triangles, all of them `normal`, on the same tree
    nodes, refs, bound, _ = interface.build_kdtree(sc["verts"], device=DEVICE_TREE)
    osc = po.OracleScene(with_visibilities(sc, ["normal"] * 4))
    osc.set_tree(nodes, refs, bound)
    plain = oracle_answers(osc, rays)
    assert (plain[0] != want[0]).any(), "no closest answer depends on the visibility flags"
    assert (plain[3] != want[3]).any(), "no verdict depends on the visibility flags"


# ---- renders: where an id is used after the hit -------------------------------------------------------------------------------
RD = dict(bounces=2, integrator="pathtracing")


def loaded(sc):
    yi = Interface()
    scenes.load_scene(yi, sc, scenes.render_settings(32, 32, 4, **RD))
    return yi


def mesh_light():
    from tests.test_meshlight_host import LAMP, meshlight
    sc = shuffled_soup(300, 7)
    sc["camera"] = dict(sc["camera"], resx=32, resy=32)
    sc["materials"] = sc["materials"] + [LAMP]
    lamp = np.concatenate([scenes._quad((-0.6, -0.6, 0.9), (-0.6, -0.2, 0.9), (-0.2, -0.2, 0.8), (-0.2, -0.6, 0.8)),
                           scenes._quad((0.3, 0.2, 0.85), (0.3, 0.6, 0.85), (0.7, 0.6, 0.9), (0.7, 0.2, 0.9))])
    sc["extra_meshes"] = [{"verts": lamp, "material": len(sc["materials"]) - 1}]
    sc["lights"] = sc["lights"] + [meshlight(2, samples=1, power=4.0)]
    return loaded(sc)


def smooth_normals():
    sc = shuffled_soup(300, 8)
    v = sc["verts"].astype(np.float64)
    ng = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    ng /= np.linalg.norm(ng, axis=1, keepdims=True)
    vn = ng[:, None, :] + np.random.default_rng(9).normal(0.0, 0.2, size=v.shape)
    sc["vnormals"] = (vn / np.linalg.norm(vn, axis=2, keepdims=True)).astype(np.float32)
    return loaded(sc)


def textured():
    from tests.test_gpu_textures import _textured_box
    sc = _textured_box(specular=False)
    sc["camera"] = dict(sc["camera"], resx=32, resy=32)
    return loaded(sc)


def instanced():
    from tests import test_gpu_instances as ti
    c = ti.FILM_CASES["pathtracing, two bounces"]
    s = ti.Scene(c["materials"], rd=scenes.render_settings(32, 32, 4, **RD), lights=c["lights"])
    box = ti.base_box(c["box"])
    base = s.mesh(box, 1001, ti.BASEMESH)
    s.mesh(ti.room())
    for m in ti.BOX_MATRICES:
        s.instance(base, m)
    s.yi.setRandState(20240, 3)
    return s.yi


def one_triangle():
    sc = scenes.cornell_soup(12, seed=1, res=(32, 32))
    sc["verts"], sc["tri_mat"] = sc["verts"][:1], sc["tri_mat"][:1]      # a floor triangle under the area light
    return loaded(sc)


RENDERS = {"mesh_light": mesh_light, "smooth_normals": smooth_normals, "textured_uv": textured, "instanced": instanced, "one_triangle": one_triangle}


@pytest.mark.parametrize("name", sorted(RENDERS))
def test_films_and_ray_counts_are_the_same_in_both_orders(monkeypatch, name):
    films, stats = [], []
    for order in ORDERS:
        monkeypatch.setenv("YAFGPU_TRI_ORDER", order)
        yi = RENDERS[name]()
        yi.render()
        films.append(yi.getFilm(32, 32))
        stats.append(yi.getRenderStats())
    a, b = films
    assert a[..., :3].any(), f"{name}: the film is not black"
    assert stats[0].rays_closest > 0 and stats[0].rays_shadow > 0
    assert stats[0].rays_closest == stats[1].rays_closest and stats[0].rays_shadow == stats[1].rays_shadow, f"{name}: ray counts, leaf vs id"
    assert a.tobytes() == b.tobytes(), f"{name}: films differ between the orders by up to {float(np.abs(a - b).max())}"
    if name == "one_triangle":
        assert stats[0].kd_nodes == 1, "a tree that is a single leaf"
