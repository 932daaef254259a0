"""wf_trace on the treelet layout (kdtree_build.h, TreeletLayout), with leaves inline in the links and with every non-empty
leaf forced through the escape array (YAFGPU_TREELET_INLINE=0): renders must give the same films and ray counts, bit for bit,
in both forms, and every ray of a batch (intersectRays / shadowRays run wf_trace) the same answer, bit for bit, as the oracle
walking the same tree with the reference's traversal.  The scenes include degenerate trees: a one-leaf tree, a tree with only
empty leaves next to the geometry, and stacks of identical triangles (leaves too large to go inline).  The stacked scenes give
big leaves, not deep lists of pending far children: of these batches' rays under 2 % overflow the short stack and restart
(test_short_stack_host.py has the soup's count); kd-restarts are covered by test_gpu_short_stack.py."""
import os

import numpy as np
import pytest

from libyafaray_amd import Interface, interface, scenes
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

DEVICE_TREE = os.environ.get("YAFGPU_BUILD") == "device"     # the suite also runs with the GPU-built tree


def render(monkeypatch, sc, rd, inline=True):
    monkeypatch.setenv("YAFGPU_TREELET_INLINE", "1" if inline else "0")
    yi = Interface()
    scenes.load_scene(yi, sc, rd)
    yi.render()
    return yi.getFilm(rd["width"], rd["height"]), yi.getRenderStats()


def stacked(n_soup, copies, seed):
    """a Cornell soup with `copies` identical triangles stacked in its middle"""
    sc = scenes.cornell_soup(n_soup, seed=seed, res=(40, 40))
    tri = np.array([[-0.3, 0.1, -0.2], [0.3, 0.1, -0.2], [0.0, 0.2, 0.3]], np.float32)[None]
    sc["verts"] = np.concatenate([sc["verts"], np.repeat(tri, copies, axis=0)]).astype(np.float32)
    sc["tri_mat"] = np.concatenate([sc["tri_mat"], np.zeros(copies, np.int32)])
    return sc


def one_leaf():
    """the light and one floor triangle: too few triangles for the builder to split"""
    sc = scenes.cornell_soup(12, seed=1, res=(32, 32))
    keep = [0, 10, 11]          # a floor triangle, the two light triangles
    sc["verts"] = sc["verts"][keep]
    sc["tri_mat"] = sc["tri_mat"][keep]
    return sc


SCENES = {
    "soup": lambda: scenes.cornell_soup(3000, seed=21, res=(40, 40)),
    "walls": lambda: scenes.cornell_soup(12, seed=2, res=(40, 40)),
    "one_leaf": one_leaf,
    "stacked_64": lambda: stacked(600, 64, 3),
    "stacked_300": lambda: stacked(2000, 300, 4),
}


@pytest.mark.parametrize("name", sorted(SCENES))
def test_inline_escape_and_one_kernel_films_are_identical(monkeypatch, name):
    """inline and escaped leaves: the same films and ray counts.  (The name is the one the suite's records know: the second
    pipeline it also compared against is retired; test_ray_batches_match_the_oracle_on_the_same_tree checks the walk ray by ray.)"""
    sc = SCENES[name]()
    rd = scenes.render_settings(sc["camera"]["resx"], sc["camera"]["resy"], 8, bounces=3)
    a = render(monkeypatch, sc, rd, True)
    b = render(monkeypatch, sc, rd, False)
    assert a[1].rays_closest == b[1].rays_closest and a[1].rays_shadow == b[1].rays_shadow, f"{name}: ray counts, inline vs escape"
    assert np.array_equal(a[0], b[0]), f"{name}: film, inline vs escape"
    assert a[1].rays_closest > 0


def batch_rays(sc, n, seed):
    """(n, 8) rays from inside the box: every other one aimed at a point of a random triangle, every fifth bounded"""
    rng = np.random.default_rng(seed)
    tris = sc["verts"].reshape(-1, 3, 3).astype(np.float64)
    o = rng.uniform(-0.95, 0.95, size=(n, 3))
    d = rng.normal(size=(n, 3))
    aim = np.arange(n) % 2 == 0
    w = rng.dirichlet(np.ones(3), size=n)
    target = np.einsum("nk,nkj->nj", w, tris[rng.integers(0, len(tris), size=n)])
    d[aim] = target[aim] - o[aim]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.concatenate([o, d, np.full((n, 1), 5e-5), np.full((n, 1), -1.0)], axis=1).astype(np.float32)
    rays[::5, 7] = rng.uniform(0.05, 1.5, size=rays[::5].shape[0]).astype(np.float32)
    return rays


@pytest.mark.parametrize("inline", [True, False])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_ray_batches_match_the_oracle_on_the_same_tree(monkeypatch, name, inline):
    monkeypatch.setenv("YAFGPU_TREELET_INLINE", "1" if inline else "0")
    sc = SCENES[name]()
    yi = Interface()
    scenes.load_scene(yi, sc, scenes.render_settings(32, 32, 1))
    yi.prepareRender()
    nodes, refs, bound, info = interface.build_kdtree(sc["verts"], device=DEVICE_TREE)
    assert yi.getRenderStats().kd_nodes == info.n_nodes, "the oracle walks the tree the scene uses"
    osc = po.OracleScene(sc)
    osc.set_tree(nodes, refs, bound)
    rays = batch_rays(sc, 3000, seed=len(name))
    tri, t, bary = yi.intersectRays(rays)
    sh = yi.shadowRays(rays)
    assert (tri >= 0).sum() > len(rays) // 10
    bad = []
    for i, r in enumerate(rays):
        h, oti, ot, ob = osc.intersect(r[:3], r[3:6], float(r[6]), float(r[7]), use_tree=True)
        want_tri, want_t, want_b = (oti, np.float32(ot), ob) if h else (-1, np.float32(0), np.zeros(3, np.float32))
        if tri[i] != want_tri or t[i].tobytes() != want_t.tobytes() or bary[i].tobytes() != want_b.tobytes():
            bad.append((i, "closest", (tri[i], t[i], bary[i]), (want_tri, want_t, want_b)))
        if bool(osc.is_shadowed(r[:3], r[3:6], float(r[6]), float(r[7]), use_tree=True)) != bool(sh[i]):
            bad.append((i, "shadow", sh[i]))
    assert not bad, f"{name} (inline={inline}): {len(bad)} ray answers differ from the oracle, first {bad[:3]}"


@pytest.mark.parametrize("name", ["one_leaf", "stacked_300"])
def test_degenerate_trees_render_like_the_oracle(monkeypatch, name):
    """the oracle's brute-force-checked walk: the same films within the parity tolerance, the same ray counts"""
    sc = SCENES[name]()
    rd = scenes.render_settings(sc["camera"]["resx"], sc["camera"]["resy"], 4, bounces=2)
    for inline in (True, False):
        film, st = render(monkeypatch, sc, rd, inline)
        ofilm, ost = po.OracleScene(sc).render(rd)
        assert st.rays_closest == ost.rays_closest and st.rays_shadow == ost.rays_shadow
        a, b = po.film_to_rgb(film)[..., :3], po.film_to_rgb(ofilm)[..., :3]
        rel = np.abs(a - b) / np.maximum(np.abs(b), 1e-3)
        assert int((rel.max(axis=-1) > 1e-4).sum()) <= 2, f"{name} (inline={inline}): film differs from the oracle"
