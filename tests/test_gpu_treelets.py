"""wf_trace on the treelet layout (kdtree_build.h, TreeletLayout): renders through the wavefront pipeline with leaves inline
in the links and with every non-empty leaf forced through the escape array (YAFGPU_TREELET_INLINE=0) must give the same
films and ray counts, bit for bit, as each other and as the one-kernel pipeline, whose kd_trace walks the 8-byte node array.
The scenes include degenerate trees: a one-leaf tree, a tree with only empty leaves next to the geometry, and stacks of
identical triangles (leaves too large to go inline, kd-restarts)."""
import numpy as np
import pytest

from libyafaray_amd import Interface, scenes
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu


def render(monkeypatch, sc, rd, pipeline, inline=True):
    monkeypatch.setenv("YAFGPU_PIPELINE", pipeline)
    monkeypatch.setenv("YAFGPU_TREELET_INLINE", "1" if inline else "0")
    yi = Interface()
    scenes.load_scene(yi, sc, rd)
    yi.setSerialReplay(False)       # the one-kernel pipeline has the per-sample light ordinal only
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
    sc = SCENES[name]()
    rd = scenes.render_settings(sc["camera"]["resx"], sc["camera"]["resy"], 8, bounces=3)
    films = {k: render(monkeypatch, sc, rd, pl, inline) for k, pl, inline in
             (("inline", "wavefront", True), ("escape", "wavefront", False), ("one_kernel", "megakernel", True))}
    a = films["inline"]
    for k in ("escape", "one_kernel"):
        b = films[k]
        assert a[1].rays_closest == b[1].rays_closest and a[1].rays_shadow == b[1].rays_shadow, f"{name}: ray counts, inline vs {k}"
        assert np.array_equal(a[0], b[0]), f"{name}: film, inline vs {k}"
    assert a[1].rays_closest > 0


@pytest.mark.parametrize("name", ["one_leaf", "stacked_300"])
def test_degenerate_trees_render_like_the_oracle(monkeypatch, name):
    """the oracle's brute-force-checked walk: the same films within the parity tolerance, the same ray counts"""
    sc = SCENES[name]()
    rd = scenes.render_settings(sc["camera"]["resx"], sc["camera"]["resy"], 4, bounces=2)
    for inline in (True, False):
        film, st = render(monkeypatch, sc, rd, "wavefront", inline)
        ofilm, ost = po.OracleScene(sc).render(rd)
        assert st.rays_closest == ost.rays_closest and st.rays_shadow == ost.rays_shadow
        a, b = po.film_to_rgb(film)[..., :3], po.film_to_rgb(ofilm)[..., :3]
        rel = np.abs(a - b) / np.maximum(np.abs(b), 1e-3)
        assert int((rel.max(axis=-1) > 1e-4).sum()) <= 2, f"{name} (inline={inline}): film differs from the oracle"
