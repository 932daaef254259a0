"""wf_trace's refill and answer paths: rays enter a wave only at a refill, and a finished ray's answer may wait in its lane for
the next refill, or leave at once when the queue has run dry.  Every ray of a batch (intersectRays / shadowRays run wf_trace)
must get the answer, bit for bit, that the oracle gives walking the same tree with the reference's traversal: for batch lengths
around every refill boundary (the refill threshold, the wave, the reservation of 512 queue entries), for lanes that are handed
a ray that misses the scene bound and never walk, for answers still held when the queue is exhausted, and for triangles whose
material's visibility decides the test.  Two renders exercise the tagged queue entries (the second ray of a shadow pair, the
second pair of a park, the segment parked beside a pair) against the oracle's film and ray counts."""
import os

import numpy as np
import pytest

from libyafaray_amd import Interface, interface, scenes
from oracle import pyoracle as po
from tests.test_gpu_treelets import batch_rays

pytestmark = pytest.mark.gpu

DEVICE_TREE = os.environ.get("YAFGPU_BUILD") == "device"     # the suite also runs with the GPU-built tree

SCENES = {
    "soup": lambda: scenes.cornell_soup(3000, seed=21, res=(40, 40)),
    "small": lambda: scenes.cornell_soup(600, seed=5, res=(32, 32)),
}
LENGTHS = [1, 23, 24, 25, 63, 64, 65, 511, 512, 513, 1537]
VISIBILITIES = ["normal", "no_shadows", "shadow_only", "invisible"]


class Pair:
    """a scene on the device and the oracle walking the same tree"""

    def __init__(self, sc):
        self.sc = sc
        self.yi = Interface()
        scenes.load_scene(self.yi, sc, scenes.render_settings(32, 32, 1))
        self.yi.prepareRender()
        nodes, refs, bound, info = interface.build_kdtree(sc["verts"], device=DEVICE_TREE)
        assert self.yi.getRenderStats().kd_nodes == info.n_nodes, "the oracle walks the tree the scene uses"
        self.osc = po.OracleScene(sc)
        self.osc.set_tree(nodes, refs, bound)
        self.bound = np.asarray(bound, np.float64)

    def oracle(self, rays):
        return oracle_answers(self.osc, rays)

    def differences(self, rays, want):
        """the rays whose device answers are not the oracle's (closest: triangle, t and barycentrics bit for bit)"""
        tri, t, bary = self.yi.intersectRays(rays)
        sh = self.yi.shadowRays(rays)
        w_tri, w_t, w_b, w_sh = want
        bad = []
        for i in range(len(rays)):
            if tri[i] != w_tri[i] or t[i].tobytes() != w_t[i].tobytes() or bary[i].tobytes() != w_b[i].tobytes():
                bad.append((i, "closest", (tri[i], t[i], bary[i]), (w_tri[i], w_t[i], w_b[i])))
            if bool(sh[i]) != bool(w_sh[i]):
                bad.append((i, "shadow", int(sh[i])))
        return bad


def oracle_answers(osc, rays):
    n = len(rays)
    tri = np.full(n, -1, np.int32); t = np.zeros(n, np.float32); bary = np.zeros((n, 3), np.float32); sh = np.zeros(n, np.int32)
    for i, r in enumerate(rays):
        h, oti, ot, ob = osc.intersect(r[:3], r[3:6], float(r[6]), float(r[7]), use_tree=True)
        if h:
            tri[i], t[i], bary[i] = oti, np.float32(ot), ob
        sh[i] = int(bool(osc.is_shadowed(r[:3], r[3:6], float(r[6]), float(r[7]), use_tree=True)))
    return tri, t, bary, sh


_PAIRS = {}


def pair(name):
    if name not in _PAIRS:
        _PAIRS[name] = Pair(SCENES[name]())
    return _PAIRS[name]


_BATCH = {}


def batch(name):
    """the longest batch of a scene and the oracle's answers to it, computed once; the shorter batches are its prefixes"""
    if name not in _BATCH:
        p = pair(name)
        rays = batch_rays(p.sc, max(LENGTHS), seed=len(name))
        _BATCH[name] = (rays, p.oracle(rays))
    return _BATCH[name]


def prefix(want, n):
    return tuple(w[:n] for w in want)


@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("name", sorted(SCENES))
def test_batch_lengths_around_every_refill_boundary(name, n):
    rays, want = batch(name)
    bad = pair(name).differences(rays[:n], prefix(want, n))
    assert not bad, f"{name}, {n} rays: {len(bad)} answers differ from the oracle, first {bad[:3]}"


def outside_rays(p, n, seed):
    """rays that start outside the scene bound and point away from it"""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    centre, half = 0.5 * (p.bound[:3] + p.bound[3:]), 0.5 * float(np.linalg.norm(p.bound[3:] - p.bound[:3]))
    o = centre + d * (half + rng.uniform(0.5, 3.0, size=(n, 1)))
    rays = np.concatenate([o, d, np.full((n, 1), 5e-5), np.full((n, 1), -1.0)], axis=1).astype(np.float32)
    rays[::3, 7] = 2.5
    return rays


@pytest.mark.parametrize("name", sorted(SCENES))
def test_lanes_that_never_walk(name):
    p = pair(name)
    away = outside_rays(p, 200, seed=7)
    tri, t, bary = p.yi.intersectRays(away)
    assert (tri == -1).all() and (t == 0).all(), "rays that miss the scene bound: every closest answer is a miss with t = 0"
    assert (p.yi.shadowRays(away) == 0).all(), "rays that miss the scene bound: no verdict is set"
    walking, want = batch(name)
    mixed = walking[:1000].copy()
    mixed[1::2] = outside_rays(p, 500, seed=8)
    tri, t, bary = p.yi.intersectRays(mixed)
    sh = p.yi.shadowRays(mixed)
    assert (tri[1::2] == -1).all() and (t[1::2] == 0).all() and (sh[1::2] == 0).all(), "every other ray misses the scene bound"
    got = (tri[::2], t[::2], bary[::2], sh[::2])
    w = tuple(x[:1000:2] for x in want)
    same = (got[0] == w[0]) & (got[1].view(np.uint32) == w[1].view(np.uint32)) & (got[2].view(np.uint32) == w[2].view(np.uint32)).all(axis=1) & (got[3] == w[3])
    assert same.all(), f"{name}: walking rays beside lanes that never walk: {np.flatnonzero(~same)[:5]} differ from the oracle"


def occluded_rays(sc, n, seed):
    """rays aimed at an interior point of a soup triangle from 0.05 in front of it"""
    rng = np.random.default_rng(seed)
    tris = sc["verts"].reshape(-1, 3, 3).astype(np.float64)[12:]      # the soup (the ten wall and two light triangles come first)
    t = tris[rng.choice(len(tris), size=n, replace=False)]
    p = t.mean(axis=1)
    nrm = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return np.concatenate([p + 0.05 * nrm, -nrm, np.full((n, 1), 5e-5), np.full((n, 1), -1.0)], axis=1).astype(np.float32)


def front_rays(n, seed):
    """rays from just inside the open front of the box, out of it"""
    rng = np.random.default_rng(seed)
    o = np.concatenate([rng.uniform(-0.9, 0.9, size=(n, 1)), np.full((n, 1), -0.999), rng.uniform(-0.9, 0.9, size=(n, 1))], axis=1)
    d = np.concatenate([rng.uniform(-0.2, 0.2, size=(n, 1)), np.full((n, 1), -1.0), rng.uniform(-0.2, 0.2, size=(n, 1))], axis=1)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([o, d, np.full((n, 1), 5e-5), np.full((n, 1), -1.0)], axis=1).astype(np.float32)


@pytest.mark.parametrize("n", [5, 70])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_answers_still_held_when_the_queue_runs_dry(name, n):
    """fewer rays than the refill threshold, and one more wave's worth than a wave: the last answers have no refill to leave with"""
    p = pair(name)
    assert (p.yi.shadowRays(occluded_rays(p.sc, n, seed=n)) == 1).all(), f"{name}: {n} occluded rays"
    assert (p.yi.shadowRays(front_rays(n, seed=n)) == 0).all(), f"{name}: {n} rays out of the open front"


@pytest.mark.parametrize("name", sorted(SCENES))
def test_short_rays_beside_one_long_ray(name):
    """64 rays that end after a few steps and one that crosses the whole box: the wave goes on for the one ray, with every other answer held or written"""
    p = pair(name)
    s = 1.0 / np.sqrt(3.0)
    diagonal = np.array([[-0.97, -0.97, -0.97, s, s, s, 5e-5, -1.0]], np.float32)
    rays = np.concatenate([occluded_rays(p.sc, 64, seed=3), diagonal])
    bad = p.differences(rays, p.oracle(rays))
    assert not bad, f"{name}: {len(bad)} of 65 answers differ from the oracle, first {bad[:3]}"


def with_visibilities(sc, names):
    """the scene with one material per entry of `names`, assigned to the triangles round robin"""
    out = dict(sc)
    out["materials"] = [{"type": "shinydiffusemat", "color": (0.7, 0.7, 0.7), "diffuse_reflect": 1.0, "visibility": v} for v in names]
    out["tri_mat"] = (np.arange(len(sc["tri_mat"])) % len(names)).astype(np.int32)
    return out


def test_visibility_decides():
    base = SCENES["small"]()
    p = Pair(with_visibilities(base, VISIBILITIES))
    rng = np.random.default_rng(11)
    n = 3000
    tris = base["verts"].reshape(-1, 3, 3).astype(np.float64)
    o = rng.uniform(-0.95, 0.95, size=(n, 3))
    target = np.einsum("nk,nkj->nj", rng.dirichlet(np.ones(3), size=n), tris[rng.integers(0, len(tris), size=n)])
    d = target - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.concatenate([o, d, np.full((n, 1), 5e-5), np.full((n, 1), -1.0)], axis=1).astype(np.float32)
    want = p.oracle(rays)
    bad = p.differences(rays, want)
    assert not bad, f"{len(bad)} answers differ from the oracle, first {bad[:3]}"
    # ... and the flags did decide: the oracle on the same triangles, all of them `normal`, on the same tree
    nodes, refs, bound, _ = interface.build_kdtree(base["verts"], device=DEVICE_TREE)
    plain = po.OracleScene(with_visibilities(base, ["normal"] * 4))
    plain.set_tree(nodes, refs, bound)
    n_tri, n_t, n_b, n_sh = oracle_answers(plain, rays)
    assert (n_tri != want[0]).any(), "no closest answer depends on the visibility flags"
    assert (n_sh != want[3]).any(), "no verdict depends on the visibility flags"


@pytest.mark.parametrize("res,spp,bounces,n_lights", [((4, 4), 1, 1, 1), ((40, 40), 8, 3, 2)])
def test_tagged_queue_entries_render_like_the_oracle(res, spp, bounces, n_lights):
    """a render shorter than one refill, and one with two lights: the second ray of a pair, the second pair of a park and the
    segment parked beside a pair all come through tagged queue entries.  The oracle walks the tree the device walks, as for the
    batches: at 1 spp the camera rays go through the pixel centres, and in this symmetric box those of the image's diagonals meet
    the box's edges exactly, where two walls are hit at the same distance and the order of the tests, i.e. the tree, picks the wall
    (on a tree of its own the oracle traces 25 shadow rays at 4x4 where it traces 24 on this one, and three pixels change their wall)."""
    sc = scenes.cornell_soup(3000, seed=21, res=res, n_lights=n_lights)
    rd = scenes.render_settings(res[0], res[1], spp, bounces=bounces)
    yi = Interface()
    scenes.load_scene(yi, sc, rd)
    yi.render()
    film, st = yi.getFilm(rd["width"], rd["height"]), yi.getRenderStats()
    nodes, refs, bound, info = interface.build_kdtree(sc["verts"], device=DEVICE_TREE)
    assert st.kd_nodes == info.n_nodes, "the oracle walks the tree the scene uses"
    osc = po.OracleScene(sc)
    osc.set_tree(nodes, refs, bound)
    ofilm, ost = osc.render(rd)
    assert st.rays_closest == ost.rays_closest and st.rays_shadow == ost.rays_shadow
    assert st.rays_closest > 0 and st.rays_shadow > 0
    a, b = po.film_to_rgb(film)[..., :3], po.film_to_rgb(ofilm)[..., :3]
    rel = np.abs(a - b) / np.maximum(np.abs(b), 1e-3)
    assert int((rel.max(axis=-1) > 1e-4).sum()) <= 2, "film differs from the oracle"
