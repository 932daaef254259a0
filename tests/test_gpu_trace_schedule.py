"""wf_trace's shrinking queue reservations: a wave sizes each reservation by what is left of the queue (trace_reservation), from
the largest size (512 entries) down to the smallest (kMin).  On a full grid no small input leaves the smallest size, so the
traversal launches run under YAFGPU_TRACE_GRID_CAP here, with one or two workgroups (4 or 8 waves).  A queue starts at 512 only
from 512 * waves * D entries on, so which lengths reach which sizes depends on the constants the library was built with: the
"drain" length of a cap is worked out from them (drain_length: about 20 500 rays for one workgroup and 41 000 for two at D = 8),
starts at 512 and drains through every multiple of 64 down to kMin, which the test checks on the library's own rule before it
believes its answers.  The fixed lengths are the boundaries of the sizes at D = 2 (4096 = 512 * 4 * 2; 6000 passes through every
size there); at D = 8 all of them stay at kMin, where 100 rays leave all static first ranges but one empty and 4095 / 4096 / 4097
end a launch on a full, an exactly spent and a one-entry reservation.  Every ray of a batch must get the oracle's answer on the same
tree, bit for bit, and a render under the cap the oracle's film and ray counts: no queue entry is handed out twice or dropped.
That the switch took effect is read from the library: the workgroups of the last traversal launches (interface.trace_schedule)."""
import numpy as np
import pytest

from libyafaray_amd import Interface, interface, scenes
from oracle import pyoracle as po
from tests.test_gpu_trace_refill import DEVICE_TREE, SCENES, pair, prefix
from tests.test_gpu_treelets import batch_rays

pytestmark = pytest.mark.gpu

LENGTHS = [1, 64, 100, 4095, 4096, 4097, 6000, "drain"]
CAPS = [1, 2]


def waves_of(cap):
    return cap * interface.trace_schedule()["waves_per_group"]


def drain_length(cap):
    """a queue that `cap` workgroups start at the largest size and drain to the smallest: the shortest one that the rule sizes at
    the largest (largest * waves * D), the static first ranges and one more round of reservations of that size, and an odd rest"""
    r, waves = interface.trace_schedule(), waves_of(cap)
    return r["max"] * waves * r["div"] + 2 * waves * r["max"] + 37


def length(n, cap):
    return drain_length(cap) if n == "drain" else n


def reservation_sizes(n, waves):
    """the sizes that a launch of `waves` waves hands out over a queue of n entries by the library's rule, the waves asking in turns
    (wf_trace's refill: static first ranges, then the cursor from waves * b0).  On the device the waves ask side by side, a wave's
    `seen` is older by the other waves' reservations, and a size is at least what this model gives at the same queue position."""
    r = interface.trace_schedule()
    sizes, first_at = [], 0
    if r["static_first"]:
        b0 = interface.trace_reservation(n, 0, waves)
        first_at = waves * b0
        sizes += [b0 for w in range(waves) if w * b0 < n]
    cursor, seen, w = 0, [0] * waves, 0
    while first_at + cursor < n:
        want = interface.trace_reservation(n, seen[w] if r["shrink"] else 0, waves)
        seen[w] = first_at + cursor
        cursor += want
        sizes.append(want)
        w = (w + 1) % waves
    return sizes


_BATCH = {}


def batch(name):
    """the longest batch of a scene and the oracle's answers to it, computed once; the shorter batches are its prefixes"""
    if name not in _BATCH:
        p = pair(name)
        rays = batch_rays(p.sc, max(length(n, cap) for n in LENGTHS for cap in CAPS), seed=40 + len(name))
        _BATCH[name] = (rays, p.oracle(rays))
    return _BATCH[name]


def assert_grids(cap):
    s = interface.trace_schedule()
    assert (s["grid_closest"], s["grid_any"]) == (cap, cap), f"YAFGPU_TRACE_GRID_CAP={cap} did not take effect: the last traversal launches ran {s}"


@pytest.mark.parametrize("cap", CAPS)
def test_the_drain_length_passes_through_every_size(cap):
    """the library's own rule on the drain length: from the largest size through every multiple of 64 to the smallest, while the
    issue's lengths, sized for D = 2, see more than one size only if the library was built so"""
    r, waves = interface.trace_schedule(), waves_of(cap)
    assert r["shrink"] == 1, "the library was built with the comparison rule"
    sizes = reservation_sizes(drain_length(cap), waves)
    print(f"{cap} workgroups, {drain_length(cap)} rays: {len(sizes)} reservations, sizes {sorted(set(sizes), reverse=True)}; "
          f"6000 rays: {sorted(set(reservation_sizes(6000, waves)), reverse=True)}")
    assert sizes[0] == r["max"] and sizes[-1] == r["min"]
    assert set(sizes) == set(range(r["min"], r["max"] + 1, 64))
    # ... and sizes change among the cursor's reservations, not only between the static range and the first of them
    dynamic = sizes[waves:] if r["static_first"] else sizes
    assert dynamic[0] == r["max"] and dynamic.count(r["max"]) >= waves and dynamic.count(r["min"]) >= waves


@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("name", sorted(SCENES))
def test_batches_through_every_reservation_size(monkeypatch, name, cap, n):
    n = length(n, cap)
    rays, want = batch(name)
    p = pair(name)
    monkeypatch.setenv("YAFGPU_TRACE_GRID_CAP", str(cap))
    bad = p.differences(rays[:n], prefix(want, n))
    assert_grids(cap)
    assert not bad, f"{name}, {cap} workgroups, {n} rays: {len(bad)} answers differ from the oracle, first {bad[:3]}"


def test_no_cap_unless_asked(monkeypatch):
    """without the switch a ray batch runs on the full grid (so the cases above would all stay at the smallest size)"""
    monkeypatch.delenv("YAFGPU_TRACE_GRID_CAP", raising=False)
    rays, want = batch("small")
    bad = pair("small").differences(rays[:100], prefix(want, 100))
    s = interface.trace_schedule()
    assert min(s["grid_closest"], s["grid_any"]) > max(CAPS), f"the last traversal launches ran {s}"
    assert not bad


def test_render_under_the_cap_like_the_oracle(monkeypatch):
    """40 x 40 at 4 spp on four waves: film and ray counts are the oracle's, walking the tree the device walks"""
    monkeypatch.setenv("YAFGPU_TRACE_GRID_CAP", "1")
    res, spp = (40, 40), 4
    sc = scenes.cornell_soup(3000, seed=21, res=res)
    rd = scenes.render_settings(res[0], res[1], spp, bounces=3)
    yi = Interface()
    scenes.load_scene(yi, sc, rd)
    yi.render()
    assert_grids(1)
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
