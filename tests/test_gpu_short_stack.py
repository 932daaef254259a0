"""The short traversal stack's overflow and its kd-restart, in all three tree walks: wf_trace<closest>, wf_trace<any> (rings of
kStack - 1 = 7 live entries) and kd_trace_ts under wf_trace_ts (a ring of kStack = 8).  This is where the device deliberately
does what the reference does not, and it meets everything else in the walk: the pending leaf (p_tmax, `z < tmin` once the leaf is
through), the `hit && z <= tmax` end, `!(tmax >= t_exit)`, and seen[] of the transparent-shadow walk, which has to keep a triangle
met again after a restart out of the filter product.

The inputs (short_stack_fixture.py) are a jittered sheet of small triangles and rays that graze it from end to end; a float64
model of the walk certifies, in every test and on the tree the test was handed, that the rays overflow the ring and restart — by
the dozen per hundred, and several times per ray (test_short_stack_host.py holds the floors).  The model certifies inputs only.
The answers are compared with the oracle: its brute force over all triangles, and its walk of the same tree with the reference's
64-entry stack, which never restarts."""
import functools

import numpy as np
import pytest

from libyafaray_amd import Interface, interface, scenes
from oracle import pyoracle as po
from tests import short_stack_fixture as ss
from tests.test_gpu_parity import ABS_FLOOR, RTOL, compare_films
from tests.test_short_stack_host import RAY_SEED, SEED

pytestmark = pytest.mark.gpu

DEVICE_TREE = __import__("os").environ.get("YAFGPU_BUILD") == "device"     # the suite also runs with the GPU-built tree
N_RAYS, N_CERT = 2048, 384
G_SHADOW, SEED_SHADOW = 88, 2      # the render of the transparent-shadow walk: 7744 + 2 triangles


@functools.lru_cache(maxsize=None)
def batch(g):
    """the sheet's scene, the grazing rays and the oracle's brute-force answers to them (shared by all cases on this sheet):
    -> (scene, rays, per ray (hit, triangle, t, barycentrics), per ray occluded)"""
    sc = ss.sheet(g, SEED[g])[1]
    rays = ss.grazing_rays(N_RAYS, RAY_SEED)
    osc = po.OracleScene(sc)
    closest = [osc.intersect(r[:3], r[3:6], float(r[6]), float(r[7]), use_tree=False) for r in rays]
    shadowed = np.array([bool(osc.is_shadowed(r[:3], r[3:6], float(r[6]), float(r[7]), use_tree=False)) for r in rays])
    return sc, rays, closest, shadowed


def setup(monkeypatch, sc, inline, builder):
    """the scene on the device, its tree built by `builder`, and the oracle holding that same tree"""
    monkeypatch.setenv("YAFGPU_TREELET_INLINE", "1" if inline else "0")
    monkeypatch.setenv("YAFGPU_BUILD", builder)
    yi = Interface()
    scenes.load_scene(yi, sc, scenes.render_settings(32, 32, 1))
    yi.prepareRender()
    nodes, refs, bound, info = interface.build_kdtree(sc["verts"], device=builder == "device")
    assert yi.getRenderStats().kd_nodes == info.n_nodes and yi.getRenderStats().kd_leaf_refs == info.n_leaf_refs, "the model and the oracle walk the tree the scene uses"
    osc = po.OracleScene(sc)
    osc.set_tree(nodes, refs, bound)
    return yi, osc, (nodes, bound, info)


def certificate(what, tree, rays, z_end, ring, floor):
    """the share of the first N_CERT rays that restart, by the model, on the tree the test was handed"""
    nodes, bound, info = tree
    r = ss.restart_counts(nodes, bound, rays[:N_CERT], z_end[:N_CERT], ring)
    share = float((r > 0).mean())
    print(f"{what}: tree depth {info.max_depth}, ring {ring}: {share:.3f} of {len(r)} rays restart, {float((r > 1).mean()):.3f} twice or more, at most {int(r.max())} times")
    assert share > 0.0 if floor is None else share >= floor, f"{what}: the input does not reach the restart path often enough"
    return share


CASES = [(g, inline, builder) for g in (64, 96) for inline in (True, False) for builder in ("host", "device")]


@pytest.mark.parametrize("g,inline,builder", CASES)
def test_closest_hits_equal_brute_force_ray_by_ray(monkeypatch, g, inline, builder):
    """wf_trace<closest>: hit or miss, the triangle, t and the barycentrics bit for bit — every ray, no allowance (the jittered
    sheet has no exact distance ties)"""
    sc, rays, closest, _ = batch(g)
    yi, osc, tree = setup(monkeypatch, sc, inline, builder)
    hit_t = np.array([c[2] if c[0] else np.inf for c in closest])
    # the host builder's floor is test_short_stack_host.py's; the device tree is another SAH tree: its share is printed
    certificate(f"sheet({g}), {builder} tree, closest hit", tree, rays, ss.ends(rays, hit_t), ss.RING_TRACE, 0.35 if builder == "host" else None)
    tri, t, bary = yi.intersectRays(rays)
    assert sum(1 for c in closest if c[0]) > N_RAYS // 4 and sum(1 for c in closest if not c[0]) > N_RAYS // 4, "rays that end at a hit and rays that pass everything"
    bad, bad_tree = [], []
    for i, r in enumerate(rays):
        for ref, out in ((closest[i], bad), (osc.intersect(r[:3], r[3:6], float(r[6]), float(r[7]), use_tree=True), bad_tree)):
            h, oti, ot, ob = ref
            want = (oti, np.float32(ot), ob) if h else (-1, np.float32(0), np.zeros(3, np.float32))
            if tri[i] != want[0] or t[i].tobytes() != want[1].tobytes() or bary[i].tobytes() != want[2].tobytes():
                out.append((i, (int(tri[i]), float(t[i])), (want[0], float(want[1]))))
    n_miss = sum(1 for i, *_ in bad if tri[i] < 0)
    first = f"; the first: {ss.describe_walk(tree[0], tree[1], rays[bad[0][0], :3], rays[bad[0][0], 3:6], float(ss.ends(rays, hit_t)[bad[0][0]]), ss.RING_TRACE)}" if bad else ""
    assert not bad, f"sheet({g}), inline={inline}, {builder} tree: {len(bad)} of {N_RAYS} rays differ from brute force ({n_miss} of them reported as misses), {bad[:3]}{first}"
    assert not bad_tree, f"sheet({g}), inline={inline}, {builder} tree: {len(bad_tree)} rays differ from the oracle's walk of the same tree, {bad_tree[:3]}"


@pytest.mark.parametrize("g,inline,builder", CASES)
def test_any_hit_verdicts_equal_brute_force_ray_by_ray(monkeypatch, g, inline, builder):
    """wf_trace<any> on the same rays, the bounded fifth (which ends inside the sheet) included: a ray that finds nothing passes
    everything, the regime that restarts most"""
    sc, rays, _, shadowed = batch(g)
    yi, osc, tree = setup(monkeypatch, sc, inline, builder)
    free = ~shadowed
    assert free.sum() >= N_RAYS / 3, "at least a third of the batch is unoccluded: the all-passing regime is present"
    assert free[::5].any() and shadowed[::5].any() and free[1::5].any()
    sel = np.nonzero(free)[0][:N_CERT]
    certificate(f"sheet({g}), {builder} tree, unoccluded any-hit rays", tree, rays[sel], ss.ends(rays[sel]), ss.RING_TRACE, 0.35 if builder == "host" else None)
    sh = yi.shadowRays(rays).astype(bool)
    bad = np.nonzero(sh != shadowed)[0]
    assert bad.size == 0, (f"sheet({g}), inline={inline}, {builder} tree: {bad.size} of {N_RAYS} verdicts differ from brute force, "
                           f"{int((~sh[bad]).sum())} of them occluded rays reported as free, first {bad[:5].tolist()}")
    by_tree = np.array([bool(osc.is_shadowed(r[:3], r[3:6], float(r[6]), float(r[7]), use_tree=True)) for r in rays])
    assert np.array_equal(sh, by_tree), "verdicts differ from the oracle's walk of the same tree"


def render(sc, rd):
    yi = Interface()
    scenes.load_scene(yi, sc, rd)
    yi.render()
    return yi.getFilm(rd["width"], rd["height"]), yi.getRenderStats()


@pytest.mark.parametrize("opaque_half", [False, True])
def test_transparent_shadows_through_the_sheet(monkeypatch, opaque_half):
    """kd_trace_ts (ring of 8): the receiver's shadow rays graze the transparent sheet from end to end; every triangle passed
    multiplies its filter in once — also one met again after a restart — and, with every other triangle opaque, blocks.  Film
    and ray counts against the oracle's render through the same tree, as test_gpu_parity.py::test_transparent_shadows has it."""
    sc = ss.shadow_scene(G_SHADOW, SEED_SHADOW, opaque_half)
    w, h = sc["camera"]["resx"], sc["camera"]["resy"]
    rd = scenes.render_settings(w, h, 2, integrator="directlighting", raydepth=2, transpShad=True, shadowDepth=8)
    # the certificate: receiver -> light rays pass everything (a transparent triangle does not end them); on the host-built tree the
    # positions of light and receiver were chosen on, and on the tree in use
    rays = ss.receiver_rays(N_CERT, 3)
    host = interface.build_kdtree(sc["verts"], threads=1)
    certificate("receiver -> light, host tree", (host[0], host[2], host[3]), rays, ss.ends(rays), ss.RING_TS, 0.25)
    nodes, refs, bound, info = interface.build_kdtree(sc["verts"], device=DEVICE_TREE)
    if DEVICE_TREE:
        certificate("receiver -> light, device tree", (nodes, bound, info), rays, ss.ends(rays), ss.RING_TS, None)
    film, st = render(sc, rd)
    assert st.kd_nodes == info.n_nodes and st.kd_leaf_refs == info.n_leaf_refs
    osc = po.OracleScene(sc)
    osc.set_tree(nodes, refs, bound)
    ofilm, ost = osc.render(rd)
    assert st.rays_closest == ost.rays_closest and st.rays_shadow == ost.rays_shadow and st.rays_shadow >= w * h
    compare_films(film, ofilm, f"transparent shadows through the sheet (opaque half: {opaque_half})", exact_weights=True)
    # the camera sees the receiver alone, and the filter product really varies over it: against the same receiver without the sheet
    bare = dict(sc, verts=sc["verts"][-2:], tri_mat=sc["tri_mat"][-2:])
    lit = po.film_to_rgb(po.OracleScene(bare).render(rd)[0])[..., :3]
    assert lit.min() > 10 * ABS_FLOOR, "every pixel lies on the lit receiver"
    ratio = po.film_to_rgb(film)[..., :3] / lit
    print(f"filter product over the receiver: min {ratio.min():.3f}, max {ratio.max():.3f}, {len(np.unique(np.round(ratio[..., 0], 3)))} levels in red")
    assert ratio.max() <= 1.0 + 10 * RTOL and len(np.unique(np.round(ratio[..., 0], 3))) >= 8 and ratio.min() < 0.5, "the film is not constant over the receiver"
    if opaque_half:
        assert (ratio.max(axis=-1) == 0.0).any() and (ratio.min(axis=-1) > 0.0).any(), "blocked and filtered rays both"


def test_counting_variant_counts_restarts_and_changes_nothing(monkeypatch):
    """YAFGPU_STATS=1 (wf_trace<*, true>, otherwise run by the benchmark alone) on a path-traced frame of the sheet: film and ray counts
    bit-identical to the plain kernels', restarts counted, and the per-ray counters — node steps, leaves, triangle tests — the same with
    leaves inline and escaped.  (`restarts` also counts walks ahead of a pending leaf: it is not the model's count and is not pinned.)"""
    sc = ss.lit_scene(64, SEED[64])
    rd = scenes.render_settings(48, 48, 4, bounces=2)
    out = {}
    for inline in (True, False):
        monkeypatch.setenv("YAFGPU_TREELET_INLINE", "1" if inline else "0")
        monkeypatch.delenv("YAFGPU_STATS", raising=False)
        plain = render(sc, rd)
        monkeypatch.setenv("YAFGPU_STATS", "1")
        counted = render(sc, rd)
        monkeypatch.delenv("YAFGPU_STATS")
        assert plain[1].rays_closest == counted[1].rays_closest > 0 and plain[1].rays_shadow == counted[1].rays_shadow > 0
        assert np.array_equal(plain[0], counted[0]), f"inline={inline}: the counting kernels render another film"
        st = counted[1]
        print(f"inline={inline}: {st.rays_closest} + {st.rays_shadow} rays, {st.interior_steps} node steps, {st.leaves} leaves, {st.tri_tests} triangle tests, {st.restarts} restarts")
        assert st.restarts > 0 and st.interior_steps > 0 and st.leaves > 0 and st.tri_tests > 0
        out[inline] = (plain[0], (st.rays_closest, st.rays_shadow, st.interior_steps, st.leaves, st.tri_tests))
    assert np.array_equal(out[True][0], out[False][0])
    assert out[True][1] == out[False][1], "inline and escaped leaves: the same rays, node steps, leaves and triangle tests"
