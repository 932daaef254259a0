"""The inputs of test_gpu_short_stack.py, certified on the CPU: the jittered sheet and the grazing rays of short_stack_fixture.py
do overflow the device's short traversal stack and make its walks restart, often and several times per ray; the ray batches the rest
of the suite sends hardly ever do.

Everything here runs short_stack_fixture.model_walk, a float64 restatement of the device's walk, over the host-built trees.  It
says what the inputs reach.  It is no reference for the kernels: the GPU tests compare those with the oracle's brute force."""
import functools

import numpy as np
import pytest

from libyafaray_amd import interface
from tests import short_stack_fixture as ss

SEED = {64: 2, 96: 96}      # the sheets' seeds (shared with test_gpu_short_stack.py)
RAY_SEED = 7
N_SAMPLE = 384


@functools.lru_cache(maxsize=None)
def case(g):
    """-> (verts, FlatTree of the host-built tree, its refs, rays, brute-force triangle and distance per ray)"""
    verts, _ = ss.sheet(g, SEED[g])
    nodes, refs, bound, info = interface.build_kdtree(verts, threads=1)
    rays = ss.grazing_rays(N_SAMPLE, RAY_SEED)
    tri, t = ss.brute_hits(verts, rays)
    return verts, ss.FlatTree(nodes, bound), refs, rays, tri, t, info


@functools.lru_cache(maxsize=None)
def walks(g, ring, mode):
    """model_walk of every sampled ray: mode "closest" ends a ray at its closest hit, "pass" lets it pass everything"""
    verts, tree, refs, rays, tri, t, info = case(g)
    z = ss.ends(rays, t if mode == "closest" else None)
    return [ss.model_walk(tree, None, r[:3], r[3:6], float(zi), ring) for r, zi in zip(rays.astype(np.float64), z)]


def first_visits(tree, leaves):
    """the non-empty leaves of a walk in first-visit order"""
    return list(dict.fromkeys(n for n in leaves if tree.arg[n] > 0))


@pytest.mark.parametrize("mode", ["closest", "pass"])
@pytest.mark.parametrize("g", [64, 96])
def test_rings_visit_the_leaves_of_the_unbounded_walk_in_its_order(g, mode):
    """a restart may re-visit leaves; it must not skip or reorder them"""
    tree = case(g)[1]
    full = walks(g, None, mode)
    assert all(w[1] == 0 for w in full), "an unbounded stack never restarts"
    for ring in (ss.RING_TRACE, ss.RING_TS):
        for i, (a, b) in enumerate(zip(full, walks(g, ring, mode))):
            assert a[0] == b[0]
            assert len(first_visits(tree, a[2])) == len([n for n in a[2] if tree.arg[n] > 0]), f"ray {i}: the unbounded walk visits a leaf twice"
            assert first_visits(tree, a[2]) == first_visits(tree, b[2]), f"g {g}, ring {ring}, ray {i}: " + ss.describe_walk(tree, None, case(g)[3][i, :3], case(g)[3][i, 3:6], np.inf, ring)
            assert (b[1] > 0) <= (a[0] > ring), f"ray {i}: a restart without an overflow"


@pytest.mark.parametrize("g", [64, 96])
def test_the_walk_cut_at_the_hit_holds_the_hit_triangle(g):
    """the leaf sequence, cut at the leaf whose cell contains the float64 brute-force hit, has a leaf that references the triangle hit"""
    verts, tree, refs, rays, tri, t, info = case(g)
    assert (tri >= 0).sum() > N_SAMPLE // 4
    for ring in (None, ss.RING_TRACE, ss.RING_TS):
        for i, w in enumerate(walks(g, ring, "closest")):
            if tri[i] < 0:
                continue
            seen = set()
            for n in w[2]:
                seen.update(refs[tree.first[n]:tree.first[n] + tree.arg[n]].tolist() if tree.arg[n] else ())
            assert int(tri[i]) in seen, f"g {g}, ring {ring}, ray {i}: triangle {tri[i]} at {t[i]} is in no leaf of " + ss.describe_walk(tree, None, rays[i, :3], rays[i, 3:6], float(ss.ends(rays, t)[i]), ring)


def shares(g, ring, mode):
    r = np.array([w[1] for w in walks(g, ring, mode)])
    return [float((r >= k).mean()) for k in (1, 2, 3)], int(r.max())


def test_certificate_floors():
    """conditions on the INPUT, met by the model alone: how many of the sampled rays restart"""
    for g in (64, 96):
        info = case(g)[6]
        for ring in (ss.RING_TRACE, ss.RING_TS):
            for mode in ("closest", "pass"):
                s, most = shares(g, ring, mode)
                print(f"sheet({g}) depth {info.max_depth}, ring {ring}, {mode}: restarting >= 1 / 2 / 3 times {s[0]:.3f} / {s[1]:.3f} / {s[2]:.3f}, most {most}; "
                      f"deepest pending list {max(w[0] for w in walks(g, ring, mode))}")
    s, most = shares(64, ss.RING_TRACE, "closest")
    assert s[0] >= 0.35 and s[1] >= 0.10 and most >= 3
    assert shares(64, ss.RING_TS, "pass")[0][0] >= 0.30


def test_the_suites_own_batches_hardly_restart():
    """why this module exists: the rays of test_gpu_treelets.batch_rays on its soup restart in under 2 % of cases"""
    from tests.test_gpu_treelets import SCENES, batch_rays
    sc = SCENES["soup"]()
    nodes, refs, bound, info = interface.build_kdtree(sc["verts"], threads=1)
    rays = batch_rays(sc, 1000, seed=len("soup"))
    tri, t = ss.brute_hits(sc["verts"].reshape(-1, 9), rays)
    share = float((ss.restart_counts(nodes, bound, rays, ss.ends(rays, t), ss.RING_TRACE) > 0).mean())
    print(f"soup: {share:.4f} of the rays restart")
    assert share < 0.02
