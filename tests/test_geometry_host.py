"""The CPU twin of tests/test_gpu_geometry.py: the oracle's brute force (OracleScene.intersect / is_shadowed, use_tree=False) and a numpy
float32 restatement (geometry_fixture.tri_test32, surface32) against the float64 references of tests/geometry_fixture.py, on the very
inputs the GPU tests run.  It shows without a GPU that the references and their bands are sound — every decided verdict is met, t, u, v
stay inside the bands —, settles the caps on the undecided share and the floors on decided hits and misses per class, and shows that
every listed misreading of the contract (geometry_fixture.MUTATIONS) is caught by a decided case."""
import functools

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import geometry_fixture as gf

F, D = np.float32, np.float64
CASES = list(range(len(gf.CASE_NAMES)))
IDS = list(gf.CASE_NAMES)
FLOOR = 50      # decided hits and decided misses every class has to hold


def ratio(got, want, band):
    """the worst |error| / (U S) of the rows given: to be compared with K"""
    if len(got) == 0:
        return 0.0
    with np.errstate(all="ignore"):
        return float(np.max(np.abs(np.asarray(got, D) - want) / (band / gf.K)))


def check_rays(what, case, R, tri, t, u, v, occluded):
    """the decided verdicts of a case's rays against what some float32 evaluation answered; prints the worst ratios -> them"""
    hit, miss = R.closest == 1, R.closest == 2
    wrong = np.nonzero((hit & (tri != R.tri)) | (miss & (tri != -1)))[0]
    assert wrong.size == 0, f"{what}, {case.name}: {wrong.size} decided closest rays differ, first {[(int(i), int(tri[i]), int(R.tri[i])) for i in wrong[:5]]}"
    rt, ru, rv = ratio(t[hit], R.t[hit], R.bt[hit]), ratio(u[hit], R.u[hit], R.bu[hit]), ratio(v[hit], R.v[hit], R.bv[hit])
    print(f"{what}, {case.name}: worst error / (U S) over {int(hit.sum())} decided hits: t {rt:.2f}, u {ru:.2f}, v {rv:.2f} (K = {gf.K})")
    assert max(rt, ru, rv) <= gf.K, f"{what}, {case.name}: t, u or v of a decided hit leaves its band"
    sh = R.shadow
    wrong = np.nonzero(((sh == 1) & ~occluded) | ((sh == 2) & occluded))[0]
    assert wrong.size == 0, f"{what}, {case.name}: {wrong.size} decided shadow verdicts differ, first {wrong[:5].tolist()}"
    return rt, ru, rv


def check_pairs(what, case, P, ok, t, u, v):
    """the decided verdicts of (ray, the triangle it was placed at) against a float32 triangle test's; an accepted pair whose determinant
    is clear of eps_tri keeps t, u, v inside the bands, decided or not"""
    wrong = np.nonzero((P.hit & ~ok) | (P.miss & ok))[0]
    assert wrong.size == 0, f"{what}, {case.name}: {wrong.size} decided pairs differ, first {wrong[:5].tolist()}"
    acc = ok & P.above
    rt, ru, rv = ratio(t[acc], P.t[acc], P.bt[acc]), ratio(u[acc], P.u[acc], P.bu[acc]), ratio(v[acc], P.v[acc], P.bv[acc])
    print(f"{what}, {case.name}: worst error / (U S) over {int(acc.sum())} accepted pairs: t {rt:.2f}, u {ru:.2f}, v {rv:.2f} (K = {gf.K})")
    assert max(rt, ru, rv) <= gf.K, f"{what}, {case.name}: t, u or v of an accepted pair leaves its band"
    return rt, ru, rv


def check_caps(case, R, P):
    """the caps on the undecided share and the floors on decided hits and misses, per class: conditions on the inputs and the bands.
    (Rays in the triangles' plane have no hits to count: all of them are decided misses.)"""
    for k, (name, cap) in enumerate(case.classes):
        m = case.cls == k
        und = float((R.closest[m] == 0).mean())
        shm = m & (case.rays[:, 6] == 0)
        und_s = float((R.shadow[shm] == 0).mean()) if shm.any() else 0.0
        und_p = float((~(P.hit | P.miss))[m].mean())
        hits, misses = int((R.closest[m] == 1).sum()), int((R.closest[m] == 2).sum())
        print(f"{case.name}, {name}: {int(m.sum())} rays, undecided closest {und:.3f}, shadow {und_s:.3f}, pairs {und_p:.3f} (cap {cap}); decided hits {hits}, misses {misses}; "
              f"decided pairs: {int(P.hit[m].sum())} hits, {int(P.miss[m].sum())} misses")
        assert max(und, und_s, und_p) <= cap, f"{case.name}, {name}: too many undecided"
        pair_floor = 0 if case.name == "ranges" else FLOOR      # (the ranges' pairs are hits by construction: the range is the ray's)
        assert misses >= FLOOR and int(P.miss[m].sum()) >= pair_floor
        if name == "in the plane":
            assert hits == 0 and misses == int(m.sum()) and bool((np.abs(P.det[m]) == 0).all()), "rays in the triangles' plane: decided misses, by a determinant of exactly zero"
        else:
            assert hits >= FLOOR and int(P.hit[m].sum()) >= FLOOR


@functools.lru_cache(maxsize=None)
def oracle_answers(ci):
    case = gf.all_cases()[ci]
    osc = po.OracleScene(gf.scene_of(case.verts))
    n = len(case.rays)
    tri, t, u, v, occ = np.full(n, -1, np.int64), np.zeros(n, F), np.zeros(n, F), np.zeros(n, F), np.zeros(n, bool)
    for i, r in enumerate(case.rays):
        h, k, tt, bary = osc.intersect(r[:3], r[3:6], float(r[6]), float(r[7]), use_tree=False)
        tri[i], t[i], u[i], v[i] = (k, tt, bary[1], bary[2]) if h else (-1, 0, 0, 0)
        if r[6] == 0:
            occ[i] = bool(osc.is_shadowed(r[:3], r[3:6], 0.0, float(r[7]), use_tree=False))
    osc.close()
    return tri, t, u, v, occ


@pytest.mark.parametrize("ci", CASES, ids=IDS)
def test_inputs_meet_the_caps_and_floors(ci):
    check_caps(gf.all_cases()[ci], gf.decided(ci), gf.decided_pairs(ci))
    assert np.isfinite(gf.all_cases()[ci].rays).all() and (np.abs(gf.all_cases()[ci].rays[:, 3:6]).max(axis=1) > 0).all()


@pytest.mark.parametrize("ci", CASES, ids=IDS)
def test_oracle_brute_force_meets_every_decided_verdict(ci):
    check_rays("oracle", gf.all_cases()[ci], gf.decided(ci), *oracle_answers(ci))


@pytest.mark.parametrize("ci", CASES, ids=IDS)
def test_float32_restatement_meets_every_decided_verdict(ci):
    case = gf.all_cases()[ci]
    check_rays("float32 numpy", case, gf.decided(ci), *gf.brute32(case.verts, case.rays))
    v = case.verts[case.target]
    check_pairs("float32 numpy", case, gf.decided_pairs(ci), *gf.tri_test32(v[:, 0], v[:, 1], v[:, 2], case.rays[:, :3], case.rays[:, 3:6]))


def test_restatement_and_oracle_answer_alike():
    """the numpy restatement is the oracle's brute force bit for bit on the soup's rays: what catches a mutation of the one would catch it
    in the other"""
    case = gf.all_cases()[0]
    a, b = oracle_answers(0), gf.brute32(case.verts, case.rays)
    for x, y in zip(a, b):
        assert np.array_equal(np.asarray(x), np.asarray(y))


def tri_mutation_catches(name):
    """decided cases, over all inputs, that a mutated float32 triangle test gets wrong: verdicts of pairs, and t, u, v of decided hits"""
    verdicts = values = 0
    for ci, case in enumerate(gf.all_cases()):
        P, v = gf.decided_pairs(ci), case.verts[case.target]
        ok, t, u, w = gf.tri_test32(v[:, 0], v[:, 1], v[:, 2], case.rays[:, :3], case.rays[:, 3:6], name)
        verdicts += int((P.hit & ~ok).sum() + (P.miss & ok).sum())
        both = P.hit & ok
        values += int((both & ((np.abs(t - P.t) > P.bt) | (np.abs(u - P.u) > P.bu) | (np.abs(w - P.v) > P.bv))).sum())
    return verdicts, values


@pytest.mark.parametrize("name,equivalent", [(n, e) for n, kind, e in gf.MUTATIONS if kind == "tri"])
def test_triangle_test_mutations_are_caught(name, equivalent):
    verdicts, values = tri_mutation_catches(name)
    print(f"{name}: {verdicts} decided verdicts and {values} values of decided hits differ")
    if equivalent:      # geometry_fixture's docstring: u > 1 and v >= 0 give u + v > 1
        assert verdicts == 0 and values == 0, "this mutation was held to be unobservable"
    else:
        assert verdicts + values > 0


# ---- the surface point -----------------------------------------------------------------------------------------------
def check_surface(what, got):
    sc, (tri, bu, bv, p) = gf.surface_scene()
    val, band, exact = gf.surface(sc, tri, bu, bv, p)
    assert np.array_equal(np.asarray(got["has_uv"], bool), val["has_uv"]), f"{what}: has_uv"
    assert np.array_equal(np.asarray(got["mat"], np.int64), val["mat"]), f"{what}: the material index"
    res = gf.surface_errors(got, val, band, exact)
    for f, (held, excluded, worst, bad) in res.items():
        print(f"{what}: {f}: {held} items held, {excluded} excluded by band, worst error / (U conditioning) {worst:.2f} (K = {gf.K})")
        assert bad.size == 0, f"{what}: {f} leaves its band at {bad.size} items, first {[(int(i), int(tri[i]), float(bu[i]), float(bv[i])) for i in bad[:4]]}"
        assert held >= 0.95 * len(tri), f"{what}: {f}: the band excludes too much"
    # the near-degenerate UVs are what the band excludes, and nothing else
    thin = tri == gf.THIN_UV
    assert res["ds_du"][1] == res["ds_dv"][1] == int(thin.sum()) and not np.isfinite(band["ds_du"][thin]).any()
    return res


def test_surface_exact_cases():
    """what the float64 surface point itself says where the answer is exact"""
    sc, (tri, bu, bv, p) = gf.surface_scene()
    val, band, exact = gf.surface(sc, tri, bu, bv, p)
    mid = (tri == gf.OPPOSED) & (bu == 0.5) & (bv == 0.5)
    assert mid.sum() == 1 and (val["n"][mid] == 0).all() and exact["n"][mid].all(), "opposed normals cancel to the zero vector"
    assert np.array_equal(val["nu"][mid][0], [1, 0, 0]) and np.array_equal(val["nv"][mid][0], [0, 1, 0]), "createCs's x = y = 0 branch"
    assert int(exact["n"].sum()) == 1
    for k, sign in ((gf.ALONG_Z_UP, 1), (gf.ALONG_Z_DOWN, -1), (gf.FLAT_UP, 1), (gf.FLAT_DOWN, -1)):
        m = tri == k
        assert (val["n"][m][:, :2] == 0).all() and (np.sign(val["n"][m][:, 2]) == sign).all()
        assert (val["nu"][m] == [sign, 0, 0]).all() and (val["nv"][m] == [0, 1, 0]).all() and exact["nu"][m].all()
    same = tri == gf.SAME_UV
    e1, e3 = sc["verts"][gf.SAME_UV].astype(D)[1] - sc["verts"][gf.SAME_UV].astype(D)[0], sc["verts"][gf.SAME_UV].astype(D)[2] - sc["verts"][gf.SAME_UV].astype(D)[1]
    frame = np.stack([val["nu"][same], val["nv"][same], val["n"][same]], axis=1)
    assert np.allclose(val["ds_du"][same], frame @ (e1 / np.linalg.norm(e1)), atol=1e-14) and np.allclose(val["ds_dv"][same], frame @ (e3 / np.linalg.norm(e3)), atol=1e-14)
    flat = (val["n"][:, 0] == 0) & (val["n"][:, 1] == 0)
    r2 = val["n"][:, 0] ** 2 + val["n"][:, 1] ** 2
    assert (r2[~flat] >= 1e-12).all(), "normals are drawn with nx^2 + ny^2 = 0 or >= 1e-12"


def test_float32_surface_point_stays_in_band():
    sc, (tri, bu, bv, p) = gf.surface_scene()
    check_surface("float32 numpy", gf.surface32(sc, tri, bu, bv, p))


@pytest.mark.parametrize("name", [n for n, kind, _ in gf.MUTATIONS if kind == "surface"])
def test_surface_mutations_are_caught(name):
    sc, (tri, bu, bv, p) = gf.surface_scene()
    with pytest.raises(AssertionError) as caught:
        check_surface(name, gf.surface32(sc, tri, bu, bv, p, name))
    print(f"{name}: {str(caught.value)[:160]}")
