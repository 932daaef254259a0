"""The triangle test and the surface point from their definitions in float64: the shared reference of tests/test_geometry_host.py (the
oracle's brute force and a numpy float32 restatement) and tests/test_gpu_geometry.py (tri_test / tri_test_flat, wf_trace, get_surface,
tex_point, tex_point_derivatives), with the inputs both run.

Written from the geometric definition and from the contract in the reference's text — Triangle::intersect (triangle.h:223-259),
updateIntersectionCachedValues (:197-207), Triangle::getSurface (triangle.cc:30-133), createCs__ (vector.h:319-337), the range tests of
TriKdTree::intersect / intersectS (kdtree_triangle.cc:782, :936) and Scene::isShadowed (scene.cc:962-970) — not from the oracle or the
device code.  float32 inputs are widened to float64 and every expression is evaluated there; no float32 rounding is restated.

The bands.  U = 2^-24 is float32's unit roundoff.  A float32 evaluation of u, v or t rounds: the stored edge (1), tvec (1), each component
of a cross product (2 products and a difference: 3), a 3-term dot product (3 products and 2 sums, of which the error analysis counts the
depth: 3), the reciprocal (1) and the final product (1): ten roundings along the longest path, each relative to a quantity no larger than
the scale S below.  K = 16 is the next power of two above ten; it is derived here and not tuned.  The scales are the first-order
conditioning of each quotient, numerator error plus |quotient| times the determinant's error, over |det|:
    S_u = |d||e2| (|tvec| + max(1, |u|) |e1|) / |det|        S_v = |d||e1| (|tvec| + max(1, |v|) |e2|) / |det|
    S_t = |e1||e2| (|tvec| + |t||d|) / |det|                  S_det = |d||e1||e2|
A float32 result may differ from the float64 one by K U S; a comparison whose float64 margin is larger than that is decided, and a
float32 evaluation has to agree with it.  Where eps_tri enters a comparison 4 U eps_tri is added: the float32 eps is the product of
float32 lengths (a square root of a 3-term sum, a max, a product: under four roundings).  Everything else is undecided: float32 may
legitimately go either way there, and nothing is asserted.  Caps on the undecided share (test_geometry_host.py) keep the bands from
hiding a failure.

The surface point's bands are K U times the conditioning of each expression: sum |b_i||n_i| / |sum b_i n_i| for the interpolated
normal, |e1||e2| / |e1 x e2| for a geometric normal, 1 / sqrt(nx^2 + ny^2) for createCs, the |du||dv| sums over |det_uv| and the
cancellation of the numerator vector for dPdU / dPdV.  The exact cases have exact answers: an all-cancelling normal sum stays the zero
vector and takes createCs's x = y = 0 branch, n = (0, 0, +-z) gives (+-1, 0, 0), (0, 1, 0), and identical UVs give the implicit mapping.

MUTATIONS lists misreadings of the contract, applied to the float32 restatements tri_test32 / surface32; every one has to be caught
by a decided case of these inputs.  One of the listed ones cannot be: with `u > 1` dropped the test still rejects, since u > 1 and
v >= 0 give u + v > 1 and v < 0 is rejected on its own — in exact arithmetic the check is redundant.  It stays in the list, marked
equivalent, and the host test shows that it changes no decided verdict; `u + v > 1` dropped stands beside it as the observable
neighbour.

This module imports neither torch nor the device library."""
import functools
from typing import NamedTuple

import numpy as np

F = np.float32
D = np.float64
U = 2.0 ** -24                          # unit roundoff of float32
K = 16                                  # roundings along the longest path (ten), to the next power of two
MIN_RAYDIST = 0.00005                   # ray.h
EPS_FACTOR = D(F(0.1)) * MIN_RAYDIST    # triangle.h:206: 0.1f * MIN_RAYDIST * max(|e1|, |e2|)
UV_DET_MIN = 1e-30                      # triangle.cc:88


def _dot(a, b):
    return (a * b).sum(axis=-1)


def _norm(a):
    return np.sqrt(_dot(a, a))


def _w(x):
    """float32 input, widened"""
    return np.asarray(x, F).astype(D)


# ---- the triangle test ---------------------------------------------------------------------------------------------
class Pairs(NamedTuple):
    """float64 triangle tests of broadcast (triangle, ray) pairs"""
    det: np.ndarray
    eps: np.ndarray
    t: np.ndarray
    u: np.ndarray
    v: np.ndarray
    bt: np.ndarray          # the bands K U S of t, u, v
    bu: np.ndarray
    bv: np.ndarray
    above: np.ndarray       # |det| clear of eps_tri from above: t, u, v and their bands mean something
    hit: np.ndarray         # decided hit
    miss: np.ndarray        # decided miss; neither: undecided


def pairs(a, b, c, o, d):
    """Triangle::intersect by its contract, float64: vertices a, b, c and ray (o, d), (..., 3) float32 arrays that broadcast"""
    a, b, c, o, d = _w(a), _w(b), _w(c), _w(o), _w(d)
    e1, e2, tv = b - a, c - a, o - a
    p = np.cross(d, e2)
    det = _dot(e1, p) + 0.0 * _dot(tv, tv)                                     # (broadcast to the pair's shape)
    q = np.cross(tv, e1)
    ne1, ne2, ntv, nd = _norm(e1), _norm(e2), _norm(tv), _norm(d)
    eps = EPS_FACTOR * np.maximum(ne1, ne2) + 0.0 * det
    ad = np.abs(det)
    with np.errstate(all="ignore"):
        u, v, t = _dot(tv, p) / det, _dot(d, q) / det, _dot(e2, q) / det
        bu = K * U * nd * ne2 * (ntv + np.fmax(1.0, np.abs(u)) * ne1) / ad
        bv = K * U * nd * ne1 * (ntv + np.fmax(1.0, np.abs(v)) * ne2) / ad
        bt = K * U * ne1 * ne2 * (ntv + np.abs(t) * nd) / ad
        bdet = K * U * nd * ne1 * ne2 + 4 * U * eps
        above, below = ad - eps > bdet, eps - ad > bdet
        be = bt + 4 * U * eps
        hit = above & (u > bu) & (1.0 - u > bu) & (v > bv) & (1.0 - (u + v) > bu + bv) & (t - eps > be)
        miss = below | (above & ((u < -bu) | (u - 1.0 > bu) | (v < -bv) | (u + v - 1.0 > bu + bv) | (eps - t > be)))
    return Pairs(det, eps, t, u, v, bt, bu, bv, above, hit, miss)


class Rays(NamedTuple):
    """float64 verdicts of rays against a scene, by brute force over all triangles"""
    closest: np.ndarray     # 0 undecided, 1 decided hit, 2 decided miss
    tri: np.ndarray         # the decided hit's triangle (-1 otherwise), its t, u, v and their bands
    t: np.ndarray
    u: np.ndarray
    v: np.ndarray
    bt: np.ndarray
    bu: np.ndarray
    bv: np.ndarray
    shadow: np.ndarray      # 0 undecided, 1 decided occluded, 2 decided free — of the rays with tmin = 0 (others: 0)


def rays(verts, ray, chunk=256):
    """rays (n, 8: from, dir, tmin, tmax; tmax < 0: unbounded) against triangles (T, 3, 3).  A pair is in range when t >= tmin and
    t < tmax hold by more than its t band (kdtree_triangle.cc:782, :936; a shadow ray's `t >= 0` is implied by t >= eps_tri).  A shadow ray
    with tmin != 0 has its origin moved in float32 first (scene.cc:966): a rounding of the input, not of the triangle test — such rays
    are left out of the shadow verdicts."""
    verts, ray = np.asarray(verts, F).reshape(-1, 3, 3), np.asarray(ray, F).reshape(-1, 8)
    n = len(ray)
    out = Rays(np.zeros(n, np.int8), np.full(n, -1, np.int64), *(np.zeros(n, D) for _ in range(6)), np.zeros(n, np.int8))
    for s in range(0, n, chunk):
        r = ray[s:s + chunk]
        P = pairs(verts[None, :, 0], verts[None, :, 1], verts[None, :, 2], r[:, None, :3], r[:, None, 3:6])
        tmin = r[:, 6].astype(D)[:, None]
        tmax = np.where(r[:, 7] < 0, np.inf, r[:, 7].astype(D))[:, None]
        with np.errstate(all="ignore"):
            H = P.hit & (P.t - tmin > P.bt) & (tmax - P.t > P.bt)
            M = P.miss | (P.above & ((tmin - P.t > P.bt) | (P.t - tmax > P.bt)))
            X = ~(H | M)
            t_hit = np.where(H, P.t, np.inf)
            k = np.argmin(t_hit, axis=1)
            rows = np.arange(len(r))
            upper = t_hit[rows, k] + P.bt[rows, k]
            # the nearest any other candidate can be: its t less its band; an undecided pair without a reliable t can be anywhere
            lower = np.where(H | (X & P.above), P.t - P.bt, np.where(X, -np.inf, np.inf))
            lower[rows, k] = np.inf
            any_h = H.any(axis=1)
            dec_hit = any_h & (lower.min(axis=1) > upper)
        dec_miss = M.all(axis=1)
        sl = slice(s, s + len(r))
        out.closest[sl] = np.where(dec_hit, 1, np.where(dec_miss, 2, 0))
        out.tri[sl] = np.where(dec_hit, k, -1)
        for dst, src in ((out.t, P.t), (out.u, P.u), (out.v, P.v), (out.bt, P.bt), (out.bu, P.bu), (out.bv, P.bv)):
            dst[sl] = np.where(dec_hit, src[rows, k], 0.0)
        out.shadow[sl] = np.where(r[:, 6] == 0, np.where(any_h, 1, np.where(dec_miss, 2, 0)), 0)
    return out


# ---- the float32 restatement (the CPU twin's subject, and what the mutations are applied to) ---------------------------
def _dot32(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross32(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def _normalize32(v):
    ln = _dot32(v, v)
    with np.errstate(all="ignore"):
        inv = np.where(ln != 0, F(1) / np.sqrt(ln), F(1)).astype(F)
    return (v * inv[..., None]).astype(F)


def tri_test32(a, b, c, o, d, mutation=None):
    """Triangle::intersect as a float32 program would run it, one rounding per operation -> (ok, t, u, v); `mutation` applies one of
    MUTATIONS"""
    a, b, c, o, d = (np.asarray(x, F) for x in (a, b, c, o, d))
    e1, e2 = (b - a).astype(F), (c - a).astype(F)
    l1, l2 = np.sqrt(_dot32(e1, e1)), np.sqrt(_dot32(e2, e2))
    ln = np.minimum(l1, l2) if mutation == "eps from min" else np.maximum(l1, l2)
    eps = (EPS_FACTOR * ln.astype(D)).astype(F)
    if mutation == "edges swapped":
        e1, e2 = e2, e1
    with np.errstate(all="ignore"):
        pvec = _cross32(d, e2)
        det = _dot32(e1, pvec) + F(0) * _dot32(o, o)
        ok = ~(det < eps) if mutation == "one-sided det window" else ~((det > -eps) & (det < eps))
        inv_det = F(1) / det
        tvec = (o - a).astype(F)
        u = _dot32(tvec, pvec) * inv_det
        ok &= ~(u < 0) if mutation in ("u > 1 dropped",) else ~((u < 0) | (u > 1))
        qvec = _cross32(tvec, e1)
        v = _dot32(d, qvec) * inv_det
        ok &= ~(v < 0) if mutation == "u + v > 1 dropped" else ~((v < 0) | (u + v > 1))
        t = _dot32(e2, qvec) * inv_det
        ok &= ~(t <= 0) if mutation == "t < eps as t <= 0" else ~(t < eps)
    z = F(0)
    return ok, np.where(ok, t, z).astype(F), np.where(ok, u, z).astype(F), np.where(ok, v, z).astype(F)


def brute32(verts, ray, mutation=None, chunk=256):
    """closest hit and occlusion of rays against all triangles with tri_test32 -> (tri or -1, t, u, v, occluded)"""
    verts, ray = np.asarray(verts, F).reshape(-1, 3, 3), np.asarray(ray, F).reshape(-1, 8)
    n = len(ray)
    tri, occ = np.full(n, -1, np.int64), np.zeros(n, bool)
    t_, u_, v_ = (np.zeros(n, F) for _ in range(3))
    for s in range(0, n, chunk):
        r = ray[s:s + chunk]
        ok, t, u, v = tri_test32(verts[None, :, 0], verts[None, :, 1], verts[None, :, 2], r[:, None, :3], r[:, None, 3:6], mutation)
        tmax = np.where(r[:, 7] < 0, F(np.inf), r[:, 7])[:, None]
        acc = ok & (t >= r[:, 6, None]) & (t < tmax)
        tt = np.where(acc, t, F(np.inf))
        k, rows = np.argmin(tt, axis=1), np.arange(len(r))
        got = acc.any(axis=1)
        sl = slice(s, s + len(r))
        tri[sl] = np.where(got, k, -1)
        t_[sl], u_[sl], v_[sl] = (np.where(got, x[rows, k], F(0)) for x in (t, u, v))
        occ[sl] = (ok & (t >= 0) & (t < tmax)).any(axis=1)
    return tri, t_, u_, v_, occ


# ---- the surface point ---------------------------------------------------------------------------------------------
def _unit(v):
    """Vec3::normalize (vector.h:227-238): a zero vector stays zero"""
    ln = _norm(v)
    with np.errstate(all="ignore"):
        return np.where((ln != 0)[..., None], v / ln[..., None], v)


def _cond_cross(x, y):
    with np.errstate(all="ignore"):
        return K * U * _norm(x) * _norm(y) / _norm(np.cross(x, y))


def create_cs(n):
    """createCs__ (vector.h:319-337), float64 -> (nu, nv)"""
    flat = (n[..., 0] == 0) & (n[..., 1] == 0)
    with np.errstate(all="ignore"):
        dd = 1.0 / np.sqrt(n[..., 1] ** 2 + n[..., 0] ** 2)
        nu = np.stack([n[..., 1] * dd, -n[..., 0] * dd, 0.0 * dd], axis=-1)
    nv = np.cross(n, nu)
    sign = np.where(n[..., 2] < 0, -1.0, 1.0)
    nu = np.where(flat[..., None], np.stack([sign, 0 * sign, 0 * sign], axis=-1), nu)
    nv = np.where(flat[..., None], np.array([0.0, 1.0, 0.0]), nv)
    return nu, nv


SURFACE_FIELDS = ("n", "ng", "nu", "nv", "orco_p", "orco_ng", "uv", "ds_du", "ds_dv")


def surface(sc, tri, bu, bv, p):
    """Triangle::getSurface by its contract, float64, of the items (triangle, bu, bv, p) of the surface scene `sc` ->
    (values, bands, exact): dicts by SURFACE_FIELDS of (n, k) arrays, plus "has_uv" and "mat" in values; exact[field] marks the items
    whose answer has no band (the exact cases); bands may be inf or nan where the expression is ill-conditioned: the caller excludes and
    counts those"""
    tri = np.asarray(tri)
    vt, vn = _w(sc["verts"][tri]), _w(sc["vn"][tri])
    a, b, c = vt[:, 0], vt[:, 1], vt[:, 2]
    e1, e2 = b - a, c - a
    ng = _unit(np.cross(e1, e2))
    b_ng = _cond_cross(e1, e2)
    bw = np.stack([1.0 - _w(bu) - _w(bv), _w(bu), _w(bv)], axis=-1)              # b_0, b_1, b_2 (triangle.h:253-255, triangle.cc:34)
    val, band, exact = {}, {}, {}
    # the normal (triangle.cc:36-45): a corner without a normal takes ng
    has_n = (vn != 0).any(axis=-1)                                               # (n, 3)
    corner = np.where(has_n[..., None], vn, ng[:, None, :])
    smooth = sc["mesh_smooth"][tri]
    total = (bw[..., None] * corner).sum(axis=1)
    n = np.where(smooth[:, None], _unit(total), ng)
    with np.errstate(all="ignore"):
        b_n = K * U * (np.abs(bw) * _norm(corner)).sum(axis=1) / _norm(total) + np.where((~has_n).any(axis=1), b_ng, 0.0)
    cancelled = smooth & (_norm(total) == 0)
    b_n = np.where(smooth, np.where(cancelled, 0.0, b_n), b_ng)
    nu, nv = create_cs(n)
    flat = (n[:, 0] == 0) & (n[:, 1] == 0)
    with np.errstate(all="ignore"):
        b_nu = (2 * b_n + K * U) / np.sqrt(n[:, 0] ** 2 + n[:, 1] ** 2)
    b_nu = np.where(flat, 0.0, b_nu)
    val.update(n=n, ng=ng, nu=nu, nv=nv)
    band.update(n=b_n, ng=b_ng, nu=b_nu, nv=np.where(flat, 0.0, b_nu + b_n + K * U))
    exact.update(n=cancelled, nu=flat, nv=flat)
    # orco (:47-64) and UV (:70-79, :108-109)
    oc = _w(sc["orco"][tri])
    has_orco, has_uv = sc["has_orco"][tri], sc["has_uv"][tri]
    val["orco_p"] = np.where(has_orco[:, None], (bw[..., None] * oc).sum(axis=1), _w(p))
    band["orco_p"] = np.where(has_orco, K * U * (np.abs(bw) * _norm(oc)).sum(axis=1), 0.0)
    exact["orco_p"] = ~has_orco
    o1, o2 = oc[:, 1] - oc[:, 0], oc[:, 2] - oc[:, 0]
    val["orco_ng"] = np.where(has_orco[:, None], _unit(np.cross(o1, o2)), ng)
    band["orco_ng"] = np.where(has_orco, _cond_cross(o1, o2), b_ng)
    uv = _w(sc["uv"][tri])
    val["uv"] = np.where(has_uv[:, None], (bw[..., None] * uv).sum(axis=1), 0.0)
    band["uv"] = np.where(has_uv[:, None], K * U * (np.abs(bw)[..., None] * np.abs(uv)).sum(axis=1), 0.0).max(axis=1)
    exact["uv"] = ~has_uv
    val["has_uv"], val["mat"] = has_uv, sc["mat"][tri]
    # dPdU, dPdV (:80-130)
    du_1, du_2 = uv[:, 0, 0] - uv[:, 2, 0], uv[:, 1, 0] - uv[:, 2, 0]
    dv_1, dv_2 = uv[:, 0, 1] - uv[:, 2, 1], uv[:, 1, 1] - uv[:, 2, 1]
    det = du_1 * dv_2 - dv_1 * du_2
    mapped = has_uv & (np.abs(det) > UV_DET_MIN)
    dp_1, dp_2 = a - c, b - c
    with np.errstate(all="ignore"):
        c_det = np.where(mapped, K * U * (np.abs(du_1 * dv_2) + np.abs(dv_1 * du_2)) / np.abs(det), 0.0)
        # whether float32 takes the mapped branch, and with which sign, is decided only where the determinant is clear of zero by its
        # own band; identical UVs give exactly zero in any precision
        unclear = has_uv & (det != 0) & ~(c_det < 0.25)
        for name, x, y, fx, fy, fall in (("ds_du", dp_1, dp_2, dv_2, -dv_1, e1), ("ds_dv", dp_2, dp_1, du_1, -du_2, c - b)):
            num = fx[:, None] * x + fy[:, None] * y
            vec = np.where(mapped[:, None], num / det[:, None], fall)
            dirn = _unit(vec)
            b_dir = np.where(mapped, K * U * (np.abs(fx) * _norm(x) + np.abs(fy) * _norm(y)) / _norm(num) + c_det, K * U)
            val[name] = np.stack([_dot(nu, dirn), _dot(nv, dirn), _dot(n, dirn)], axis=-1)
            band[name] = np.where(unclear, np.inf, b_dir + np.maximum(band["nv"], b_n) + K * U)
    return val, band, exact


def surface32(sc, tri, bu, bv, p, mutation=None):
    """the same as a float32 program would run it -> dict of float32 arrays by SURFACE_FIELDS, plus has_uv and mat"""
    tri = np.asarray(tri)
    vt, vn = sc["verts"][tri].astype(F), sc["vn"][tri].astype(F)
    a, b, c = vt[:, 0], vt[:, 1], vt[:, 2]
    e1, e2, e3 = (b - a).astype(F), (c - a).astype(F), (c - b).astype(F)
    ng = _normalize32(_cross32(e1, e2))
    bu, bv = np.asarray(bu, F), np.asarray(bv, F)
    w0, w1, w2 = (F(1) - bu - bv)[:, None], bu[:, None], bv[:, None]
    if mutation == "v and w swapped in the normal":
        w1, w2 = w2, w1
    has_n = (vn != 0).any(axis=-1)
    corner = np.where(has_n[..., None], vn, ng[:, None, :]).astype(F)
    smooth = has_n.any(axis=1)
    n = np.where(smooth[:, None], _normalize32(corner[:, 0] * w0 + corner[:, 1] * w1 + corner[:, 2] * w2), ng).astype(F)
    w1, w2 = bu[:, None], bv[:, None]
    flat = (n[:, 0] == 0) & (n[:, 1] == 0)
    with np.errstate(all="ignore"):
        dd = F(1) / np.sqrt(n[:, 1] * n[:, 1] + n[:, 0] * n[:, 0])
        nu = np.stack([n[:, 1] * dd, -n[:, 0] * dd, np.zeros_like(dd)], axis=-1).astype(F)
        nv = _cross32(n, nu)
    sign = np.where(n[:, 2] < 0, F(-1), F(1))
    nu = np.where(flat[:, None], np.stack([sign, 0 * sign, 0 * sign], axis=-1), nu).astype(F)
    nv = np.where(flat[:, None], np.array([0, 1, 0], F), nv).astype(F)
    out = dict(n=n, ng=ng, nu=nu, nv=nv, mat=sc["mat"][tri])
    oc, has_orco = sc["orco"][tri].astype(F), sc["has_orco"][tri]
    out["orco_p"] = np.where(has_orco[:, None], oc[:, 0] * w0 + oc[:, 1] * w1 + oc[:, 2] * w2, np.asarray(p, F)).astype(F)
    out["orco_ng"] = np.where(has_orco[:, None], _normalize32(_cross32((oc[:, 1] - oc[:, 0]).astype(F), (oc[:, 2] - oc[:, 0]).astype(F))), ng).astype(F)
    uv = sc["uv"][tri].astype(F)
    has_uv = np.ones_like(sc["has_uv"][tri]) if mutation == "has_uv ignored" else sc["has_uv"][tri]
    out["has_uv"] = has_uv
    out["uv"] = np.where(has_uv[:, None], uv[:, 0] * w0 + uv[:, 1] * w1 + uv[:, 2] * w2, F(0)).astype(F)
    du_1, du_2, dv_1, dv_2 = uv[:, 0, 0] - uv[:, 2, 0], uv[:, 1, 0] - uv[:, 2, 0], uv[:, 0, 1] - uv[:, 2, 1], uv[:, 1, 1] - uv[:, 2, 1]
    det = du_1 * dv_2 - dv_1 * du_2
    mapped = has_uv & (np.abs(det) > F(UV_DET_MIN))
    with np.errstate(all="ignore"):
        inv = (F(1) / det)[:, None]
        dp_1, dp_2 = (-e2, -e3) if mutation != "dPdU from (e1, e2)" else (e1, e2)
        dp_du = np.where(mapped[:, None], (dp_1 * dv_2[:, None] - dp_2 * dv_1[:, None]) * inv, e1).astype(F)
        dp_dv = np.where(mapped[:, None], (dp_2 * du_1[:, None] - dp_1 * du_2[:, None]) * inv, e3).astype(F)
    for name, vec in (("ds_du", _normalize32(dp_du)), ("ds_dv", _normalize32(dp_dv))):
        out[name] = np.stack([_dot32(nu, vec), _dot32(nv, vec), _dot32(n, vec)], axis=-1).astype(F)
    return out


# (name, which restatement it is applied to, equivalent: changes no decided verdict — see the module's docstring)
MUTATIONS = [("edges swapped", "tri", False), ("eps from min", "tri", False), ("t < eps as t <= 0", "tri", False), ("one-sided det window", "tri", False),
             ("u > 1 dropped", "tri", True), ("u + v > 1 dropped", "tri", False), ("v and w swapped in the normal", "surface", False),
             ("dPdU from (e1, e2)", "surface", False), ("has_uv ignored", "surface", False)]


# ---- the inputs ----------------------------------------------------------------------------------------------------
class Case(NamedTuple):
    name: str
    verts: np.ndarray       # (T, 3, 3) float32
    rays: np.ndarray        # (n, 8) float32
    target: np.ndarray      # (n,) the triangle every ray was placed at: the pair op 29 tests
    cls: np.ndarray         # (n,) index into classes
    classes: tuple          # (name, cap on the undecided share)


def _tri_frame(a, b, c):
    e1, e2 = b - a, c - a
    nrm = np.cross(e1, e2)
    return e1, e2, nrm / np.linalg.norm(nrm)


def _aim(o, target, rng, scale=True):
    """a float32 ray from o through target; the direction is of unit length, scaled by up to 4 either way, or (scale=False) as long as
    the way to the target"""
    o = np.asarray(o, D).astype(F)
    d = np.asarray(target, D) - o.astype(D)
    if scale:
        d = d / np.linalg.norm(d) * np.exp(rng.uniform(np.log(0.25), np.log(4.0)))
    return np.concatenate([o, d.astype(F), [F(0), F(-1)]]).astype(F)


def random_triangles(rng, n, lo=1e-3, hi=10.0, extent=50.0):
    """sizes log-uniform in lo..hi, a third needles (aspect 1e-3..1e-1: a ray within K U / aspect of a needle's plane is undecided by
    its determinant, and a soup ray meets a hundred needles; slivers with one edge 1e-6..1e-3 of the other), one in
    sixteen far from the origin (offset 1e4, size 1)"""
    out = np.zeros((n, 3, 3), D)
    i = 0
    while i < n:
        size = np.exp(rng.uniform(np.log(lo), np.log(hi)))
        a = rng.uniform(-extent, extent, 3)
        if i % 16 == 5:
            size, a = 1.0, a + 1e4 * np.sign(rng.normal(size=3))
        x = rng.normal(size=3); x /= np.linalg.norm(x)
        y = np.cross(x, rng.normal(size=3)); y /= np.linalg.norm(y)
        if i % 3 == 1:
            thin = np.exp(rng.uniform(np.log(1e-3), np.log(1e-1)))
            b, c = a + size * x, a + size * (rng.uniform(0.2, 0.8) * x + thin * y)
        elif i % 12 == 2:
            short = np.exp(rng.uniform(np.log(1e-6), np.log(1e-3)))
            b, c = a + size * short * y, a + size * x
        else:
            b, c = a + size * (x + rng.uniform(-0.3, 0.3) * y), a + size * (rng.uniform(-0.3, 0.7) * x + rng.uniform(0.4, 1.0) * y)
        out[i] = a, b, c
        r = out[i].astype(F).astype(D)
        i += bool(np.linalg.norm(np.cross(r[1] - r[0], r[2] - r[0])) > 0)          # (again, should float32 have collapsed it)
    return out.astype(F)


@functools.lru_cache(maxsize=None)
def case_soup(n_tris=512, n_rays=8192, seed=11):
    """(a) a soup in a 100-unit volume; rays aimed at and round triangles (a wider range of barycentrics than the triangle's), grazing
    ones, rays from within eps_tri of a triangle's plane, and rays between random points"""
    rng = np.random.default_rng(seed)
    verts = random_triangles(rng, n_tris)
    vd = verts.astype(D)
    ray, target, cls = [], [], []
    for i in range(n_rays):
        k = int(rng.integers(n_tris))
        a, b, c = vd[k]
        e1, e2, nrm = _tri_frame(a, b, c)
        size = max(np.linalg.norm(e1), np.linalg.norm(e2))
        kind = i % 8
        bu, bv = rng.uniform(-0.3, 1.1), rng.uniform(-0.3, 1.1)
        if kind < 4 and bu + bv > 1 and rng.random() < 0.6:
            bu, bv = 1 - bu, 1 - bv
        p = a + bu * e1 + bv * e2
        if kind == 7:          # between random points of the volume
            r = _aim(rng.uniform(-50, 50, 3), rng.uniform(-50, 50, 3), rng)
        elif kind == 6:        # from just off the plane, inside eps_tri and outside
            h = EPS_FACTOR * size * rng.choice([0.2, 0.5, 2.0, 4.0])
            w = nrm * rng.choice([-1, 1]) + 0.3 * rng.normal(size=3)
            w /= abs(np.dot(w, nrm))
            r = _aim(p - h * w, p + size * w, rng, scale=False)
        else:
            tilt = rng.uniform(0, 1.0) if kind < 5 else rng.uniform(5.0, 200.0)         # grazing: far along the plane
            inplane = np.cross(nrm, rng.normal(size=3)); inplane /= np.linalg.norm(inplane)
            w = nrm * rng.choice([-1, 1]) + tilt * inplane
            w /= np.linalg.norm(w)
            r = _aim(p + w * size * np.exp(rng.uniform(np.log(0.1), np.log(100.0))), p, rng)
        ray.append(r); target.append(k); cls.append(0)
    return Case("soup", verts, np.array(ray, F), np.array(target), np.array(cls), (("soup", 0.10),))


RINGS = (-64, -8, -2, 2, 8, 64)          # bands outside (-) and inside (+)
DISTANCES = (0.1, 1.0, 10.0, 100.0)      # triangle sizes


def _placed(verts, tris, rng, distances=DISTANCES, spots=(0.2, 0.5, 0.85), near=10):
    """rays at RINGS bands inside and outside each edge and each vertex of the triangles `tris`, from both sides, from `distances`
    triangle sizes away, and rays that start within eps_tri of the plane -> (rays, target, class: 0 edge, 1 vertex, 2 plane)"""
    vd = verts.astype(D)
    ray, target, cls = [], [], []
    for k in tris:
        a, b, c = vd[k]
        e1, e2, nrm = _tri_frame(a, b, c)
        size = max(np.linalg.norm(e1), np.linalg.norm(e2))
        centre = (a + b + c) / 3
        for side in (-1, 1):
            for dist in distances:
                w = side * nrm + rng.uniform(-1, 1) * e1 / np.linalg.norm(e1) + rng.uniform(-1, 1) * e2 / np.linalg.norm(e2)
                o = (centre + dist * size * w / np.linalg.norm(w)).astype(F)
                # edges: (start, along, inward per unit of the barycentric that vanishes there, which bands)
                for start, along, inward, which in ((a, e1, e2, "v"), (a, e2, e1, "u"), (b, c - b, -(e1 + e2) / 2, "uv")):
                    for s in spots:
                        q = start + s * along
                        P = pairs(a.astype(F), b.astype(F), c.astype(F), o, (q - o.astype(D)).astype(F))
                        bb = {"u": P.bu, "v": P.bv, "uv": P.bu + P.bv}[which]
                        # moving by x * inward changes that barycentric by x (edge bc: u + v by -x, for inward = -(e1 + e2) / 2)
                        for ring in RINGS:
                            ray.append(_aim(o, q + ring * float(bb) * inward, rng)); target.append(k); cls.append(0)
                for vtx in (a, b, c):
                    P = pairs(a.astype(F), b.astype(F), c.astype(F), o, (vtx - o.astype(D)).astype(F))
                    for ring in RINGS:      # towards the centroid by f moves every barycentric condition by at least f / 3
                        ray.append(_aim(o, vtx + 3 * ring * float(P.bu + P.bv) * (centre - vtx), rng)); target.append(k); cls.append(1)
            for h in (0.1, 0.3, 0.5, 2.0, 3.0, 8.0):      # starting off the plane by h * eps_tri
                for _ in range(near):
                    bu, bv = rng.uniform(0.1, 0.4), rng.uniform(0.1, 0.4)
                    w = side * nrm + 0.4 * rng.uniform(-1, 1) * e1 / np.linalg.norm(e1)
                    w /= abs(np.dot(w, nrm))
                    q = a + bu * e1 + bv * e2
                    ray.append(_aim(q - h * EPS_FACTOR * size * w, q + size * w, rng, scale=False)); target.append(k); cls.append(2)
    return np.array(ray, F), np.array(target), np.array(cls)


PLACED_CLASSES = (("edges", 0.25), ("vertices", 0.25), ("near the plane", 0.25))


@functools.lru_cache(maxsize=None)
def case_single(which):
    """(b) one triangle, a one-leaf tree: of size 1 at the origin, or of size 0.01 far from it"""
    rng = np.random.default_rng(21 + which)
    tri = np.array([[0.3, -0.2, 0.1], [1.7, 0.4, -0.3], [0.1, 1.1, 0.9]], D)
    if which == 1:
        tri = tri * 0.01 + np.array([50.0, -30.0, 20.0])
    verts = tri.astype(F)[None]
    r, t, c = _placed(verts, [0], rng)
    return Case(f"single {which}", verts, r, t, c, PLACED_CLASSES)


@functools.lru_cache(maxsize=None)
def case_fan_strip():
    """(c) a fan of 8 triangles round a shared vertex (a shallow cone) and a strip of 8 with shared edges (gently folded), apart from each
    other: a decided ray has to name the right neighbour"""
    rng = np.random.default_rng(31)
    apex = np.array([0.0, 0.0, 0.4])
    rim = [np.array([1.5 * np.cos(2 * np.pi * k / 8 + 0.1), 1.5 * np.sin(2 * np.pi * k / 8 + 0.1), 0.05 * (-1) ** k]) for k in range(8)]
    fan = [(apex, rim[k], rim[(k + 1) % 8]) for k in range(8)]
    pts = [np.array([6.0 + 0.7 * (k // 2), (k % 2) * 1.1 + 0.1 * k, 0.15 * np.sin(1.3 * k)]) for k in range(10)]
    strip = [(pts[k], pts[k + 1], pts[k + 2]) if k % 2 == 0 else (pts[k + 1], pts[k], pts[k + 2]) for k in range(8)]
    verts = np.array(fan + strip, D).astype(F)
    r, t, c = _placed(verts, range(16), rng, distances=(0.3, 30.0), spots=(0.5,), near=2)
    return Case("fan and strip", verts, r, t, c, PLACED_CLASSES)


@functools.lru_cache(maxsize=None)
def case_plane(axis):
    """(d) 64 disjoint triangles in one axis-aligned plane: the scene's bound has zero thickness.  Crossing rays, perpendicular
    axis-parallel rays, and rays lying in the plane, which miss: their determinant is exactly zero"""
    rng = np.random.default_rng(41 + axis)
    i, j = [k for k in range(3) if k != axis]
    level = F(0.75)
    verts = np.zeros((64, 3, 3), D)
    for k in range(64):
        base = np.array([(k % 8) * 1.25, (k // 8) * 1.25])
        pts = base + np.array([[0.1, 0.1], [1.1, 0.2], [0.3, 1.1]]) + rng.uniform(-0.08, 0.08, (3, 2))
        if k % 2:
            pts = pts[::-1]
        verts[k, :, i], verts[k, :, j], verts[k, :, axis] = pts[:, 0], pts[:, 1], level
    verts = verts.astype(F)
    vd = verts.astype(D)
    ray, target, cls = [], [], []
    for n in range(768):
        k = int(rng.integers(64))
        a, b, c = vd[k]
        bu, bv = rng.uniform(-0.2, 1.0), rng.uniform(-0.2, 1.0)
        p = a + bu * (b - a) + bv * (c - a)
        kind = n % 3
        if kind == 0:      # crossing
            w = rng.normal(size=3); w[axis] = rng.choice([-1, 1]) * rng.uniform(0.05, 2.0)
            r = _aim(p + w * rng.uniform(0.5, 20.0), p, rng)
        elif kind == 1:    # perpendicular, axis-parallel: the other two components are exactly zero
            o = p.astype(F).astype(D); o[axis] = level + rng.choice([-1, 1]) * rng.uniform(0.5, 20.0)
            r = _aim(o, np.where(np.arange(3) == axis, float(level), o), rng)
        else:              # in the plane
            o = p + np.where(np.arange(3) == axis, 0.0, rng.uniform(-3, 3, 3)); o[axis] = level
            q = p.copy(); q[axis] = level
            r = _aim(o, q, rng)
        ray.append(r); target.append(k); cls.append(1 if kind == 2 else 0)
    return Case(f"plane {axis}", verts, np.array(ray, F), np.array(target), np.array(cls), (("crossing", 0.10), ("in the plane", 0.0)))


@functools.lru_cache(maxsize=None)
def case_range():
    """(e) tmin and tmax at RINGS t-bands round the hit distance (closest rays; tmax alone for shadow rays, which keep tmin = 0), in a
    small soup where another triangle may lie behind the one that leaves the range"""
    rng = np.random.default_rng(51)
    verts = random_triangles(rng, 48, lo=1.0, hi=4.0, extent=3.0)
    vd = verts.astype(D)
    ray, target, cls = [], [], []
    while len(ray) < 160 * 2 * len(RINGS):
        k = int(rng.integers(48))
        a, b, c = vd[k]
        if k % 16 == 5:
            continue
        bu, bv = rng.uniform(0.15, 0.4), rng.uniform(0.15, 0.4)
        p = a + bu * (b - a) + bv * (c - a)
        w = rng.normal(size=3); w /= np.linalg.norm(w)
        base = _aim(p + w * rng.uniform(2.0, 12.0), p, rng)
        P = pairs(verts[k, 0], verts[k, 1], verts[k, 2], base[:3], base[3:6])
        if not bool(P.hit):
            continue
        for ring in RINGS:
            edge = F(float(P.t) - ring * float(P.bt))          # + ring: the hit is inside the range by `ring` bands
            lo_ray, hi_ray = base.copy(), base.copy()
            lo_ray[6] = edge
            hi_ray[7] = F(float(P.t) + ring * float(P.bt))
            ray += [lo_ray, hi_ray]; target += [k, k]; cls += [0, 1]
    return Case("ranges", verts, np.array(ray, F), np.array(target), np.array(cls), (("tmin", 0.25), ("tmax", 0.25)))


def scene_of(verts):
    """the triangles as a scene that scenes.load_scene and the oracle accept: one diffuse material, no lights"""
    verts = np.ascontiguousarray(verts, F).reshape(-1, 3, 3)
    cam = {"type": "perspective", "from": (0.0, -5.0, 1.0), "to": (0.0, 0.0, 0.0), "up": (0.0, -5.0, 2.0), "resx": 8, "resy": 8, "focal": 1.0}
    return {"verts": verts, "tri_mat": np.zeros(len(verts), np.int32), "vnormals": None,
            "materials": [{"type": "shinydiffusemat", "color": (0.7, 0.7, 0.7), "diffuse_reflect": 1.0}], "lights": [], "camera": cam}


CASE_NAMES = ("soup", "single 0", "single 1", "fan and strip", "plane 0", "plane 1", "plane 2", "ranges")


@functools.lru_cache(maxsize=None)
def all_cases():
    """the cases (a) to (e), made on first use"""
    cases = [case_soup(), case_single(0), case_single(1), case_fan_strip(), case_plane(0), case_plane(1), case_plane(2), case_range()]
    assert tuple(c.name for c in cases) == CASE_NAMES
    return cases


@functools.lru_cache(maxsize=None)
def decided(case_index):
    """the float64 verdicts of a case's rays (shared by every test of the process)"""
    c = all_cases()[case_index]
    return rays(c.verts, c.rays)


@functools.lru_cache(maxsize=None)
def decided_pairs(case_index):
    """the float64 test of every ray of a case against the triangle it was placed at"""
    c = all_cases()[case_index]
    v = c.verts[c.target]
    return pairs(v[:, 0], v[:, 1], v[:, 2], c.rays[:, :3], c.rays[:, 3:6])


# ---- the surface scene -----------------------------------------------------------------------------------------------
BARYCENTRICS = [(0, 0), (1, 0), (0, 1), (0.5, 0), (0, 0.5), (0.5, 0.5), (0.3, 0.7), (0.25, 0.75)]
OPPOSED, ALONG_Z_UP, ALONG_Z_DOWN = 3, 4, 5           # triangles of the smooth mesh
SAME_UV, THIN_UV = 24 + 2, 24 + 3                     # triangles of the mapped mesh
FLAT_UP, FLAT_DOWN = 48 + 1, 48 + 2                   # triangles of the plain mesh, in the plane z = 0.5


@functools.lru_cache(maxsize=None)
def surface_scene():
    """three meshes, triangles [0, 24) smooth with per-corner normals (some corners without one), [24, 48) with UVs and orco under
    material 1, [48, 64) with neither under material 2; per triangle corner arrays, zeros where a mesh has none"""
    rng = np.random.default_rng(61)
    T = 64
    verts = random_triangles(rng, T, lo=0.5, hi=2.0, extent=4.0)
    for k in range(T):      # well-shaped ones: the needles and the far ones belong to the triangle test's inputs
        if k % 3 == 1 or k % 12 == 2 or k % 16 == 5:
            a = rng.uniform(-4, 4, 3)
            verts[k] = (a + np.array([[0, 0, 0], rng.uniform(0.5, 1.5, 3) * [1, 0.2, -0.3], rng.uniform(0.5, 1.5, 3) * [-0.2, 1, 0.4]])).astype(F)
    for k, flip in ((FLAT_UP, False), (FLAT_DOWN, True)):
        pts = np.array([[0.25, 0.5, 0.5], [1.75, 0.75, 0.5], [0.5, 2.0, 0.5]]) + [3.0 * flip, 0, 0]
        verts[k] = (pts[::-1] if flip else pts).astype(F)
    vd = verts.astype(D)
    vn = np.zeros((T, 3, 3), F)
    for k in range(24):
        ng = _tri_frame(*vd[k])[2]
        for cnr in range(3):
            if (k + cnr) % 5 == 0 and k > 5:
                continue                                           # a corner without a normal
            nrm = ng + 0.5 * rng.normal(size=3)
            vn[k, cnr] = (nrm / np.linalg.norm(nrm) * rng.uniform(0.5, 2.0)).astype(F)
    vn[OPPOSED, 2] = -vn[OPPOSED, 1]
    vn[ALONG_Z_UP], vn[ALONG_Z_DOWN] = F([0, 0, 1]), F([0, 0, -1])
    uv, orco = np.zeros((T, 3, 2), F), np.zeros((T, 3, 3), F)
    uv[24:48] = rng.uniform(-1.0, 2.0, (24, 3, 2)).astype(F)
    uv[SAME_UV] = uv[SAME_UV, 0]
    uv[THIN_UV, 2] = (0.5 * (uv[THIN_UV, 0].astype(D) + uv[THIN_UV, 1].astype(D))).astype(F)       # collinear up to the rounding: excluded by band
    orco[24:48] = rng.uniform(-1.0, 1.0, (24, 3, 3)).astype(F)
    idx = np.arange(T)
    sc = dict(verts=verts, vn=vn, uv=uv, orco=orco, mesh_smooth=idx < 24, has_uv=(idx >= 24) & (idx < 48), has_orco=(idx >= 24) & (idx < 48),
              mat=np.where(idx < 24, 0, np.where(idx < 48, 1, 2)).astype(np.int64), meshes=((0, 24), (24, 48), (48, 64)))
    # the items: every triangle at every barycentric and at four interior points
    tri, bu, bv = [], [], []
    for k in range(T):
        pts = BARYCENTRICS + [tuple(x) for x in rng.dirichlet([1, 1, 1], 4)[:, 1:]]
        tri += [k] * len(pts); bu += [q[0] for q in pts]; bv += [q[1] for q in pts]
    tri, bu, bv = np.array(tri), np.array(bu, F), np.array(bv, F)
    p = (vd[tri, 0] + bu.astype(D)[:, None] * (vd[tri, 1] - vd[tri, 0]) + bv.astype(D)[:, None] * (vd[tri, 2] - vd[tri, 0])).astype(F)
    return sc, (tri, bu, bv, p)


def surface_errors(got, val, band, exact):
    """per field: (items held, items excluded by band, worst error / (U * conditioning), items outside the band or, in an exact case,
    not equal)"""
    out = {}
    for f in SURFACE_FIELDS:
        g, w = np.asarray(got[f], D), val[f]
        err = np.abs(g - w).max(axis=-1)
        bnd = np.asarray(band[f], D)
        ex = exact.get(f, np.zeros(len(err), bool))
        usable = np.isfinite(bnd) & (bnd < 1e-2)
        held = usable | ex
        with np.errstate(all="ignore"):
            ratio = np.where(usable & ~ex & (bnd > 0), err / (bnd / K), 0.0)
        bad = np.nonzero((ex & (err != 0)) | (usable & ~ex & (err > bnd)))[0]
        out[f] = (int(held.sum()), int((~held).sum()), float(ratio.max()), bad)
    return out
