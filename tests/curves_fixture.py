"""A restatement of Scene::endCurveMesh (scene.cc:154-281) for the curve tests: what a strand's points, radii and shape become.

Float32 throughout, one rounding per operation in the order the reference's expressions give; doubles where the source has them:
the radius (C's double pow, a double sum narrowed to `float r`), the two extrusion scales (double products narrowed by
operator*(float, Vec3)) and the second texture coordinate of a segment (su + 1. / (n - 1)).  math.pow and math.sqrt are the C library's
double functions; numpy's power is not used, its SIMD variants need not agree with libm bit for bit."""
import math

import numpy as np

F = np.float32


def scales(n, strand_start, strand_end, strand_shape):
    """(h, s) per point, float32 (n,): h = (float)(0.5 * r), s = (float)(1.5 * r / sqrt(3.f)), r the radius of scene.cc:172-179"""
    start, end, shape = F(strand_start), F(strand_end), F(strand_shape)
    diff = float(F(end - start))
    h, s = np.zeros(n, F), np.zeros(n, F)
    for i in range(n):
        if shape < 0:
            r = float(start) + math.pow(float(F(F(i) / F(n - 1))), float(F(F(1) + shape))) * diff
        else:
            r = float(start) + (1 - math.pow(float(F(F(n - i - 1) / F(n - 1))), float(F(F(1) - shape)))) * diff
        r = F(r)
        h[i] = F(0.5 * float(r))
        s[i] = F(1.5 * float(r) / math.sqrt(float(F(3))))
    return h, s


def sq3(v):
    return (v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def normalize(v):
    """Vec3::normalize, vector.h:249-260"""
    l = sq3(v)
    with np.errstate(divide="ignore", invalid="ignore"):
        scaled = v * (F(1.0) / np.sqrt(l))[..., None]
    return np.where((l != 0)[..., None], scaled, v)


def create_cs(n):
    """createCs__, vector.h:319-337, on (k, 3) float32"""
    n = np.asarray(n, F)
    z_branch = (n[:, 0] == 0) & (n[:, 1] == 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        d = F(1.0) / np.sqrt(n[:, 1] * n[:, 1] + n[:, 0] * n[:, 0])
        u = np.stack([n[:, 1] * d, -n[:, 0] * d, np.zeros(len(n), F)], -1)
        v = cross(n, u)
    uz = np.stack([np.where(n[:, 2] < 0, F(-1), F(1)), np.zeros(len(n), F), np.zeros(len(n), F)], -1)
    vz = np.tile(np.array([0, 1, 0], F), (len(n), 1))
    return np.where(z_branch[:, None], uz, u).astype(F), np.where(z_branch[:, None], vz, v).astype(F)


def extrude(points, h, s):
    """(o, a, b), (n, 3) float32 each: a = o - h * v - s * u, b = o - h * v + s * u in the frame of the tangent to the next point; the last
    point keeps the frame of the one before it (scene.cc:169-193)"""
    o = np.ascontiguousarray(points, F).reshape(-1, 3)
    n = len(o)
    at = np.minimum(np.arange(n), n - 2)
    u, v = create_cs(normalize(o[at + 1] - o[at]))
    m = o - h[:, None] * v
    su = s[:, None] * u
    return o, (m - su).astype(F), (m + su).astype(F)


def triangles(points, strand_start, strand_end, strand_shape):
    """the strand's 6 * (n - 1) + 2 triangles in the reference's order: corner vertices (t, 3, 3) and UVs (t, 3, 2), float32"""
    pts = np.ascontiguousarray(points, F).reshape(-1, 3)
    n = len(pts)
    h, s = scales(n, strand_start, strand_end, strand_shape)
    o, a, b = extrude(pts, h, s)
    verts, uv = [(o[0], b[0], a[0])], [(F(0), F(0), F(0))]                # close bottom: Triangle(a_1, a_3, a_2), iu of segment 0
    su = sv = F(0)
    for j in range(n - 1):
        su = F(F(j) / F(n - 1))
        sv = F(float(su) + 1.0 / (n - 1))
        k = j + 1
        verts += [(o[j], a[k], o[k]), (o[j], a[j], a[k]), (a[j], b[k], a[k]), (a[j], b[j], b[k]), (b[k], b[j], o[j]), (b[k], o[j], o[k])]
        uv += [(su, sv, sv), (su, su, sv), (su, sv, sv), (su, su, sv), (sv, su, su), (sv, su, sv)]
    verts.append((o[n - 1], a[n - 1], b[n - 1]))                          # close top, with the last segment's iv
    uv.append((sv, sv, sv))
    uv = np.array(uv, F)
    return np.array(verts, F), np.stack([uv, uv], -1)


def strand(n, seed, length=1.0, origin=(0.0, 0.0, 0.0)):
    """a wavy strand of n points growing from `origin`"""
    rng = np.random.default_rng(seed)
    step = rng.normal(size=(n - 1, 3)) * 0.3 + np.array([0.2, 0.1, 1.0])
    p = np.concatenate([np.zeros((1, 3)), np.cumsum(step, 0)]) * (length / max(n - 1, 1))
    return (p + np.asarray(origin)).astype(F)
