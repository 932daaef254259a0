"""Shared by the tests of the short traversal stack and its kd-restart (test_short_stack_host.py, test_gpu_short_stack.py).

The three tree walks of the device (wf_trace<closest>, wf_trace<any>, kd_trace_ts) keep a short ring of pending far children
per lane instead of the reference's 64-entry stack, and restart at the root when an entry was overwritten.  Ordinary scenes
hardly go there; the inputs here do: a jittered sheet of small triangles in one plane, and rays that graze it diagonally, so
that a ray crosses a split plane of every level of the tree over and over and its list of pending far children runs deep.

model_walk is a float64 restatement of the device's walk.  Its only job is to CERTIFY that an input reaches the restart path
(how deep the pending list gets, how often a ring of a given size restarts).  It is not a reference: no device answer is ever
compared with it.  The references of the GPU tests are the oracle's brute force and the oracle's own walk with the
reference's 64-entry stack."""
import numpy as np

RING_TRACE = 7      # live entries of wf_trace's ring (kStack - 1: the slot above the top is written unconditionally)
RING_TS = 8         # live entries of kd_trace_ts's ring (kStack)
RAY_TMIN = 5e-5
X_END = 1.3         # the rays run from x = -X_END to x = +X_END


def sheet_verts(g, seed):
    """the g x g jittered sheet in the plane z = 0 over [-1, 1]^2 as (g * g, 9) float32: one small triangle per cell, cell centres on
    the grid, every vertex offset ~ N(0, (0.3 / g)^2) per coordinate (so nothing lies exactly in a plane, on a line or at a tie)"""
    rng = np.random.default_rng(seed)
    c = (np.arange(g) + 0.5) * (2.0 / g) - 1.0
    cx, cy = np.meshgrid(c, c, indexing="ij")
    centres = np.stack([cx, cy, np.zeros((g, g))], axis=-1).reshape(-1, 1, 3)
    return (centres + rng.normal(0.0, 0.3 / g, size=(g * g, 3, 3))).astype(np.float32).reshape(-1, 9)


def _scene(verts, tri_mat, materials, lights, camera):
    return {"verts": np.ascontiguousarray(verts, np.float32).reshape(-1, 3, 3), "tri_mat": np.asarray(tri_mat, np.int32), "vnormals": None,
            "materials": materials, "lights": lights, "camera": camera}


WHITE = {"type": "shinydiffusemat", "color": (0.7, 0.7, 0.7), "diffuse_reflect": 1.0}


def sheet(g, seed):
    """-> (verts (g * g, 9) float32, a scene scenes.load_scene accepts: the sheet alone, diffuse, under a point light; the scene of
    the ray batches, whose tree is the tree of the sheet)"""
    verts = sheet_verts(g, seed)
    cam = {"type": "perspective", "from": (0.0, -2.5, 1.5), "to": (0.0, 0.0, 0.0), "up": (0.0, -2.5, 2.5), "resx": 32, "resy": 32, "focal": 1.4}
    lights = [{"type": "pointlight", "from": (0.3, -0.2, 1.5), "color": (1.0, 1.0, 1.0), "power": 10.0}]
    return verts, _scene(verts, np.zeros(len(verts), np.int32), [dict(WHITE)], lights, cam)


def _quad(a, b, c, d):
    return np.array([[a, b, c], [a, c, d]], np.float32).reshape(2, 9)


LIGHT_POS = (-X_END, -1.2, 0.01)
RECEIVER = {"x": (1.05, X_END), "y": (0.5, 1.3), "z": (-0.02, 0.02)}      # a ramp beyond the sheet's far edge, rising by 0.04 over 0.25 in x


def shadow_scene(g, seed, opaque_half=False, res=(48, 14)):
    """the sheet, transparent (its transmit filter < 1, so every triangle a shadow ray passes shows in the filter product), an
    opaque receiver beyond its far edge — a quad that rises from z = -0.02 at x = 1.05 to z = +0.02 at x = 1.3 — and a point light
    at the other end, just above the sheet's plane: the receiver's shadow rays graze the sheet from end to end.  The camera looks
    down on the receiver and sees nothing else.  opaque_half: every other triangle of the sheet is opaque, so that rays are
    blocked on their way as well."""
    verts = sheet_verts(g, seed)
    (x0, x1), (y0, y1), (z0, z1) = RECEIVER["x"], RECEIVER["y"], RECEIVER["z"]
    quad = _quad((x0, y0, z0), (x1, y0, z1), (x1, y1, z1), (x0, y1, z0))      # its normal points up and a little toward the light
    tri_mat = np.zeros(len(verts) + 2, np.int32)
    tri_mat[-2:] = 1
    if opaque_half:
        tri_mat[1:len(verts):2] = 2
    materials = [{"type": "shinydiffusemat", "color": (0.9, 0.6, 0.3), "diffuse_reflect": 0.5, "transparency": 0.8, "transmit_filter": 0.7},
                 dict(WHITE), {"type": "shinydiffusemat", "color": (0.2, 0.3, 0.8), "diffuse_reflect": 1.0}]
    lights = [{"type": "pointlight", "from": LIGHT_POS, "color": (1.0, 1.0, 1.0), "power": 200.0}]
    # straight down from z = 2, the picture's width along y: 0.71 x 0.21 of the receiver's 0.8 x 0.25
    cx, cy = 0.5 * (x0 + x1), 0.5 * (y0 + y1)
    cam = {"type": "perspective", "from": (cx, cy, 2.0), "to": (cx, cy, 0.0), "up": (cx + 1.0, cy, 2.0), "resx": res[0], "resy": res[1], "focal": 2.8}
    return _scene(np.concatenate([verts, quad]), tri_mat, materials, lights, cam)


def receiver_rays(n, seed):
    """(n, 8) rays from points of the receiver to the light of shadow_scene, as the direct-lighting estimate sends them (unbounded here:
    the certificate is for rays that pass everything)"""
    rng = np.random.default_rng(seed)
    (x0, x1), (z0, z1) = RECEIVER["x"], RECEIVER["z"]
    u = rng.uniform(0.0, 1.0, size=n)
    p = np.stack([x0 + u * (x1 - x0), rng.uniform(*RECEIVER["y"], size=n), z0 + u * (z1 - z0)], axis=1)
    d = np.asarray(LIGHT_POS)[None] - p
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([p, d, np.full((n, 1), RAY_TMIN), np.full((n, 1), -1.0)], axis=1).astype(np.float32)


def lit_scene(g, seed, res=(48, 48)):
    """the sheet, diffuse, under a Cornell-style quad light on emissive geometry, seen from a low camera with a narrow view along it:
    every camera ray grazes the sheet, and so do many of the bounces off its triangles"""
    verts = sheet_verts(g, seed)
    x0, y0, x1, y1, z = -0.25, -0.25, 0.25, 0.25, 0.6
    quad = _quad((x0, y0, z), (x0, y1, z), (x1, y1, z), (x1, y0, z))
    tri_mat = np.zeros(len(verts) + 2, np.int32)
    tri_mat[-2:] = 1
    materials = [dict(WHITE), {"type": "light_mat", "color": (1.0, 1.0, 1.0), "power": 15.0}]
    lights = [{"type": "arealight", "corner": (x0, y0, z), "point1": (x0, y1, z), "point2": (x1, y0, z), "color": (1.0, 1.0, 1.0), "power": 15.0, "samples": 1}]
    cam = {"type": "perspective", "from": (-1.6, -1.2, 0.03), "to": (0.6, 0.5, -0.03), "up": (-1.6, -1.2, 1.03), "resx": res[0], "resy": res[1], "focal": 10.0}
    return _scene(np.concatenate([verts, quad]), tri_mat, materials, lights, cam)


def grazing_rays(n, seed, bounded_every=5):
    """(n, 8) float32 rays (origin, direction, tmin, tmax; tmax -1: unbounded) that graze the sheet diagonally: from x = -1.3 to
    x = +1.3, y from [-1.3, -0.5] to [0.5, 1.3], |z| <= 0.02 at both ends.  Every bounded_every-th ray is bounded, its tmax drawn so
    that it ends inside the sheet's extent.  All coordinates are drawn from continuous distributions: no ray is aimed at a vertex,
    an edge or a split plane."""
    rng = np.random.default_rng(seed)
    a = np.stack([np.full(n, -X_END), rng.uniform(-1.3, -0.5, n), rng.uniform(-0.02, 0.02, n)], axis=1)
    b = np.stack([np.full(n, X_END), rng.uniform(0.5, 1.3, n), rng.uniform(-0.02, 0.02, n)], axis=1)
    length = np.linalg.norm(b - a, axis=1, keepdims=True)
    d = (b - a) / length
    rays = np.concatenate([a, d, np.full((n, 1), RAY_TMIN), np.full((n, 1), -1.0)], axis=1)
    # inside the sheet's extent: |x| <= 1 and |y| <= 1 (the ray rises in x and in y)
    t_in = np.maximum((-1.0 - a[:, 0]) / d[:, 0], (-1.0 - a[:, 1]) / d[:, 1])
    t_out = np.minimum((1.0 - a[:, 0]) / d[:, 0], (1.0 - a[:, 1]) / d[:, 1])
    u = rng.uniform(0.1, 0.9, n)
    sel = np.arange(n) % bounded_every == 0
    rays[sel, 7] = (t_in + u * (t_out - t_in))[sel]
    return rays.astype(np.float32)


def brute_hits(verts, rays):
    """float64 brute force over (n, 9) triangles, Moeller-Trumbore as Triangle::intersect has it: -> (tri (n,) int, -1: none; t (n,)
    float64, inf: none) — the closest hit with tmin <= t < tmax of every ray"""
    v = np.asarray(verts, np.float64).reshape(-1, 3, 3)
    a, e1, e2 = v[:, 0], v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
    tri, ts = np.full(len(rays), -1, np.int64), np.full(len(rays), np.inf)
    for i, r in enumerate(np.asarray(rays, np.float64)):
        o, d = r[:3], r[3:6]
        pvec = np.cross(d, e2)
        det = np.einsum("ij,ij->i", e1, pvec)
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = 1.0 / det
            tvec = o - a
            u = np.einsum("ij,ij->i", tvec, pvec) * inv
            qvec = np.cross(tvec, e1)
            w = np.einsum("ij,ij->i", qvec, d[None]) * inv
            t = np.einsum("ij,ij->i", e2, qvec) * inv
        ok = (det != 0) & (u >= 0) & (u <= 1) & (w >= 0) & (u + w <= 1) & (t >= r[6]) & ((r[7] < 0) | (t < r[7]))
        if ok.any():
            t = np.where(ok, t, np.inf)
            tri[i] = int(np.argmin(t)); ts[i] = t[tri[i]]
    return tri, ts


class FlatTree:
    """the flattened tree of interface.build_kdtree as Python lists (the model walks node by node: numpy scalars would cost 10x)"""

    def __init__(self, nodes, bound):
        nodes = np.ascontiguousarray(nodes, np.uint32).reshape(-1, 2)
        flags = nodes[:, 1]
        self.kind = (flags & 3).tolist()                      # 0..2: split axis, 3: leaf
        self.arg = (flags >> 2).tolist()                      # interior: right child (left is node + 1); leaf: reference count
        self.split = nodes[:, 0].copy().view(np.float32).astype(np.float64).tolist()
        self.first = nodes[:, 0].tolist()                     # leaf: first reference
        self.lo = [float(x) for x in bound[:3]]
        self.hi = [float(x) for x in bound[3:]]


def _walk(tree, o, d, z_end, ring):
    """one walk, with a ring of `ring` live entries (None: unbounded) -> (largest pending list, restarts, leaves visited, restart
    positions: indices into the leaf list)"""
    inv = [1.0 / x if x != 0.0 else float("inf") for x in d]
    enter, leave = -float("inf"), float("inf")
    for k in range(3):                                        # Bound::cross: the slabs
        if d[k] != 0.0:
            t0, t1 = (tree.lo[k] - o[k]) * inv[k], (tree.hi[k] - o[k]) * inv[k]
            enter, leave = max(enter, min(t0, t1)), min(leave, max(t0, t1))
    if not (enter <= leave and leave >= 0.0 and enter <= z_end):
        return 0, 0, [], []
    t_exit, tmin, tmax = leave, max(enter, 0.0), leave
    node, pending, lost, deepest, restarts, leaves, at = 0, [], False, 0, 0, [], []
    kind, arg, split = tree.kind, tree.arg, tree.split
    while True:
        if z_end < tmin:
            break
        while kind[node] != 3:
            # the node step's three cases: the near child alone, the far child alone, or both (the far child is noted)
            k = kind[node]
            tplane = (split[node] - o[k]) * inv[k]
            below = o[k] < split[node] or (o[k] == split[node] and d[k] <= 0.0)
            near, far = (node + 1, arg[node]) if below else (arg[node], node + 1)
            if not (tplane <= tmax) or tplane <= 0.0:
                node = near
            elif tplane < tmin:
                node = far
            else:
                pending.append((far, tmax))
                if ring is not None and len(pending) > ring:
                    del pending[0]                            # the ring drops its oldest entry: the farthest pending child
                    lost = True
                deepest = max(deepest, len(pending))
                node, tmax = near, tplane
        leaves.append(node)
        # the end of a leaf: a hit inside its cell ends the ray, else the nearest pending child, a restart, or the end
        if z_end <= tmax:
            break
        if pending:
            tmin = tmax
            node, tmax = pending.pop()
        elif lost and not (tmax >= t_exit):
            tmin = tmax if tmax > tmin else tmax + max(abs(tmax) * 1.2e-7, 1e-30)
            tmax, node, lost = t_exit, 0, False
            restarts += 1
            at.append(len(leaves))
        else:
            break
    return deepest, restarts, leaves, at


def model_walk(nodes, bound, o, d, z_end, ring):
    """The device's t-based walk restated in float64 over the flattened tree (nodes, bound) of interface.build_kdtree (or a FlatTree
    of them, to convert once for many rays), for the ray (o, d) that ends at distance z_end — its closest hit, its tmax, or inf for a
    ray that passes everything —, with a ring of `ring` live entries (None: unbounded).
    -> (the largest pending list an unbounded stack would have held, the restarts with the given ring, the leaves visited: node indices
    in visiting order, empty leaves included, re-visits after a restart included).
    A certificate for inputs, NOT a reference for answers: see the module's docstring."""
    tree = nodes if isinstance(nodes, FlatTree) else FlatTree(nodes, bound)
    o, d = [float(x) for x in o], [float(x) for x in d]
    deepest = _walk(tree, o, d, z_end, None)[0]
    _, restarts, leaves, _ = _walk(tree, o, d, z_end, ring)
    return deepest, restarts, leaves


def describe_walk(nodes, bound, o, d, z_end, ring):
    """a failing ray for the eye: its leaf sequence (node:count) with the restarts marked"""
    tree = nodes if isinstance(nodes, FlatTree) else FlatTree(nodes, bound)
    deepest, restarts, leaves, at = _walk(tree, [float(x) for x in o], [float(x) for x in d], z_end, ring)
    out = []
    for i, n in enumerate(leaves):
        if i in at:
            out.append("| restart |")
        out.append(f"{n}:{tree.arg[n]}")
    return f"ring {ring}: deepest {deepest}, {restarts} restarts, leaves " + " ".join(out)


def restart_counts(nodes, bound, rays, z_end, ring):
    """restarts of every ray of a batch (z_end: per ray) -> int array"""
    tree = FlatTree(nodes, bound)
    return np.array([model_walk(tree, None, r[:3], r[3:6], float(z), ring)[1] for r, z in zip(np.asarray(rays, np.float64), z_end)])


def ends(rays, hit_t=None):
    """z_end of every ray: its closest hit (hit_t, inf where none) if given, cut at a bounded ray's tmax"""
    z = np.full(len(rays), np.inf) if hit_t is None else np.asarray(hit_t, np.float64).copy()
    tmax = np.asarray(rays, np.float64)[:, 7]
    return np.where(tmax >= 0, np.minimum(z, tmax), z)
