"""Shared by the tests of the directional, sun and sphere lights: the reader of tests/golden/ref_lights_{ieee,fast}.json.gz — what the reference's own DirectionalLight, SunLight and SphereLight (compiled
where they lie by oracle/Makefile, driver oracle/ref_harness/ref_lights.cc) gave on seeded inputs.  Every light was made by its
factory() from the ParamMap stored with it; a refused call's outputs are zeros —, and a scene with one light of each of the five types."""
import functools
import gzip
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

# leaf function -> (types that have it, input columns, output columns: ok first)
LEAVES = {"illuminate": ("directionallight", 3, 8), "illum_sample": ("sunlight spherelight", None, 9), "intersect": ("sunlight", 3, 6)}


@functools.lru_cache(maxsize=None)
def load(variant):
    with gzip.open(os.path.join(HERE, "golden", f"ref_lights_{variant}.json.gz"), "rt") as f:
        return json.load(f)


def u2f(a):
    return np.asarray(a, dtype=np.uint32).view(np.float32)


def light(doc, name):
    """the set's parameters in the dict form libyafaray_amd.scenes.load_scene and oracle.pyoracle.light_desc take"""
    p = dict(doc[name + "_params"])
    for k in ("direction", "from", "color"):
        if k in p:
            p[k] = tuple(float(np.float32(v)) for v in p[k])
    return p


def sets(doc, light_type=None):
    return [n for n in doc["sets"] if light_type is None or doc[n + "_params"]["type"] == light_type]


def leaf(doc, name, fn):
    """-> inputs (n, k) float32, outputs (n, m) as uint32 bit patterns (column 0: 1.0f or 0.0f, whether the call was taken)"""
    key_in = next(k for k in doc if k.startswith(f"{name}_{fn}_in"))
    key_out = next(k for k in doc if k.startswith(f"{name}_{fn}_out"))
    n_in, n_out = int(key_in.rsplit("_in", 1)[1]), int(key_out.rsplit("_out", 1)[1])
    return u2f(doc[key_in]).reshape(-1, n_in), np.asarray(doc[key_out], dtype=np.uint32).reshape(-1, n_out)


def five_light_scene(n_tris=800, seed=41, res=(48, 40)):
    """scenes.cornell_soup with its lights replaced by one of each of the five types, all inside the soup's room: the area light under the
    ceiling (on its emissive quad), a point light, a finite directional light whose cylinder comes down on part of the room, a sun that
    shines in through the open front, a sphere light"""
    from libyafaray_amd import scenes
    sc = scenes.cornell_soup(n_tris, seed=seed, res=res)
    sc["lights"] = [dict(sc["lights"][0], samples=2),
                    {"type": "pointlight", "from": (0.5, -0.4, 0.3), "color": (1.0, 0.9, 0.7), "power": 1.5},
                    {"type": "directionallight", "direction": (0.1, -0.15, 1.0), "color": (0.9, 1.0, 0.8), "power": 1.2, "infinite": False,
                     "from": (-0.3, -0.2, 0.9), "radius": 0.6},
                    {"type": "sunlight", "direction": (0.2, -0.9, 0.4), "color": (1.0, 0.9, 0.75), "power": 1.5, "angle": 5.0, "samples": 2},
                    {"type": "spherelight", "from": (0.3, -0.3, 0.3), "radius": 0.1, "color": (1.0, 0.9, 0.8), "power": 8.0, "samples": 3}]
    return sc
