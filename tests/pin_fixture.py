"""Shared by the tests of the spot light, the IES light and the architect / angular / equirectangular cameras: the reader of
tests/golden/ref_spot_ies_{ieee,fast}.json.gz and tests/golden/ref_cameras_{ieee,fast}.json.gz — what the reference's own SpotLight, IesLight,
IesData and the three camera classes (compiled where they lie by oracle/Makefile, drivers oracle/ref_harness/ref_spot_ies.cc and
ref_cameras.cc) gave.  Every object was made by its factory() from the ParamMap stored with it; a refused call's outputs are zeros; an IES
row whose lookup the reference takes at or beyond the last entry of an angle map (it reads past its array there) carries a mark and no value."""
import functools
import gzip
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
POINT_KEYS = ("direction", "from", "to", "up", "color")


@functools.lru_cache(maxsize=None)
def load(kind, variant):
    """kind: "spot_ies" or "cameras"; variant: "ieee" or "fast" """
    with gzip.open(os.path.join(HERE, "golden", f"ref_{kind}_{variant}.json.gz"), "rt") as f:
        return json.load(f)


def u2f(a):
    return np.asarray(a, dtype=np.uint32).view(np.float32)


def params(doc, name, ies_dir=None):
    """the set's parameters in the dict form libyafaray_amd.scenes.load_scene and Interface.paramsSet take; an IES light's file name is
    joined to `ies_dir` (where tests/ies_fixture.write put the file)"""
    p = dict(doc[name + "_params"])
    for k in POINT_KEYS:
        if k in p:
            p[k] = tuple(float(np.float32(v)) for v in p[k])
    if "file" in p and ies_dir is not None:
        p["file"] = os.path.join(str(ies_dir), p["file"])
    return p


def leaf(doc, name, fn):
    """-> inputs (n, k) float32, outputs (n, m) as uint32 bit patterns, keep (n,) bool: the rows that carry a value (all, where the leaf has
    no mark)"""
    key_in = next(k for k in doc if k.startswith(f"{name}_{fn}_in"))
    key_out = next(k for k in doc if k.startswith(f"{name}_{fn}_out"))
    n_in, n_out = int(key_in.rsplit("_in", 1)[1]), int(key_out.rsplit("_out", 1)[1])
    inp, out = u2f(doc[key_in]).reshape(-1, n_in), np.asarray(doc[key_out], dtype=np.uint32).reshape(-1, n_out)
    mark = doc.get(f"{name}_{fn}_mark")
    keep = np.ones(len(inp), bool) if mark is None else ~np.asarray(mark, bool)
    assert len(inp) == len(out) == len(keep)
    return inp, out, keep


def same(got, want, what, keep=None):
    """bit for bit, +0 / -0 not distinguished, on the rows of `keep`"""
    got = np.ascontiguousarray(got, dtype=np.float32).view(np.uint32).reshape(want.shape)
    bad = (got != want) & ~(((got | want) & 0x7fffffff) == 0)
    if keep is not None:
        bad &= keep[:, None]
    assert not bad.any(), f"{what}: {bad.sum()} of {bad.size} words differ, first row {np.nonzero(bad.any(axis=1))[0][0]}: " \
                          f"{got[bad.any(axis=1)][0].view(np.float32)} vs {want[bad.any(axis=1)][0].view(np.float32)}"
