"""Spot lights on the host: createLight's "spotlight" (SpotLight::factory and constructor, light_spot.cc:258-296, :29-42) against the float32
restatement of tests/spot_fixture.py, word for word; the acceptance rule (a spotlight needs both `from` and `to`), every refusal by its
parameter's name, disabled lights, the light order and the XML loader.  No GPU needed.

Every test here fails without the feature: createLight refused every spotlight."""
import os
import subprocess

import numpy as np
import pytest

from libyafaray_amd import Interface, interface
from tests import spot_fixture as spf
from tests.test_lights_host import bits, color, light_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AIM = {"from": (0.25, -0.5, 2.0), "to": (0.75, 0.25, 0.0)}
PHRASE = "spotlight with the from and to it aims along"


def spot(**kw):
    return light_of(dict({"type": "spotlight"}, **kw))


# ---- acceptance ---------------------------------------------------------------------------------------------------------
def test_spotlight_with_from_and_to_is_accepted():
    yi, h = spot(**AIM)
    assert h, yi.getLastError()
    rec = yi.getLights()
    assert rec.shape[0] == 1 and int(rec[0, :1].view(np.int32)[0]) == spf.TYPE_SPOT


@pytest.mark.parametrize("params", [{}, {"from": AIM["from"]}, {"to": AIM["to"]}], ids=["bare", "only_from", "only_to"])
def test_spotlight_without_from_or_to_is_refused(params):
    yi, h = spot(**params)
    msg = yi.getLastError()
    assert not h and "scope" in msg and "sunlight" in msg and PHRASE in msg, msg
    assert yi.getLights().shape[0] == 0


@pytest.mark.parametrize("params, needle", [
    ({"to": AIM["from"]}, "from and to"),
    ({"cone_angle": 0.0}, "cone_angle"), ({"cone_angle": -10.0}, "cone_angle"), ({"cone_angle": 180.5}, "cone_angle"),
    ({"cone_angle": float("nan")}, "cone_angle"), ({"cone_angle": float("inf")}, "cone_angle"),
    ({"blend": -0.01}, "blend"), ({"blend": 1.01}, "blend"), ({"blend": float("nan")}, "blend"),
    ({"soft_shadows": True, "samples": 0}, "samples"), ({"soft_shadows": True, "samples": -3}, "samples"),
    ({"photon_only": True}, "photon_only"),
])
def test_refusals_name_their_parameter(params, needle):
    yi, h = spot(**dict(AIM, **params))
    assert not h and needle in yi.getLastError(), (params, yi.getLastError())
    assert yi.getLights().shape[0] == 0


def test_samples_below_one_do_not_matter_to_a_dirac_spot():
    yi, h = spot(**dict(AIM, samples=0))
    assert h, yi.getLastError()
    assert [int(x) for x in yi.getLights()[0, :2].view(np.int32)] == [spf.TYPE_SPOT, 1]


# ---- the record ---------------------------------------------------------------------------------------------------------
AXES = {"+x": ((1.0, 2.0, 3.0), (2.0, 2.0, 3.0)), "-x": ((1.0, 2.0, 3.0), (-2.5, 2.0, 3.0)), "+y": ((0.0, 0.0, 0.0), (0.0, 4.0, 0.0)),
        "-y": ((0.5, 0.5, 0.5), (0.5, -1.0, 0.5)), "+z": ((0.0, 0.0, -1.0), (0.0, 0.0, 2.0)), "-z": ((0.0, 0.0, 3.0), (0.0, 0.0, 0.0)),
        "skew": (AIM["from"], AIM["to"])}


@pytest.mark.parametrize("soft", [False, True], ids=["dirac", "soft"])
@pytest.mark.parametrize("axis", sorted(AXES))
def test_record_word_for_word(axis, soft):
    frm, to = AXES[axis]
    col, power = (0.9, 0.7, 0.3), 2.5
    for angle in (5.0, 45.0, 90.0, 120.0, 180.0):
        for blend in (0.0, 0.15, 0.5, 1.0):
            yi, h = spot(**{"from": frm, "to": to, "color": color(*col), "power": power, "cone_angle": angle, "blend": blend,
                            "soft_shadows": soft, "samples": 5, "shadowFuzzyness": 0.75})
            assert h, yi.getLastError()
            c = spf.consts(frm, to, col, power, angle, blend, 0.75)
            want = spf.record(c, soft, 5)
            got = bits(yi.getLights()[0])
            assert np.array_equal(got, want), (axis, angle, blend, np.nonzero(got != want)[0], got.view(np.float32), want.view(np.float32))
            if blend == 0.0:
                assert c["cos_start"] == c["cos_end"] and np.isinf(c["icos_diff"])


def test_constants_are_what_the_constructor_says():
    """the restatement itself against the plain formulas: the polynomial fCos__ stays within 1.1e-3 of the cosine, the inner cone is
    never narrower than nothing, and icos_diff_ is the reciprocal of the difference"""
    for angle in (5.0, 45.0, 90.0, 120.0, 180.0):
        for blend in (0.15, 0.5, 1.0):
            c = spf.consts(*AXES["skew"], cone_angle=angle, blend=blend)
            assert abs(float(c["cos_end"]) - np.cos(np.radians(angle))) < 1.1e-3
            assert abs(float(c["cos_start"]) - np.cos(np.radians(angle) * (1.0 - blend))) < 1.1e-3
            assert c["cos_start"] > c["cos_end"] and c["icos_diff"] == np.float32(1.0 / float(np.float32(c["cos_start"] - c["cos_end"])))


def test_defaults():
    yi, h = spot(**{"from": (0.0, 0.0, 0.0), "to": (0.0, 0.0, -1.0)})      # the reference's own defaults, spelled out
    assert h, yi.getLastError()
    rec = yi.getLights()[0]
    want = spf.record(spf.consts((0, 0, 0), (0, 0, -1), (1, 1, 1), 1.0, 45.0, 0.15, 1.0))
    assert np.array_equal(bits(rec), want)
    assert rec[4:7].tolist() == [0, 0, 1] and rec[7:10].tolist() == [-1, 0, 0] and rec[10:13].tolist() == [0, 1, 0]
    soft = spot(**{"from": (0.0, 0.0, 0.0), "to": (0.0, 0.0, -1.0), "soft_shadows": True})[0].getLights()[0]
    assert [int(x) for x in soft[:4].view(np.int32)] == [spf.TYPE_SPOT_SOFT, 8, 1, 0]


def test_each_parameter_alone():
    base = spot(**AIM)[0].getLights()[0]

    def rec_of(**kw):
        yi, h = spot(**dict(AIM, **kw))
        assert h, yi.getLastError()
        return yi.getLights()[0]

    def changed(rec):
        return sorted(set(np.nonzero(bits(rec) != bits(base))[0].tolist()))

    assert changed(rec_of(color=color(0.5, 0.25, 0.125))) == [25, 26, 27]
    assert rec_of(power=3.0)[25:28].tolist() == [3, 3, 3]
    assert changed(rec_of(cone_angle=30.0)) == [13, spf.W_COS_START, spf.W_ICOS_DIFF]
    assert changed(rec_of(blend=0.5)) == [spf.W_COS_START, spf.W_ICOS_DIFF]
    assert changed(rec_of(shadowFuzzyness=0.25)) == [spf.W_FUZZY]
    assert changed(rec_of(cast_shadows=False)) == [2]
    assert changed(rec_of(samples=5)) == []                            # a Dirac light has one sample
    assert changed(rec_of(soft_shadows=True)) == [0, 1]
    assert [int(x) for x in rec_of(soft_shadows=True, samples=5)[:2].view(np.int32)] == [spf.TYPE_SPOT_SOFT, 5]
    for k, v in (("with_caustic", False), ("with_diffuse", False), ("photon_only", False)):
        assert changed(rec_of(**{k: v})) == [], k                      # read and unused


def test_disabled_spot_leaves_no_record():
    yi, h = spot(**dict(AIM, light_enabled=False))
    assert h, yi.getLastError()
    assert yi.getLights().shape[0] == 0


def test_spots_keep_their_place_in_the_light_order():
    yi = Interface(strict=False)
    yi.startScene(0)
    order = [("a", {"type": "pointlight", "from": (0.0, 0.0, 1.0)}), ("b", dict({"type": "spotlight"}, **AIM)),
             ("c", dict({"type": "spotlight", "light_enabled": False}, **AIM)), ("d", {"type": "sunlight", "direction": (0.0, 0.0, 1.0)}),
             ("e", dict({"type": "spotlight", "soft_shadows": True}, **AIM)), ("f", {"type": "pointlight", "from": (1.0, 0.0, 1.0)})]
    for name, params in order:
        yi.paramsClearAll(); yi.paramsSet(params)
        assert yi.createLight(name), yi.getLastError()
    assert [int(t) for t in yi.getLights()[:, 0].view(np.int32)] == [1, 11, 3, 12, 1]


# ---- yafgpu_scene_create ------------------------------------------------------------------------------------------------
DESC_CASES = {
    "type_6": (-2, "light 0: unknown type"), "type_13": (-2, "light 0: unknown type"),
    "cos_end_nan": (-3, "spot light 0: the cosines of its cone are not finite"),
    "cos_start_infinite": (-3, "spot light 0: the cosines of its cone are not finite"),
    "icos_diff_nan": (-3, "spot light 0: icos_diff is not a number"), "fuzzy_nan": (-3, "spot light 0: shadow_fuzzy is not finite"),
    "axis_nan": (-3, "spot light 0: its axis is not finite"),
}
VALID = ["valid", "valid_soft", "valid_blend_zero"]


@pytest.fixture(scope="module")
def desc_answers(tmp_path_factory):
    lib = interface.lib_path()
    exe = tmp_path_factory.mktemp("spot_desc") / "spot_desc_cases"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "spot_desc_cases.cpp"),
                    lib, "-Wl,-rpath," + os.path.dirname(os.path.abspath(lib)), "-o", str(exe)], check=True, timeout=300)
    out = subprocess.run([str(exe)], check=True, timeout=120, capture_output=True, text=True).stdout
    got = {}
    for ln in out.splitlines():
        name, code, msg = ln.split(" ", 2)
        got[name] = (int(code), msg)
    return got


def test_every_descriptor_case_answered(desc_answers):
    assert set(desc_answers) == set(DESC_CASES) | set(VALID)


@pytest.mark.parametrize("case", sorted(DESC_CASES))
def test_descriptor_refused_before_device_work(desc_answers, case):
    """types 6 and 13 stay unknown; a spot record's numbers are checked before anything is allocated"""
    assert desc_answers[case] == DESC_CASES[case]


@pytest.mark.parametrize("case", VALID)
def test_valid_descriptor_is_taken(desc_answers, case):
    """0, or the first HIP call's failure where the machine has no device"""
    code, msg = desc_answers[case]
    assert code == 0 or (code == -100 and msg.startswith("hip")), (code, msg)


# ---- XML ------------------------------------------------------------------------------------------------------------------
XML = """<?xml version="1.0"?>
<scene type="triangle">
<material name="white"><type sval="shinydiffusemat"/><color r="0.8" g="0.8" b="0.8" a="1"/><diffuse_reflect fval="1"/></material>
<light name="Key"><type sval="spotlight"/><from x="0.25" y="-0.5" z="2"/><to x="0.75" y="0.25" z="0"/>
  <color r="1" g="0.9" b="0.8" a="1"/><power fval="4"/><cone_angle fval="35"/><blend fval="0.4"/></light>
<light name="Fill"><type sval="spotlight"/><from x="-1" y="0" z="1.5"/><to x="0" y="0" z="-1"/>
  <color r="0.5" g="0.5" b="1" a="1"/><power fval="2"/><cone_angle fval="60"/><blend fval="0.15"/>
  <soft_shadows bval="true"/><samples ival="3"/><shadowFuzzyness fval="0.5"/><cast_shadows bval="false"/></light>
<camera name="cam"><type sval="perspective"/><from x="0" y="-3" z="0"/><to x="0" y="0" z="0"/><up x="0" y="-3" z="1"/>
  <resx ival="16"/><resy ival="16"/><focal fval="1.2"/></camera>
<integrator name="default"><type sval="directlighting"/><caustic_type sval="none"/></integrator>
<integrator name="volintegr"><type sval="none"/></integrator>
<mesh id="1" vertices="4" faces="2" has_orco="false" has_uv="false" type="0">
  <p x="-1" y="-1" z="-1"/><p x="1" y="-1" z="-1"/><p x="1" y="1" z="-1"/><p x="-1" y="1" z="-1"/>
  <set_material sval="white"/><f a="0" b="1" c="2"/><f a="0" b="2" c="3"/>
</mesh>
<render><camera_name sval="cam"/><integrator_name sval="default"/><volintegrator_name sval="volintegr"/>
  <width ival="16"/><height ival="16"/><AA_passes ival="1"/><AA_minsamples ival="1"/>
  <AA_pixelwidth fval="1"/><filter_type sval="box"/><tile_size ival="8"/></render>
</scene>
"""
XML_LIGHTS = [("Key", {"type": "spotlight", "from": (0.25, -0.5, 2.0), "to": (0.75, 0.25, 0.0), "color": color(1.0, 0.9, 0.8), "power": 4.0,
                       "cone_angle": 35.0, "blend": 0.4}),
              ("Fill", {"type": "spotlight", "from": (-1.0, 0.0, 1.5), "to": (0.0, 0.0, -1.0), "color": color(0.5, 0.5, 1.0), "power": 2.0,
                        "cone_angle": 60.0, "blend": 0.15, "soft_shadows": True, "samples": 3, "shadowFuzzyness": 0.5, "cast_shadows": False})]


def test_xml_scene_loads_to_the_records_of_the_api_calls(tmp_path):
    p = tmp_path / "spots.xml"
    p.write_text(XML)
    yi = Interface(strict=False)
    assert yi.loadXml(str(p)), yi.getLastError()
    got = yi.getLights()
    api = Interface(strict=False)
    api.startScene(0)
    for name, params in XML_LIGHTS:
        api.paramsClearAll(); api.paramsSet(params)
        assert api.createLight(name), api.getLastError()
    want = api.getLights()
    assert got.shape == want.shape == (2, 34) and np.array_equal(bits(got), bits(want))
    assert [int(t) for t in got[:, 0].view(np.int32)] == [11, 12] and [int(t) for t in got[:, 1].view(np.int32)] == [1, 3]
    want1 = spf.record(spf.consts((-1, 0, 1.5), (0, 0, -1), (0.5, 0.5, 1.0), 2.0, 60.0, 0.15, 0.5), True, 3)
    want1[2] = 0                                                       # cast_shadows off
    assert np.array_equal(bits(got[1]), want1)


# ---- the reference's compiled SpotLight -----------------------------------------------------------------------------------
# tests/golden/ref_spot_ies_{ieee,fast}.json.gz: SpotLight made by its factory in the reference harness (oracle/ref_harness/ref_spot_ies.cc)
from tests import pin_fixture as pin                                   # noqa: E402
from tests.test_oracle_golden import FAST_ATOL, FAST_RTOL              # noqa: E402

SPOT_LEAVES = (("illuminate", lambda c, x: spf.illuminate(c, x)), ("illum_sample", lambda c, x: spf.illum_sample(c, x[:, :3], x[:, 3], x[:, 4])),
               ("intersect", lambda c, x: spf.intersect(c, x[:, :3], x[:, 3:6])))


def pinned_consts(p):
    return spf.consts(p["from"], p["to"], p["color"], p["power"], p.get("cone_angle", 45.0), p.get("blend", 0.15), p.get("shadowFuzzyness", 1.0))


def record_consts(r):
    """the constants the leaf functions read, taken from a yafgpu_light record's words"""
    return {"ndir": r[4:7], "du": r[7:10], "dv": r[10:13], "cos_end": r[13], "cos_start": r[spf.W_COS_START], "icos_diff": r[spf.W_ICOS_DIFF],
            "fuzzy": r[spf.W_FUZZY], "color": r[25:28], "position": r[29:32]}


def spot_sets(doc):
    return [(n, fns) for names, fns in ((doc["spot_sets"], SPOT_LEAVES[:2]), (doc["intersect_sets"], SPOT_LEAVES[2:])) for n in names]


def test_fixture_lights_are_the_gpu_tests_lights():
    from tests import test_gpu_spot as g
    doc = pin.load("spot_ies", "ieee")
    assert len(doc["spot_sets"]) == len(g.LEAF) and len(doc["intersect_sets"]) == len(g.ORIGIN_LIGHTS)
    for name, (a, b, f, s) in zip(doc["spot_sets"], g.LEAF):
        p = pin.params(doc, name)
        assert (p["from"], p["to"], p["color"], p["power"]) == tuple(tuple(float(np.float32(v)) for v in t) if isinstance(t, tuple) else t
                                                                      for t in (g.FROM, g.TO, g.COL, g.POWER))
        assert (p["cone_angle"], np.float32(p["blend"]), p["shadowFuzzyness"], p["soft_shadows"]) == (a, np.float32(b), f, s)
    for name, (frm, to) in zip(doc["intersect_sets"], g.ORIGIN_LIGHTS):
        p = pin.params(doc, name)
        assert p["from"] == tuple(float(np.float32(v)) for v in frm) and p["to"] == tuple(float(np.float32(v)) for v in to)
        assert (p["cone_angle"], p["blend"], p["soft_shadows"]) == (45.0, 0.5, True)


def test_restatement_reproduces_the_reference_bit_for_bit():
    """tests/spot_fixture.py on the inputs of the IEEE fixture: every output word of illuminate, illumSample and intersect, the three
    flags; and the same leaf functions fed with the words of the record createLight makes of the stored parameters, which holds
    colour times power, the axis, du / dv, both cosines, icos_diff_ and the fuzzyness to the reference's constructor at once"""
    doc = pin.load("spot_ies", "ieee")
    for name, fns in spot_sets(doc):
        p = pin.params(doc, name)
        yi, h = light_of({k: (color(*v) if k == "color" else v) for k, v in p.items()})
        assert h, (name, yi.getLastError())
        rec = yi.getLights()[0]
        soft = bool(p["soft_shadows"])
        assert doc[name + "_flags3"] == [int(not soft), int(soft), p["samples"]]
        assert [int(x) for x in rec[:2].view(np.int32)] == [spf.TYPE_SPOT_SOFT if soft else spf.TYPE_SPOT, p["samples"] if soft else 1]
        for fn, restated in fns:
            inp, want, _ = pin.leaf(doc, name, fn)
            pin.same(restated(pinned_consts(p), inp), want, f"{name} {fn}")
            pin.same(restated(record_consts(rec), inp), want, f"{name} {fn} from the record's words")


def test_record_cosines_straddle_what_the_reference_took_and_refused():
    """cos_end_: the largest cosine the reference refused lies below the record's word, the smallest it accepted at or above it.  cos_start_:
    illumSample hands out colour times power untouched at or above it and scaled by the smoothstep below: every row whose colour is
    smaller lies below the record's word, every row at or above it carries the record's colour bit for bit"""
    doc = pin.load("spot_ies", "ieee")
    for name in doc["spot_sets"]:
        p = pin.params(doc, name)
        yi, h = light_of({k: (color(*v) if k == "color" else v) for k, v in p.items()})
        rec = yi.getLights()[0]
        inp, want, _ = pin.leaf(doc, name, "illum_sample")
        out = want.view(np.float32)
        _, dist_sqr, dist, cosa, _ = spf._to_light(record_consts(rec), inp[:, :3])
        ok = out[:, 0] == 1
        away = dist != 0
        assert cosa[away & ~ok].max() < rec[13] <= cosa[ok].min(), name
        # the threshold rows sit ON the cone and on its float neighbour below (ref_spot_ies.cc places them there)
        assert cosa[ok].min() == rec[13] and np.nextafter(cosa[away & ~ok].max(), np.float32(2)) == rec[13], name
        far = ok & (out[:, 5] > 1)
        full = (out[:, 6:9] == rec[25:28]).all(axis=1)
        less = (out[:, 6:9] < rec[25:28]).all(axis=1)
        assert (full | less)[far].all() and full[far].any(), name
        assert full[far & (cosa >= rec[spf.W_COS_START])].all(), name
        if p["blend"] > 0:
            assert less[far].any() and cosa[far & less].max() < rec[spf.W_COS_START], name
        else:
            assert full[far].all() and rec[spf.W_COS_START] == rec[13]


def falloff_step(c, pts, over_dist_sqr):
    """what a float step of cos_end_ moves the colour by, (n, 3), in float64 from the formulas: the two builds of the reference form the
    5 degree cone's cos_end_ a float step apart (2^-24 for a cosine in [0.5, 1)), which moves the smoothstep's argument v = (cosa - cos_end_)
    * icos_diff_ by dv = 2^-24 * icos_diff_ and s(v) = v^2 (3 - 2 v) by at most s'(v) dv + 3 dv^2 with s'(v) = 6 v (1 - v); the colour is
    colour x power x s(v), over the squared distance in illuminate and, nearer than 1, in illumSample.  (The caller doubles it: icos_diff_
    moves with cos_end_ too, by the same relative amount.)"""
    ldir = c["position"].astype(np.float64) - pts.astype(np.float64)
    d2 = (ldir ** 2).sum(axis=1)
    with np.errstate(all="ignore"):
        cosa = ldir @ c["ndir"].astype(np.float64) / np.sqrt(d2)
        v = np.clip((cosa - float(c["cos_end"])) * float(c["icos_diff"]), 0.0, 1.0)
        dv = 2.0 ** -24 * float(c["icos_diff"]) if np.isfinite(c["icos_diff"]) else 0.0
        ds = 6.0 * v * (1.0 - v) * dv + 3.0 * dv * dv
        k = np.where(over_dist_sqr | (d2 < 1.0), 1.0 / d2, 1.0)
    return np.nan_to_num(c["color"].astype(np.float64)[None, :] * (k * ds)[:, None], nan=0.0, posinf=0.0)


def test_release_flag_build_of_the_reference_agrees():
    """the two builds of the reference against each other, then the restatement against the release-flag one on the rows where the two
    agree on `ok`.  The smoothstep's argument (cosa - cos_end_) * icos_diff_ cancels: one float step of cosa (6e-8) is a relative
    6e-8 * icos_diff_ / v of v, unbounded towards the cone's edge.  So the band of a falloff row is twice what the two builds of the
    reference differ by on that row ("Spot lights": the largest measured difference is written there), never less than the
    tolerances every release-flag fixture is compared with"""
    ieee, fast = pin.load("spot_ies", "ieee"), pin.load("spot_ies", "fast")
    worst = 0.0
    for name, fns in spot_sets(ieee):
        p = pin.params(ieee, name)
        assert pin.params(fast, name) == p
        for fn, restated in fns:
            inp, a, _ = pin.leaf(ieee, name, fn)
            inp_f, b, _ = pin.leaf(fast, name, fn)
            # the same rows, but for those the driver places ON a cone: they follow each build's own cosines, which differ by a float step
            # for the 5 degree cone, so that each build's rows sit at its own threshold and on either side of it
            same_input = (inp.view(np.uint32) == inp_f.view(np.uint32)).all(axis=1)
            assert same_input.mean() > 0.6 and (same_input.all() or p["cone_angle"] == 5.0), (name, fn, same_input.mean())
            # Such a row is a threshold row of a threshold the two builds put a float step apart: each build was asked its own question there.
            # The comparison between the two fixtures leaves them out; the restatement is held to the release-flag build's own rows below.
            a, b = a.view(np.float32).astype(np.float64), b.view(np.float32).astype(np.float64)
            agree = (a[:, 0] == b[:, 0]) & same_input
            assert (a[:, 0] != b[:, 0]).mean() < 0.01, (name, fn, (a[:, 0] != b[:, 0]).mean())
            between = np.abs(a - b)
            over = between - (FAST_ATOL + FAST_RTOL * np.abs(b))
            worst = max(worst, float((between[agree] / np.maximum(np.abs(b[agree]), 1e-30)).max()))
            band = np.maximum(FAST_ATOL + FAST_RTOL * np.abs(b), 2.0 * between)
            got = restated(pinned_consts(p), inp_f).astype(np.float64)
            bad = (np.abs(got - b) > band) & agree[:, None]
            assert not bad.any(), (name, fn, int(bad.sum()), np.nonzero(bad.any(axis=1))[0][:5])
            # the rows asked apart: the release-flag build's own question and answer against the restatement with the plain tolerances,
            # wherever the restatement (IEEE thresholds, a float step from that build's) decides `ok` as that build did
            apart = ~same_input & (got[:, 0] == b[:, 0])
            tol = FAST_ATOL + FAST_RTOL * np.abs(b)
            tol[:, -3:] += 2.0 * falloff_step(pinned_consts(p), inp_f[:, :3], fn == "illuminate")
            assert (np.abs(got - b) <= tol)[apart].all(), (name, fn)
            assert same_input.all() or apart.sum() >= 0.5 * (~same_input).sum(), (name, fn, int(apart.sum()))
            print(f"{name} {fn}: {int((a[:, 0] != b[:, 0]).sum())} rows of {len(a)} differ in ok, {int((~same_input).sum())} were asked apart, {int((over[agree] > 0).any(axis=1).sum())} rows beyond the plain tolerances between the builds")
    print(f"largest relative difference between the two builds of the reference: {worst:.3g}")
