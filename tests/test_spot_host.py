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
