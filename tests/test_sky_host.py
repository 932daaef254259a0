"""The sky backgrounds on the host: GradientBackground::factory (background_gradient.cc:61-103), SunSkyBackground's factory and
constructor (background_sunsky.cc:37-76, :181-264), the background light they add, the refusals, the XML loader, and which sunsky
tables have rows without energy.  No GPU needed.  The restatements are in tests/sky_fixture.py."""
import numpy as np
import pytest

from libyafaray_amd import Interface
from tests import sky_fixture as sf
from tests.test_background_host import LIGHT_BACKGROUND, W_ABS, W_CLAMP, background, fresh, light_rows, prepared_scene
from tests.test_lights_host import F, bits, ints

HOR, ZEN = ("color", 0.9, 0.7, 0.5, 1.0), ("color", 0.2, 0.35, 0.8, 1.0)
GRAD = {"type": "gradientback", "horizon_color": HOR, "zenith_color": ZEN}
EPS = 2.0 ** -52


def rgb(c):
    return np.array(c[1:4], np.float32)


# ---- gradientback ---------------------------------------------------------------------------------------------------
def test_gradientback_defaults_and_every_parameter():
    yi = fresh()
    assert background(yi, "bg", GRAD), yi.getLastError()
    b, k = yi.getBackground("bg"), yi.getSky("bg")
    assert (b["kind"], b["has_ibl"], b["shoots_caustic"]) == (4, 0, 1) and b["power"] == 1
    assert yi.getLights().shape[0] == 0                             # no ibl, no light
    # power defaults to 1; the ground colours default to the sky's
    for name, want in (("horizon", HOR), ("zenith", ZEN), ("horizon_ground", HOR), ("zenith_ground", ZEN)):
        assert np.array_equal(bits(k[name]), bits(rgb(want))), name
    # every parameter: the factory multiplies power into all four colours; with_caustic = false does not reach the background (:84)
    gh, gz = ("color", 0.3, 0.25, 0.2, 1.0), ("color", 0.05, 0.1, 0.02, 1.0)
    yi = fresh()
    assert background(yi, "bg", dict(GRAD, horizon_ground_color=gh, zenith_ground_color=gz, power=2.5, ibl=True, ibl_samples=5,
                                     cast_shadows=False, with_caustic=False, with_diffuse=False, light_enabled=False)), yi.getLastError()
    b, k = yi.getBackground("bg"), yi.getSky("bg")
    assert (b["kind"], b["has_ibl"], b["shoots_caustic"]) == (4, 1, 1) and b["power"] == F(2.5)
    for name, want in (("horizon", HOR), ("zenith", ZEN), ("horizon_ground", gh), ("zenith_ground", gz)):
        assert np.array_equal(bits(k[name]), bits(rgb(want) * F(2.5))), name
    # the light: samples, cast_shadows, no clamp, abs_intersect false; light_enabled is not among the parameters the factory passes on
    rec, types = light_rows(yi)
    assert types == [LIGHT_BACKGROUND]
    assert list(ints(rec[0])[:3]) == [LIGHT_BACKGROUND, 5, 0] and rec[0, W_CLAMP] == 0 and int(rec[0, W_ABS:].view(np.int32)[0]) == 0
    # the light's defaults
    yi = fresh()
    assert background(yi, "bg", dict(GRAD, ibl=True)), yi.getLastError()
    assert list(ints(yi.getLights()[0])[:3]) == [LIGHT_BACKGROUND, 16, 1]
    # a background of another type leaves the sky record zero
    assert background(yi, "c", {"type": "constant", "color": HOR}), yi.getLastError()
    k = yi.getSky("c")
    assert not k["horizon"].any() and k["theta_s"] == 0 and not k["perez_Y"].any()


# ---- sunsky ---------------------------------------------------------------------------------------------------------
def test_sunsky_defaults_and_the_light():
    yi = fresh()
    assert background(yi, "bg", {"type": "sunsky", "from": (1.0, 1.0, 1.0)}), yi.getLastError()
    b, k = yi.getBackground("bg"), yi.getSky("bg")
    assert (b["kind"], b["has_ibl"], b["shoots_caustic"]) == (5, 0, 1) and b["power"] == 1
    assert k["turbidity"] == 4 and k["power"] == 1 and np.array_equal(k["from"], [1, 1, 1])
    assert yi.getLights().shape[0] == 0
    want, _ = sf.sunsky_constants((1.0, 1.0, 1.0))                   # turbidity 4, a_var .. e_var 1
    assert k["theta_s"] == want["theta_s"] and np.allclose(k["perez_Y"], want["perez_Y"], rtol=1e-14, atol=0)
    # the light is asked for by background_light / light_samples (not ibl / ibl_samples), defaults 8 samples and shadows
    yi = fresh()
    assert background(yi, "bg", {"type": "sunsky", "from": (1.0, 1.0, 1.0), "background_light": True, "ibl_samples": 3}), yi.getLastError()
    rec, types = light_rows(yi)
    assert types == [LIGHT_BACKGROUND] and list(ints(rec[0])[:3]) == [LIGHT_BACKGROUND, 8, 1]
    assert rec[0, W_CLAMP] == 0 and int(rec[0, W_ABS:].view(np.int32)[0]) == 0
    yi = fresh()
    assert background(yi, "bg", {"type": "sunsky", "from": (1.0, 1.0, 1.0), "ibl": True}), yi.getLastError()
    assert yi.getLights().shape[0] == 0 and yi.getBackground("bg")["has_ibl"] == 0
    yi = fresh()
    assert background(yi, "bg", {"type": "sunsky", "from": (1.0, 1.0, 1.0), "power": 0.75, "background_light": True, "light_samples": 3,
                                 "cast_shadows": False, "cast_shadows_sun": False, "sun_power": 3.0, "add_sun": False,
                                 "with_caustic": False, "with_diffuse": False, "light_enabled": False}), yi.getLastError()
    b = yi.getBackground("bg")
    assert (b["has_ibl"], b["shoots_caustic"]) == (1, 1) and b["power"] == F(0.75) and yi.getSky("bg")["power"] == F(0.75)
    assert list(ints(yi.getLights()[0])[:3]) == [LIGHT_BACKGROUND, 3, 0]


VARS = (1.0, 1.0, 1.0, 1.0, 1.0)


@pytest.mark.parametrize("frm, turbidity, var", [(f, t, VARS) for f, t in sf.SUNSKY_CASES] + [((1.0, 0.2, 0.15), 2.5, (1.3, 0.7, 1.1, 0.85, 1.25)),
                                                                                              (sf.SUNSKY_EMPTY[0], sf.SUNSKY_EMPTY[1], VARS)])
def test_sunsky_record_against_the_constructor_in_float64(frm, turbidity, var):
    """Every value of the record is a sum of at most twelve rounded double operations over terms whose magnitudes add up to `scale`, and
    takes at most one C library result (acos, atan2 or tan) that enters those sums with a factor no larger than the term it stands in.
    The library and the restatement round each operation alike (IEEE double, no contraction) and call the same C library, so they
    should agree exactly; were the library results one ulp apart, the values would differ by that ulp of their term plus half an ulp
    per operation it passes through.  Bound: 16 ulps of `scale` — twelve operations at half an ulp, the library's ulp, and as much again."""
    yi = fresh()
    p = {"type": "sunsky", "from": frm, "turbidity": turbidity}
    p.update({n: v for n, v in zip(("a_var", "b_var", "c_var", "d_var", "e_var"), var)})
    assert background(yi, "bg", p), yi.getLastError()
    k = yi.getSky("bg")
    want, scale = sf.sunsky_constants(frm, turbidity, var)
    assert k["turbidity"] == F(turbidity) and np.array_equal(k["from"], np.array(frm, np.float32))
    assert k["theta_s"] == want["theta_s"] == float(np.float32(want["theta_s"]))      # fAcos__'s float, widened
    for name in ("phi_s", "zenith_x", "zenith_y", "zenith_Y", "perez_x", "perez_y", "perez_Y"):
        err = np.abs(np.asarray(k[name]) - np.asarray(want[name]))
        assert (err <= 16 * EPS * np.asarray(scale[name])).all(), (name, k[name], want[name], err / EPS)
    assert (frm[2] < 0) == (k["theta_s"] > np.pi / 2)


# ---- refusals -------------------------------------------------------------------------------------------------------
def test_refusals_name_their_cause():
    yi = fresh()
    # the bare calls stay outside the scope, and say what the type would need
    for t, needs in (("sunsky", "from"), ("gradientback", "horizon_color"), ("darksky", "spectral")):
        assert not background(yi, "bg", {"type": t})
        msg = yi.getLastError()
        assert "scope" in msg and "constant" in msg and "textureback" in msg and needs in msg, msg
    assert not background(yi, "bg", {"type": "gradientback", "horizon_color": HOR})
    assert "zenith_color" in yi.getLastError() and "scope" in yi.getLastError()
    assert not background(yi, "bg", {"type": "gradientback", "zenith_color": ZEN})
    assert "horizon_color" in yi.getLastError()
    # darksky stays refused whatever it is given
    assert not background(yi, "bg", {"type": "darksky", "from": (1.0, 1.0, 1.0), "turbidity": 3.0})
    assert "scope" in yi.getLastError() and "spectral" in yi.getLastError()
    # add_sun: the parameter, the cause, and what does the job
    assert not background(yi, "bg", {"type": "sunsky", "from": (1.0, 1.0, 1.0), "add_sun": True})
    msg = yi.getLastError()
    assert "add_sun" in msg and "spectral" in msg and "sunlight" in msg, msg
    # values that are not finite, and a direction that is none
    assert not background(yi, "bg", dict(GRAD, zenith_color=("color", 0.2, float("nan"), 0.8, 1.0)))
    assert "finite" in yi.getLastError()
    assert not background(yi, "bg", dict(GRAD, power=float("inf")))
    assert "finite" in yi.getLastError()
    assert not background(yi, "bg", {"type": "sunsky", "from": (1.0, 1.0, 1.0), "turbidity": float("nan")})
    assert "finite" in yi.getLastError() and "turbidity" in yi.getLastError()
    assert not background(yi, "bg", {"type": "sunsky", "from": (1.0, float("inf"), 1.0)})
    assert "finite" in yi.getLastError()
    assert not background(yi, "bg", {"type": "sunsky", "from": (0.0, 0.0, 0.0)})
    assert "zero vector" in yi.getLastError() and "from" in yi.getLastError()
    assert yi.getLights().shape[0] == 0                             # a refused background leaves no light behind


def test_two_skies_with_lights_are_refused_at_prepare_render(tmp_path):
    sun = {"type": "sunsky", "from": (1.0, 1.0, 1.0), "background_light": True}
    for pair in ((("a", dict(GRAD, ibl=True)), ("b", sun)), (("a", sun), ("b", sun)), (("a", dict(GRAD, ibl=True)), ("b", dict(GRAD, ibl=True)))):
        yi = prepared_scene(tmp_path, list(pair), "a")
        assert not yi.prepareRender()
        assert "more than one background" in yi.getLastError()
    # a sky with a light that is not the selected background
    yi = prepared_scene(tmp_path, [("lit", sun), ("plain", GRAD)], "plain")
    assert not yi.prepareRender()
    assert "background_name" in yi.getLastError()


# ---- the XML loader -------------------------------------------------------------------------------------------------
XML = """<?xml version="1.0"?>
<scene type="triangle">
<material name="white"><type sval="shinydiffusemat"/><color r="0.8" g="0.8" b="0.8" a="1"/><diffuse_reflect fval="1"/></material>
<camera name="cam"><type sval="perspective"/><from x="0" y="-3" z="0"/><to x="0" y="0" z="0"/><up x="0" y="-3" z="1"/>
  <resx ival="16"/><resy ival="16"/><focal fval="1.2"/></camera>
%(background)s
<integrator name="default"><type sval="directlighting"/><caustic_type sval="none"/></integrator>
<integrator name="volintegr"><type sval="none"/></integrator>
<mesh id="1" vertices="4" faces="2" has_orco="false" has_uv="false" type="0">
  <p x="-1" y="-1" z="-1"/><p x="1" y="-1" z="-1"/><p x="1" y="1" z="-1"/><p x="-1" y="1" z="-1"/>
  <set_material sval="white"/><f a="0" b="1" c="2"/><f a="0" b="2" c="3"/>
</mesh>
<render><camera_name sval="cam"/><integrator_name sval="default"/><volintegrator_name sval="volintegr"/>
  <background_name sval="world_background"/>
  <width ival="16"/><height ival="16"/><AA_passes ival="1"/><AA_minsamples ival="1"/>
  <AA_pixelwidth fval="1"/><filter_type sval="box"/><tile_size ival="8"/></render>
</scene>
"""
XML_SUNSKY = """<background name="world_background"><type sval="sunsky"/><from x="1" y="0.2" z="0.15"/><turbidity fval="2.5"/>
  <a_var fval="1"/><b_var fval="1"/><c_var fval="1"/><d_var fval="1"/><e_var fval="1"/><add_sun bval="false"/><sun_power fval="1"/>
  <background_light bval="true"/><light_samples ival="6"/><power fval="1.25"/><cast_shadows bval="true"/><cast_shadows_sun bval="true"/>
  <with_caustic bval="true"/><with_diffuse bval="true"/></background>"""
XML_GRADIENT = """<background name="world_background"><type sval="gradientback"/><horizon_color r="0.9" g="0.7" b="0.5" a="1"/>
  <zenith_color r="0.2" g="0.35" b="0.8" a="1"/><horizon_ground_color r="0.3" g="0.25" b="0.2" a="1"/>
  <zenith_ground_color r="0.05" g="0.1" b="0.02" a="1"/><power fval="2"/><ibl bval="true"/><ibl_samples ival="7"/>
  <cast_shadows bval="false"/><with_caustic bval="true"/><with_diffuse bval="true"/></background>"""


def test_xml_scene_with_each_sky_loads(tmp_path):
    p = tmp_path / "sunsky.xml"
    p.write_text(XML % {"background": XML_SUNSKY})
    yi = Interface(strict=False)
    assert yi.loadXml(str(p)), yi.getLastError()
    rec, types = light_rows(yi)
    assert types == [LIGHT_BACKGROUND] and list(ints(rec[0])[:3]) == [LIGHT_BACKGROUND, 6, 1]
    b, k = yi.getBackground("world_background"), yi.getSky("world_background")
    want, scale = sf.sunsky_constants((1.0, 0.2, 0.15), 2.5)
    assert (b["kind"], b["has_ibl"]) == (5, 1) and k["power"] == F(1.25) and k["theta_s"] == want["theta_s"]
    assert abs(k["zenith_Y"] - want["zenith_Y"]) <= 16 * EPS * scale["zenith_Y"]
    p = tmp_path / "gradient.xml"
    p.write_text(XML % {"background": XML_GRADIENT})
    yi = Interface(strict=False)
    assert yi.loadXml(str(p)), yi.getLastError()
    rec, types = light_rows(yi)
    assert types == [LIGHT_BACKGROUND] and list(ints(rec[0])[:3]) == [LIGHT_BACKGROUND, 7, 0]
    b, k = yi.getBackground("world_background"), yi.getSky("world_background")
    assert (b["kind"], b["has_ibl"]) == (4, 1)
    assert np.array_equal(bits(k["zenith_ground"]), bits(np.array([0.05, 0.1, 0.02], np.float32) * F(2)))
    assert np.array_equal(bits(k["horizon"]), bits(np.array([0.9, 0.7, 0.5], np.float32) * F(2)))


# ---- which sunsky tables have rows without energy ---------------------------------------------------------------------
def empty_rows(frm, turbidity):
    """the rows of the background light's tables whose integral is not a finite number above zero, by the restatement"""
    k, _ = sf.sunsky_constants(frm, turbidity)
    dirs, yy, sintheta, nu = sf.table_dirs()
    tab = sf.sky_tables(sf.sunsky_eval(k, dirs), yy, sintheta, nu)
    ok = (tab[:sf.NV, 1] > 0) & np.isfinite(tab[:sf.NV, 1])
    return int((~ok).sum()), tab


def test_which_sunsky_tables_have_rows_without_energy():
    """What the GPU tests rely on: the four accepted cases leave no latitude row without energy, the sun well below the horizon leaves many
    (and the scene with its light is then refused on the device, tests/test_gpu_sky.py)."""
    for frm, turbidity in sf.SUNSKY_CASES:
        n, tab = empty_rows(frm, turbidity)
        assert n == 0 and tab[sf.NV, 1] > 0, (frm, turbidity, n)
    n, _ = empty_rows(*sf.SUNSKY_EMPTY)
    print("rows without energy for", sf.SUNSKY_EMPTY, ":", n, "of", sf.NV)
    assert 100 < n < sf.NV
