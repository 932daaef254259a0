"""The mask material on the host: MaskMaterial::factory (material_mask.cc:133-190) as createMaterial restates it — its parameters and
defaults as yafaray_getMaskMaterial hands them back, every refusal with its cause, the XML loader — and the material table the device
scene gets (yafaray_getMaterialTable): the mask's record and the two hidden clones of its sub-materials it picks from.  No GPU needed."""
import os

import numpy as np
import pytest

from libyafaray_amd import Interface
from tests.test_lights_host import F, bits

MAT_SHINYDIFFUSE, MAT_GLASS, MAT_MASKED = 0, 3, 7
BSDF_SPECULAR, BSDF_GLOSSY, BSDF_DIFFUSE, BSDF_REFLECT, BSDF_TRANSMIT, BSDF_FILTER, BSDF_VOLUMETRIC = 0x1, 0x2, 0x4, 0x10, 0x20, 0x40, 0x100
W = Interface.MATERIAL_FIELDS

RED = {"type": "shinydiffusemat", "color": ("color", 0.8, 0.1, 0.1, 1.0), "diffuse_reflect": 1.0}
BLUE = {"type": "shinydiffusemat", "color": ("color", 0.1, 0.1, 0.8, 1.0), "diffuse_reflect": 0.9}
VALUE_NODE = {"type": "value", "name": "val", "scalar": 0.6}


def fresh():
    yi = Interface(strict=False)
    yi.startScene(0)
    return yi


def material(yi, name, params, nodes=()):
    yi.paramsClearAll()
    yi.paramsSet(params)
    for node in nodes:
        yi.paramsPushList()
        yi.paramsSet(dict(node, element="shader_node"))
        yi.paramsEndList()
    return yi.createMaterial(name)


def texture(yi, name, texels=None):
    yi.paramsClearAll()
    yi.paramsSet({"type": "image", "interpolate": "none", "color_space": "LinearRGB"})
    return yi.createTextureFromMemory(name, np.full((2, 2, 4), 0.25, np.float32) if texels is None else texels)


def two_subs(yi, a=RED, b=BLUE):
    assert material(yi, "a", a), yi.getLastError()
    assert material(yi, "b", b), yi.getLastError()


def mask(yi, name="m", nodes=(VALUE_NODE,), **kw):
    p = {"type": "mask_mat", "material1": "a", "material2": "b", "mask": "val"}
    p.update(kw)
    return material(yi, name, {k: v for k, v in p.items() if v is not None}, nodes)


# ---- the factory ---------------------------------------------------------------------------------------------------------
def test_defaults_and_read_back():
    yi = fresh()
    two_subs(yi)
    assert mask(yi), yi.getLastError()
    m = yi.getMaskMaterial("m")
    assert (m["material1"], m["material2"]) == (0, 1)
    assert bits(m["threshold"]) == bits(F(0.5)) and (m["mask_slot"], m["n_nodes"]) == (0, 1)
    assert m["receive_shadows"] is True and m["visibility"] == 0
    assert m["bsdf_flags"] == BSDF_DIFFUSE | BSDF_REFLECT
    # threshold is read as a double and kept in a float member (material_mask.cc:137, :30-31): 0.7 narrows to float32's 0.7
    assert mask(yi, "m2", threshold=0.7, material1="b", material2="a", receive_shadows=False, visibility="shadow_only"), yi.getLastError()
    m = yi.getMaskMaterial("m2")
    assert bits(m["threshold"]) == bits(np.float32(np.float64(0.7))) and float(m["threshold"]) != 0.7
    assert (m["material1"], m["material2"], m["receive_shadows"], m["visibility"]) == (1, 0, False, 2)
    # the types are the factory's: a threshold given as an int is not read (ParamMap::getParam)
    assert mask(yi, "m3", threshold=1), yi.getLastError()
    assert bits(yi.getMaskMaterial("m3")["threshold"]) == bits(F(0.5))
    # an unknown visibility word means normal (:153-157)
    assert mask(yi, "m4", visibility="sideways"), yi.getLastError()
    assert yi.getMaskMaterial("m4")["visibility"] == 0
    assert not yi._L.yafaray_getMaskMaterial(yi._h, b"a", None) and "no such mask_mat" in yi.getLastError()
    assert not yi._L.yafaray_getMaskMaterial(yi._h, b"nope", None)


def test_the_mask_node_is_found_behind_the_nodes_it_reads():
    """the mask's own list: what `mask` reaches, in evaluation order, and nothing else of the list"""
    yi = fresh()
    two_subs(yi)
    assert texture(yi, "t0")
    nodes = [dict(type="layer", name="top", input="map", mode=0, do_color=False, do_scalar=True, color_input=False, def_val=1.0, upper_value=0.0),
             dict(type="texture_mapper", name="map", texture="t0", texco="uv"),
             dict(type="value", name="stray", scalar=0.1)]
    assert mask(yi, nodes=nodes, mask="top"), yi.getLastError()
    m = yi.getMaskMaterial("m")
    assert (m["mask_slot"], m["n_nodes"]) == (1, 2)
    t = yi.getMaterialTable()
    assert t[2, W["n_nodes"]] == 2 and t[2, W["sh_diffuse"]] == 1 and t[2, W["n_bump"]] == 0


def test_union_of_flags_and_transparency():
    yi = fresh()
    two_subs(yi, a=dict(RED, transparency=0.5), b={"type": "mirror", "color": ("color", 1.0, 1.0, 1.0, 1.0), "reflect": 0.9})
    assert mask(yi), yi.getLastError()
    f = yi.getMaskMaterial("m")["bsdf_flags"]
    assert f == BSDF_DIFFUSE | BSDF_REFLECT | BSDF_TRANSMIT | BSDF_FILTER | BSDF_SPECULAR
    t = yi.getMaterialTable()
    assert t[2, W["type"]] == MAT_MASKED and t[2, W["bsdf_flags"]] == f and t[2, W["is_transparent"]] == 1      # isTransparent: either one's (:86-89)
    two = fresh()
    two_subs(two)
    assert mask(two)
    assert two.getMaterialTable()[2, W["is_transparent"]] == 0


# ---- refusals ------------------------------------------------------------------------------------------------------------
GLOSSY = {"type": "glossy", "color": ("color", 0.9, 0.9, 0.9, 1.0), "diffuse_color": ("color", 0.5, 0.5, 0.5, 1.0), "diffuse_reflect": 0.4, "glossy_reflect": 0.6,
          "exponent": 40.0, "as_diffuse": False}
GLASS = {"type": "glass", "IOR": 1.5, "filter_color": ("color", 0.9, 1.0, 0.9, 1.0), "transmit_filter": 0.8}


def refused(yi, words, **kw):
    assert not mask(yi, **kw)
    msg = yi.getLastError()
    for w in words:
        assert w in msg, msg
    return msg


def test_refusals_name_their_cause():
    yi = fresh()
    two_subs(yi)
    refused(yi, ["mask_mat", "material1", "missing"], material1=None)
    refused(yi, ["mask_mat", "material2", "missing"], material2=None)
    refused(yi, ["material1", "nope", "names no material"], material1="nope")
    refused(yi, ["material2", "nope", "names no material"], material2="nope")
    refused(yi, ["no mask parameter"], mask=None)
    refused(yi, ["mask shader node", "other", "does not exist"], mask="other")
    refused(yi, ["does not exist"], nodes=())                                    # loadNodes of an empty list succeeds; `mask` then names nothing
    # a node list that fails to load: an unknown node type, a texture_mapper without its texture, a name twice (material_node.cc:150-205)
    refused(yi, ["node list failed to load"], nodes=(VALUE_NODE, dict(type="fractal", name="x")))
    refused(yi, ["node list failed to load"], nodes=(dict(type="texture_mapper", name="val", texture="not_there"),))
    refused(yi, ["node list failed to load"], nodes=(VALUE_NODE, VALUE_NODE))
    # the limit of 16 reachable nodes holds for the mask's own list
    chain = [dict(type="value", name="n0", scalar=0.5)]
    chain += [dict(type="layer", name=f"n{k}", input=f"n{k - 1}", mode=0, do_color=False, do_scalar=True, color_input=False, def_val=1.0, upper_value=0.0) for k in range(1, 17)]
    refused(yi, ["16 nodes"], nodes=chain, mask="n16")
    assert mask(yi, "chain16", nodes=chain[:16], mask="n15"), yi.getLastError()
    # no mask under a mask
    assert mask(yi), yi.getLastError()
    refused(yi, ["nesting", "not built"], name="mm", material1="m")
    refused(yi, ["nesting", "not built"], name="mm", material2="m")
    # nothing half made stays behind
    assert not yi._L.yafaray_getMaskMaterial(yi._h, b"mm", None)
    assert len(yi.getMaterialTable()) == 2 + (1 + 2) * 2


@pytest.mark.parametrize("partner", ["glass", "transparent shinydiffuse", "translucent shinydiffuse"])
def test_glossy_beside_a_transmitting_partner_is_refused(partner):
    """recursiveRaytrace's glossy branch reads the mask's flags, the union (integrator_montecarlo.cc:895-919)"""
    other = {"glass": GLASS, "transparent shinydiffuse": dict(RED, transparency=0.4), "translucent shinydiffuse": dict(RED, translucency=0.4)}[partner]
    for a, b in ((GLOSSY, other), (other, GLOSSY)):
        yi = fresh()
        two_subs(yi, a, b)
        refused(yi, ["glossy", "union", "integrator_montecarlo.cc:895-919"])
    # rough glass takes the reflect + transmit case alone and finds MaskMaterial without the two-direction sample
    yi = fresh()
    two_subs(yi, {"type": "rough_glass", "IOR": 1.5, "alpha": 0.3}, RED)
    refused(yi, ["rough glass", "integrator_montecarlo.cc:895-919"])
    # a glossy lobe beside opaque partners is fine, and so is glass beside a diffuse one
    for a, b in ((GLOSSY, RED), (GLOSSY, {"type": "mirror"}), (GLASS, RED), (dict(GLOSSY, as_diffuse=True), GLASS)):
        yi = fresh()
        two_subs(yi, a, b)
        assert mask(yi), yi.getLastError()


def test_out_of_scope_message_lists_what_is_in_scope():
    yi = fresh()
    assert not material(yi, "x", {"type": "blend_mat"})
    msg = yi.getLastError()
    assert "scope" in msg and "blend_mat" in msg
    for accepted in ("shinydiffusemat", "glossy", "coated_glossy", "glass", "rough_glass", "mirror", "light_mat", "mask_mat"):
        assert accepted in msg, msg


# ---- the material table --------------------------------------------------------------------------------------------------
def test_clones_carry_the_masks_material_level_fields():
    """receive_shadows and visibility are the mask's; a sub-material's additionaldepth, flat_material, transparent bias and absorption
    are read off the mask in the reference (which has none) and do not show in the clones; the sub-materials' own records keep them"""
    yi = fresh()
    a = dict(RED, additionaldepth=3, flat_material=True, transparency=0.3, transparentbias_factor=0.25, transparentbias_multiply_raydepth=True, receive_shadows=False)
    b = dict(GLASS, absorption=("color", 0.5, 0.7, 0.9, 1.0), absorption_dist=2.0, additionaldepth=2)
    two_subs(yi, a, b)
    assert mask(yi, visibility="no_shadows"), yi.getLastError()
    t = yi.getMaterialTable()
    assert len(t) == 5 and list(t[2, W["c_index"]:W["c_index"] + 2]) == [3, 4]
    f32 = t.view(np.float32)
    # the originals
    assert t[0, W["additional_depth"]] == 3 and t[0, W["flat"]] == 1 and f32[0, W["transp_bias_factor"]] == F(0.25) and t[0, W["transp_bias_mult"]] == 1
    assert t[0, W["receive_shadows"]] == 0
    assert t[1, W["additional_depth"]] == 2 and t[1, W["has_vol_i"]] == 1 and (f32[1, W["beer_sigma"]:W["beer_sigma"] + 3] > 0).all()
    assert t[1, W["bsdf_flags"]] & BSDF_VOLUMETRIC
    for clone, orig in ((3, 0), (4, 1)):
        c = t[clone]
        assert c[W["type"]] == t[orig, W["type"]] and c[W["bsdf_flags"]] == t[orig, W["bsdf_flags"]]
        assert c[W["receive_shadows"]] == 1 and c[W["visibility"]] == 1                     # the mask's
        assert c[W["additional_depth"]] == 0 and f32[clone, W["transp_bias_factor"]] == 0 and c[W["transp_bias_mult"]] == 0
        assert c[W["has_vol_i"]] == 0 and (f32[clone, W["beer_sigma"]:W["beer_sigma"] + 3] == 0).all()
        assert c[W["flat"]] & 1 == 0                                                        # isFlat() is the mask's: false
        # everything else is the sub-material's record, word for word
        touched = [W["receive_shadows"], W["visibility"], W["flat"], W["additional_depth"], W["transp_bias_factor"], W["transp_bias_mult"], W["has_vol_i"],
                   W["beer_sigma"], W["beer_sigma"] + 1, W["beer_sigma"] + 2]
        keep = np.setdiff1d(np.arange(Interface.MATERIAL_WORDS), touched)
        assert np.array_equal(c[keep], t[orig, keep])
    # ShinyDiffuseMaterial::eval's own flat_material_ test (material_shiny_diffuse.cc:275) stays the sub-material's: flat 2
    assert t[3, W["flat"]] == 2 and t[4, W["flat"]] == 0
    assert t[2, W["flat"]] == 0 and t[2, W["additional_depth"]] == 0 and t[2, W["has_vol_i"]] == 0


def test_clones_share_the_node_ranges_of_their_sub_materials():
    yi = fresh()
    assert texture(yi, "t0")
    noded = dict(RED, diffuse_shader="d", bump_shader="b")
    nodes = [dict(type="texture_mapper", name="d", texture="t0", texco="uv"), dict(type="texture_mapper", name="b", texture="t0", texco="uv", bump_strength=1.0)]
    assert material(yi, "a", noded, nodes), yi.getLastError()
    assert material(yi, "b", BLUE)
    assert mask(yi), yi.getLastError()
    t = yi.getMaterialTable()
    assert (t[0, W["node_first"]], t[0, W["n_nodes"]], t[0, W["bump_first"]], t[0, W["n_bump"]]) == (0, 1, 1, 1)
    assert (t[2, W["node_first"]], t[2, W["n_nodes"]]) == (2, 1)                            # the mask's own node, behind material a's two
    for w in ("node_first", "n_nodes", "bump_first", "n_bump"):
        assert t[3, W[w]] == t[0, W[w]] and t[4, W[w]] == t[1, W[w]]


# ---- XML -----------------------------------------------------------------------------------------------------------------
PAINT = """<material name="paint"><type sval="shinydiffusemat"/><color r="0.8" g="0.1" b="0.1" a="1"/><diffuse_reflect fval="1"/></material>
"""
METAL = """<material name="metal"><type sval="glossy"/><color r="0.9" g="0.9" b="0.9" a="1"/><diffuse_color r="0.5" g="0.5" b="0.5" a="1"/>
  <diffuse_reflect fval="0.4"/><glossy_reflect fval="0.6"/><exponent fval="50"/><as_diffuse bval="true"/></material>
"""
LABEL = """<material name="label"><type sval="mask_mat"/><material1 sval="metal"/><material2 sval="paint"/><mask sval="mask_layer"/><threshold fval="0.7"/>
  <receive_shadows bval="false"/>
  <list_element><element sval="shader_node"/><name sval="mask_layer"/><type sval="layer"/><input sval="map"/><mode ival="0"/>
    <do_color bval="false"/><do_scalar bval="true"/><color_input bval="false"/><def_val fval="1"/><upper_value fval="0"/></list_element>
  <list_element><element sval="shader_node"/><name sval="map"/><type sval="texture_mapper"/><texture sval="decal"/><texco sval="uv"/></list_element>
</material>
"""
XML = """<?xml version="1.0"?>
<scene type="triangle">
<texture name="decal"><type sval="image"/><filename sval="%(image)s"/><interpolate sval="none"/></texture>
%(materials)s<camera name="cam"><type sval="perspective"/><from x="0" y="-3" z="0"/><to x="0" y="0" z="0"/><up x="0" y="-3" z="1"/>
  <resx ival="16"/><resy ival="16"/><focal fval="1.2"/></camera>
<integrator name="default"><type sval="directlighting"/></integrator>
<integrator name="volintegr"><type sval="none"/></integrator>
<mesh id="1" vertices="4" faces="2" has_orco="false" has_uv="true" type="0">
  <p x="-1" y="0" z="-1"/><p x="1" y="0" z="-1"/><p x="1" y="0" z="1"/><p x="-1" y="0" z="1"/>
  <uv u="0" v="0"/><uv u="1" v="0"/><uv u="1" v="1"/><uv u="0" v="1"/>
  <set_material sval="label"/><f a="0" b="1" c="2" uv_a="0" uv_b="1" uv_c="2"/><f a="0" b="2" c="3" uv_a="0" uv_b="2" uv_c="3"/>
</mesh>
<render><camera_name sval="cam"/><integrator_name sval="default"/><volintegrator_name sval="volintegr"/>
  <width ival="16"/><height ival="16"/><AA_passes ival="1"/><AA_minsamples ival="1"/>
  <AA_pixelwidth fval="1"/><filter_type sval="box"/><tile_size ival="8"/></render>
</scene>
"""
IMAGE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "test01_tex.png")


def test_xml_scene_with_a_mask_defined_after_its_sub_materials(tmp_path):
    """strings and a <list_element> list: the grammar needs nothing new.  prepareRender then flattens the scene and passes every check
    of the device scene's creation; without a GPU the only thing left to fail is the first device allocation"""
    p = tmp_path / "mask.xml"
    p.write_text(XML % {"image": IMAGE, "materials": PAINT + METAL + LABEL})
    yi = Interface(strict=False)
    assert yi.loadXml(str(p)), yi.getLastError()
    m = yi.getMaskMaterial("label")
    assert (m["material1"], m["material2"]) == (1, 0) and bits(m["threshold"]) == bits(np.float32(np.float64(0.7)))
    assert (m["mask_slot"], m["n_nodes"], m["receive_shadows"]) == (1, 2, False)
    t = yi.getMaterialTable()
    assert len(t) == 5 and t[2, W["type"]] == MAT_MASKED and list(t[2, W["c_index"]:W["c_index"] + 2]) == [3, 4]
    ok = yi.prepareRender()
    assert ok or yi.getLastError().startswith("scene upload: hip"), yi.getLastError()


def test_xml_mask_before_its_sub_materials_is_refused(tmp_path):
    """the reference's factory looks its sub-materials up when it runs (material_mask.cc:143-146): one defined later does not exist yet"""
    p = tmp_path / "mask_first.xml"
    p.write_text(XML % {"image": IMAGE, "materials": METAL + LABEL + PAINT})
    yi = Interface(strict=False)
    assert not yi.loadXml(str(p))
    assert "label" in yi.getLastError() and "material2" in yi.getLastError() and "names no material" in yi.getLastError(), yi.getLastError()
