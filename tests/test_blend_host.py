"""The blend material on the host: BlendMaterial::factory and constructor (material_blend.cc:464-544, :38-49) as createMaterial restates
them — the parameters and defaults as yafaray_getBlendMaterial hands them back, every refusal with its cause, the XML loader — and the
material table the device scene gets (yafaray_getMaterialTable): the blend's record and the hidden clones of the two sub-materials its
functions run on.  No GPU needed."""
import numpy as np
import pytest

from libyafaray_amd import Interface
from tests.test_lights_host import F, bits
from tests.test_mask_host import BLUE, GLASS, GLOSSY, IMAGE, METAL, PAINT, RED, VALUE_NODE, W, XML, fresh, material, texture, two_subs

MAT_SHINYDIFFUSE, MAT_GLASS, MAT_MASKED, MAT_BLEND = 0, 3, 7, 8
BSDF_SPECULAR, BSDF_GLOSSY, BSDF_DIFFUSE, BSDF_REFLECT, BSDF_TRANSMIT, BSDF_FILTER, BSDF_EMIT, BSDF_VOLUMETRIC = 0x1, 0x2, 0x4, 0x10, 0x20, 0x40, 0x80, 0x100
MIRROR = {"type": "mirror", "color": ("color", 1.0, 1.0, 1.0, 1.0), "reflect": 0.9}


def blend(yi, name="m", nodes=(), **kw):
    p = {"type": "blend_mat", "material1": "a", "material2": "b"}
    p.update(kw)
    return material(yi, name, {k: v for k, v in p.items() if v is not None}, nodes)


def refused(yi, words, **kw):
    assert not blend(yi, **kw)
    msg = yi.getLastError()
    for w in words:
        assert w in msg, msg
    return msg


# ---- the factory ---------------------------------------------------------------------------------------------------------
def test_defaults_and_read_back():
    yi = fresh()
    two_subs(yi)
    assert blend(yi), yi.getLastError()
    m = yi.getBlendMaterial("m")
    assert (m["material1"], m["material2"]) == (0, 1)
    assert bits(m["blend_value"]) == bits(F(0.5))                                             # :468
    assert (m["node_driven"], m["mask_slot"], m["n_nodes"]) == (False, -1, 0)                 # no `mask`: the constant blends, recalc_blend_ false
    assert m["receive_shadows"] is True and m["visibility"] == 0
    assert m["bsdf_flags"] == BSDF_DIFFUSE | BSDF_REFLECT and m["additional_depth"] == 0
    # blend_value is read as a double and kept in a float member (:468, :483, :45): 0.3 narrows to float32's 0.3
    assert blend(yi, "m2", blend_value=0.3, material1="b", material2="a", receive_shadows=False, visibility="shadow_only", mat_pass_index=3, samplingfactor=2.0), yi.getLastError()
    m = yi.getBlendMaterial("m2")
    assert bits(m["blend_value"]) == bits(np.float32(np.float64(0.3))) and float(m["blend_value"]) != 0.3
    assert (m["material1"], m["material2"], m["receive_shadows"], m["visibility"]) == (1, 0, False, 2)
    # it is not clamped: getBlendVal clamps ival alone (:74)
    assert blend(yi, "m3", blend_value=1.4), yi.getLastError()
    assert bits(yi.getBlendMaterial("m3")["blend_value"]) == bits(np.float32(np.float64(1.4)))
    # the types are the factory's: a blend_value given as an int is not read (ParamMap::getParam)
    assert blend(yi, "m4", blend_value=1), yi.getLastError()
    assert bits(yi.getBlendMaterial("m4")["blend_value"]) == bits(F(0.5))
    for k, (word, v) in enumerate((("normal", 0), ("no_shadows", 1), ("shadow_only", 2), ("invisible", 3), ("sideways", 0))):      # :495-499
        assert blend(yi, f"v{k}", visibility=word), yi.getLastError()
        assert yi.getBlendMaterial(f"v{k}")["visibility"] == v
    assert not yi._L.yafaray_getBlendMaterial(yi._h, b"a", None) and "no such blend_mat" in yi.getLastError()
    assert not yi._L.yafaray_getBlendMaterial(yi._h, b"nope", None)


def test_a_node_drives_the_blend_when_mask_names_one():
    """the blend's own list: what `mask` reaches, in evaluation order, and nothing else of the list (:515-541)"""
    yi = fresh()
    two_subs(yi)
    assert texture(yi, "t0")
    nodes = [dict(type="layer", name="top", input="map", mode=0, do_color=False, do_scalar=True, color_input=False, def_val=1.0, upper_value=0.0),
             dict(type="texture_mapper", name="map", texture="t0", texco="uv"),
             dict(type="value", name="stray", scalar=0.1)]
    assert blend(yi, nodes=nodes, mask="top", blend_value=0.25), yi.getLastError()
    m = yi.getBlendMaterial("m")
    assert (m["node_driven"], m["mask_slot"], m["n_nodes"]) == (True, 1, 2)
    assert bits(m["blend_value"]) == bits(F(0.25))                                            # kept: getVolumeHandler reads the constant (:457)
    t = yi.getMaterialTable()
    assert t[2, W["type"]] == MAT_BLEND and t[2, W["n_nodes"]] == 2 and t[2, W["sh_diffuse"]] == 1 and t[2, W["n_bump"]] == 0
    # nodes without `mask`: they load and none is reached
    assert blend(yi, "m2", nodes=nodes), yi.getLastError()
    m = yi.getBlendMaterial("m2")
    assert (m["node_driven"], m["mask_slot"], m["n_nodes"]) == (False, -1, 0)


def test_union_of_flags_depth_and_transparency():
    yi = fresh()
    two_subs(yi, a=dict(RED, transparency=0.5, additionaldepth=2), b=dict(MIRROR))
    assert material(yi, "c", dict(GLOSSY, additionaldepth=5)), yi.getLastError()
    assert material(yi, "l", {"type": "light_mat", "color": ("color", 1.0, 1.0, 1.0, 1.0), "power": 2.0})
    assert blend(yi), yi.getLastError()
    m = yi.getBlendMaterial("m")
    assert m["bsdf_flags"] == BSDF_DIFFUSE | BSDF_REFLECT | BSDF_TRANSMIT | BSDF_FILTER | BSDF_SPECULAR       # :42
    assert m["additional_depth"] == 2                                                                       # :48: the larger one
    t = yi.getMaterialTable()
    assert t[4, W["type"]] == MAT_BLEND and t[4, W["bsdf_flags"]] == m["bsdf_flags"] and t[4, W["is_transparent"]] == 1      # :332-335: either one's
    assert t[4, W["additional_depth"]] == 2 and t[4, W["flat"]] == 0
    assert blend(yi, "m2", material1="b", material2="c"), yi.getLastError()
    m = yi.getBlendMaterial("m2")
    assert m["bsdf_flags"] == BSDF_SPECULAR | BSDF_GLOSSY | BSDF_DIFFUSE | BSDF_REFLECT and m["additional_depth"] == 5
    assert blend(yi, "m3", material1="l", material2="b"), yi.getLastError()
    assert yi.getBlendMaterial("m3")["bsdf_flags"] == BSDF_EMIT | BSDF_SPECULAR
    t = yi.getMaterialTable()
    assert t[5, W["is_transparent"]] == 0 and t[6, W["is_transparent"]] == 0


# ---- refusals ------------------------------------------------------------------------------------------------------------
def test_the_bare_call_stays_refused_as_the_reference_refuses_it():
    yi = fresh()
    assert not material(yi, "x", {"type": "blend_mat"})
    msg = yi.getLastError()
    assert "scope" in msg and "blend_mat" in msg and "material1" in msg and "missing" in msg and "material_blend.cc:479" in msg
    for accepted in ("shinydiffusemat", "glossy", "coated_glossy", "glass", "rough_glass", "mirror", "light_mat", "mask_mat", "blend_mat"):
        assert accepted in msg, msg
    # a type that is out of scope now lists blend_mat among the accepted ones
    assert not material(yi, "y", {"type": "translucent"})
    assert "scope" in yi.getLastError() and "blend_mat" in yi.getLastError()


def test_refusals_name_their_cause():
    yi = fresh()
    two_subs(yi)
    refused(yi, ["blend_mat", "material1", "missing"], material1=None)
    refused(yi, ["blend_mat", "material2", "missing"], material2=None)
    refused(yi, ["material1", "nope", "names no material"], material1="nope")
    refused(yi, ["material2", "nope", "names no material"], material2="nope")
    refused(yi, ["mask shader node", "other", "does not exist"], nodes=(VALUE_NODE,), mask="other")
    refused(yi, ["does not exist"], mask="val")                                  # loadNodes of an empty list succeeds; `mask` then names nothing
    # a node list that fails to load — with or without `mask`: an unknown node type, a texture_mapper without its texture, a name twice
    refused(yi, ["node list failed to load"], nodes=(VALUE_NODE, dict(type="fractal", name="x")), mask="val")
    refused(yi, ["node list failed to load"], nodes=(VALUE_NODE, dict(type="fractal", name="x")))
    refused(yi, ["node list failed to load"], nodes=(dict(type="texture_mapper", name="val", texture="not_there"),), mask="val")
    refused(yi, ["node list failed to load"], nodes=(VALUE_NODE, VALUE_NODE), mask="val")
    # the limit of 16 reachable nodes holds for the blend's own list
    chain = [dict(type="value", name="n0", scalar=0.5)]
    chain += [dict(type="layer", name=f"n{k}", input=f"n{k - 1}", mode=0, do_color=False, do_scalar=True, color_input=False, def_val=1.0, upper_value=0.0) for k in range(1, 17)]
    refused(yi, ["16 nodes"], nodes=chain, mask="n16")
    assert blend(yi, "chain16", nodes=chain[:16], mask="n15"), yi.getLastError()
    # wireframe shading, as for every material
    refused(yi, ["blend_mat", "wireframe"], wireframe_amount=0.5)
    assert blend(yi, "wire0", wireframe_amount=0.0), yi.getLastError()
    # no blend under a blend, no mask under a blend, no blend under a mask
    assert blend(yi), yi.getLastError()
    assert material(yi, "k", {"type": "mask_mat", "material1": "a", "material2": "b", "mask": "val"}, (VALUE_NODE,)), yi.getLastError()
    for sub, kind in (("m", "blend_mat"), ("k", "mask_mat")):
        refused(yi, [kind, "nesting", "not built"], name="mm", material1=sub)
        refused(yi, [kind, "nesting", "not built"], name="mm", material2=sub)
    for key in ("material1", "material2"):
        p = {"type": "mask_mat", "material1": "a", "material2": "b", "mask": "val"}
        p[key] = "m"
        assert not material(yi, "km", p, (VALUE_NODE,))
        assert "blend_mat" in yi.getLastError() and "under a mask" in yi.getLastError() and "not built" in yi.getLastError(), yi.getLastError()
    # nothing half made stays behind
    assert not yi._L.yafaray_getBlendMaterial(yi._h, b"mm", None)


def test_a_sub_material_with_a_bump_shader_is_refused():
    yi = fresh()
    assert texture(yi, "t0")
    bumped = dict(RED, bump_shader="b")
    nodes = [dict(type="texture_mapper", name="b", texture="t0", texco="uv", bump_strength=1.0)]
    assert material(yi, "a", bumped, nodes), yi.getLastError()
    assert material(yi, "b", BLUE)
    refused(yi, ["material1", "bump shader", "blendSurfacePoints__", "surface.cc:137-151"])
    refused(yi, ["material2", "bump shader"], material1="b", material2="a")


@pytest.mark.parametrize("partner", ["glass", "transparent shinydiffuse", "translucent shinydiffuse"])
def test_glossy_beside_a_transmitting_partner_is_refused(partner):
    """recursiveRaytrace's glossy branch reads the blend's flags, the union (integrator_montecarlo.cc:895-919), and would call the
    two-direction sample (material_blend.cc:216-236), which is not restated: refused as under a mask, in the same words"""
    other = {"glass": GLASS, "transparent shinydiffuse": dict(RED, transparency=0.4), "translucent shinydiffuse": dict(RED, translucency=0.4)}[partner]
    for a, b in ((GLOSSY, other), (other, GLOSSY)):
        yi = fresh()
        two_subs(yi, a, b)
        refused(yi, ["glossy", "union", "integrator_montecarlo.cc:895-919"])
    yi = fresh()
    two_subs(yi, {"type": "rough_glass", "IOR": 1.5, "alpha": 0.3}, RED)
    refused(yi, ["rough glass", "integrator_montecarlo.cc:895-919"])
    for a, b in ((GLOSSY, RED), (GLOSSY, MIRROR), (GLASS, RED), (dict(GLOSSY, as_diffuse=True), GLASS)):
        yi = fresh()
        two_subs(yi, a, b)
        assert blend(yi), yi.getLastError()


# ---- the material table --------------------------------------------------------------------------------------------------
def test_clones_are_the_sub_materials_and_the_blend_carries_the_material_level_fields():
    yi = fresh()
    a = dict(RED, additionaldepth=3, flat_material=True, transparency=0.3, transparentbias_factor=0.25, transparentbias_multiply_raydepth=True, receive_shadows=False)
    b = dict(GLASS, absorption=("color", 0.5, 0.7, 0.9, 1.0), absorption_dist=2.0, additionaldepth=2)
    two_subs(yi, a, b)
    assert blend(yi, visibility="no_shadows", blend_value=0.8), yi.getLastError()
    t = yi.getMaterialTable()
    assert len(t) == 5 and list(t[2, W["c_index"]:W["c_index"] + 2]) == [3, 4]
    f32 = t.view(np.float32)
    for clone, orig in ((3, 0), (4, 1)):
        # the sub-material's record, word for word, but for flat: isFlat() is the blend's, ShinyDiffuseMaterial::eval's own test stays (2)
        keep = np.setdiff1d(np.arange(Interface.MATERIAL_WORDS), [W["flat"]])
        assert np.array_equal(t[clone, keep], t[orig, keep])
    assert t[3, W["flat"]] == 2 and t[4, W["flat"]] == 0
    # the blend's own record: what the integrators read off sp.material_
    r = t[2]
    assert r[W["type"]] == MAT_BLEND and r[W["visibility"]] == 1 and r[W["receive_shadows"]] == 1 and r[W["flat"]] == 0
    assert r[W["additional_depth"]] == 3 and r[W["is_transparent"]] == 1
    assert r[W["bsdf_flags"]] == t[0, W["bsdf_flags"]] | t[1, W["bsdf_flags"]] and r[W["bsdf_flags"]] & BSDF_VOLUMETRIC
    assert f32[2, W["transp_bias_factor"]] == 0 and r[W["transp_bias_mult"]] == 0           # Material's defaults: the factory reads neither
    assert bits(f32[2, W["transmit_filter"]]) == bits(np.float32(np.float64(0.8)))
    # getVolumeHandler (:450-462): only the glass has one, so it is the blend's whatever the value
    sig = slice(W["beer_sigma"], W["beer_sigma"] + 3)
    assert r[W["has_vol_i"]] == 1 and np.array_equal(t[2, sig], t[1, sig])


def test_volume_handler_is_chosen_by_the_constant():
    """both absorb: material1's at blend_val_ <= 0.5f, material2's above (:455-459) — the constant, also under a node"""
    ga = dict(GLASS, absorption=("color", 0.5, 0.7, 0.9, 1.0), absorption_dist=2.0)
    gb = dict(GLASS, absorption=("color", 0.9, 0.4, 0.6, 1.0), absorption_dist=1.0)
    for value, pick in ((0.5, 0), (0.2, 0), (0.5000001, 1), (1.0, 1)):
        yi = fresh()
        two_subs(yi, ga, gb)
        assert blend(yi, blend_value=value, nodes=(VALUE_NODE,), mask="val"), yi.getLastError()
        t = yi.getMaterialTable()
        sig = slice(W["beer_sigma"], W["beer_sigma"] + 3)
        assert not np.array_equal(t[0, sig], t[1, sig])
        assert t[2, W["has_vol_i"]] == 1 and np.array_equal(t[2, sig], t[pick, sig]), value
    yi = fresh()
    two_subs(yi)
    assert blend(yi)
    assert yi.getMaterialTable()[2, W["has_vol_i"]] == 0


def test_clones_share_the_node_ranges_of_their_sub_materials():
    yi = fresh()
    assert texture(yi, "t0")
    nodes = [dict(type="texture_mapper", name="d", texture="t0", texco="uv")]
    assert material(yi, "a", dict(RED, diffuse_shader="d"), nodes), yi.getLastError()
    assert material(yi, "b", dict(GLOSSY, diffuse_shader="d"), nodes), yi.getLastError()
    assert blend(yi, nodes=(VALUE_NODE,), mask="val"), yi.getLastError()
    t = yi.getMaterialTable()
    assert (t[0, W["node_first"]], t[0, W["n_nodes"]]) == (0, 1) and (t[1, W["node_first"]], t[1, W["n_nodes"]]) == (1, 1)
    assert (t[2, W["node_first"]], t[2, W["n_nodes"]], t[2, W["sh_diffuse"]]) == (2, 1, 0)      # the blend's own node, behind its sub-materials'
    for w in ("node_first", "n_nodes", "bump_first", "n_bump"):
        assert t[3, W[w]] == t[0, W[w]] and t[4, W[w]] == t[1, W[w]]
    # masks and blends side by side: every one gets its own two clones, in creation order
    assert material(yi, "k", {"type": "mask_mat", "material1": "a", "material2": "b", "mask": "val"}, (VALUE_NODE,)), yi.getLastError()
    assert blend(yi, "m2", material1="b", material2="a")
    t = yi.getMaterialTable()
    assert len(t) == 5 + 6
    assert [list(t[i, W["c_index"]:W["c_index"] + 2]) for i in (2, 3, 4)] == [[5, 6], [7, 8], [9, 10]]
    assert [t[i, W["type"]] for i in (2, 3, 4)] == [MAT_BLEND, MAT_MASKED, MAT_BLEND]


# ---- XML -----------------------------------------------------------------------------------------------------------------
DIRT = """<material name="label"><type sval="blend_mat"/><material1 sval="metal"/><material2 sval="paint"/><mask sval="mask_layer"/><blend_value fval="0.7"/>
  <receive_shadows bval="false"/>
  <list_element><element sval="shader_node"/><name sval="mask_layer"/><type sval="layer"/><input sval="map"/><mode ival="0"/>
    <do_color bval="false"/><do_scalar bval="true"/><color_input bval="false"/><def_val fval="1"/><upper_value fval="0"/></list_element>
  <list_element><element sval="shader_node"/><name sval="map"/><type sval="texture_mapper"/><texture sval="decal"/><texco sval="uv"/></list_element>
</material>
"""


def test_xml_scene_with_a_node_driven_blend(tmp_path):
    """strings, a float and a <list_element> list: the grammar needs nothing new.  prepareRender then flattens the scene and passes every
    check of the device scene's creation; without a GPU the only thing left to fail is the first device allocation"""
    p = tmp_path / "blend.xml"
    p.write_text(XML % {"image": IMAGE, "materials": PAINT + METAL + DIRT})
    yi = Interface(strict=False)
    assert yi.loadXml(str(p)), yi.getLastError()
    m = yi.getBlendMaterial("label")
    assert (m["material1"], m["material2"]) == (1, 0) and bits(m["blend_value"]) == bits(np.float32(np.float64(0.7)))
    assert (m["node_driven"], m["mask_slot"], m["n_nodes"], m["receive_shadows"]) == (True, 1, 2, False)
    t = yi.getMaterialTable()
    assert len(t) == 5 and t[2, W["type"]] == MAT_BLEND and list(t[2, W["c_index"]:W["c_index"] + 2]) == [3, 4]
    ok = yi.prepareRender()
    assert ok or yi.getLastError().startswith("scene upload: hip"), yi.getLastError()


def test_xml_blend_before_its_sub_materials_is_refused(tmp_path):
    """the reference's factory looks its sub-materials up when it runs (material_blend.cc:480-482): one defined later does not exist yet"""
    p = tmp_path / "blend_first.xml"
    p.write_text(XML % {"image": IMAGE, "materials": METAL + DIRT + PAINT})
    yi = Interface(strict=False)
    assert not yi.loadXml(str(p))
    assert "label" in yi.getLastError() and "material2" in yi.getLastError() and "names no material" in yi.getLastError(), yi.getLastError()
