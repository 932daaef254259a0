"""Ambient occlusion on the host: the four parameters DirectLightIntegrator::factory (integrator_direct_light.cc:200-207, :220-223) and
PathIntegrator::factory (integrator_path_tracer.cc:355-358, :375-378) read, their defaults and types as yafaray_getIntegratorAO hands
them back, the refusals, the XML loader.  No GPU needed."""
import os

import numpy as np
import pytest

from libyafaray_amd import Interface
from tests.test_lights_host import F, bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def fresh():
    yi = Interface(strict=False)
    yi.startScene(0)
    return yi


def integrator(yi, name, params):
    yi.paramsClearAll()
    yi.paramsSet(params)
    return yi.createIntegrator(name)


@pytest.mark.parametrize("kind", ["directlighting", "pathtracing"])
def test_defaults_and_parsed_values(kind):
    yi = fresh()
    assert integrator(yi, "a", {"type": kind}), yi.getLastError()
    ao = yi.getIntegratorAO("a")
    assert (ao["do_AO"], ao["AO_samples"]) == (False, 32) and ao["AO_distance"] == F(1) and np.array_equal(ao["AO_color"], np.ones(3, np.float32))
    # every parameter; pathtracing takes do_AO too (it only feeds render passes the GPU path does not have)
    assert integrator(yi, "b", {"type": kind, "do_AO": True, "AO_samples": 7, "AO_distance": 0.3, "AO_color": ("color", 0.25, 0.5, 0.75, 1.0)}), yi.getLastError()
    ao = yi.getIntegratorAO("b")
    assert (ao["do_AO"], ao["AO_samples"]) == (True, 7)
    # AO_distance is read as a double and kept as a float (ao_dist_): 0.3 narrows to float32's 0.3
    assert bits(ao["AO_distance"]) == bits(np.float32(np.float64(0.3))) and float(ao["AO_distance"]) != 0.3
    assert np.array_equal(bits(ao["AO_color"]), bits(np.array([0.25, 0.5, 0.75], np.float32)))
    # the types are the factory's: an AO_samples given as a float, an AO_distance given as an int are not read (ParamMap::getParam)
    assert integrator(yi, "c", {"type": kind, "do_AO": True, "AO_samples": 7.0, "AO_distance": 2}), yi.getLastError()
    ao = yi.getIntegratorAO("c")
    assert ao["AO_samples"] == 32 and ao["AO_distance"] == F(1)
    assert not yi._L.yafaray_getIntegratorAO(yi._h, b"nope", None, None, None, None)
    assert "no such integrator" in yi.getLastError()


def test_do_ao_false_leaves_everything_as_it_was():
    """what exporters have been sending all along (do_AO false beside the other three) is accepted and only recorded; sample counts the
    estimate could not use are no reason to refuse an integrator that does not run it"""
    yi = fresh()
    assert integrator(yi, "a", {"type": "directlighting", "do_AO": False, "AO_samples": 0, "AO_distance": 1.0, "AO_color": ("color", 0.9, 0.9, 0.9, 1.0)}), yi.getLastError()
    ao = yi.getIntegratorAO("a")
    assert ao["do_AO"] is False and ao["AO_samples"] == 0
    assert integrator(yi, "b", {"type": "pathtracing", "do_AO": False, "AO_samples": 100000}), yi.getLastError()
    # the other refusals of the factory still stand
    assert not integrator(yi, "c", {"type": "directlighting", "caustics": True})
    assert "photon" in yi.getLastError()


@pytest.mark.parametrize("kind", ["directlighting", "pathtracing"])
def test_sample_count_refusals_name_the_parameter(kind):
    yi = fresh()
    for n in (0, -3):
        assert not integrator(yi, "a", {"type": kind, "do_AO": True, "AO_samples": n})
        assert "AO_samples" in yi.getLastError() and "at least 1" in yi.getLastError()
    assert not integrator(yi, "a", {"type": kind, "do_AO": True, "AO_samples": 4096})
    assert "AO_samples" in yi.getLastError() and "4095" in yi.getLastError()
    for n in (1, 4095):
        assert integrator(yi, "a", {"type": kind, "do_AO": True, "AO_samples": n}), yi.getLastError()


def scene_with_lights(n_lights, integ):
    """a one-triangle scene with n_lights point lights, up to (not including) prepareRender"""
    yi = fresh()
    yi.paramsClearAll()
    yi.paramsSet({"type": "shinydiffusemat", "color": ("color", 0.8, 0.8, 0.8, 1.0)})
    mat = yi.createMaterial("white")
    for k in range(n_lights):
        yi.paramsClearAll()
        yi.paramsSet({"type": "pointlight", "from": (0.01 * k, 0.0, 2.0), "power": 1.0})
        assert yi.createLight(f"L{k}")
    yi.paramsClearAll()
    yi.paramsSet({"type": "perspective", "from": (0.0, -3.0, 0.0), "to": (0.0, 0.0, 0.0), "up": (0.0, -3.0, 1.0), "resx": 8, "resy": 8})
    assert yi.createCamera("cam")
    assert integrator(yi, "default", integ), yi.getLastError()
    assert integrator(yi, "volintegr", {"type": "none"})
    yi.startGeometry()
    yi.startTriMesh(yi.getNextFreeId(), 3, 1, False, False, 0)
    for v in ((-1.0, 0.0, -1.0), (1.0, 0.0, -1.0), (0.0, 0.0, 1.0)):
        yi.addVertex(*v)
    yi.addTriangle(0, 1, 2, mat)
    yi.endTriMesh()
    yi.endGeometry()
    yi.paramsClearAll()
    yi.paramsSet({"camera_name": "cam", "integrator_name": "default", "volintegrator_name": "volintegr", "width": 8, "height": 8})
    return yi


def test_prepare_render_refuses_ao_beside_more_than_254_lights():
    yi = scene_with_lights(255, {"type": "directlighting", "do_AO": True, "AO_samples": 4})
    assert not yi.prepareRender()
    assert "do_AO" in yi.getLastError() and "254" in yi.getLastError()


XML = """<?xml version="1.0"?>
<scene type="triangle">
<material name="white"><type sval="shinydiffusemat"/><color r="0.8" g="0.8" b="0.8" a="1"/><diffuse_reflect fval="1"/></material>
<camera name="cam"><type sval="perspective"/><from x="0" y="-3" z="0"/><to x="0" y="0" z="0"/><up x="0" y="-3" z="1"/>
  <resx ival="16"/><resy ival="16"/><focal fval="1.2"/></camera>
<integrator name="default"><type sval="directlighting"/>
  <AO_color r="0.5" g="0.25" b="0.125" a="1"/><AO_distance fval="0.75"/><AO_samples ival="5"/><do_AO bval="true"/></integrator>
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


def test_xml_scene_with_ao_loads_with_its_values(tmp_path):
    p = tmp_path / "ao.xml"
    p.write_text(XML)
    yi = Interface(strict=False)
    assert yi.loadXml(str(p)), yi.getLastError()
    ao = yi.getIntegratorAO("default")
    assert (ao["do_AO"], ao["AO_samples"]) == (True, 5) and ao["AO_distance"] == F(0.75)
    assert np.array_equal(bits(ao["AO_color"]), bits(np.array([0.5, 0.25, 0.125], np.float32)))


@pytest.mark.parametrize("name", ["test01_dl.xml", "test01_pt.xml", "test01_tex.xml"])
def test_golden_xml_scenes_carry_their_ao_parameters(name):
    """the exporter's scenes send all four with do_AO false: they load as before and the values are there"""
    yi = Interface(strict=False)
    assert yi.loadXml(os.path.join(ROOT, "tests", "golden", name)), yi.getLastError()
    ao = yi.getIntegratorAO("default")
    assert (ao["do_AO"], ao["AO_samples"]) == (False, 32) and ao["AO_distance"] == F(1)
    assert (ao["AO_color"] > 0.5).all() and (ao["AO_color"] <= 1).all()
