"""Mesh instances on the host: Scene::addInstance (scene.cc:1105-1130) as yafaray_addInstance restates it — what it stores as
yafaray_getInstances hands it back (own id, base, matrix, the four flags TriangleObjectInstance copies from its base when it is made,
object_geom.cc:104-121), every refusal with its cause, and the <instance> / <transform> elements of the XML loader
(import_xml.cc:450-460, :640-671).  No GPU needed."""
import numpy as np

from libyafaray_amd import Interface

RED = {"type": "shinydiffusemat", "color": ("color", 0.8, 0.1, 0.1, 1.0), "diffuse_reflect": 1.0}
BASEMESH = 0x0200

M_GENERAL = np.array([[0.5, -0.25, 0.125, 1.5], [0.75, 2.0, -1.0, -3.25], [0.0, 1.0, 0.5, 0.1], [0.0, 0.0, 0.0, 1.0]], np.float32)


def fresh():
    yi = Interface(strict=False)
    yi.startScene(0)
    return yi


def material(yi, name="red", params=RED):
    yi.paramsClearAll()
    yi.paramsSet(params)
    mat = yi.createMaterial(name)
    assert mat, yi.getLastError()
    return mat


def quad(yi, mid, mat, type_=0, has_orco=False, has_uv=False):
    """a unit square of two triangles under id `mid`; the geometry block is left open for smoothMesh"""
    assert yi.startTriMesh(mid, 4, 2, has_orco, has_uv, type_), yi.getLastError()
    for p in [(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0)]:
        if has_orco:
            yi.addVertexWithOrco(*p, *[2.0 * c for c in p])
        else:
            yi.addVertex(*p)
    if has_uv:
        for uv in [(0, 0), (1, 0), (1, 1), (0, 1)]:
            yi.addUv(*uv)
        assert yi.addTriangleWithUv(0, 1, 2, 0, 1, 2, mat) and yi.addTriangleWithUv(0, 2, 3, 0, 2, 3, mat)
    else:
        assert yi.addTriangle(0, 1, 2, mat) and yi.addTriangle(0, 2, 3, mat)
    assert yi.endTriMesh(), yi.getLastError()


def test_add_instance_on_an_existing_base_and_read_back():
    yi = fresh()
    mat = material(yi)
    assert yi.startGeometry()
    quad(yi, 7, mat, BASEMESH, has_orco=True, has_uv=True)
    assert yi.endGeometry()
    assert yi.addInstance(7, M_GENERAL), yi.getLastError()
    assert yi.addInstance(7, np.eye(4)), yi.getLastError()         # no geometry-state check: issued at document level
    got = yi.getInstances()
    assert len(got) == 2
    assert [g["base"] for g in got] == [7, 7]
    ids = [g["id"] for g in got]
    assert len(set(ids)) == 2 and 7 not in ids and all(i > 0 for i in ids) and ids == sorted(ids), ids      # ids of their own, in object-id order
    assert np.array_equal(got[0]["matrix"].view(np.uint32), M_GENERAL.view(np.uint32))
    assert np.array_equal(got[1]["matrix"], np.eye(4, dtype=np.float32))
    for g in got:
        assert (g["has_orco"], g["has_uv"], g["is_smooth"], g["normals_exported"]) == (True, True, False, False)
    # the next free id lies beyond the instances' ids
    assert yi.getNextFreeId() not in ids + [7]


def test_any_mesh_can_be_a_base_flagged_or_not():
    yi = fresh()
    mat = material(yi)
    assert yi.startGeometry()
    quad(yi, 1, mat)                  # a visible, non-base mesh
    quad(yi, 2, mat, BASEMESH)
    assert yi.endGeometry()
    assert yi.addInstance(1, np.eye(4)), yi.getLastError()
    assert yi.addInstance(2, np.eye(4)), yi.getLastError()
    assert [g["base"] for g in yi.getInstances()] == [1, 2]


def test_flags_are_copied_at_the_call():
    """is_smooth_ as it stands at addInstance: a base smoothed before one call and after another (object_geom.cc:108-111)"""
    yi = fresh()
    mat = material(yi)
    assert yi.startGeometry()
    quad(yi, 3, mat, BASEMESH)
    assert yi.addInstance(3, np.eye(4)), yi.getLastError()          # before smoothMesh
    assert yi.smoothMesh(3, 181.0), yi.getLastError()
    assert yi.addInstance(3, M_GENERAL), yi.getLastError()          # after
    assert yi.endGeometry()
    first, second = yi.getInstances()
    assert (first["is_smooth"], first["normals_exported"]) == (False, False)
    assert (second["is_smooth"], second["normals_exported"]) == (True, False)
    # exported normals are a flag of their own
    assert yi.startGeometry()
    assert yi.startTriMesh(4, 3, 1, False, False, BASEMESH)
    for p in [(0, 0, 0), (1, 0, 0), (0, 1, 0)]:
        yi.addVertex(*p)
        yi.addNormal(0.0, 0.0, 1.0)
    assert yi.addTriangle(0, 1, 2, mat) and yi.endTriMesh() and yi.endGeometry()
    assert yi.addInstance(4, np.eye(4)), yi.getLastError()
    third = [g for g in yi.getInstances() if g["base"] == 4][0]
    assert (third["is_smooth"], third["normals_exported"]) == (False, True)


def test_every_refusal_names_its_cause():
    yi = fresh()
    mat = material(yi)
    # the empty scene: the refusal tests/test_host_api.py holds
    assert not yi.addInstance(1, np.eye(4))
    assert "addInstance" in yi.getLastError() and "doesn't exist" in yi.getLastError(), yi.getLastError()
    assert yi.startGeometry()
    quad(yi, 1, mat, BASEMESH)
    assert yi.endGeometry()
    assert not yi.addInstance(5, np.eye(4))
    assert "addInstance" in yi.getLastError() and "5" in yi.getLastError(), yi.getLastError()
    assert not yi.addInstance(1, None)
    assert "addInstance" in yi.getLastError() and "null matrix" in yi.getLastError(), yi.getLastError()
    for bad in (np.nan, np.inf, -np.inf):
        m = np.eye(4, dtype=np.float32)
        m[2, 1] = bad
        assert not yi.addInstance(1, m)
        assert "addInstance" in yi.getLastError() and "non-finite" in yi.getLastError() and "m21" in yi.getLastError(), yi.getLastError()
    assert yi.getInstances() == []                                   # a refused call stores nothing
    assert yi.addInstance(1, np.eye(4)), yi.getLastError()
    inst = yi.getInstances()[0]["id"]
    assert not yi.addInstance(inst, np.eye(4))
    err = yi.getLastError()
    assert "addInstance" in err and "itself an instance" in err and "not built" in err and "object_geom.cc:104-121" in err, err
    assert len(yi.getInstances()) == 1
    # an instance has no normals of its own
    assert yi.startGeometry()
    assert not yi.smoothMesh(inst, 181.0)
    assert "smoothMesh" in yi.getLastError() and "instance" in yi.getLastError(), yi.getLastError()
    assert yi.smoothMesh(1, 181.0), yi.getLastError()
    assert yi.endGeometry()


def test_start_scene_forgets_instances():
    yi = fresh()
    mat = material(yi)
    assert yi.startGeometry()
    quad(yi, 1, mat)
    assert yi.endGeometry()
    assert yi.addInstance(1, np.eye(4)), yi.getLastError()
    assert len(yi.getInstances()) == 1
    assert yi.startScene(0)
    assert yi.getInstances() == []
    assert not yi.addInstance(1, np.eye(4)) and "addInstance" in yi.getLastError()      # the meshes went with them


XML_HEAD = """<?xml version="1.0"?>
<scene type="triangle">
<material name="red">
  <type sval="shinydiffusemat"/>
  <color r="0.8" g="0.1" b="0.1" a="1"/>
</material>
<mesh id="3" vertices="3" faces="1" has_orco="false" has_uv="false" type="512">
  <p x="0" y="0" z="0"/>
  <p x="1" y="0" z="0"/>
  <p x="0" y="1" z="0"/>
  <set_material sval="red"/>
  <f a="0" b="1" c="2"/>
</mesh>
"""


def transform(m):
    return "<transform " + " ".join(f'm{i}{j}="{float(m[i][j])!r}"' for i in range(4) for j in range(4)) + "/>"


def test_xml_scene_with_two_instances(tmp_path):
    m2 = np.eye(4, dtype=np.float32)
    m2[:3, 3] = (2.0, -1.0, 0.5)
    path = tmp_path / "instances.xml"
    path.write_text(XML_HEAD + f'<instance base_object_id="3">\n  {transform(M_GENERAL)}\n</instance>\n'
                    + f'<instance base_object_id="3">\n  {transform(m2)}\n</instance>\n</scene>\n')
    yi = Interface(strict=False)
    assert yi.loadXml(str(path)), yi.getLastError()
    got = yi.getInstances()
    assert [g["base"] for g in got] == [3, 3]
    assert np.array_equal(got[0]["matrix"].view(np.uint32), M_GENERAL.view(np.uint32))      # atof into a float
    assert np.array_equal(got[1]["matrix"].view(np.uint32), m2.view(np.uint32))
    assert all(g["id"] != 3 for g in got) and got[0]["id"] != got[1]["id"]


def test_xml_incomplete_transform_is_refused(tmp_path):
    """the reference multiplies with the uninitialised floats of its float[4][4] (import_xml.cc:650-661)"""
    attrs = transform(np.eye(4)).replace(' m23="0.0"', "")
    assert "m23" not in attrs
    path = tmp_path / "incomplete.xml"
    path.write_text(XML_HEAD + f'<instance base_object_id="3">\n  {attrs}\n</instance>\n</scene>\n')
    yi = Interface(strict=False)
    assert not yi.loadXml(str(path))
    assert "transform" in yi.getLastError() and "sixteen" in yi.getLastError(), yi.getLastError()
    assert yi.getInstances() == []
    # an unknown base is the call's own refusal
    path.write_text(XML_HEAD + f'<instance base_object_id="9">\n  {transform(np.eye(4))}\n</instance>\n</scene>\n')
    yi = Interface(strict=False)
    assert not yi.loadXml(str(path))
    assert "addInstance" in yi.getLastError(), yi.getLastError()
