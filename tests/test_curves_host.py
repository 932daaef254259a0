"""Curve meshes on the host: Scene::startCurveMesh / endCurveMesh (scene.cc:133-281) as yafaray_startCurveMesh / yafaray_endCurveMesh
restate them — the state machine with every refusal and its cause, what endCurveMesh stores as yafaray_getCurves hands it back (the
points and the two extrusion scales per point, held bit for bit to tests/curves_fixture.py's restatement of the radius), the bulk
yafaray_addCurves against the loop of single calls it is defined as, and the <curve> element of the XML loader
(import_xml.cc:461-546).  No GPU needed: the triangles are made on the device, tests/test_gpu_curves.py holds those."""
import numpy as np
import pytest

from libyafaray_amd import Interface
from tests import curves_fixture as cf

F = np.float32
U = np.uint32
RED = {"type": "shinydiffusemat", "color": ("color", 0.8, 0.1, 0.1, 1.0), "diffuse_reflect": 1.0}
BLUE = {"type": "shinydiffusemat", "color": ("color", 0.1, 0.1, 0.8, 1.0), "diffuse_reflect": 1.0}


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


def curve(yi, cid, points, mat, start, end, shape):
    assert yi.startCurveMesh(cid, len(points)), yi.getLastError()
    for k, p in enumerate(points):
        assert yi.addVertex(*[float(x) for x in p]) == k
    return yi.endCurveMesh(mat, start, end, shape)


def refused(yi, ok, *needles):
    assert not ok
    for n in needles:
        assert n in yi.getLastError(), yi.getLastError()


# ---- the state machine ------------------------------------------------------------------------------------------------------------
def test_start_is_refused_outside_geometry_and_inside_an_open_object():
    yi = fresh()
    mat = material(yi)
    refused(yi, yi.startCurveMesh(5, 10), "startCurveMesh:")                       # the ready state: the refusal tests/test_host_api.py holds
    assert yi.getLastError().startswith("startCurveMesh:")
    assert yi.startGeometry()
    assert yi.startTriMesh(1, 3, 1, False, False, 0)
    refused(yi, yi.startCurveMesh(5, 10), "startCurveMesh:", "mesh is open")
    for p in [(0, 0, 0), (1, 0, 0), (0, 1, 0)]:
        yi.addVertex(*p)
    assert yi.addTriangle(0, 1, 2, mat) and yi.endTriMesh()
    assert yi.startCurveMesh(5, 10), yi.getLastError()
    refused(yi, yi.startCurveMesh(6, 10), "startCurveMesh:", "already open")       # a second start inside a curve
    assert yi.addVertex(0, 0, 0) == 0 and yi.addVertex(0, 0, 1) == 1
    assert yi.endCurveMesh(mat, 0.1, 0.05, 0.0), yi.getLastError()
    assert yi.endGeometry()
    assert [c["id"] for c in yi.getCurves()] == [5]


def test_end_is_refused_with_the_cause():
    yi = fresh()
    mat = material(yi)
    refused(yi, yi.endCurveMesh(None, 0.1, 0.1, 0.0), "endCurveMesh:")             # the ready state, a null material: tests/test_host_api.py's call
    assert yi.getLastError().startswith("endCurveMesh:")
    assert yi.startGeometry()
    refused(yi, yi.endCurveMesh(mat, 0.1, 0.1, 0.0), "endCurveMesh:", "no curve mesh is open")
    assert yi.startCurveMesh(1, 2) and yi.addVertex(0, 0, 0) == 0 and yi.addVertex(0, 0, 1) == 1
    refused(yi, yi.endCurveMesh(None, 0.1, 0.1, 0.0), "endCurveMesh:", "null material")
    for n_points in (0, 1):
        refused(yi, curve(yi, 2, [(0, 0, float(k)) for k in range(n_points)], mat, 0.1, 0.1, 0.0), "endCurveMesh:", "two or more points", f"has {n_points}")
    refused(yi, curve(yi, 3, [(0, 0, 0), (0, float("nan"), 1)], mat, 0.1, 0.1, 0.0), "endCurveMesh:", "non-finite coordinate in point 1")
    refused(yi, curve(yi, 3, [(0, 0, 0), (0, 1e300, 1)], mat, 0.1, 0.1, 0.0), "endCurveMesh:", "non-finite coordinate")      # overflows a float
    for params in ((float("inf"), 0.1, 0.0), (0.1, float("nan"), 0.0), (0.1, 0.1, float("inf"))):
        refused(yi, curve(yi, 4, [(0, 0, 0), (0, 0, 1)], mat, *params), "endCurveMesh:", "non-finite strand_start, strand_end or strand_shape")
    refused(yi, curve(yi, 4, [(0, 0, 0), (0, 0, 1)], mat, 0.1, 0.2, -1.5), "endCurveMesh:", "non-finite radius at point 0")   # pow(0, -0.5)
    # a refused end closes the block and drops the object: the geometry block goes on
    assert yi.getCurves() == []
    assert curve(yi, 4, [(0, 0, 0), (0, 0, 1)], mat, 0.1, 0.2, 0.5), yi.getLastError()
    assert yi.endGeometry(), yi.getLastError()
    assert [c["id"] for c in yi.getCurves()] == [4]


def test_only_add_vertex_is_accepted_inside_a_curve():
    yi = fresh()
    mat = material(yi)
    assert yi.startGeometry() and yi.startCurveMesh(1, 3)
    assert yi.addVertex(0, 0, 0) == 0
    for call, name in [(lambda: yi.addTriangle(0, 0, 0, mat), "addTriangle"), (lambda: yi.addTriangleWithUv(0, 0, 0, 0, 0, 0, mat), "addTriangle"),
                       (lambda: yi.addUv(0.5, 0.5) >= 0, "addUv"), (lambda: yi.addVertexWithOrco(0, 0, 0, 0, 0, 0) >= 0, "addVertex"),
                       (lambda: yi.addTriangles(np.zeros((3, 3), F), np.arange(3, dtype=np.int32), mat), "addTriangles"),
                       (lambda: yi.endTriMesh(), "endTriMesh"), (lambda: yi.startTriMesh(2, 3, 1, False, False, 0), "startTriMesh")]:
        refused(yi, call(), name + ":", "curve mesh is open")
    yi.addNormal(0.0, 0.0, 1.0)
    assert "addNormal:" in yi.getLastError() and "curve mesh is open" in yi.getLastError(), yi.getLastError()
    refused(yi, yi.endGeometry(), "endGeometry")
    assert yi.addVertex(0, 0, 1) == 1                                                  # none of them disturbed the strand
    assert yi.endCurveMesh(mat, 0.2, 0.1, 0.0) and yi.endGeometry(), yi.getLastError()
    (c,) = yi.getCurves()
    assert np.array_equal(c["points"][:, :3], np.array([(0, 0, 0), (0, 0, 1)], F))


def test_smooth_mesh_and_add_instance_on_a_curve_are_refused():
    yi = fresh()
    mat = material(yi)
    assert yi.startGeometry()
    assert curve(yi, 9, [(0, 0, 0), (0, 0, 1), (0, 1, 2)], mat, 0.1, 0.0, 0.0), yi.getLastError()
    refused(yi, yi.smoothMesh(9, 181.0), "smoothMesh:", "curve mesh")
    refused(yi, yi.smoothMesh(0, 181.0), "smoothMesh:", "curve mesh")                  # "the current object" is the curve
    refused(yi, yi.addInstance(9, np.eye(4)), "addInstance:", "curve mesh")
    assert yi.endGeometry()
    refused(yi, yi.addInstance(9, np.eye(4)), "addInstance:", "curve mesh")
    assert yi.getInstances() == [] and len(yi.getCurves()) == 1


def test_ids_are_shared_with_meshes_and_instances():
    yi = fresh()
    mat = material(yi)
    assert yi.startGeometry()
    first = yi.getNextFreeId()
    assert curve(yi, first, [(0, 0, 0), (0, 0, 1)], mat, 0.1, 0.1, 0.0)
    assert yi.getNextFreeId() != first
    assert curve(yi, 40, [(0, 0, 0), (0, 0, 1)], mat, 0.1, 0.1, 0.0)
    # a mesh started under a curve's id takes its place, as in the one slot of meshes_[id]
    assert yi.startTriMesh(40, 3, 1, False, False, 0)
    for p in [(0, 0, 0), (1, 0, 0), (0, 1, 0)]:
        yi.addVertex(*p)
    assert yi.addTriangle(0, 1, 2, mat) and yi.endTriMesh() and yi.endGeometry()
    assert [c["id"] for c in yi.getCurves()] == [first]
    assert yi.addInstance(40, np.eye(4)), yi.getLastError()
    assert yi.startScene(0) and yi.getCurves() == []


# ---- what endCurveMesh stores -------------------------------------------------------------------------------------------------------
SHAPES = (-0.5, 0.0, 0.7)
COUNTS = (2, 3, 17)
RADII = ((0.05, 0.0125), (0.03, 0.03), (0.04, 0.0))      # a taper; start = end; a tip radius of 0, the common export


@pytest.mark.parametrize("shape", SHAPES)
def test_stored_scales_are_the_restated_radius_bit_for_bit(shape):
    yi = fresh()
    mat = material(yi)
    other = material(yi, "blue", BLUE)
    assert yi.startGeometry()
    want = []
    for n in COUNTS:
        for start, end in RADII:
            pts = cf.strand(n, 100 * n + len(want))
            cid = yi.getNextFreeId()
            use = other if len(want) % 2 else mat
            assert curve(yi, cid, pts, use, start, end, shape), yi.getLastError()
            want.append((cid, pts, len(want) % 2, start, end))
    assert yi.endGeometry()
    got = yi.getCurves()
    assert [c["id"] for c in got] == [w[0] for w in want]
    for c, (cid, pts, mat_index, start, end) in zip(got, want):
        n = len(pts)
        h, s = cf.scales(n, start, end, shape)
        assert c["material"] == mat_index
        assert (c["strand_start"], c["strand_end"], c["strand_shape"]) == (F(start), F(end), F(shape))
        assert c["points"].shape == (n, 5)
        assert np.array_equal(c["points"][:, :3].view(U), pts.view(U))
        assert np.array_equal(c["points"][:, 3].view(U), h.view(U)), (n, start, end, shape, c["points"][:, 3], h)
        assert np.array_equal(c["points"][:, 4].view(U), s.view(U)), (n, start, end, shape, c["points"][:, 4], s)
        # what the radius does: the root and the tip are what was asked for
        r = c["points"][:, 3].astype(np.float64) * 2
        assert r[0] == F(F(start) * F(1)) and abs(r[-1] - end) <= 1e-7
        if start == end:
            assert (c["points"][:, 3] == c["points"][0, 3]).all()
        if end == 0.0:
            assert c["points"][-1, 3] == 0 and c["points"][-1, 4] == 0, "a tip radius of exactly 0"


def test_the_restated_radius_takes_both_branches():
    """the sign of strand_shape picks the expression (scene.cc:172-179); at shape 0 both are linear but round differently"""
    h_neg, _ = cf.scales(17, 0.05, 0.0125, -0.5)
    h_zero, _ = cf.scales(17, 0.05, 0.0125, 0.0)
    h_pos, _ = cf.scales(17, 0.05, 0.0125, 0.7)
    assert (h_neg[1:-1] < h_zero[1:-1]).all() and (h_pos[1:-1] > h_zero[1:-1]).all()      # t^0.5 runs ahead of t: thins early; 1 - (1 - t)^0.3 lags: stays thick
    assert (np.diff(h_neg) < 0).all() and (np.diff(h_pos) < 0).all()


# ---- addCurves ------------------------------------------------------------------------------------------------------------------------
def test_add_curves_is_the_loop_of_single_calls():
    counts = [2, 17, 3, 9, 2]
    pts = np.concatenate([cf.strand(n, 7 + k, origin=(k, 0, 0)) for k, n in enumerate(counts)])
    a, b = fresh(), fresh()
    ma, mb = material(a), material(b)
    for yi in (a, b):                 # something before, so that ids do not start at 1 by accident
        assert yi.startGeometry() and curve(yi, 2, [(0, 0, 0), (1, 0, 0)], ma if yi is a else mb, 0.1, 0.1, 0.0)
    ids = a.addCurves(counts, pts, ma, 0.05, 0.0, -0.25)
    assert ids is not None, a.getLastError()
    loop_ids, at = [], 0
    for n in counts:
        cid = b.getNextFreeId()
        assert curve(b, cid, pts[at:at + n], mb, 0.05, 0.0, -0.25), b.getLastError()
        loop_ids.append(cid); at += n
    assert list(ids) == loop_ids and 2 not in loop_ids
    assert a.endGeometry() and b.endGeometry()
    ca, cb = a.getCurves(), b.getCurves()
    assert len(ca) == len(cb) == len(counts) + 1
    for x, y in zip(ca, cb):
        assert (x["id"], x["material"]) == (y["id"], y["material"])
        assert (x["strand_start"], x["strand_end"], x["strand_shape"]) == (y["strand_start"], y["strand_end"], y["strand_shape"])
        assert np.array_equal(x["points"].view(U), y["points"].view(U))
    assert a.getNextFreeId() == b.getNextFreeId()
    # it stops at the first refusal, with that call's cause, and keeps what came before
    c = fresh()
    mc = material(c)
    assert c.startGeometry()
    assert c.addCurves([2, 1, 2], np.zeros((5, 3), F) + np.arange(5, dtype=F)[:, None], mc, 0.1, 0.1, 0.0) is None
    assert "endCurveMesh:" in c.getLastError() and "two or more points" in c.getLastError(), c.getLastError()
    assert len(c.getCurves()) == 1
    d = fresh()
    assert d.addCurves([2], np.zeros((2, 3), F), material(d), 0.1, 0.1, 0.0) is None and "startCurveMesh:" in d.getLastError()      # outside geometry


# ---- XML ------------------------------------------------------------------------------------------------------------------------------
XML_HEAD = """<?xml version="1.0"?>
<scene type="triangle">
<material name="red">
  <type sval="shinydiffusemat"/>
  <color r="0.8" g="0.1" b="0.1" a="1"/>
</material>
"""
XML_POINTS = [(0.0, 0.0, 0.0), (0.1, 0.0, 0.5), (0.1, 0.2, 1.0), (0.0, 0.25, 1.5)]


def curve_xml(attrs, material_name="red", points=XML_POINTS):
    body = "".join(f'  <p x="{x!r}" y="{y!r}" z="{z!r}"/>\n' for x, y, z in points)
    return (f"<curve {attrs}>\n{body}  <strand_start fval=\"0.0625\"/>\n  <strand_end fval=\"0.01\"/>\n  <strand_shape fval=\"-0.3\"/>\n"
            f"  <set_material sval=\"{material_name}\"/>\n</curve>\n")


def test_xml_curve_equals_the_same_scene_by_calls(tmp_path):
    path = tmp_path / "curves.xml"
    path.write_text(XML_HEAD + curve_xml('id="12" vertices="4"') + curve_xml('vertices="4"') + "</scene>\n")
    yi = Interface(strict=False)
    assert yi.loadXml(str(path)), yi.getLastError()
    by_calls = fresh()
    mat = material(by_calls)
    ids = [12]
    for k in range(2):
        assert by_calls.startGeometry()
        if k == 1:
            ids.append(by_calls.getNextFreeId())       # an id omitted takes the next free one
        assert curve(by_calls, ids[k], XML_POINTS, mat, 0.0625, 0.01, -0.3), by_calls.getLastError()
        assert by_calls.endGeometry()
    got, want = yi.getCurves(), by_calls.getCurves()
    assert sorted(c["id"] for c in got) == sorted(ids) and ids[1] != 12
    assert len(got) == len(want) == 2
    for x, y in zip(got, want):
        assert (x["id"], x["material"]) == (y["id"], y["material"])
        assert (x["strand_start"], x["strand_end"], x["strand_shape"]) == (y["strand_start"], y["strand_end"], y["strand_shape"]) == (F(0.0625), F(0.01), F(-0.3))
        assert np.array_equal(x["points"].view(U), y["points"].view(U))
    # the geometry block was closed again: the scene is in the ready state
    assert yi.startGeometry() and yi.endGeometry()


def test_xml_curve_with_an_unknown_material_is_refused(tmp_path):
    """the reference warns "Unknown material!" and goes on with a null pointer"""
    path = tmp_path / "unknown.xml"
    path.write_text(XML_HEAD + curve_xml('id="3" vertices="4"', material_name="green") + "</scene>\n")
    yi = Interface(strict=False)
    assert not yi.loadXml(str(path))
    assert "curve" in yi.getLastError() and "unknown material" in yi.getLastError() and "green" in yi.getLastError(), yi.getLastError()
    assert yi.getCurves() == []
    # no <set_material> at all is endCurveMesh's own refusal
    path.write_text(XML_HEAD + curve_xml('id="3" vertices="4"').replace('  <set_material sval="red"/>\n', "") + "</scene>\n")
    yi = Interface(strict=False)
    assert not yi.loadXml(str(path))
    assert "endCurveMesh:" in yi.getLastError() and "null material" in yi.getLastError(), yi.getLastError()
