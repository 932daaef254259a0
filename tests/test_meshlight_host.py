"""The mesh light on the host: its factory (light_meshlight.cc:231-262) restated bit for bit, the getLights() row, light_enabled /
photon_only, the XML loader, the look-up of the mesh at prepareRender (MeshLight::init, :75-86) and every refusal with its cause.  No GPU
needed: where prepareRender gets as far as the device, a machine without one answers "scene upload: hip...", which counts as passed.
The float32 restatements of MeshLight::initIs, ::illumSample and ::intersect here are shared with tests/test_gpu_meshlight.py."""
import numpy as np
import pytest

from libyafaray_amd import Interface, scenes
from tests.test_gpu_lights import plane_scene
from tests.test_lights_host import F, W_COLOR, bits, color, cross, dot, ints, light_of

TYPE_MESH = 7
# word offsets in a yafgpu_light record (include/yafgpu.h): the mesh light's words in the union, then area behind the colour
W_FIRST, W_COUNT, W_POOL, W_DOUBLE, W_ROW, W_AREA = 4, 5, 6, 7, 8, 28
M_PI = 3.14159265358979323846


def iw(rec, w):
    return int(np.asarray(rec[w], np.float32).view(np.int32))


# ---- float32 restatements in the reference's operation order (float64 only where the reference has a double) ----
def tri_areas(v):
    """Triangle::surfaceArea, triangle.cc:169-179, for (n, 3, 3) corners: 0.5 * (edge_1 ^ edge_2).length(), the 0.5 a double"""
    v = np.asarray(v, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        c = cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
        return (0.5 * np.sqrt(dot(c, c)).astype(np.float64)).astype(np.float32)


def pdf1d(func):
    """Pdf1D's constructor, util_sample.h:89-122 -> cdf_ (n + 1), integral_; the running sum is a double, in index order"""
    n = len(func)
    run = np.cumsum(func.astype(np.float64) * (1.0 / float(n)))          # c += (double)f[i - 1] * delta  (np.cumsum adds in index order)
    cdf = np.concatenate([[F(0)], run.astype(np.float32)]).astype(np.float32)
    integral = np.float32(run[-1])
    with np.errstate(all="ignore"):
        cdf[1:] = cdf[1:] / integral
    return cdf, integral


def total_area(func):
    """MeshLight::initIs, light_meshlight.cc:61-68: a double sum of the float areas in index order, narrowed"""
    return np.float32(np.cumsum(func.astype(np.float64))[-1])


def d_sample(cdf, u):
    """Pdf1D::dSample, util_sample.h:144-160: the u == 0 shortcut, then std::lower_bound over the n + 1 entries"""
    idx = np.searchsorted(cdf, u, side="left").astype(np.int64) - 1
    return np.where(u == 0, 0, np.maximum(idx, 0))


def illum_sample(verts, normals, cdf, area, double_sided, col, p, s1, s2):
    """MeshLight::illumSample (light_meshlight.cc:110-148) with sampleSurface (:88-106) and Triangle::sample (triangle.cc:181-192)
    -> (n, 9): ok, wi.dir_, wi.tmax_, s.pdf_, s.col_ (zeros where refused), and the triangle each sample chose"""
    n_tris = verts.shape[0]
    prim = d_sample(cdf, s1)
    refused = prim >= n_tris                        # "Sampling error!"
    pc = np.minimum(prim, n_tris - 1)
    with np.errstate(all="ignore"):
        delta = cdf[pc + 1]
        ss1 = np.where(pc > 0, (s1 - cdf[pc]) / (delta - cdf[pc]), s1 / delta).astype(np.float32)
        su1 = np.sqrt(ss1)
        u = F(1) - su1
        v = s2 * su1
        a, b, c = verts[pc, 0], verts[pc, 1], verts[pc, 2]
        pl = (a * u[:, None] + b * v[:, None]) + c * (F(1) - u - v)[:, None]
        ldir = pl - p
        dist_sqr = dot(ldir, ldir)
        dist = np.sqrt(dist_sqr)
        ok = ~refused & ~(dist <= 0)
        ldir = ldir * (F(1) / dist)[:, None]
        cos = -dot(ldir, normals[pc])
        back = cos <= 0
        if double_sided:
            cos = np.where(back, -cos, cos)
        else:
            ok &= ~back
        amc = F(area) * cos
        pdf = (dist_sqr.astype(np.float64) * M_PI / np.where(amc == 0, F(1e-8), amc).astype(np.float64)).astype(np.float32)
    out = np.zeros((len(s1), 9), np.float32)
    out[:, 0] = ok
    out[ok, 1:4] = ldir[ok]; out[ok, 4] = dist[ok]; out[ok, 5] = pdf[ok]; out[ok, 6:9] = np.asarray(col, np.float32)
    return out, prim


def tri_test(rows, frm, d):
    """Triangle::intersect (triangle.h:223-259) of every ray with ONE triangle's 48-byte record rows = (a, eps, e1, e2) -> hit, t"""
    a, eps, e1, e2 = rows
    with np.errstate(all="ignore"):
        pvec = cross(d, np.broadcast_to(e2, d.shape))
        det = dot(np.broadcast_to(e1, d.shape), pvec)
        ok = ~((det > -eps) & (det < eps))
        inv = F(1) / det
        tvec = frm - a
        u = dot(tvec, pvec) * inv
        ok &= ~((u < 0) | (u > 1))
        qvec = cross(tvec, np.broadcast_to(e1, d.shape))
        v = dot(d, qvec) * inv
        ok &= ~((v < 0) | ((u + v) > 1))
        t = dot(np.broadcast_to(e2, d.shape), qvec) * inv
        ok &= ~(t < eps)
    return ok, t


def intersect(rows, normals, area, double_sided, col, frm, d, tmin):
    """MeshLight::intersect (light_meshlight.cc:190-213) over the light's triangle records in index order, the closest hit with
    tmin <= t < infinity as TriKdTree::intersect takes it (kdtree_triangle.cc:780-817) -> (n, 6): ok, t, ipdf, col; the triangle hit (-1:
    none); and the brute-force closest t over the same records (inf: none)"""
    n = frm.shape[0]
    z = np.full(n, np.inf, np.float32); hit = np.full(n, -1, np.int64)
    every = np.full((len(rows), n), np.inf, np.float32)
    for k, r in enumerate(rows):
        ok, t = tri_test(r, frm, d)
        take = ok & (t >= tmin)
        every[k, take] = t[take]
        better = take & (t < z)
        z = np.where(better, t, z); hit = np.where(better, k, hit)
    found = hit >= 0
    hc = np.maximum(hit, 0)
    with np.errstate(all="ignore"):
        cos = dot(d, -normals[hc])
        back = cos <= 0
        ok = found.copy()
        if double_sided:
            cos = np.abs(cos)
        else:
            ok &= ~back
        idist_sqr = F(1) / (z * z)
        ipdf = (((idist_sqr * F(area)) * cos).astype(np.float64) * (1.0 / M_PI)).astype(np.float32)
    out = np.zeros((n, 6), np.float32)
    out[:, 0] = ok; out[ok, 1] = z[ok]; out[ok, 2] = ipdf[ok]; out[ok, 3:6] = np.asarray(col, np.float32)
    return out, hit, every.min(axis=0)


# ---- scenes: the plane of tests/test_gpu_lights.py as mesh 1, every further mesh under its own id from 2 on ----
QUAD = scenes._quad((-0.5, -0.5, 2.0), (-0.5, 0.5, 2.0), (0.5, 0.5, 2.0), (0.5, -0.5, 2.0))          # faces -z: down onto the plane
LAMP = {"type": "light_mat", "color": (1.0, 1.0, 1.0), "power": 1.0}


def meshlight(obj=2, **kw):
    return dict({"type": "meshlight", "object": obj, "color": (1.0, 1.0, 1.0), "power": 2.0, "samples": 4}, **kw)


def scene_with(meshes, lights, res=8, **kw):
    sc = plane_scene(lights, res=res, **kw)
    sc["materials"] = sc["materials"] + [LAMP]
    sc["extra_meshes"] = [{"verts": np.asarray(v, np.float32), "material": len(sc["materials"]) - 1} for v in meshes]
    return sc


def loaded(sc, res=8, spp=1, **kw):
    yi = Interface(strict=False)
    rd = scenes.render_settings(res, res, spp, integrator="directlighting", **kw)
    yi.handles = scenes.load_scene(yi, sc, rd)      # the material handles, for tests that add geometry of their own afterwards
    return yi, rd


def prepared(yi):
    """prepareRender got through every host-side check: it succeeded, or the first HIP call found no device"""
    ok = yi.prepareRender()
    return bool(ok) or yi.getLastError().startswith("scene upload: hip")


# ---- the factory ----
def test_defaults():
    yi, h = light_of({"type": "meshlight", "object": 3})
    assert h, yi.getLastError()
    rec = yi.getLights()
    assert rec.shape == (1, 34)
    r = rec[0]
    typ, samples, cast, inf = ints(r)
    assert (typ, samples, cast, inf) == (TYPE_MESH, 4, 1, 0)
    assert iw(r, W_DOUBLE) == 0 and iw(r, W_FIRST) == -1 and iw(r, W_COUNT) == 0 and r[W_AREA] == 0        # no mesh yet
    assert np.array_equal(bits(r[W_COLOR:W_COLOR + 3]), bits(np.full(3, F(1) * F(1) * F(M_PI), np.float32)))


def test_every_parameter_and_the_colour_bit_for_bit():
    """color * (float)power * M_PI (light_meshlight.cc:255): Rgb * float twice, the second with M_PI narrowed (color.h:266)"""
    for power in (3.7, 0.1, 1e-3, 12345.678):
        yi, h = light_of({"type": "meshlight", "object": 2, "color": color(0.9, 0.5, 0.25), "power": power, "samples": 9, "double_sided": True,
                          "light_enabled": True, "cast_shadows": False, "with_caustic": False, "with_diffuse": True, "photon_only": False})
        assert h, yi.getLastError()
        r = yi.getLights()[0]
        assert tuple(ints(r)[:3]) == (TYPE_MESH, 9, 0) and iw(r, W_DOUBLE) == 1
        want = (np.array([0.9, 0.5, 0.25], np.float32) * F(power)) * F(M_PI)
        assert np.array_equal(bits(r[W_COLOR:W_COLOR + 3]), bits(want)), power


def test_disabled_light_stays_out_of_the_light_order():
    yi = Interface(strict=False)
    yi.startScene(0)
    for name, on in (("a", True), ("b", False), ("c", True)):
        yi.paramsClearAll()
        yi.paramsSet({"type": "meshlight", "object": 2, "light_enabled": on, "samples": 1 + ord(name)})
        assert yi.createLight(name), yi.getLastError()
    rec = yi.getLights()
    assert [int(s) for s in rec[:, 1].view(np.int32)] == [1 + ord("a"), 1 + ord("c")]


def test_photon_only_and_a_bare_meshlight_are_refused():
    yi, h = light_of({"type": "meshlight", "object": 2, "photon_only": True})
    assert not h and "photon_only" in yi.getLastError()
    for p in ({"type": "meshlight"}, {"type": "meshlight", "object": 2.0}):      # no object; a float is no object id
        yi, h = light_of(p)
        assert not h
        msg = yi.getLastError()
        assert "scope" in msg and "sunlight" in msg and "meshlight" in msg and "object" in msg, msg


# ---- the mesh, looked up at prepareRender ----
def test_lights_before_and_after_their_mesh_both_resolve():
    """load_scene creates its lights before the geometry; a third is created after.  Two lights share object 2 (legal), one sits on the
    plane's own mesh, whose material is no light_mat (legal too: the reference does not care)"""
    fan = np.concatenate([QUAD, QUAD + np.float32(1.5)])
    yi, rd = loaded(scene_with([QUAD, fan], [meshlight(2), meshlight(3, double_sided=True)]))
    yi.paramsClearAll()
    yi.paramsSet({"type": "meshlight", "object": 2, "power": 0.5})
    assert yi.createLight("late"), yi.getLastError()
    yi.paramsClearAll()
    yi.paramsSet({"type": "meshlight", "object": 1})
    assert yi.createLight("on_the_plane"), yi.getLastError()
    scenes.set_render_params(yi, rd)
    assert prepared(yi), yi.getLastError()
    rec = yi.getLights()
    # scene rows: the plane's two, then mesh 2's two, then mesh 3's four; the pool takes a light's triangles in light order
    assert [(iw(r, W_FIRST), iw(r, W_COUNT), iw(r, W_POOL)) for r in rec] == [(2, 2, 0), (4, 4, 2), (2, 2, 6), (0, 2, 8)]
    plane = scenes._quad((-10, -10, 0), (10, -10, 0), (10, 10, 0), (-10, 10, 0))
    for r, mesh in zip(rec, (QUAD, fan, QUAD, plane)):
        assert np.array_equal(bits(r[W_AREA]), bits(total_area(tri_areas(mesh)))), "area_: the double sum of the float areas, narrowed"


XML = """<?xml version="1.0"?>
<scene type="triangle">
<material name="white"><type sval="shinydiffusemat"/><color r="0.8" g="0.8" b="0.8" a="1"/><diffuse_reflect fval="1"/></material>
<material name="lamp"><type sval="light_mat"/><color r="1" g="1" b="1" a="1"/><power fval="10"/></material>
<light name="Shade"><type sval="meshlight"/><object ival="2"/><color r="1" g="0.9" b="0.8" a="1"/><power fval="2.5"/>
  <samples ival="6"/><double_sided bval="true"/><cast_shadows bval="true"/><light_enabled bval="true"/><photon_only bval="false"/>
  <with_caustic bval="true"/><with_diffuse bval="true"/></light>
<camera name="cam"><type sval="perspective"/><from x="0" y="-3" z="0"/><to x="0" y="0" z="0"/><up x="0" y="-3" z="1"/>
  <resx ival="16"/><resy ival="16"/><focal fval="1.2"/></camera>
<integrator name="default"><type sval="directlighting"/><caustic_type sval="none"/></integrator>
<integrator name="volintegr"><type sval="none"/></integrator>
<mesh id="1" vertices="4" faces="2" has_orco="false" has_uv="false" type="0">
  <p x="-1" y="-1" z="-1"/><p x="1" y="-1" z="-1"/><p x="1" y="1" z="-1"/><p x="-1" y="1" z="-1"/>
  <set_material sval="white"/><f a="0" b="1" c="2"/><f a="0" b="2" c="3"/>
</mesh>
<mesh id="2" vertices="3" faces="1" has_orco="false" has_uv="false" type="0">
  <p x="-0.5" y="-0.5" z="1"/><p x="0" y="0.5" z="1"/><p x="0.5" y="-0.5" z="1"/>
  <set_material sval="lamp"/><f a="0" b="1" c="2"/>
</mesh>
<render><camera_name sval="cam"/><integrator_name sval="default"/><volintegrator_name sval="volintegr"/>
  <width ival="16"/><height ival="16"/><AA_passes ival="1"/><AA_minsamples ival="1"/>
  <AA_pixelwidth fval="1"/><filter_type sval="box"/><tile_size ival="8"/></render>
</scene>
"""


def test_xml_round_trip(tmp_path):
    p = tmp_path / "meshlight.xml"
    p.write_text(XML)
    yi = Interface(strict=False)
    assert yi.loadXml(str(p)), yi.getLastError()
    r = yi.getLights()[0]
    assert tuple(ints(r)[:3]) == (TYPE_MESH, 6, 1) and iw(r, W_DOUBLE) == 1
    assert np.array_equal(bits(r[W_COLOR:W_COLOR + 3]), bits((np.array([1, 0.9, 0.8], np.float32) * F(2.5)) * F(M_PI)))
    assert prepared(yi), yi.getLastError()
    r = yi.getLights()[0]
    assert (iw(r, W_FIRST), iw(r, W_COUNT), iw(r, W_POOL)) == (2, 1, 0)


# ---- refusals at prepareRender, each with its cause; the interface stays unprepared ----
def refused(yi, *needles):
    assert not yi.prepareRender()
    msg = yi.getLastError()
    for n in needles:
        assert n in msg, msg
    assert not yi.getRenderSize()[0] and "prepareRender" in yi.getLastError()      # unprepared


def test_object_that_names_no_mesh():
    yi, _ = loaded(scene_with([QUAD], [meshlight(9)]))
    refused(yi, "meshlight object 9", "names no mesh")


def test_a_failed_prepare_after_a_good_one_leaves_the_interface_unprepared():
    yi, rd = loaded(scene_with([QUAD], [meshlight(2)]))
    assert prepared(yi), yi.getLastError()
    yi.paramsClearAll()
    yi.paramsSet({"type": "meshlight", "object": 9})
    assert yi.createLight("nowhere")
    scenes.set_render_params(yi, rd)
    refused(yi, "names no mesh")


def test_object_that_names_a_curve_or_an_instance():
    yi, rd = loaded(scene_with([QUAD], [meshlight(5)]))
    assert yi.startGeometry() and yi.startCurveMesh(5, 2)
    yi.addVertex(0.0, 0.0, 1.0); yi.addVertex(0.0, 0.0, 1.5)
    assert yi.endCurveMesh(yi.handles[0], 0.05, 0.01, 0.0) and yi.endGeometry()
    scenes.set_render_params(yi, rd)
    refused(yi, "meshlight object 5", "curve mesh or an instance", "device only")
    yi, rd = loaded(scene_with([QUAD], [meshlight(3)]))
    assert yi.addInstance(2, np.eye(4)), yi.getLastError()            # takes the next free id, 3
    assert yi.getInstances()[0]["id"] == 3
    scenes.set_render_params(yi, rd)
    refused(yi, "meshlight object 3", "curve mesh or an instance", "device only")


def test_a_mesh_that_is_not_rendered():
    yi, rd = loaded(scene_with([QUAD], [meshlight(7)]))
    assert yi.startGeometry() and yi.startTriMesh(7, 6, 2, False, False, 0x0200)           # a base mesh for instances: no rows of its own
    assert yi.addTriangles(QUAD.reshape(-1, 3), np.arange(6, dtype=np.int32), yi.handles[0]) and yi.endTriMesh() and yi.endGeometry()
    scenes.set_render_params(yi, rd)
    refused(yi, "meshlight object 7", "not rendered")


def test_a_mesh_with_no_triangles():
    yi, rd = loaded(scene_with([QUAD], [meshlight(7)]))
    assert yi.startGeometry() and yi.startTriMesh(7, 0, 0, False, False, 0) and yi.endTriMesh() and yi.endGeometry()
    scenes.set_render_params(yi, rd)
    refused(yi, "meshlight object 7", "no triangles")


@pytest.mark.parametrize("case", ["zero", "not finite"])
def test_a_mesh_without_a_usable_area(case):
    if case == "zero":
        v = np.array([[[0, 0, 1], [1, 1, 2], [2, 2, 3]], [[0, 0, 1], [0, 0, 1], [0, 0, 1]]], np.float32)      # collinear, and a point
    else:
        v = np.array([[[0, 0, 1], [3e30, 0, 1], [0, 3e30, 1]]], np.float32)                                    # finite corners, an infinite cross product
    assert not (tri_areas(v).sum() > 0 and np.isfinite(tri_areas(v).sum()))
    yi, _ = loaded(scene_with([v], [meshlight(2)]))
    refused(yi, "meshlight object 2", "total area is zero or not finite")


def test_ao_with_more_than_254_lights_is_still_refused():
    yi, _ = loaded(scene_with([QUAD], [meshlight(2)] * 255), do_AO=True, AO_samples=4)
    refused(yi, "do_AO", "254")

