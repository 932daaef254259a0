"""Host-side mirror of yafaray4::Interface (include/interface/interface.h:48-139) over the C ABI.

Method names and argument meaning follow the reference class (and its SWIG module
src/bindings/yafaray4_interface.i), so a script written against the reference's Python bindings
ports by changing the import.  Error behaviour follows the reference too (False / None on failure)
with the diagnostic available from getLastError(); `strict=True` raises instead.
"""
import ctypes as C
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))


def lib_path():
    # YAFARAY_LIBRARY: test support (tests/asan builds the host side with a device stub under AddressSanitizer)
    return os.environ.get("YAFARAY_LIBRARY") or os.path.join(_HERE, "libyafaray_gpu.so")


class YafaRayError(RuntimeError):
    pass


class RenderStats(C.Structure):
    _fields_ = [
        ("rays_closest", C.c_uint64), ("rays_shadow", C.c_uint64), ("interior_steps", C.c_uint64), ("leaves", C.c_uint64),
        ("tri_tests", C.c_uint64), ("camera_samples", C.c_uint64), ("restarts", C.c_uint64),
        ("tree_build_seconds", C.c_double), ("upload_seconds", C.c_double), ("render_seconds", C.c_double),
        ("kd_nodes", C.c_uint32), ("kd_leaf_refs", C.c_uint32), ("kd_max_depth", C.c_uint32), ("n_triangles", C.c_uint32),
        ("scene_device_bytes", C.c_uint64),
    ]


PUTPIXEL = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float)
FLUSH = C.CFUNCTYPE(None, C.c_void_p, C.c_int)
EXCHANGE = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_uint64)      # yafaray_plane_exchange_t
AREA = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int)


class FilmHeader(C.Structure):
    """yafaray_film_header_t: the eleven words behind a film file's magic"""
    _fields_ = [("computer_node", C.c_uint32), ("base_sampling_offset", C.c_uint32), ("sampling_offset", C.c_uint32),
                ("w", C.c_int32), ("h", C.c_int32), ("cx0", C.c_int32), ("cx1", C.c_int32), ("cy0", C.c_int32), ("cy1", C.c_int32),
                ("n_passes", C.c_int32), ("n_aux", C.c_int32)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class Output(C.Structure):
    _fields_ = [("user", C.c_void_p), ("putPixel", PUTPIXEL), ("flush", FLUSH), ("flushArea", AREA), ("highlightArea", AREA)]


_lib = None

# every symbol include/yafaray_c_api.h and include/yafgpu.h declare (checked by tests/test_abi.py)
C_API_SYMBOLS = [
    "yafaray_createInterface", "yafaray_destroyInterface", "yafaray_getLastError", "yafaray_getVersion",
    "yafaray_startScene", "yafaray_startGeometry", "yafaray_endGeometry", "yafaray_getNextFreeId",
    "yafaray_startTriMesh", "yafaray_endTriMesh", "yafaray_addVertex", "yafaray_addNormal", "yafaray_addTriangle",
    "yafaray_smoothMesh", "yafaray_getMeshCornerNormals", "yafaray_getLights", "yafaray_getBackground", "yafaray_getSky", "yafaray_getCamera", "yafaray_getIntegratorAO", "yafaray_getMaskMaterial", "yafaray_getIesLight", "yafaray_getBlendMaterial", "yafaray_getMaterialTable", "yafaray_addTriangles",
    "yafaray_startTriMeshPtr", "yafaray_addVertexWithOrco", "yafaray_addUv", "yafaray_addTriangleWithUv",
    "yafaray_startCurveMesh", "yafaray_endCurveMesh", "yafaray_addCurves", "yafaray_getCurves", "yafaray_addInstance", "yafaray_getInstances",
    "yafaray_paramsSetColorArray", "yafaray_paramsSetMatrix", "yafaray_paramsSetMatrixD", "yafaray_setInputColorSpace",
    "yafaray_createObject", "yafaray_createVolumeRegion", "yafaray_createImageHandler",
    "yafaray_setLoggingAndBadgeSettings", "yafaray_setupRenderPasses", "yafaray_setInteractive", "yafaray_getRenderParameters",
    "yafaray_setConsoleVerbosityLevel", "yafaray_setLogVerbosityLevel", "yafaray_setParamsBadgePosition", "yafaray_getDrawParams",
    "yafaray_printDebug", "yafaray_printVerbose", "yafaray_printInfo", "yafaray_printParams", "yafaray_printWarning", "yafaray_printError",
    "yafaray_setOutput2",
    "yafaray_paramsSetPoint", "yafaray_paramsSetString", "yafaray_paramsSetBool", "yafaray_paramsSetInt",
    "yafaray_paramsSetFloat", "yafaray_paramsSetColor", "yafaray_paramsClearAll", "yafaray_paramsStartList",
    "yafaray_paramsPushList", "yafaray_paramsEndList",
    "yafaray_createTexture", "yafaray_createTextureFromMemory", "yafaray_getTextureImage",
    "yafaray_createLight", "yafaray_createMaterial", "yafaray_createCamera", "yafaray_createBackground",
    "yafaray_createIntegrator", "yafaray_clearAll", "yafaray_render", "yafaray_abort", "yafaray_getRenderedImage",
    "yafaray_getFilm", "yafaray_getRenderStats", "yafaray_setShard", "yafaray_setPlaneExchange", "yafaray_setSerialReplay", "yafaray_getRandState", "yafaray_setRandState", "yafaray_prepareRender",
    "yafaray_renderPassDevice", "yafaray_getRenderSize", "yafaray_loadXml", "yafaray_intersectRays", "yafaray_shadowRays", "yafaray_probe", "yafaray_setProfiling", "yafaray_getKernelProfile", "yafaray_setPassPipelining",
    "yafaray_commGetUniqueId", "yafaray_commCreate", "yafaray_commDestroy", "yafaray_commRank", "yafaray_commWorld", "yafaray_commLastError",
    "yafaray_commBackend", "yafaray_reduceFilm", "yafaray_allReduce", "yafaray_commExchange", "yafaray_setComm",
    "yafaray_setFilmPath", "yafaray_getFilmPath", "yafaray_getFilmResume", "yafaray_writeFilmFile", "yafaray_readFilmFile", "yafaray_filmLastError",
    "yafaray_createImageOutput", "yafaray_destroyImageOutput", "yafaray_imageOutputLastError", "yafaray_imageOutputCallbacks",
    "yafaray_filmToImage", "yafaray_writeImageFile",
]
GPU_ABI_SYMBOLS = [
    "yafgpu_last_error", "yafgpu_device_count", "yafgpu_set_device", "yafgpu_scene_create", "yafgpu_scene_destroy",
    "yafgpu_scene_info", "yafgpu_planes_bytes", "yafgpu_render_tiles", "yafgpu_film_combine", "yafgpu_render_to_host", "yafgpu_render_passes_to_host",
    "yafgpu_trace_closest", "yafgpu_trace_shadow", "yafgpu_trace_reservation", "yafgpu_trace_schedule", "yafgpu_scene_get_tree", "yafgpu_probe",
    "yafgpu_kdtree_build", "yafgpu_kdtree_build_device", "yafgpu_kdtree_info", "yafgpu_kdtree_get", "yafgpu_kdtree_destroy", "yafgpu_kdtree_treelets", "yafgpu_kdtree_tri_order",
    "yafgpu_set_profiling", "yafgpu_scene_set_pass_pipelining", "yafgpu_get_profile", "yafgpu_scene_set_abort_flag", "yafgpu_scene_set_exchange", "yafgpu_glibc_rand",
    "yafgpu_image_bytes", "yafgpu_film_to_image", "yafgpu_scene_film_to_image",
]


def load():
    """Load libyafaray_gpu.so.  No fallback: a missing library is an error."""
    global _lib
    if _lib is not None:
        return _lib
    p = lib_path()
    if not os.path.exists(p):
        raise YafaRayError(f"{p} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                           f"(libyafaray_amd/csrc/build.sh); there is no CPU fallback")
    L = C.CDLL(p)
    vp, cp, ci, cd, cf = C.c_void_p, C.c_char_p, C.c_int, C.c_double, C.c_float
    sig = {
        "yafaray_createInterface": (vp, []), "yafaray_destroyInterface": (None, [vp]),
        "yafaray_getLastError": (cp, [vp]), "yafaray_getVersion": (cp, []),
        "yafaray_startScene": (ci, [vp, ci]), "yafaray_startGeometry": (ci, [vp]), "yafaray_endGeometry": (ci, [vp]),
        "yafaray_getNextFreeId": (C.c_uint, [vp]),
        "yafaray_startTriMesh": (ci, [vp, C.c_uint, ci, ci, ci, ci, ci, ci]), "yafaray_endTriMesh": (ci, [vp]),
        "yafaray_addVertex": (ci, [vp, cd, cd, cd]), "yafaray_addNormal": (None, [vp, cd, cd, cd]),
        "yafaray_addTriangle": (ci, [vp, ci, ci, ci, vp]), "yafaray_smoothMesh": (ci, [vp, C.c_uint, cd]),
        "yafaray_getMeshCornerNormals": (ci, [vp, C.c_uint, C.POINTER(cf), ci]),
        "yafaray_getLights": (ci, [vp, vp, ci]),
        "yafaray_getBackground": (ci, [vp, cp, vp]),
        "yafaray_getSky": (ci, [vp, cp, vp]),
        "yafaray_getCamera": (ci, [vp, cp, vp]),
        "yafaray_getIntegratorAO": (ci, [vp, cp, C.POINTER(ci), C.POINTER(ci), C.POINTER(cf), C.POINTER(cf)]),
        "yafaray_getMaskMaterial": (ci, [vp, cp, vp]),
        "yafaray_getBlendMaterial": (ci, [vp, cp, vp]),
        "yafaray_getIesLight": (ci, [vp, cp, C.POINTER(ci), C.POINTER(ci), C.POINTER(ci), C.POINTER(cf), C.POINTER(cf), C.POINTER(cf), ci]),
        "yafaray_getMaterialTable": (ci, [vp, vp, ci]),
        "yafaray_addTriangles": (ci, [vp, ci, C.POINTER(cf), ci, C.POINTER(ci), vp]),
        "yafaray_startTriMeshPtr": (ci, [vp, C.POINTER(C.c_uint), ci, ci, ci, ci, ci, ci]),
        "yafaray_addVertexWithOrco": (ci, [vp, cd, cd, cd, cd, cd, cd]), "yafaray_addUv": (ci, [vp, cf, cf]),
        "yafaray_addTriangleWithUv": (ci, [vp, ci, ci, ci, ci, ci, ci, vp]),
        "yafaray_startCurveMesh": (ci, [vp, C.c_uint, ci, ci]), "yafaray_endCurveMesh": (ci, [vp, vp, cf, cf, cf]),
        "yafaray_addCurves": (ci, [vp, ci, C.POINTER(ci), C.POINTER(cf), vp, cf, cf, cf, C.POINTER(C.c_uint)]),
        "yafaray_getCurves": (ci, [vp, vp, ci, C.POINTER(ci)]),
        "yafaray_addInstance": (ci, [vp, C.c_uint, C.POINTER(cf)]), "yafaray_getInstances": (ci, [vp, vp, ci]),
        "yafaray_paramsSetColorArray": (None, [vp, cp, C.POINTER(cf), ci]), "yafaray_paramsSetMatrix": (None, [vp, cp, C.POINTER(cf), ci]),
        "yafaray_paramsSetMatrixD": (None, [vp, cp, C.POINTER(cd), ci]), "yafaray_setInputColorSpace": (None, [vp, cp, cf]),
        "yafaray_createObject": (C.c_uint, [vp, cp]), "yafaray_createVolumeRegion": (vp, [vp, cp]), "yafaray_createImageHandler": (vp, [vp, cp, ci]),
        "yafaray_setLoggingAndBadgeSettings": (ci, [vp]), "yafaray_setupRenderPasses": (ci, [vp]), "yafaray_setInteractive": (ci, [vp, ci]),
        "yafaray_getRenderParameters": (ci, [vp, C.c_char_p, ci]),
        "yafaray_setConsoleVerbosityLevel": (None, [vp, cp]), "yafaray_setLogVerbosityLevel": (None, [vp, cp]),
        "yafaray_setParamsBadgePosition": (None, [vp, cp]), "yafaray_getDrawParams": (ci, [vp]),
        "yafaray_printDebug": (None, [vp, cp]), "yafaray_printVerbose": (None, [vp, cp]), "yafaray_printInfo": (None, [vp, cp]),
        "yafaray_printParams": (None, [vp, cp]), "yafaray_printWarning": (None, [vp, cp]), "yafaray_printError": (None, [vp, cp]),
        "yafaray_setOutput2": (None, [vp, C.POINTER(Output)]),
        "yafaray_paramsSetPoint": (None, [vp, cp, cd, cd, cd]), "yafaray_paramsSetString": (None, [vp, cp, cp]),
        "yafaray_paramsSetBool": (None, [vp, cp, ci]), "yafaray_paramsSetInt": (None, [vp, cp, ci]),
        "yafaray_paramsSetFloat": (None, [vp, cp, cd]), "yafaray_paramsSetColor": (None, [vp, cp, cf, cf, cf, cf]),
        "yafaray_paramsClearAll": (None, [vp]), "yafaray_paramsStartList": (None, [vp]),
        "yafaray_paramsPushList": (None, [vp]), "yafaray_paramsEndList": (None, [vp]),
        "yafaray_createLight": (vp, [vp, cp]), "yafaray_createMaterial": (vp, [vp, cp]),
        "yafaray_createTexture": (vp, [vp, cp]), "yafaray_createTextureFromMemory": (vp, [vp, cp, ci, ci, C.POINTER(C.c_float)]),
        "yafaray_getTextureImage": (ci, [vp, cp, C.POINTER(ci), C.POINTER(ci), C.POINTER(C.c_float), ci]),
        "yafaray_createCamera": (vp, [vp, cp]), "yafaray_createBackground": (vp, [vp, cp]),
        "yafaray_createIntegrator": (vp, [vp, cp]), "yafaray_clearAll": (None, [vp]),
        "yafaray_render": (ci, [vp, C.POINTER(Output), vp]), "yafaray_abort": (None, [vp]),
        "yafaray_getRenderedImage": (ci, [vp, ci, C.POINTER(Output)]),
        "yafaray_getFilm": (ci, [vp, C.POINTER(cf), ci, ci]), "yafaray_getRenderStats": (ci, [vp, C.POINTER(RenderStats)]),
        "yafaray_setShard": (None, [vp, ci, ci]), "yafaray_setPlaneExchange": (None, [vp, EXCHANGE, vp]), "yafaray_setSerialReplay": (None, [vp, ci]), "yafaray_prepareRender": (ci, [vp]),
        "yafaray_renderPassDevice": (ci, [vp, vp, vp, vp]), "yafaray_getRenderSize": (ci, [vp, C.POINTER(ci), C.POINTER(ci)]),
        "yafaray_loadXml": (ci, [vp, cp]), "yafaray_getRandState": (None, [vp, C.POINTER(ci), C.POINTER(ci)]), "yafaray_setRandState": (None, [vp, ci, ci]),
        "yafaray_intersectRays": (ci, [vp, ci, C.POINTER(cf), C.POINTER(ci), C.POINTER(cf), C.POINTER(cf)]),
        "yafaray_shadowRays": (ci, [vp, ci, C.POINTER(cf), C.POINTER(ci)]),
        "yafaray_probe": (ci, [vp, ci, ci, C.POINTER(cf), ci, C.POINTER(cf), ci]),
        "yafaray_setProfiling": (ci, [vp, ci]),
        "yafaray_setPassPipelining": (ci, [vp, ci]),
        "yafaray_getKernelProfile": (ci, [vp, C.POINTER(cd), C.POINTER(C.c_uint64)]),
        "yafaray_commGetUniqueId": (ci, [C.c_char_p]), "yafaray_commCreate": (vp, [C.c_char_p, ci, ci, ci]), "yafaray_commDestroy": (None, [vp]),
        "yafaray_commRank": (ci, [vp]), "yafaray_commWorld": (ci, [vp]), "yafaray_commLastError": (cp, []), "yafaray_commBackend": (cp, []),
        "yafaray_reduceFilm": (ci, [vp, vp, C.c_uint64, ci, vp]), "yafaray_allReduce": (ci, [vp, vp, C.c_uint64, vp]),
        "yafaray_commExchange": (ci, [vp, vp, C.c_uint64]), "yafaray_setComm": (None, [vp, vp]),
        "yafaray_setFilmPath": (None, [vp, cp]), "yafaray_getFilmPath": (cp, [vp]),
        "yafaray_getFilmResume": (None, [vp, C.POINTER(ci), C.POINTER(C.c_uint), C.POINTER(C.c_uint)]),
        "yafaray_writeFilmFile": (ci, [cp, C.POINTER(FilmHeader), C.POINTER(cf)]),
        "yafaray_readFilmFile": (ci, [cp, C.POINTER(FilmHeader), C.POINTER(cf), C.c_uint64]), "yafaray_filmLastError": (cp, []),
        "yafaray_createImageOutput": (vp, [vp, vp, cp, ci, ci]), "yafaray_destroyImageOutput": (None, [vp]),
        "yafaray_imageOutputLastError": (cp, [vp]), "yafaray_imageOutputCallbacks": (C.POINTER(Output), [vp]),
        "yafaray_filmToImage": (ci, [C.POINTER(cf), ci, ci, cp, cf, ci, ci, vp]), "yafaray_writeImageFile": (ci, [cp, cp, ci, ci, ci, vp]),
        "yafgpu_last_error": (cp, []), "yafgpu_device_count": (ci, []), "yafgpu_set_device": (ci, [ci]),
        "yafgpu_planes_bytes": (C.c_uint64, [ci, ci]),
        "yafgpu_film_combine": (ci, [vp, vp, ci, ci, vp]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


def _b(s):
    return s.encode() if isinstance(s, str) else s


class Interface:
    """yafaray4::Interface.  See include/yafaray_c_api.h for the per-method reference citations."""

    def __init__(self, strict=True):
        self._L = load()
        self._h = self._L.yafaray_createInterface()
        self.strict = strict
        self._keep = []

    # -- plumbing
    def close(self):
        if self._h:
            self._L.yafaray_destroyInterface(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def getLastError(self):
        return self._L.yafaray_getLastError(self._h).decode()

    def getVersion(self):
        return self._L.yafaray_getVersion().decode()

    def _ok(self, r, what):
        if not r and self.strict:
            raise YafaRayError(f"{what}: {self.getLastError()}")
        return bool(r)

    def _obj(self, r, what):
        if not r and self.strict:
            raise YafaRayError(f"{what}: {self.getLastError()}")
        return r

    # -- scene
    def startScene(self, type=0):
        return self._ok(self._L.yafaray_startScene(self._h, type), "startScene")

    def startGeometry(self):
        return self._ok(self._L.yafaray_startGeometry(self._h), "startGeometry")

    def endGeometry(self):
        return self._ok(self._L.yafaray_endGeometry(self._h), "endGeometry")

    def getNextFreeId(self):
        return self._L.yafaray_getNextFreeId(self._h)

    def startTriMesh(self, id, vertices, triangles, has_orco, has_uv=False, type=0, obj_pass_index=0):
        return self._ok(self._L.yafaray_startTriMesh(self._h, id, vertices, triangles, int(has_orco), int(has_uv), type,
                                                     obj_pass_index), "startTriMesh")

    def endTriMesh(self):
        return self._ok(self._L.yafaray_endTriMesh(self._h), "endTriMesh")

    def addVertex(self, x, y, z):
        return self._L.yafaray_addVertex(self._h, x, y, z)

    def addNormal(self, nx, ny, nz):
        self._L.yafaray_addNormal(self._h, nx, ny, nz)

    def addTriangle(self, a, b, c, mat):
        return self._ok(self._L.yafaray_addTriangle(self._h, a, b, c, mat), "addTriangle")

    def startTriMeshPtr(self, vertices, triangles, has_orco, has_uv=False, type=0, obj_pass_index=0):
        """-> the id the scene picked (the reference's SWIG typemap returns it the same way)"""
        mid = C.c_uint(0)
        ok = self._ok(self._L.yafaray_startTriMeshPtr(self._h, C.byref(mid), vertices, triangles, int(has_orco), int(has_uv), type, obj_pass_index), "startTriMeshPtr")
        return mid.value if ok else 0

    def addVertexWithOrco(self, x, y, z, ox, oy, oz):
        return self._L.yafaray_addVertexWithOrco(self._h, x, y, z, ox, oy, oz)

    def addUv(self, u, v):
        return self._L.yafaray_addUv(self._h, u, v)

    def addTriangleWithUv(self, a, b, c, uv_a, uv_b, uv_c, mat):
        return self._ok(self._L.yafaray_addTriangleWithUv(self._h, a, b, c, uv_a, uv_b, uv_c, mat), "addTriangle")

    def startCurveMesh(self, id, vertices, obj_pass_index=0):
        """Scene::startCurveMesh: opens a strand under `id`; addVertex gives its points, endCurveMesh closes it"""
        return self._ok(self._L.yafaray_startCurveMesh(self._h, id, vertices, obj_pass_index), "startCurveMesh")

    def endCurveMesh(self, mat, strand_start, strand_end, strand_shape):
        """Scene::endCurveMesh: root radius, tip radius and shape exponent; the 6 * (n - 1) + 2 triangles are made on the device at scene set-up"""
        return self._ok(self._L.yafaray_endCurveMesh(self._h, mat, strand_start, strand_end, strand_shape), "endCurveMesh")

    def addCurves(self, n_points, points, mat, strand_start, strand_end, strand_shape):
        """many strands in one call (the loop of getNextFreeId / startCurveMesh / addVertex / endCurveMesh): n_points[k] points for curve k,
        taken in turn from points (sum(n_points), 3).  -> the object ids as uint32, or None when a call of the loop was refused"""
        cnt = np.ascontiguousarray(n_points, dtype=np.int32).reshape(-1)
        pts = np.ascontiguousarray(points, dtype=np.float32).reshape(-1)
        if cnt.size and (cnt.min() < 0 or int(cnt.sum()) * 3 != pts.size):
            raise ValueError("addCurves: points must hold sum(n_points) xyz triples")
        ids = np.zeros(max(cnt.size, 1), dtype=np.uint32)
        ok = self._ok(self._L.yafaray_addCurves(self._h, cnt.size, cnt.ctypes.data_as(C.POINTER(C.c_int)), pts.ctypes.data_as(C.POINTER(C.c_float)), mat,
                                                strand_start, strand_end, strand_shape, ids.ctypes.data_as(C.POINTER(C.c_uint))), "addCurves")
        return ids[:cnt.size] if ok else None

    def getCurves(self):
        """what endCurveMesh stored, in object-id order: a list of dicts with the curve's id, material index, the three strand parameters as
        float32 and `points`, float32 (n, 5): x y z and the two extrusion scales h, s"""
        need = C.c_int(0)
        n = self._L.yafaray_getCurves(self._h, None, 0, C.byref(need))
        w = np.zeros(max(need.value, 1), dtype=np.int32)
        self._L.yafaray_getCurves(self._h, w.ctypes.data_as(C.c_void_p), need.value, None)
        out, at = [], 0
        for _ in range(n):
            npts = int(w[at + 1])
            f = w[at + 3:at + 6].view(np.float32)
            out.append({"id": int(w[at]) & 0xffffffff, "material": int(w[at + 2]), "strand_start": f[0], "strand_end": f[1], "strand_shape": f[2],
                        "points": w[at + 6:at + 6 + 5 * npts].view(np.float32).reshape(npts, 5).copy()})
            at += 6 + 5 * npts
        return out

    def addInstance(self, base_object_id, obj_to_world):
        """Scene::addInstance: the base mesh's triangles under obj_to_world (4 x 4, row major) as one more object; None passes a null matrix"""
        m = None if obj_to_world is None else (C.c_float * 16)(*[float(x) for x in np.asarray(obj_to_world, np.float32).reshape(16)])
        return self._ok(self._L.yafaray_addInstance(self._h, base_object_id, m), "addInstance")

    def getInstances(self):
        """what addInstance stored, in object-id order: a list of dicts with the instance's own id, its base, the flags it copied from the
        base at the call and the matrix as float32 (4, 4)"""
        n = self._L.yafaray_getInstances(self._h, None, 0)
        out = np.zeros((max(n, 1), 22), dtype=np.int32)
        self._L.yafaray_getInstances(self._h, out.ctypes.data_as(C.c_void_p), n)
        return [{"id": int(r[0]), "base": int(r[1]), "has_orco": bool(r[2]), "has_uv": bool(r[3]), "is_smooth": bool(r[4]), "normals_exported": bool(r[5]),
                 "matrix": r[6:].view(np.float32).reshape(4, 4).copy()} for r in out[:n]]

    def createObject(self, name):
        return self._obj(self._L.yafaray_createObject(self._h, _b(name)), "createObject")

    def createVolumeRegion(self, name):
        return self._obj(self._L.yafaray_createVolumeRegion(self._h, _b(name)), "createVolumeRegion")

    def createImageHandler(self, name, add_to_table=True):
        """type "tga" | "hdr" | "pic" | "png", width, height, alpha_channel, for_output from the current parameters -> a handle for ImageOutput"""
        return self._obj(self._L.yafaray_createImageHandler(self._h, _b(name), int(add_to_table)), "createImageHandler")

    def createImageOutput(self, handler, path, border_x=0, border_y=0):
        """-> an ImageOutput for render(output=...) / setOutput2, or None when it is refused (strict: raises)"""
        h = self._obj(self._L.yafaray_createImageOutput(self._h, handler, _b(os.fspath(path)), int(border_x), int(border_y)), "createImageOutput")
        return ImageOutput(self, h) if h else None

    def _output_table(self, output, keep):
        """the yafaray_output_t for `output`: an ImageOutput's own table, or thunks around an object with putPixel(view, x, y, rgba) [and flush(view)]"""
        if output is None:
            return None
        if isinstance(output, ImageOutput):
            return output.callbacks()
        out = Output()
        pp = PUTPIXEL(lambda u, v, x, y, r, g, b, a: int(bool(output.putPixel(v, x, y, (r, g, b, a)))))
        fl = FLUSH(lambda u, v: output.flush(v) if hasattr(output, "flush") else None)
        keep[:] = [pp, fl, out]
        out.putPixel = pp
        out.flush = fl
        return C.pointer(out)

    def setOutput2(self, output):
        """Interface::setOutput2: a second output, fed in color_space2 / gamma2; None detaches it"""
        self._keep2 = []
        self._output2 = output
        self._L.yafaray_setOutput2(self._h, self._output_table(output, self._keep2))

    def setLoggingAndBadgeSettings(self):
        return self._ok(self._L.yafaray_setLoggingAndBadgeSettings(self._h), "setLoggingAndBadgeSettings")

    def setupRenderPasses(self):
        return self._ok(self._L.yafaray_setupRenderPasses(self._h), "setupRenderPasses")

    def setInteractive(self, interactive):
        return bool(self._L.yafaray_setInteractive(self._h, int(interactive)))

    def getRenderParameters(self):
        """the render ParamMap as a dict of strings"""
        n = self._L.yafaray_getRenderParameters(self._h, None, 0)
        buf = C.create_string_buffer(n + 1)
        self._L.yafaray_getRenderParameters(self._h, buf, n + 1)
        return dict(line.split("=", 1) for line in buf.value.decode().splitlines() if "=" in line)

    def setConsoleVerbosityLevel(self, level):
        self._L.yafaray_setConsoleVerbosityLevel(self._h, _b(level))

    def setLogVerbosityLevel(self, level):
        self._L.yafaray_setLogVerbosityLevel(self._h, _b(level))

    def setParamsBadgePosition(self, position="none"):
        self._L.yafaray_setParamsBadgePosition(self._h, _b(position))

    def getDrawParams(self):
        return bool(self._L.yafaray_getDrawParams(self._h))

    def printInfo(self, msg):
        self._L.yafaray_printInfo(self._h, _b(msg))

    def printWarning(self, msg):
        self._L.yafaray_printWarning(self._h, _b(msg))

    def printError(self, msg):
        self._L.yafaray_printError(self._h, _b(msg))

    def setInputColorSpace(self, color_space_string, gamma_val):
        self._L.yafaray_setInputColorSpace(self._h, _b(color_space_string), gamma_val)

    def paramsSetMatrix(self, name, m, transpose=False):
        a = (C.c_float * 16)(*[float(x) for x in np.asarray(m, np.float32).reshape(16)])
        self._L.yafaray_paramsSetMatrix(self._h, _b(name), a, int(transpose))

    def paramsSetMemMatrix(self, name, m, transpose=False):
        self.paramsSetMatrix(name, m, transpose)

    def addTriangles(self, verts, indices, mat):
        v = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
        i = np.ascontiguousarray(indices, dtype=np.int32).reshape(-1, 3)
        return self._ok(self._L.yafaray_addTriangles(self._h, v.shape[0], v.ctypes.data_as(C.POINTER(C.c_float)), i.shape[0],
                                                     i.ctypes.data_as(C.POINTER(C.c_int)), mat), "addTriangles")

    def smoothMesh(self, id, angle):
        return self._ok(self._L.yafaray_smoothMesh(self._h, id, angle), "smoothMesh")

    def getMeshCornerNormals(self, id, n_tris):
        out = np.zeros((n_tris, 3, 3), dtype=np.float32)
        self._ok(self._L.yafaray_getMeshCornerNormals(self._h, id, out.ctypes.data_as(C.POINTER(C.c_float)), out.size), "getMeshCornerNormals")
        return out

    def getLights(self):
        """the scene's enabled lights in Scene::addLight order, as the device gets them: one row of the 34 words of a yafgpu_light
        (include/yafgpu.h) each, as float32 (the int fields type / samples / cast_shadows / infinite are words 0-3: view them as int32)"""
        n = self._L.yafaray_getLights(self._h, None, 0)
        out = np.zeros((max(n, 0), 34), dtype=np.float32)
        if n > 0:
            self._L.yafaray_getLights(self._h, out.ctypes.data_as(C.c_void_p), n)
        return out

    def getBackground(self, name):
        """the yafgpu_background record (include/yafgpu.h) createBackground made under `name`, as a dict"""
        out = np.zeros(12, dtype=np.float32)
        self._ok(self._L.yafaray_getBackground(self._h, _b(name), out.ctypes.data_as(C.c_void_p)), "getBackground")
        i = out.view(np.int32)
        return {"kind": int(i[0]), "color": out[1:4].copy(), "power": out[4], "texture": int(i[5]), "projection": int(i[6]),
                "rotation": out[7], "sin_r": out[8], "cos_r": out[9], "has_ibl": int(i[10]), "shoots_caustic": int(i[11])}

    def getSky(self, name):
        """the yafgpu_sky record (include/yafgpu.h) createBackground made under `name`, as a dict: a gradientback's four colours
        (float32, already times power) and a sunsky's constants (float64); zeros for every other type of background"""
        out = np.zeros(30, dtype=np.float64)                  # 240 bytes: 20 float words, then 20 doubles
        self._ok(self._L.yafaray_getSky(self._h, _b(name), out.ctypes.data_as(C.c_void_p)), "getSky")
        f, d = out[:10].view(np.float32), out[10:]
        return {"horizon": f[0:3].copy(), "zenith": f[3:6].copy(), "horizon_ground": f[6:9].copy(), "zenith_ground": f[9:12].copy(),
                "power": f[12], "from": f[13:16].copy(), "turbidity": f[16],
                "theta_s": d[0], "phi_s": d[1], "zenith_x": d[2], "zenith_y": d[3], "zenith_Y": d[4],
                "perez_x": d[5:10].copy(), "perez_y": d[10:15].copy(), "perez_Y": d[15:20].copy()}

    CAMERA_WORDS = 69
    CAMERA_INT_FIELDS = ("resx", "resy", "bokeh_type", "bokeh_bias", "type", "circular", "projection")

    def getCamera(self, name):
        """the yafgpu_camera record (include/yafgpu.h) createCamera made under `name`, as a dict: float32 arrays / scalars, ints
        for the fields of CAMERA_INT_FIELDS"""
        out = np.zeros(self.CAMERA_WORDS, dtype=np.float32)
        self._ok(self._L.yafaray_getCamera(self._h, _b(name), out.ctypes.data_as(C.c_void_p)), "getCamera")
        layout = [("position", 3), ("vto", 3), ("vup", 3), ("vright", 3), ("near_p", 3), ("near_n", 3), ("far_p", 3), ("far_n", 3),
                  ("resx", 1), ("resy", 1), ("aperture", 1), ("dof_distance", 1), ("bokeh_type", 1), ("bokeh_bias", 1), ("bokeh_rotation", 1),
                  ("dof_rt", 3), ("dof_up", 3), ("ls", 16), ("cam_x", 3), ("cam_y", 3), ("cam_z", 3), ("focal_distance", 1), ("aspect_ratio", 1),
                  ("type", 1), ("focal_length", 1), ("max_radius", 1), ("circular", 1), ("projection", 1)]
        rec, at, i = {}, 0, out.view(np.int32)
        for field, n in layout:
            if field in self.CAMERA_INT_FIELDS:
                rec[field] = int(i[at])
            else:
                rec[field] = out[at:at + n].copy() if n > 1 else out[at]
            at += n
        assert at == self.CAMERA_WORDS
        return rec

    def getIntegratorAO(self, name):
        """the ambient occlusion settings createIntegrator parsed for the integrator `name`, as a dict"""
        do_ao, samples, dist = C.c_int(0), C.c_int(0), C.c_float(0.0)
        col = (C.c_float * 3)()
        self._ok(self._L.yafaray_getIntegratorAO(self._h, _b(name), C.byref(do_ao), C.byref(samples), C.byref(dist), col), "getIntegratorAO")
        return {"do_AO": bool(do_ao.value), "AO_samples": int(samples.value), "AO_distance": np.float32(dist.value),
                "AO_color": np.array(list(col), dtype=np.float32)}

    def getMaskMaterial(self, name):
        """what createMaterial parsed for the mask_mat `name`, as a dict: the indices of material1 / material2 in creation order, the
        threshold as the float32 it is kept as, the mask node's slot among the mask's n_nodes nodes, and the material-level fields"""
        out = np.zeros(8, dtype=np.int32)
        self._ok(self._L.yafaray_getMaskMaterial(self._h, _b(name), out.ctypes.data_as(C.c_void_p)), "getMaskMaterial")
        return {"material1": int(out[0]), "material2": int(out[1]), "threshold": out.view(np.float32)[2], "mask_slot": int(out[3]), "n_nodes": int(out[4]),
                "receive_shadows": bool(out[5]), "visibility": int(out[6]), "bsdf_flags": int(out[7]) & 0xffffffff}

    def getIesLight(self, name):
        """what createLight parsed from the file of the ieslight `name`, as a dict: the photometric type, the two angle maps in degrees, the
        table (n_hor, n_vert) as read, max_rad (1 / its largest value) and the largest vertical angle in radians, all float32"""
        t, nh, nv, mr, mv = C.c_int(0), C.c_int(0), C.c_int(0), C.c_float(0), C.c_float(0)
        self._ok(self._L.yafaray_getIesLight(self._h, _b(name), C.byref(t), C.byref(nh), C.byref(nv), C.byref(mr), C.byref(mv), None, 0), "getIesLight")
        n_hor, n_vert = nh.value, nv.value
        out = np.zeros(n_hor + n_vert + n_hor * n_vert, dtype=np.float32)
        self._ok(self._L.yafaray_getIesLight(self._h, _b(name), None, None, None, None, None, out.ctypes.data_as(C.POINTER(C.c_float)), out.size), "getIesLight")
        return {"type": t.value, "hor": out[:n_hor].copy(), "vert": out[n_hor:n_hor + n_vert].copy(),
                "table": out[n_hor + n_vert:].reshape(n_hor, n_vert).copy(), "max_rad": np.float32(mr.value), "max_v_angle": np.float32(mv.value)}

    def getBlendMaterial(self, name):
        """what createMaterial parsed for the blend_mat `name`, as a dict: the indices of material1 / material2 in creation order, blend_value
        as the float32 it is kept as, whether a shader node drives the blend, that node's slot among the blend's n_nodes nodes (-1 without
        one), and the material-level fields: the blend's own receive_shadows and visibility, the union of the sub-materials' flags and the
        larger of their additional depths"""
        out = np.zeros(10, dtype=np.int32)
        self._ok(self._L.yafaray_getBlendMaterial(self._h, _b(name), out.ctypes.data_as(C.c_void_p)), "getBlendMaterial")
        return {"material1": int(out[0]), "material2": int(out[1]), "blend_value": out.view(np.float32)[2], "node_driven": bool(out[3]), "mask_slot": int(out[4]),
                "n_nodes": int(out[5]), "receive_shadows": bool(out[6]), "visibility": int(out[7]), "bsdf_flags": int(out[8]) & 0xffffffff, "additional_depth": int(out[9])}

    MATERIAL_WORDS = 96
    # word offsets of the yafgpu_material fields (include/yafgpu.h) that tests of the material table read
    MATERIAL_FIELDS = {"type": 0, "visibility": 1, "receive_shadows": 2, "flat": 3, "bsdf_flags": 4, "c_index": 10, "transmit_filter": 27, "is_transparent": 30,
                       "has_vol_i": 61, "beer_sigma": 62, "node_first": 65, "n_nodes": 66, "sh_diffuse": 67, "bump_first": 79, "n_bump": 80,
                       "additional_depth": 82, "transp_bias_factor": 83, "transp_bias_mult": 84}

    def getMaterialTable(self):
        """the material table as the device scene gets it: one row of the 96 words of a yafgpu_material (include/yafgpu.h) per record, as
        int32 (view a float field as float32) — the materials in creation order, then two hidden clones per mask_mat and per blend_mat"""
        n = self._L.yafaray_getMaterialTable(self._h, None, 0)
        out = np.zeros((max(n, 0), self.MATERIAL_WORDS), dtype=np.int32)
        if n > 0:
            self._L.yafaray_getMaterialTable(self._h, out.ctypes.data_as(C.c_void_p), n)
        return out

    # -- params
    def paramsSetPoint(self, name, x, y, z):
        self._L.yafaray_paramsSetPoint(self._h, _b(name), x, y, z)

    def paramsSetString(self, name, s):
        self._L.yafaray_paramsSetString(self._h, _b(name), _b(s))

    def paramsSetBool(self, name, b):
        self._L.yafaray_paramsSetBool(self._h, _b(name), int(b))

    def paramsSetInt(self, name, i):
        self._L.yafaray_paramsSetInt(self._h, _b(name), int(i))

    def paramsSetFloat(self, name, f):
        self._L.yafaray_paramsSetFloat(self._h, _b(name), float(f))

    def paramsSetColor(self, name, r, g, b, a=1.0):
        self._L.yafaray_paramsSetColor(self._h, _b(name), r, g, b, a)

    def paramsClearAll(self):
        self._L.yafaray_paramsClearAll(self._h)

    def paramsStartList(self):
        self._L.yafaray_paramsStartList(self._h)

    def paramsPushList(self):
        self._L.yafaray_paramsPushList(self._h)

    def paramsEndList(self):
        self._L.yafaray_paramsEndList(self._h)

    def paramsSet(self, d):
        """Convenience: fill the ParamMap from a dict, typed like the XML grammar (import_xml.cc:273-318):
        str -> sval, bool -> bval, int -> ival, float -> fval, 3-tuple -> point, ('color', r,g,b[,a]) -> colour."""
        for k, v in d.items():
            if isinstance(v, str):
                self.paramsSetString(k, v)
            elif isinstance(v, bool):
                self.paramsSetBool(k, v)
            elif isinstance(v, (int, np.integer)):
                self.paramsSetInt(k, v)
            elif isinstance(v, (float, np.floating)):
                self.paramsSetFloat(k, v)
            elif isinstance(v, tuple) and len(v) in (4, 5) and v[0] == "color":
                self.paramsSetColor(k, *[float(t) for t in v[1:]])
            elif len(v) == 3:
                self.paramsSetPoint(k, float(v[0]), float(v[1]), float(v[2]))
            else:
                raise TypeError(f"parameter {k}: {v!r}")

    # -- factories
    def createLight(self, name):
        return self._obj(self._L.yafaray_createLight(self._h, _b(name)), "createLight")

    def createMaterial(self, name):
        return self._obj(self._L.yafaray_createMaterial(self._h, _b(name)), "createMaterial")

    def createTexture(self, name):
        return self._obj(self._L.yafaray_createTexture(self._h, _b(name)), "createTexture")

    def createTextureFromMemory(self, name, texels):
        """texels: (height, width, 4) float32, as the reference's ImageHandler::getPixel would return them"""
        import numpy as np
        px = np.ascontiguousarray(texels, dtype=np.float32)
        return self._obj(self._L.yafaray_createTextureFromMemory(self._h, _b(name), px.shape[1], px.shape[0], px.ctypes.data_as(C.POINTER(C.c_float))), "createTextureFromMemory")

    def getTextureImage(self, name):
        import numpy as np
        w, h = C.c_int(0), C.c_int(0)
        self._ok(self._L.yafaray_getTextureImage(self._h, _b(name), C.byref(w), C.byref(h), None, 0), "getTextureImage")
        px = np.zeros((h.value, w.value, 4), np.float32)
        self._ok(self._L.yafaray_getTextureImage(self._h, _b(name), C.byref(w), C.byref(h), px.ctypes.data_as(C.POINTER(C.c_float)), px.size), "getTextureImage")
        return px

    def createCamera(self, name):
        return self._obj(self._L.yafaray_createCamera(self._h, _b(name)), "createCamera")

    def createBackground(self, name):
        return self._obj(self._L.yafaray_createBackground(self._h, _b(name)), "createBackground")

    def createIntegrator(self, name):
        return self._obj(self._L.yafaray_createIntegrator(self._h, _b(name)), "createIntegrator")

    def clearAll(self):
        self._L.yafaray_clearAll(self._h)

    # -- render
    def render(self, output=None, progress=None):
        """output: None, an ImageOutput (the file is written from the device film) or an object with putPixel(view, x, y, rgba) [and flush(view)]"""
        self._keep = []
        return self._ok(self._L.yafaray_render(self._h, self._output_table(output, self._keep), None), "render")

    def getRenderedImage(self, output, num_view=0):
        """Interface::getRenderedImage: the last render's image once more, into `output` (and the second output, when one is set)"""
        keep = []
        return self._ok(self._L.yafaray_getRenderedImage(self._h, num_view, self._output_table(output, keep)), "getRenderedImage")

    def abort(self):
        self._L.yafaray_abort(self._h)

    def loadXml(self, path):
        return self._ok(self._L.yafaray_loadXml(self._h, _b(path)), "loadXml")

    # -- additions (measurement / multi-GPU)
    def setShard(self, index, count):
        self._L.yafaray_setShard(self._h, index, count)

    def setPlaneExchange(self, fn):
        """fn(device_pointer: int, n_floats: int): sum that float32 device array over all ranks in place (see
        libyafaray_amd.parallel.plane_exchange); None detaches it"""
        if fn is None:
            self._exchange = None
            self._L.yafaray_setPlaneExchange(self._h, EXCHANGE(0), None)
            return

        def thunk(user, ptr, n):
            try:
                fn(int(ptr or 0), int(n))
                return 0
            except Exception as e:            # an exception must not unwind through the C caller
                print(f"plane exchange failed: {e!r}", file=sys.stderr)
                return 1
        self._exchange = EXCHANGE(thunk)
        self._L.yafaray_setPlaneExchange(self._h, self._exchange, None)

    def setComm(self, comm):
        """attach a FilmComm (libyafaray_amd.parallel): plane / light-counter exchanges of a sharded render run over its RCCL
        communicator inside the library; None detaches"""
        self._comm = comm
        self._L.yafaray_setComm(self._h, comm.handle if comm is not None else None)

    def setFilmPath(self, path):
        """the image output path without extension, e.g. "out/frame0007": with it the render parameter film_save_load ("save" |
        "load-save") writes and loads "<path> - node NNNN.film" (include/yafaray_c_api.h); None or "" detaches it"""
        self._L.yafaray_setFilmPath(self._h, None if path is None else _b(os.fspath(path)))

    def getFilmPath(self):
        return self._L.yafaray_getFilmPath(self._h).decode()

    def getFilmResume(self):
        """what the last render loaded -> (film files loaded, merged sampling_offset, merged base_sampling_offset)"""
        n, so, bo = C.c_int(0), C.c_uint(0), C.c_uint(0)
        self._L.yafaray_getFilmResume(self._h, C.byref(n), C.byref(so), C.byref(bo))
        return n.value, so.value, bo.value

    def setSerialReplay(self, on):
        self._L.yafaray_setSerialReplay(self._h, int(bool(on)))

    def getRandState(self):
        """(srand seed, values consumed since) of the libc stream the tile seeds continue — what the oracle needs to
        render the same scene (`rand_srand`, `rand_skip`)"""
        a, b = C.c_int(), C.c_int()
        self._L.yafaray_getRandState(self._h, C.byref(a), C.byref(b))
        return a.value, b.value

    def setRandState(self, srand_seed, skip=0):
        """the embedder called libc srand(seed) itself after building the scene (and drew `skip` values): tile seeds continue there"""
        self._L.yafaray_setRandState(self._h, int(srand_seed), int(skip))

    def prepareRender(self):
        return self._ok(self._L.yafaray_prepareRender(self._h), "prepareRender")

    def getRenderSize(self):
        w, h = C.c_int(), C.c_int()
        self._ok(self._L.yafaray_getRenderSize(self._h, C.byref(w), C.byref(h)), "getRenderSize")
        return w.value, h.value

    def renderPassDevice(self, d_planes, d_counters=0, stream=0):
        return self._ok(self._L.yafaray_renderPassDevice(self._h, C.c_void_p(d_planes), C.c_void_p(d_counters or None),
                                                         C.c_void_p(stream or None)), "renderPassDevice")

    def intersectRays(self, rays):
        """rays (n,8) float32 -> (tri (n,) int32, t (n,), bary (n,3))"""
        r = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 8)
        n = r.shape[0]
        tri = np.zeros(n, np.int32); t = np.zeros(n, np.float32); bary = np.zeros((n, 3), np.float32)
        fp = C.POINTER(C.c_float)
        self._ok(self._L.yafaray_intersectRays(self._h, n, r.ctypes.data_as(fp), tri.ctypes.data_as(C.POINTER(C.c_int)),
                                               t.ctypes.data_as(fp), bary.ctypes.data_as(fp)), "intersectRays")
        return tri, t, bary

    def shadowRays(self, rays):
        r = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 8)
        sh = np.zeros(r.shape[0], np.int32)
        self._ok(self._L.yafaray_shadowRays(self._h, r.shape[0], r.ctypes.data_as(C.POINTER(C.c_float)),
                                            sh.ctypes.data_as(C.POINTER(C.c_int))), "shadowRays")
        return sh

    def probe(self, op, inp, n_out):
        """device-side component probe; inp (n, n_in) float32 (integers as bit patterns) -> (n, n_out) float32"""
        x = np.ascontiguousarray(inp, dtype=np.float32)
        x = x.reshape(x.shape[0], -1)
        out = np.zeros((x.shape[0], n_out), np.float32)
        fp = C.POINTER(C.c_float)
        self._ok(self._L.yafaray_probe(self._h, op, x.shape[0], x.ctypes.data_as(fp), x.shape[1], out.ctypes.data_as(fp), n_out), "probe")
        return out

    def setPassPipelining(self, mode):
        """-1: by size (default), 0: off, 1: on — consecutive independent passes on two internal streams (include/yafgpu.h)"""
        return self._ok(self._L.yafaray_setPassPipelining(self._h, int(mode)), "setPassPipelining")

    def setProfiling(self, enable):
        return self._ok(self._L.yafaray_setProfiling(self._h, int(enable)), "setProfiling")

    def getKernelProfile(self):
        """-> {name: (total_ms, launches)} of the last profiled pass"""
        ms = (C.c_double * 4)(); n = (C.c_uint64 * 4)()
        self._ok(self._L.yafaray_getKernelProfile(self._h, ms, n), "getKernelProfile")
        names = ("trace_closest", "trace_shadow", "shade", "other")
        return {k: (ms[i], int(n[i])) for i, k in enumerate(names)}

    def getFilm(self, width, height):
        film = np.zeros((height, width, 5), dtype=np.float32)
        self._ok(self._L.yafaray_getFilm(self._h, film.ctypes.data_as(C.POINTER(C.c_float)), width, height), "getFilm")
        return film

    def getRenderStats(self):
        s = RenderStats()
        self._L.yafaray_getRenderStats(self._h, C.byref(s))
        return s


class ImageOutput:
    """ImageOutput (common/output_image.cc) over a handler of createImageHandler: the render window goes into the handler's image at the
    border and one file is written under the path.  Made by Interface.createImageOutput; pass it to render(output=...) or setOutput2."""

    def __init__(self, interface, handle):
        self._yi = interface          # the handler is the interface's: keep it alive
        self._L = interface._L
        self._h = handle

    def callbacks(self):
        """the yafaray_output_t the library recognises (a pointer into the image output): a caller may also drive it pixel by pixel"""
        return self._L.yafaray_imageOutputCallbacks(self._h)

    def putPixel(self, num_view, x, y, rgba):
        t = self.callbacks().contents
        return bool(t.putPixel(t.user, num_view, x, y, rgba[0], rgba[1], rgba[2], rgba[3]))

    def flush(self, num_view=0):
        """saves the file; False when it could not be written (getLastError())"""
        t = self.callbacks().contents
        t.flush(t.user, num_view)
        return self.getLastError() == ""

    def getLastError(self):
        return self._L.yafaray_imageOutputLastError(self._h).decode()

    def close(self):
        if self._h:
            self._L.yafaray_destroyImageOutput(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


IMAGE_FLOAT, IMAGE_RGBA8, IMAGE_RGBE = 0, 1, 2      # YAFGPU_IMAGE_* (include/yafgpu.h)


def film_to_image(film, color_space="LinearRGB", gamma=1.0, alpha=True, format=IMAGE_RGBA8):
    """A film ((h, w, 5) float32, what getFilm / read_film_file return) through the device's output stage: normalised, clamped, converted
    to the colour space and packed -> (h, w, 4) float32 for IMAGE_FLOAT, (h, w, 4) uint8 r g b a for IMAGE_RGBA8 or r g b e for
    IMAGE_RGBE.  Needs a GPU.  Raises YafaRayError with the cause on failure."""
    px = np.ascontiguousarray(film, dtype=np.float32)
    if px.ndim != 3 or px.shape[2] != 5:
        raise ValueError("film must be (height, width, 5)")
    h, w = px.shape[:2]
    out = np.zeros((h, w, 4), dtype=np.float32 if format == IMAGE_FLOAT else np.uint8)
    L = load()
    if not L.yafaray_filmToImage(px.ctypes.data_as(C.POINTER(C.c_float)), w, h, _b(color_space), float(gamma), int(bool(alpha)), int(format),
                                 out.ctypes.data_as(C.c_void_p)):
        raise YafaRayError(L.yafaray_filmLastError().decode())
    return out


def write_image_file(path, file_type, pixels, alpha=False):
    """Write packed pixels ((h, w, 4) uint8: r g b a for "tga" and "png", r g b e for "hdr" / "pic") as an image file, on the host.
    Without alpha a tga / png file holds r g b alone.  False on failure, with the cause in film_last_error()."""
    px = np.ascontiguousarray(pixels, dtype=np.uint8)
    if px.ndim != 3 or px.shape[2] != 4:
        raise ValueError("pixels must be (height, width, 4) uint8")
    return bool(load().yafaray_writeImageFile(_b(os.fspath(path)), _b(file_type), px.shape[1], px.shape[0], int(bool(alpha)), px.ctypes.data_as(C.c_void_p)))


# the C API's spelling
filmToImage = film_to_image
writeImageFile = write_image_file


class TreeInfo(C.Structure):
    _fields_ = [("n_nodes", C.c_uint32), ("n_leaf_refs", C.c_uint32), ("max_depth", C.c_uint32), ("n_tris", C.c_uint32),
                ("build_seconds", C.c_double), ("upload_seconds", C.c_double), ("device_bytes", C.c_uint64)]


def build_kdtree(verts, threads=0, device=False):
    """Build of the flattened kd-tree the kernels walk, on the host (no GPU needed) or on the device
    -> (nodes (n,2) u32, refs (m,) u32, bound (6,) f32, info)."""
    L = load()
    v = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 9)
    L.yafgpu_kdtree_build.restype = C.c_void_p
    L.yafgpu_kdtree_build.argtypes = [C.POINTER(C.c_float), C.c_int32, C.c_int32]
    L.yafgpu_kdtree_build_device.restype = C.c_void_p
    L.yafgpu_kdtree_build_device.argtypes = [C.POINTER(C.c_float), C.c_int32]
    L.yafgpu_kdtree_info.argtypes = [C.c_void_p, C.POINTER(TreeInfo)]
    L.yafgpu_kdtree_get.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_float)]
    L.yafgpu_kdtree_destroy.argtypes = [C.c_void_p]
    if device:
        h = L.yafgpu_kdtree_build_device(v.ctypes.data_as(C.POINTER(C.c_float)), v.shape[0])
        if not h:
            raise YafaRayError("device kd build: " + L.yafgpu_last_error().decode())
    else:
        h = L.yafgpu_kdtree_build(v.ctypes.data_as(C.POINTER(C.c_float)), v.shape[0], threads)
    info = TreeInfo()
    L.yafgpu_kdtree_info(h, C.byref(info))
    nodes = np.zeros((max(info.n_nodes, 1), 2), np.uint32)
    refs = np.zeros(max(info.n_leaf_refs, 1), np.uint32)
    bound = np.zeros(6, np.float32)
    up = C.POINTER(C.c_uint32)
    L.yafgpu_kdtree_get(h, nodes.ctypes.data_as(up), refs.ctypes.data_as(up), bound.ctypes.data_as(C.POINTER(C.c_float)))
    L.yafgpu_kdtree_destroy(h)
    return nodes[:info.n_nodes], refs[:info.n_leaf_refs], bound, info


def build_treelets(nodes, inline_leaves=True):
    """The treelet layout the traversal kernels walk, built from a flattened tree as build_kdtree returns it
    -> (treelets (n,8) u32, escaped leaves (m,2) u32, root link).  See libyafaray_amd/csrc/kdtree_build.h."""
    L = load()
    up = C.POINTER(C.c_uint32)
    L.yafgpu_kdtree_treelets.argtypes = [up, C.c_uint32, C.c_int32, up, up, up, up, up]
    nd = np.ascontiguousarray(nodes, dtype=np.uint32).reshape(-1, 2)
    nw, nl, root = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    rc = L.yafgpu_kdtree_treelets(nd.ctypes.data_as(up), nd.shape[0], int(bool(inline_leaves)), None, C.byref(nw), None, C.byref(nl), C.byref(root))
    if rc:
        raise YafaRayError(f"treelet layout: {rc}")
    words = np.zeros(max(nw.value, 1), np.uint32)
    leaves = np.zeros(max(nl.value, 1), np.uint32)
    rc = L.yafgpu_kdtree_treelets(nd.ctypes.data_as(up), nd.shape[0], int(bool(inline_leaves)), words.ctypes.data_as(up), C.byref(nw),
                                  leaves.ctypes.data_as(up), C.byref(nl), C.byref(root))
    if rc:
        raise YafaRayError(f"treelet layout: {rc}")
    return words[:nw.value].reshape(-1, 8), leaves[:nl.value].reshape(-1, 2), root.value


def tri_order(refs, n_tris):
    """Where wf_trace's own copy of the triangle records keeps every triangle (kdtree_build.h, tri_order): pos (n_tris,) u32, from
    the leaf references as build_kdtree returns them (no GPU needed).  YAFGPU_TRI_ORDER=id makes the scene take the identity instead."""
    L = load()
    up = C.POINTER(C.c_uint32)
    L.yafgpu_kdtree_tri_order.argtypes = [up, C.c_uint32, C.c_uint32, up]
    L.yafgpu_kdtree_tri_order.restype = None
    r = np.ascontiguousarray(refs, dtype=np.uint32).reshape(-1)
    pos = np.zeros(max(int(n_tris), 1), np.uint32)
    L.yafgpu_kdtree_tri_order(r.ctypes.data_as(up), r.shape[0], int(n_tris), pos.ctypes.data_as(up))
    return pos[:int(n_tris)]


def trace_reservation(n, seen, waves):
    """the queue entries a traversal wave reserves with `seen` of `n` handed out, by the rule the library was built with"""
    L = load()
    L.yafgpu_trace_reservation.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32]
    L.yafgpu_trace_reservation.restype = C.c_uint32
    return int(L.yafgpu_trace_reservation(n, seen, waves))


def trace_schedule():
    """the traversal kernels' queue schedule as built, and the workgroups of this process's last traversal launches (include/yafgpu.h)"""
    L = load()
    info = (C.c_uint32 * 8)()
    L.yafgpu_trace_schedule.argtypes = [C.POINTER(C.c_uint32)]
    L.yafgpu_trace_schedule.restype = None
    L.yafgpu_trace_schedule(info)
    keys = ("min", "max", "div", "shrink", "static_first", "waves_per_group", "grid_closest", "grid_any")
    return dict(zip(keys, (int(v) for v in info)))


def planes_bytes(width, height):
    return load().yafgpu_planes_bytes(width, height)


def film_combine(d_planes, d_film, width, height, stream=0):
    rc = load().yafgpu_film_combine(C.c_void_p(d_planes), C.c_void_p(d_film), width, height, C.c_void_p(stream or None))
    if rc:
        raise YafaRayError(load().yafgpu_last_error().decode())


FILM_HEADER_FIELDS = tuple(k for k, _ in FilmHeader._fields_)


def film_last_error():
    """why this thread's last read_film_file / write_film_file failed"""
    return load().yafaray_filmLastError().decode()


def write_film_file(path, header, film):
    """Write `film` ((h, w, 5) float32: r, g, b, a, weight — what getFilm returns) as a film file.  header: a dict with computer_node,
    base_sampling_offset, sampling_offset, cx0, cx1, cy0, cy1 (absent: 0; cx1 / cy1 absent: cx0 + w / cy0 + h); w and h come from the
    film.  The file holds the combined pass alone (n_passes 1, n_aux 0).  False on failure (film_last_error())."""
    px = np.ascontiguousarray(film, dtype=np.float32)
    if px.ndim != 3 or px.shape[2] != 5:
        raise ValueError("film must be (height, width, 5)")
    h = FilmHeader()
    for k in ("computer_node", "base_sampling_offset", "sampling_offset", "cx0", "cy0"):
        setattr(h, k, int(header.get(k, 0)))
    h.h, h.w = px.shape[0], px.shape[1]
    h.cx1 = int(header.get("cx1", h.cx0 + h.w))
    h.cy1 = int(header.get("cy1", h.cy0 + h.h))
    h.n_passes, h.n_aux = 1, 0
    return bool(load().yafaray_writeFilmFile(_b(os.fspath(path)), C.byref(h), px.ctypes.data_as(C.POINTER(C.c_float))))


def read_film_file(path, out=None, header_only=False):
    """Read a film file -> (header dict, film (h, w, 5) float32), or the header dict alone with header_only; False on failure, with the
    cause in film_last_error().  Pass 0 is read, further passes are skipped.  out: a C-contiguous float32 array of h * w * 5 values to
    read into (it is returned in place of a new one, and left untouched on failure)."""
    L, p, h = load(), _b(os.fspath(path)), FilmHeader()
    if header_only:
        return h.as_dict() if L.yafaray_readFilmFile(p, C.byref(h), None, 0) else False
    if out is None:
        if not L.yafaray_readFilmFile(p, C.byref(h), None, 0):
            return False
        out = np.zeros((h.h, h.w, 5), dtype=np.float32)
    elif out.dtype != np.float32 or not out.flags.c_contiguous:
        raise ValueError("out must be a C-contiguous float32 array")
    if not L.yafaray_readFilmFile(p, C.byref(h), out.ctypes.data_as(C.POINTER(C.c_float)), out.size):
        return False
    return h.as_dict(), out


def film_to_rgba(film):
    """Pixel::normalized (util_image_buffers.h:39-43)."""
    w = film[..., 4:5]
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(w != 0, film[..., :4] / w, 0.0).astype(np.float32)
