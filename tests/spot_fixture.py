"""TEST SUPPORT: the float32 restatement of SpotLight (light_spot.cc): its constructor (:29-42), illuminate (:81-110), illumSample
(:112-151) and intersect (:219-256), operation for operation, in numpy float32 on top of the createCs__ / sampleCone__ / fSqrt__ / normalize
restatements tests/ies_fixture.py uses and np_fcos of tests/test_gpu_ibl.py.  Shared by tests/test_spot_host.py and tests/test_gpu_spot.py.
Photon emission (the Pdf1D of the smoothstep, interv_1_ / interv_2_, emitPhoton, emitSample, emitPdf) is not restated."""
import numpy as np

from tests.ies_fixture import D2R, create_cs, sample_cone
from tests.test_gpu_ibl import np_fcos
from tests.test_lights_host import F, dot, fsqrt, normalize

# word offsets in a yafgpu_light record (include/yafgpu.h) behind direction (4), du (7), dv (10) and cos_angle (13)
W_COS_START, W_ICOS_DIFF, W_FUZZY = 14, 15, 16
TYPE_SPOT, TYPE_SPOT_SOFT = 11, 12


def consts(frm, to, color=(1.0, 1.0, 1.0), power=1.0, cone_angle=45.0, blend=0.15, fuzzy=1.0):
    """SpotLight's constructor, :34-42: the angles in double with the float 1.f - falloff, fCos__ of the narrowed angles, icos_diff_ a
    double quotient of the float difference, narrowed (infinite when the two cosines are equal)"""
    frm = np.array(frm, np.float32); to = np.array(to, np.float32)
    ndir = normalize(frm - to)
    du, dv = create_cs(-ndir)
    rad_angle = np.float64(F(cone_angle)) * D2R
    rad_inner = rad_angle * np.float64(F(1) - F(blend))
    cos_start = np_fcos(np.float32(rad_inner))[()]
    cos_end = np_fcos(np.float32(rad_angle))[()]
    with np.errstate(divide="ignore"):
        icos_diff = np.float32(np.float64(1.0) / np.float64(F(cos_start - cos_end)))
    return {"position": frm, "ndir": ndir.astype(np.float32), "du": du[0], "dv": dv[0], "cos_start": F(cos_start), "cos_end": F(cos_end),
            "icos_diff": icos_diff, "fuzzy": F(fuzzy), "color": np.array(color, np.float32) * F(power)}


def falloff(c, cosa):
    """:102-103: the smoothstep of a cosine between cos_end_ and cos_start_"""
    with np.errstate(all="ignore"):
        v = (cosa - c["cos_end"]) * c["icos_diff"]
        return ((v * v) * (F(3) - F(2) * v)).astype(np.float32)


def _to_light(c, p):
    ldir = c["position"] - p
    dist_sqr = dot(ldir, ldir)
    with np.errstate(all="ignore"):
        dist = fsqrt(dist_sqr)
        ldir = ldir * (F(1) / dist)[:, None]
        cosa = dot(np.broadcast_to(c["ndir"], ldir.shape), ldir)
        ok = ~(dist == 0) & ~(cosa < c["cos_end"])
    return ldir.astype(np.float32), dist_sqr, dist, cosa, ok


def illuminate(c, p):
    """SpotLight::illuminate, :81-110 -> (n, 8): ok, wi.dir_, wi.tmax_, colour (zeros where it refuses)"""
    ldir, dist_sqr, dist, cosa, ok = _to_light(c, p)
    with np.errstate(all="ignore"):
        idist_sqr = F(1) / dist_sqr
        plain = cosa >= c["cos_start"]
        scale = np.where(plain, idist_sqr, falloff(c, cosa) * idist_sqr).astype(np.float32)
        col = c["color"][None, :] * scale[:, None]
    out = np.zeros((p.shape[0], 8), np.float32)
    out[:, 0] = ok; out[ok, 1:4] = ldir[ok]; out[ok, 4] = dist[ok]; out[ok, 5:8] = col[ok]
    return out


def illum_sample(c, p, s_1, s_2):
    """SpotLight::illumSample, :112-151 -> (n, 9): ok, wi.dir_, wi.tmax_, pdf, ls.col (zeros where it refuses).  The cone is the LIGHT's
    (du_, dv_, cos_end_) around the direction to the light, the samples scaled by shadow_fuzzy_; pdf = dist_sqr, and below 1 it becomes 1
    with the colour divided by dist_sqr (:144-148)"""
    ldir, dist_sqr, dist, cosa, ok = _to_light(c, p)
    n = p.shape[0]
    s_1 = np.asarray(s_1, np.float32) * c["fuzzy"]; s_2 = np.asarray(s_2, np.float32) * c["fuzzy"]
    with np.errstate(all="ignore"):
        wdir = sample_cone(ldir, np.broadcast_to(c["du"], (n, 3)), np.broadcast_to(c["dv"], (n, 3)), c["cos_end"], s_1, s_2).astype(np.float32)
        plain = cosa >= c["cos_start"]
        col = np.where(plain[:, None], c["color"][None, :], c["color"][None, :] * falloff(c, cosa)[:, None]).astype(np.float32)
        near = dist_sqr < F(1)
        pdf = np.where(near, F(1), dist_sqr).astype(np.float32)
        col = np.where(near[:, None], col / dist_sqr[:, None], col).astype(np.float32)
    out = np.zeros((n, 9), np.float32)
    out[:, 0] = ok; out[ok, 1:4] = wdir[ok]; out[ok, 4] = dist[ok]; out[ok, 5] = pdf[ok]; out[ok, 6:9] = col[ok]
    return out


def intersect(c, frm, d):
    """SpotLight::intersect, :219-256 -> (n, 6): ok, t, ipdf, colour (zeros where it refuses).  The exact-zero test on the offset of the
    hit point from the light along the axis (:231) and the hit point's distance from the WORLD ORIGIN against the double 1e-2 (:233)"""
    frm = np.asarray(frm, np.float32); d = np.asarray(d, np.float32)
    n = frm.shape[0]
    axis = np.broadcast_to(-c["ndir"], (n, 3)).astype(np.float32)          # dir_
    pos = np.broadcast_to(c["position"], (n, 3))
    with np.errstate(all="ignore"):
        cos_a = dot(axis, d)
        t = (dot(axis, pos - frm) / cos_a).astype(np.float32)
        p = (frm + d * t[:, None]).astype(np.float32)
        ok = ~(cos_a == 0) & ~(t < 0) & (dot(axis, p - pos) == 0) & (dot(p, p).astype(np.float64) <= 1e-2) & ~(cos_a < c["cos_end"])
        plain = cos_a >= c["cos_start"]
        col = np.where(plain[:, None], c["color"][None, :], c["color"][None, :] * falloff(c, cos_a)[:, None]).astype(np.float32)
        ipdf = (F(1) / (t * t)).astype(np.float32)
    out = np.zeros((n, 6), np.float32)
    out[:, 0] = ok; out[ok, 1] = t[ok]; out[ok, 2] = ipdf[ok]; out[ok, 3:6] = col[ok]
    return out


def record(c, soft=False, samples=8):
    """the 34 words of the yafgpu_light record createLight makes of these constants (cast_shadows on), as uint32"""
    r = np.zeros(34, np.float32)
    r[:4] = np.array([TYPE_SPOT_SOFT if soft else TYPE_SPOT, samples if soft else 1, 1, 0], np.int32).view(np.float32)
    r[4:7] = c["ndir"]; r[7:10] = c["du"]; r[10:13] = c["dv"]; r[13] = c["cos_end"]
    r[W_COS_START] = c["cos_start"]; r[W_ICOS_DIFF] = c["icos_diff"]; r[W_FUZZY] = c["fuzzy"]
    r[25:28] = c["color"]; r[29:32] = c["position"]
    return r.view(np.uint32)
