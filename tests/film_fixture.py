"""The film of a render, composed from its definition in float64: the shared reference of tests/test_film_filters_host.py (the oracle's
film) and tests/test_gpu_film_filters.py (the device's film), and the box scene they and tests/test_gpu_cameras.py render.

ImageFilm's constructor and ImageFilm::addSample (imagefilm.cc:60-122, :124-177, :925-1015) are restated from the reference's text: the
filter table in float32 numpy scalars over the three leaf functions that tests/test_oracle_golden.py pins bit for bit to the reference
(fExp2__, fSin__, fSqrt__ as the oracle library's yor_fexp2, yor_fsin, yor_fsqrt), the footprint and the table indices in double as
addSample forms them.  Every term `colour * weight` is rounded once to float32, as both films form it, and the terms are summed in
float64.  A film that adds exactly these terms in float32, in any order and any association, stays within bound() of that sum: the bound
is derived from the number of terms, no measured tolerance enters.

This module imports neither torch nor the device library; the oracle library is loaded on first use."""
from typing import NamedTuple

import numpy as np

from libyafaray_amd import scenes
from oracle import pyoracle as po

F = np.float32
D = np.float64
M32 = 0xffffffff
M_PI, M_PI_2, M_LOG2E = 3.14159265358979323846, 1.57079632679489661923, 1.4426950408889634074
GAUSS_EXP = 0.00247875                 # imagefilm.cc:85
TABLE_SIZE, MAX_FILTER_SIZE = 16, 8    # imagefilm.h: FILTER_TABLE_SIZE, MAX_FILTER_SIZE
U = 2.0 ** -24                         # unit roundoff of float32

# ---- the scene -------------------------------------------------------------------------------------------------------
W, H, TILE = 24, 16, 7
FACE_COLOURS = [(0.5, 0.25, 0.125), (0.125, 0.5, 0.25), (0.25, 0.125, 0.5), (0.75, 0.5, 0.25), (0.25, 0.75, 0.5), (0.5, 0.25, 0.75)]
BACKGROUND = (0.125, 0.375, 0.625)
# towards the corner of the +y face, the floor and the removed +x face: two surfaces and the background meet inside the frame (and inside
# CROP), with edges in several directions
FILM_CAMERA = {"type": "perspective", "from": (1.2, 0.9, -1.1), "to": (2.0, 2.0, -2.0), "up": (1.5, 0.7, 0.0), "resx": W, "resy": H, "focal": 0.3}


def box_scene(cam, removed=2):
    """a closed box of half-width 2 around the camera: six light_mat quads, double sided, colours in eighths (sums of a few samples are
    exact); face `removed` (+x) is left out so that some rays escape to the background"""
    q, r = scenes._quad, 2.0
    faces = [q((-r, -r, r), (r, -r, r), (r, r, r), (-r, r, r)), q((-r, -r, -r), (r, -r, -r), (r, -r, r), (-r, -r, r)),
             q((r, -r, -r), (r, r, -r), (r, r, r), (r, -r, r)), q((r, r, -r), (-r, r, -r), (-r, r, r), (r, r, r)),
             q((-r, r, -r), (-r, -r, -r), (-r, -r, r), (-r, r, r)), q((-r, -r, -r), (-r, r, -r), (r, r, -r), (r, -r, -r))]
    keep = [k for k in range(6) if k != removed]
    verts = np.concatenate([faces[k] for k in keep]).astype(F)
    mats = np.repeat(np.arange(len(keep)), 2).astype(np.int32)
    materials = [{"type": "light_mat", "color": FACE_COLOURS[k], "power": 1.0, "double_sided": True} for k in keep]
    return {"verts": verts, "tri_mat": mats, "vnormals": None, "materials": materials, "lights": [], "camera": dict(cam)}


def box_settings(spp=1, **kw):
    return scenes.render_settings(kw.pop("width", W), kw.pop("height", H), spp, integrator="directlighting", tile_size=TILE, background=BACKGROUND, **kw)


def film_settings(filter_type, pixelwidth, spp=4, **kw):
    return box_settings(spp, filter_type=filter_type, AA_pixelwidth=pixelwidth, **kw)


CROP = dict(xstart=5, ystart=3, width=13, height=9)
# (id, filter, AA_pixelwidth, further settings): mitchell 4.0 clamps to the half-width 4.0, gauss 0.3 to 0.501 (still the table path)
HOST_CASES = [("gauss 1.5", "gauss", 1.5, {}), ("mitchell 1.2", "mitchell", 1.2, {}), ("lanczos 2.0", "lanczos", 2.0, {}), ("box 2.5", "box", 2.5, {}),
              ("mitchell 4.0", "mitchell", 4.0, {}), ("gauss 0.3", "gauss", 0.3, {}), ("lanczos 8.0 crop", "lanczos", 8.0, CROP)]


def colours_by_triangle(sc, tri):
    """the light_mat colour of every hit triangle, the background where tri < 0 -> (n, 3) float32"""
    tri = np.asarray(tri)
    by_tri = np.array([sc["materials"][m]["color"] for m in sc["tri_mat"]], F)
    return np.where((tri >= 0)[:, None], by_tri[np.maximum(tri, 0)], np.array(BACKGROUND, F)[None, :]).astype(F)


# ---- the filter table ------------------------------------------------------------------------------------------------
def _box(dx, dy):
    return F(1)                                                            # :60


def _mitchell(dx, dy):
    x = F(2) * F(po.lib().yor_fsqrt(F(dx * dx + dy * dy)))                 # :89
    if x >= F(2):
        return F(0)
    if x >= F(1):                                                          # :95, float constants throughout
        return F(x * (x * (x * F(-0.38888889) + F(2.0)) - F(3.33333333)) + F(1.77777778))
    return F(x * x * (F(1.16666666) * x - F(2.0)) + F(0.88888889))         # :98


def _gauss(dx, dy):
    r_2 = F(dx * dx + dy * dy)                                             # :103
    e = F(po.lib().yor_fexp2(F(F(M_LOG2E) * F(F(-6) * r_2))))              # fExp__(a) = fExp2__((float) M_LOG2E * a)
    return max(F(0), F(D(e) - GAUSS_EXP))                                  # :104: float - double, narrowed


def _lanczos(dx, dy):
    x = F(po.lib().yor_fsqrt(F(dx * dx + dy * dy)))                        # :110
    if x == F(0):
        return F(1)
    if -2 < x < 2:
        a, b = F(M_PI * D(x)), F(M_PI_2 * D(x))                            # :116-117: double products, narrowed
        return F(F(F(po.lib().yor_fsin(a)) * F(po.lib().yor_fsin(b))) / F(a * b))
    return F(0)


FILTERS = {"box": _box, "mitchell": _mitchell, "gauss": _gauss, "lanczos": _lanczos}


def filter_table(filter_type):
    """filter_table_ (imagefilm.cc:152-174): the filter at ((x + .5) / 16, (y + .5) / 16), [y, x], float32"""
    f, scale = FILTERS[filter_type], F(1) / F(TABLE_SIZE)
    table = np.zeros((TABLE_SIZE, TABLE_SIZE), F)
    with np.errstate(all="ignore"):
        for y in range(TABLE_SIZE):
            for x in range(TABLE_SIZE):
                table[y, x] = f(F(F(x) + F(.5)) * scale, F(F(y) + F(.5)) * scale)
    return table


def film_geometry(rd):
    """(filterw_, table_scale_), both float32 (imagefilm.cc:127, :158-165, :176)"""
    filterw = F(D(F(rd.get("AA_pixelwidth", 1.5))) * 0.5)
    kind = rd.get("filter_type", "box")
    if kind == "mitchell":
        filterw = F(filterw * F(2.6))
    elif kind == "gauss":
        filterw = F(filterw * F(2))
    filterw = min(max(F(0.501), filterw), F(0.5) * F(MAX_FILTER_SIZE))
    return F(filterw), F(0.9999 * TABLE_SIZE / D(filterw))


# ---- the camera samples ----------------------------------------------------------------------------------------------
class Samples(NamedTuple):
    """one row per camera sample, in the order pixel row, pixel, pass, sample"""
    px: np.ndarray          # int64: the pixel, in camera coordinates
    py: np.ndarray
    pas: np.ndarray         # int64: the pass
    s: np.ndarray           # int64: the sample's index within its pass
    dx: np.ndarray          # float32: the position within the pixel
    dy: np.ndarray

    def __len__(self):
        return len(self.px)

    def take(self, keep):
        return Samples(*(a[keep] for a in self))

    def positions(self):
        """the image positions handed to Camera::shootRay (integrator_tiled.cc:403)"""
        return (self.px.astype(F) + self.dx).astype(F), (self.py.astype(F) + self.dy).astype(F)


def sampling_offs(px, py):
    fnv = lambda v: int(po.lib().yor_fnv32a(v & M32))
    return fnv((py * fnv(px)) & M32)                                       # integrator_tiled.cc:386


def pass_schedule(rd):
    """[(first sample number, samples)] of every pass"""
    spp, passes = int(rd.get("AA_minsamples", 1)), int(rd.get("AA_passes", 1))
    inc = int(rd.get("AA_inc_samples", spp))
    assert passes == 1 or rd.get("AA_threshold") == 0.0, "an adaptive pass resamples what the film decides"
    return [(0, spp)] + [(spp + k * inc, inc) for k in range(passes - 1)]


def sample_offsets(rd):
    """the sub-pixel positions of every camera sample of a render (TiledIntegrator::renderTile, integrator_tiled.cc:386-403): one pass
    of n > 1 samples is stratified in x and ri_lp in y, one sample sits in the centre, several passes (all of them: AA_threshold 0.0)
    draw riVdC / riS at the running sample number"""
    L = po.lib()
    schedule = pass_schedule(rd)
    x0, y0 = rd.get("xstart", 0), rd.get("ystart", 0)
    rows = []
    for py in range(y0, y0 + rd["height"]):
        for px in range(x0, x0 + rd["width"]):
            so = sampling_offs(px, py)
            for k, (pass_offset, n) in enumerate(schedule):
                for s in range(n):
                    pixel_sample = (pass_offset + s) & M32
                    if len(schedule) > 1:
                        dx, dy = F(L.yor_ri_vdc(pixel_sample, so)), F(L.yor_ri_s(pixel_sample, so))
                    elif n > 1:
                        d_1 = F(1.0 / float(F(n)))
                        dx, dy = F((0.5 + float(F(s))) * float(d_1)), F(L.yor_ri_lp((s + so) & M32, 0))
                    else:
                        dx, dy = F(0.5), F(0.5)
                    rows.append((px, py, k, s, dx, dy))
    cols = list(zip(*rows))
    return Samples(*(np.array(c, np.int64) for c in cols[:4]), *(np.array(c, F) for c in cols[4:]))


def tile_rank(rd, samples, world):
    """the shard that renders every sample: tile t of the window, row-major, belongs to rank t % world (ImageSplitter's linear order)"""
    t = int(rd["tile_size"])
    ntx = (rd["width"] + t - 1) // t
    return (((samples.py - rd.get("ystart", 0)) // t) * ntx + (samples.px - rd.get("xstart", 0)) // t) % world


# ---- the film --------------------------------------------------------------------------------------------------------
def clamp_proportional(rgb, max_value):
    """Rgb::clampProportionalRgb (color.h:412-445) over rows, float32"""
    rgb = np.array(rgb, F)
    if not max_value > 0:
        return rgb
    mx = F(max_value)
    max_rgb = rgb.max(axis=1)
    with np.errstate(all="ignore"):
        adj = (mx / max_rgb).astype(F)
    over = max_rgb > mx
    first = np.argmax(rgb >= max_rgb[:, None], axis=1)       # r, else g, else b: the first component that reaches the maximum
    out = (rgb * adj[:, None]).astype(F)
    out[np.arange(len(rgb)), first] = mx
    return np.where(over[:, None], out, rgb).astype(F)


def round2int(v):
    """round2Int__ (util_math.h:41): int(val + (.5 - 1.4e-11)), a truncation towards zero"""
    return np.trunc(np.asarray(v, D) + (.5 - 1.4e-11)).astype(np.int64)


def footprint_terms(rd, samples):
    """every (sample, covered pixel) pair of ImageFilm::addSample (imagefilm.cc:933-968) -> (sample index, film row, film column, weight):
    the extent dx_0..dx_1 x dy_0..dy_1 clipped to the window, the table indices formed in double"""
    filterw, table_scale = film_geometry(rd)
    table = filter_table(rd.get("filter_type", "box"))
    fw, ts = D(filterw), D(table_scale)
    cx0, cy0 = rd.get("xstart", 0), rd.get("ystart", 0)
    cx1, cy1 = cx0 + rd["width"], cy0 + rd["height"]
    x, y, dx, dy = samples.px, samples.py, samples.dx.astype(D), samples.dy.astype(D)
    dx_0, dx_1 = np.maximum(cx0 - x, round2int(dx - fw)), np.minimum(cx1 - x - 1, round2int(dx + fw - 1.0))
    dy_0, dy_1 = np.maximum(cy0 - y, round2int(dy - fw)), np.minimum(cy1 - y - 1, round2int(dy + fw - 1.0))
    assert ((dx_1 - dx_0 <= MAX_FILTER_SIZE) & (dy_1 - dy_0 <= MAX_FILTER_SIZE)).all()       # x_index[MAX_FILTER_SIZE + 1]
    x_offs, y_offs = dx - 0.5, dy - 0.5
    out = []
    if len(samples):
        for j in range(int(dy_0.min()), int(dy_1.max()) + 1):
            yi = np.floor(np.abs((D(j) - y_offs) * ts)).astype(np.int64)
            for i in range(int(dx_0.min()), int(dx_1.max()) + 1):
                sel = np.nonzero((dx_0 <= i) & (i <= dx_1) & (dy_0 <= j) & (j <= dy_1))[0]
                if len(sel):
                    xi = np.floor(np.abs((D(i) - x_offs[sel]) * ts)).astype(np.int64)
                    out.append((sel, y[sel] + j - cy0, x[sel] + i - cx0, table[yi[sel], xi]))
    if not out:
        return tuple(np.zeros(0, t) for t in (np.int64, np.int64, np.int64, F))
    return tuple(np.concatenate(c) for c in zip(*out))


def compose(rd, samples, colours):
    """the film of `samples` with the float32 colours `colours` (n, 3: alpha is 1) -> (ref (h, w, 5) float64, mag (h, w, 5) float64,
    count (h, w) int64): per pixel the sum of its terms, of their absolute values, and their number.  A term is colour_c * weight rounded
    once to float32 (pixel.col_ += col * filter_wt) and the weight itself (pixel.weight_ += filter_wt); the colour is clamped as
    addSample clamps it (imagefilm.cc:975)"""
    rgb = clamp_proportional(np.asarray(colours, F).reshape(-1, 3), rd.get("AA_clamp_samples", 0.0))
    rgba = np.concatenate([rgb, np.ones((len(rgb), 1), F)], axis=1)
    assert len(rgba) == len(samples)
    idx, fy, fx, w = footprint_terms(rd, samples)
    terms = np.concatenate([(rgba[idx] * w[:, None]).astype(F), w[:, None]], axis=1).astype(D)
    h, wd = rd["height"], rd["width"]
    ref, mag, count = np.zeros((h, wd, 5), D), np.zeros((h, wd, 5), D), np.zeros((h, wd), np.int64)
    np.add.at(ref, (fy, fx), terms)
    np.add.at(mag, (fy, fx), np.abs(terms))
    np.add.at(count, (fy, fx), 1)
    return ref, mag, count


def bound(mag, count):
    """the rounding error bound of a float32 sum of `count` given terms of absolute sum `mag`, in any order and any association:
    gamma_n * mag with n = count + 1, gamma_n = n u / (1 - n u).  (count - 1 additions round; the two more pay for a partial sum that
    joins the rest in an addition of its own.)"""
    n = (np.asarray(count) + 1).astype(D)
    return (n * U / (1.0 - n * U))[..., None] * mag
