"""The wide-filter path of wf_accumulate (every reconstruction filter but the box of one pixel: table weights, a footprint with negative
offsets clipped on four sides, float atomics into plane 0) against the float64 composition of tests/film_fixture.py, which
tests/test_film_filters_host.py checks against the oracle on the CPU.

Every camera sample is coloured by the triangle the device's own intersectRays reports for its restated ray (light_mat colours, no
lights: the colour of a sample is its surface's or the background's), the film is composed from ImageFilm::addSample's definition, and
the device's film must lie within the rounding error bound of a float32 sum of exactly those terms in any order — on every pixel and
channel, without an allowance for outliers.  One splat that is dropped, doubled or read from the wrong table entry leaves the bound.

The wide path is run with crop windows off the origin, both width clamps, accumulating passes, AA_clamp_samples, shards, several chunks
per pass, pipelined passes and frames smaller than the footprint.  Adaptive passes (AA_threshold > 0) with a wide filter are left out
on purpose: with weights that are no integers the resampled set cannot be read off the film, and a last-bit difference from the atomics
may flip a noise decision legitimately.

Frames are 24 x 16 or smaller, tiles of 7."""
import numpy as np
import pytest

from libyafaray_amd import Interface, scenes
from tests import film_fixture as ff
from tests.test_cameras_host import RECORD, shoot
from tests.test_gpu_pipeline import _passes

pytestmark = pytest.mark.gpu

F = np.float32
SCENE = ff.box_scene(ff.FILM_CAMERA)
SMALL = dict(xstart=0, ystart=0, width=7, height=5)


@pytest.fixture(scope="module", autouse=True)
def torch_first():
    """(as in the other GPU modules: let torch open the GPU before the library does)"""
    import torch
    torch.cuda.init()


def loaded(rd):
    yi = Interface()
    scenes.load_scene(yi, SCENE, rd)
    return yi


def device(rd, shard=None):
    yi = loaded(rd)
    if shard:
        yi.setShard(*shard)
    yi.render()
    return yi.getFilm(rd["width"], rd["height"]).copy(), yi


_samples, _composed = {}, {}


def coloured_samples(yi, rd):
    """(samples, colours) of a render: computed once per window and sample schedule (the filter moves no sample), from the hits of the
    device's own tree"""
    key = tuple(rd.get(k) for k in ("width", "height", "xstart", "ystart", "AA_minsamples", "AA_passes", "AA_inc_samples"))
    if key not in _samples:
        samples = ff.sample_offsets(rd)
        frm, dr, tmin, tmax, wt = shoot(RECORD["perspective"](SCENE["camera"]), *samples.positions())
        assert (wt != 0).all()
        tri, _, _ = yi.intersectRays(np.column_stack([frm, dr, tmin, tmax]).astype(F))
        _samples[key] = (samples, ff.colours_by_triangle(SCENE, tri))
    return _samples[key]


def composed(yi, rd):
    """(samples, colours, ref, mag, count), the composition shared between the tests of the same settings and left unchanged"""
    key = tuple(sorted((k, v) for k, v in rd.items()))
    if key not in _composed:
        samples, colours = coloured_samples(yi, rd)
        out = (samples, colours) + ff.compose(rd, samples, colours)
        for a in out[1:]:
            a.setflags(write=False)
        _composed[key] = out
    return _composed[key]


def ratio(film, ref, bnd):
    err = np.abs(np.asarray(film, np.float64) - ref)
    with np.errstate(all="ignore"):
        return err, float(np.nanmax(np.where(err == 0, 0.0, err / bnd), initial=0.0))


def assert_within(what, film, ref, mag, count, factor=1.0):
    bnd = factor * ff.bound(mag, count)
    assert np.isfinite(film).all(), what
    err, worst = ratio(film, ref, bnd)
    print(f"{what}: largest error / bound {worst:.3f}")
    bad = err > bnd
    assert not bad.any(), f"{what}: {int(bad.any(axis=-1).sum())} pixels outside the bound, largest error / bound {worst:.3g}, first at {np.argwhere(bad)[0]}"


def n_samples(rd):
    return rd["width"] * rd["height"] * sum(n for _, n in ff.pass_schedule(rd))


def assert_counts(yi, n):
    st = yi.getRenderStats()
    assert (st.camera_samples, st.rays_closest, st.rays_shadow) == (n, n, 0)


def checked(what, rd, full_frame_mix=True):
    """render, compose, hold the film to the bound -> (film, samples, colours, ref, mag, count)"""
    film, yi = device(rd)
    samples, colours, ref, mag, count = composed(yi, rd)
    assert len(samples) == n_samples(rd)
    if full_frame_mix:
        escaped = (colours == np.array(ff.BACKGROUND, F)).all(axis=1)
        assert escaped.any() and not escaped.all() and len(np.unique(colours, axis=0)) >= 3, "the frame does not mix surfaces and background"
    assert_within(what, film, ref, mag, count)
    assert_counts(yi, len(samples))
    return film, samples, colours, ref, mag, count


# ---- a. the cases of the host test -----------------------------------------------------------------------------------
@pytest.mark.parametrize("what,kind,width,kw", ff.HOST_CASES, ids=[c[0] for c in ff.HOST_CASES])
def test_film_within_the_bound(what, kind, width, kw):
    checked(what, ff.film_settings(kind, width, **kw))


# ---- b. wide boxes are exact -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("window", [{}, ff.CROP], ids=["full", "crop"])
@pytest.mark.parametrize("width", [2.5, 1.3])
def test_wide_box_bit_for_bit(width, window):
    """all colours are multiples of 1 / 8 and all weights 1: every summation order is exact, the weights are the numbers of terms"""
    film, _, _, ref, _, count = checked(f"box {width}", ff.film_settings("box", width, **window))
    assert ff.film_geometry(ff.film_settings("box", width))[0] > F(0.501)
    assert np.array_equal(film.view(np.uint32), ref.astype(F).view(np.uint32))
    assert np.array_equal(film[..., 4], count) and np.array_equal(film[..., 3], count)
    assert count.max() > 4, "no pixel receives a neighbour's sample"


# ---- c. crop windows -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window", [ff.CROP, SMALL], ids=["off the origin", "7 x 5 at the origin"])
@pytest.mark.parametrize("kind,width", [("gauss", 1.5), ("mitchell", 1.2)])
def test_crop_windows(kind, width, window):
    """the left and top clips away from the frame's edge, and a window of one tile (it sees one surface: its weights and clips count)"""
    checked(f"{kind} {width} {window}", ff.film_settings(kind, width, **window), full_frame_mix=window is ff.CROP)


# ---- d. accumulating passes ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,width", [("gauss", 1.5), ("lanczos", 2.0)])
def test_accumulating_passes(kind, width):
    """three passes of 2 samples at riVdC / riS positions add into the same plane"""
    rd = ff.film_settings(kind, width, spp=2, AA_passes=3, AA_inc_samples=2, AA_threshold=0.0)
    film, samples, *_ = checked(f"{kind} {width}, three passes", rd)
    assert len(samples) == ff.W * ff.H * 6 and set(samples.pas) == {0, 1, 2}
    one, _ = device(ff.film_settings(kind, width, spp=2))
    assert not np.array_equal(film[..., 4], one[..., 4]), "the later passes added nothing"


# ---- e. AA_clamp_samples ---------------------------------------------------------------------------------------------
def test_clamped_samples():
    rd = ff.film_settings("mitchell", 1.2, AA_clamp_samples=0.4)
    _, samples, colours, ref, mag, count = checked("mitchell 1.2, clamp 0.4", rd)
    assert colours.max() == F(0.75)
    unclamped, _, _ = ff.compose(dict(rd, AA_clamp_samples=0.0), samples, colours)
    assert (np.abs(unclamped - ref) > ff.bound(mag, count)).any(), "the clamp cannot be seen in this film"


# ---- f. frames smaller than the footprint ----------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(1, 1), (24, 1), (1, 16)])
def test_frames_smaller_than_the_footprint(w, h):
    """mitchell 4.0 reaches 4 pixels to every side: all four clips act on one sample"""
    checked(f"mitchell 4.0, {w} x {h}", ff.film_settings("mitchell", 4.0, spp=3, width=w, height=h), full_frame_mix=False)


# ---- g. shards -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3])
def test_shards(world):
    """every rank's film holds the splats of its own tiles' samples, those into the other ranks' tiles included"""
    rd = ff.film_settings("gauss", 1.5)
    total = np.zeros((ff.H, ff.W, 5), np.float64)
    for r in range(world):
        film, yi = device(rd, shard=(r, world))
        samples, colours, ref, mag, count = composed(yi, rd)
        mine = ff.tile_rank(rd, samples, world) == r
        assert 0 < mine.sum() < len(samples)
        part, part_mag, part_count = ff.compose(rd, samples.take(mine), colours[mine])
        assert_within(f"gauss 1.5, shard {r} of {world}", film, part, part_mag, part_count)
        assert_counts(yi, int(mine.sum()))
        owned = np.zeros((ff.H, ff.W), bool)
        owned[samples.py[mine], samples.px[mine]] = True
        assert (film[~owned][:, 4] != 0).any(), "no splat landed in another rank's tile"
        total += film
    assert_within(f"gauss 1.5, {world} shards summed", total, ref, mag, count)


# ---- h. several chunks per pass --------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,width", [("gauss", 1.5), ("mitchell", 4.0)])
def test_chunks(kind, width, monkeypatch):
    """1536 paths in chunks of at most 256: the splats of a chunk land on pixels of the chunks before and after it"""
    rd = ff.film_settings(kind, width)
    whole, _, _, ref, mag, count = checked(f"{kind} {width}, one chunk", rd)
    monkeypatch.setenv("YAFGPU_WF_CHUNK", "256")
    film, yi = device(rd)
    monkeypatch.delenv("YAFGPU_WF_CHUNK")
    assert_within(f"{kind} {width}, chunks of 256", film, ref, mag, count)
    assert_counts(yi, n_samples(rd))
    assert_within(f"{kind} {width}, chunks of 256 against one chunk", film, whole.astype(np.float64), mag, count, factor=2.0)


# ---- i. pipelined passes ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reuse_planes", [False, True])
def test_pipelined_passes(reuse_planes):
    rd = ff.film_settings("gauss", 1.5)
    runs = []
    for mode in (0, 1):
        yi = loaded(rd)
        yi.setPassPipelining(mode)
        yi.prepareRender()
        planes, counters = _passes(yi, 4, reuse_planes)
        _, _, ref, mag, count = composed(yi, rd)
        for k, p in enumerate(planes):
            assert_within(f"gauss 1.5, pipelining {mode}, pass {k}", p[0], ref, mag, count)
            assert not p[1:].any(), f"pass {k}: a wide filter wrote to the neighbour planes"
        runs.append(counters)
    assert np.array_equal(runs[0], runs[1]), runs
    n = n_samples(rd)
    assert (runs[0][0], runs[0][1], runs[0][5]) == (4 * n, 0, 4 * n)


# ---- j. the same render twice ----------------------------------------------------------------------------------------
def test_render_twice():
    """the atomics' order is the only freedom: two renders of one scene differ by rounding alone, and the second starts from zero"""
    rd = ff.film_settings("mitchell", 1.2)
    yi = loaded(rd)
    films = []
    for k in range(2):
        yi.render()
        films.append(yi.getFilm(ff.W, ff.H).copy())
        _, _, ref, mag, count = composed(yi, rd)
        assert_within(f"mitchell 1.2, render {k}", films[k], ref, mag, count)
        assert_counts(yi, n_samples(rd))
    assert_within("mitchell 1.2, second render against the first", films[1][..., 4:], films[0][..., 4:].astype(np.float64), mag[..., 4:], count, factor=2.0)
