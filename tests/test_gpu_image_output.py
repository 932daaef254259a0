"""Image file output on the device: the output stage (libyafaray_amd/csrc/yafgpu_output.hip) through yafaray_filmToImage, an image
output as the second output of a small render, and the render_xml tool.

The expected values of the output stage come from the route that was there before it: a film is loaded as the film of a resumed
one-pass render (film_save_load = "load-save" with AA_passes = 1 only combines the films: no path work, the film comes back as it went
in, x + 0 + 0 + 0), and yafaray_render's host loop hands it, pixel by pixel, to a ColorOutput's putPixel.  The float format must equal
those pixels bit for bit; the 8-bit and RGBE formats must equal the numpy restatement of the two packers (tests/image_output_fixture.py)
applied to them.  Every pixel is compared and there is no tolerance: both sides are the same float32 / float64 expressions."""
import os

import numpy as np
import pytest

from libyafaray_amd import Interface, interface, render_xml, scenes
from libyafaray_amd.interface import IMAGE_FLOAT, IMAGE_RGBA8, IMAGE_RGBE
from tests import image_output_fixture as iof
from tests import xml_writer

pytestmark = pytest.mark.gpu

F = np.float32
SHAPES = [(1, 1), (67, 5), (256, 3)]      # one pixel; no multiple of a wavefront or of the 256-thread block; three blocks
SPACES = [("sRGB", 1.0), ("XYZ", 1.0), ("LinearRGB", 1.0), ("Raw_Manual_Gamma", 2.2), ("Raw_Manual_Gamma", 1.8)]


@pytest.fixture(scope="module", autouse=True)
def torch_first():
    """(as in the other GPU modules: let torch open the GPU before the library does)"""
    import torch
    torch.cuda.init()


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def special_pixels():
    """rows of r, g, b, a, weight that between them take every branch of the output stage"""
    up = lambda v: np.nextafter(F(v), F(np.inf))
    down = lambda v: np.nextafter(F(v), F(-np.inf))
    t = F(0.0031308)
    px = [
        (0.5, 0.25, 0.125, 0.75, 0.0),                       # weight 0: a zero pixel whatever the colours are
        (-0.5, 0.25, -1e-3, 0.5, 1.0),                       # negative colours
        (-1.0, -2.0, -3.0, 1.0, 2.0),                        # all negative: black
        (0.1, 0.2, 0.3, -0.5, 1.0), (0.1, 0.2, 0.3, 1.5, 1.0), (0.1, 0.2, 0.3, 3.0, 4.0),      # alpha below 0 and above 1
        (t, down(t), up(t), 1.0, 1.0), (0.003, 0.0032, 0.0031, 0.5, 1.0), (2 * t, 2 * down(t), 2 * up(t), 1.0, 2.0),      # around the sRGB knee
        (1e-33, 5e-33, 2e-34, 1.0, 1.0), (F(1e-32), down(1e-32), 0.0, 1.0, 1.0), (up(1e-32), 0.0, 1e-35, 1.0, 1.0),          # around RGBE's 1e-32
        (3e-32, 1e-32, 1e-33, 0.5, 3.0), (0.0, 0.0, 0.0, 1.0, 1.0), (1e-38, 1e-39, 0.0, 1.0, 1.0),
        (1e10, 1.0, 1e-10, 1.0, 1.0), (1e20, 1e19, 1e18, 1.0, 1.0), (1e30, 1e29, 5e29, 1.0, 1.0), (3e30, 1e30, 1e25, 0.5, 3.0),      # the exponent byte
        (1.0, 1.0, 1.0, 1.0, 1.0), (up(1.0), down(1.0), 1.0, down(1.0), 1.0), (2.0, 0.5, 1.0, up(1.0), 1.0),                  # around 1: the clamp
        (0.3, 0.6, 0.9, 0.7, 3.0), (0.3, 0.6, 0.9, 0.7, 0.1), (7.0, 5.0, 3.0, 1.0, 7.0), (1.0, 1.0, 1.0, 1.0, 255.0),          # weights whose reciprocal rounds
    ]
    for e in range(-24, 25, 3):                               # exact powers of two
        px.append((2.0 ** e, 2.0 ** (e - 1), 2.0 ** (e + 1), 2.0 ** min(e, 0), 1.0))
        px.append((2.0 ** e, down(2.0 ** e), up(2.0 ** e) / 2, 1.0, 2.0 ** (e % 5)))
    for k in (1, 2, 3, 64, 127, 128, 129, 254, 255):          # one step under k / 255 truncates to k - 1, where rounding would give k
        px.append((down(F(k) / F(255)), up(F(k) / F(255)), F(k) / F(255), down(F(k) / F(255)), 1.0))
    for k in range(256):                                      # every k / 255 as float32 with weight 1: c * 255.f lands on k exactly
        px.append((F(k) / F(255), F(k * (1.0 / 255.0)), F(255 - k) / F(255), F(k) / F(255), 1.0))
    return np.array(px, dtype=F)


def build_film(w, h):
    sp = special_pixels()
    n = w * h
    film = np.zeros((n, 5), dtype=F)
    if n == 1:
        film[0] = (0.6, 0.0031, 1.7, 0.5, 3.0)
    else:
        rng = np.random.default_rng(w * 1000 + h)
        k = min(n, len(sp))
        film[:k] = sp[:k]
        rest = n - k
        wt = rng.uniform(0.5, 4.0, size=rest).astype(F)
        film[k:, :4] = (rng.uniform(-0.1, 1.4, size=(rest, 4)).astype(F) * wt[:, None]).astype(F)
        film[k:, 4] = wt
    assert np.isfinite(film).all()
    return film.reshape(h, w, 5)


class Collector:
    def __init__(self, w, h):
        self.px = np.full((h, w, 4), np.nan, dtype=F)
        self.flushed = 0

    def putPixel(self, view, x, y, rgba):
        self.px[y, x] = rgba
        return True

    def flush(self, view):
        self.flushed += 1


_HOST = {}


def host_route(tmp_path_factory, shape, space):
    """what putPixel receives from yafaray_render's host loop for build_film(*shape) in that colour space (computed once, shared)"""
    key = (shape, space)
    if key in _HOST:
        return _HOST[key]
    w, h = shape
    film = build_film(w, h)
    ykey = ("interface", shape)
    if ykey not in _HOST:
        yi = Interface(strict=True)
        scenes.load_scene(yi, scenes.cornell_soup(8, seed=2, res=(w, h)), scenes.render_settings(w, h, 1, bounces=1, film_save_load="load-save"))
        _HOST[ykey] = yi
    yi = _HOST[ykey]
    d = tmp_path_factory.mktemp("film")
    path = d / "frame"
    assert interface.write_film_file(str(path) + " - node 0000.film", {}, film), interface.film_last_error()
    yi.setFilmPath(path)
    yi.paramsSetString("color_space", space[0]); yi.paramsSetFloat("gamma", space[1])
    c = Collector(w, h)
    assert yi.render(output=c)
    assert yi.getFilmResume()[0] == 1 and c.flushed == 1 and yi.getRenderStats().camera_samples == 0
    assert np.array_equal(yi.getFilm(w, h), film), "the resumed one-pass render did not hand the film back as it went in"
    assert not np.isnan(c.px).any()
    c.px.setflags(write=False)
    _HOST[key] = c.px
    return c.px


@pytest.mark.parametrize("space", SPACES, ids=[f"{s}-{g}" for s, g in SPACES])
@pytest.mark.parametrize("shape", SHAPES, ids=[f"{w}x{h}" for w, h in SHAPES])
def test_film_to_image_equals_the_host_route_and_the_packers(tmp_path_factory, shape, space):
    w, h = shape
    film = build_film(w, h)
    want = host_route(tmp_path_factory, shape, space)
    got = interface.film_to_image(film, space[0], space[1], True, IMAGE_FLOAT)
    bad = np.nonzero((bits(got) != bits(want)).any(axis=-1))
    assert len(bad[0]) == 0, f"float: {len(bad[0])} of {w * h} pixels differ, first at {bad[1][0], bad[0][0]}: film {film[bad[0][0], bad[1][0]]} -> {got[bad[0][0], bad[1][0]]} vs {want[bad[0][0], bad[1][0]]}"
    for alpha in (True, False):
        got8 = interface.film_to_image(film, space[0], space[1], alpha, IMAGE_RGBA8)
        want8 = iof.pack_rgba8(want, alpha)
        bad = np.nonzero((got8 != want8).any(axis=-1))
        assert len(bad[0]) == 0, f"rgba8 alpha {alpha}: {len(bad[0])} pixels differ, first {want[bad[0][0], bad[1][0]]} -> {got8[bad[0][0], bad[1][0]]} vs {want8[bad[0][0], bad[1][0]]}"
    gote = interface.film_to_image(film, space[0], space[1], True, IMAGE_RGBE)
    wante = iof.pack_rgbe(want)
    bad = np.nonzero((gote != wante).any(axis=-1))
    assert len(bad[0]) == 0, f"rgbe: {len(bad[0])} pixels differ, first {want[bad[0][0], bad[1][0]]} -> {gote[bad[0][0], bad[1][0]]} vs {wante[bad[0][0], bad[1][0]]}"


def test_the_test_film_takes_every_branch():
    """what the cases above rest on: the 67 x 5 and 256 x 3 films hold every special pixel the docstring of special_pixels promises, and the
    numpy packers see both sides of their thresholds on them"""
    sp = special_pixels()
    assert len(sp) <= 67 * 5
    lin = iof.pack_rgba8(np.where(sp[:, 4:5] != 0, sp[:, :4] / np.where(sp[:, 4:5] != 0, sp[:, 4:5], 1), 0).astype(F), True)
    assert lin[-256:, 0].tolist() == list(range(256))                            # every 8-bit level comes out of the k / 255 rows
    assert lin[-265:-256, 0].tolist() == [0, 1, 2, 63, 126, 127, 128, 253, 254]  # and a step below them the level below: a truncation
    e = iof.pack_rgbe(np.maximum(sp[:, :4], 0))
    assert (e[:, 3] == 0).any() and e[:, 3].max() > 128 + 95 and e[:, 3][e[:, 3] > 0].min() < 128 - 95
    assert interface.film_to_image(np.zeros((2, 3, 5), F), "LinearRGB", 1.0, False, IMAGE_RGBA8).tolist() == [[[0, 0, 0, 255]] * 3] * 2
    with pytest.raises(interface.YafaRayError, match="colour space"):
        interface.film_to_image(np.zeros((2, 3, 5), F), "CMYK")
    with pytest.raises(interface.YafaRayError, match="pixel format"):
        interface.film_to_image(np.zeros((2, 3, 5), F), "sRGB", format=7)


# ---- an image output as the second output of a render ----------------------------------------------------------------------------------
W = H = 16


@pytest.fixture(scope="module")
def rendered():
    """a 16 x 16 render of cornell_soup, box filter, 2 samples -> (interface, the pixels its first output received)"""
    yi = Interface(strict=False)
    scenes.load_scene(yi, scenes.cornell_soup(40, seed=4, res=(W, H)), scenes.render_settings(W, H, 2, bounces=2))
    for k in ("color_space", "color_space2"):
        yi.paramsSetString(k, "sRGB")
    return yi


FILES = [("tga", False), ("tga", True), ("png", False), ("png", True), ("hdr", False)]


@pytest.mark.parametrize("file_type,alpha", FILES)
@pytest.mark.parametrize("border", [(0, 0, W, H), (5, 3, 24, 20)], ids=["fit", "border"])
def test_image_output_as_second_output(tmp_path, rendered, file_type, alpha, border):
    yi = rendered
    bx, by, iw, ih = border
    yi.paramsSetString("type", file_type); yi.paramsSetInt("width", iw); yi.paramsSetInt("height", ih); yi.paramsSetBool("alpha_channel", alpha)
    handler = yi._L.yafaray_createImageHandler(yi._h, b"second", 0)
    assert handler, yi.getLastError()
    yi.paramsSetInt("width", W); yi.paramsSetInt("height", H)
    path = tmp_path / f"second.{file_type}"
    out = yi.createImageOutput(handler, path, bx, by)
    c = Collector(W, H)
    yi.setOutput2(out)
    try:
        assert yi.render(output=c), yi.getLastError()
    finally:
        yi.setOutput2(None)
    assert c.flushed == 1 and not np.isnan(c.px).any() and c.px[..., :3].max() > 0.05
    full = np.zeros((ih, iw, 4), dtype=F)
    full[by:by + H, bx:bx + W] = c.px
    want = iof.pack_rgbe(full) if file_type == "hdr" else iof.pack_rgba8(full, alpha)
    inside = np.zeros((ih, iw), dtype=bool)
    inside[by:by + H, bx:bx + W] = True
    want[~inside] = 0                                    # outside the render window the image stays zero, the alpha byte too
    got = iof.decode_file(path, file_type)
    assert np.array_equal(got, want if (alpha or file_type == "hdr") else want[..., :3]), f"{int((got != (want if (alpha or file_type == 'hdr') else want[..., :3])).sum())} bytes differ"
    if border[0]:
        assert not got[~inside].any() and got[inside].any()
    # the image once more, as the only output of getRenderedImage: the same file
    first = path.read_bytes()
    os.remove(path)
    assert yi.getRenderedImage(out) and path.read_bytes() == first
    out.close()


def test_a_handler_smaller_than_the_render_is_refused_before_the_render(tmp_path, rendered):
    yi = rendered
    yi.paramsSetString("type", "png"); yi.paramsSetInt("width", W); yi.paramsSetInt("height", H - 1)
    handler = yi._L.yafaray_createImageHandler(yi._h, b"small", 0)
    yi.paramsSetInt("height", H)
    out = yi.createImageOutput(handler, tmp_path / "small.png")
    c = Collector(W, H)
    yi.setOutput2(out)
    try:
        assert not yi.render(output=c)
    finally:
        yi.setOutput2(None)
    err = yi.getLastError()
    assert "16 x 16" in err and "16 x 15" in err and "does not fit" in err, err
    assert c.flushed == 0 and np.isnan(c.px).all() and not os.path.exists(tmp_path / "small.png")
    # as the first output, into a directory that is not there: the render fails with the path and the cause
    yi.paramsSetInt("height", H)
    big = yi._L.yafaray_createImageHandler(yi._h, b"big", 0)
    lost = yi.createImageOutput(big, tmp_path / "missing" / "x.png")
    assert not yi.render(output=lost)
    assert "missing" in yi.getLastError() and "cannot be created" in yi.getLastError() and "No such file" in yi.getLastError(), yi.getLastError()
    out.close(); lost.close()


# ---- the tool --------------------------------------------------------------------------------------------------------------------------------
def test_render_xml_writes_the_film_of_its_render(tmp_path, capsys):
    """(the XML loader takes the frame's size from the file: the camera's resx / resy and the render's width / height have to agree, so the
    reference's 480 x 270 test scene cannot be rendered smaller; a 16 x 16 scene written here takes its place)"""
    xml = tmp_path / "scene.xml"
    xml_writer.write(xml, scenes.cornell_soup(40, seed=4, res=(W, H)), dict(scenes.render_settings(W, H, 2, bounces=2), color_space="sRGB"))
    out = tmp_path / "out.png"
    yi = render_xml.render_xml(xml, out, None, alpha=True)
    c = Collector(W, H)
    assert yi.getRenderedImage(c)
    got = iof.decode_file(out, "png")
    assert got.shape == (H, W, 4) and np.array_equal(got, iof.pack_rgba8(c.px, True)) and got[..., :3].any()
    # the command line: format by option, and a failure's exit status
    assert render_xml.main([str(xml), "-o", str(tmp_path / "cli.img"), "-f", "tga"]) == 0
    assert iof.decode_file(tmp_path / "cli.img", "tga").shape == (H, W, 3)
    assert "camera samples" in capsys.readouterr().out
    assert render_xml.main([str(xml), "-o", str(tmp_path / "cli.bmp")]) == 1
    assert render_xml.main([str(tmp_path / "absent.xml"), "-o", str(tmp_path / "x.png")]) == 1
