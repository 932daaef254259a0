"""Image file output on the host (no GPU): the image handler factory, the three encoders (libyafaray_amd/csrc/yafaray_image.cpp) behind
yafaray_writeImageFile, and an image output driven pixel by pixel.

The encoders restate TgaHandler / HdrHandler / PngHandler ::saveToFile (imagehandler_tga.cc:47, imagehandler_hdr.cc:392-533,
imagehandler_png.cc:64).  Every file is read back two ways — by the project's own decoder (createTexture + getTextureImage with
color_space LinearRGB and texture_optimization none, so that the decoder neither linearises nor re-quantises) and by decoders written
in tests/image_output_fixture.py in plain numpy / zlib — and both must give the input bytes back exactly.

One limit of the first way: the project's HDR decoder restates the reference's reader of FLAT scanlines, which keeps pixel 0 of a
scanline only (imagehandler_hdr.cc:296 steps by the width).  For the two widths below 8 that way therefore sees column 0; the numpy
decoder sees every pixel."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from libyafaray_amd import Interface, interface
from tests import image_output_fixture as iof

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = iof.pixel_cases()
FILE_TYPES = [("tga", False), ("tga", True), ("png", False), ("png", True), ("hdr", False)]


def fresh(strict=False):
    yi = Interface(strict=strict)
    assert yi.startScene(0)
    return yi


# ---- the factory ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("file_type", ["tga", "hdr", "pic", "png"])
def test_handler_factory_accepts_the_three_formats(file_type):
    yi = fresh()
    for k, extra in enumerate([{}, {"alpha_channel": True}, {"alpha_channel": False, "for_output": True}, {"denoiseEnabled": False, "img_grayscale": False},
                               {"denoiseHLum": 3, "denoiseHCol": 3, "denoiseMix": 0.8}]):
        yi.paramsClearAll()
        yi.paramsSet(dict({"type": file_type, "width": 5 + k, "height": 3}, **extra))
        assert yi.createImageHandler(f"ih{k}"), yi.getLastError()
    # for_output = false: accepted without a size, and an output refuses the handler
    yi.paramsClearAll(); yi.paramsSet({"type": file_type, "for_output": False})
    h = yi.createImageHandler("input")
    assert h, yi.getLastError()
    assert yi.createImageOutput(h, "unused." + file_type) is None and "for_output" in yi.getLastError()
    # not in the table: the name stays free
    yi.paramsClearAll(); yi.paramsSet({"type": file_type, "width": 2, "height": 2})
    assert yi._L.yafaray_createImageHandler(yi._h, b"loose", 0) and yi._L.yafaray_createImageHandler(yi._h, b"loose", 0)
    yi.close()


def test_handler_factory_refusals_name_their_cause():
    yi = fresh()
    yi.paramsClearAll()
    assert not yi.createImageHandler("ih") and "createImageHandler" in yi.getLastError() and "type" in yi.getLastError()      # the bare call
    size = {"width": 4, "height": 4}
    for params, needles in [
        (dict(size), ["type"]),
        (dict(size, type="jpg"), ["jpg", "no encoder"]), (dict(size, type="jpeg"), ["jpeg", "no encoder"]), (dict(size, type="tif"), ["tif", "no encoder"]),
        (dict(size, type="tiff"), ["tiff", "no encoder"]), (dict(size, type="exr"), ["exr", "no encoder"]),
        (dict(size, type="bmp"), ["unknown image type", "bmp"]),
        (dict(type="tga"), ["width 0", "height 0"]), (dict(type="png", width=4, height=0), ["height 0"]), (dict(type="hdr", width=-3, height=2), ["width -3"]),
        (dict(size, type="png", denoiseEnabled=True), ["denoiseEnabled", "OpenCV"]),
        (dict(size, type="tga", img_grayscale=True), ["img_grayscale"]),
        (dict(type="tga", width=70000, height=2), ["65535"]),
        (dict(type="png", width=65536, height=65536), ["2^26"]),
    ]:
        yi.paramsClearAll(); yi.paramsSet(params)
        assert not yi.createImageHandler("refused"), params
        for n in needles:
            assert n in yi.getLastError(), (params, yi.getLastError())
    yi.paramsClearAll(); yi.paramsSet(dict(size, type="tga"))
    assert yi.createImageHandler("twice")
    assert not yi.createImageHandler("twice") and "already exists" in yi.getLastError()
    h = yi.createImageHandler("third")
    assert yi.createImageOutput(h, "x.tga", -1, 0) is None and "negative border" in yi.getLastError()
    assert yi.createImageOutput(h, "", 0, 0) is None
    assert yi.createImageOutput(None, "x.tga") is None
    yi.clearAll()      # releases the handlers: the stale handle is recognised, not followed
    assert yi.createImageOutput(h, "x.tga") is None and "not one of this interface's" in yi.getLastError()
    yi.close()


# ---- the encoders --------------------------------------------------------------------------------------------------------------------------
def project_decode(path):
    yi = Interface(strict=True)
    yi.startScene(0)
    yi.paramsClearAll()
    yi.paramsSet({"type": "image", "filename": str(path), "color_space": "LinearRGB", "texture_optimization": "none"})
    assert yi.createTexture("t")
    px = yi.getTextureImage("t")
    yi.close()
    return px


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("file_type,alpha", FILE_TYPES)
def test_written_files_read_back_exactly(tmp_path, case, file_type, alpha):
    px = CASES[case]
    h, w = px.shape[:2]
    path = tmp_path / f"{case}.{file_type}"
    assert interface.write_image_file(path, file_type, px, alpha), interface.film_last_error()
    # the test's own decoder: header, footer, pixel order / header text, run-length blocks / chunks, CRCs, filter bytes
    got = iof.decode_file(path, file_type)
    want = px if (alpha or file_type == "hdr") else px[..., :3]
    assert got.shape == want.shape and np.array_equal(got, want), f"{case} {file_type}: {int((got != want).sum())} bytes differ"
    if file_type == "tga":
        assert os.path.getsize(path) == 18 + 27 + w * h * (4 if alpha else 3) + 26
    # the project's decoder
    tex = project_decode(path)
    assert tex.shape == (h, w, 4)
    if file_type == "hdr":
        expect = iof.texels_of_rgbe(px)
        if w < 8:      # flat scanlines: the decoder keeps a scanline's first pixel only (see the module's docstring); the rest stay zero
            assert np.array_equal(tex[:, 0], expect[:, 0]) and not tex[:, 1:].any()
            return
    else:
        expect = iof.texels_of_rgba8(px, file_type, alpha)
    assert np.array_equal(tex.view(np.uint32), expect.view(np.uint32)), f"{case} {file_type}: {int((tex != expect).sum())} texels differ"


def test_hdr_scanlines_use_the_references_blocks(tmp_path):
    """writeScanline's choices, on a row where they can be told apart: a run of 4 or more becomes a run block, shorter repeats stay literal
    unless they open the scanline, a literal block holds at most 128 bytes and a run block at most 127"""
    row = np.zeros((1, 300, 4), dtype=np.uint8)
    row[0, :, 0] = [9, 9] + [5] * 200 + list(range(1, 99))                  # a short run at the start, a long run, literals
    row[0, :, 1] = (list(range(1, 131)) * 3)[:300]                         # 300 literals
    row[0, :, 2] = 7                                                       # one value
    row[0, :, 3] = [128] * 3 + [129] * 4 + [130] * 293
    assert interface.write_image_file(tmp_path / "row.hdr", "hdr", row)
    data = (tmp_path / "row.hdr").read_bytes()
    body = data[len(iof.HDR_HEADER.format(h=1, w=300)):]
    assert body[:4] == bytes([2, 2, 1, 44])
    want = bytes([128 + 2, 9, 128 + 127, 5, 128 + 73, 5, 98] + list(range(1, 99)))                     # channel 0
    lit = (list(range(1, 131)) * 3)[:300]
    want += bytes([128] + lit[:128] + [128] + lit[128:256] + [44] + lit[256:])                          # channel 1
    want += bytes([128 + 127, 7, 128 + 127, 7, 128 + 46, 7])                                            # channel 2
    want += bytes([128 + 3, 128, 128 + 4, 129, 128 + 127, 130, 128 + 127, 130, 128 + 39, 130])        # channel 3
    assert body[4:] == want


def test_unwritable_paths_and_overflowing_sizes_are_refused(tmp_path):
    px = CASES["7x3"]
    for file_type in ("tga", "png", "hdr"):
        assert not interface.write_image_file(tmp_path / "no" / "such" / f"dir.{file_type}", file_type, px)
        err = interface.film_last_error()
        assert "cannot be created" in err and "No such file or directory" in err and "dir." + file_type in err, err
    assert not interface.write_image_file(tmp_path / "x.jpg", "jpg", px) and "no encoder" in interface.film_last_error()
    # sizes: a one-pixel buffer behind a size of 2^32 pixels and more — refused before anything is allocated or read
    L = interface.load()
    one = (C.c_uint8 * 4)(1, 2, 3, 4)
    for w, h in [(65536, 65536), (2**31 - 1, 2**31 - 1), (2**31 - 1, 1), (8193, 8193), (0, 4), (4, 0), (-1, 1)]:
        for file_type in (b"tga", b"png", b"hdr"):
            assert not L.yafaray_writeImageFile(str(tmp_path / "big").encode(), file_type, w, h, 1, one)
            err = interface.film_last_error()
            assert "image size" in err and str(w) in err, err
    assert not os.path.exists(tmp_path / "big")
    assert not L.yafaray_writeImageFile(str(tmp_path / "null").encode(), b"png", 1, 1, 0, None) and "no pixels" in interface.film_last_error()


def test_encoders_under_sanitizers(tmp_path):
    """tests/image_write_cases.cpp, built with csrc/yafaray_image.cpp under AddressSanitizer + UBSan as a program of its own, writes the
    same cases: its files are byte for byte the library's, its refusals have causes, and the sanitizers report nothing"""
    files = tmp_path / "cases"
    files.mkdir()
    for name, px in CASES.items():
        stem = "case_" + name
        (files / f"{stem}.px").write_bytes(px.tobytes())
    exe = tmp_path / "image_write_cases"
    src = os.path.join(ROOT, "libyafaray_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-g", "-O1", "-Wall",
                    "-I" + src, os.path.join(ROOT, "tests", "image_write_cases.cpp"), os.path.join(src, "yafaray_image.cpp"), "-o", str(exe), "-lz"],
                   check=True, timeout=600, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:max_allocation_size_mb=4096", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe), str(files)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and f"wrote {5 * len(CASES)}, refused 28, failures 0" in r.stdout and "runtime error" not in r.stdout + r.stderr, \
        f"rc {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}"
    for name, px in CASES.items():
        stem = "case_" + name
        for file_type, alpha in FILE_TYPES:
            mine = tmp_path / f"lib_{stem}.{file_type}"
            assert interface.write_image_file(mine, file_type, px, alpha)
            theirs = files / f"{stem}{'_a' if alpha else ''}.{file_type}"
            assert mine.read_bytes() == theirs.read_bytes(), f"{stem} {file_type} alpha {alpha}"


# ---- an image output driven pixel by pixel -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("file_type,alpha", FILE_TYPES)
def test_callback_table_driven_pixel_by_pixel_writes_the_same_file(tmp_path, file_type, alpha):
    """A foreign caller of the callback table: putPixel stores at (x + bx, y + by), flush packs on the host and saves.  The file is the one
    writeImageFile writes for the same pixels packed by the numpy restatement of the packers, margin included."""
    rng = np.random.default_rng(5)
    w, h, bx, by, W, H = 9, 4, 2, 1, 13, 6
    rgba = rng.uniform(-0.2, 1.3, size=(h, w, 4)).astype(np.float32)
    rgba[0, :, :3] = (np.arange(w, dtype=np.float32)[:, None] * 28 / 255).astype(np.float32)      # k / 255 values: the truncation shows
    rgba[1, 0, :3] = [1e-33, 1e-34, 0]
    rgba[1, 1, :3] = [4.0, 0.5, 1e30]
    rgba[1, 2, :3] = [2.0 ** -7, 2.0 ** -9, 0.0]
    yi = fresh(strict=True)
    yi.paramsClearAll(); yi.paramsSet({"type": file_type, "width": W, "height": H, "alpha_channel": alpha})
    out = yi.createImageOutput(yi.createImageHandler("ih"), tmp_path / f"driven.{file_type}", bx, by)
    table = out.callbacks().contents
    assert table.user and table.putPixel and table.flush
    for y in range(h):
        for x in range(w):
            assert out.putPixel(0, x, y, rgba[y, x])
    assert out.putPixel(0, W, 0, (1, 1, 1, 1)) and out.putPixel(0, -bx - 1, 0, (1, 1, 1, 1))      # outside the image: dropped
    assert out.flush(0), out.getLastError()
    full = np.zeros((H, W, 4), dtype=np.float32)
    full[by:by + h, bx:bx + w] = rgba
    # (RgbePixel's cast of a negative product is undefined; the library packs a negative channel to the byte 0, like a clamped one)
    packed = iof.pack_rgbe(np.maximum(full, 0)) if file_type == "hdr" else iof.pack_rgba8(full, alpha)
    ref = tmp_path / f"reference.{file_type}"
    assert interface.write_image_file(ref, file_type, packed, alpha)
    assert (tmp_path / f"driven.{file_type}").read_bytes() == ref.read_bytes()
    got = iof.decode_file(tmp_path / f"driven.{file_type}", file_type)
    assert got.shape[:2] == (H, W) and not got[:by, :, :3].any() and not got[:, :bx, :3].any() and not got[by + h:, :, :3].any() and not got[:, bx + w:, :3].any()
    # a path that cannot be written: flush reports it
    bad = yi.createImageOutput(yi.createImageHandler("ih2"), tmp_path / "missing" / f"x.{file_type}")
    assert bad.putPixel(0, 0, 0, (1, 1, 1, 1)) and not bad.flush(0)
    assert "cannot be created" in bad.getLastError() and "missing" in bad.getLastError()
    out.close(); bad.close(); yi.close()


def test_render_refuses_a_window_that_does_not_fit_before_anything_runs(tmp_path):
    """no scene at all: were the fit checked after the set-up, the render would fail on the missing camera instead"""
    yi = fresh()
    yi.paramsClearAll(); yi.paramsSet({"type": "png", "width": 12, "height": 12})
    out = yi.createImageOutput(yi.createImageHandler("ih"), tmp_path / "small.png", 2, 0)
    yi.paramsClearAll(); yi.paramsSet({"width": 11, "height": 12})
    assert not yi.render(output=out)
    err = yi.getLastError()
    assert "11 x 12" in err and "12 x 12" in err and "(2, 0)" in err and "does not fit" in err, err
    yi.setOutput2(out)
    assert not yi.render() and "does not fit" in yi.getLastError()
    yi.paramsClearAll(); yi.paramsSet({"width": 10, "height": 12, "images_autosave_interval_type": "pass-interval"})
    assert not yi.render() and "images_autosave_interval_type" in yi.getLastError()
    yi.setOutput2(None)
    assert not os.path.exists(tmp_path / "small.png")
    out.close(); yi.close()


def test_new_symbols_are_listed_and_exported():
    lib = C.CDLL(interface.lib_path())
    for n in ["yafaray_createImageHandler", "yafaray_createImageOutput", "yafaray_destroyImageOutput", "yafaray_imageOutputCallbacks", "yafaray_imageOutputLastError",
              "yafaray_filmToImage", "yafaray_writeImageFile"]:
        assert n in interface.C_API_SYMBOLS and hasattr(lib, n), n
    for n in ["yafgpu_film_to_image", "yafgpu_scene_film_to_image", "yafgpu_image_bytes"]:
        assert n in interface.GPU_ABI_SYMBOLS and hasattr(lib, n), n
    from tests import test_abi
    for header, listed in [("yafaray_c_api.h", interface.C_API_SYMBOLS), ("yafgpu.h", interface.GPU_ABI_SYMBOLS)]:
        assert set(listed) == set(test_abi.declared_functions(header))
