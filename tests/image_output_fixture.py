"""Test support for image file output: the two pixel packers restated in numpy, decoders for the three file formats written here in
plain numpy / zlib (nothing of the library is used to read its own files back), and the pixel cases the encoder tests share."""
import struct
import zlib

import numpy as np

TGA_ID = b"Image rendered with YafaRay"
TGA_FOOTER = b"\0" * 8 + b"TRUEVISION-XFILE.\0"
HDR_HEADER = "#?RADIANCE\n# Image created with YafaRay\nEXPOSURE=1\nFORMAT=32-bit_rle_rgbe\n\n-Y {h} +X {w}\n"


# ---- the packers (TgaPixelRgba::operator= / PngHandler::saveToFile:138-141; RgbePixel::operator=(const Rgb &)) -------------------------
def pack_rgba8(rgba, alpha):
    """(..., 4) float32 -> (..., 4) uint8: clampRgba01, then (uint8_t)(c * 255.f), a truncation; without alpha the alpha byte is 255"""
    c = np.asarray(rgba, dtype=np.float32)
    c = np.where(c < 0, np.float32(0), np.where(c > 1, np.float32(1), c)).astype(np.float32)
    out = (c * np.float32(255.0)).astype(np.float32).astype(np.int32).astype(np.uint8)
    if not alpha:
        out[..., 3] = 255
    return out


def pack_rgbe(rgba):
    """(..., 4) float32 -> (..., 4) uint8 r g b e: v = max(r, g, b); below 1e-32 four zero bytes; else v = (float)(frexp(v, &e) * 255.9999 / v)
    with the product and the quotient in float64, bytes (uint8_t)(c * v) and (uint8_t)(e + 128)"""
    c = np.asarray(rgba, dtype=np.float32)
    v = np.maximum(c[..., 0], np.maximum(c[..., 1], c[..., 2])).astype(np.float32)
    live = (v.astype(np.float64) >= 1e-32) & np.isfinite(v)      # (a largest channel that is not finite: four zero bytes, as the library defines it)
    vs = np.where(live, v, np.float32(1))
    m, e = np.frexp(vs)
    s = (m.astype(np.float64) * 255.9999 / vs.astype(np.float64)).astype(np.float32)
    out = np.zeros(c.shape[:-1] + (4,), dtype=np.uint8)
    for k in range(3):
        out[..., k] = (c[..., k] * s).astype(np.float32).astype(np.int32).astype(np.uint8)
    out[..., 3] = ((e.astype(np.int32) + 128) & 0xff).astype(np.uint8)
    out[~live] = 0
    return out


# ---- decoders ----------------------------------------------------------------------------------------------------------------------------
def decode_tga(data):
    """-> (h, w, 3 or 4) uint8 r g b [a]; checks the header, the id, the footer and the file's length"""
    (id_len, cmap_type, img_type, cm_first, cm_n, cm_bits, x0, y0, w, h, depth, desc) = struct.unpack("<BBBHHBHHHHBB", data[:18])
    assert (id_len, cmap_type, img_type, cm_first, cm_n, cm_bits, x0, y0) == (len(TGA_ID), 0, 2, 0, 0, 0, 0, 0), "TGA header"
    assert depth in (24, 32) and desc == (0x20 | (0x08 if depth == 32 else 0)), "uncompressed true colour, top-left origin, 8 alpha bits with 32"
    assert data[18:18 + id_len] == TGA_ID
    bpp = depth // 8
    assert len(data) == 18 + 27 + w * h * bpp + 26, "TGA length"
    assert data[-26:] == TGA_FOOTER
    px = np.frombuffer(data, dtype=np.uint8, count=w * h * bpp, offset=18 + id_len).reshape(h, w, bpp)
    return px[..., [2, 1, 0] + ([3] if bpp == 4 else [])].copy()


def decode_hdr(data):
    """-> (h, w, 4) uint8 r g b e; checks the header text and every scanline's signature, and that no byte is left over"""
    end = data.index(b"\n\n") + 2
    end = data.index(b"\n", end) + 1
    head = data[:end].decode("ascii")
    dims = head.splitlines()[-1].split()
    h, w = int(dims[1]), int(dims[3])
    assert head == HDR_HEADER.format(h=h, w=w), repr(head)
    pos = end
    out = np.zeros((h, w, 4), dtype=np.uint8)
    if w < 8 or w > 0x7fff:      # no run-length signature can hold such a width: flat pixels
        assert len(data) == pos + w * h * 4
        return np.frombuffer(data, dtype=np.uint8, offset=pos).reshape(h, w, 4).copy()
    for y in range(h):
        assert data[pos:pos + 4] == bytes([2, 2, w >> 8, w & 0xff]), f"scanline {y}: start signature"
        pos += 4
        for chan in range(4):
            x = 0
            while x < w:
                count = data[pos]; pos += 1
                if count > 128:
                    count &= 0x7f
                    assert count >= 2 and x + count <= w, "run length"
                    out[y, x:x + count, chan] = data[pos]; pos += 1
                else:
                    assert count >= 1 and x + count <= w, "literal length"
                    out[y, x:x + count, chan] = np.frombuffer(data, dtype=np.uint8, count=count, offset=pos); pos += count
                x += count
    assert pos == len(data), "bytes after the last scanline"
    return out


def decode_png(data):
    """-> (h, w, 3 or 4) uint8; checks the signature, every chunk's CRC, the header's fields and every row's filter byte"""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, []
    while pos < len(data):
        n, = struct.unpack(">I", data[pos:pos + 4])
        ctype, body = data[pos + 4:pos + 8], data[pos + 8:pos + 8 + n]
        crc, = struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])
        assert crc == (zlib.crc32(ctype + body) & 0xffffffff), f"CRC of {ctype!r}"
        chunks.append((ctype, body))
        pos += 12 + n
    assert pos == len(data) and chunks[0][0] == b"IHDR" and chunks[-1] == (b"IEND", b"")
    w, h, depth, ctype, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, comp, filt, lace) == (8, 0, 0, 0) and ctype in (2, 6)
    ch = 3 if ctype == 2 else 4
    raw = zlib.decompress(b"".join(b for t, b in chunks if t == b"IDAT"))
    stride = w * ch
    assert len(raw) == (stride + 1) * h
    out = np.zeros((h, stride), dtype=np.uint8)
    prev = np.zeros(stride, dtype=np.int32)
    for y in range(h):
        ft = raw[(stride + 1) * y]
        line = np.frombuffer(raw, dtype=np.uint8, count=stride, offset=(stride + 1) * y + 1).astype(np.int32)
        assert ft in (0, 1, 2, 3, 4), "row filter"
        if ft == 2:
            line = (line + prev) & 0xff
        elif ft != 0:
            cur = np.zeros(stride, dtype=np.int32)
            for i in range(stride):
                a = cur[i - ch] if i >= ch else 0
                b = prev[i]
                c = prev[i - ch] if i >= ch else 0
                if ft == 1:
                    p = a
                elif ft == 3:
                    p = (a + b) >> 1
                else:
                    q = a + b - c
                    pa, pb, pc = abs(q - a), abs(q - b), abs(q - c)
                    p = a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)
                cur[i] = (line[i] + p) & 0xff
            line = cur
        out[y] = line
        prev = line
    return out.reshape(h, w, ch)


def decode_file(path, file_type):
    with open(path, "rb") as f:
        data = f.read()
    return {"tga": decode_tga, "hdr": decode_hdr, "pic": decode_hdr, "png": decode_png}[file_type](data)


# ---- what the project's own decoders (createTexture + getTextureImage, LinearRGB, texture_optimization none) return for known bytes ------
def texels_of_rgba8(px, file_type, alpha):
    """TgaHandler::loadFromFile: (float)(byte * INV_255) with INV_255 a double; PngHandler: byte * (float)INV_8.  No alpha in the file: 1"""
    b = np.asarray(px, dtype=np.uint8)
    if file_type == "tga":
        t = (b.astype(np.float64) * 0.00392156862745098039).astype(np.float32)
    else:
        t = b.astype(np.float32) * np.float32(0.00392156862745098039)
    if not alpha:
        t[..., 3] = 1.0
    return t


def texels_of_rgbe(px):
    """RgbePixel::getRgba: f = ldexp(1.0, e - 136) as a float, (f * r, f * g, f * b, 1); all zero where e is 0"""
    b = np.asarray(px, dtype=np.uint8)
    f = np.ldexp(1.0, b[..., 3].astype(np.int32) - 136).astype(np.float32)
    t = np.ones(b.shape[:-1] + (4,), dtype=np.float32)
    for k in range(3):
        t[..., k] = np.where(b[..., 3] != 0, f * b[..., k].astype(np.float32), np.float32(0))
    return t


# ---- the pixel cases of the encoder tests ------------------------------------------------------------------------------------------------
def run_rows():
    """(3, 300, 4) uint8: rows that between them hold runs of 1, 3, 4, 127, 128 and 200 equal bytes in every channel — 127 is the longest
    run one block holds, 128 the longest literal block — with the runs in another order in each channel"""
    def filled(runs):      # the runs asked for, then single bytes and short runs up to the row's 300
        runs, k = list(runs), 0
        while sum(runs) < 300:
            runs.append(min((1, 1, 1, 3, 1, 4)[k % 6], 300 - sum(runs)))
            k += 1
        return runs

    def line(runs, seed):      # neighbouring runs differ, so every run is as long as it says; no byte is 0
        vals, out, last = np.random.default_rng(seed), [], -1
        for n in runs:
            v = int(vals.integers(1, 256))
            while v == last:
                v = int(vals.integers(1, 256))
            out += [v] * n
            last = v
        assert len(out) == 300
        return out
    layouts = [filled([1, 3, 4, 127]), filled([128, 1, 4, 3]), filled([200, 1, 3, 4])]
    img = np.zeros((3, 300, 4), dtype=np.uint8)
    for chan in range(4):
        for row in range(3):
            runs = layouts[(row + chan) % 3]
            img[row, :, chan] = line(runs if chan % 2 == 0 else runs[::-1], 100 * chan + row)
    return img


def pixel_cases():
    """name -> (h, w, 4) uint8.  As RGBE bytes they are valid pixels: an exponent byte of 0 only with zero mantissas, and no pixel whose three
    mantissas are all 1 (a flat scanline would read it as an old-style run)"""
    rng = np.random.default_rng(20240607)
    cases = {}
    for w, h in [(1, 1), (7, 3), (9, 2), (67, 5)]:
        px = rng.integers(0, 256, size=(h, w, 4), dtype=np.uint8)
        px[..., 3] = np.maximum(px[..., 3], 1)
        px[..., 0] = np.where((px[..., :3] == 1).all(axis=-1), 2, px[..., 0])
        if w * h > 4:
            px[h // 2, w // 2] = 0          # a black pixel
            px[0, w - 1, 3] = 255           # the largest exponent / full alpha
        cases[f"{w}x{h}"] = px
    cases["runs_300x3"] = run_rows()
    return cases
