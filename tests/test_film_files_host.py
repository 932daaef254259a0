"""Film files on the host (no GPU): the layout the writer produces, what the reader accepts and refuses, the film path of an interface,
and the reader and writer under AddressSanitizer + UBSan as a program of their own (tests/film_asan).

The layout is the reference's (ImageFilm::imageFilmSave / imageFilmLoad, imagefilm.cc:1560-1657, :1340-1465; strings file.cc:169-194),
little-endian:
    "YAF_FILMv1" 0x00 | u32 computer_node, base_sampling_offset, sampling_offset | i32 w, h, cx0, cx1, cy0, cy1, n_passes, n_aux
    | (n_passes + n_aux) x h x w x { f32 r, g, b, a, weight }"""
import os
import struct
import subprocess

import numpy as np
import pytest

from libyafaray_amd import interface
from libyafaray_amd.interface import Interface, read_film_file, write_film_file, film_last_error

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAGIC = b"YAF_FILMv1\0"
HEADER_BYTES = 11 + 44


def film_bytes(ints, *passes, magic=MAGIC):
    """a film file from its eleven header integers and its passes (float32 arrays)"""
    return magic + struct.pack("<3I8i", *ints) + b"".join(np.ascontiguousarray(p, "<f4").tobytes() for p in passes)


def small_film(h=1, w=2, seed=5):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((h, w, 5)).astype(np.float32)


def header_ints(w, h, n_passes=1, n_aux=0, node=3, base=7, offset=2, cx0=3, cy0=5):
    return (node, base, offset, w, h, cx0, cx0 + w, cy0, cy0 + h, n_passes, n_aux)


def test_written_file_has_the_reference_layout(tmp_path):
    h, w = 3, 5
    film = small_film(h, w)
    film[0, 0] = [np.float32(-0.0), np.float32(np.inf), np.float32(1e-42), np.float32(np.nan), np.float32(3.0)]      # every bit pattern travels as it is
    path = tmp_path / "frame - node 0003.film"
    assert write_film_file(path, {"computer_node": 3, "base_sampling_offset": 7, "sampling_offset": 2, "cx0": 3, "cy0": 5}, film), film_last_error()
    raw = path.read_bytes()
    assert len(raw) == 11 + 44 + h * w * 20
    assert raw[:10] == b"YAF_FILMv1" and raw[10] == 0
    assert tuple(np.frombuffer(raw, "<u4", 3, 11)) == (3, 7, 2)
    assert tuple(np.frombuffer(raw, "<i4", 8, 23)) == (w, h, 3, 3 + w, 5, 5 + h, 1, 0)
    payload = np.frombuffer(raw, "<f4", h * w * 5, HEADER_BYTES).reshape(h, w, 5)
    assert np.array_equal(payload.view(np.uint32), film.view(np.uint32))
    got = read_film_file(path)
    assert got, film_last_error()
    hdr, back = got
    assert hdr == dict(zip(interface.FILM_HEADER_FIELDS, (3, 7, 2, w, h, 3, 3 + w, 5, 5 + h, 1, 0)))
    assert back.shape == (h, w, 5) and np.array_equal(back.view(np.uint32), film.view(np.uint32))
    assert read_film_file(path, header_only=True) == hdr


def test_a_reference_shaped_file_reads_as_its_first_pass(tmp_path):
    """the reference always carries one auxiliary pass (renderpasses.cc:277-279): pass 0 is taken, the rest is skipped"""
    h, w = 2, 3
    combined, aux = small_film(h, w, 1), small_film(h, w, 2) + np.float32(100)
    path = tmp_path / "cpu - node 0001.film"
    path.write_bytes(film_bytes(header_ints(w, h, n_passes=1, n_aux=1, node=1), combined, aux))
    got = read_film_file(path)
    assert got, film_last_error()
    hdr, film = got
    assert (hdr["n_passes"], hdr["n_aux"], hdr["computer_node"]) == (1, 1, 1)
    assert np.array_equal(film.view(np.uint32), combined.view(np.uint32))
    # three passes and two auxiliary ones: still pass 0
    path.write_bytes(film_bytes(header_ints(w, h, n_passes=3, n_aux=2), combined, aux, aux, aux, aux))
    hdr, film = read_film_file(path)
    assert (hdr["n_passes"], hdr["n_aux"]) == (3, 2) and np.array_equal(film.view(np.uint32), combined.view(np.uint32))


FILM_2X1 = small_film(1, 2)
GOOD_2X1 = film_bytes(header_ints(2, 1), FILM_2X1)
assert len(GOOD_2X1) == 95


def rejected_files():
    """name -> (bytes, a word the error text must hold); every film is 2 x 1"""
    files = {f"truncated_{n:02d}": (GOOD_2X1[:n], "truncated") for n in range(len(GOOD_2X1))}      # every length from 0 to full size - 1
    files["one_extra_byte"] = (GOOD_2X1 + b"\0", "trailing")
    files["wrong_magic"] = (film_bytes(header_ints(2, 1), FILM_2X1, magic=b"YAF_FILMv2\0"), "magic")
    files["unterminated_magic"] = (film_bytes(header_ints(2, 1), FILM_2X1, magic=b"YAF_FILMv1!"), "unterminated")
    files["negative_w"] = (film_bytes(header_ints(-2, 1)[:3] + (-2,) + header_ints(2, 1)[4:], FILM_2X1), "negative")
    files["negative_n_passes"] = (film_bytes(header_ints(2, 1, n_passes=-1), FILM_2X1), "negative")
    files["two_billion_squared"] = (film_bytes(header_ints(2, 1)[:3] + (2_000_000_000, 2_000_000_000) + header_ints(2, 1)[5:], FILM_2X1), "promises")
    return files


REJECTED = rejected_files()


@pytest.mark.parametrize("name", sorted(REJECTED))
def test_rejected_file(tmp_path, name):
    data, word = REJECTED[name]
    path = tmp_path / "bad.film"
    path.write_bytes(data)
    mark = np.float32(-12345.0)
    out = np.full((1, 2, 5), mark, np.float32)
    assert read_film_file(path, out=out) is False
    err = film_last_error()
    assert word in err and "bad.film" in err, err
    assert (out == mark).all(), "the output buffer was written to"
    assert read_film_file(path, header_only=True) is False and word in film_last_error()


def test_missing_file_and_wrong_buffer_size(tmp_path):
    assert read_film_file(tmp_path / "none.film") is False and "cannot be opened" in film_last_error()
    path = tmp_path / "ok.film"
    path.write_bytes(GOOD_2X1)
    out = np.full(15, np.float32(7), np.float32)
    assert read_film_file(path, out=out) is False and "floats" in film_last_error()
    assert (out == 7).all()
    assert read_film_file(path), film_last_error()
    assert film_last_error() == ""


def test_film_path_round_trip(tmp_path):
    yi = Interface()
    assert yi.getFilmPath() == ""
    yi.setFilmPath(tmp_path / "out" / "frame0007")
    assert yi.getFilmPath() == str(tmp_path / "out" / "frame0007")
    yi.setFilmPath(None)
    assert yi.getFilmPath() == ""
    yi.setFilmPath("frame")
    assert yi.getFilmPath() == "frame"
    yi.setFilmPath("")
    assert yi.getFilmPath() == ""
    assert yi.getFilmResume() == (0, 0, 0)
    yi.close()


def test_reader_and_writer_under_sanitizers(tmp_path):
    """A program of its own (tests/film_asan/film_files_main.cpp, built with csrc/yafaray_image.cpp) reads, refuses and rewrites the
    same crafted files.  Nothing is loaded into Python and nothing is preloaded.

    A reader that allocated what a lying header asks for must die instead of passing.  AddressSanitizer cannot start under an
    address-space limit (its shadow memory is a reservation of terabytes), so the two halves run apart: the sanitized program with the
    sanitizer's own ceiling on a single allocation at the same 12 GB, and the same program built without a sanitizer under a 12 GB
    RLIMIT_AS."""
    import resource
    libasan = subprocess.run(["gcc", "-print-file-name=libasan.a"], capture_output=True, text=True).stdout.strip()      # linked in statically
    if not os.path.isabs(libasan) or not os.path.exists(libasan):
        pytest.skip("no libasan on this machine")
    files = tmp_path / "films"
    files.mkdir()
    for name, (data, _) in REJECTED.items():
        (files / f"bad_{name}.film").write_bytes(data)
    (files / "ok_one_pass.film").write_bytes(GOOD_2X1)
    (files / "ok_reference_shaped.film").write_bytes(film_bytes(header_ints(2, 1, n_passes=1, n_aux=1), FILM_2X1, FILM_2X1 + np.float32(1)))
    (files / "ok_empty_frame.film").write_bytes(film_bytes(header_ints(0, 0)))
    bins = tmp_path / "bin"
    subprocess.run(["bash", os.path.join(ROOT, "tests", "film_asan", "build.sh"), str(bins)], check=True, timeout=600, capture_output=True)
    expected = f"read 3, refused {len(REJECTED)}, failures 0"

    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:max_allocation_size_mb=12288", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(bins / "film_files_asan"), str(files)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and expected in r.stdout and "runtime error" not in r.stdout + r.stderr, f"rc {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}"

    def limit():
        resource.setrlimit(resource.RLIMIT_AS, (12 << 30, 12 << 30))
    r = subprocess.run([str(bins / "film_files_plain"), str(files)], capture_output=True, text=True, timeout=300, preexec_fn=limit)
    assert r.returncode == 0 and expected in r.stdout, f"rc {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}"
