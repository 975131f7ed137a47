"""CPU: the host EXIF reader (openpano_amd/csrc/jpeg_exif.hpp behind op_jpeg_exif).  No GPU.

1. op_jpeg_exif gives the constructed (orientation, focal35) for every variant of tests/exif_craft.py -- well-formed, junk
   ((1, 0), never an error) and the edge placements -- at every orientation, on several fixtures;
2. op_jpeg_probe still accepts every spliced file, with the stored shape;
3. the return codes: NULL and a negative size are OP_ERR_INVALID, a file without SOI is what op_jpeg_probe says, a header that
   ends early is no error, either output may be NULL;
4. where Pillow imports: for every well-formed variant x orientation 1..8, ImageOps.exif_transpose of the file equals the
   index map (exif_craft.orient_map) of the serial restatement's decode, and getexif() agrees on the orientation;
5. the sanitizer program tests/harness/jpeg_exif_fuzz.cc: a stand-alone binary built with -fsanitize=address,undefined, more
   than 2000 seeded mutations of three crafted segments; nothing is loaded into Python and nothing is preloaded."""
import ctypes as C
import io
import os
import shutil
import subprocess

import numpy as np
import pytest

import exif_craft as X
import jpeg_dec_cases as D
from openpano_amd import hip

FUZZ = os.path.join(D.ROOT, "tests", "harness", "jpeg_exif_fuzz.cc")
BASES = ("size_17x17_420", "size_8x8_444", "grey_37x53", "rst3_37x53_444")
FOCAL = 28


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return D.build_ref(tmp_path_factory.mktemp("jpegexifref"))


def _raw(data, size=None, want_o=True, want_f=True):
    o, f = C.c_int(-7), C.c_int(-7)
    r = hip.lib().op_jpeg_exif(data, len(data) if size is None else size, C.byref(o) if want_o else None, C.byref(f) if want_f else None)
    return r, o.value, f.value


def test_exports():
    assert hip.lib().op_abi_version() == 12
    assert hasattr(hip.lib(), "op_jpeg_exif") and hasattr(hip.lib(), "op_views_decode_jpeg_oriented")


@pytest.mark.parametrize("name", sorted(X.ALL))
def test_every_variant(name):
    for base in BASES:
        jpg = D.data(base)
        for o in range(1, 9):
            focal = FOCAL + o
            f, want = X.ALL[name](jpg, o, focal)
            assert f != jpg
            assert _raw(f) == (D.OP_OK,) + want, (name, base, o)
            assert hip.jpeg_exif(f) == want
            assert hip.jpeg_probe(f)[:2] == hip.jpeg_probe(jpg)[:2] == (D.DIGESTS[base]["h"], D.DIGESTS[base]["w"]), (name, base, o)


def test_groups_are_what_they_say():
    jpg = D.data(BASES[0])
    assert all(X.JUNK[k](jpg, 6, FOCAL)[1] == (1, 0) for k in X.JUNK)
    assert {X.WELL_FORMED[k](jpg, 6, FOCAL)[1][0] for k in X.WELL_FORMED} == {1, 6}      # 1: the variant without the tag
    assert {X.WELL_FORMED[k](jpg, 6, FOCAL)[1][1] for k in X.WELL_FORMED} == {0, FOCAL}
    assert hip.jpeg_exif(jpg) == (1, 0)                                                   # no EXIF at all
    assert hip.jpeg_exif(D.data("exif_com_37x53_422"))[0] in range(1, 9)                  # the fixture Pillow wrote with an Exif block


def test_return_codes():
    jpg = X.with_orientation(D.data(BASES[0]), 6)
    L = hip.lib()
    assert L.op_jpeg_exif(None, 10, None, None) == D.OP_ERR_INVALID and b"op_jpeg_exif" in L.op_last_error()
    assert _raw(jpg, size=-1)[0] == D.OP_ERR_INVALID
    assert _raw(jpg, want_o=False) == (D.OP_OK, -7, 0) and _raw(jpg, want_f=False) == (D.OP_OK, 6, -7)
    assert L.op_jpeg_exif(jpg, len(jpg), None, None) == D.OP_OK
    for bad in (b"", b"\xff", b"\xff\xd8\xff", b"\x89PNG\r\n\x1a\n" + bytes(40), jpg[1:]):
        h = C.c_int()
        probe = L.op_jpeg_probe(bad, len(bad), C.byref(h), None, None)
        assert probe == D.OP_ERR_INVALID and _raw(bad)[0] == probe, bad[:8]
        with pytest.raises(hip.OpenPanoHipError, match="error -1: op_jpeg_exif: no SOI"):
            hip.jpeg_exif(bad)
    # a header that ends early is the decoder's to refuse, not the reader's: whatever was read before the end counts
    at = jpg.index(b"\xff\xe1")
    n = int.from_bytes(jpg[at + 2: at + 4], "big")
    assert _raw(jpg[: at + 2 + n]) == (D.OP_OK, 6, 0)
    for cut in range(4, at + 2 + n):
        assert _raw(jpg[:cut]) == (D.OP_OK, 1, 0), cut
    assert _raw(jpg[:2] + b"\x00\x00" + jpg[2:]) == (D.OP_OK, 1, 0)      # no marker where a segment should begin


def _pillow():
    try:
        from PIL import Image, ImageOps, features
    except ImportError:
        return None
    return (Image, ImageOps) if features.check("jpg") else None


def test_well_formed_variants_equal_pillow(ref):
    pil = _pillow()
    if pil is None:
        pytest.skip("Pillow with libjpeg not available")
    Image, ImageOps = pil
    for base in ("size_17x17_420", "size_40x56_420"):
        jpg = D.data(base)
        stored = D.ref_decode(ref, jpg)
        assert D.digest(stored) == D.DIGESTS[base]["sha256"]
        for name in sorted(X.WELL_FORMED):
            for o in range(1, 9):
                f, (want_o, _) = X.WELL_FORMED[name](jpg, o, FOCAL)
                im = Image.open(io.BytesIO(f))
                assert im.getexif().get(X.ORIENTATION, 1) == want_o, (name, o)
                got = np.asarray(ImageOps.exif_transpose(im).convert("RGB"))
                want = X.orient_map(stored, want_o)
                assert got.shape == want.shape and np.array_equal(got, want), (base, name, o)


def test_orient_map_is_the_table():
    s = np.arange(5 * 7 * 3, dtype=np.uint8).reshape(5, 7, 3)
    h, w = 5, 7
    for o in range(1, 9):
        v = X.orient_map(s, o)
        assert v.shape == ((h, w, 3) if o < 5 else (w, h, 3))
        for y in range(v.shape[0]):
            for x in range(v.shape[1]):
                want = {1: (y, x), 2: (y, w - 1 - x), 3: (h - 1 - y, w - 1 - x), 4: (h - 1 - y, x),
                        5: (x, y), 6: (h - 1 - x, y), 7: (h - 1 - x, w - 1 - y), 8: (x, w - 1 - y)}[o]
                assert np.array_equal(v[y, x], s[want]), (o, y, x)
    assert len({X.orient_map(s, o).tobytes() for o in range(1, 9)}) == 8


def test_sanitizer_program(tmp_path):
    """host code only, as a program of its own: nothing is loaded into Python and nothing is preloaded"""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "jpeg_exif_fuzz")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", D.CSRC, FUZZ, "-o", exe])
    jpg = D.data("size_8x8_444")
    crafted = [("orient_last", 6), ("MM_focal_sub", 3), ("focal_sub_wins", 8)]
    paths, want = [], []
    for name, o in crafted:
        f, w = X.WELL_FORMED[name](jpg, o, FOCAL)
        p = tmp_path / (name + ".jpg")
        p.write_bytes(f)
        paths.append(str(p)); want.append("%d %d" % w)
    r = subprocess.run([exe] + paths, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    lines = r.stdout.strip().splitlines()
    assert [l.rsplit(": ", 1)[1] for l in lines[:3]] == want, lines[:3]
    assert lines[-1].startswith("mutations ") and int(lines[-1].split()[1]) >= 2000 + 3, lines[-1]
