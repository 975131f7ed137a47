"""Inputs, serial reference and independent decoder shared by test_png_ref_cpu.py and test_gpu_png.py.

The decoder uses ``struct``, ``binascii.crc32`` and ``zlib.decompressobj`` only; the reference encoder is
tests/harness/png_ref.c compiled with gcc (the serial restatement of openpano_amd/csrc/png.hip)."""
import binascii
import ctypes as C
import os
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

import natural
from openpano_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "tests", "harness", "png_ref.c")
SEG = 61440          # bytes of filtered stream per segment (png.hip PNG_SEG, png_ref.c SEG)
SIGNATURE = b"\x89PNG\r\n\x1a\n"


def build_ref(tmpdir):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("gcc not available")
    so = os.path.join(str(tmpdir), "libpng_ref.so")
    subprocess.check_call([gcc, "-std=c11", "-O2", "-Wall", "-fPIC", "-shared", HARNESS, "-o", so])
    L = C.CDLL(so)
    L.png_ref_bound.restype = C.c_long
    L.png_ref_bound.argtypes = [C.c_int, C.c_int]
    L.png_ref_segment.restype = C.c_long
    L.png_ref_encode.restype = C.c_long
    L.png_ref_encode.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_long]
    assert L.png_ref_segment() == SEG
    return L


def ref_encode(L, rgb):
    """the harness's file for an (H, W, 3) uint8 array"""
    rgb = np.ascontiguousarray(rgb, np.uint8)
    h, w, _ = rgb.shape
    cap = L.png_ref_bound(h, w)
    out = np.empty(cap, np.uint8)
    n = L.png_ref_encode(rgb.ctypes.data_as(C.c_void_p), h, w, out.ctypes.data_as(C.c_void_p), cap)
    assert n > 0, n
    return out[:n].tobytes()


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)


def unfilter(F, h, w):
    """filtered scanlines -> (H, W, 3) uint8; numpy per row where the recurrence allows, asserting 0 <= type <= 4"""
    R = 3 * w
    F = np.frombuffer(F, np.uint8).reshape(h, R + 1)
    out = np.zeros((h, R), np.uint8)
    zero = np.zeros(R, np.uint8)
    for y in range(h):
        t = int(F[y, 0]); line = F[y, 1:]
        assert 0 <= t <= 4, f"row {y}: filter type {t}"
        up = out[y - 1] if y else zero
        if t == 0:
            out[y] = line
        elif t == 1:
            out[y] = np.cumsum(line.reshape(w, 3).astype(np.uint32), axis=0).astype(np.uint8).reshape(R)
        elif t == 2:
            out[y] = line + up
        else:
            cur = [0] * R; ln = line.tolist(); u = up.tolist()
            for x in range(R):
                a = cur[x - 3] if x >= 3 else 0
                c = u[x - 3] if x >= 3 else 0
                pred = (a + u[x]) >> 1 if t == 3 else _paeth(a, u[x], c)
                cur[x] = (ln[x] + pred) & 255
            out[y] = cur
    return out.reshape(h, w, 3)


def decode(png):
    """-> dict(h, w, pixels (H, W, 3) uint8, filtered bytes, idat payload bytes, n_idat); every structural rule asserted"""
    assert png[:8] == SIGNATURE
    pos = 8; chunks = []
    while pos < len(png):
        n, = struct.unpack(">I", png[pos: pos + 4])
        typ = png[pos + 4: pos + 8]; data = png[pos + 8: pos + 8 + n]
        crc, = struct.unpack(">I", png[pos + 8 + n: pos + 12 + n])
        assert len(data) == n and binascii.crc32(typ + data) & 0xFFFFFFFF == crc, f"chunk {typ} at {pos}: bad CRC"
        chunks.append((typ, data)); pos += 12 + n
    assert pos == len(png)
    types = [t for t, _ in chunks]
    assert types[0] == b"IHDR" and types[-1] == b"IEND" and set(types[1:-1]) == {b"IDAT"} and len(chunks[-1][1]) == 0, types[:4]
    w, h, depth, ctype, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, ctype, comp, filt, lace) == (8, 2, 0, 0, 0)
    payload = b"".join(d for t, d in chunks if t == b"IDAT")
    z = zlib.decompressobj()
    F = z.decompress(payload)
    assert z.eof and z.unused_data == b"" and z.unconsumed_tail == b""
    assert len(F) == h * (1 + 3 * w)
    return dict(h=h, w=w, pixels=unfilter(F, h, w), filtered=F, payload=payload, n_idat=len(types) - 2)


def _rand(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def _smooth(h, w, seed):
    """compressible but not trivial: a colour gradient plus low-amplitude noise"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([(x * 3 + y) % 256, (x + y * 2) % 256, (x * y // 7) % 256], axis=-1)
    return ((base + rng.integers(0, 4, (h, w, 3))) % 256).astype(np.uint8)


def _checker(h, w, cell):
    y, x = np.mgrid[0:h, 0:w]
    m = ((y // cell + x // cell) & 1).astype(bool)
    out = np.empty((h, w, 3), np.uint8)
    out[m] = (200, 30, 90); out[~m] = (10, 240, 17)
    return out


def quantise(canvas):
    """k_to_u8's expression (csrc/blend.hip): Color::NO (negative) -> 255, v * 255 in fp32, truncated"""
    v = np.where(canvas < 0, np.float32(1), canvas).astype(np.float32)
    return (v * np.float32(255)).astype(np.uint8)


def blended_canvas():
    from checkers import Oracle
    from openpano_amd.config import PanoConfig
    cfg = PanoConfig()
    views, homos = synth.pano_scene(3, 120, 160, seed=11, proj="flat")
    canvas, _ = Oracle(cfg).blend(views, homos, 0, 1, cfg)
    return quantise(canvas)


def natural_crop():
    return natural.crop_u8("uav", 300, 900, 400, 600)


# name -> builder; the stream length h * (1 + 3w) against SEG is what the size cases are about
CASES = {
    "1x1": lambda: _rand((1, 1, 3), 1),
    "1x700": lambda: _smooth(1, 700, 2),
    "700x1": lambda: _smooth(700, 1, 3),
    # 1 + 3w = 1000: SEG falls at byte 440 of row 61 (mid-row; 439 = 3 * 146 + 1: after the first byte of a pixel)
    "boundary_mid_pixel_150x333": lambda: _smooth(150, 333, 4),
    # 1 + 3w = 1024: SEG = 60 rows exactly
    "one_segment_60x341": lambda: _smooth(60, 341, 5),
    "two_segments_120x341": lambda: _smooth(120, 341, 6),
    # 2 SEG + 1 = 122881 = 1 + 3 * 40960
    "two_segments_plus_one_1x40960": lambda: _smooth(1, 40960, 7),
    "all255_763x7999": lambda: np.full((763, 7999, 3), 255, np.uint8),
    "random_97x211": lambda: _rand((97, 211, 3), 8),
    "random_one_segment_60x341": lambda: _rand((60, 341, 3), 9),
    "checker_200x300": lambda: _checker(200, 300, 8),
    "natural_400x600": natural_crop,
    "blended": blended_canvas,
}
NEEDS_PIL = {"natural_400x600"}


def case(name):
    if name in NEEDS_PIL and not natural.available():
        pytest.skip("PIL not available")
    return np.ascontiguousarray(CASES[name](), np.uint8)


def stored_bound(h, w):
    """size the file never exceeds: every segment stored in one block (SEG <= 65535: 5 bytes), one chunk per
    segment (12) plus IHDR, zlib-header, Adler and IEND chunks (4 x 12), signature 8, IHDR 13, zlib header + Adler 6"""
    n = h * (1 + 3 * w)
    nseg = -(-n // SEG)
    return n + 5 * nseg + 12 * (nseg + 4) + 8 + 13 + 6
