"""Inputs, serial reference and marker walk shared by test_jpeg_ref_cpu.py and test_gpu_jpeg.py.

The reference encoder is tests/harness/jpeg_ref.c compiled with gcc (the serial restatement of openpano_amd/csrc/jpeg.hip,
DESIGN.md section 13); its jpeg_ref_stats says what the last encode went through.  walk() checks a file's marker structure
with ``struct`` only.  Pillow (libjpeg) is the independent oracle of the CPU test and is never needed by a GPU test."""
import ctypes as C
import functools
import io
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import png_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "tests", "harness", "jpeg_ref.c")
KERNEL = os.path.join(ROOT, "openpano_amd", "csrc", "jpeg.hip")
S444, S420 = 0, 1                       # OP_JPEG_444, OP_JPEG_420
RI = {S444: 32, S420: 8}                # MCUs per restart interval (jpeg.hip OP_JPEG_RI_444 / _420, the same knobs in jpeg_ref.c)
BLOCKS = {S444: 3, S420: 6}             # blocks per MCU
BLOCK_BYTES = 208                       # worst case of one block: 20 + 63 * 26 bits
SLOT = {s: 2 * BLOCK_BYTES * RI[s] * BLOCKS[s] for s in RI}      # an interval at its worst, every byte stuffed
QUALITIES = (1, 50, 90, 100)
SUBSAMPLINGS = (S444, S420)
PIL_SUBSAMPLING = {S444: 0, S420: 2}


class Stats(C.Structure):
    """jpeg_ref_stats_t of jpeg_ref.c"""
    _fields_ = [(k, C.c_int32) for k in ("stuffed", "stuffed_pad", "zrl", "no_eob", "dummy_right", "dummy_bottom", "max_dc_cat",
                                         "max_ac_cat", "intervals", "max_interval_bytes")]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}

    def __repr__(self):
        return f"Stats({self.as_dict()})"


def build_ref(tmpdir, flags=()):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("gcc not available")
    so = os.path.join(str(tmpdir), "libjpeg_ref.so")
    subprocess.check_call([gcc, "-std=c11", "-O2", "-Wall", "-fPIC", "-shared", *flags, HARNESS, "-o", so])
    L = C.CDLL(so)
    L.jpeg_ref_stats.restype = None
    L.jpeg_ref_stats.argtypes = [C.POINTER(Stats)]
    L.jpeg_ref_bound.restype = C.c_long
    L.jpeg_ref_bound.argtypes = [C.c_int, C.c_int, C.c_int]
    L.jpeg_ref_interval.argtypes = [C.c_int]
    L.jpeg_ref_slot.argtypes = [C.c_int]
    L.jpeg_ref_encode.restype = C.c_long
    L.jpeg_ref_encode.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_long]
    for s in SUBSAMPLINGS:
        assert L.jpeg_ref_interval(s) == RI[s] and L.jpeg_ref_slot(s) == SLOT[s]
    return L


def kernel_intervals():
    """the restart intervals jpeg.hip is compiled with by default, read from its source"""
    src = open(KERNEL).read()
    return {s: int(re.search(rf"#define OP_JPEG_RI_{n} (\d+)", src).group(1)) for s, n in ((S444, "444"), (S420, "420"))}


def ref_encode(L, rgb, quality, subsampling):
    """the harness's file for an (H, W, 3) uint8 array"""
    rgb = np.ascontiguousarray(rgb, np.uint8)
    h, w, _ = rgb.shape
    cap = L.jpeg_ref_bound(h, w, subsampling)
    out = np.empty(cap, np.uint8)
    n = L.jpeg_ref_encode(rgb.ctypes.data_as(C.c_void_p), h, w, quality, subsampling, out.ctypes.data_as(C.c_void_p), cap)
    assert n > 0, n
    return out[:n].tobytes()


def ref_stats(L):
    """what the last ref_encode on L went through"""
    s = Stats()
    L.jpeg_ref_stats(C.byref(s))
    return s


def pillow():
    """PIL.Image when it can write JPEG with restart markers, else None"""
    try:
        import PIL
        from PIL import Image, features
    except ImportError:
        return None
    if not features.check("jpg") or tuple(int(x) for x in PIL.__version__.split(".")[:2]) < (10, 2):   # restart_marker_blocks: 10.2
        return None
    return Image


def pillow_encode(Image, rgb, quality, subsampling, interval):
    """libjpeg's file: standard tables, `interval` MCUs per restart interval (0: no restart markers)"""
    b = io.BytesIO()
    Image.fromarray(rgb).save(b, "JPEG", quality=quality, subsampling=PIL_SUBSAMPLING[subsampling], optimize=False,
                              restart_marker_blocks=interval)
    return b.getvalue()


def walk(jpg):
    """-> dict(h, w, sampling, dri, intervals (list of entropy-coded byte strings), segments ([(marker, payload)]));
    asserts segment lengths, restart markers in order mod 8, no other FF xx inside the scan, EOI at the very end"""
    assert jpg[:2] == b"\xff\xd8"
    pos = 2; segs = []; info = {}
    while True:
        assert jpg[pos] == 0xFF, f"byte {pos}: no marker"
        m = jpg[pos + 1]
        n, = struct.unpack(">H", jpg[pos + 2: pos + 4])
        body = jpg[pos + 4: pos + 2 + n]
        assert len(body) == n - 2
        segs.append((m, body)); pos += 2 + n
        if m == 0xC0:
            p, h, w, nc = struct.unpack(">BHHB", body[:6])
            assert p == 8 and nc == 3 and len(body) == 6 + 3 * nc
            info.update(h=h, w=w, sampling=tuple(body[7 + 3 * c] for c in range(3)), tq=tuple(body[8 + 3 * c] for c in range(3)))
        elif m == 0xDD:
            info["dri"], = struct.unpack(">H", body)
        elif m == 0xDA:
            break
    assert [m for m, _ in segs] == [0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDD, 0xDA], [hex(m) for m, _ in segs]
    assert jpg[-2:] == b"\xff\xd9"
    scan = jpg[pos:-2]
    intervals = []; start = 0; i = 0; k = 0
    while i < len(scan):
        if scan[i] != 0xFF:
            i += 1; continue
        assert i + 1 < len(scan), "FF at the scan's end"
        nxt = scan[i + 1]
        if nxt == 0x00:
            i += 2; continue
        assert nxt == 0xD0 + (k & 7), f"scan byte {i}: FF {nxt:02X} where RST{k & 7} or a stuffed byte belongs"
        intervals.append(scan[start:i]); k += 1; i += 2; start = i
    intervals.append(scan[start:])
    mcu = 16 if info["sampling"][0] == 0x22 else 8
    nmcu = -(-info["h"] // mcu) * -(-info["w"] // mcu)
    assert len(intervals) == -(-nmcu // info["dri"]), (len(intervals), nmcu, info["dri"])
    assert all(len(iv) > 0 for iv in intervals)
    info.update(intervals=intervals, segments=segs)
    return info


def _rand(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def _smooth(h, w, seed):
    return png_cases._smooth(h, w, seed)


def _checker01(h, w):
    """saturated one-pixel checker: the largest AC coefficients"""
    y, x = np.mgrid[0:h, 0:w]
    return np.repeat((((y + x) & 1) * 255).astype(np.uint8)[..., None], 3, axis=2)


def _block_steps(h, w):
    """8 x 8 blocks alternately black and white: the largest DC differences (category 11 at quality 100, 4:4:4)"""
    y, x = np.mgrid[0:h, 0:w]
    return np.repeat(((((y >> 3) + (x >> 3)) & 1) * 255).astype(np.uint8)[..., None], 3, axis=2)


@functools.lru_cache(maxsize=None)
def _blended():
    return png_cases.blended_canvas()


# name -> builder.  With the MCU at 8 x 8 (4:4:4) or 16 x 16 (4:2:0) and RI = 32 / 8: 8x256 and 16x128 are exactly one
# interval, 8x264 and 16x144 one MCU more, 136x136 is 289 / 81 MCUs = 10 / 11 intervals (the marker index wraps past RST7).
CASES = {
    "1x1": lambda: _rand((1, 1, 3), 1),
    "8x8": lambda: _smooth(8, 8, 2),
    "9x17": lambda: _smooth(9, 17, 3),
    "16x16": lambda: _smooth(16, 16, 4),
    "17x33": lambda: _smooth(17, 33, 5),
    "37x53": lambda: _smooth(37, 53, 6),
    # 5 x 7 blocks of Y: right and bottom dummy blocks at 4:2:0; 20 chroma rows: 4 rows of the last chroma block are repeats
    # of a DOWNSAMPLED row (padding the full-resolution rows to 48 first would average other rows)
    "chroma_bottom_40x56": lambda: _rand((40, 56, 3), 7),
    "64x9": lambda: _smooth(64, 9, 8),
    "8x130": lambda: _smooth(8, 130, 9),
    "24x8": lambda: _smooth(24, 8, 10),
    "one_interval_444_8x256": lambda: _smooth(8, 256, 11),
    "one_interval_plus_one_444_8x264": lambda: _smooth(8, 264, 12),
    "one_interval_420_16x128": lambda: _smooth(16, 128, 13),
    "one_interval_plus_one_420_16x144": lambda: _smooth(16, 144, 14),
    "marker_wrap_136x136": lambda: _smooth(136, 136, 15),
    "random_31x47": lambda: _rand((31, 47, 3), 16),
    "checker01_32x32": lambda: _checker01(32, 32),
    "block_steps_16x64": lambda: _block_steps(16, 64),
    "all255_16x64": lambda: np.full((16, 64, 3), 255, np.uint8),
    "natural_400x600": png_cases.natural_crop,
    "blended": _blended,
}
NEEDS_PIL = {"natural_400x600"}
# config 4's canvas: once on the CPU and once on the GPU, at the default settings
BIG = ("all255_763x7999", lambda: np.full((763, 7999, 3), 255, np.uint8), 90, S420)
COMBOS = [(name, q, s) for name in CASES for q in QUALITIES for s in SUBSAMPLINGS]


def combo_id(name, q, s):
    return f"{name}-q{q}-{'444' if s == S444 else '420'}"


def case(name):
    if name in NEEDS_PIL and not png_cases.natural.available():
        pytest.skip("PIL not available")
    return np.ascontiguousarray(CASES[name](), np.uint8)
