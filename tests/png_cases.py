"""Inputs, serial reference and independent decoder shared by test_png_ref_cpu.py, test_gpu_png.py and test_gpu_png_variant.py.

The decoder uses ``struct``, ``binascii.crc32`` and ``zlib.decompressobj`` only; the reference encoder is
tests/harness/png_ref.c compiled with gcc (the serial restatement of openpano_amd/csrc/png.hip).  Its png_ref_stats says which branches the last
encode went through; REACHES holds, per crafted input, what that input is there to reach, and the CPU test asserts it."""
import binascii
import ctypes as C
import functools
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
MAXBITS = (15, 15, 7)                   # shipped code-length limits: literal / length, distance, code-length alphabet
VARIANT_MAXBITS = (11, 11, 5)           # the variant build: the Kraft fix-up of huff_build runs on ordinary inputs
VARIANT_FLAGS = ["-DOP_PNG_LIT_MAXBITS=11", "-DOP_PNG_DIST_MAXBITS=11", "-DOP_PNG_CL_MAXBITS=5"]
LIT, DIST, CL = 0, 1, 2


class Stats(C.Structure):
    """png_ref_stats_t of png_ref.c"""
    _fields_ = [("limited", C.c_int32 * 3), ("limited_dynamic", C.c_int32 * 3), ("depth", C.c_int32 * 3), ("maxlen", C.c_int32 * 3),
                ("stored", C.c_int32), ("dynamic", C.c_int32), ("len_codes", C.c_uint32), ("dist_codes", C.c_uint32),
                ("cl_syms", C.c_uint32), ("limited_not_last", C.c_int32), ("maxbits", C.c_int32 * 3)]

    def __repr__(self):
        return ("Stats(" + ", ".join(f"{k}={list(getattr(self, k))}" for k in ("limited", "limited_dynamic", "depth", "maxlen", "maxbits"))
                + f", stored={self.stored}, dynamic={self.dynamic}, len_codes={self.len_codes:#x}, dist_codes={self.dist_codes:#x}, "
                f"cl_syms={self.cl_syms:#x}, limited_not_last={self.limited_not_last})")


def build_ref(tmpdir, flags=()):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("gcc not available")
    so = os.path.join(str(tmpdir), "libpng_ref.so")
    subprocess.check_call([gcc, "-std=c11", "-O2", "-Wall", "-fPIC", "-shared", *flags, HARNESS, "-o", so])
    L = C.CDLL(so)
    L.png_ref_stats.restype = None
    L.png_ref_stats.argtypes = [C.POINTER(Stats)]
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


def ref_stats(L):
    """what the last ref_encode on L went through"""
    s = Stats()
    L.png_ref_stats(C.byref(s))
    return s


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
    """canvas_byte (csrc/internal.hpp): Color::NO (negative) -> 255, v * 255 in fp32, truncated"""
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


# ---- inputs that reach the Kraft fix-up of huff_build at the shipped limits.  A Huffman tree is deeper than
# k only if its counts grow like Fibonacci numbers over more than k + 1 symbols; natural images never do that within one
# 61440-byte segment, so these are built for it.  All of them are rows of bytes that the None filter leaves as they are.
def _fib(k):
    a = [1, 1]
    while len(a) < k:
        a.append(a[-1] + a[-2])
    return a[:k]


def _lit_skew_row(rng, nbytes):
    """32 equiprobable values and a 15-symbol Fibonacci chain (counts 1, 1, 2, ..., 610), shuffled: the literal tree is 16 deep.
    (A pure Fibonacci stream does not get there: the greedy parse turns its frequent symbols into matches.)"""
    chain = np.repeat(np.arange(15, dtype=np.uint8), _fib(15))
    bulk = (rng.integers(0, 32, nbytes - len(chain)) + 64).astype(np.uint8)
    return rng.permutation(np.concatenate([chain, bulk]))


def _lit_limit(h, w, seed):
    rng = np.random.default_rng(seed)
    return np.stack([_lit_skew_row(rng, 3 * w) for _ in range(h)]).reshape(h, w, 3)


# code length -> number of literal values that get it (Fibonacci again, on the 19-symbol alphabet): value v occurs
# 2^(13 - length) times, so the literal tree has these lengths up to what the few matches of the parse disturb
_CL_PROFILE = {2: 1, 13: 1, 4: 2, 5: 3, 11: 5, 7: 8, 9: 13, 6: 21, 12: 34, 10: 55}


def _cl_limit(seed):
    rng = np.random.default_rng(seed)
    lens = rng.permutation(np.repeat(list(_CL_PROFILE), list(_CL_PROFILE.values())))
    stream = np.repeat(np.arange(len(lens), dtype=np.uint8), 1 << (13 - lens))
    stream = np.concatenate([stream, np.zeros(-len(stream) % 3, np.uint8)])
    return rng.permutation(stream).reshape(1, -1, 3)


def _hash3(F, p):
    """png.hip / png_ref.c hash3"""
    return (((int(F[p]) | int(F[p + 1]) << 8 | int(F[p + 2]) << 16) * 2654435761) & 0xFFFFFFFF) >> 19


# matches planted per distance code, rarest first: each count is above the sum of all counts two or more places before it
# (Fibonacci plus 6 % of slack, so that a handful of lost or accidental matches do not flatten the tree): 17 codes, 16 deep
_DIST_COUNTS = [1, 1, 4, 5, 9, 14, 24, 39, 64, 105, 173, 285, 468, 770, 1266, 2082, 3424]
_DIST_CODES = [0, 2] + list(range(29, 14, -1))      # distance 1, distance 3, then the hash candidate from 32768 down to 257


@functools.lru_cache(maxsize=None)
def _dist_limit(seed, w=20479):
    """One row of 4-byte tokens on a grid that the 240-byte sub-blocks respect (3 literals follow the filter byte).  A token is
    fresh noise or a copy of the 4 bytes at a chosen distance.  The parse is followed as the row grows (the hash heads as png.hip
    keeps them: the latest position per hash among the EARLIER groups of 256), so that a copy's source is the candidate the
    encoder will look at, the match stops after 4 bytes, and noise that would match something by accident is drawn again."""
    rng = np.random.default_rng(seed)
    N = 1 + 3 * w

    def fresh(n):
        return (rng.integers(-110, 111, n) & 255).astype(np.uint8)      # small as signed bytes: the None filter wins

    F = np.zeros(N + 8, np.uint8)
    F[1:] = fresh(N + 7)
    need = dict(zip(_DIST_CODES, _DIST_COUNTS))
    placed = dict.fromkeys(_DIST_CODES, 0)
    head = {}                           # hash -> latest position in the groups below `committed`
    latest = np.zeros(N, bool)          # position is some hash's head
    committed = 0

    def accident(p, before):
        """a match of 3 or more at p that nobody planted: distance 1, distance 3, or the hash candidate"""
        if F[p] == F[p - 1] == F[p + 1] == F[p + 2]:
            return True
        if p >= 3 and F[p] == F[p - 3] and F[p + 1] == F[p - 2] and F[p + 2] == F[p - 1]:
            return True
        s = (before if p < committed else head).get(_hash3(F, p))
        return s is not None and p - s <= 32768 and F[s] == F[p] and F[s + 1] == F[p + 1] and F[s + 2] == F[p + 2]

    ntok = (N - 4) // 4
    for t in range(ntok):
        i = 4 + 4 * t
        before = dict(head) if i % 256 == 0 else None       # what positions i - 2, i - 1 of the group before see
        while committed + 256 <= i:
            for p in range(committed, committed + 256):
                h = _hash3(F, p)
                if h in head:
                    latest[head[h]] = False
                head[h] = p
                latest[p] = True
            committed += 256
        remaining = sum(need[c] - placed[c] for c in _DIST_CODES)
        want = remaining > 0 and i >= 8 and rng.random() < 1.5 * remaining / max(1, ntok - t - 8)
        for attempt in range(50):
            code = None
            if want and attempt < 20:
                order = sorted((c for c in _DIST_CODES if placed[c] < need[c]), key=lambda c: -(need[c] - placed[c]) / need[c])
                c = order[min(attempt // 3, len(order) - 1)]
                if c == 0:                                   # x | x x x x
                    if F[i - 1] == F[i - 2]:
                        continue
                    F[i: i + 4] = F[i - 1]; after = F[i - 1]
                elif c == 2:                                 # a b c | a b c a
                    if F[i - 3] == F[i - 2] == F[i - 1] or F[i - 4] == F[i - 1]:
                        continue
                    F[i: i + 4] = [F[i - 3], F[i - 2], F[i - 1], F[i - 3]]; after = F[i - 2]
                else:
                    e = c // 2 - 1
                    lo = ((2 + (c & 1)) << e) + 1; hi = lo + (1 << e) - 1      # the distances of code c (RFC 1951, 3.2.5)
                    a = max(1, i - hi); b = min(i - lo, committed - 1)
                    live = np.nonzero(latest[a: b + 1])[0] if b >= a else []
                    if len(live) == 0:
                        continue
                    s = a + int(live[rng.integers(len(live))])
                    if F[s - 1] == F[i - 1]:
                        continue
                    F[i: i + 4] = F[s: s + 4]; after = F[s + 4]
                code = c
            else:
                F[i: i + 4] = fresh(4)
            bad = i >= 6 and (accident(i - 2, before) or accident(i - 1, before))
            if code is None:
                bad = bad or accident(i, before) or accident(i + 1, before)
            elif code >= 15:
                bad = bad or head.get(_hash3(F, i)) != s
            if bad:
                continue
            if code is not None:
                placed[code] += 1
                while F[i + 4] == after:                     # the match ends after 4 bytes
                    F[i + 4] = fresh(1)[0]
            break
        else:
            raise AssertionError(f"no token fits at byte {i}")
    assert placed == need, placed
    return F[1: N].reshape(1, w, 3).copy()


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
    # 60001 bytes, one segment (the last): the literal / length tree is 16 deep
    "lit_limit_1x20000": lambda: _lit_limit(1, 20000, 47),
    # rows of 61438 bytes, three segments: the same in a segment that is NOT the last (an empty stored block follows the limited table)
    "lit_limit_3x20479": lambda: _lit_limit(3, 20479, 48),
    "dist_limit_1x20479": lambda: _dist_limit(0),
    "cl_limit_1x2593": lambda: _cl_limit(0),
}
# what a crafted input is there to reach at the shipped limits: alphabet -> (dynamic segments whose table the limiter rewrote,
# depth of the unlimited tree), and whether one of those segments is not the last.  Asserted from png_ref_stats by
# test_png_ref_cpu.py; an input that stops meeting its line has lost its purpose.
REACHES = {
    "lit_limit_1x20000": dict(alphabet=LIT, segments=1, depth=16, not_last=False),
    "lit_limit_3x20479": dict(alphabet=LIT, segments=3, depth=16, not_last=True),
    "dist_limit_1x20479": dict(alphabet=DIST, segments=1, depth=16, not_last=False),
    "cl_limit_1x2593": dict(alphabet=CL, segments=1, depth=9, not_last=False),
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
