"""Fixtures, serial restatement and host model shared by test_jpeg_dec_cpu.py and test_gpu_jpeg_dec.py.

The restatement is tests/harness/jpeg_dec_ref.c compiled with gcc (the device decoder of openpano_amd/csrc/jpeg_dec.hip as plain
loops).  The fixtures are the Pillow-written files of tests/golden/jpeg_dec with the sha256 of their
expected RGB in digests.json; Pillow itself is needed only by the CPU test's comparison with libjpeg."""
import ctypes as C
import hashlib
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "jpeg_dec")
HARNESS = os.path.join(ROOT, "tests", "harness", "jpeg_dec_ref.c")
FUZZ = os.path.join(ROOT, "tests", "harness", "jpeg_dec_fuzz.cc")
CSRC = os.path.join(ROOT, "openpano_amd", "csrc")
OP_OK, OP_ERR_INVALID, OP_ERR_UNSUPPORTED = 0, -1, -4
S444, S420, S422, GREY = 0, 1, 2, 3
DIGESTS = json.load(open(os.path.join(GOLDEN, "digests.json")))
REFUSED = ("progressive_37x53",)                          # fixtures outside the format
NAMES = [n for n in sorted(DIGESTS) if n not in REFUSED]


def data(name):
    return open(os.path.join(GOLDEN, name + ".jpg"), "rb").read()


def sampling_of(name):
    return GREY if name.startswith("grey") else {"444": S444, "420": S420, "422": S422}[name.rsplit("_", 1)[1]]


class Stats(C.Structure):
    """jpeg_dec_ref_stats_t of jpeg_dec_ref.c"""
    _fields_ = [(k, C.c_int32) for k in ("stuffed", "zrl", "end63", "max_dc_cat", "max_ac_cat", "max_code_len", "intervals", "blocks",
                                         "max_zrl_chain", "unpadded", "unpadded_last", "pad_zero", "end_ff", "eob_after_dc", "full_blocks", "run15")] + \
               [("end63_zrl", C.c_int32 * 4), ("dc_bound", C.c_int32 * 12), ("ac_bound", C.c_int32 * 11)]

    def as_dict(self):
        return {k: getattr(self, k) if t is C.c_int32 else list(getattr(self, k)) for k, t in self._fields_}


def build_ref(tmpdir):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("gcc not available")
    so = os.path.join(str(tmpdir), "libjpeg_dec_ref.so")
    subprocess.check_call([gcc, "-std=c11", "-O2", "-Wall", "-fPIC", "-shared", HARNESS, "-o", so])
    L = C.CDLL(so)
    L.jpeg_dec_ref_stats.restype = None
    L.jpeg_dec_ref_stats.argtypes = [C.POINTER(Stats)]
    L.jpeg_dec_ref_probe.argtypes = [C.c_char_p, C.c_long, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.jpeg_dec_ref_decode.restype = C.c_long
    L.jpeg_dec_ref_decode.argtypes = [C.c_char_p, C.c_long, C.c_void_p, C.c_long, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.jpeg_dec_ref_trace.restype = C.c_long
    L.jpeg_dec_ref_trace.argtypes = [C.c_char_p, C.c_long, C.c_long, C.c_void_p, C.c_long]
    return L


def ref_decode(L, jpg):
    """the restatement's (H, W, 3) uint8 pixels of a file"""
    h, w, s = C.c_int(), C.c_int(), C.c_int()
    assert L.jpeg_dec_ref_probe(jpg, len(jpg), C.byref(h), C.byref(w), C.byref(s)) == 0
    out = np.empty((h.value, w.value, 3), np.uint8)
    r = L.jpeg_dec_ref_decode(jpg, len(jpg), out.ctypes.data_as(C.c_void_p), out.size, C.byref(h), C.byref(w))
    assert r == 0, r
    return out


def ref_stats(L):
    s = Stats()
    L.jpeg_dec_ref_stats(C.byref(s))
    return s


def ref_trace(L, jpg, S):
    """(nsub, 4) uint32: position, block in MCU, zigzag position (| 0x100: the last of its interval), blocks completed, at every subsequence's end"""
    n = L.jpeg_dec_ref_trace(jpg, len(jpg), S, None, 0)
    assert n > 0, n
    out = np.zeros((n, 4), np.uint32)
    assert L.jpeg_dec_ref_trace(jpg, len(jpg), S, out.ctypes.data_as(C.c_void_p), n) == n
    return out


def digest(rgb):
    return hashlib.sha256(np.ascontiguousarray(rgb, np.uint8).tobytes()).hexdigest()


def build_model(tmpdir, sanitize=False):
    """tests/harness/jpeg_dec_fuzz.cc: as a shared library (the host model of passes A, B, C over jpeg_dec_core.hpp), or with
    sanitize=True as the stand-alone sanitizer program; -> path"""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    if sanitize:
        exe = os.path.join(str(tmpdir), "jpeg_dec_fuzz")
        subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fwrapv", "-I", CSRC, FUZZ, "-o", exe])
        return exe
    so = os.path.join(str(tmpdir), "libjpeg_dec_model.so")
    subprocess.check_call([gxx, "-std=c++17", "-O2", "-Wall", "-fPIC", "-shared", "-DJPEG_DEC_MODEL_LIB", "-I", CSRC, FUZZ, "-o", so])
    return so


def load_model(so):
    L = C.CDLL(so)
    L.jpeg_dec_model.restype = C.c_long
    # file, size, S, states (nsub x 4 uint32 or NULL), cap, rgb (or NULL), rounds, max subsequences of an interval, error word
    L.jpeg_dec_model.argtypes = [C.c_char_p, C.c_long, C.c_int, C.c_void_p, C.c_long, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_uint)]
    return L


# ---- header patches of a good file, for the refusals
def segments(jpg):
    """[(offset of the FF, marker, payload length)] up to and including SOS"""
    pos = 2; out = []
    while True:
        assert jpg[pos] == 0xFF
        m = jpg[pos + 1]
        n = int.from_bytes(jpg[pos + 2: pos + 4], "big")
        out.append((pos, m, n - 2))
        pos += 2 + n
        if m == 0xDA:
            return out


def find(jpg, marker):
    return next(o for o, m, _ in segments(jpg) if m == marker)


def patched(jpg, what):
    b = bytearray(jpg)
    sof = find(jpg, 0xC0)
    if what == "precision12":
        b[sof + 4] = 12
    elif what == "sof9":
        b[sof + 1] = 0xC9
    elif what == "four_components":
        b[sof + 9] = 4
    elif what == "sampling41":
        b[sof + 11] = 0x41
    elif what == "dqt16":
        b[find(jpg, 0xDB) + 4] |= 0x10
    elif what == "second_sos":
        sos = find(jpg, 0xDA)
        n = int.from_bytes(jpg[sos + 2: sos + 4], "big")
        eoi = jpg.rindex(b"\xff\xd9")
        b = bytearray(jpg[:eoi] + jpg[sos: sos + 2 + n] + b"\x00\x00" + jpg[eoi:])
    elif what == "cut_in_header":
        b = b[: find(jpg, 0xC4) + 30]
    elif what == "no_eoi":
        b = b[: jpg.rindex(b"\xff\xd9")]
    else:
        raise KeyError(what)
    return bytes(b)


PATCHES = {"precision12": OP_ERR_UNSUPPORTED, "sof9": OP_ERR_UNSUPPORTED, "four_components": OP_ERR_UNSUPPORTED, "sampling41": OP_ERR_UNSUPPORTED,
           "dqt16": OP_ERR_UNSUPPORTED, "second_sos": OP_ERR_UNSUPPORTED, "cut_in_header": OP_ERR_INVALID, "no_eoi": OP_ERR_INVALID}


# ---- corrupt entropy-coded data that the device must answer with OP_ERR_INVALID (the sanitizer program passes the same three)
def scan_range(jpg):
    o, _, n = segments(jpg)[-1]
    return o + 4 + n, jpg.rindex(b"\xff\xd9")


def corrupt(what):
    """-> (a corrupt file, the good file it was made from)"""
    if what == "all_ones":            # FF 00 FF 00 FF 00 on the true path: 24 one-bits, which no table codes
        jpg = data("size_37x53_420")
        b0, _ = scan_range(jpg)
        return jpg[:b0 + 3] + b"\xff\x00\xff\x00\xff\x00" + jpg[b0 + 9:], jpg
    if what == "one_mcu_short":       # the frame says 8 x 9, two MCUs at 4:4:4; the scan holds one
        jpg = data("size_8x8_444")
        b = bytearray(jpg)
        sof = find(jpg, 0xC0)
        assert b[sof + 7: sof + 9] == b"\x00\x08"
        b[sof + 8] = 9
        return bytes(b), jpg
    if what == "stray_dht":           # FF C4 in the data
        jpg = data("size_37x53_422")
        b0, _ = scan_range(jpg)
        return jpg[:b0 + 5] + b"\xff\xc4" + jpg[b0 + 7:], jpg
    raise KeyError(what)


CORRUPT = ("all_ones", "one_mcu_short", "stray_dht")
