"""CPU: the rules of the device JPEG decoder (openpano_amd/csrc/jpeg_dec.hip), checked without a device.

1. the serial restatement tests/harness/jpeg_dec_ref.c equals Pillow / libjpeg byte for byte on every fixture (where Pillow
   imports), the fixtures regenerate to the committed bytes, and everywhere the restatement matches digests.json;
2. the restatement's stats show that each hazard is reached on the file built for it;
3. op_jpeg_probe, through the library's host parser: every fixture accepted with its size and sampling, the refusals;
4. the host model of passes A / B / C over jpeg_dec_core.hpp, at subsequences of 32, 64, 256 and 1024 bits: the sequential
   decoder's state at every subsequence boundary, the round bound, the pixels;
5. the sanitizer program: a stand-alone binary built with -fsanitize=address,undefined from the same sources, 2000 seeded
   mutations of three fixtures and the GPU test's three corrupt streams."""
import ctypes as C
import importlib.util
import io
import os
import subprocess

import numpy as np
import pytest

import jpeg_dec_cases as D

LIB = os.path.join(D.ROOT, "openpano_amd", "libopenpano_hip.so")


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return D.build_ref(tmp_path_factory.mktemp("jpegdecref"))


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    return D.load_model(D.build_model(tmp_path_factory.mktemp("jpegdecmodel")))


@pytest.fixture(scope="module")
def decoded(ref):
    """the restatement's pixels of every fixture, computed once"""
    return {n: D.ref_decode(ref, D.data(n)) for n in D.NAMES}


def _pillow():
    try:
        from PIL import Image, features
    except ImportError:
        return None
    return Image if features.check("jpg") else None


def test_fixture_directory():
    files = sorted(f for f in os.listdir(D.GOLDEN) if f.endswith(".jpg"))
    assert files == sorted(n + ".jpg" for n in D.DIGESTS)
    total = sum(os.path.getsize(os.path.join(D.GOLDEN, f)) for f in os.listdir(D.GOLDEN))
    assert total < 400 * 1024, total
    for n, d in D.DIGESTS.items():
        assert d["bytes"] == len(D.data(n))


def test_restatement_matches_digests(decoded):
    for n in D.NAMES:
        assert decoded[n].shape == (D.DIGESTS[n]["h"], D.DIGESTS[n]["w"], 3), n
        assert D.digest(decoded[n]) == D.DIGESTS[n]["sha256"], n


def test_restatement_equals_pillow(decoded):
    Image = _pillow()
    if Image is None:
        pytest.skip("Pillow with libjpeg not available")
    for n in D.NAMES:
        want = np.asarray(Image.open(io.BytesIO(D.data(n))).convert("RGB"))
        diff = np.argwhere(decoded[n] != want)
        assert len(diff) == 0, (n, len(diff), diff[:3].tolist())


def test_fixtures_regenerate():
    if _pillow() is None:
        pytest.skip("Pillow with libjpeg not available")
    spec = importlib.util.spec_from_file_location("make_jpeg_dec_fixtures", os.path.join(D.GOLDEN, "make_jpeg_dec_fixtures.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    try:
        fx = mod.fixtures()
    except ImportError:
        pytest.skip("the natural image needs Pillow")
    assert sorted(fx) == sorted(D.DIGESTS)
    assert not [n for n, b in fx.items() if b != D.data(n)]


def test_hazards_are_reached(ref):
    def stats(name):
        D.ref_decode(ref, D.data(name))
        return D.ref_stats(ref).as_dict()
    for s in ("444", "422", "420"):
        st = stats(f"opt_random_37x53_{s}")
        # optimised tables of a dense stream: FF bytes, blocks that end on coefficient 63, codes longer than a byte
        assert st["stuffed"] > 0 and st["end63"] > 0 and st["max_code_len"] > 8, (s, st)
        assert _table_sizes(D.data(f"opt_flat_17x17_{s}"))[0x10] == 1 and _table_sizes(D.data(f"opt_flat_17x17_{s}"))[0x11] == 1, s   # AC tables of one code
        assert _table_sizes(D.data(f"opt_flat_17x17_{s}"))[0x00] == 2, s
        st = stats(f"checker01_32x32_{s}")
        assert st["max_ac_cat"] == 10 and st["max_code_len"] == 16, (s, st)                       # Annex K's longest codes
        assert stats(f"rst1_37x53_{s}")["intervals"] == {"444": 35, "422": 20, "420": 12}[s]
        assert stats(f"rst3_37x53_{s}")["intervals"] == {"444": 12, "422": 7, "420": 4}[s]        # 35 and 20 MCUs: a partial last interval
        assert stats(f"rstrow_37x53_{s}")["intervals"] == {"444": 5, "422": 5, "420": 3}[s]
        assert stats(f"size_37x53_{s}")["intervals"] == 1
    assert stats("block_steps_16x64_444")["max_dc_cat"] == 11
    assert stats("natural_400x600_q90_420")["zrl"] > 0 and stats("natural_400x600_q50_422")["zrl"] > 0
    jpg = D.data("exif_com_37x53_420")
    segs = D.segments(jpg)
    app1 = [(o, n) for o, m, n in segs if m == 0xE1]
    assert app1 and b"\xff\xd8" in jpg[app1[0][0]: app1[0][0] + app1[0][1]] and b"\xff\xda" in jpg[app1[0][0]: app1[0][0] + app1[0][1]]
    assert any(m == 0xFE for _, m, _ in segs)


def _table_sizes(jpg):
    """{Tc << 4 | Th: number of codes} of a file's DHT segments"""
    out = {}
    for o, m, n in D.segments(jpg):
        if m == 0xC4:
            p = jpg[o + 4: o + 4 + n]; i = 0
            while i < len(p):
                c = sum(p[i + 1: i + 17]); out[p[i]] = c; i += 17 + c
    return out


# ---- op_jpeg_probe: the library's host parser, no device needed
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        pytest.skip("libopenpano_hip.so not built")
    L = C.CDLL(LIB)
    L.op_last_error.restype = C.c_char_p
    L.op_jpeg_probe.argtypes = [C.c_char_p, C.c_int64, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    return L


def _probe(L, jpg):
    h, w, s = C.c_int(-7), C.c_int(-7), C.c_int(-7)
    r = L.op_jpeg_probe(jpg, len(jpg), C.byref(h), C.byref(w), C.byref(s))
    return r, h.value, w.value, s.value


def test_abi_is_additive(lib):
    assert lib.op_abi_version() == 12
    for name in ("op_jpeg_probe", "op_views_decode_jpeg", "op_views_copy", "op_debug_set_jpeg_subseq_bits"):
        assert hasattr(lib, name), name
    out = C.c_void_p()
    assert lib.op_views_decode_jpeg(None, None, None, 1, C.byref(out)) == D.OP_ERR_INVALID and not out
    assert b"op_views_decode_jpeg" in lib.op_last_error()
    assert lib.op_views_copy(None, None, 0, None) == D.OP_ERR_INVALID
    assert lib.op_debug_set_jpeg_subseq_bits(None, 64) == D.OP_ERR_INVALID


def test_probe_accepts_every_fixture(lib):
    for n in D.NAMES:
        assert _probe(lib, D.data(n)) == (D.OP_OK, D.DIGESTS[n]["h"], D.DIGESTS[n]["w"], D.sampling_of(n)), n
    good = D.data("size_37x53_420")
    assert _probe(lib, good + b"trailing bytes \xff\xd9 \xff\xda after EOI")[0] == D.OP_OK
    assert lib.op_jpeg_probe(good, len(good), None, None, None) == D.OP_OK


def test_probe_refusals(lib):
    r = _probe(lib, D.data("progressive_37x53"))
    assert r[0] == D.OP_ERR_UNSUPPORTED and b"progressive" in lib.op_last_error()
    for base in ("size_37x53_420", "rst3_37x53_444"):
        good = D.data(base)
        for what, code in D.PATCHES.items():
            assert _probe(lib, D.patched(good, what))[0] == code, (base, what, lib.op_last_error())
    one_by_eight = bytearray(D.data("size_8x8_444"))
    sof = D.find(bytes(one_by_eight), 0xC0)
    one_by_eight[sof + 5: sof + 7] = b"\x00\x01"
    assert _probe(lib, bytes(one_by_eight))[0] == D.OP_ERR_INVALID and b"below 2" in lib.op_last_error()
    assert _probe(lib, b"")[0] == D.OP_ERR_INVALID and _probe(lib, b"\x89PNG\r\n\x1a\n")[0] == D.OP_ERR_INVALID
    # a stray marker in the data is not the parser's business: the device flags it
    assert _probe(lib, D.corrupt("stray_dht")[0])[0] == D.OP_OK
    assert lib.op_jpeg_probe(None, 0, None, None, None) == D.OP_ERR_INVALID


# ---- the synchronisation, on the host
SUBSEQ_BITS = (32, 64, 256, 1024)


def _model(M, jpg, S, shape=None):
    n = M.jpeg_dec_model(jpg, len(jpg), S, None, 0, None, C.byref(C.c_int()), C.byref(C.c_int()), C.byref(C.c_uint()))
    st = np.zeros((max(n, 0), 4), np.uint32)
    rgb = np.zeros(shape, np.uint8) if shape else None
    r, ml, e = C.c_int(), C.c_int(), C.c_uint()
    n = M.jpeg_dec_model(jpg, len(jpg), S, st.ctypes.data_as(C.c_void_p), len(st), rgb.ctypes.data_as(C.c_void_p) if shape else None,
                         C.byref(r), C.byref(ml), C.byref(e))
    return n, st, rgb, r.value, ml.value, e.value


def test_model_reaches_the_sequential_state(ref, model, decoded, record_property):
    largest = {S: (0, None) for S in SUBSEQ_BITS}
    for name in D.NAMES:
        jpg = D.data(name)
        for S in SUBSEQ_BITS:
            want = D.ref_trace(ref, jpg, S)
            n, st, rgb, rounds, maxl, err = _model(model, jpg, S, decoded[name].shape)
            assert err == 0 and n == len(want), (name, S, n, len(want), err)
            assert np.array_equal(rgb, decoded[name]), (name, S)
            assert np.array_equal(st[:, 3], want[:, 3]), (name, S, "blocks completed per subsequence")
            # every boundary inside an interval: position, block in the MCU, zigzag position.  (An interval's last
            # subsequence ends in the bits that pad it to a byte, where the restatement stops at the last block.)
            inner = (want[:, 2] & 0x100) == 0
            want[:, 2] &= 0xFF
            assert (~inner).sum() == D.ref_stats(ref).intervals
            assert np.array_equal(st[inner, :3], want[inner, :3]), (name, S)
            # after round r the subsequences 0..r are right: an interval of L subsequences takes at most L - 1 rounds
            assert rounds <= max(maxl - 1, 0), (name, S, rounds, maxl)
            if rounds > largest[S][0]:
                largest[S] = (rounds, name)
    record_property("largest_round_counts", str(largest))
    print("largest round counts:", largest)


def test_model_flags_the_corrupt_streams(model):
    want = {"all_ones": 4 | 32 | 64, "one_mcu_short": 64, "stray_dht": 1}      # JD_ERR_* bits that may appear
    for what in D.CORRUPT:
        bad, good = D.corrupt(what)
        for S in SUBSEQ_BITS:
            n, _, _, _, _, err = _model(model, bad, S)
            assert n == -100 and err and not (err & ~want[what]) , (what, S, n, err)
            assert _model(model, good, S)[0] > 0


def test_sanitizer_program(tmp_path):
    """host code only, as a program of its own: nothing is loaded into Python and nothing is preloaded"""
    exe = D.build_model(tmp_path, sanitize=True)
    paths = [os.path.join(D.GOLDEN, n + ".jpg") for n in ("size_40x56_420", "rst3_37x53_444", "exif_com_37x53_422")]
    paths.append(os.path.join(D.GOLDEN, "opt_random_37x53_444.jpg"))      # decoded once, not mutated: it never resynchronises (the round bound)
    for what in D.CORRUPT:
        p = tmp_path / (what + ".jpg")
        p.write_bytes(D.corrupt(what)[0])
        paths.append(str(p))
    r = subprocess.run([exe] + paths, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    lines = r.stdout.strip().splitlines()
    assert [l.rsplit(": ", 1)[1] for l in lines[:7]] == ["decoded"] * 4 + ["refused"] * 3, lines[:7]
    assert lines[-1].startswith("decoded ")
