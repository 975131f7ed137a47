"""CPU: the device JPEG decoder's rules on streams that libjpeg's writer never produces, without a device.

The files of tests/golden/jpeg_craft come from the coefficient-level writer tests/jpeg_craft.py: tables per component, odd
Huffman shapes, every EXTEND boundary, FF bytes and restart markers placed on the byte, DRI edge values, unusual segment layouts.

1. the writer regenerates the committed bytes; the restatement tests/harness/jpeg_dec_ref.c equals Pillow / libjpeg byte for
   byte on every file (where Pillow imports) and digests.json everywhere;
2. hazard assertions: the restatement's stats, the headers and the scan bytes show that each file is the case it is named for;
3. the host model of passes A / B / C at S = 32, 64, 256, 1024 (65536 too for the two-bit file) reaches the sequential state
   and the pixels on every file;
4. every corrupt file sets its bit of the error word in the model, at every S;
5. op_jpeg_probe accepts the corpus and refuses what the parser must refuse, with the reason named;
6. the sanitizer program (a stand-alone binary, nothing loaded into Python) runs over the corrupt files and some good ones."""
import ctypes as C
import io
import os
import subprocess

import numpy as np
import pytest

import jpeg_craft as K
import jpeg_craft_cases as X
import jpeg_dec_cases as D

LIB = os.path.join(D.ROOT, "openpano_amd", "libopenpano_hip.so")
COLOUR = ("444", "422", "420")
SUBSEQ_BITS = (32, 64, 256, 1024)


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return D.build_ref(tmp_path_factory.mktemp("jpegcraftref"))


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    return D.load_model(D.build_model(tmp_path_factory.mktemp("jpegcraftmodel")))


@pytest.fixture(scope="module")
def decoded(ref):
    """the restatement's pixels and stats of every file, computed once"""
    out = {}
    for n in X.NAMES:
        rgb = D.ref_decode(ref, X.data(n))
        rgb.setflags(write=False)
        out[n] = (rgb, D.ref_stats(ref).as_dict())
    return out


def _pillow():
    try:
        from PIL import Image, features
    except ImportError:
        return None
    return Image if features.check("jpg") else None


def test_fixture_directory():
    files = sorted(f for f in os.listdir(X.GOLDEN) if f.endswith(".jpg"))
    assert files == sorted(n + ".jpg" for n in X.DIGESTS)
    assert sum(os.path.getsize(os.path.join(X.GOLDEN, f)) for f in os.listdir(X.GOLDEN)) < 150 * 1024
    for n, d in X.DIGESTS.items():
        assert d["bytes"] == len(X.data(n))
        assert d["bytes"] < 2048 or n == X.TWOBIT or n in X.STRADDLE_TILE, n


def test_writer_regenerates_the_committed_bytes():
    fx = X.generator().fixtures()
    assert sorted(fx) == X.NAMES
    assert not [n for n, b in fx.items() if b != X.data(n)]


def test_restatement_matches_digests(decoded):
    for n in X.NAMES:
        assert decoded[n][0].shape == (X.DIGESTS[n]["h"], X.DIGESTS[n]["w"], 3), n
        assert D.digest(decoded[n][0]) == X.DIGESTS[n]["sha256"], n


def test_restatement_equals_pillow(decoded):
    Image = _pillow()
    if Image is None:
        pytest.skip("Pillow with libjpeg not available")
    for n in X.NAMES:
        want = np.asarray(Image.open(io.BytesIO(X.data(n))).convert("RGB"))
        diff = np.argwhere(decoded[n][0] != want)
        assert len(diff) == 0, (n, len(diff), diff[:3].tolist())


# ---- hazards: no case may silently stop being one
def _header(jpg):
    """what the segments before the scan say: marker order, SOF components, SOS selectors, DHT tables, DQT ids, DRI values"""
    h = {"order": [], "dht": [], "dqt": [], "dri": [], "fill": 0}
    pos = 2
    while True:
        while jpg[pos + 1] == 0xFF:
            pos += 1; h["fill"] += 1
        m = jpg[pos + 1]; n = int.from_bytes(jpg[pos + 2: pos + 4], "big"); p = jpg[pos + 4: pos + 2 + n]
        h["order"].append(m)
        if m == 0xC0:
            h["sof"] = [(p[6 + 3 * c], p[7 + 3 * c], p[8 + 3 * c]) for c in range(p[5])]
        elif m == 0xC4:
            i = 0; seg = []
            while i < len(p):
                cnt = list(p[i + 1: i + 17]); k = sum(cnt)
                seg.append((p[i] >> 4, p[i] & 15, cnt, list(p[i + 17: i + 17 + k]))); i += 17 + k
            h["dht"].append(seg)
        elif m == 0xDB:
            h["dqt"].append([(p[i] & 15, list(p[i + 1: i + 65])) for i in range(0, len(p), 65)])
        elif m == 0xDD:
            h["dri"].append(int.from_bytes(p, "big"))
        elif m == 0xDA:
            h["sos"] = [(p[1 + 2 * c], p[2 + 2 * c] >> 4, p[2 + 2 * c] & 15) for c in range(p[0])]
            return h
        pos += 2 + n


def _scan(jpg):
    b0, e = D.scan_range(jpg)
    return jpg[b0:e]


def _tables(h):
    """{(Tc, Th): (counts, vals)}, a later definition over an earlier one"""
    return {(tc, th): (cnt, vals) for seg in h["dht"] for tc, th, cnt, vals in seg}


def _repatch(jpg, h, swap):
    """the file with the Cb and Cr table ids exchanged: swap = "tq" in SOF, "huff" in SOS"""
    b = bytearray(jpg)
    if swap == "tq":
        at = D.find(jpg, 0xC0) + 4 + 6
        b[at + 3 + 2], b[at + 6 + 2] = b[at + 6 + 2], b[at + 3 + 2]
    else:
        at = D.find(jpg, 0xDA) + 4 + 1
        b[at + 2 + 1], b[at + 4 + 1] = b[at + 4 + 1], b[at + 2 + 1]
    return bytes(b)


def test_hazards_per_component_tables_and_ids(ref, decoded):
    for s in COLOUR:
        jpg = X.data(f"tables3_{s}")
        h = _header(jpg)
        assert [c[2] for c in h["sof"]] == [0, 2, 1] and [c[1:] for c in h["sos"]] == [(0, 2), (3, 0), (1, 3)], s
        q = {i: t for seg in h["dqt"] for i, t in seg}
        assert q[2] == [1] * 64 and q[1] == [37] * 64 and len({tuple(q[i]) for i in q}) == 3
        t = _tables(h)
        assert len({(tuple(t[k][0]), tuple(t[k][1])) for k in ((0, 0), (0, 3), (0, 1))}) == 3 and len({(tuple(t[k][0]), tuple(t[k][1])) for k in ((1, 2), (1, 0), (1, 3))}) == 3
        # a decoder that took Cb's tables for Cr would show: each exchange changes the pixels, or no longer decodes
        for swap in ("tq", "huff"):
            other = _repatch(jpg, h, swap)
            assert other != jpg
            hh, ww = C.c_int(), C.c_int()
            out = np.zeros_like(decoded[f"tables3_{s}"][0])
            r = ref.jpeg_dec_ref_decode(other, len(other), out.ctypes.data_as(C.c_void_p), out.size, C.byref(hh), C.byref(ww))
            assert r == -1 or (r == 0 and (out != decoded[f"tables3_{s}"][0]).sum() > 500), (s, swap, r)
        h = _header(X.data(f"shared_tables_{s}"))
        assert [c[1:] for c in h["sos"]] == [(0, 0)] * 3 and sorted(_tables(h)) == [(0, 0), (1, 0)]
        for name, ids in ((f"ids_012_{s}", [0, 1, 2]), (f"ids_7_200_33_{s}", [7, 200, 33]), (f"ids_adobe_{s}", [1, 2, 3])):
            h = _header(X.data(name))
            assert [c[0] for c in h["sof"]] == ids and [c[0] for c in h["sos"]] == ids, name
            assert (0xEE in h["order"] and 0xE0 not in h["order"]) if "adobe" in name else h["order"][0] == 0xE0, name
        assert X.data(f"ids_adobe_{s}")[X.data(f"ids_adobe_{s}").index(b"Adobe") + 11] == 1
    for name, dri in (("grey_hi_ids", []), ("grey_hi_ids_rst1", [1])):
        h = _header(X.data(name))
        assert h["sof"] == [(0, 0x11, 3)] and h["sos"] == [(0, 2, 3)] and h["dri"] == dri, name
    assert decoded["grey_hi_ids_rst1"][1]["intervals"] == 15
    assert np.array_equal(decoded["grey_hi_ids"][0], decoded["grey_hi_ids_rst1"][0])


def test_hazards_huffman_shapes(decoded):
    for s in COLOUR:
        t = _tables(_header(X.data(f"huff_skew_{s}")))
        assert all(cnt == [1] * 16 for cnt, _ in t.values()), s
        used = _code_lengths_used(X.data(f"huff_skew_{s}"))
        assert any({15, 16} <= u for u in used.values()), (s, used)
        assert decoded[f"huff_skew_{s}"][1]["max_code_len"] == 16
        t = _tables(_header(X.data(f"huff_flat8_{s}")))
        for (tc, th), (cnt, vals) in t.items():
            assert cnt == [0] * 7 + [len(vals)] + [0] * 8 and len(vals) == (200 if tc else 12), (s, tc, th)
        used = _symbols_used(X.data(f"huff_flat8_{s}"))
        assert all(len(used[k]) < len(t[k][1]) // 2 for k in t if k[0]), s                   # most of the 200 are unused
        t = _tables(_header(X.data(f"huff_shuffled_{s}")))
        falls = 0
        for cnt, vals in t.values():
            k = 0
            for c in cnt:
                falls += sum(1 for a, b in zip(vals[k: k + c], vals[k + 1: k + c]) if a > b); k += c
        assert falls > 5, s
        h = _header(X.data(f"huff_redefined_{s}"))
        first = {(tc, th): vals for seg in h["dht"][:2] for tc, th, _, vals in seg}
        last = _tables(h)
        assert sorted(first) == sorted(last) and all(first[k] != last[k][1] for k in last), s
        for k in (0, 1):      # luma and chroma share neither here: four tables, each given twice
            assert (k, 0) in last and (k, 1) in last


def _walk(jpg):
    """the (Tc, Th, symbol, code length) of every symbol of a good file's scan, by a decoder of the writer's own tables"""
    h = _header(jpg)
    tables = _tables(h)
    dec = {k: {(code, ln): sym for sym, (code, ln) in K.codes_of(t).items()} for k, t in tables.items()}
    samp = h["sof"][0][1]
    ny = (samp >> 4) * (samp & 15) if len(h["sof"]) == 3 else 1
    comps = [0] * ny + ([1, 2] if len(h["sof"]) == 3 else [])
    out = []
    for part in _split_intervals(_scan(jpg)):
        bits = "".join(f"{b:08b}" for b in part.replace(b"\xff\x00", b"\xff"))
        pos = 0; k = 0
        while "0" in bits[pos:]:      # what is left is a block: the padding is 1-bits, and no code is all ones
            c = comps[k % len(comps)]
            zz = 0
            while zz < 64:
                key = (0, h["sos"][c][1]) if zz == 0 else (1, h["sos"][c][2])
                code = 0; ln = 0
                while (code, ln) not in dec[key]:
                    code = code << 1 | int(bits[pos]); pos += 1; ln += 1
                sym = dec[key][(code, ln)]
                out.append((key[0], key[1], sym, ln))
                pos += sym & 15
                zz = 1 if zz == 0 else 64 if sym == 0 else zz + 16 if sym == 0xF0 else zz + (sym >> 4) + 1
            k += 1
    return out


def _split_intervals(scan):
    out = []; i = 0; start = 0
    while i < len(scan) - 1:
        if scan[i] == 0xFF and (scan[i + 1] & 0xF8) == 0xD0:
            out.append(scan[start:i]); start = i + 2; i += 2
        elif scan[i] == 0xFF:
            i += 2
        else:
            i += 1
    return out + [scan[start:]]


def _code_lengths_used(jpg):
    used = {}
    for tc, th, _, ln in _walk(jpg):
        used.setdefault((tc, th), set()).add(ln)
    return used


def _symbols_used(jpg):
    used = {}
    for tc, th, sym, _ in _walk(jpg):
        used.setdefault((tc, th), set()).add(sym)
    return used


def test_hazards_extend_and_runs(decoded):
    for name in ("extend_all_grey", "extend_all_420"):
        st = decoded[name][1]
        assert st["dc_bound"][1:] == [15] * 11 and st["ac_bound"][1:] == [15] * 10, (name, st)      # all four boundary values of every category
        assert st["max_dc_cat"] == 11 and st["max_ac_cat"] == 10
        assert st["eob_after_dc"] > 40 and st["full_blocks"] >= 1 and st["max_zrl_chain"] == 3 and st["run15"] >= 3, (name, st)
        assert all(v >= 1 for v in st["end63_zrl"]), (name, st)       # coefficient 63 behind 0, 1, 2 and 3 ZRLs
        syms = _symbols_used(X.data(name))
        assert any(s >= 0xF1 for k, u in syms.items() if k[0] for s in u), name


def test_hazards_interval_endings(decoded):
    for s in COLOUR:
        st = decoded[f"pad0_{s}"][1]
        assert st["intervals"] > 1 and st["pad_zero"] >= 2, (s, st)
        st = decoded[f"pad_none_{s}"][1]      # an interval inside the scan and the scan itself end on a byte boundary
        assert st["unpadded"] >= 2 and st["unpadded_last"] == 1 and st["intervals"] > 2, (s, st)
        scan = _scan(X.data(f"ends_ff_{s}"))
        assert decoded[f"ends_ff_{s}"][1]["end_ff"] >= 2 and scan.endswith(b"\xff\x00"), s
        assert any(scan[i: i + 3] == b"\xff\x00\xff" and (scan[i + 3] & 0xF8) == 0xD0 for i in range(len(scan) - 3)), s
        assert X.data(f"ends_ff_{s}").endswith(b"\xff\x00\xff\xd9")
        assert _scan(X.data(f"starts_ff_{s}")).startswith(b"\xff\x00"), s
        assert decoded[f"starts_ff_{s}"][1]["intervals"] > 1


def test_hazards_straddles(decoded):
    tile, run = 8192, 8                                       # JD_WG * JD_RUN and JD_RUN of k_jd_scan
    a, b = (_scan(X.data(n)) for n in X.STRADDLE_TILE)
    assert len(a) > tile and a[tile - 1: tile + 1] == b"\xff\x00" and decoded[X.STRADDLE_TILE[0]][1]["intervals"] == 1
    assert len(b) > tile and b[tile - 1: tile + 1] == b"\xff\xd0" and b.index(b"\xff\xd0") == tile - 1
    assert decoded[X.STRADDLE_TILE[1]][1]["intervals"] == 2
    a, b = (_scan(X.data(n)) for n in X.STRADDLE_RUN)
    assert any(a[i: i + 2] == b"\xff\x00" for i in range(run - 1, len(a), run))
    assert any(b[i] == 0xFF and (b[i + 1] & 0xF8) == 0xD0 for i in range(run - 1, len(b) - 1, run))
    for n in X.STRADDLE_TILE + X.STRADDLE_RUN:
        assert X.DIGESTS[n]["h"] == X.DIGESTS[n]["w"] == (64 if n in X.STRADDLE_TILE else 16)


def test_hazards_dri_and_layouts(decoded):
    mcus = {"444": 15, "422": 9, "420": 6}
    for s in COLOUR:
        n = mcus[s]
        want = {"eq": ([n], 1), "plus1": ([n + 1], 1), "65535": ([65535], 1), "0": ([0], 1), "1_then_0": ([1, 0], 1), "0_then_3": ([0, 3], n // 3),
                "minus1": ([n - 1], 2)}
        for tag, (dri, intervals) in want.items():
            name = f"dri_{tag}_{s}"
            assert _header(X.data(name))["dri"] == dri and decoded[name][1]["intervals"] == intervals, name
            assert np.array_equal(decoded[name][0], decoded[f"dri_eq_{s}"][0]), name       # the same coefficients in every one
        order = lambda tag: [m for m in _header(X.data(f"layout_{tag}_{s}"))["order"] if m != 0xE0]
        assert order("tables_around_sof") == [0xC4] * 4 + [0xC0, 0xDB, 0xDB, 0xDA]
        assert order("split") == [0xDB, 0xDB, 0xC0] + [0xC4] * 4 + [0xDA]
        assert order("joined") == [0xDB, 0xC0, 0xC4, 0xDA]
        h = _header(X.data(f"layout_dqt_twice_{s}"))
        assert [i for seg in h["dqt"] for i, _ in seg] == [0, 1, 0, 1] and h["dqt"][0][0][1] != h["dqt"][1][0][1]
        assert order("dri_first")[:2] == [0xDD, 0xDB] and decoded[f"layout_dri_first_{s}"][1]["intervals"] == (n + 1) // 2
        jpg = X.data(f"layout_fill_{s}")
        assert _header(jpg)["fill"] == 6 and b"\xff\xff\xff\xff\xc0" in jpg and b"\xff\xff\xff\xff\xda" in jpg
        jpg = X.data(f"layout_empty_segments_{s}")
        assert b"\xff\xfe\x00\x02\xff" in jpg and b"\xff\xef\x00\x02\xff" in jpg
        for tag in ("tables_around_sof", "joined", "dqt_twice", "fill", "empty_segments"):
            assert np.array_equal(decoded[f"layout_{tag}_{s}"][0], decoded[f"layout_split_{s}"][0]), (tag, s)


def test_hazard_two_bit_blocks(ref, decoded):
    jpg = X.data(X.TWOBIT)
    st = decoded[X.TWOBIT][1]
    assert st["blocks"] == 128 * 256 == st["eob_after_dc"] and st["max_code_len"] == 2 and len(jpg) < 9 * 1024
    tr = D.ref_trace(ref, jpg, 65536)
    assert tr[:, 3].max() > 30000 and tr[:, 3].max() <= 65536 // 2 + 1, tr[:, 3]      # blocks completed by one subsequence: near the bound of JD_S_MAX
    rgb = decoded[X.TWOBIT][0]
    assert sorted(np.unique(rgb).tolist()) == [128, 130] and (rgb[..., 0] == 130).sum() > 2 ** 19      # the DC steps show


# ---- the synchronisation, on the host
def _model(M, jpg, S, shape=None):
    n = M.jpeg_dec_model(jpg, len(jpg), S, None, 0, None, C.byref(C.c_int()), C.byref(C.c_int()), C.byref(C.c_uint()))
    st = np.zeros((max(n, 0), 4), np.uint32)
    rgb = np.zeros(shape, np.uint8) if shape else None
    r, ml, e = C.c_int(), C.c_int(), C.c_uint()
    n = M.jpeg_dec_model(jpg, len(jpg), S, st.ctypes.data_as(C.c_void_p), len(st), rgb.ctypes.data_as(C.c_void_p) if shape else None,
                         C.byref(r), C.byref(ml), C.byref(e))
    return n, st, rgb, r.value, ml.value, e.value


def test_model_reaches_the_sequential_state(ref, model, decoded, record_property):
    largest = {}
    for name in X.NAMES:
        jpg = X.data(name)
        for S in SUBSEQ_BITS + ((65536,) if name == X.TWOBIT else ()):
            want = D.ref_trace(ref, jpg, S)
            n, st, rgb, rounds, maxl, err = _model(model, jpg, S, decoded[name][0].shape)
            assert err == 0 and n == len(want), (name, S, n, len(want), err)
            assert np.array_equal(rgb, decoded[name][0]), (name, S)
            assert np.array_equal(st[:, 3], want[:, 3]), (name, S, "blocks completed per subsequence")
            inner = (want[:, 2] & 0x100) == 0
            want[:, 2] &= 0xFF
            assert (~inner).sum() == decoded[name][1]["intervals"]
            assert np.array_equal(st[inner, :3], want[inner, :3]), (name, S)
            assert rounds <= max(maxl - 1, 0), (name, S, rounds, maxl)
            if rounds > largest.get(S, (0, None))[0]:
                largest[S] = (rounds, name)
    record_property("largest_round_counts", str(largest))
    print("largest round counts:", largest)


def test_model_flags_the_corrupt_streams(model):
    good = X.data("grey_hi_ids_rst1")
    for what, (bit, may) in X.CORRUPT.items():
        bad = X.corrupt(what)
        assert bad != good
        for S in SUBSEQ_BITS + (65536,):
            n, _, _, _, _, err = _model(model, bad, S)
            assert n == -100 and err & bit and not (err & ~(bit | may)), (what, S, n, err)
    for S in SUBSEQ_BITS:
        assert _model(model, good, S)[0] > 0


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


def test_probe_accepts_the_corpus(lib):
    for n in X.NAMES:
        assert _probe(lib, X.data(n)) == (D.OP_OK, X.DIGESTS[n]["h"], X.DIGESTS[n]["w"], X.sampling_of(n)), n
    for what in X.CORRUPT:      # corrupt data is not the parser's business
        assert _probe(lib, X.corrupt(what))[0] == D.OP_OK, what


def test_probe_refusals(lib):
    for what, (code, why) in X.REFUSED.items():
        assert _probe(lib, X.refused(what))[0] == code, (what, lib.op_last_error())
        assert why.encode() in lib.op_last_error(), (what, lib.op_last_error())


def test_complete_codes_are_where_libjpeg_and_this_decoder_part(lib):
    """A prefix code that uses the all-ones codeword: jd_huff_build takes it, libjpeg refuses the DHT.  Pinned, not changed; so
    no fixture may hold one, or Pillow could not be its yardstick."""
    for n in X.NAMES:
        for key, (cnt, _) in _tables(_header(X.data(n))).items():
            assert sum(c << (16 - ln) for ln, c in enumerate(cnt, 1)) < 1 << 16, (n, key)      # Kraft sum below 1
    _, kw = X.parts("shared_tables_444")
    complete = K.craft_raw(**dict(kw, tables={**kw["tables"], (0, 0): ([2] + [0] * 15, [0, 1])}))      # the DC table of every component (libjpeg looks at the tables a scan uses)
    assert _probe(lib, complete)[:3] == (D.OP_OK, 24, 40)
    Image = _pillow()
    if Image is not None:
        with pytest.raises(Exception):
            Image.open(io.BytesIO(complete)).convert("RGB")
        assert Image.open(io.BytesIO(X.data("shared_tables_444"))).convert("RGB").size == (40, 24)


def test_sanitizer_program(tmp_path):
    """host code only, as a program of its own: nothing is loaded into Python and nothing is preloaded"""
    exe = D.build_model(tmp_path, sanitize=True)
    good = ["tables3_420", "huff_skew_444", "extend_all_420", "straddle_run_ffd0_444", "huff_flat8_422", "dri_0_then_3_444", "straddle_tile_ffd0_444"]
    paths = [os.path.join(X.GOLDEN, n + ".jpg") for n in good]      # the first three are also mutated 2000 times
    for what in X.CORRUPT:
        p = tmp_path / (what + ".jpg")
        p.write_bytes(X.corrupt(what))
        paths.append(str(p))
    r = subprocess.run([exe] + paths, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    lines = r.stdout.strip().splitlines()
    assert [l.rsplit(": ", 1)[1] for l in lines[:len(paths)]] == ["decoded"] * len(good) + ["refused"] * len(X.CORRUPT), lines[:len(paths)]
    assert lines[-1].startswith("decoded ")
