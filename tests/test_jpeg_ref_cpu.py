"""JPEG encoder, the parts that need no GPU:

1. the library is still ABI 12 and exports the encoder's five entry points (it loads without a device);
2. the serial restatement of the device encoder (tests/harness/jpeg_ref.c) writes, for every input of jpeg_cases.CASES at
   qualities 1, 50, 90, 100 and both samplings, the file libjpeg writes (Pillow: optimize off, the same restart interval) --
   byte for byte.  Skipped only where Pillow is missing, has no JPEG codec or is older than restart_marker_blocks;
3. the same files against tests/golden/jpeg_ref_digests.json, recorded where 2 held: pins the bytes without Pillow;
4. a walk of the markers with ``struct`` only: segment lengths, DRI, RSTn in order mod 8, no other FF xx in the scan, EOI last;
5. jpeg_ref_stats: each crafted input reaches what it was built for (REACHES), and no interval outgrows its slot;
6. size: on natural_400x600 at quality 90 the restart markers cost at most 3 % over libjpeg's file without them;
7. (no reciprocal: the quantiser divides, in the kernel and in the restatement);
8. quality 100 at 4:2:0 -- the reference's own out.jpg format -- decodes to the pixels of libjpeg's file without restart markers;
9. the restart intervals of jpeg.hip, of the restatement and of jpeg_cases agree."""
import hashlib
import io
import json
import os
import struct

import numpy as np
import pytest

import jpeg_cases as J
from openpano_amd import hip

DIGESTS = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_ref_digests.json")))
IDS = [J.combo_id(*c) for c in J.COMBOS]

# (case, quality, sampling) -> what the restatement's statistics must show for it.  DC category 11 and AC category 10 are the
# format's largest (a DC difference of +-2040, an AC coefficient of +-1023 at quantiser 1), and both are reached.
REACHES = {
    ("random_31x47", 100, J.S444): lambda s: s["stuffed"] > 0 and s["no_eob"] > 0,
    ("chroma_bottom_40x56", 100, J.S420): lambda s: s["stuffed_pad"] > 0 and s["dummy_right"] > 0 and s["dummy_bottom"] > 0,
    ("chroma_bottom_40x56", 100, J.S444): lambda s: s["stuffed_pad"] > 0 and s["dummy_right"] == 0 and s["dummy_bottom"] == 0,
    ("one_interval_plus_one_444_8x264", 50, J.S444): lambda s: s["zrl"] > 0 and s["intervals"] == 2,
    ("one_interval_444_8x256", 90, J.S444): lambda s: s["intervals"] == 1,
    ("one_interval_420_16x128", 90, J.S420): lambda s: s["intervals"] == 1,
    ("one_interval_plus_one_420_16x144", 90, J.S420): lambda s: s["intervals"] == 2,
    ("marker_wrap_136x136", 90, J.S444): lambda s: s["intervals"] >= 9,
    ("marker_wrap_136x136", 90, J.S420): lambda s: s["intervals"] >= 9,
    ("block_steps_16x64", 100, J.S444): lambda s: s["max_dc_cat"] == 11,
    ("checker01_32x32", 100, J.S444): lambda s: s["max_ac_cat"] == 10,
    ("checker01_32x32", 100, J.S420): lambda s: s["max_ac_cat"] == 10,
    ("all255_16x64", 1, J.S420): lambda s: s["max_ac_cat"] == 0 and s["zrl"] == 0,
}


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return J.build_ref(tmp_path_factory.mktemp("jpegref"))


@pytest.fixture(scope="module")
def runs(ref):
    """(case, quality, sampling) -> (file, statistics) of the restatement, every combination encoded once"""
    out = {}
    for name, q, s in J.COMBOS:
        if name in J.NEEDS_PIL and not J.png_cases.natural.available():
            continue
        jpg = J.ref_encode(ref, J.case(name), q, s)
        out[(name, q, s)] = (jpg, J.ref_stats(ref).as_dict())
    return out


@pytest.fixture(scope="module")
def big(ref):
    name, make, q, s = J.BIG
    rgb = make()
    return rgb, J.ref_encode(ref, rgb, q, s), J.ref_stats(ref).as_dict()


def _get(runs, combo):
    if combo not in runs:
        pytest.skip("PIL not available")
    return runs[combo]


def _require_pillow():
    Image = J.pillow()
    if Image is None:
        pytest.skip("Pillow with a JPEG codec and restart_marker_blocks (10.2) not available")
    return Image


def _first_difference(a, b):
    n = min(len(a), len(b))
    return next((i for i in range(n) if a[i] != b[i]), n)


def test_abi_12_and_symbols():
    L = hip.lib()
    assert L.op_abi_version() == 12
    for name in ("op_canvas_encode_jpeg", "op_jpeg_encode_u8", "op_jpeg_size", "op_jpeg_copy", "op_jpeg_free"):
        assert hasattr(L, name), name


def test_restart_intervals_agree(ref):
    assert J.kernel_intervals() == J.RI
    for s in J.SUBSAMPLINGS:
        assert ref.jpeg_ref_interval(s) == J.RI[s] and ref.jpeg_ref_slot(s) == J.SLOT[s]
    assert ref.jpeg_ref_interval(2) == -1


@pytest.mark.parametrize("combo", J.COMBOS, ids=IDS)
def test_reference_file_equals_libjpeg(runs, combo):
    Image = _require_pillow()
    name, q, s = combo
    got, _ = _get(runs, combo)
    want = J.pillow_encode(Image, J.case(name), q, s, J.RI[s])
    assert got == want, f"restatement {len(got)} bytes, libjpeg {len(want)} bytes, first difference at byte {_first_difference(got, want)}"


@pytest.mark.parametrize("combo", J.COMBOS, ids=IDS)
def test_reference_file_digest(runs, combo):
    got, _ = _get(runs, combo)
    assert hashlib.sha256(got).hexdigest() == DIGESTS[J.combo_id(*combo)]


def test_big_canvas(big):
    rgb, got, st = big
    name, _, q, s = J.BIG
    assert hashlib.sha256(got).hexdigest() == DIGESTS[J.combo_id(name, q, s)]
    info = J.walk(got)
    assert (info["h"], info["w"]) == rgb.shape[:2] and len(info["intervals"]) == st["intervals"] == 3000
    assert st["max_interval_bytes"] <= J.SLOT[s]
    Image = J.pillow()
    if Image is not None:
        assert got == J.pillow_encode(Image, rgb, q, s, J.RI[s])


@pytest.mark.parametrize("combo", J.COMBOS, ids=IDS)
def test_marker_walk(runs, combo):
    name, q, s = combo
    jpg, st = _get(runs, combo)
    info = J.walk(jpg)
    h, w, _ = J.case(name).shape
    assert (info["h"], info["w"]) == (h, w)
    assert info["dri"] == J.RI[s]
    assert info["sampling"] == ((0x22, 0x11, 0x11) if s == J.S420 else (0x11, 0x11, 0x11)) and info["tq"] == (0, 1, 1)
    assert len(info["intervals"]) == st["intervals"]
    assert max(len(iv) for iv in info["intervals"]) == st["max_interval_bytes"] <= J.SLOT[s]
    segs = info["segments"]
    assert segs[0][1] == b"JFIF\0" + struct.pack(">BBBHHBB", 1, 1, 0, 1, 1, 0, 0)
    assert [b[0] for m, b in segs if m == 0xDB] == [0, 1] and all(len(b) == 65 for m, b in segs if m == 0xDB)
    assert [b[0] for m, b in segs if m == 0xC4] == [0x00, 0x10, 0x01, 0x11]
    assert segs[-1][1] == bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])


def test_huffman_tables_are_the_standard_ones(runs):
    """the DHT segments against those of a file libjpeg writes without `optimize`, and the counts of ITU T.81 Annex K.3"""
    jpg, _ = runs[("8x8", 90, J.S420)]
    dht = [b for m, b in J.walk(jpg)["segments"] if m == 0xC4]
    assert list(dht[0][1:17]) == [0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0] and list(dht[0][17:]) == list(range(12))
    assert list(dht[2][1:17]) == [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0] and list(dht[2][17:]) == list(range(12))
    assert list(dht[1][1:17]) == [0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125] and len(dht[1]) == 17 + 162
    assert list(dht[3][1:17]) == [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119] and len(dht[3]) == 17 + 162
    Image = _require_pillow()
    theirs = J.pillow_encode(Image, J.case("8x8"), 90, J.S420, J.RI[J.S420])
    assert dht == [b for m, b in J.walk(theirs)["segments"] if m == 0xC4]


@pytest.mark.parametrize("combo", list(REACHES), ids=[J.combo_id(*c) for c in REACHES])
def test_crafted_inputs_reach_their_lines(runs, combo):
    _, st = runs[combo]
    assert REACHES[combo](st), st


def test_every_line_is_reached_and_no_interval_outgrows_its_slot(runs, ref):
    top = {}
    for (name, q, s), (_, st) in runs.items():
        assert st["max_interval_bytes"] <= J.SLOT[s] == ref.jpeg_ref_slot(s), (name, q, s, st)
        for k, v in st.items():
            top[k] = max(top.get(k, 0), v)
    for k in ("stuffed", "stuffed_pad", "zrl", "no_eob", "dummy_right", "dummy_bottom"):
        assert top[k] > 0, k
    assert top["max_dc_cat"] == 11 and top["max_ac_cat"] == 10


@pytest.mark.parametrize("s", J.SUBSAMPLINGS, ids=["444", "420"])
def test_restart_markers_cost_at_most_3_percent(runs, s):
    Image = _require_pillow()
    got, _ = _get(runs, ("natural_400x600", 90, s))
    plain = J.pillow_encode(Image, J.case("natural_400x600"), 90, s, 0)
    print(f"natural_400x600 q90 {'420' if s else '444'}: {len(got)} / {len(plain)} = {len(got) / len(plain):.4f}")
    assert len(got) <= 1.03 * len(plain)


@pytest.mark.parametrize("name", list(J.CASES))
def test_quality_100_420_decodes_like_the_file_without_markers(runs, name):
    Image = _require_pillow()
    got, _ = _get(runs, (name, 100, J.S420))
    plain = J.pillow_encode(Image, J.case(name), 100, J.S420, 0)
    a = np.asarray(Image.open(io.BytesIO(got)).convert("RGB"))
    b = np.asarray(Image.open(io.BytesIO(plain)).convert("RGB"))
    assert a.shape == J.case(name).shape and np.array_equal(a, b)
