"""The crafted JPEG corpus of tests/golden/jpeg_craft and the files derived from it at test time, shared by
test_jpeg_craft_cpu.py and test_gpu_jpeg_craft.py.

The good files come from tests/jpeg_craft.py through make_jpeg_craft_fixtures.py; digests.json holds the sha256 of Pillow's RGB
for each.  corrupt(name) builds streams that no entropy coder writes, which the device must answer with OP_ERR_INVALID and
the error bit named here; refused(name) builds files the host parser must turn away."""
import importlib.util
import json
import os

import jpeg_craft as K
import jpeg_dec_cases as D

GOLDEN = os.path.join(D.ROOT, "tests", "golden", "jpeg_craft")
DIGESTS = json.load(open(os.path.join(GOLDEN, "digests.json")))
NAMES = sorted(DIGESTS)
TWOBIT = "twobit_grey_1024x2048"
STRADDLE_TILE = ("straddle_tile_ff00_444", "straddle_tile_ffd0_444")
STRADDLE_RUN = ("straddle_run_ff00_444", "straddle_run_ffd0_444")
PILLOW_MIX = ("size_37x53_420", "rst1_37x53_444", "opt_random_37x53_422", "grey_9x9", "checker01_32x32_420")      # of tests/golden/jpeg_dec

# the error word of jpeg_dec_core.hpp and what err_text of jpeg_dec.hip says for each bit
MARKER, INTERVALS, CODE, INDEX, CAT, END, COUNT = 1, 2, 4, 8, 16, 32, 64
PHRASE = {MARKER: "a marker other than RSTn in the entropy-coded data, or RSTn out of order",
          INTERVALS: "the number of restart intervals is not the frame's",
          INDEX: "a run past coefficient 63",
          CAT: "a coefficient category out of range",
          COUNT: "an interval does not hold the frame's number of blocks"}


def data(name):
    return open(os.path.join(GOLDEN, name + ".jpg"), "rb").read()


def sampling_of(name):
    return D.GREY if "grey" in name else {"444": D.S444, "420": D.S420, "422": D.S422}[name.rsplit("_", 1)[1]]


def generator():
    spec = importlib.util.spec_from_file_location("make_jpeg_craft_fixtures", os.path.join(GOLDEN, "make_jpeg_craft_fixtures.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_parts = {}


def parts(name):
    if name not in _parts:
        _parts[name] = generator().parts(name)
        assert K.craft_raw(**_parts[name][1]) == data(name), name
    return _parts[name]


# ---- corrupt entropy-coded data, all derived from grey_hi_ids_rst1: 24 x 40 grey, 15 blocks, one per restart interval,
# DC table 2, AC table 3.  {name: (the bit that must be set, the bits that may accompany it)}
CORRUPT = {"rst1_for_rst0": (MARKER, 0),              # the first marker is RST1
           "rst_one_more": (INTERVALS, 0),            # a 15th marker, in order, behind the last interval
           "rst_one_less": (INTERVALS, 0),            # the 14th marker is missing
           "fill_in_scan": (MARKER, 0),               # FF FF D0: libjpeg skips the fill byte, this decoder refuses
           "dc_cat12": (CAT, 0),                      # a DC symbol 12 and its twelve bits
           "ac_size11": (CAT, 0),                     # an AC symbol 0B and its eleven bits
           "zrl_past_63": (INDEX, 0),                 # a ZRL at zigzag position 51
           "run_past_63": (INDEX, 0),                 # a symbol D1 (run 13) at zigzag position 51
           "block_extra": (COUNT, 0)}                 # two blocks in an interval of one MCU
BLOCK = 7                                             # the block the symbol-level cases rewrite


def corrupt(name):
    c, kw = parts("grey_hi_ids_rst1")
    scan = kw["scan"]
    if name == "rst1_for_rst0":
        return K.craft_raw(**dict(kw, scan=scan.replace(b"\xff\xd0", b"\xff\xd1", 1)))
    if name == "rst_one_more":
        return K.craft_raw(**dict(kw, scan=scan + b"\xff\xd6"))
    if name == "rst_one_less":
        at = scan.rindex(b"\xff\xd5")
        return K.craft_raw(**dict(kw, scan=scan[:at] + scan[at + 2:]))
    if name == "fill_in_scan":
        return K.craft_raw(**dict(kw, scan=scan.replace(b"\xff\xd0", b"\xff\xff\xd0", 1)))
    # the symbol-level cases write the scan again, over tables that also hold the symbols an encoder never uses
    far = [0] * 64; far[50] = 1                        # DC 0, three ZRLs, symbol 11: the next coefficient is number 51
    freq = K.symbol_counts(list(c) + [far], [0], (2,), (3,), 1)
    freq[(0, 2)][12] = 1
    for s in (0x0B, 0xD1, 0xF0):
        freq[(1, 3)].setdefault(s, 1)
    tables = {k: K.table_for(f, "optimal", dc=k[0] == 0) for k, f in freq.items()}
    sc = K.Scan(tables)
    for i, zz in enumerate(c):
        if i:
            sc.marker(i - 1)
        if i != BLOCK:
            sc.block(zz, 0, 2, 3)
        elif name == "dc_cat12":
            sc.symbol(0, 2, 12); sc.bits(0xABC, 12); sc.symbol(1, 3, 0x00)
        elif name == "ac_size11":
            sc.symbol(0, 2, 0); sc.symbol(1, 3, 0x0B); sc.bits(0x555, 11); sc.symbol(1, 3, 0x00)
        elif name in ("zrl_past_63", "run_past_63"):
            for ac, sym, b, n in K.block_events(far, 0)[:-1]:      # without its EOB
                sc.symbol(ac, 3 if ac else 2, sym); sc.bits(b, n)
            if name == "zrl_past_63":
                sc.symbol(1, 3, 0xF0)
            else:
                sc.symbol(1, 3, 0xD1); sc.bits(1, 1)
        elif name == "block_extra":
            sc.block(zz, 0, 2, 3); sc.block(zz, int(zz[0]), 2, 3)
        else:
            raise KeyError(name)
    return K.craft_raw(**dict(kw, scan=sc.bytes(), tables=tables))


# ---- files the parser refuses: {name: (code, words of the reason)}
REFUSED = {"luma_1x2": (D.OP_ERR_UNSUPPORTED, "sampling other than 4:4:4, 4:2:2 or 4:2:0"),
           "chroma_2x1": (D.OP_ERR_UNSUPPORTED, "chroma sampling other than 1 x 1"),
           "tq_undefined": (D.OP_ERR_INVALID, "missing DQT"),
           "td_undefined": (D.OP_ERR_INVALID, "missing DHT"),
           "ta_undefined": (D.OP_ERR_INVALID, "missing DHT"),
           "dht_oversubscribed": (D.OP_ERR_INVALID, "DHT counts are no prefix code")}


def refused(name):
    _, kw = parts("shared_tables_444")
    if name == "luma_1x2":
        return K.craft_raw(**dict(kw, samp=[0x12, 0x11, 0x11]))
    if name == "chroma_2x1":
        return K.craft_raw(**dict(kw, samp=[0x11, 0x21, 0x11]))
    if name == "tq_undefined":
        return K.craft_raw(**dict(kw, tq=[0, 3, 1]))
    if name == "td_undefined":
        return K.craft_raw(**dict(kw, td=[0, 2, 0]))
    if name == "ta_undefined":
        return K.craft_raw(**dict(kw, ta=[0, 0, 1]))
    if name == "dht_oversubscribed":      # three codes of one bit
        return K.craft_raw(**dict(kw, tables={**kw["tables"], (0, 0): ([3] + [0] * 15, [0, 1, 2])}))
    raise KeyError(name)
