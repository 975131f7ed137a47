"""Writes the JPEG files of this directory and digests.json (sha256 of each file's expected RGB) with tests/jpeg_craft.py.

    python tests/golden/jpeg_craft/make_jpeg_craft_fixtures.py [--check]

These are streams that libjpeg's writer never produces: per-component tables, odd Huffman shapes,
every EXTEND boundary, hand-placed FF bytes and restart markers, DRI edge values, unusual segment layouts.  `fixtures()`
returns {name: file bytes} from seeded coefficients and needs numpy only; tests/test_jpeg_craft_cpu.py regenerates the files
and compares them with the committed bytes.  The expected RGB in digests.json is Pillow's, Image.open(f).convert("RGB"), so
writing the digests needs Pillow; every amplitude stays inside what an encoder could emit, so that libjpeg's range limits and
SIMD paths are not what is tested."""
import hashlib
import io
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(os.path.dirname(HERE))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)
import jpeg_craft as K      # noqa: E402

COLOUR = ("444", "422", "420")
SMALL = (24, 40)            # 15 / 9 / 6 MCUs at 4:4:4 / 4:2:2 / 4:2:0: two MCU rows and columns at least, a partial edge at 4:2:0
TILE = 8192                 # bytes of a tile of k_jd_scan; a thread's run is 8
ONES = [1] * 64


def blocks(rng, n, dc=24, amp=3, density=0.35, runs=None):
    """n blocks: a DC in [-dc, dc], ACs of magnitude 1..amp; with runs, zero runs drawn from it (few distinct symbols)"""
    c = np.zeros((n, 64), np.int64)
    c[:, 0] = rng.integers(-dc, dc + 1, n)
    mag = rng.integers(1, amp + 1, (n, 63)) * rng.choice((-1, 1), (n, 63))
    if runs is None:
        c[:, 1:] = np.where(rng.random((n, 63)) < density * np.linspace(1.5, 0.3, 63), mag, 0)
        return c
    for b in range(n):
        k = 1 + int(rng.choice(runs))
        while k < 64 and rng.random() < 0.8:
            c[b, k] = mag[b, k - 1]
            k += 1 + int(rng.choice(runs))
    return c


def scene(sampling, seed, h=SMALL[0], w=SMALL[1], **kw):
    """seeded blocks for an h x w image; chroma blocks are quieter than luma blocks"""
    nmcu, comps = K.geometry(h, w, sampling)
    rng = np.random.default_rng(seed)
    c = blocks(rng, nmcu * len(comps), **kw)
    for i in range(len(c)):
        if comps[i % len(comps)]:
            c[i, 0] //= 2
    return c


def dc_walk(diffs):
    """DC values whose differences hold `diffs` in order, with a step back into [-1024, 1023] wherever the next would leave it"""
    out = []; dc = 0
    for d in diffs:
        if not -1024 <= dc + d <= 1023:
            dc = -1024 if d > 0 else 1023
            out.append(dc)
        dc += d
        out.append(dc)
    out.append(0)
    return out


def extend_blocks():
    """-> (blocks that walk the DC through all four boundary values of the categories 1..11 and end in an EOB each,
    blocks of DC 0 whose ACs hold the four boundary values of the categories 1..10 and the special runs)"""
    bound = lambda s: (2 ** s - 1, -(2 ** s - 1), 2 ** (s - 1), -(2 ** (s - 1)))
    walk = dc_walk([v for s in range(1, 12) for v in bound(s)])
    dcs = np.zeros((len(walk), 64), np.int64)
    dcs[:, 0] = walk
    acs = []
    spots = (1, 5, 17, 33, 47, 62)
    for s in range(1, 11):
        for i, v in enumerate(bound(s)):
            b = np.zeros(64, np.int64); b[spots[(s + i) % len(spots)]] = v
            acs.append(b)
    for first, v in ((46, 1023), (30, -1023), (0, 512), (0, -1)):      # coefficient 63 behind one, two, three and three ZRLs
        b = np.zeros(64, np.int64); b[63] = v
        if first:
            b[first] = 1
        acs.append(b)
    b = np.zeros(64, np.int64); b[1] = 2; b[17] = -3; b[33] = 5; b[49] = 300      # run 15 with sizes 2, 3, 9
    acs.append(b)
    full = np.zeros(64, np.int64)
    full[1:] = np.random.default_rng(63).integers(1, 4, 63) * np.random.default_rng(64).choice((-1, 1), 63)
    acs.append(full)
    return dcs, np.array(acs)


def extend_all(sampling):
    dcs, acs = extend_blocks()
    if sampling == "grey":
        seq = np.concatenate([dcs, acs])
        cols = 14; rows = -(-len(seq) // cols)
        c = np.zeros((rows * cols, 64), np.int64); c[:len(seq)] = seq
        return K.craft(8 * rows, 8 * cols, "grey", c)
    # 4:2:0: luma holds both lists, Cb the DC walk, Cr the AC blocks; short lists are padded with blocks of difference 0
    luma = np.concatenate([dcs, acs])
    nmcu = max(-(-len(luma) // 4), len(dcs), len(acs))
    cols = 13; rows = -(-nmcu // cols); nmcu = rows * cols
    pad = lambda a, n: np.concatenate([a, np.zeros((n - len(a), 64), np.int64)])
    y = pad(luma, 4 * nmcu).reshape(nmcu, 4, 64); cb = pad(dcs, nmcu); cr = pad(acs, nmcu)
    c = np.concatenate([y, cb[:, None], cr[:, None]], axis=1).reshape(-1, 64)
    return K.craft(16 * rows, 16 * cols, "420", c, tq=(0, 0, 0), td=(0, 1, 1), ta=(0, 1, 1))


def search(make, ok, what, tries=4000):
    """the first seed whose file passes ok(file, scan, ends)"""
    for seed in range(tries):
        ends = []
        f, kw = make(seed, ends)
        if ok(f, kw["scan"], ends):
            return f
    raise RuntimeError("no seed reaches " + what)


def _marker_at(scan, i):
    return i + 1 < len(scan) and scan[i] == 0xFF and (scan[i + 1] & 0xF8) == 0xD0


# ---- tile straddles: 64 x 64 at 4:4:4 with fixed 8-bit codes, so that a tuning MCU changes no code and every coefficient of
# magnitude 1 costs 9 bits, of magnitude 2 or 3 ten
def _straddle_tables():
    """DC: twelve 8-bit codes.  AC: 255 8-bit codes, symbol 01 the last (1111 1110): a run of +1 coefficients is then
    1111 1110 1 repeated, eight 1-bits every nine bits, which fall on a byte boundary every nine bytes"""
    legal = [0x00, 0xF0] + [r << 4 | s for r in range(16) for s in range(1, 11) if (r, s) != (0, 1)]
    spare = [r << 4 | s for s in range(11, 16) for r in range(16)] + [r << 4 for r in range(1, 15)]      # never written
    ac = legal + spare[: 254 - len(legal)] + [0x01]
    return {(0, 0): ([0] * 7 + [12] + [0] * 8, list(range(12))), (1, 0): ([0] * 7 + [255] + [0] * 8, ac)}


def straddle(kind):
    """kind "ff00": an unbroken scan with a stuffed FF at offset 8191 and its 00 at 8192; "ffd0": interval 0 is exactly 8191
    bytes, so that RST0 lies across the tile boundary.  MCU 0 (three blocks of DC 0, so that no later difference changes) is
    tuned: a coefficients of -1 and b of 2 move everything behind it by 9 a + 10 b bits."""
    _, comps = K.geometry(64, 64, "444")
    c = scene("444", 7 if kind == "ff00" else 8, 64, 64, amp=3, density=0.7, dc=30)
    c[:3] = 0
    tables = _straddle_tables()
    length = [0]                # bytes of the scan of the first n blocks, padded and stuffed
    sc = K.Scan(tables); pred = [0, 0, 0]
    for i, zz in enumerate(c):
        pred[comps[i % 3]] = sc.block(zz, pred[comps[i % 3]], 0, 0)
        k = -sc.n % 8
        by = ((sc.acc << k) | ((1 << k) - 1)).to_bytes((sc.n + k) // 8, "big")
        length.append(len(by) + by.count(b"\xff"))
    ri = 0
    if kind == "ff00":          # two blocks of +1 coefficients (142 bytes) that begin some 100 bytes before the boundary
        j = max(n for n in range(3, 192) if length[n] <= TILE - 100)
        c[j: j + 2, 1:] = 1
    else:                       # the largest interval that, with an empty MCU 0, stays 12 bytes or more below the boundary
        ri = max(r for r in range(1, 64) if length[3 * r] <= TILE - 1 - 12)
    last = 3 * ri if ri else len(c)
    tail = K.Scan(tables); pred = [0, 0, 0]
    for i in range(3, last):
        pred[comps[i % 3]] = tail.block(c[i], pred[comps[i % 3]], 0, 0)
    found = None
    for n in range(190):
        for a in range(n + 1):
            t = np.zeros(189, np.int64); t[:a] = -1; t[a: n] = 2
            m = np.zeros((3, 64), np.int64); m[:, 1:] = t.reshape(3, 63)
            head = K.Scan(tables)
            for blk in m:
                head.block(blk, 0, 0, 0)
            head.bits(tail.acc, tail.n)
            s = head.bytes()
            if (s[TILE - 1: TILE + 1] == b"\xff\x00") if kind == "ff00" else len(s) == TILE - 1:
                found = m
                break
        if found is not None:
            break
    else:
        raise RuntimeError("no tuning found")
    c[:3] = found
    f, kw = K.craft(64, 64, "444", c, huff={k: (tuple(t[0]), tuple(t[1])) for k, t in tables.items()}, ri=ri, info=True)
    assert len(kw["scan"]) > TILE and kw["scan"][TILE - 1: TILE + 1] == (b"\xff\x00" if kind == "ff00" else b"\xff\xd0")
    return f


def twobit():
    """1024 x 2048 grey: every block is a DC difference of 0 and an EOB, two bits, but every 97th, which steps the DC by one
    quantiser step (+1, then -1) so that a block written to the wrong place shows"""
    n = 128 * 256
    c = np.zeros((n, 64), np.int64)
    c[:, 0] = (np.arange(n) // 97) & 1
    return K.craft(1024, 2048, "grey", c, qtables={0: [16] * 64})


RAMP = [2 + (3 * k) % 7 for k in range(64)]


def parts(name):
    """-> (coefficients, the arguments of craft_raw) of a file that the tests derive corrupt and refused files from"""
    h, w = SMALL
    if name == "grey_hi_ids_rst1":
        c = scene("grey", 14)
        return c, K.craft(h, w, "grey", c, ids=(0,), tq=(3,), td=(2,), ta=(3,), qtables={3: RAMP}, ri=1, info=True)[1]
    if name == "shared_tables_444":
        c = scene("444", 2)
        return c, K.craft(h, w, "444", c, tq=(0, 1, 1), qtables={0: RAMP, 1: [5] * 64}, info=True)[1]
    raise KeyError(name)


def fixtures():
    out = {}
    ramp = RAMP
    h, w = SMALL
    for s in COLOUR:
        nmcu, comps = K.geometry(h, w, s)
        # per-component tables: Cb all 1 against Cr all 37, three Huffman pairs
        c = scene(s, 1, amp=2, density=0.2, dc=8)
        for i in range(len(c)):
            if comps[i % len(comps)] == 1:
                c[i, 1:] *= 9
        out[f"tables3_{s}"] = K.craft(h, w, s, c, tq=(0, 2, 1), td=(0, 3, 1), ta=(2, 0, 3), qtables={0: ramp, 2: ONES, 1: [37] * 64})
        out[f"shared_tables_{s}"] = K.craft(h, w, s, scene(s, 2), tq=(0, 1, 1), qtables={0: ramp, 1: [5] * 64})      # parts() repeats this
        q2 = dict(tq=(0, 1, 1), qtables={0: ramp, 1: [4] * 64}, td=(0, 1, 1), ta=(0, 1, 1))
        out[f"ids_012_{s}"] = K.craft(h, w, s, scene(s, 3), ids=(0, 1, 2), **q2)
        out[f"ids_7_200_33_{s}"] = K.craft(h, w, s, scene(s, 4), ids=(7, 200, 33), **q2)
        out[f"ids_adobe_{s}"] = K.craft(h, w, s, scene(s, 5), layout=["ADOBE", "DQT", "SOF", "DHT", "SOS"], **q2)
        # Huffman shapes
        out[f"huff_skew_{s}"] = K.craft(h, w, s, scene(s, 6, amp=3, dc=6, runs=(0, 1, 2)), huff="skew", **q2)
        out[f"huff_flat8_{s}"] = K.craft(h, w, s, scene(s, 7), huff="flat8", **q2)
        out[f"huff_shuffled_{s}"] = K.craft(h, w, s, scene(s, 8, amp=7), huff="shuffled", **q2)
        _, kw = K.craft(h, w, s, scene(s, 9), info=True, **q2)
        wrong = [(k, (t[0], t[1][::-1])) for k, t in sorted(kw["tables"].items())]      # the same lengths, the symbols reversed
        out[f"huff_redefined_{s}"] = K.craft_raw(**dict(kw, layout=["JFIF", "DQT", "SOF", ("DHT", wrong[:2]), ("DHT", wrong[2:]), "DHT", "SOS"]))
        # interval endings
        out[f"pad0_{s}"] = K.craft(h, w, s, scene(s, 10), ri=2, pad=0, **q2)
        out[f"pad_none_{s}"] = search(lambda seed, e: K.craft(h, w, s, scene(s, 1000 + seed), ri=1, info=True, ends=e, **q2),
                                      lambda f, sc, e: e[0] % 8 == 0 and e[-1] % 8 == 0, "intervals without padding")
        # coefficient 63 = 255 is eight 1-bits at the end of an interval: its last byte is FF wherever the bits fall
        c = scene(s, 15)
        c[len(comps) - 1, 63] = c[-1, 63] = 255
        out[f"ends_ff_{s}"] = K.craft(h, w, s, c, ri=1, tq=(0, 1, 1), qtables={0: ONES, 1: ONES}, td=(0, 1, 1), ta=(0, 1, 1))
        out[f"starts_ff_{s}"] = K.craft(h, w, s, scene(s, 11), ri=2, huff={(0, 0): "skew"}, **q2)
        # DRI edges
        for tag, dri in (("eq", [nmcu]), ("plus1", [nmcu + 1]), ("65535", [65535]), ("0", [0]), ("1_then_0", [1, 0]), ("0_then_3", [0, 3]), ("minus1", [nmcu - 1])):
            out[f"dri_{tag}_{s}"] = K.craft(h, w, s, scene(s, 12), layout=["JFIF", "DQT", "SOF", "DHT"] + [("DRI", d) for d in dri] + ["SOS"], **q2)
        # segment layouts
        c = scene(s, 13)
        for tag, lay in (("tables_around_sof", ["JFIF", "DHT", "SOF", "DQT", "SOS"]),
                         ("split", ["JFIF", "DQT", "SOF", "DHT", "SOS"]),
                         ("joined", ["JFIF", "DQT*", "SOF", "DHT*", "SOS"]),
                         ("dqt_twice", ["JFIF", ("DQT", [(0, [99] * 64), (1, [1] * 64)]), "DQT", "SOF", "DHT", "SOS"]),
                         ("dri_first", ["JFIF", ("DRI", 2), "DQT", "SOF", "DHT", "SOS"]),
                         ("fill", ["JFIF", "DQT", "FILL", "SOF", "DHT", "FILL", "SOS"]),
                         ("empty_segments", ["JFIF", ("COM", b""), "DQT", ("APP", 15, b""), "SOF", "DHT", "SOS"])):
            out[f"layout_{tag}_{s}"] = K.craft(h, w, s, c, layout=lay, **q2)
    c = scene("grey", 14)
    out["grey_hi_ids"] = K.craft(h, w, "grey", c, ids=(0,), tq=(3,), td=(2,), ta=(3,), qtables={3: ramp})
    out["grey_hi_ids_rst1"] = K.craft_raw(**parts("grey_hi_ids_rst1")[1])
    out["extend_all_grey"] = extend_all("grey")
    out["extend_all_420"] = extend_all("420")
    out["straddle_tile_ff00_444"] = straddle("ff00")
    out["straddle_tile_ffd0_444"] = straddle("ffd0")
    small = lambda seed, e: K.craft(16, 16, "444", scene("444", 3000 + seed, 16, 16, amp=15, density=0.8), ri=1, info=True, ends=e)
    out["straddle_run_ff00_444"] = search(small, lambda f, sc, e: any(sc[i: i + 2] == b"\xff\x00" for i in range(7, len(sc), 8)), "FF 00 across two runs")
    out["straddle_run_ffd0_444"] = search(small, lambda f, sc, e: any(_marker_at(sc, i) for i in range(7, len(sc), 8)), "FF Dn across two runs")
    out["twobit_grey_1024x2048"] = twobit()
    return out


def expected_rgb(data):
    from PIL import Image
    return np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(data)).convert("RGB")))


def main():
    fx = fixtures()
    if "--check" in sys.argv:
        bad = [n for n, b in fx.items() if open(os.path.join(HERE, n + ".jpg"), "rb").read() != b]
        print("differ:", bad) if bad else print("all", len(fx), "files regenerate to the committed bytes")
        sys.exit(1 if bad else 0)
    digests = {}
    for n, b in sorted(fx.items()):
        open(os.path.join(HERE, n + ".jpg"), "wb").write(b)
        rgb = expected_rgb(b)
        digests[n] = {"h": int(rgb.shape[0]), "w": int(rgb.shape[1]), "bytes": len(b), "sha256": hashlib.sha256(rgb.tobytes()).hexdigest()}
    with open(os.path.join(HERE, "digests.json"), "w") as f:
        json.dump(digests, f, indent=1, sort_keys=True)
        f.write("\n")
    print(len(fx), "files,", sum(len(b) for b in fx.values()), "bytes")


if __name__ == "__main__":
    main()
