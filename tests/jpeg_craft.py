"""A coefficient-level writer of baseline JPEG files for the decoder's tests, in plain Python and numpy.

Its input is quantised coefficients per block, in scan order and zigzag order, not pixels: the decoder is an integer function
of the file, so a test can choose every symbol of the stream and needs no forward DCT.  Everything libjpeg's writer keeps
constant is a parameter here: component ids, Tq / Td / Ta per component, up to four tables of each kind, the shape of the
Huffman codes, the restart interval, the pad bit, and the order and grouping of the header segments.

    craft(h, w, sampling, coefs, ...)      a file from coefficients
    craft_raw(h, w, samp, scan, ...)       a file from header fields and raw scan bytes (for streams no entropy coder writes)
    Scan                                   the bit writer behind both, for scans that are wrong on purpose

No complete code is ever built: the all-ones codeword stays free, as libjpeg demands of a DHT."""
import heapq

import numpy as np

SAMPLING = {"444": (1, 1, 3), "422": (2, 1, 3), "420": (2, 2, 3), "grey": (1, 1, 1)}
PROFILES = ("optimal", "shuffled", "skew", "flat8")


def geometry(h, w, sampling):
    """-> (MCUs, the component of each block of an MCU)"""
    hs, vs, nc = SAMPLING[sampling]
    nmcu = -(-w // (8 * hs)) * -(-h // (8 * vs))
    return nmcu, [0] * (hs * vs if nc == 3 else 1) + ([1, 2] if nc == 3 else [])


def size_bits(v):
    """category and value bits of a coefficient or DC difference (the inverse of EXTEND)"""
    v = int(v)
    s = abs(v).bit_length()
    return s, v if v >= 0 else v + (1 << s) - 1


def block_events(zz, pred):
    """the symbols of one block: [(0 for DC / 1 for AC, symbol, value bits, their number)]"""
    s, b = size_bits(int(zz[0]) - pred)
    ev = [(0, s, b, s)]
    nz = [k for k in range(1, 64) if zz[k]]
    run = 0
    for k in range(1, (nz[-1] if nz else 0) + 1):
        if not zz[k]:
            run += 1
            continue
        while run > 15:
            ev.append((1, 0xF0, 0, 0)); run -= 16
        s, b = size_bits(zz[k])
        ev.append((1, run << 4 | s, b, s)); run = 0
    if not nz or nz[-1] < 63:
        ev.append((1, 0x00, 0, 0))
    return ev


# ---- Huffman tables: (counts[16], vals)
def codes_of(table):
    """{symbol: (code, length)} of the canonical code"""
    counts, vals = table
    out = {}; code = 0; k = 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            out.setdefault(vals[k], (code, length)); code += 1; k += 1
        code <<= 1
    return out


def _optimal_counts(weights):
    """codes per length (index 1..16) of a Huffman code over the weights plus one reserved leaf, limited to 16 bits by the
    adjustment of the standard's Annex K.3, the reserved (all-ones) code taken out of the longest length"""
    heap = [(0, 0, [0])] + [(wt, i + 1, [i + 1]) for i, wt in enumerate(weights)]
    depth = [0] * (len(weights) + 1)
    heapq.heapify(heap)
    tick = len(heap)
    while len(heap) > 1:
        a = heapq.heappop(heap); b = heapq.heappop(heap)
        for leaf in a[2] + b[2]:
            depth[leaf] += 1
        heapq.heappush(heap, (a[0] + b[0], tick, a[2] + b[2])); tick += 1
    bits = [0] * (max(depth) + 2)
    for d in depth:
        bits[d] += 1
    for i in range(len(bits) - 1, 16, -1):
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2; bits[i - 1] += 1; bits[j + 1] += 2; bits[j] -= 1
    bits = (bits + [0] * 17)[:17]
    bits[max(i for i in range(17) if bits[i])] -= 1
    return bits


def table_for(freq, profile="optimal", dc=False):
    """a table that codes every symbol of freq ({symbol: count}) with a code of the named shape:
    optimal   Huffman lengths limited to 16 bits, symbols of a length in ascending order (what libjpeg's optimiser writes)
    shuffled  the same lengths, symbols of a length in descending order
    skew      one code per length 1..16: unused symbols take the short codes, the stream's rarest symbol the 16-bit one
    flat8     every code 8 bits long: 200 codes for AC (twelve for DC), most of them unused"""
    if isinstance(profile, tuple):
        return list(profile[0]), list(profile[1])
    need = sorted(freq, key=lambda s: (-freq[s], s))
    spare = [s for s in (range(16) if dc else range(255, 0, -1)) if s not in freq]
    if profile in ("optimal", "shuffled"):
        bits = _optimal_counts([freq[s] for s in need])
        vals = []; k = 0
        for length in range(1, 17):
            vals += sorted(need[k: k + bits[length]], reverse=profile == "shuffled"); k += bits[length]
        return bits[1:], vals
    if profile == "skew":
        assert len(need) <= 16, "a skewed table holds 16 symbols"
        return [1] * 16, spare[: 16 - len(need)] + need
    if profile == "flat8":
        n = max(len(need), 12 if dc else 200)
        assert n <= 255
        return [0] * 7 + [n] + [0] * 8, need + spare[: n - len(need)]
    raise KeyError(profile)


# ---- the entropy-coded data
class Scan:
    """A bit writer over a set of Huffman tables {(Tc, Th): (counts, vals)}.  block() writes a block as an encoder would;
    symbol(), bits(), align() and marker() write whatever they are told."""

    def __init__(self, tables, pad=1):
        self.codes = {k: codes_of(t) for k, t in tables.items()}
        self.pad = pad
        self.out = bytearray()
        self.acc = 0; self.n = 0
        self.ends = []                  # bits written since the last align(), at every align()

    def bits(self, v, n):
        self.acc = self.acc << n | (v & ((1 << n) - 1)); self.n += n

    def symbol(self, tc, th, sym):
        code, length = self.codes[(tc, th)][sym]
        self.bits(code, length)

    def block(self, zz, pred, td, ta):
        """-> the block's DC value, the next block's predictor"""
        for ac, sym, b, n in block_events(zz, pred):
            self.symbol(ac, ta if ac else td, sym)
            self.bits(b, n)
        return int(zz[0])

    def align(self, pad=None):
        """pad to a byte with the pad bit, stuff FF bytes, and move the bits out"""
        pad = self.pad if pad is None else pad
        self.ends.append(self.n)
        k = -self.n % 8
        self.bits((1 << k) - 1 if pad else 0, k)
        self.out += self.acc.to_bytes(self.n // 8, "big").replace(b"\xff", b"\xff\x00")
        self.acc = 0; self.n = 0

    def marker(self, k, pad=None):
        self.align(pad)
        self.out += bytes([0xFF, 0xD0 + (k & 7)])

    def raw(self, b):
        self.align()
        self.out += b

    def bytes(self):
        self.align()
        return bytes(self.out)


def symbol_counts(coefs, comps, td, ta, ri):
    """{(Tc, Th): {symbol: count}} of a scan"""
    freq = {}
    pred = [0, 0, 0]
    bpm = len(comps)
    for i, zz in enumerate(coefs):
        if ri and i % (ri * bpm) == 0:
            pred = [0, 0, 0]
        c = comps[i % bpm]
        for ac, sym, _, _ in block_events(zz, pred[c]):
            f = freq.setdefault((ac, ta[c] if ac else td[c]), {})
            f[sym] = f.get(sym, 0) + 1
        pred[c] = int(zz[0])
    return freq


def encode_scan(coefs, comps, td, ta, tables, ri=0, pad=1, ends=None):
    """the scan of an encoder: ri MCUs per restart interval (0: none), RSTn between the intervals.  ends: a list that receives
    the number of data bits of every interval"""
    sc = Scan(tables, pad)
    bpm = len(comps)
    pred = [0, 0, 0]
    for i, zz in enumerate(coefs):
        if ri and i and i % (ri * bpm) == 0:
            sc.marker(i // (ri * bpm) - 1)
            pred = [0, 0, 0]
        c = comps[i % bpm]
        pred[c] = sc.block(zz, pred[c], td[c], ta[c])
    out = sc.bytes()
    if ends is not None:
        ends += sc.ends
    return out


# ---- the header
def _seg(marker, payload):
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload)


def _dqt(items):
    return _seg(0xDB, b"".join(bytes([i]) + bytes(int(v) for v in t) for i, t in items))


def _dht(items):
    return _seg(0xC4, b"".join(bytes([tc << 4 | th]) + bytes(t[0]) + bytes(t[1]) for (tc, th), t in items))


JFIF = _seg(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
ADOBE = _seg(0xEE, b"Adobe\x00\x64\x00\x00\x00\x00\x01")      # transform 1: YCbCr


def default_layout(ri=0):
    return ["JFIF", "DQT", "SOF", "DHT"] + ([("DRI", ri)] if ri else []) + ["SOS"]


def craft_raw(h, w, samp, scan, ids, tq, td, ta, qtables, tables, layout=None):
    """SOI, the segments `layout` names, the scan bytes as they are, EOI.  samp: the sampling byte of each component.
    layout entries: "JFIF", "ADOBE", ("APP", n, payload), ("COM", payload), "FILL" (FF FF FF before the next marker),
    "DQT" / "DHT" (every table in a segment of its own), "DQT*" / "DHT*" (all in one segment), ("DQT", [id or (id, table)])
    and ("DHT", [(Tc, Th) or ((Tc, Th), table)]) (one segment of exactly these), ("DRI", n), "SOF", "SOS"."""
    out = bytearray(b"\xff\xd8")
    nc = len(samp)
    for e in layout or default_layout():
        kind, args = (e, ()) if isinstance(e, str) else (e[0], e[1:])
        if kind == "JFIF":
            out += JFIF
        elif kind == "ADOBE":
            out += ADOBE
        elif kind == "APP":
            out += _seg(0xE0 + args[0], args[1])
        elif kind == "COM":
            out += _seg(0xFE, args[0])
        elif kind == "FILL":
            out += b"\xff\xff\xff"
        elif kind in ("DQT", "DQT*", "DHT", "DHT*"):
            have = qtables if kind[1] == "Q" else tables
            # an id ((Tc, Th) for DHT) names the file's own table; (id, table) carries one
            items = [(k, have[k]) if isinstance(k, int) or (kind[1] == "H" and isinstance(k[0], int)) else k for k in (args[0] if args else sorted(have))]
            write = _dqt if kind[1] == "Q" else _dht
            if args or kind.endswith("*"):
                out += write(items)
            else:
                for it in items:
                    out += write([it])
        elif kind == "DRI":
            out += _seg(0xDD, int(args[0]).to_bytes(2, "big"))
        elif kind == "SOF":
            out += _seg(0xC0, bytes([8]) + h.to_bytes(2, "big") + w.to_bytes(2, "big") + bytes([nc]) +
                        b"".join(bytes([ids[c], samp[c], tq[c]]) for c in range(nc)))
        elif kind == "SOS":
            out += _seg(0xDA, bytes([nc]) + b"".join(bytes([ids[c], td[c] << 4 | ta[c]]) for c in range(nc)) + b"\x00\x3f\x00")
        else:
            raise KeyError(kind)
    return bytes(out) + bytes(scan) + b"\xff\xd9"


def restart_interval(layout, nmcu):
    """the MCUs per interval a decoder takes from the layout's last DRI; 0 where the scan is unbroken"""
    ri = 0
    for e in layout:
        if not isinstance(e, str) and e[0] == "DRI":
            ri = int(e[1])
    return ri if 0 < ri < nmcu else 0


def craft(h, w, sampling, coefs, ids=None, tq=None, td=None, ta=None, qtables=None, huff="optimal", ri=0, pad=1, layout=None, info=False, ends=None):
    """coefs: (blocks, 64) integers, blocks in scan order (MCU by MCU), coefficients in zigzag order, the DC as its value.
    qtables: {id: 64 values in zigzag order}.  huff: a profile of table_for for every table, or {(Tc, Th): profile or
    (counts, vals)} ("optimal" where a key is missing).  ri is written as DRI by the default layout; with a layout of the
    caller's, the layout's last DRI decides where the restart markers go.  info=True: -> (file, the arguments of craft_raw);
    ends: as in encode_scan."""
    hs, vs, nc = SAMPLING[sampling]
    nmcu, comps = geometry(h, w, sampling)
    coefs = np.asarray(coefs).reshape(-1, 64)
    assert len(coefs) == nmcu * len(comps), (len(coefs), nmcu, len(comps))
    ids = list(ids or (1, 2, 3))[:nc]
    tq = list(tq or (0, 0, 0))[:nc]; td = list(td or (0, 0, 0))[:nc]; ta = list(ta or (0, 0, 0))[:nc]
    qtables = dict(qtables or {0: [1] * 64})
    layout = list(layout or default_layout(ri))
    eff = restart_interval(layout, nmcu)
    spec = huff if isinstance(huff, dict) else {}
    tables = {k: table_for(f, spec.get(k, huff if isinstance(huff, str) else "optimal"), dc=k[0] == 0)
              for k, f in symbol_counts(coefs, comps, td, ta, eff).items()}
    for k, t in spec.items():           # tables no component uses may be written too
        if k not in tables and isinstance(t, tuple):
            tables[k] = (list(t[0]), list(t[1]))
    scan = encode_scan(coefs, comps, td, ta, tables, eff, pad, ends)
    samp = [hs << 4 | vs, 0x11, 0x11][:nc]
    kw = dict(h=h, w=w, samp=samp, scan=scan, ids=ids, tq=tq, td=td, ta=ta, qtables=qtables, tables=tables, layout=layout)
    out = craft_raw(**kw)
    return (out, kw) if info else out
