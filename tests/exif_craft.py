"""EXIF blocks built with struct and spliced into the fixtures of tests/golden/jpeg_dec at run time, for test_jpeg_exif_cpu.py and
test_gpu_jpeg_oriented.py.  No file is committed: every variant is a function of a good JPEG, an
orientation and a focal length, and returns the spliced file with the (orientation, focal35) the reader's rules give for it,
known by construction.

Three groups:
  WELL_FORMED  EXIF as cameras write it: both byte orders, the orientation as SHORT and as LONG, the focal tag in the Exif
               sub-IFD and in IFD0, the orientation entry first, last and absent;
  JUNK         EXIF the reader must shrug off: (1, 0) and no error for every one;
  EDGE         files whose oddity is not in the block the reader takes: an XMP APP1 in front, a second Exif APP1 behind, Exif
               after DQT, an entry count clipped to the segment, a sub-IFD pointer past the segment next to a good orientation.
               By the rules the values are the constructed ones, not (1, 0).
orient_map is the table of the issue and of include/openpano_hip.h, restated with index arrays."""
import struct

import numpy as np

SHORT, LONG, ASCII = 3, 4, 2
ORIENTATION, EXIF_IFD, FOCAL35, MAKE = 0x0112, 0x8769, 0xA405, 0x010F
EXIF_ID = b"Exif\x00\x00"


def entry(order, tag, typ, count, value):
    """one 12-byte IFD entry; value: an int (left-justified in the field, as TIFF has it) or 4 raw bytes"""
    e = "<" if order == "II" else ">"
    if isinstance(value, bytes):
        field = value.ljust(4, b"\x00")[:4]
    elif typ == SHORT:
        field = struct.pack(e + "HH", value & 0xFFFF, 0)
    else:
        field = struct.pack(e + "I", value & 0xFFFFFFFF)
    return struct.pack(e + "HHI", tag, typ, count) + field


def tiff(order, ifd0, sub=None, ifd0_at=8, count0=None, magic=42):
    """a TIFF block: header, IFD0 (a list of entries; an entry with value None takes the sub-IFD's offset), the sub-IFD.
    count0 overrides IFD0's entry count, ifd0_at the offset the header names (the IFD itself stays at 8)"""
    e = "<" if order == "II" else ">"
    sub_at = 8 + 2 + 12 * len(ifd0) + 4
    body = b"".join(x if x is not None else entry(order, EXIF_IFD, LONG, 1, sub_at) for x in ifd0)
    out = order.encode() + struct.pack(e + "HI", magic, ifd0_at)
    out += struct.pack(e + "H", len(ifd0) if count0 is None else count0) + body + struct.pack(e + "I", 0)
    if sub is not None:
        out += struct.pack(e + "H", len(sub)) + b"".join(sub) + struct.pack(e + "I", 0)
    return out


def app1(payload):
    return b"\xff\xe1" + struct.pack(">H", len(payload) + 2) + payload


def exif_segment(tiff_block, ident=EXIF_ID):
    return app1(ident + tiff_block)


def _segments(jpg):
    pos = 2; out = []
    while True:
        assert jpg[pos] == 0xFF, pos
        m = jpg[pos + 1]; n = int.from_bytes(jpg[pos + 2: pos + 4], "big")
        out.append((pos, m, n))
        pos += 2 + n
        if m == 0xDA:
            return out


def splice(jpg, segment, after=None):
    """the file with `segment` behind SOI and APP0 (after=None) or behind the first segment with marker `after`"""
    segs = _segments(jpg)
    assert not any(m == 0xE1 for _, m, _ in segs), "the base file has an APP1 of its own"
    if after is None:
        at = 2 + (2 + segs[0][2] if segs[0][1] == 0xE0 else 0)
    else:
        o, _, n = next(s for s in segs if s[1] == after)
        at = o + 2 + n
    return jpg[:at] + segment + jpg[at:]


def _o(order, o, typ=SHORT, count=1):
    return entry(order, ORIENTATION, typ, count, o)


def _f(order, f):
    return entry(order, FOCAL35, SHORT, 1, f)


def _make(order):
    return entry(order, MAKE, ASCII, 4, b"cam\x00")


# name -> f(jpg, o, focal) -> (file, (orientation, focal35) by construction)
WELL_FORMED = {
    "II_short": lambda j, o, f: (splice(j, exif_segment(tiff("II", [_o("II", o)]))), (o, 0)),
    "MM_short": lambda j, o, f: (splice(j, exif_segment(tiff("MM", [_o("MM", o)]))), (o, 0)),
    "II_long": lambda j, o, f: (splice(j, exif_segment(tiff("II", [_o("II", o, LONG)]))), (o, 0)),
    "MM_long": lambda j, o, f: (splice(j, exif_segment(tiff("MM", [_o("MM", o, LONG)]))), (o, 0)),
    "II_focal_sub": lambda j, o, f: (splice(j, exif_segment(tiff("II", [_o("II", o), None], [_f("II", f)]))), (o, f)),
    "MM_focal_sub": lambda j, o, f: (splice(j, exif_segment(tiff("MM", [_o("MM", o), None], [_f("MM", f)]))), (o, f)),
    "II_focal_ifd0": lambda j, o, f: (splice(j, exif_segment(tiff("II", [_o("II", o), _f("II", f)]))), (o, f)),
    "MM_focal_ifd0": lambda j, o, f: (splice(j, exif_segment(tiff("MM", [_o("MM", o), _f("MM", f)]))), (o, f)),
    "focal_sub_wins": lambda j, o, f: (splice(j, exif_segment(tiff("II", [_o("II", o), _f("II", f + 1), None], [_f("II", f)]))), (o, f)),
    "focal_zero": lambda j, o, f: (splice(j, exif_segment(tiff("MM", [_o("MM", o), None], [_f("MM", 0)]))), (o, 0)),
    "orient_first": lambda j, o, f: (splice(j, exif_segment(tiff("MM", [_o("MM", o), _make("MM"), None], [_f("MM", f)]))), (o, f)),
    "orient_last": lambda j, o, f: (splice(j, exif_segment(tiff("II", [_make("II"), None, _o("II", o)], [_make("II"), _f("II", f)]))), (o, f)),
    "orient_absent": lambda j, o, f: (splice(j, exif_segment(tiff("II", [_make("II"), None], [_f("II", f)]))), (1, f)),
    "no_app0": lambda j, o, f: (splice(j[:2] + j[2 + 2 + _segments(j)[0][2]:] if _segments(j)[0][1] == 0xE0 else j,
                                       exif_segment(tiff("II", [_o("II", o)]))), (o, 0)),
}

_PAST = 0x7FF0


def _cut_entry(j, o):
    """an entry count of 200, and the segment ends six bytes into the first entry"""
    t = tiff("II", [_o("II", o)], count0=200)
    return splice(j, exif_segment(t[:8 + 2 + 6]))


JUNK = {
    "bad_exif_id": lambda j, o, f: splice(j, exif_segment(tiff("II", [_o("II", o), _f("II", f)]), b"Exif\x00\x01")),
    "bad_tiff_magic": lambda j, o, f: splice(j, exif_segment(tiff("II", [_o("II", o), _f("II", f)], magic=43))),
    "bad_byte_order": lambda j, o, f: splice(j, exif_segment(b"IM" + tiff("II", [_o("II", o)])[2:])),
    "mixed_byte_order": lambda j, o, f: splice(j, exif_segment(b"MM" + tiff("II", [_o("II", o)])[2:])),
    "ifd_offset_past": lambda j, o, f: splice(j, exif_segment(tiff("MM", [_o("MM", o), _f("MM", f)], ifd0_at=_PAST))),
    "ifd_offset_at_end": lambda j, o, f: splice(j, exif_segment(tiff("II", [_o("II", o)], ifd0_at=len(tiff("II", [_o("II", o)])) - 1))),
    "ifd_offset_huge": lambda j, o, f: splice(j, exif_segment(tiff("II", [_o("II", o)], ifd0_at=0xFFFFFFFF))),
    "count_zero": lambda j, o, f: splice(j, exif_segment(tiff("II", [_o("II", o), _f("II", f)], count0=0))),
    "count_past_truncated_entry": lambda j, o, f: _cut_entry(j, o),
    "sub_pointer_past": lambda j, o, f: splice(j, exif_segment(tiff("II", [entry("II", EXIF_IFD, LONG, 1, _PAST)], [_f("II", f)]))),
    "sub_pointer_short": lambda j, o, f: splice(j, exif_segment(tiff("II", [entry("II", EXIF_IFD, SHORT, 1, 26)], [_f("II", f)]))),
    "orientation_0": lambda j, o, f: splice(j, exif_segment(tiff("II", [_o("II", 0)]))),
    "orientation_9": lambda j, o, f: splice(j, exif_segment(tiff("MM", [_o("MM", 9)]))),
    "orientation_65535": lambda j, o, f: splice(j, exif_segment(tiff("II", [_o("II", 65535)]))),
    "orientation_long_65544": lambda j, o, f: splice(j, exif_segment(tiff("II", [_o("II", 65536 + 8, LONG)]))),
    "orientation_count_2": lambda j, o, f: splice(j, exif_segment(tiff("II", [_o("II", o, SHORT, 2)]))),
    "orientation_ascii": lambda j, o, f: splice(j, exif_segment(tiff("II", [_o("II", o, ASCII)]))),
    "focal_long": lambda j, o, f: splice(j, exif_segment(tiff("II", [entry("II", FOCAL35, LONG, 1, f)]))),
    "exif_too_short": lambda j, o, f: splice(j, app1(EXIF_ID + b"II\x2a\x00\x08\x00\x00")),      # seven bytes behind the identifier
    "empty_app1": lambda j, o, f: splice(j, app1(b"")),
}
for _k in list(JUNK):
    JUNK[_k] = (lambda g: lambda j, o, f: (g(j, o, f), (1, 0)))(JUNK[_k])

XMP = app1(b"http://ns.adobe.com/xap/1.0/\x00<x:xmpmeta xmlns:x='adobe:ns:meta/'><tiff:Orientation>7</tiff:Orientation></x:xmpmeta>")


def _other(o):
    return o % 8 + 1


EDGE = {
    "xmp_in_front": lambda j, o, f: (splice(j, XMP + exif_segment(tiff("II", [_o("II", o)]))), (o, 0)),
    "second_exif_behind": lambda j, o, f: (splice(j, exif_segment(tiff("II", [_o("II", o)])) + exif_segment(tiff("MM", [_o("MM", _other(o)), _f("MM", f)]))), (o, 0)),
    "exif_after_dqt": lambda j, o, f: (splice(j, exif_segment(tiff("MM", [_o("MM", o), _f("MM", f)])), after=0xDB), (o, f)),
    "count_clipped": lambda j, o, f: (splice(j, exif_segment(tiff("II", [_o("II", o)], count0=0xFFFF))), (o, 0)),
    "orientation_and_sub_pointer_past": lambda j, o, f: (splice(j, exif_segment(tiff("II", [_o("II", o), entry("II", EXIF_IFD, LONG, 1, _PAST)], [_f("II", f)]))), (o, 0)),
}

ALL = {**WELL_FORMED, **JUNK, **EDGE}


def with_orientation(jpg, o, order="II"):
    """the plainest file that carries orientation o"""
    return splice(jpg, exif_segment(tiff(order, [_o(order, o)])))


def orient_map(s, o):
    """view of the stored frame s (h, w, 3) under EXIF orientation o: the table of op_views_decode_jpeg_oriented, index by index"""
    h, w = s.shape[:2]
    y, x = np.mgrid[0:h, 0:w] if o < 5 else np.mgrid[0:w, 0:h]
    sy, sx = {1: (y, x), 2: (y, w - 1 - x), 3: (h - 1 - y, w - 1 - x), 4: (h - 1 - y, x),
              5: (x, y), 6: (h - 1 - x, y), 7: (h - 1 - x, w - 1 - y), 8: (x, w - 1 - y)}[o]
    return np.ascontiguousarray(s[sy, sx])
