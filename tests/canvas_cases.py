"""Canvases, sources and numpy models shared by the tests of the canvas stage (csrc/canvas.hip): the crop to the largest valid
rectangle (k_crop_heights / k_crop_lines / k_crop_pick), the byte quantisation (k_to_u8, canvas_byte) and the cylinder pre-warp
(k_cyl_project and its trig-table cache).  test_canvas_cases_cpu.py proves that the cases are what they claim and that oracle,
reference and the models here agree on them; test_gpu_canvas.py holds the device to the oracle on the same cases.  No tests here.

A canvas with chosen content comes from a one-view flat blend through the identity (there is no upload-a-canvas entry point):
the canvas has the view's shape, canvas pixel (i, j) is valid where the view's pixels (i..i+1, j..j+1) all are, column 0, the
last column and the last row are invalid, and the colours are the view's to within one ulp.  Invalid canvas regions are
therefore unions of 2 x 2 squares: a "one-column notch" of a family below is two columns wide, and what a search meets first is
still the column the family names.  Every family's claim is checked on the canvas mask itself, never on the view."""
import collections
import zlib

import numpy as np

from openpano_amd.config import PanoConfig

F = np.float32
CHUNK, THREADS = 64, 256            # CROP_CHUNK and the block size of k_crop_lines / k_crop_pick / k_to_u8
CROP_LDS_MAX = 150 * 1024           # op_canvas_crop refuses above this many bytes of dynamic LDS
HOMO = np.eye(3)[None]


def blend_cfg():
    return PanoConfig(ESTIMATE_CAMERA=0, TRANS=1, ORDERED_INPUT=1, LAZY_READ=0, MULTIBAND=0, MAX_OUTPUT_SIZE=40000)


def crop_lds_bytes(w):
    """dynamic LDS of k_crop_lines: the line's w heights and the minima of its 64-column chunks"""
    return 4 * (w + -(-w // CHUNK))


MAX_CROP_WIDTH = 37809
assert crop_lds_bytes(MAX_CROP_WIDTH) == CROP_LDS_MAX and crop_lds_bytes(MAX_CROP_WIDTH + 1) > CROP_LDS_MAX     # 37809 + 591 = 38400 ints


# ---- the models ------------------------------------------------------------------------------------------------------------

def heights_of(mask):
    """height[line][k]: the number of consecutive valid pixels of column k that end at (line, k)"""
    out = np.zeros(mask.shape, np.int64)
    run = np.zeros(mask.shape[1], np.int64)
    for line in range(mask.shape[0]):
        run = np.where(mask[line], run + 1, 0)
        out[line] = run
    return out


def line_extents(hs):
    """per column k of one line of heights: the first and last column of the longest run around k on which height >= hs[k]
    (left = right = k where hs[k] == 0, which no caller looks at).  From the definition: per distinct height v the runs of
    ``hs >= v`` are found once, and every column of height v takes the run it lies in."""
    hs = np.asarray(hs)
    w = len(hs)
    left, right = np.arange(w), np.arange(w)
    for v in np.unique(hs[hs > 0]):
        ge = np.concatenate([[False], hs >= v, [False]])
        edge = np.flatnonzero(ge[1:] != ge[:-1])            # run r covers columns edge[2r] .. edge[2r + 1] - 1
        start, stop = edge[0::2], edge[1::2]
        at = np.flatnonzero(hs == v)
        run = np.searchsorted(start, at, side="right") - 1
        left[at], right[at] = start[run], stop[run] - 1
    return left, right


def crop_model(mask):
    """crop() of the reference (lib/imgproc.cc:200-235) on a validity mask -> (x0, y0, w, h, n_ties).  Every (line, k) with
    height hk > 0 is a candidate: the rectangle of height hk over the extent of k; the winner is the first strictly greater
    area in (line, k) order; n_ties counts the other candidates that reach the winning area with another rectangle.
    Nothing valid: the reference's 0 x 1 answer, (0, 1, 1, 0, 0)."""
    height = heights_of(mask)
    cands = []                                              # (area, line, k, left, right, hk) of every line's candidates
    for line in range(mask.shape[0]):
        hs = height[line]
        k = np.flatnonzero(hs > 0)
        if len(k) == 0:
            continue
        left, right = line_extents(hs)
        area = (right[k] - left[k] + 1) * hs[k]
        cands.append(np.stack([area, np.full(len(k), line), k, left[k], right[k], hs[k]], axis=1))
    if not cands:
        return 0, 1, 1, 0, 0
    c = np.concatenate(cands)                               # already in (line, k) order
    best = c[:, 0].max()
    tie = c[c[:, 0] == best]
    _, line, _, left, right, hk = tie[0]
    rect = (int(left), int(line - hk + 1), int(right - left + 1), int(hk))
    same = (tie[:, 3] == left) & (tie[:, 4] == right) & (tie[:, 1] == line) & (tie[:, 5] == hk)
    return rect + (int((~same).sum()),)


def byte_model(canvas):
    """write_rgb's quantisation (lib/imgio.cc:98-113): Color::NO -> white, fl32(v * 255) truncated"""
    v = np.asarray(canvas, F)
    return (np.where(v < 0, F(1), v) * F(255)).astype(np.uint8)


# ---- crop cases ------------------------------------------------------------------------------------------------------------

CropCase = collections.namedtuple("CropCase", "id family vmask info")       # vmask: validity of the VIEW's pixels


def _seed(name):
    return zlib.crc32(name.encode())


def view_mask_for(want):
    """the view mask whose canvas mask is ``want`` closed by the 2 x 2 square: a view pixel is valid where any wanted canvas
    pixel reads it"""
    v = want.copy()
    v[:, 1:] |= want[:, :-1]
    v[1:, :] |= want[:-1, :]
    v[1:, 1:] |= want[:-1, :-1]
    return v


def view_of(case):
    """the fp32 view of a crop case: seeded colours in [0, 1), Color::NO where the view mask is false"""
    v = np.random.default_rng(_seed(case.id)).random(case.vmask.shape + (3,), dtype=F)
    v[~case.vmask] = -1
    return v


def canvas_mask(canvas):
    return canvas[..., 0] >= 0


def _framed(h, w):
    """everything a canvas of this shape can hold: all but column 0, the last column and the last row"""
    m = np.zeros((h, w), bool)
    m[:-1, 1:-1] = True
    return m


def _case(name, family, want, **info):
    return CropCase(name, family, view_mask_for(want & _framed(*want.shape)), info)


def _from_heights(heights, rows):
    """a canvas mask of ``rows`` lines (+ the invalid last one) whose columns stand on line rows - 1 with these heights"""
    heights = np.asarray(heights)
    m = np.zeros((rows + 1, len(heights)), bool)
    m[:rows] = np.arange(rows)[:, None] >= rows - heights[None, :]
    return m


# A. everything valid.  At W = 65, 129, 257 and 513 the last chunk is the invalid last column alone, so the winner cannot span
# every chunk there: 257 and 513 are widths of families B to E, 65 and 129 of family F.
A_WIDTHS = (63, 64, 66, 128, 255, 256, 258, 1030)
FAMILY_A = [_case("A_full_w%d" % w, "A", _framed(7, w)) for w in A_WIDTHS]


# B. a plateau of seven lines; the notch columns stand one line high.  side "start": the notch is columns (p - 1, p) and the
# winner starts at p + 1, every search from the right of it meets p first; side "end": columns (p, p + 1), the winner ends at
# p - 1.  The longer side wins, and 64 columns fit left of the notch only from p = 65 on.
def _notch(p, side, w):
    m = _framed(8, w)
    lo = p - 1 if side == "start" else p
    m[:6, lo: lo + 2] = False
    return _case("B_notch_p%d_%s_w%d" % (p, side, w), "B", m, p=p, side=side)


FAMILY_B = ([_notch(p, "start", 513) for p in (63, 64, 65, 127, 128, 129)] + [_notch(p, "start", 257) for p in (63, 64, 65)]
            + [_notch(p, "end", 192) for p in (127, 128, 129)] + [_notch(129, "end", 255)])


# C. staircases: column blocks whose heights rise strictly and then fall strictly, over the whole width
def _staircase(name, w, widths):
    widths = list(widths)
    if len(widths) % 2 == 0:                                # an odd number of steps: 1, 2, .., peak, .., 2, 1
        widths[-2:] = [widths[-2] + widths[-1]]
    n = len(widths)
    up = (n + 1) // 2
    level = np.concatenate([np.arange(1, up + 1), np.arange(up - 1, 0, -1)])
    heights = np.zeros(w, np.int64)
    heights[1: 1 + int(np.sum(widths))] = np.repeat(level, widths)
    return _case(name, "C", _from_heights(heights, int(level.max())), steps=n)


def _random_widths(seed, w):
    rng = np.random.default_rng(seed)
    out = []
    while sum(out) < w - 2:
        out.append(int(rng.integers(1, 41)))
    out[-1] -= sum(out) - (w - 2)
    return [x for x in out if x > 0]


FAMILY_C = ([_staircase("C_stairs_w%d_step%d" % (w, s), w, [s] * (((w - 2) // s - 1) | 1)) for w, s in ((258, 7), (513, 7), (513, 23), (1030, 23), (1030, 61))]
            + [_staircase("C_stairs_w%d_seed%d" % (w, s), w, _random_widths(s, w)) for w, s in ((258, 1), (513, 2), (513, 3), (1030, 4))])


# D. two rectangles of equal area on one line; k1 < k2 are the first columns that reach it, the winner is k1's
def _two_rects(name, w, a, b, **info):
    """a, b: (first column, columns, lines) of two rectangles standing on line 11"""
    heights = np.zeros(w, np.int64)
    for x, cols, lines in (a, b):
        heights[x: x + cols] = lines
    return _case(name, "D", _from_heights(heights, 12), k1=min(a[0], b[0]), k2=max(a[0], b[0]), **info)


def _stairs_tie(name, w, x, heights):
    """a falling staircase whose last two steps tie: k1 is the one-column step, k2 = k1 + 1 the first column of the lowest"""
    hs = np.zeros(w, np.int64)
    hs[x: x + len(heights)] = heights
    k1 = x + int(np.flatnonzero(np.diff(heights) < 0)[0]) + 1
    return _case(name, "D", _from_heights(hs, 12), k1=k1, k2=k1 + 1, overlap=True)


TALL, WIDE = (10, 12), (20, 6)          # (columns, lines): 120 pixels each
FAMILY_D = [
    _two_rects("D_same_thread_tall_first", 513, (5,) + TALL, (261,) + WIDE),
    _two_rects("D_same_thread_wide_first", 513, (5,) + WIDE, (261,) + TALL),
    _two_rects("D_later_at_lower_tid_tall_first", 513, (100,) + TALL, (256,) + WIDE),
    _two_rects("D_later_at_lower_tid_wide_first", 513, (100,) + WIDE, (256,) + TALL),
    _two_rects("D_later_at_lower_tid_w1030", 1030, (300,) + TALL, (768,) + WIDE),
    _stairs_tie("D_adjacent", 258, 20, [10, 10, 10, 8, 4, 4, 4, 4]),            # 4 x 8 = 8 x 4 = 32 > 3 x 10
    _stairs_tie("D_adjacent_across_256", 513, 251, [7, 7, 7, 7, 6, 3, 3, 3, 3, 3]),  # 5 x 6 = 10 x 3 = 30 > 4 x 7; k1 = 255, k2 = 256
]


# E. two rectangles of equal area that end on different lines; the winner is the one that ends first, wherever its columns are
def _two_lines(name, h, w, first, second):
    """first, second: (last line, first column, columns, lines); first ends on the earlier line"""
    m = np.zeros((h, w), bool)
    for line, x, cols, lines in (first, second):
        m[line - lines + 1: line + 1, x: x + cols] = True
    return _case(name, "E", m, line1=first[0], line2=second[0], x1=first[1])


FAMILY_E = [_two_lines("E_lines_5_11_w258", 13, 258, (5, 100, 20, 6), (11, 10, 12, 10)),
            _two_lines("E_lines_5_11_w513", 13, 513, (5, 300, 20, 6), (11, 200, 12, 10))]
for _l1, _l2 in ((100, 101), (255, 256), (100, 356)):      # neighbouring threads, threads 255 and 0, one thread of k_crop_pick
    FAMILY_E += [_two_lines("E_lines_%d_%d_later_left" % (_l1, _l2), 600, 40, (_l1, 20, 12, 10), (_l2, 2, 15, 8)),
                 _two_lines("E_lines_%d_%d_later_right" % (_l1, _l2), 600, 40, (_l1, 2, 12, 10), (_l2, 20, 15, 8))]


# F. blend-like canvases: a valid interior with Color::NO borders and holes, 40 lines; the two narrow widths have a last chunk of
# one column
def _holey(seed, h, w):
    rng = np.random.default_rng(seed)
    m = np.ones((h, w), bool)
    m[: rng.integers(0, 5)] = False; m[h - rng.integers(1, 5):] = False
    m[:, : rng.integers(1, 12)] = False; m[:, w - rng.integers(3, 15):] = False
    for _ in range(w // 50):
        y, x = rng.integers(0, h), rng.integers(0, w)
        m[y: y + rng.integers(1, 10), x: x + rng.integers(1, 14)] = False
    return m


FAMILY_F = ([_case("F_holes_w%d_seed%d" % (w, s), "F", _holey(10 * w + s, 40, w)) for w in (300, 700) for s in range(4)]
            + [_case("F_holes_w%d_seed%d" % (w, s), "F", _holey(10 * w + s, 40, w)) for w in (65, 129) for s in range(2)])


# G. degenerate canvases.  A view of two columns leaves no canvas pixel valid; one of three columns leaves column 1, so the
# W = 3 canvas without a valid pixel comes from a view without one.
def _pixels(name, h, w, rows, cols, **info):
    m = np.zeros((h, w), bool)
    m[rows, cols] = True
    return _case(name, "G", m, **info)


FAMILY_G = [_pixels("G_one_pixel", 5, 6, 2, 3, shape=(1, 1)), _pixels("G_one_row", 5, 70, 2, slice(None), shape=(1, 68)),
            _pixels("G_one_column", 6, 7, slice(None), 3, shape=(5, 1)),
            CropCase("G_w3_full_view", "G", np.ones((5, 3), bool), dict(shape=(4, 1))),
            CropCase("G_w2_full_view", "G", np.ones((5, 2), bool), dict(shape=(0, 1))),
            CropCase("G_w3_no_view_pixel", "G", np.zeros((5, 3), bool), dict(shape=(0, 1)))]


# H. three lines, one invalid view pixel at (0, W / 3): two lines right of it beat one line of the whole width.  16500 needs
# 67 032 B of dynamic LDS (above the 64 KiB a kernel gets unasked), 37809 is the widest canvas crop accepts, 37810 is refused.
def _wide(w):
    v = np.ones((3, w), bool)
    v[0, w // 3] = False
    return CropCase("H_wide_w%d" % w, "H", v, dict(w=w))


WIDE_LDS, WIDE_MAX, WIDE_REFUSED = _wide(16500), _wide(MAX_CROP_WIDTH), _wide(MAX_CROP_WIDTH + 1)
assert 64 * 1024 < crop_lds_bytes(16500) == 67032
FAMILY_H = [WIDE_LDS, WIDE_MAX, WIDE_REFUSED]

CROP_SMALL = FAMILY_A + FAMILY_B + FAMILY_C + FAMILY_D + FAMILY_E + FAMILY_F + FAMILY_G        # A-G
CROP_CASES = CROP_SMALL + FAMILY_H


def chunks_spanned(x0, w, width):
    """does the rectangle's extent reach every 64-column chunk of a line of this width?"""
    return x0 < CHUNK and (x0 + w - 1) // CHUNK == (width - 1) // CHUNK


def far_extents(mask):
    """(columns of the last valid line whose left extent lies in another chunk than their own, the same for the right extent)"""
    height = heights_of(mask)
    line = int(np.flatnonzero(mask.any(axis=1))[-1])
    hs = height[line]
    left, right = line_extents(hs)
    k = np.flatnonzero(hs > 0)
    return int((left[k] // CHUNK != k // CHUNK).sum()), int((right[k] // CHUNK != k // CHUNK).sum())


def check_family(case, mask):
    """the precondition of a case's family on a canvas mask (the oracle's here, the device's in test_gpu_canvas.py)"""
    x0, y0, w, h, n_ties = crop_model(mask)
    width = mask.shape[1]
    f, info = case.family, case.info
    if f == "A":            # the chunk-minimum skip of every thread runs through every chunk
        assert mask[:-1, 1:-1].all() and not mask[-1].any() and not mask[:, 0].any() and not mask[:, -1].any()
        assert (w, h) == (width - 2, mask.shape[0] - 1) and chunks_spanned(x0, w, width)
    elif f == "B":          # the winner's extent stops at the notch column p, which sits on or next to a chunk boundary
        p = info["p"]
        assert p % CHUNK in (CHUNK - 1, 0, 1) and width >= 192 and w >= CHUNK
        assert (x0 == p + 1) if info["side"] == "start" else (x0 + w - 1 == p - 1)
        assert not mask[y0, p] and mask[y0 + h - 1, p]              # a shorter column, not an empty one
    elif f == "C":          # both searches leave the column's own chunk for at least a quarter of the columns
        hs = heights_of(mask)[mask.shape[0] - 2]
        steps = hs[np.flatnonzero(np.diff(hs))]
        peak = int(np.argmax(steps))
        assert (np.diff(steps[: peak + 1]) > 0).all() and (np.diff(steps[peak:]) < 0).all() and len(steps) >= 11
        far_left, far_right = far_extents(mask)
        assert far_left >= width / 4 and far_right >= width / 4, (far_left, far_right)
    elif f == "D":          # two candidates of one line tie, the earlier column's rectangle wins
        k1, k2 = info["k1"], info["k2"]
        hs = heights_of(mask)[mask.shape[0] - 2]
        left, right = line_extents(hs)
        area = (right - left + 1) * hs
        assert n_ties >= 1 and area[k1] == area[k2] == area.max() == w * h and hs[k1] != hs[k2]
        assert np.flatnonzero(area == area.max())[0] == k1 and np.flatnonzero((area == area.max()) & (hs == hs[k2]))[0] == k2
        assert (x0, w, h) == (left[k1], right[k1] - left[k1] + 1, hs[k1]) and y0 + h - 1 == mask.shape[0] - 2
        assert info.get("overlap") or right[k1] < left[k2]
    elif f == "E":          # two candidates on different lines tie, the earlier line's rectangle wins
        l1, l2 = info["line1"], info["line2"]
        assert n_ties >= 1 and l1 < l2 and y0 + h - 1 == l1 and x0 == info["x1"]
        best2 = max((r - l + 1) * v for l, r, v in zip(*line_extents(heights_of(mask)[l2]), heights_of(mask)[l2]))
        assert best2 == w * h
    elif f == "F":
        assert w * h >= 0.1 * mask.size and not mask.all()
    elif f == "G":
        assert (h, w) == info["shape"] and mask.sum() == h * w
    elif f == "H":
        assert width == info["w"] and mask.shape[0] == 3 and w > width // 2 and h == 2
    else:
        raise AssertionError(f)
    return x0, y0, w, h


# ---- byte cases ------------------------------------------------------------------------------------------------------------

def byte_values():
    """k / 255 in fp32 for every byte k, its neighbours one and two ulps either side (clipped to [0, 1]), 0, 1 and the smallest
    denormal"""
    base = (np.arange(256, dtype=np.float64) / 255).astype(F)
    out = [base]
    for step in (1, 2):
        lo, hi = base, base
        for _ in range(step):
            lo, hi = np.nextafter(lo, F(-1)), np.nextafter(hi, F(2))
        out += [lo, hi]
    vals = np.clip(np.concatenate(out), 0, 1).astype(F)
    return np.concatenate([vals, np.array([0, 1, np.nextafter(F(0), F(1))], F)])


def _byte_fill(n, seed):
    vals = byte_values()
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.permutation(vals) for _ in range(-(-n // len(vals)))])[:n]


def byte_view():
    """20 x 82: lines 0..15, columns 1..80 hold every value of byte_values() (three times, each in another order), line 16 and
    the border columns more of them, lines 17..19 are Color::NO"""
    v = _byte_fill(20 * 82 * 3, 5).reshape(20, 82, 3).copy()
    v[:16, 1:81] = _byte_fill(16 * 80 * 3, 6).reshape(16, 80, 3)
    v[17:] = -1
    return v


# crops whose element count h * w * 3 (always a multiple of 3) sits around the 256-thread block of k_to_u8: 3, 255 (one short
# of a block), 258 (two into the second), 513 = 2 * 256 + 1, 768 = 3 * 256 and 1281 = 5 * 256 + 1
COUNT_SHAPES = [(1, 1), (5, 17), (2, 43), (9, 19), (16, 16), (7, 61)]
assert [h * w * 3 for h, w in COUNT_SHAPES] == [3, 255, 258, 513, 768, 1281]


def count_view(h, w):
    """an all-valid view whose canvas crops to h x w, filled from byte_values()"""
    return _byte_fill((h + 1) * (w + 2) * 3, 100 * h + w).reshape(h + 1, w + 2, 3).copy()


def on_integer(v):
    """(fl32(v * 255) is an integer, it is the float one ulp below an integer) for canvas values v in [0, 1]"""
    p = np.asarray(v, F) * F(255)
    up = np.nextafter(p, F(1000))
    return p == np.floor(p), (p != np.floor(p)) & (up == np.floor(up))


# ---- cylinder cases --------------------------------------------------------------------------------------------------------

CYL_SHAPES = [(3, 3), (9, 5), (5, 90), (64, 64), (67, 130), (40, 260)]
CYL_FACTORS = (0.5, 1.0, 1.3)
CYL_FOCALS = (12, 24, 37, 60)
CYL_CASES = [(h, w, hf, fl) for h, w in CYL_SHAPES for hf in CYL_FACTORS for fl in CYL_FOCALS]
CYL_EMPTY = (2, 2, 1.0, 37)             # output width 0
# two focal lengths that give a 67 x 130 image the same output width and another radius (found by search over
# hip.cyl_warp_shape; test_canvas_cases_cpu.py asserts the property): the trig table of one must not serve the other
CACHE_PAIR = (67, 130, 1.0, 59, 60)


def cyl_cfg(focal):
    return PanoConfig(FOCAL_LENGTH=focal)


def cyl_image(h, w):
    return np.random.default_rng(1000 * h + w).random((h, w, 3), dtype=F)


def cyl_bytes(h, w):
    return np.random.default_rng(1000 * h + w + 1).integers(0, 256, (h, w, 3), dtype=np.uint8)


def cyl_holes(h, w):
    """the fp32 image with a block of Color::NO in it"""
    img = cyl_image(h, w)
    img[h // 3: h // 3 + max(1, h // 4), w // 3: w // 3 + max(1, w // 4)] = -1
    return img


def twin(u8):
    """the fp32 image read_img makes of decoder bytes (lib/imgio.cc:54-56)"""
    return (u8.astype(np.float64) / 255.0).astype(F)
