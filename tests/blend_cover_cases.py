"""The blend's image-cover walk (csrc/blend_sample.hpp: tile_cover / walk_cover) past 64, 256 and 4096 views: scenes, the
case table and a numpy model of the walk.  Shared by test_blend_cover_cases_cpu.py (the claims of every case, oracle ==
reference, the model against one-line slips) and test_gpu_blend_cover.py (HIP == oracle on every case).  No GPU import.

A 64 x 4 pixel workgroup marks the images whose ROI meets its tile -- one image per lane, one 64-bit ballot word per 64
images, 256 images per pass of the marking loop, COVER_WORDS * 64 = 4096 images per round -- and every pixel then walks the
marked images in ascending index order with the exact per-pixel test.  The fp32 sums of the reference run in image order and
its multiband winner is the first image with the strictly largest weight, so the order is part of the result.

Scenes.  grid_scene: small views on a regular pitch, integer translations (ROI exactly (w + 1) x (h + 1) at (L, T)), the
list order permuted so that the images over one pixel have indices scattered over words, passes and rounds, a distinct
exposure factor per view so that a change of order changes the fp32 sums, and pairs of list positions that share one
placement (equal weights everywhere: the multiband winner must be the lower index).  SEAMS: flat scenes of 6 views whose ROI
borders fall at, one short of and one past the tile boundaries."""
import functools

import numpy as np

from openpano_amd.config import PanoConfig

COVER_WORDS = 64
ROUND = COVER_WORDS * 64          # images per round
PASS = 256                        # images per pass of the marking loop (one per thread)
TILE_W, TILE_H = 64, 4


def _cfg(**kv):
    base = dict(ESTIMATE_CAMERA=0, TRANS=1, ORDERED_INPUT=1, LAZY_READ=0, MULTIBAND=0)
    base.update(kv)
    return PanoConfig(**base)


# the blend modes of the table; mb3: k_mb_first_fused + k_mb_blur_fused<6,true> + k_mb_bands<2>; mb7: k_mb_accumulate, and
# n in gridDim.y of six fused blur launches
MODES = {
    "linear": _cfg(ESTIMATE_CAMERA=1, TRANS=0, ORDERED_INPUT=0),     # the config refuses ORDERED_INPUT 0 in any other mode
    "ordered": _cfg(),
    "lazy": _cfg(LAZY_READ=1),
    "mb3": _cfg(MULTIBAND=3),
    "mb7": _cfg(MULTIBAND=7),
}
SMALL_MODES = ("linear", "ordered", "lazy", "mb3", "mb7")
LARGE_MODES = ("linear", "lazy", "mb3")        # from 4096 views up: the oracle stays within a few seconds per case

VIEW_W, VIEW_H, PITCH = 12, 10, 5
# n -> (columns of the grid, pairs of list positions (a, b) that share a's placement, the branch the count is there for)
GRID = {
    64: (16, ((3, 40),), "one full word: the pair sits in its lo and hi halves"),
    65: (16, ((3, 64),), "one image in the second word (s_cover[1], the loop bound padded to whole waves)"),
    128: (16, ((3, 70),), "two full words"),
    129: (16, ((3, 70), (5, 128)), "one image in the third word"),
    256: (16, ((3, 70), (5, 200)), "one full pass of the marking loop"),
    257: (16, ((3, 70), (5, 256)), "the second pass of the marking loop (k += 256), one image in it"),
    4096: (66, ((3, 70), (5, 4000)), "exactly one full round: n - k0 < 4096 is false, k1 = k0 + 4096"),
    4097: (66, ((3, 70), (5, 4096)), "a second round of one image, the accumulators carried into it"),
    4200: (66, ((3, 70), (5, 4099), (4097, 4170)), "a second round of more than one word"),
}


def _world(seed, h, w):
    return (np.random.default_rng(seed).random((h, w, 3), dtype=np.float32) * np.float32(0.8) + np.float32(0.1)).astype(np.float32)


def _homo(L, T, w, h):
    return np.array([[1.0, 0, L + w / 2], [0, 1.0, T + h / 2], [0, 0, 1.0]])


def grid_scene(n, w=VIEW_W, h=VIEW_H, pitch=PITCH, cols=16, seed=0, dups=()):
    """n views of w x h on a grid of `cols` columns and `pitch` pixels, list position p showing grid cell order[p] of a
    seeded permutation; for (a, b) in dups, position b is placed on a's cell (its contents stay those of its own cell).
    Every view is scaled by its own exposure factor in [0.7, 1].  -> (views, homos (n, 3, 3), identity_idx): the identity
    view is the one on cell 0, at the origin of the canvas."""
    rng = np.random.default_rng(seed)
    order = rng.permutation(n)
    expo = (0.7 + 0.3 * rng.permutation(n) / max(n - 1, 1)).astype(np.float32)
    cell = order.copy()
    for a, b in dups:
        cell[b] = cell[a]
    identity_idx = int(np.flatnonzero(order == 0)[0])
    assert all(b != identity_idx for _, b in dups) and cell[identity_idx] == 0
    rows = -(-n // cols)
    world = _world(seed + 1000, (rows - 1) * pitch + h, (cols - 1) * pitch + w)
    views, homos = [], []
    for p in range(n):
        sl, st = int(order[p] % cols) * pitch, int(order[p] // cols) * pitch
        L, T = int(cell[p] % cols) * pitch, int(cell[p] // cols) * pitch
        views.append(np.ascontiguousarray(world[st:st + h, sl:sl + w] * expo[p], np.float32))
        homos.append(_homo(L, T, w, h))
    return views, np.stack(homos), identity_idx


def flat_views(specs, seed):
    """views of one world placed by integer translation: spec (L, T, w, h) -> ROI (L, T, L + w, T + h); view 0 is the
    identity view and sits at the origin"""
    assert specs[0][:2] == (0, 0)
    W = max(L + w for L, T, w, h in specs); H = max(T + h for L, T, w, h in specs)
    world = _world(seed, H, W)
    expo = np.linspace(1.0, 0.75, len(specs)).astype(np.float32)
    views = [np.ascontiguousarray(world[T:T + h, L:L + w] * expo[k], np.float32) for k, (L, T, w, h) in enumerate(specs)]
    return views, np.stack([_homo(*s) for s in specs]), 0


# name -> (specs (L, T, w, h), the ROI coordinates the scene is there for: axis -> values that must occur)
SEAMS = {
    # x0 at the last column of a tile, the first of the next and one past, for the first and the second boundary
    "x0": ([(0, 0, 150, 14), (63, 0, 9, 9), (64, 1, 9, 9), (65, 2, 9, 9), (127, 3, 9, 9), (128, 4, 9, 9)],
           {"x0": (63, 64, 65, 127, 128)}),
    # x1 one short of, at and one past j0 = 64; the views (52 ..) and (60 ..) are one tile column wide as far as the tile
    # starting at 64 sees them (x1 == j0): under LAZY_READ that tile must skip them and column 63 must still get them
    "x1": ([(0, 0, 150, 14), (50, 0, 13, 9), (52, 1, 12, 9), (40, 2, 25, 9), (60, 3, 4, 9), (120, 4, 8, 9)],
           {"x1": (63, 64, 65, 128)}),
    "y0": ([(0, 0, 80, 16), (5, 3, 12, 6), (19, 4, 12, 6), (33, 5, 12, 6), (47, 7, 12, 6), (61, 8, 12, 6)],
           {"y0": (3, 4, 5, 7, 8)}),
    "y1": ([(0, 0, 80, 16), (5, 1, 12, 2), (19, 1, 12, 3), (33, 2, 12, 3), (47, 3, 12, 4), (61, 4, 12, 4)],
           {"y1": (3, 4, 5, 7, 8)}),
}
SEAM_MODES = ("ordered", "lazy", "mb3")


class Case:
    """one blend call: scene() -> (views as the device takes them, their fp32 twins for the oracle, homos, identity_idx),
    the config, the gain arguments of hip.blend / Oracle.blend, and what it is there for"""

    def __init__(self, name, scene_key, mode, why, gains=None):
        self.name, self.scene_key, self.mode, self.why, self.gains = name, scene_key, mode, why, gains
        self.cfg = MODES[mode]

    def scene(self):
        return scene(self.scene_key)

    def gain_args(self):
        return {} if self.gains is None else self.gains(len(self.scene()[0]))


@functools.lru_cache(maxsize=None)
def scene(key):
    """-> (views, fp32 twins, homos, identity_idx); key: ("grid", n), ("seam", name), ("mixed", n) or ("overlap", n)"""
    kind, arg = key
    if kind == "seam":
        views, homos, idx = flat_views(SEAMS[arg][0], seed=41)
        return views, views, homos, idx
    if kind == "overlap":
        views, homos, idx = grid_scene(arg, cols=16, seed=arg)
        return views, views, homos, idx
    cols, dups, _ = GRID[arg]
    views, homos, idx = grid_scene(arg, cols=cols, seed=arg, dups=dups)
    if kind == "mixed":           # every other view as decoder bytes; the oracle reads what read_img makes of them
        dev = [np.clip(np.rint(v * 255.0), 0, 255).astype(np.uint8) if k % 2 else v for k, v in enumerate(views)]
        twins = [(v.astype(np.float64) / 255.0).astype(np.float32) if v.dtype == np.uint8 else v for v in dev]
        return dev, twins, homos, idx
    return views, views, homos, idx


OVERLAP_N = 300


def overlap_scene():
    """the permuted grid at 300 views for the overlap statistics (csrc/overlap.hip: overlap_walk): the second pass of its
    own marking loop (n > 256), a lattice tile met by far more images than one chunk of the walk holds, and overlapping pairs
    (a, b) with a and b far apart.  -> (views, homos, identity_idx)"""
    views, _, homos, idx = scene(("overlap", OVERLAP_N))
    return views, homos, idx


def pair_arrays(n):
    """(a, b) of every pair in the order of op_gain_overlap's arrays (hip.pair_index)"""
    return np.triu_indices(n, 1)


def _image_gains(n):
    """per-image gains in [0.6, 1.6]: bright samples clamp; two rows exactly 1"""
    G = np.random.default_rng(n).uniform(0.6, 1.6, (n, 3)).astype(np.float32)
    G[1] = 1.0; G[n - 1] = 1.0
    return dict(gains=G)


def _vignette(n):
    g = _image_gains(n)["gains"]
    return dict(gains=g, vignette=np.array((-0.5, 0.4, -0.2), np.float32))


def _block_gains(n):
    M = np.random.default_rng(n + 7).uniform(0.6, 1.6, (n, 2, 2, 3)).astype(np.float32)
    M[1] = 1.0
    return dict(gains=M)


def _build_cases():
    out = []
    for n, (_, _, why) in GRID.items():
        for mode in (SMALL_MODES if n <= 257 else LARGE_MODES):
            out.append(Case("grid%d-%s" % (n, mode), ("grid", n), mode, why))
    for name in SEAMS:
        for mode in SEAM_MODES:
            out.append(Case("seam_%s-%s" % (name, mode), ("seam", name), mode, "ROI borders around the tile boundaries: %s" % (SEAMS[name][1],)))
    for mode in ("linear", "mb3"):
        out.append(Case("gains4200-%s" % mode, ("grid", 4200), mode, "per-image gains at gains + 3 k, k up to 4199", _image_gains))
        out.append(Case("vignette257-%s" % mode, ("grid", 257), mode, "the curve at gains + 3 n behind 257 gain rows", _vignette))
        out.append(Case("block257-%s" % mode, ("grid", 257), mode, "2 x 2 block gains at gains + 3 k bx by", _block_gains))
        out.append(Case("mixed129-%s" % mode, ("mixed", 129), mode, "uint8 and fp32 views alternating along the walk (the U8 instances)"))
    return out


CASES = _build_cases()
CASE = {c.name: c for c in CASES}


def rois(meta):
    """the inclusive canvas ROI (x0, y0, x1, y1) of every image (Coor truncation, stitcher_image.cc:123-129), (n, 4) int"""
    minx, miny, _, _, resx, resy = meta["geom"]
    r = np.asarray(meta["ranges"], np.float64)
    return np.stack([((r[:, 0] - minx) / resx).astype(np.int64), ((r[:, 1] - miny) / resy).astype(np.int64),
                     ((r[:, 2] - minx) / resx).astype(np.int64), ((r[:, 3] - miny) / resy).astype(np.int64)], axis=1)


def _clip(r, H, W, excl):
    """the pixels of ROI r that pass the per-pixel test inside an H x W extent, as (y slice, x slice); None when empty"""
    x0, y0, x1, y1 = (int(v) for v in r)
    xa, xb, ya, yb = max(x0, 0), min(x1 - excl, W - 1), max(y0, 0), min(y1 - excl, H - 1)
    if xb < xa or yb < ya:
        return None
    return slice(ya, yb + 1), slice(xa, xb + 1)


def cover_spans(R, H, W, lazy=0):
    """per pixel of the H x W canvas: how many images pass the per-pixel test, and the lowest and highest index among them.
    -> dict(count, covered, words, passes, rounds): the numbers of covered pixels, and of pixels whose covering images lie in
    different 64-image words, different 256-image passes and different 4096-image rounds"""
    cnt = np.zeros((H, W), np.int32); lo = np.full((H, W), 1 << 30, np.int64); hi = np.full((H, W), -1, np.int64)
    for k, r in enumerate(R):
        s = _clip(r, H, W, 1 if lazy else 0)
        if s is None:
            continue
        cnt[s] += 1; lo[s] = np.minimum(lo[s], k); hi[s] = np.maximum(hi[s], k)
    some = cnt > 0
    span = lambda sh: int((some & ((lo >> sh) != (hi >> sh))).sum())
    return dict(count=cnt, covered=int(some.sum()), words=span(6), passes=span(8), rounds=span(12))


def brute_lists(R, H, W, lazy=0):
    """every pixel's covering images in ascending index order, the walk of the reference: (lists (H, W, C) int32 padded
    with -1, counts (H, W))"""
    excl = 1 if lazy else 0
    cnt = np.zeros((H, W), np.int32)
    for r in R:
        s = _clip(r, H, W, excl)
        if s is not None:
            cnt[s] += 1
    lists = np.full((H, W, max(int(cnt.max()), 1)), -1, np.int32)
    cnt[:] = 0
    ii, jj = np.mgrid[0:H, 0:W]
    for k, r in enumerate(R):
        s = _clip(r, H, W, excl)
        if s is None:
            continue
        lists[ii[s], jj[s], cnt[s]] = k
        cnt[s] += 1
    return lists, cnt


def brute_marks(R, H, W, lazy=0):
    """per tile (by, bx) of the grid over H x W: the images with at least one pixel of the whole 64 x 4 tile (the tile is not
    clipped to the canvas: neither is the device's test) passing the per-pixel test, ascending"""
    excl = 1 if lazy else 0
    R = np.asarray(R)
    out = {}
    for by in range((H + TILE_H - 1) // TILE_H):
        for bx in range((W + TILE_W - 1) // TILE_W):
            i0, j0 = by * TILE_H, bx * TILE_W
            m = (np.maximum(R[:, 0], j0) <= np.minimum(R[:, 2] - excl, j0 + TILE_W - 1)) & \
                (np.maximum(R[:, 1], i0) <= np.minimum(R[:, 3] - excl, i0 + TILE_H - 1))
            out[(by, bx)] = tuple(int(k) for k in np.flatnonzero(m))
    return out


class CoverFault(Exception):
    """the model read an image past the table, a ballot word that no wave wrote, or wrote a word past s_cover"""


SLIPS = ("x0_lt", "x1_lt", "y0_lt", "y1_lt", "excl_forgotten", "excl_always", "walk_words_floor", "mark_bound_floor",
         "k1_arms_swapped", "hi_before_lo", "k0_dropped")


def cover_model(R, H, W, lazy=0, slip=None):
    """tile_cover + walk_cover + the per-pixel test, restated lane by lane over the grid of 64 x 4 tiles on an H x W extent
    (the canvas; (H + 1) x (W + 1) for the multiband first level): per round of 4096 images and pass of 256, thread t tests
    image k0 + 256 p + t with the expressions of blend_sample.hpp and every wave stores its ballot as word (k - k0) >> 6;
    the walk reads `words` words, each lo half then hi half, lowest bit first, and visits k0 + 64 wd + b.
    slip: one of SLIPS, the one-line change it names.  -> (marks per tile, lists, counts) as brute_marks / brute_lists give
    them; raises CoverFault where the device would read or write out of bounds or read an unwritten word."""
    assert slip is None or slip in SLIPS
    R = np.asarray(R, np.int64)
    n = len(R)
    X0, Y0, X1, Y1 = R[:, 0], R[:, 1], R[:, 2], R[:, 3]
    excl = 1 if lazy else 0
    if slip == "excl_forgotten":
        excl = 0
    if slip == "excl_always":
        excl = 1
    pix_excl = 1 if lazy else 0            # the per-pixel test (linear_sample) is not part of any slip
    visits = []                            # (tile, ordered image list) of every tile
    marks = {}
    t = np.arange(PASS)
    for by in range((H + TILE_H - 1) // TILE_H):
        for bx in range((W + TILE_W - 1) // TILE_W):
            i0, j0 = by * TILE_H, bx * TILE_W
            s_cover = [None] * COVER_WORDS
            marked, order = [], []
            for k0 in range(0, n, ROUND):
                left = n - k0
                if slip == "k1_arms_swapped":
                    k1 = k0 + ROUND if left < ROUND else n
                else:
                    k1 = n if left < ROUND else k0 + ROUND
                bound = (((k1 - k0) if slip == "mark_bound_floor" else (k1 - k0 + 63)) & ~63) + k0
                for p0 in range(k0, bound, PASS):
                    k = p0 + t
                    run = k < bound
                    inb = run & (k < k1)
                    if (inb & (k >= n)).any():
                        raise CoverFault("tile (%d, %d): image %d read, the table holds %d" % (by, bx, int(k[inb & (k >= n)][0]), n))
                    kk = np.minimum(k, n - 1)
                    a = (X0[kk] < j0 + 63) if slip == "x0_lt" else (X0[kk] <= j0 + 63)
                    b = (X1[kk] - excl > j0) if slip == "x1_lt" else (X1[kk] - excl >= j0)
                    c = (Y0[kk] < i0 + 3) if slip == "y0_lt" else (Y0[kk] <= i0 + 3)
                    d = (Y1[kk] - excl > i0) if slip == "y1_lt" else (Y1[kk] - excl >= i0)
                    hit = inb & a & b & c & d
                    for wv in range(PASS // 64):
                        if run[wv * 64]:
                            word = (int(k[wv * 64]) - k0) >> 6
                            if word >= COVER_WORDS:
                                raise CoverFault("tile (%d, %d): ballot word %d written, s_cover holds %d" % (by, bx, word, COVER_WORDS))
                            s_cover[word] = hit[wv * 64:(wv + 1) * 64].copy()
                cnt = left if left < ROUND else ROUND
                words = (cnt if slip == "walk_words_floor" else cnt + 63) >> 6
                for wd in range(words):
                    bits = s_cover[wd]
                    if bits is None:
                        raise CoverFault("tile (%d, %d): ballot word %d read, no wave wrote it" % (by, bx, wd))
                    lo, hi = np.flatnonzero(bits[:32]), 32 + np.flatnonzero(bits[32:])
                    for bit in (np.concatenate([hi, lo]) if slip == "hi_before_lo" else np.concatenate([lo, hi])):
                        marked.append(k0 + wd * 64 + int(bit))
                        order.append((0 if slip == "k0_dropped" else k0) + wd * 64 + int(bit))
            marks[(by, bx)] = tuple(sorted(marked))
            visits.append((i0, j0, order))
    deep = max((len(o) for _, _, o in visits), default=1)
    lists = np.full((H, W, max(deep, 1)), -1, np.int32); cnt = np.zeros((H, W), np.int32)
    ii, jj = np.mgrid[0:H, 0:W]
    for i0, j0, order in visits:
        ya, yb, xa, xb = i0, min(i0 + TILE_H, H) - 1, j0, min(j0 + TILE_W, W) - 1        # live pixels of the tile
        for k in order:
            x0, y0, x1, y1 = (int(v) for v in R[k])
            a, b, c, d = max(x0, xa), min(x1 - pix_excl, xb), max(y0, ya), min(y1 - pix_excl, yb)
            if b < a or d < c:
                continue
            s = (slice(c, d + 1), slice(a, b + 1))
            lists[ii[s], jj[s], cnt[s]] = k
            cnt[s] += 1
    return marks, lists[:, :, :max(int(cnt.max()), 1)], cnt


def model_differs(R, H, W, lazy, slip):
    """None when cover_model under `slip` marks and visits what the brute force does, else a one-line description"""
    try:
        marks, lists, cnt = cover_model(R, H, W, lazy, slip)
    except CoverFault as e:
        return "fault: %s" % e
    want_l, want_c = brute_lists(R, H, W, lazy)
    if not np.array_equal(cnt, want_c):
        return "%d pixels visit another number of images" % int((cnt != want_c).sum())
    deep = max(lists.shape[2], want_l.shape[2])
    pad = lambda a: np.concatenate([a, np.full(a.shape[:2] + (deep - a.shape[2],), -1, np.int32)], axis=2)
    if not np.array_equal(pad(lists), pad(want_l)):
        return "%d pixels visit their images in another order" % int((pad(lists) != pad(want_l)).any(axis=2).sum())
    want_m = brute_marks(R, H, W, lazy)
    bad = [t for t in want_m if want_m[t] != marks[t]]
    if bad:
        return "%d tiles mark another set of images" % len(bad)
    return None


def tie_pixels(R, shapes_hw, pair, H, W):
    """the pixels of the H x W canvas where both images of `pair` -- same placement, same size -- hold a valid sample and no
    other image has a larger multiband weight: the winner-takes-all map is decided between the two.  Integer translations:
    image k's sample at (i, j) is its pixel (i - y0, j - x0), valid while both bilinear taps exist."""
    def weight(k):
        x0, y0 = int(R[k][0]), int(R[k][1])
        h, w = shapes_hw[k]
        out = np.full((H, W), -1.0, np.float32)
        ya, yb, xa, xb = y0, min(y0 + h - 2, H - 1), x0, min(x0 + w - 2, W - 1)
        if yb < ya or xb < xa:
            return out
        oy = np.arange(ya, yb + 1, dtype=np.float64)[:, None] - y0; ox = np.arange(xa, xb + 1, dtype=np.float64)[None, :] - x0
        v = (0.5 - np.abs(ox / w - 0.5)) * (0.5 - np.abs(oy / h - 0.5))
        out[ya:yb + 1, xa:xb + 1] = (np.maximum(v, 0.0) + 1e-6).astype(np.float32)
        return out
    a, b = pair
    assert tuple(R[a]) == tuple(R[b]) and tuple(shapes_hw[a]) == tuple(shapes_hw[b])
    wa = weight(a)
    best = np.full((H, W), -1.0, np.float32)
    for k in range(len(R)):
        if k in pair:
            continue
        r = R[k]
        if r[2] < R[a][0] or r[0] > R[a][2] or r[3] < R[a][1] or r[1] > R[a][3]:
            continue
        best = np.maximum(best, weight(k))
    return int(((wa > 0) & (wa >= best)).sum())
