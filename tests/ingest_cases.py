"""Sources, configs and numpy restatements shared by the tests of the SIFT ingest kernel (k_grey_octaves, csrc/pyramid.hip) OFF
resize ratio 1, where its working-tile half interpolates instead of copying: test_ingest_cases_cpu.py (oracle against the
reference, the preconditions of the GPU tests, the model of the octave section's candidate rectangle) and test_gpu_ingest.py.
sift_cases.py pins everything behind this kernel at ratio 1.  No tests here."""
import numpy as np

import sift_cases as sc
from openpano_amd.config import PanoConfig

F = np.float32
WT, WR = 64, 14             # working-image tile of k_grey_octaves (WT, OP_GREY_WR)
TR, TC = 24, 72             # its per-workgroup coordinate tables


def working_dims(sh, sw, ws):
    """feature/feature.cc:33-34 as build_plan states it (csrc/sift_plan.cc), every step in fp32"""
    ratio = F(F(ws) * F(2.0)) / F(sw + sh)
    return int(F(sh) * ratio), int(F(sw) * ratio)


def source_for(wh, ww, ratio, ws=None, span=3):
    """(sh, sw, SIFT_WORKING_SIZE) whose working image is exactly wh x ww at a resize ratio as near ``ratio`` as the integers
    allow and never 1 (sh + sw != 2 ws), or None.  ``ws`` pins the working size (the images of one batch share a config)."""
    best = None
    h0, w0, s0 = round(wh / ratio), round(ww / ratio), (wh + ww) // 2
    for s in ([ws] if ws is not None else range(max(s0 - 2, 1), s0 + 4)):
        for sh in range(max(h0 - span, 2), h0 + span + 1):
            for sw in range(max(w0 - span, 2), w0 + span + 1):
                if sh + sw == 2 * s or working_dims(sh, sw, s) != (wh, ww):
                    continue
                key = (abs(2.0 * s / (sh + sw) - ratio), abs(sh - h0) + abs(sw - w0), s, sh, sw)
                if best is None or key < best:
                    best = key
    return None if best is None else (best[3], best[4], best[2])


# resize ratios: config 5's own (4000 x 3000 at 800), one half, config 4's (1300 x 867), config 2's (600 x 400), the 240 x 320
# views of the other tests, and a large up-scale whose source is a handful of pixels
RATIOS = [("r0.23", 1600.0 / 7000), ("r0.5", 0.5), ("r0.74", 1600.0 / 2167), ("r1.6", 1.6), ("r2.86", 1600.0 / 560), ("r8", 8.0)]
UPSCALE = ("r1.6", "r2.86", "r8")
COARSE = ("r8",)            # the grid of reachable working sizes is coarse there: one value on each side of both seams is asked for
SEAM_H = (3 * WR - 1, 3 * WR, 3 * WR + 1)           # 41, 42, 43
SEAM_W = (2 * WT - 1, 2 * WT, 2 * WT + 1)           # 127, 128, 129


def _seam_cases():
    out = []
    for name, ratio in RATIOS:
        for wh in SEAM_H:
            for ww in SEAM_W:
                src = source_for(wh, ww, ratio)
                if src is not None:
                    out.append(("%s_%dx%d" % (name, wh, ww), name, src, {}))
    return out


# (id, ratio class, (sh, sw, SIFT_WORKING_SIZE), further config): the working image one short of, at and one past 3 x 14 rows
# and 2 x 64 columns, four octaves (the last one 15 x 45 or so).  The parity of wh + ww against 2 ws leaves five of the nine
# pairs reachable at most ratios, all nine at 0.5, two at the large up-scale (8.5: 42 x 127 and 43 x 129 from 5 x 15).
SEAM_CASES = _seam_cases()

# every row and column index comes from a clamp of resize_coord (2 x 2) or nearly so; two octaves.  In bounds by the code:
# a run is six elements at column index <= sw - 2 of rows sx and sx + 1 <= sh - 1, an element without taps reads the run at 0.
# The reference accepts all four (test_ingest_cases_cpu.py).
SMALL_SOURCES = [("src_%dx%d" % (sh, sw), "small", (sh, sw, 48), dict(NUM_OCTAVE=2)) for sh, sw in ((2, 2), (2, 9), (9, 2), (3, 3))]

# the octave section at resize factors 0.83 and 0.77 instead of 0.71 (the two rows of test_config_variants.py that change
# SCALE_FACTOR), and eight octaves on a working image large enough for them (smallest octave 8 x 12)
_SF12 = dict(SCALE_FACTOR=1.2, NUM_SCALE=12, NUM_OCTAVE=5)
_SF13 = dict(SCALE_FACTOR=1.3, NUM_SCALE=8, GAUSS_WINDOW_FACTOR=8, GAUSS_SIGMA=1.2)


def _scale_rows():
    out = []
    for tag, kv in (("sf1.2", _SF12), ("sf1.3", _SF13)):
        for wh, ww, cls in ((43, 128, "r0.74"), (41, 128, "r2.86")):
            src = source_for(wh, ww, dict(RATIOS)[cls])
            out.append(("%s_%s_%dx%d" % (tag, cls, wh, ww), cls, src, kv))
    out.append(("oct8_r0.74_85x128", "r0.74", source_for(85, 128, dict(RATIOS)["r0.74"]), dict(NUM_OCTAVE=8)))
    return out


SCALE_ROWS = _scale_rows()

# SCALE_FACTOR below 1 makes octaves LARGER than the working image, the one way past the tables of the octave section
# (its candidate rectangle outgrows TR x TC): see test_ingest_cases_cpu.py for what the reference makes of it
FALLBACK_CASE = ("sf0.9_r0.74_43x128", "r0.74", source_for(43, 128, dict(RATIOS)["r0.74"]), dict(SCALE_FACTOR=0.9, NUM_OCTAVE=2))

# byte images at the shapes of real jobs (configs 4 and 2), default working size: (id, h, w, seed)
BIG_U8 = [("cfg4_867x1300", 867, 1300, 4), ("cfg2_400x600", 400, 600, 2)]

# batches (op_sift_batch): working images around 7 x 14 rows and 3 x 64 columns, two shapes under ONE working size per ratio
# class (the images of a call share the config; the parity of wh + ww leaves two of the nine pairs per working size).
# Down-scaling: 98 x 191 and 97 x 192, 3 x 7 = 21 tiles each, so with n copies the tile count of a group runs through every
# residue mod 8.  Up-scaling: 98 x 193 (4 x 7 = 28 tiles) and 99 x 192 (3 x 8 = 24), the one-past sides of both seams.
BATCHES = [("r0.74", 145, ((98, 191), (97, 192))), ("r2.86", 146, ((98, 193), (99, 192)))]


def batch_sources(cls, ws, shapes):
    """[(sh, sw, ws)] of the working shapes of one BATCHES row"""
    return [source_for(wh, ww, dict(RATIOS)[cls], ws=ws, span=6) for wh, ww in shapes]


def ntile(wh, ww, n):
    return -(-ww // WT) * -(-wh // WR) * n


def cfg_of(case):
    _, _, (_, _, ws), kv = case
    return PanoConfig(SIFT_WORKING_SIZE=ws, **sc.LOOSE, **kv)


def case_seed(case):
    _, _, (sh, sw, ws), _ = case
    return 7 + sc.shape_seed(sh, sw) + 31 * ws


def f32_image(case):
    """the fp32 source of a case: sift_cases.dense, so every pixel of every plane carries information"""
    _, _, (sh, sw, _), _ = case
    return sc.dense(sh, sw, case_seed(case))


def to_u8(img):
    return (img * 255 + 0.5).astype(np.uint8)


def all_bytes(u8, seed=0):
    """every byte value 0..255 planted once per channel, at pixels spread over the image (another order per channel)"""
    h, w, _ = u8.shape
    assert h * w >= 256
    rng = np.random.default_rng(seed)
    out = u8.copy()
    for ch in range(3):
        at = rng.choice(h * w, 256, replace=False)
        out.reshape(-1, 3)[at, ch] = rng.permutation(256).astype(np.uint8)
    return out


def u8_image(case):
    """the byte source of a case; the first seam case's holds all 256 byte values in each channel"""
    u8 = to_u8(f32_image(case))
    return all_bytes(u8) if case[0] == SEAM_CASES[0][0] else u8


def rgb_u8_image(case):
    """bytes with three independent channels over the whole range: a run read one element off, or channels swapped, is another
    working image (the grey textures above cannot tell)"""
    _, _, (sh, sw, _), _ = case
    return np.random.default_rng(case_seed(case) + 1).integers(0, 256, (sh, sw, 3), dtype=np.uint8)


def twin(u8):
    """the fp32 image read_img makes of decoder bytes (lib/imgio.cc:54-56)"""
    return (u8.astype(np.float64) / 255.0).astype(np.float32)


def big_u8(h, w, seed):
    return to_u8(sc.dense(h, w, seed))


# ---- numpy fp32 restatements of csrc/pyramid.hip, same operation order; every argument may be an array ----

def resize_coord(d, inv_f, srcn):
    """resize_coord (lib/imgproc.cc:32-44) of destination indices d -> (source index, weight, lower clamp taken, upper clamp taken)"""
    rr = (np.asarray(d).astype(F) + F(0.5)) * np.asarray(inv_f, F) - F(0.5)
    ss = np.floor(rr).astype(np.int64)
    rr = rr - ss.astype(F)
    lo = ss < 0
    hi = ~lo & (ss + 1 >= srcn)
    ss = np.where(lo, 0, np.where(hi, np.asarray(srcn) - 2, ss))
    rr = np.where(lo, F(0), np.where(hi, F(1), rr)).astype(F)
    return ss, rr, lo, hi


def inv_factor(dstn, srcn):
    """ifx of resize_bilinear: 1.f / ((float)dstn / srcn)"""
    return F(1) / (np.asarray(dstn).astype(F) / np.asarray(srcn).astype(F))


def octave_extent(n, scale_factor, o):
    """feature/dog.cc:105-107 as build_plan states it: ceil(n * (float)pow((double)SCALE_FACTOR, -o)), SCALE_FACTOR a float"""
    factor = F(float(F(scale_factor)) ** -o)
    return np.ceil(np.asarray(n).astype(F) * factor).astype(np.int64)


def candidate_rect(t0, tile, n, on):
    """r_lo / r_hi (c_lo / c_hi) of the octave section for the tile that starts at t0: working extent n, octave extent on"""
    t0 = np.asarray(t0)
    f = np.asarray(on).astype(F) / np.asarray(n).astype(F)
    lo = np.floor((t0.astype(F) + F(0.5)) * f - F(0.5)).astype(np.int64) - 1
    hi = np.ceil(((t0 + tile).astype(F) + F(0.5)) * f - F(0.5)).astype(np.int64) + 2
    return np.maximum(lo, 0), np.minimum(hi, on)
