"""GPU: every kernel path of the multiband blender and every gain mode of its level 0 (csrc/blend.hip: blend_impl,
k_mb_first_fused<GM>, k_mb_blur_fused, k_mb_blur, k_mb_bands, k_mb_accumulate) against the C oracle
(oracle/blend_oracle.c: orc_blend_multiband_gained), bit for bit.

blend_impl picks its kernels from the Gaussian half-width of each level -- GaussCache (feature/gaussian.cc:17-40) with
GAUSS_WINDOW_FACTOR wf: wf at levels 0-2, floor(1.5 wf) at levels 3-8, 2 wf at level 9 -- and from the level count:
  half-width 6 or 9   k_mb_blur_fused<C, level == 0> (both passes in one kernel; level 0 also writes its band)
  any other           k_mb_blur<true, 0> then k_mb_blur<false, 0> (the generic two-pass blur)
  MULTIBAND <= 6      k_mb_bands<NL> (NL = MULTIBAND, one less when the fused level 0 wrote its band)
  MULTIBAND > 6       k_mb_accumulate, one pass per level
  half-width > 15     refused (OP_ERR_UNSUPPORTED), before any device work.
The shipped factor 6 with the level counts of the other blend tests never leaves the fused blur and k_mb_bands<1..4>.

1. path matrix without gains: flat, cylindrical and spherical rows that together reach every instance above;
2. edge geometry: views smaller than the blur window (every ROI pixel inside the replicate halo), ROI widths at and one
   either side of the fused kernel's band width (256 - 2C) and ROI heights at and one either side of its segment
   height (SEG), for C = 6 and 9 -- the sizes are asserted from the call's ROIs;
3. every gain mode on multiband rows (a non-shipped window factor and the cylindrical row among them), with views and
   gains that clamp at level 0, gains exactly 1, block grids that a transposition changes and a vignetting curve with
   non-unit gains; one flat row puts valid samples on the ROI pixels one past the target, which feed the blurs;
4. a too-wide blur is refused with its message, and the next blend on the same context still equals the oracle."""
import math

import numpy as np
import pytest

from openpano_amd import hip, synth
from openpano_amd.config import PanoConfig

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.close()


def _cfg(**kv):
    base = dict(ESTIMATE_CAMERA=1, ORDERED_INPUT=0, LAZY_READ=0, MULTIBAND=0)
    base.update(kv)
    return PanoConfig(**base)


def _flat_cfg(**kv):
    return _cfg(ESTIMATE_CAMERA=0, TRANS=1, ORDERED_INPUT=1, **kv)


def _cyl_cfg(**kv):
    return _cfg(ESTIMATE_CAMERA=0, CYLINDER=1, ORDERED_INPUT=1, **kv)


def _compare(got, want, what):
    assert got.shape == want.shape, what
    if not np.array_equal(got, want):
        no_g, no_w = got[..., 0] < 0, want[..., 0] < 0
        both = ~(no_g | no_w)
        diff = np.abs(got[both] - want[both])
        raise AssertionError("%s: canvas differs: mask flips %d, max |d| %g, unequal pixels %d"
                             % (what, int((no_g != no_w).sum()), float(diff.max()) if diff.size else 0.0, int((diff != 0).sum())))


def _device(ctx, cfg, views, homos, method, idx, **gk):
    cv = hip.blend(ctx, cfg, views, homos, method, idx, **gk)
    x = cv.numpy(); cv.free()
    return x


def half_widths(wf, levels):
    """the blur half-width of every level but the last (gauss_taps: kw = ceil(0.3 (sigma / 2 - 1) + 0.8) wf, odd)"""
    out = []
    for level in range(levels - 1):
        sigma = float(np.float32(math.sqrt(level * 2 + 1.0) * 4))
        kw = int(math.ceil(0.3 * (float(np.float32(np.float32(sigma) / np.float32(2) - np.float32(1)))) + 0.8) * wf)
        out.append((kw | 1) // 2)
    return out


def kernel_instances(wf, levels):
    """the multiband kernels blend_impl launches for (GAUSS_WINDOW_FACTOR, MULTIBAND)"""
    cs = half_widths(wf, levels)
    ks = set()
    for level, c in enumerate(cs):
        if c in (6, 9):
            ks.add("k_mb_blur_fused<%d,%s>" % (c, "true" if level == 0 else "false"))
        else:
            ks |= {"k_mb_blur<true,0>", "k_mb_blur<false,0>"}
    if levels > 6:
        ks.add("k_mb_accumulate")
    else:
        ks.add("k_mb_bands<%d>" % (levels - (1 if cs and cs[0] in (6, 9) else 0)))
    return ks, cs


def _rois(meta):
    """the inclusive canvas ROI (x0, y0, x1, y1) of every image (Coor truncation, stitcher_image.cc:123-129)"""
    minx, miny, _, _, resx, resy = meta["geom"]
    return [(int((r[0] - minx) / resx), int((r[1] - miny) / resy), int((r[2] - minx) / resx), int((r[3] - miny) / resy))
            for r in meta["ranges"]]


def flat_scene(specs, seed, identity_idx):
    """views of one world placed by translation and scale: spec (L, T, w, h, s) puts the w x h view on the canvas-space
    rectangle [L, L + s w] x [T, T + s h] (homography [[s, 0, L + s w / 2], [0, s, T + s h / 2], [0, 0, 1]]; the
    identity view must have s = 1).  Integer L, T with s = 1 give an ROI of exactly (w + 1) x (h + 1)."""
    W = int(max(L + s * w for L, T, w, h, s in specs)) + 8
    H = int(max(T + s * h for L, T, w, h, s in specs)) + 8
    world = synth.make_world(seed, H + 16, W + 16, work_scale=4.0, density=500.0)
    views, homos = [], []
    for L, T, w, h, s in specs:
        rr = (8 + int(T) + (np.arange(h) * s).astype(int))[:, None]
        cc = (8 + int(L) + (np.arange(w) * s).astype(int))[None, :]
        views.append(np.ascontiguousarray(world[rr, cc], np.float32))
        homos.append(np.array([[s, 0, L + s * w / 2], [0, s, T + s * h / 2], [0, 0, 1.0]]))
    assert specs[identity_idx][4] == 1
    return views, np.stack(homos)


def _valid_past_target(views, meta, H, W):
    """samples of ROI pixels one past the target (row H or column W) that interpolate() accepts, flat projection: the
    device's fp64 map (proj2homo, space_to_image) restated in the same operation order"""
    minx, miny, _, _, resx, resy = meta["geom"]
    count = 0
    for k, (x0, y0, x1, y1) in enumerate(_rois(meta)):
        d = meta["homo_inv"][k]
        h, w = views[k].shape[:2]
        for i in range(y0, y1 + 1):
            for j in range(x0, x1 + 1):
                if i < H and j < W:
                    continue
                hx, hy, hz = j * resx + minx, i * resy + miny, 1.0
                rx = d[0] * hx + d[1] * hy + d[2] * hz
                ry = d[3] * hx + d[4] * hy + d[5] * hz
                rz = d[6] * hx + d[7] * hy + d[8] * hz
                if rz < 0:
                    continue
                ox, oy = rx * (1.0 / rz) + w * 0.5, ry * (1.0 / rz) + h * 0.5
                fr, fc = math.floor(np.float32(oy)), math.floor(np.float32(ox))
                count += fr >= 0 and fc >= 0 and fc + 1 < w and fr + 1 < h
    return count


# ---- 1. path matrix, no gains ----
PATHS = [                        # (proj, method, cfg)
    ("flat", 0, _flat_cfg(MULTIBAND=6)),                              # fused<6,true>, <6,false>, <9,false>; k_mb_bands<5>
    ("camera", 1, _cyl_cfg(MULTIBAND=6, GAUSS_WINDOW_FACTOR=4)),      # generic at 0-2, fused<6,false> from 3; k_mb_bands<6>
    ("camera", 2, _cfg(MULTIBAND=5, GAUSS_WINDOW_FACTOR=9)),          # fused<9,true>, <9,false>, generic at 3; k_mb_bands<4>
    ("flat", 0, _flat_cfg(MULTIBAND=7, GAUSS_WINDOW_FACTOR=10)),      # generic at half-widths 10 and 15; k_mb_accumulate
    ("camera", 2, _cfg(MULTIBAND=7, GAUSS_WINDOW_FACTOR=10)),
]


def test_path_matrix_reaches_every_kernel():
    """the rows of this file reach every multiband kernel instance of blend_impl (the dispatch above)"""
    want = {"k_mb_blur<true,0>", "k_mb_blur<false,0>", "k_mb_blur_fused<6,true>", "k_mb_blur_fused<6,false>",
            "k_mb_blur_fused<9,true>", "k_mb_blur_fused<9,false>", "k_mb_bands<5>", "k_mb_bands<6>", "k_mb_accumulate"}
    got = set()
    for _, _, cfg in PATHS:
        ks, cs = kernel_instances(cfg.GAUSS_WINDOW_FACTOR, cfg.MULTIBAND)
        assert max(cs) <= 15
        got |= ks
    assert want <= got, want - got
    assert half_widths(10, 7) == [10, 10, 10, 15, 15, 15]            # the widest blur the device takes
    assert half_widths(6, 11) == [6, 6, 6, 9, 9, 9, 9, 9, 9, 12]


@pytest.mark.parametrize("proj,method,bcfg", PATHS, ids=["flat-wf6-mb6", "cyl-wf4-mb6", "sph-wf9-mb5", "flat-wf10-mb7", "sph-wf10-mb7"])
def test_multiband_paths_equal_oracle(ctx, oracle, proj, method, bcfg):
    views, homos = synth.pano_scene(5, 200, 280, seed=101 + method, proj=proj)
    want, _ = oracle.blend(views, homos, method, 2, bcfg)
    assert (want >= 0).mean() > 0.5
    _compare(_device(ctx, bcfg, views, homos, method, 2), want, (proj, bcfg.GAUSS_WINDOW_FACTOR, bcfg.MULTIBAND))


# ---- 2. edge geometry ----
# (L, T, w, h, s): ROI widths 243 / 244 / 245 around 256 - 2 * 6 and 237 / 238 / 239 around 256 - 2 * 9, heights
# 111 / 112 / 113 around SEG(6) = 8 * 14 and 119 / 120 / 121 around SEG(9) = 6 * 20; two views smaller than any window
EDGE_SPECS = [(0, 6, 242, 110, 1), (120, 4, 243, 111, 1), (240, 2, 244, 112, 1), (360, 0, 236, 118, 1),
              (480, 3, 237, 119, 1), (600, 5, 238, 120, 1), (130, 50, 5, 4, 1), (400, 60, 9, 7, 1)]
EDGE_CFGS = [_flat_cfg(MULTIBAND=5), _flat_cfg(MULTIBAND=4, GAUSS_WINDOW_FACTOR=9), _flat_cfg(MULTIBAND=6, GAUSS_WINDOW_FACTOR=4)]


@pytest.mark.parametrize("bcfg", EDGE_CFGS, ids=["wf6-mb5", "wf9-mb4", "wf4-mb6"])
def test_multiband_edge_geometry_equals_oracle(ctx, oracle, bcfg):
    views, homos = flat_scene(EDGE_SPECS, seed=17, identity_idx=1)
    want, meta = oracle.blend(views, homos, 0, 1, bcfg)
    rois = _rois(meta)
    widths, heights = {x1 - x0 + 1 for x0, _, x1, _ in rois}, {y1 - y0 + 1 for _, y0, _, y1 in rois}
    for c in (6, 9):
        band, seg = 256 - 2 * c, (8 if c <= 6 else 6) * (2 * c + 2)
        assert {band - 1, band, band + 1} <= widths, (c, sorted(widths))
        assert {seg - 1, seg, seg + 1} <= heights, (c, sorted(heights))
    small = [r for r in rois if r[2] - r[0] + 1 <= 6 and r[3] - r[1] + 1 <= 6]     # ROI within a half-width of both borders
    assert small and (want >= 0).mean() > 0.5
    _compare(_device(ctx, bcfg, views, homos, 0, 1), want, (bcfg.GAUSS_WINDOW_FACTOR, bcfg.MULTIBAND))


# ---- 3. gains in multiband ----
# flat: the last view at half scale, placed so that its ROI's last row and column lie one past the target and still hold
# valid samples; the right and bottom edges of the canvas are its own
GAIN_SPECS = [(0, 4, 200, 150, 1), (110, 0, 210, 160, 1), (230, 6, 200, 150, 1), (350, 2, 220, 156, 1), (480.75, 10.75, 240, 300, 0.5)]
GAIN_ROWS = [                    # (name, cfg)
    ("flat-wf6-mb5", _flat_cfg(MULTIBAND=5)),
    ("cyl-wf4-mb6", _cyl_cfg(MULTIBAND=6, GAUSS_WINDOW_FACTOR=4)),
    ("sph-wf9-mb5", _cfg(MULTIBAND=5, GAUSS_WINDOW_FACTOR=9)),
]
GRIDS = [(3, 2), (1, 5), (16, 1), (5, 3)]            # (bx, by): none of them survives a transposition


def _gain_scene(name):
    if name.startswith("flat"):
        views, homos = flat_scene(GAIN_SPECS, seed=23, identity_idx=2)
        return views, homos, 0, 2
    views, homos = synth.pano_scene(5, 200, 280, seed=111, proj="camera")
    return views, homos, (1 if name.startswith("cyl") else 2), 2


def _gains(n, seed):
    """per-image gains in [0.6, 2.2] (bright samples clamp), image 1 exactly 1 and one more channel exactly 1"""
    G = np.random.default_rng(seed).uniform(0.6, 2.2, (n, 3)).astype(np.float32)
    G[1] = 1.0
    G[3, 2] = 1.0
    return G


@pytest.mark.parametrize("name,bcfg", GAIN_ROWS, ids=[r[0] for r in GAIN_ROWS])
def test_multiband_gain_modes_equal_oracle(ctx, oracle, name, bcfg):
    views, homos, method, idx = _gain_scene(name)
    n = len(views)
    plain, meta = oracle.blend(views, homos, method, idx, bcfg)
    H, W = plain.shape[:2]
    assert (plain >= 0).mean() > 0.5
    if method == 0:
        x0, y0, x1, y1 = _rois(meta)[-1]
        assert (x1, y1) == (W, H) and _valid_past_target(views, meta, H, W) > 100
    G = _gains(n, 5)
    assert max((views[k] * G[k]).max() for k in range(n)) > 1.5           # level 0 clamps
    jobs = [("image", dict(gains=G))]
    for bx, by in GRIDS:
        M = np.random.default_rng(bx * 16 + by).uniform(0.6, 2.2, (n, by, bx, 3)).astype(np.float32)
        M[1] = 1.0
        M[n - 1, 0, -1, :] = 1.0
        jobs.append(("block %dx%d" % (bx, by), dict(gains=M)))
    for poly in ((-0.5, 0.4, -0.2), (0.35, -0.1, 0.05)):
        jobs.append(("vignette %s" % (poly,), dict(gains=G, vignette=np.array(poly, np.float32))))
    jobs.append(("vignette, gains 1", dict(gains=None, vignette=np.array((-0.5, 0.4, -0.2), np.float32))))
    for what, gk in jobs:
        want, _ = oracle.blend(views, homos, method, idx, bcfg, **gk)
        assert not np.array_equal(want, plain), what
        _compare(_device(ctx, bcfg, views, homos, method, idx, **gk), want, (name, what))


# ---- 4. refusal ----
@pytest.mark.parametrize("wf,levels", [(8, 11), (16, 2)])
def test_too_wide_blur_refused_then_blend_equals_oracle(ctx, oracle, wf, levels):
    assert max(half_widths(wf, levels)) > 15
    views, homos = synth.pano_scene(4, 120, 160, seed=7, proj="camera")
    bad = _cfg(MULTIBAND=levels, GAUSS_WINDOW_FACTOR=wf)
    with pytest.raises(hip.OpenPanoHipError, match=r"error -4: op_blend: Gaussian kernel wider than 31 taps"):
        hip.blend(ctx, bad, views, homos, 2, 1)
    with pytest.raises(hip.OpenPanoHipError, match=r"error -4: op_blend_block_gains: Gaussian kernel wider than 31 taps"):
        hip.blend(ctx, bad, views, homos, 2, 1, gains=np.full((4, 2, 3, 3), 1.5, np.float32))
    cfg = _cfg(MULTIBAND=4)
    for gk in (dict(), dict(gains=np.full(4, 1.25, np.float32))):
        want, _ = oracle.blend(views, homos, 2, 1, cfg, **gk)
        _compare(_device(ctx, cfg, views, homos, 2, 1, **gk), want, ("after refusal", wf, levels))
