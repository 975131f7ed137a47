"""GPU: every C-layer call gives the device pool back what it took -- on success after its results are freed, and on the
argument refusals that come after blocks were allocated and copies queued (op_debug_pool_stats / hip.pool_stats()).

The pool is process-wide and does not track streams; a call's blocks belong to its CallBlocks (csrc/internal.hpp), which
frees them on every exit and waits for the call's stream first unless the call already has.  The figures compared are
live_blocks and live_bytes (cached_bytes moves whenever a block changes hands).  A context's arenas and the SIFT workspace
are hipMalloc memory, not pool blocks.  Exits that only a failing runtime call reaches are not provoked here."""
from openpano_amd.hip import pool_stats          # the module needs the accessor: without it, it fails here

import gc

import numpy as np
import pytest

from openpano_amd import hip, synth
from openpano_amd.config import PanoConfig

pytestmark = pytest.mark.gpu
N, H, W, MID = 4, 120, 160, 1
METHOD = 2                                        # spherical, the "camera" scene's projection
GAINS = np.array([[1.1, 0.9, 1.05], [0.95, 1.0, 1.1], [1.2, 1.05, 0.9], [0.9, 1.1, 1.0]], np.float32)


class balanced:
    """live blocks and bytes of the pool are the same after the block as before it"""

    def __enter__(self):
        gc.collect()                              # handles an earlier test left to the collector go now, not in the window
        self.before = pool_stats()[:2]
        return self

    def __exit__(self, et, ev, tb):
        if et is None:
            assert pool_stats()[:2] == self.before


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.close()


def _blend_cfg(mb=0):
    return PanoConfig(ESTIMATE_CAMERA=1, ORDERED_INPUT=0, LAZY_READ=0, MULTIBAND=mb)


_scene = []


def scene():
    if not _scene:
        views, homos = synth.pano_scene(N, H, W, seed=7, proj="camera")
        views = [np.ascontiguousarray(v, np.float32) for v in views]
        for v in views:
            v.setflags(write=False)
        _scene.append((views, np.asarray(homos)))
    return _scene[0]


def small_images(n, seed=11):
    return [np.ascontiguousarray(v, np.float32) for v in synth.image_set(n, 48, 64, seed=seed, overlap=0.5)]


# ---- 1. success paths -------------------------------------------------------------------------------------------------
def test_pool_stats_reads(ctx):
    live, nbytes, cached = pool_stats()
    assert live >= 0 and nbytes >= 0 and cached >= 0
    with balanced() as b:
        v = hip.Views.upload(ctx, small_images(2))
        assert pool_stats()[0] == b.before[0] + 1 and pool_stats()[1] > b.before[1]       # one block, counted while held
        v.free()


def test_sift_one_group(ctx, cfg):
    imgs = small_images(4)
    with balanced():
        f = hip.sift_batch(ctx, cfg, imgs)
        assert f.num_images == 4
        f.free()


def test_sift_three_groups(ctx, cfg):
    a = small_images(4)
    imgs = [a[0], a[1], np.ascontiguousarray(a[2].transpose(1, 0, 2)), (a[3] * 255).astype(np.uint8)]
    assert [(x.shape, x.dtype.name) for x in imgs] == [((48, 64, 3), "float32")] * 2 + [((64, 48, 3), "float32"), ((48, 64, 3), "uint8")]
    with balanced():
        f = hip.sift_batch(ctx, cfg, imgs)
        assert f.num_images == 4
        f.free()


@pytest.mark.parametrize("n", [16, 4], ids=["pipelined_two_chunks", "plain"])
def test_sift_host_call(ctx, cfg, n):
    imgs = small_images(n)
    rows = 4096 * n
    desc = np.empty((rows, 128), np.float32); coor = np.empty((rows, 2), np.float64)
    call = hip.SiftHostCall(ctx, cfg, imgs, desc.ctypes.data, coor.ctypes.data, rows)
    with balanced():
        f = call()
        assert f.num_images == n and 0 < f.total <= rows
        f.free()


def test_sift_staged(ctx, cfg):
    img = small_images(1)[0]
    with balanced():
        st = hip.sift_staged(ctx, cfg, img, planes=False)
        assert len(st.desc) == len(st.coor)


def test_match_ransac_concat(ctx, cfg):
    imgs = small_images(4)
    pairs = [(0, 1), (1, 2), (2, 3)]
    with balanced():
        f = hip.sift_batch(ctx, cfg, imgs)
        m = hip.match_pairs_handle(ctx, cfg, f, pairs)
        assert m.total > 0                        # the result list is a pool block
        res = hip.ransac_pairs(ctx, cfg, f, m, pairs, [(64, 48)] * 4, base_seed=3)
        assert len(res) == 3
        m2 = hip.match_pairs_handle(ctx, cfg, f, pairs[:1])
        both = hip.Matches.concat(ctx, m, m2)
        assert both.total == m.total + m2.total
        both.free(); m2.free(); m.free(); f.free()


@pytest.mark.parametrize("source", ["host", "views"])
@pytest.mark.parametrize("mode", ["none", "image", "block", "vignette"])
@pytest.mark.parametrize("mb", [0, 3])
def test_blend(ctx, mb, mode, source):
    views, homos = scene()
    kw = dict(none={}, image=dict(gains=GAINS), block=dict(gains=np.tile(GAINS[:, None, None, :], (1, 2, 3, 1))),
              vignette=dict(gains=GAINS, vignette=(-0.1, 0.02, -0.01)))[mode]
    with balanced():
        src = hip.Views.upload(ctx, views) if source == "views" else views
        cv = hip.blend(ctx, _blend_cfg(mb), src, homos, METHOD, MID, **kw)
        assert cv.h > 0 and cv.w > 0
        cv.free()
        if source == "views":
            src.free()


def test_overlap_passes(ctx):
    views, homos = scene()
    call = hip.BlendCall(ctx, _blend_cfg(), views, homos, METHOD, MID)
    with balanced():
        assert call.overlap_sums()[0].sum() > 0
        assert call.block_overlap_sums(2, 2)[0].sum() > 0
        assert call.vignette_overlap_sums()[0].sum() > 0


def test_canvas_consumers(ctx):
    views, homos = scene()
    with balanced():
        cv = hip.blend(ctx, _blend_cfg(), views, homos, METHOD, MID)
        with balanced():
            cropped, (x0, y0) = cv.crop()
            assert 0 < cropped.h <= cv.h and 0 < cropped.w <= cv.w
            cropped.free()
        with balanced():
            assert cv.numpy_u8().shape == (cv.h, cv.w, 3)
        with balanced():
            assert cv.png_bytes()[:8] == b"\x89PNG\r\n\x1a\n"
        cv.free()


def test_encode_png_u8(ctx):
    img = (small_images(1)[0] * 255).astype(np.uint8)
    with balanced():
        assert hip.encode_png_u8(ctx, img)[:8] == b"\x89PNG\r\n\x1a\n"


def test_cyl_warp_from_host(ctx, cfg):
    img = scene()[0][0]
    with balanced():
        cv = hip.cyl_warp(ctx, cfg, img, 1.0)
        assert cv.h > 0 and cv.w > 0
        cv.free()


# ---- 2. refusals after images 0 and 1 were queued -------------------------------------------------------------------------
ENTRIES = {          # C entry point -> (BlendCall keywords, the call -> a tuple of arrays)
    "op_blend": ({}, lambda c: _canvas(c)),
    "op_blend_gains": (dict(gains=GAINS), lambda c: _canvas(c)),
    "op_gain_overlap": ({}, lambda c: c.overlap_sums()),
    "op_gain_block_overlap": ({}, lambda c: c.block_overlap_sums(2, 2)),
    "op_vignette_overlap": ({}, lambda c: c.vignette_overlap_sums()),
}


def _canvas(call):
    cv = call()
    a = cv.numpy(); cv.free()
    return (a,)


def _spoil_range(call):
    old = call.arr[2].range[0]
    call.arr[2].range[0] = call.geom.proj_min[0] - 10 * call.geom.resolution[0]
    return "image range outside proj_range", lambda: call.arr[2].range.__setitem__(0, old)


def _spoil_height(call):
    old = call.arr[2].h
    call.arr[2].h = 1
    return "bad image 2", lambda: setattr(call.arr[2], "h", old)


@pytest.mark.parametrize("source", ["host", "views"])
@pytest.mark.parametrize("spoil", [_spoil_range, _spoil_height], ids=["range", "height"])
@pytest.mark.parametrize("entry", list(ENTRIES))
def test_refusal_balances_and_leaves_the_pool_usable(ctx, entry, spoil, source):
    views, homos = scene()
    kw, run = ENTRIES[entry]
    src = hip.Views.upload(ctx, views) if source == "views" else views
    try:
        call = hip.BlendCall(ctx, _blend_cfg(), src, homos, METHOD, MID, **kw)
        want = run(call)                          # before any refusal
        assert all(a.size > 0 for a in want)
        with balanced():
            message, restore = spoil(call)
            with pytest.raises(hip.OpenPanoHipError, match="error -1: .*" + message):
                run(call)
            restore()
        with balanced():
            got = run(call)
        assert len(got) == len(want) and all(np.array_equal(g, w) for g, w in zip(got, want))
    finally:
        if source == "views":
            src.free()
