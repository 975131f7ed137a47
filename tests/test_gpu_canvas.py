"""GPU: the canvas stage (csrc/canvas.hip) on the cases of tests/canvas_cases.py -- the crop to the largest valid rectangle
(k_crop_heights / k_crop_lines / k_crop_pick) with extents that end on chunk boundaries, searches that skip whole chunks, ties
within a line and across lines, more than 256 lines, more than 64 KiB of dynamic LDS and the width limit; the byte
quantisation (k_to_u8) at the values where fl32(v * 255) sits on an integer or one ulp below and at element counts around its
256-thread block; the cylinder pre-warp from fp32, bytes and resident views at tiny shapes, off the default focal length,
with Color::NO in the source, and its trig-table cache across two radii of one output width.  Everything is bit-exact against
the C oracle, which test_canvas_cases_cpu.py shows equal to the reference and to the models at every case used here; each
family's claim is asserted again on the canvas the device returns."""
import zlib

import numpy as np
import pytest

import canvas_cases as cc

pytestmark = pytest.mark.gpu
NOPTS = np.zeros((0, 2))


@pytest.fixture(scope="module")
def ctx():
    from openpano_amd import hip
    c = hip.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def orc():
    from checkers import Oracle
    return Oracle(cc.blend_cfg())


def _canvas(ctx, view):
    from openpano_amd import hip
    return hip.blend(ctx, cc.blend_cfg(), [view], cc.HOMO, 0, 0)


def _crop_equals_oracle(ctx, orc, case):
    view = cc.view_of(case)
    want_full = orc.blend([view], cc.HOMO, 0, 0)[0]
    cv = _canvas(ctx, view)
    try:
        full = cv.numpy()
        assert np.array_equal(full, want_full), case.id                 # a blend difference is not blamed on crop
        x0, y0, w, h = cc.check_family(case, cc.canvas_mask(full))
        want, off = orc.crop(want_full)
        cropped, got_off = cv.crop()
        try:
            assert got_off == off == (x0, y0), (case.id, got_off, off, (x0, y0))
            assert (cropped.h, cropped.w) == want.shape[:2] == (h, w), (case.id, cropped.h, cropped.w, want.shape)
            assert np.array_equal(cropped.numpy(), want), case.id
            assert np.array_equal(cropped.numpy_u8(), orc.to_u8(want)), case.id
        finally:
            cropped.free()
    finally:
        cv.free()


DEVICE_CROP = cc.CROP_SMALL + [cc.WIDE_LDS, cc.WIDE_MAX]


@pytest.mark.parametrize("case", DEVICE_CROP, ids=[c.id for c in DEVICE_CROP])
def test_crop_case(ctx, orc, case):
    """the device canvas equals the oracle's, the family's claim holds on it, and crop() returns the oracle's origin, shape and
    pixels -- the model's rectangle -- and the oracle's bytes; the empty results (0 x 1) come back without error"""
    _crop_equals_oracle(ctx, orc, case)


def test_crop_cases_in_mixed_order_on_one_context(ctx, orc):
    """the families interleaved (widths and line counts change from call to call, the 16500- and 37809-wide canvases between
    small ones), then the first case again: nothing is carried from one call to the next"""
    order = sorted(DEVICE_CROP, key=lambda c: (zlib.crc32(c.id.encode()) % 7, c.family))
    assert len({c.family for c in order[:12]}) >= 5
    for case in order + [order[0]]:
        _crop_equals_oracle(ctx, orc, case)


def test_crop_width_limit(ctx, orc):
    """37810 columns: refused by the argument check (OP_ERR_UNSUPPORTED), before anything is allocated or launched; the
    context goes on cropping, the widest accepted canvas included"""
    from openpano_amd import hip
    cv = _canvas(ctx, cc.view_of(cc.WIDE_REFUSED))
    try:
        assert (cv.h, cv.w) == (3, cc.MAX_CROP_WIDTH + 1)
        before = hip.pool_stats()[:2]
        with pytest.raises(hip.OpenPanoHipError, match=r"error -4: op_canvas_crop: canvas wider than"):
            cv.crop()
        assert hip.pool_stats()[:2] == before
    finally:
        cv.free()
    _crop_equals_oracle(ctx, orc, cc.FAMILY_B[0])
    _crop_equals_oracle(ctx, orc, cc.WIDE_MAX)


# ---- bytes -------------------------------------------------------------------------------------------------------------------

def test_bytes_at_the_quantisation_edges(ctx, orc):
    cv = _canvas(ctx, cc.byte_view())
    try:
        full = cv.numpy()
        assert np.array_equal(full, orc.blend([cc.byte_view()], cc.HOMO, 0, 0)[0])
        m = cc.canvas_mask(full)
        on, below = cc.on_integer(full[m])
        assert len(np.unique(full[m][on])) >= 200 and len(np.unique(full[m][below])) >= 200 and not m.all()
        got = cv.numpy_u8()
        assert len(np.unique(got[m])) == 256
        assert np.array_equal(got, orc.to_u8(full)) and np.array_equal(got, cc.byte_model(full))
    finally:
        cv.free()


@pytest.mark.parametrize("h,w", cc.COUNT_SHAPES, ids=["%dx%d_%d" % (h, w, 3 * h * w) for h, w in cc.COUNT_SHAPES])
def test_bytes_at_element_counts_around_the_block(ctx, orc, h, w):
    """3, 255, 258, 513, 768 and 1281 elements (h * w * 3 is a multiple of 3): the last block of k_to_u8 holds 3, 255, 2, 1,
    256 and 1 of them"""
    cv = _canvas(ctx, cc.count_view(h, w))
    try:
        cropped, off = cv.crop()
        try:
            assert (cropped.h, cropped.w) == (h, w) and off == (1, 0)
            f32 = cropped.numpy()
            assert np.array_equal(f32, orc.crop(orc.blend([cc.count_view(h, w)], cc.HOMO, 0, 0)[0])[0])
            got = cropped.numpy_u8()
            assert got.size == 3 * h * w and np.array_equal(got, orc.to_u8(f32)) and np.array_equal(got, cc.byte_model(f32))
        finally:
            cropped.free()
    finally:
        cv.free()


def test_bytes_of_an_empty_crop(ctx):
    by = {c.id: c for c in cc.FAMILY_G}
    for name in ("G_w2_full_view", "G_w3_no_view_pixel"):
        cv = _canvas(ctx, cc.view_of(by[name]))
        cropped, off = cv.crop()
        try:
            assert (cropped.h, cropped.w) == (0, 1) and off == (0, 1)
            assert cropped.numpy_u8().shape == (0, 1, 3)
        finally:
            cropped.free(); cv.free()


# ---- cylinder ----------------------------------------------------------------------------------------------------------------

def _warp(ctx, cfg, image, hf):
    from openpano_amd import hip
    cv = hip.cyl_warp(ctx, cfg, image, hf)
    out = cv.numpy()
    cv.free()
    return out


@pytest.mark.parametrize("h,w", cc.CYL_SHAPES, ids=["%dx%d" % s for s in cc.CYL_SHAPES])
def test_cyl_warp_cases(ctx, orc, h, w):
    """every h_factor and focal length of a shape: the fp32 image, the fp32 image with a Color::NO block, the byte image
    against the oracle on its fp32 twin, and the fp32 and byte images as resident views"""
    from openpano_amd import hip
    f32, holes, u8 = cc.cyl_image(h, w), cc.cyl_holes(h, w), cc.cyl_bytes(h, w)
    views = hip.Views.upload(ctx, [f32, u8])
    try:
        dev_f32, dev_u8 = views.images()
        assert len(dev_f32) == 3 and dev_u8[3] == "u8"
        for (_, _, hf, fl) in [c for c in cc.CYL_CASES if c[:2] == (h, w)]:
            cfg = cc.cyl_cfg(fl)
            want = orc.cyl_warp(f32, hf, NOPTS, cfg)[0]
            assert want.size > 0 and (want[..., 0] >= 0).any()
            assert np.array_equal(_warp(ctx, cfg, f32, hf), want), (hf, fl)
            assert np.array_equal(_warp(ctx, cfg, dev_f32, hf), want), (hf, fl)
            want_holes = orc.cyl_warp(holes, hf, NOPTS, cfg)[0]
            assert ((want_holes[..., 0] < 0) & (want[..., 0] >= 0)).any()
            assert np.array_equal(_warp(ctx, cfg, holes, hf), want_holes), (hf, fl)
            want_u8 = orc.cyl_warp(cc.twin(u8), hf, NOPTS, cfg)[0]
            assert np.array_equal(_warp(ctx, cfg, u8, hf), want_u8), (hf, fl)
            assert np.array_equal(_warp(ctx, cfg, dev_u8, hf), want_u8), (hf, fl)
    finally:
        views.free()


def test_cyl_warp_of_two_by_two_is_refused(ctx, orc):
    from openpano_amd import hip
    h, w, hf, fl = cc.CYL_EMPTY
    assert orc.cyl_warp(cc.cyl_image(h, w), hf, NOPTS, cc.cyl_cfg(fl))[0].shape[1] == 0
    before = hip.pool_stats()[:2]
    for img in (cc.cyl_image(h, w), cc.cyl_bytes(h, w)):
        with pytest.raises(hip.OpenPanoHipError, match=r"error -1: op_cyl_warp: empty output"):
            hip.cyl_warp(ctx, cc.cyl_cfg(fl), img, hf)
    assert hip.pool_stats()[:2] == before


def test_cyl_trig_table_follows_the_radius(ctx, orc):
    """focal lengths 59 and 60 give a 67 x 130 image the same output width and another radius: A, B, A, B on one context"""
    from openpano_amd import hip
    h, w, hf, fa, fb = cc.CACHE_PAIR
    img = cc.cyl_image(h, w)
    assert hip.cyl_warp_shape(cc.cyl_cfg(fa), w, h, hf)[:2] == hip.cyl_warp_shape(cc.cyl_cfg(fb), w, h, hf)[:2]
    want = {f: orc.cyl_warp(img, hf, NOPTS, cc.cyl_cfg(f))[0] for f in (fa, fb)}
    assert want[fa].shape == want[fb].shape and not np.array_equal(want[fa], want[fb])
    for f in (fa, fb, fa, fb):
        assert np.array_equal(_warp(ctx, cc.cyl_cfg(f), img, hf), want[f]), f


CROP_OF_WARP = [(67, 130, 1.0, 24, False), (40, 260, 1.3, 12, False), (64, 64, 0.5, 37, True)]


@pytest.mark.parametrize("h,w,hf,fl,holes", CROP_OF_WARP)
def test_crop_of_a_warped_image(ctx, orc, h, w, hf, fl, holes):
    """curved borders (and a hole): masks the blend cases do not produce, the first valid up to column 0"""
    from openpano_amd import hip
    img = cc.cyl_holes(h, w) if holes else cc.cyl_image(h, w)
    cfg = cc.cyl_cfg(fl)
    warped = orc.cyl_warp(img, hf, NOPTS, cfg)[0]
    want, off = orc.crop(warped)
    x0, y0, cw, ch, _ = cc.crop_model(cc.canvas_mask(warped))
    assert off == (x0, y0) and want.shape[:2] == (ch, cw) and want.size > warped.size // 4
    cv = hip.cyl_warp(ctx, cfg, img, hf)
    try:
        assert np.array_equal(cv.numpy(), warped)
        cropped, got_off = cv.crop()
        try:
            assert got_off == off and np.array_equal(cropped.numpy(), want)
            assert np.array_equal(cropped.numpy_u8(), orc.to_u8(want))
        finally:
            cropped.free()
    finally:
        cv.free()
