"""CPU: the additive C-ABI of resident views (op_views_*, still ABI 12), its argument checks -- made before any device
work, so they run without a GPU -- and the byte -> float conversion the sampler uses."""
from openpano_amd.hip import Views          # the module needs the feature: without it, it fails here

import ctypes as C

import numpy as np

from openpano_amd import hip

OP_ERR_INVALID = -1


def test_symbols_and_abi_version():
    L = hip.lib()
    for name in ("op_views_upload", "op_views_count", "op_views_image", "op_views_blend_image", "op_views_free"):
        assert hasattr(L, name), name
    assert L.op_abi_version() == 12
    assert (hip.OP_SRC_DEVICE, hip.OP_SRC_U8) == (1, 2)
    assert all(hasattr(Views, m) for m in ("upload", "images", "blend_images", "free"))


def test_null_arguments_are_invalid():
    L = hip.lib()
    img = (hip.OpImage * 1)()
    out = C.c_void_p()
    assert L.op_views_upload(None, img, 1, C.byref(out)) == OP_ERR_INVALID and not out
    assert b"op_views_upload" in L.op_last_error()
    fake_ctx = C.c_void_p(8)                     # never dereferenced: every check below precedes the first use of the context
    assert L.op_views_upload(fake_ctx, None, 1, C.byref(out)) == OP_ERR_INVALID
    assert L.op_views_upload(fake_ctx, img, 0, C.byref(out)) == OP_ERR_INVALID
    assert L.op_views_upload(fake_ctx, img, 1, None) == OP_ERR_INVALID
    assert L.op_views_upload(fake_ctx, img, 1, C.byref(out)) == OP_ERR_INVALID       # NULL data
    px = np.zeros((4, 4, 3), np.uint8)
    for h, w, on_device, dtype in ((1, 4, 0, 1), (4, 1, 0, 1), (4, 4, 0, 2), (4, 4, 0, -1), (4, 4, 2, 1)):
        img[0] = hip.OpImage(px.ctypes.data_as(C.c_void_p), h, w, on_device, dtype)
        assert L.op_views_upload(fake_ctx, img, 1, C.byref(out)) == OP_ERR_INVALID, (h, w, on_device, dtype)
    assert not out
    assert L.op_views_count(None) == OP_ERR_INVALID
    one, bl = hip.OpImage(), hip.OpBlendImage()
    assert L.op_views_image(None, 0, C.byref(one)) == OP_ERR_INVALID
    assert L.op_views_blend_image(None, 0, C.byref(bl)) == OP_ERR_INVALID
    L.op_views_free(None)                        # a no-op


def test_byte_conversions_equal_the_division():
    """read_img: (float)((double)b / 255.0).  The sampler multiplies by the double 1.0 / 255.0 instead; the fp32 division
    is the other exact form.  The fp32 multiply by 1.f / 255.f is NOT one (so it must never be used)."""
    b = np.arange(256)
    ref = (b.astype(np.float64) / 255.0).astype(np.float32)
    assert np.array_equal((b.astype(np.float64) * (1.0 / 255.0)).astype(np.float32), ref)       # csrc/blend_sample.hpp: byte_pixel
    assert np.array_equal(b.astype(np.float32) / np.float32(255.0), ref)
    bad = b.astype(np.float32) * (np.float32(1.0) / np.float32(255.0))
    assert (bad != ref).sum() == 126
