"""GPU: cylinder mode's perspective correction (k_canvas_perspective, csrc/canvas.hip) on the cases of tests/perspective_cases.py --
every canvas shape, content and homography, under ORDERED_INPUT 0 and 1 and LAZY_READ 0 and 1 -- bit-exact against the numpy
restatement perspective_ref, which test_perspective_cpu.py shows to be what it claims; the canvas upload round-trips; bad arguments
come back as errors before any device work."""
import numpy as np
import pytest

import perspective_cases as pc

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def ctx():
    from openpano_amd import hip
    c = hip.Context(0)
    yield c
    c.close()


def _cfg(ordered, lazy):
    from openpano_amd.config import PanoConfig
    # the pass reads ORDERED_INPUT and LAZY_READ only; the mode stays the default one, which allows ORDERED_INPUT 0 (main.cc:257-258)
    return PanoConfig(ORDERED_INPUT=ordered, LAZY_READ=lazy)


@pytest.mark.parametrize("case", pc.CASES, ids=[c.id for c in pc.CASES])
def test_perspective_case(ctx, case):
    from openpano_amd import hip
    src, inv = pc.canvas_of(case), pc.homography_of(case)
    cv = hip.Canvas.upload(ctx, src)
    try:
        assert (cv.h, cv.w) == (case.h, case.w)
        for ordered, lazy in pc.FLAGS:
            out = cv.perspective(inv, _cfg(ordered, lazy))
            try:
                got = out.numpy()
            finally:
                out.free()
            want = pc.perspective_ref(src, inv, ordered, lazy)
            assert got.shape == want.shape
            assert np.array_equal(got, want), (case.id, ordered, lazy, int((got != want).any(axis=2).sum()))
        assert np.array_equal(cv.numpy(), src)              # the source canvas is left as it was
    finally:
        cv.free()


def test_upload_round_trips(ctx):
    """bit for bit, Color::NO, -0, denormals and values outside [0, 1] included; the bytes are write_rgb's"""
    from openpano_amd import hip
    for h, w in pc.SHAPES + [(1, 1)]:
        v = np.random.default_rng(7 * h + w).random((h, w, 3), dtype=F)
        v.reshape(-1)[:: 5] = -1
        v.reshape(-1)[1:: 7] = np.array([-0.0, np.nextafter(F(0), F(1)), 1.0, 3.5, 1e-30], F)[np.arange(len(v.reshape(-1)[1:: 7])) % 5]
        cv = hip.Canvas.upload(ctx, v)
        try:
            got = cv.numpy()
            assert (cv.h, cv.w) == (h, w) and np.array_equal(got.view(np.uint32), v.view(np.uint32))
        finally:
            cv.free()


def test_bad_arguments(ctx):
    from openpano_amd import hip
    import ctypes as C
    L = hip.lib()
    before = hip.pool_stats()[:2]
    buf = np.zeros((2, 2, 3), F)
    out = C.c_void_p()
    for args in ((None, buf.ctypes.data_as(C.c_void_p), 2, 2, C.byref(out)), (ctx.handle, None, 2, 2, C.byref(out)),
                 (ctx.handle, buf.ctypes.data_as(C.c_void_p), 0, 2, C.byref(out)), (ctx.handle, buf.ctypes.data_as(C.c_void_p), 2, -1, C.byref(out)),
                 (ctx.handle, buf.ctypes.data_as(C.c_void_p), 2, 2, None)):
        assert L.op_canvas_upload(*args) == -1 and b"op_canvas_upload: bad argument" in L.op_last_error()
    with pytest.raises(ValueError):
        hip.Canvas.upload(ctx, np.zeros((4, 4), F))
    cv = hip.Canvas.upload(ctx, buf)
    try:
        live = hip.pool_stats()[:2]
        cfg = hip.OpConfig.from_config(_cfg(1, 0))
        eye = np.eye(3).reshape(9)
        p = eye.ctypes.data_as(C.c_void_p)
        for args in ((None, C.byref(cfg), cv.handle, p, C.byref(out)), (ctx.handle, None, cv.handle, p, C.byref(out)),
                     (ctx.handle, C.byref(cfg), None, p, C.byref(out)), (ctx.handle, C.byref(cfg), cv.handle, None, C.byref(out)),
                     (ctx.handle, C.byref(cfg), cv.handle, p, None)):
            assert L.op_canvas_perspective(*args) == -1 and b"op_canvas_perspective: bad argument" in L.op_last_error()
        for bad in (np.nan, np.inf, -np.inf):
            for k in (0, 4, 8):
                m = np.eye(3).reshape(9)
                m[k] = bad
                with pytest.raises(hip.OpenPanoHipError, match=r"error -1: op_canvas_perspective: inv\[%d\] is not finite" % k):
                    cv.perspective(m, _cfg(1, 0))
        assert hip.pool_stats()[:2] == live
        # and the context goes on working
        good = cv.perspective(np.eye(3), _cfg(1, 0))
        assert np.array_equal(good.numpy(), pc.perspective_ref(buf, np.eye(3), 1, 0))
        good.free()
    finally:
        cv.free()
    assert hip.pool_stats()[:2] == before
