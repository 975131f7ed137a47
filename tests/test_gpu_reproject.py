"""GPU: the re-projection of a finished panorama (k_canvas_reproject, csrc/reproject.hip) on the cases of tests/reproject_cases.py --
every source shape and content, every output shape, planets, views, cube faces, with and without wrap -- bit-exact against the numpy
restatement, which test_reproject_cpu.py shows to be what it claims.  The view matrices are op_view_look's own, so the host
libm cannot enter.  Bad arguments come back as errors with the device pool unchanged; the result encodes like any canvas; and the
standalone C++ program gives the Python path's bytes."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import reproject_cases as rc

pytestmark = pytest.mark.gpu
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMO = os.path.join(ROOT, "openpano_amd", "host", "stitch_demo")


@pytest.fixture(scope="module")
def ctx():
    from openpano_amd import hip
    c = hip.Context(0)
    yield c
    c.close()


def _frame(f):
    from openpano_amd import hip
    return hip.OpPanoFrame(float(f[0]), float(f[1]), float(f[2]), float(f[3]), int(f[4]))


def _view_of(spec):
    """an OpViewSpec as the restatement takes it"""
    return (spec.out_h, spec.out_w, np.array(list(spec.rot), np.float64), np.float64(spec.focal))


def _run(cv, frame, spec):
    out = cv.reproject(_frame(frame), spec)
    try:
        assert (out.h, out.w) == (spec.out_h, spec.out_w)
        return out.numpy()
    finally:
        out.free()


def _same(got, want, what):
    assert got.shape == want.shape, what
    assert np.array_equal(got, want), (what, int((got != want).any(axis=2).sum()))


@pytest.mark.parametrize("content", rc.CONTENTS)
@pytest.mark.parametrize("hw", rc.SOURCES, ids=["%dx%d" % s for s in rc.SOURCES])
def test_reproject_cases(ctx, hw, content):
    from openpano_amd import hip
    src = rc.source_of(hw, content)
    cv = hip.Canvas.upload(ctx, src)
    sampled = 0
    try:
        for wrap in (0, 1):
            base = rc.frame_of(hw, wrap)
            for n in rc.PLANETS:
                got = _run(cv, base, hip.view_planet(n))
                _same(got, rc.planet_ref(src, n, wrap), ("planet", n, wrap))
                sampled += int((got[..., 0] >= 0).sum())
            for name, yaw, pitch, roll, hfov, frame in rc.looks_of(hw, wrap):
                for oh, ow in rc.OUTPUTS:
                    spec = hip.view_look(yaw, pitch, roll, hfov, ow, oh)
                    got = _run(cv, frame, spec)
                    _same(got, rc.rectilinear_ref(src, frame, _view_of(spec)), (name, oh, ow, wrap))
                    sampled += int((got[..., 0] >= 0).sum())
            for face in range(6):
                spec = hip.view_cube_face(face, rc.CUBE_N)
                assert np.array_equal(np.array(list(spec.rot)), np.array(rc.CUBE[face][0], np.float64)) and spec.focal == 0.5 * rc.CUBE_N
                got = _run(cv, base, spec)
                _same(got, rc.rectilinear_ref(src, base, _view_of(spec)), ("cube", face, wrap))
                sampled += int((got[..., 0] >= 0).sum())
        assert np.array_equal(cv.numpy(), src)                  # the source canvas is left as it was
    finally:
        cv.free()
    if content == "random":
        assert (sampled > 1000) == (hw[0] > 1)                  # a one-row source has no second tap row: every pixel is NO


def test_empty_source_gives_an_all_no_canvas(ctx):
    from openpano_amd import hip
    src = np.full((9, 12, 3), -1, F)                            # crop() of a canvas without a valid pixel is empty
    cv = hip.Canvas.upload(ctx, src)
    empty, _ = cv.crop()
    try:
        assert empty.h == 0 or empty.w == 0
        for spec in (hip.view_planet(7), hip.view_look(0, 0, 0, 1.0, 65, 5)):
            for wrap in (0, 1):
                got = _run(empty, rc.frame_of((9, 12), wrap), spec)
                assert got.shape == (spec.out_h, spec.out_w, 3) and (got == -1).all()
    finally:
        empty.free(); cv.free()


def test_bad_arguments_leave_the_pool_alone(ctx):
    from openpano_amd import hip
    L = hip.lib()
    src = rc.source_of((37, 53), "random")
    before = hip.pool_stats()[:2]
    cv = hip.Canvas.upload(ctx, src)
    try:
        live = hip.pool_stats()[:2]
        good_f, good_s = _frame(rc.frame_of((37, 53), 0)), hip.view_look(0, 0, 0, 1.0, 8, 8)
        out = C.c_void_p()
        for args in ((None, cv.handle, C.byref(good_f), C.byref(good_s), C.byref(out)), (ctx.handle, None, C.byref(good_f), C.byref(good_s), C.byref(out)),
                     (ctx.handle, cv.handle, None, C.byref(good_s), C.byref(out)), (ctx.handle, cv.handle, C.byref(good_f), None, C.byref(out)),
                     (ctx.handle, cv.handle, C.byref(good_f), C.byref(good_s), None)):
            assert L.op_canvas_reproject(*args) == -1 and b"op_canvas_reproject: bad argument" in L.op_last_error()

        def frame(**kw):
            f = _frame(rc.frame_of((37, 53), 0))
            for k, v in kw.items():
                setattr(f, k, v)
            return f

        def spec(**kw):
            s = hip.view_look(0, 0, 0, 1.0, 8, 8)
            for k, v in kw.items():
                if k.startswith("rot"):
                    s.rot[int(k[3:])] = v
                else:
                    setattr(s, k, v)
            return s
        bad = [(good_f, spec(mode=2), "unknown mode"), (good_f, spec(mode=-1), "unknown mode"), (good_f, spec(out_h=0), "size below 1"),
               (good_f, spec(out_w=-4), "size below 1"), (good_f, spec(mode=0, out_w=9), "planet is square"), (good_f, spec(focal=0.0), "focal"),
               (good_f, spec(focal=-2.0), "focal"), (good_f, spec(focal=np.nan), "not finite"), (good_f, spec(rot4=np.inf), "not finite"),
               (good_f, spec(rot8=np.nan), "not finite"), (frame(lon0=np.nan), good_s, "not finite"), (frame(lat0=-np.inf), good_s, "not finite"),
               (frame(step_lon=np.inf), good_s, "not finite"), (frame(step_lat=np.nan), good_s, "not finite"), (frame(step_lon=0.0), good_s, "step is zero"),
               (frame(step_lat=0.0), good_s, "step is zero"), (frame(step_lat=0.0, wrap=1), good_s, "step is zero"), (frame(wrap=2), good_s, "wrap is neither"),
               (frame(wrap=1, lon0=3.2), good_s, "lon0 outside"), (frame(wrap=1, lon0=-3.1415926535897936), good_s, "lon0 outside")]
        for f, s, what in bad:
            with pytest.raises(hip.OpenPanoHipError, match=r"error -1: op_canvas_reproject: .*" + what):
                cv.reproject(f, s)
        with pytest.raises(hip.OpenPanoHipError, match=r"error -4: op_canvas_reproject"):
            cv.reproject(good_f, spec(out_h=70000))
        assert hip.pool_stats()[:2] == live
        # a zero step_lon is fine under wrap, and the context goes on working
        ok_f = frame(step_lon=0.0, wrap=1)
        got = _run(cv, (ok_f.lon0, ok_f.lat0, 0.0, ok_f.step_lat, 1), good_s)
        _same(got, rc.rectilinear_ref(src, (ok_f.lon0, ok_f.lat0, 0.0, ok_f.step_lat, 1), _view_of(good_s)), "after the refusals")
        assert hip.pool_stats()[:2] == live
    finally:
        cv.free()
    assert hip.pool_stats()[:2] == before


def test_two_calls_agree_and_the_result_encodes(ctx):
    from openpano_amd import hip
    src = rc.source_of(rc.SPHERE, "hole")
    frame = _frame(rc.frame_of(rc.SPHERE, 1))
    cv = hip.Canvas.upload(ctx, src)
    try:
        for spec in (hip.view_planet(64), hip.view_look(0.4, 0.2, 0.1, 1.5, 130, 63), hip.view_cube_face(3, 32)):
            a, b = cv.reproject(frame, spec), cv.reproject(frame, spec)
            try:
                px = a.numpy()
                assert np.array_equal(px, b.numpy())
                u8 = (np.where(px < 0, F(1), px) * F(255)).astype(np.uint8)             # write_rgb's quantisation
                assert np.array_equal(a.numpy_u8(), u8)
                assert a.jpeg_bytes(90, "420") == hip.encode_jpeg_u8(ctx, u8, 90, "420")
                assert a.jpeg_bytes(75, "444") == hip.encode_jpeg_u8(ctx, u8, 75, "444")
                assert a.png_bytes() == hip.encode_png_u8(ctx, u8)
            finally:
                a.free(); b.free()
    finally:
        cv.free()


# ---- the standalone C++ program -------------------------------------------------------------------------------------------------
def _demo(args):
    assert os.path.exists(DEMO), "build it: make -C openpano_amd/csrc"
    r = subprocess.run([DEMO] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stderr


def _canvases(buf, offset, count):
    out = []
    for _ in range(count):
        h, w = struct.unpack_from("<2i", buf, offset)
        out.append(np.frombuffer(buf, F, h * w * 3, offset + 8).reshape(h, w, 3))
        offset += 8 + h * w * 3 * 4
    return out, offset


FACES = ("_px", "_nx", "_py", "_ny", "_pz", "_nz")


@pytest.mark.parametrize("wrap", (0, 1))
def test_stitch_demo_reproject_equals_the_python_path(ctx, tmp_path, wrap):
    from openpano_amd import hip
    src = rc.source_of(rc.SPHERE, "hole")
    f = rc.frame_of(rc.SPHERE, wrap)
    with open(tmp_path / "pano.bin", "wb") as fo:
        fo.write(struct.pack("<2i", *src.shape[:2]) + src.tobytes())
    common = ["--frame", ",".join(float(v).hex() for v in f[:4])] + (["--wrap"] if wrap else [])
    cv = hip.Canvas.upload(ctx, src)
    try:
        _demo([tmp_path / "pano.bin", tmp_path / "planet.bin", 0, "reproject", "--planet", 64, "--png", tmp_path / "planet.png",
               "--jpeg", tmp_path / "planet.jpg"] + common)
        want = cv.reproject(_frame(f), hip.view_planet(64))
        (got,), end = _canvases(open(tmp_path / "planet.bin", "rb").read(), 0, 1)
        assert end == os.path.getsize(tmp_path / "planet.bin")
        assert got.tobytes() == want.numpy().tobytes()
        assert open(tmp_path / "planet.png", "rb").read() == want.png_bytes() and open(tmp_path / "planet.jpg", "rb").read() == want.jpeg_bytes()
        want.free()
        _demo([tmp_path / "pano.bin", tmp_path / "cube.bin", 0, "reproject", "--cube", 8, "--png", tmp_path / "cube.png"] + common)
        faces, end = _canvases(open(tmp_path / "cube.bin", "rb").read(), 0, 6)
        assert end == os.path.getsize(tmp_path / "cube.bin")
        for k, got in enumerate(faces):
            want = cv.reproject(_frame(f), hip.view_cube_face(k, 8))
            assert got.tobytes() == want.numpy().tobytes(), k
            assert open(tmp_path / ("cube%s.png" % FACES[k]), "rb").read() == want.png_bytes(), k
            want.free()
        _demo([tmp_path / "pano.bin", tmp_path / "view.bin", 0, "reproject", "--view", "0.4,0.2,0.1,1.5,130x63"] + common)
        (got,), _ = _canvases(open(tmp_path / "view.bin", "rb").read(), 0, 1)
        want = cv.reproject(_frame(f), hip.view_look(0.4, 0.2, 0.1, 1.5, 130, 63))
        assert got.tobytes() == want.numpy().tobytes()
        want.free()
    finally:
        cv.free()


def test_stitch_demo_build_then_view_stays_on_the_device(tmp_path):
    """camera_build --cube: the panorama of HipStitcher::build_canvas, the frame HipStitcher::pano_frame reports for it, and the
    six faces, which are the restatement's for that panorama and frame"""
    from openpano_amd import synth
    n, h, w = 5, 300, 400
    views, _, _ = synth.rotating_views(n, h, w, seed=77, step_deg=22.0)
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("<3i", n, h, w))
        for v in views:
            f.write(np.ascontiguousarray(v, F).tobytes())
    err = _demo([tmp_path / "in.bin", tmp_path / "out.bin", 42, "camera_build", "--cube", 16, "--jpeg", tmp_path / "face.jpg"])
    m = re.search(r"Frame: (\S+) (\S+) (\S+) (\S+) (\d)", err)
    assert m, err[-1000:]
    frame = tuple(float.fromhex(m.group(k)) for k in range(1, 5)) + (int(m.group(5)),)
    assert frame[4] == 0 and -np.pi < frame[0] < 0 and frame[2] > 0 and frame[3] > 0
    buf = open(tmp_path / "out.bin", "rb").read()
    (pano,), at = _canvases(buf, 0, 1)
    assert pano.shape[0] > 150 and pano.shape[1] > 600
    faces, end = _canvases(buf, at, 6)
    assert end == len(buf)
    for k, got in enumerate(faces):
        want = rc.rectilinear_ref(pano, frame, rc.cube_view(k, 16))
        assert np.array_equal(got, want), k
        assert os.path.getsize(tmp_path / ("face%s.jpg" % FACES[k])) > 100
    assert (faces[4][..., 0] >= 0).mean() > 0.2                  # +z looks at the middle of the sweep
    assert (faces[5] == -1).all()                               # and -z away from it
