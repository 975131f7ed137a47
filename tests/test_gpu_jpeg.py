"""GPU: the device JPEG encoder (openpano_amd/csrc/jpeg.hip).  The oracle is the serial restatement
tests/harness/jpeg_ref.c, whose files test_jpeg_ref_cpu.py holds equal to libjpeg's; nothing here needs Pillow's codec.

1. encode_jpeg_u8 on every input of jpeg_cases.CASES, at qualities 1, 50, 90, 100 and both samplings, gives the restatement's
   bytes; so does Canvas.jpeg_bytes() of an fp32 canvas made from the same input, against the restatement run on numpy_u8();
2. config 4's all-background 763 x 7999 canvas, once;
3. Canvas.jpeg_bytes() for linear and multiband blends, flat / cylindrical / spherical, cropped and uncropped;
4. two encodes of one canvas, and encodes on two contexts, give identical bytes;
5. bad quality / sampling and an empty canvas are OP_ERR_INVALID, 1 x 65536 is OP_ERR_UNSUPPORTED, and no pool block stays live;
6. stitch_demo --jpeg writes the restatement's file for the panorama of its own out.bin, and out.bin does not change;
7. hip_write_jpeg from a C++ program, both overloads."""
import os
import struct
import subprocess

import numpy as np
import pytest

import jpeg_cases as J
import png_cases
from openpano_amd import hip, synth
from openpano_amd.config import PanoConfig

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMO = os.path.join(ROOT, "openpano_amd", "host", "stitch_demo")
NAMES = {J.S444: "444", J.S420: "420"}


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return J.build_ref(tmp_path_factory.mktemp("jpegref"))


def _same(got, want, what):
    if got != want:
        n = min(len(got), len(want))
        first = next((i for i in range(n) if got[i] != want[i]), n)
        pytest.fail(f"{what}: device {len(got)} bytes, reference {len(want)} bytes, first difference at byte {first}")


@pytest.mark.parametrize("name", list(J.CASES))
def test_device_file_equals_reference(ctx, ref, name):
    rgb = J.case(name)
    for q in J.QUALITIES:
        for s in J.SUBSAMPLINGS:
            _same(hip.encode_jpeg_u8(ctx, rgb, q, s), J.ref_encode(ref, rgb, q, s), J.combo_id(name, q, s))
    assert hip.encode_jpeg_u8(ctx, rgb) == hip.encode_jpeg_u8(ctx, rgb, 90, "420")
    assert hip.encode_jpeg_u8(ctx, rgb, 50, "444") == hip.encode_jpeg_u8(ctx, rgb, 50, hip.JPEG_444)


@pytest.mark.parametrize("name", list(J.CASES))
def test_canvas_path_equals_reference(ctx, ref, name):
    """an fp32 canvas of the input's shape (the one-view flat blend of the input as fp32: interpolated content, a Color::NO
    border); the restatement runs on its quantisation.  op_blend takes no view below 2 x 2, so 1 x 1 is edge-padded to that."""
    rgb = J.case(name)
    view = ((rgb.astype(np.float32) + np.float32(0.5)) / np.float32(255)).astype(np.float32)
    view = np.pad(view, ((0, max(0, 2 - view.shape[0])), (0, max(0, 2 - view.shape[1])), (0, 0)), mode="edge")
    cv = hip.blend(ctx, PanoConfig(), [view], np.eye(3)[None], 0, 0)
    try:
        assert (cv.h, cv.w) == view.shape[:2]
        u8 = cv.numpy_u8()
        assert np.array_equal(u8, png_cases.quantise(cv.numpy()))
        for q in J.QUALITIES:
            for s in J.SUBSAMPLINGS:
                _same(cv.jpeg_bytes(q, NAMES[s]), J.ref_encode(ref, u8, q, s), "canvas " + J.combo_id(name, q, s))
    finally:
        cv.free()


def test_config4_canvas(ctx, ref):
    name, make, q, s = J.BIG
    rgb = make()
    got = hip.encode_jpeg_u8(ctx, rgb, q, s)
    _same(got, J.ref_encode(ref, rgb, q, s), name)
    assert len(J.walk(got)["intervals"]) == 3000


# (projection method, pano_scene kind, MULTIBAND)
BLENDS = [(0, "flat", 0), (1, "camera", 0), (2, "camera", 0), (0, "flat", 3), (1, "camera", 3), (2, "camera", 3)]


@pytest.mark.parametrize("proj,kind,multiband", BLENDS, ids=[f"proj{p}_mb{m}" for p, _, m in BLENDS])
def test_canvas_jpeg(ctx, ref, proj, kind, multiband):
    cfg = PanoConfig(MULTIBAND=multiband)
    views, homos = synth.pano_scene(3, 120, 160, seed=21 + proj, proj=kind)
    cv = hip.blend(ctx, cfg, views, homos, proj, 1)
    cropped, _ = cv.crop()
    try:
        for c in (cv, cropped):
            assert c.h > 0 and c.w > 0
            u8 = c.numpy_u8()
            jpg = c.jpeg_bytes()
            info = J.walk(jpg)
            assert (info["h"], info["w"], info["dri"]) == (c.h, c.w, J.RI[J.S420])
            _same(jpg, J.ref_encode(ref, u8, 90, J.S420), "default settings")
            _same(c.jpeg_bytes(100, "444"), J.ref_encode(ref, u8, 100, J.S444), "quality 100, 4:4:4")
            assert jpg == hip.encode_jpeg_u8(ctx, u8)
        assert (cv.numpy() < 0).any()                       # the uncropped canvas has Color::NO background in it
    finally:
        cropped.free(); cv.free()


def test_write_jpeg(ctx, tmp_path):
    views, homos = synth.pano_scene(3, 120, 160, seed=5, proj="flat")
    cv = hip.blend(ctx, PanoConfig(), views, homos, 0, 1)
    try:
        cv.write_jpeg(tmp_path / "a.jpg", quality=50, subsampling="444")
        assert open(tmp_path / "a.jpg", "rb").read() == cv.jpeg_bytes(50, "444")
    finally:
        cv.free()


def test_deterministic_across_calls_and_contexts(ctx):
    cfg = PanoConfig()
    views, homos = synth.pano_scene(3, 120, 160, seed=5, proj="camera")
    cv = hip.blend(ctx, cfg, views, homos, 2, 1)
    a = cv.jpeg_bytes(); b = cv.jpeg_bytes()
    cv.free()
    other = hip.Context(0)
    try:
        cv2 = hip.blend(other, cfg, views, homos, 2, 1)
        c = cv2.jpeg_bytes()
        cv2.free()
    finally:
        other.close()
    assert a == b and a == c
    rgb = J.case("marker_wrap_136x136")
    assert hip.encode_jpeg_u8(ctx, rgb, 100, "444") == hip.encode_jpeg_u8(ctx, rgb.copy(), 100, "444")


def test_bad_arguments_and_pool(ctx):
    rgb = J.case("17x33")
    views, homos = synth.pano_scene(1, 60, 80, seed=3, proj="flat")
    cv = hip.blend(ctx, PanoConfig(), views, homos, 0, 0)
    nothing = hip.blend(ctx, PanoConfig(), [np.full_like(views[0], -1.0)], homos, 0, 0)
    empty, _ = nothing.crop()                                # no valid pixel anywhere: crop() finds no rectangle
    before = hip.pool_stats()[:2]
    try:
        for q in (0, 101, -5):
            with pytest.raises(hip.OpenPanoHipError, match=r"error -1: op_jpeg_encode_u8: quality outside 1\.\.100"):
                hip.encode_jpeg_u8(ctx, rgb, q, "420")
            with pytest.raises(hip.OpenPanoHipError, match=r"error -1: op_canvas_encode_jpeg: quality outside 1\.\.100"):
                cv.jpeg_bytes(q)
        for s in (2, -1, 420):
            with pytest.raises(hip.OpenPanoHipError, match=r"error -1: op_jpeg_encode_u8: unknown subsampling"):
                hip.encode_jpeg_u8(ctx, rgb, 90, s)
            with pytest.raises(hip.OpenPanoHipError, match=r"error -1: op_canvas_encode_jpeg: unknown subsampling"):
                cv.jpeg_bytes(90, s)
        with pytest.raises(ValueError):
            cv.jpeg_bytes(90, "422")
        for shape in ((1, 65536, 3), (65536, 1, 3)):
            with pytest.raises(hip.OpenPanoHipError, match=r"op_jpeg_encode_u8: a JPEG frame header holds 16-bit dimensions") as e:
                hip.encode_jpeg_u8(ctx, np.zeros(shape, np.uint8))
            assert "error -4:" in str(e.value)                 # OP_ERR_UNSUPPORTED
        assert hip.pool_stats()[:2] == before                # refused before anything was allocated
        assert empty.h == 0 or empty.w == 0
        with pytest.raises(hip.OpenPanoHipError, match=r"error -1: op_canvas_encode_jpeg: empty image"):
            empty.jpeg_bytes()
        with pytest.raises(hip.OpenPanoHipError, match=r"error -1: op_jpeg_encode_u8: empty image"):
            hip.encode_jpeg_u8(ctx, np.zeros((0, 5, 3), np.uint8))
        # the widest and the tallest image the format holds
        for shape in ((1, 65535, 3), (65535, 1, 3)):
            assert len(J.walk(hip.encode_jpeg_u8(ctx, np.zeros(shape, np.uint8), 90, "444"))["intervals"]) == 256
        # a handle that is alive holds no device block, and after the calls above none is left live
        h = hip.C.c_void_p()
        hip.check(hip.lib().op_canvas_encode_jpeg(ctx.handle, cv.handle, 90, hip.JPEG_420, hip.C.byref(h)))
        assert hip.lib().op_jpeg_size(h) > 600
        hip.lib().op_jpeg_free(h)
        assert hip.pool_stats()[:2] == before
    finally:
        empty.free(); nothing.free(); cv.free()


def _run_demo(tmp_path, views, tag, extra):
    n = len(views); h, w, _ = views[0].shape
    fin, fout = tmp_path / "in.bin", tmp_path / f"out_{tag}.bin"
    with open(fin, "wb") as f:
        f.write(struct.pack("<3i", n, h, w))
        for v in views:
            f.write(np.ascontiguousarray(v, np.float32).tobytes())
    r = subprocess.run([DEMO, str(fin), str(fout), "42", "camera_build"] + extra, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return open(fout, "rb").read()


def test_stitch_demo_jpeg(ref, tmp_path):
    assert os.path.exists(DEMO), "build it: make -C openpano_amd/csrc"
    views, _, _ = synth.rotating_views(5, 300, 400, seed=77, step_deg=22.0)
    jpg_path, jpg444_path = tmp_path / "out.jpg", tmp_path / "out444.jpg"
    plain = _run_demo(tmp_path, views, "plain", [])
    flagged = _run_demo(tmp_path, views, "jpeg", ["--jpeg", str(jpg_path)])
    flagged444 = _run_demo(tmp_path, views, "jpeg444", ["--jpeg-444", "--jpeg", str(jpg444_path), "--jpeg-quality", "100"])
    assert flagged == plain and flagged444 == plain
    H, W = struct.unpack_from("<2i", plain, 0)
    pano = np.frombuffer(plain, np.float32, count=H * W * 3, offset=8).reshape(H, W, 3)
    assert (pano < 0).any() and (pano >= 0).any()
    u8 = png_cases.quantise(pano)
    _same(open(jpg_path, "rb").read(), J.ref_encode(ref, u8, 90, J.S420), "--jpeg")
    _same(open(jpg444_path, "rb").read(), J.ref_encode(ref, u8, 100, J.S444), "--jpeg --jpeg-quality 100 --jpeg-444")


def test_hip_write_jpeg_from_cpp(ref, tmp_path):
    exe = tmp_path / "jpeg_write_selftest"
    lib_dir = os.path.join(ROOT, "openpano_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fopenmp", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(lib_dir, "host"),
                           "-o", str(exe), os.path.join(ROOT, "tests", "harness", "jpeg_write_selftest.cc"),
                           "-L", lib_dir, "-lopenpano_hip", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib"])
    rng = np.random.default_rng(12)
    h, w = 97, 131
    mat = rng.uniform(0, 1, (h, w, 3)).astype(np.float32)
    mat[10:30, 40:90] = -1.0                                # Color::NO
    mat[0, 0] = (0.0, 1.0, 0.5)
    fin, fout = tmp_path / "mat.bin", tmp_path / "mat.jpg"
    cjpg, cbin = tmp_path / "canvas.jpg", tmp_path / "canvas.bin"
    with open(fin, "wb") as f:
        f.write(struct.pack("<2i", h, w)); f.write(mat.tobytes())
    r = subprocess.run([str(exe), str(fin), str(fout), str(cjpg), str(cbin)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    want = png_cases.quantise(mat)
    assert (want[10:30, 40:90] == 255).all()
    _same(open(fout, "rb").read(), J.ref_encode(ref, want, 90, J.S420), "hip_write_jpeg(Mat32f)")
    # the overload that takes the device canvas (here: the matrix's cylinder pre-warp)
    raw = open(cbin, "rb").read()
    ch, cw = struct.unpack_from("<2i", raw, 0)
    canvas = np.frombuffer(raw, np.float32, count=ch * cw * 3, offset=8).reshape(ch, cw, 3)
    assert (canvas < 0).any() and (canvas >= 0).any()
    _same(open(cjpg, "rb").read(), J.ref_encode(ref, png_cases.quantise(canvas), 100, J.S444), "hip_write_jpeg(op_canvas)")
