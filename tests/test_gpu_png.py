"""GPU: the device PNG encoder (openpano_amd/csrc/png.hip, C-ABI 12).

1. encode_png_u8 on every input of png_cases.CASES gives the bytes of the serial restatement (tests/harness/png_ref.c);
2. Canvas.png_bytes() for linear and multiband blends, flat / cylindrical / spherical, cropped and uncropped, decodes to
   exactly Canvas.numpy_u8() and equals encode_png_u8(numpy_u8());
3. two encodes of one canvas, and encodes on two contexts, give identical bytes;
4. stitch_demo --png writes a file that decodes to the quantised panorama of its own out.bin, and out.bin does not change;
5. hip_write_png from a C++ program: the Mat32f overload decodes to write_png's expression applied to the matrix, the
   op_canvas overload to the quantised device canvas;
6. an empty canvas is OP_ERR_INVALID and op_last_error() says why."""
import os
import struct
import subprocess

import numpy as np
import pytest

import png_cases
from openpano_amd import hip, synth
from openpano_amd.config import PanoConfig

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMO = os.path.join(ROOT, "openpano_amd", "host", "stitch_demo")


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return png_cases.build_ref(tmp_path_factory.mktemp("pngref"))


@pytest.mark.parametrize("name", list(png_cases.CASES))
def test_device_file_equals_reference(ctx, ref, name):
    rgb = png_cases.case(name)
    got = hip.encode_png_u8(ctx, rgb)
    want = png_cases.ref_encode(ref, rgb)
    if got != want:
        n = min(len(got), len(want))
        first = next((i for i in range(n) if got[i] != want[i]), n)
        pytest.fail(f"{name}: device {len(got)} bytes, reference {len(want)} bytes, first difference at byte {first}")


# (projection method, pano_scene kind, MULTIBAND)
BLENDS = [(0, "flat", 0), (1, "camera", 0), (2, "camera", 0), (0, "flat", 3), (1, "camera", 3), (2, "camera", 3)]


@pytest.mark.parametrize("proj,kind,multiband", BLENDS, ids=[f"proj{p}_mb{m}" for p, _, m in BLENDS])
def test_canvas_png(ctx, proj, kind, multiband):
    cfg = PanoConfig(MULTIBAND=multiband)
    views, homos = synth.pano_scene(3, 120, 160, seed=21 + proj, proj=kind)
    cv = hip.blend(ctx, cfg, views, homos, proj, 1)
    cropped, _ = cv.crop()
    try:
        for c in (cv, cropped):
            assert c.h > 0 and c.w > 0
            want = c.numpy_u8()
            png = c.png_bytes()
            d = png_cases.decode(png)
            assert (d["h"], d["w"]) == (c.h, c.w)
            assert np.array_equal(d["pixels"], want)
            assert png == hip.encode_png_u8(ctx, want)
        assert (cv.numpy() < 0).any()                       # the uncropped canvas has Color::NO background in it
    finally:
        cropped.free(); cv.free()


def test_deterministic_across_calls_and_contexts(ctx):
    cfg = PanoConfig()
    views, homos = synth.pano_scene(3, 120, 160, seed=5, proj="camera")
    cv = hip.blend(ctx, cfg, views, homos, 2, 1)
    a = cv.png_bytes(); b = cv.png_bytes()
    cv.free()
    other = hip.Context(0)
    try:
        cv2 = hip.blend(other, cfg, views, homos, 2, 1)
        c = cv2.png_bytes()
        cv2.free()
    finally:
        other.close()
    assert a == b and a == c
    rgb = png_cases.case("boundary_mid_pixel_150x333")
    assert hip.encode_png_u8(ctx, rgb) == hip.encode_png_u8(ctx, rgb.copy())


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


def test_stitch_demo_png(tmp_path):
    assert os.path.exists(DEMO), "build it: make -C openpano_amd/csrc"
    views, _, _ = synth.rotating_views(5, 300, 400, seed=77, step_deg=22.0)
    png_path = tmp_path / "out.png"
    plain = _run_demo(tmp_path, views, "plain", [])
    flagged = _run_demo(tmp_path, views, "png", ["--png", str(png_path)])
    assert flagged == plain
    H, W = struct.unpack_from("<2i", plain, 0)
    pano = np.frombuffer(plain, np.float32, count=H * W * 3, offset=8).reshape(H, W, 3)
    d = png_cases.decode(open(png_path, "rb").read())
    assert (d["h"], d["w"]) == (H, W)
    assert np.array_equal(d["pixels"], png_cases.quantise(pano))
    assert (pano < 0).any() and (pano >= 0).any()


def test_hip_write_png_from_cpp(tmp_path):
    exe = tmp_path / "png_write_selftest"
    lib_dir = os.path.join(ROOT, "openpano_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fopenmp", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(lib_dir, "host"),
                           "-o", str(exe), os.path.join(ROOT, "tests", "harness", "png_write_selftest.cc"),
                           "-L", lib_dir, "-lopenpano_hip", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib"])
    rng = np.random.default_rng(12)
    h, w = 97, 131
    mat = rng.uniform(0, 1, (h, w, 3)).astype(np.float32)
    mat[10:30, 40:90] = -1.0                                # Color::NO
    mat[0, 0] = (0.0, 1.0, 0.5)
    fin, fout = tmp_path / "mat.bin", tmp_path / "mat.png"
    cpng, cbin = tmp_path / "canvas.png", tmp_path / "canvas.bin"
    with open(fin, "wb") as f:
        f.write(struct.pack("<2i", h, w)); f.write(mat.tobytes())
    r = subprocess.run([str(exe), str(fin), str(fout), str(cpng), str(cbin)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    d = png_cases.decode(open(fout, "rb").read())
    want = png_cases.quantise(mat)
    assert (want[10:30, 40:90] == 255).all()
    assert np.array_equal(d["pixels"], want)
    # the overload that takes the device canvas (here: the matrix's cylinder pre-warp)
    raw = open(cbin, "rb").read()
    ch, cw = struct.unpack_from("<2i", raw, 0)
    canvas = np.frombuffer(raw, np.float32, count=ch * cw * 3, offset=8).reshape(ch, cw, 3)
    d = png_cases.decode(open(cpng, "rb").read())
    assert (d["h"], d["w"]) == (ch, cw) and (canvas < 0).any() and (canvas >= 0).any()
    assert np.array_equal(d["pixels"], png_cases.quantise(canvas))


def test_empty_canvas_is_invalid(ctx):
    cfg = PanoConfig()
    views, homos = synth.pano_scene(1, 60, 80, seed=3, proj="flat")
    nothing = [np.full_like(views[0], -1.0)]                # no valid pixel anywhere: crop() finds no rectangle
    cv = hip.blend(ctx, cfg, nothing, homos, 0, 0)
    empty, _ = cv.crop()
    try:
        assert empty.h == 0 or empty.w == 0
        with pytest.raises(hip.OpenPanoHipError, match=r"error -1: op_canvas_encode_png: empty canvas"):
            empty.png_bytes()
        with pytest.raises(hip.OpenPanoHipError, match=r"error -1: op_png_encode_u8: empty image"):
            hip.encode_png_u8(ctx, np.zeros((0, 5, 3), np.uint8))
    finally:
        empty.free(); cv.free()
