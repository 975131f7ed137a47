"""GPU: the device JPEG decoder (openpano_amd/csrc/jpeg_dec.hip).  The oracle is the serial restatement
tests/harness/jpeg_dec_ref.c, which test_jpeg_dec_cpu.py holds equal to libjpeg; nothing here needs Pillow.

1. Views.decode_jpeg equals the restatement for every fixture of tests/golden/jpeg_dec, one at a time and all in one batch,
   at subsequences of 32 and 64 bits and at the default;
2. a fixture with more subsequences than the workgroup has threads, and several rounds;
3. files of the project's own serial encoder (jpeg_cases), with restart intervals and as unbroken scans;
4. encode_jpeg_u8 -> decode_jpeg -> sift_batch / blend equals the same from Views.upload of the restatement's bytes;
5. two decodes and two contexts agree;
6. three corrupt streams are OP_ERR_INVALID, the context goes on decoding, no pool block stays live; a refusal in the middle
   of a batch names its index and allocates nothing;
7. op_views_copy returns uploaded fp32 and byte views;
8. stitch_demo --jpeg-list equals a run on in.bin of the same pixels."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import jpeg_cases as J
import jpeg_dec_cases as D
from openpano_amd import hip, synth
from openpano_amd.config import PanoConfig

pytestmark = pytest.mark.gpu
DEMO = os.path.join(D.ROOT, "openpano_amd", "host", "stitch_demo")


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return D.build_ref(tmp_path_factory.mktemp("jpegdecref"))


@pytest.fixture(scope="module")
def decoded(ref):
    """the restatement's pixels of every fixture, computed once and shared"""
    out = {n: D.ref_decode(ref, D.data(n)) for n in D.NAMES}
    for n in D.NAMES:
        assert D.digest(out[n]) == D.DIGESTS[n]["sha256"], n
        out[n].setflags(write=False)
    return out


def _decode(ctx, files):
    v = hip.Views.decode_jpeg(ctx, files)
    try:
        assert v.count == len(files)
        return [v.numpy(i) for i in range(v.count)]
    finally:
        v.free()


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == np.uint8, (what, got.shape, want.shape)
    diff = np.argwhere(got != want)
    assert len(diff) == 0, (what, len(diff), diff[:3].tolist())


@pytest.mark.parametrize("bits", [0, 32, 64], ids=["default", "S32", "S64"])
def test_every_fixture(ctx, decoded, bits):
    ctx.set_jpeg_subseq_bits(bits)
    try:
        for n in D.NAMES:
            _same(_decode(ctx, [D.data(n)])[0], decoded[n], (n, bits))
        batch = _decode(ctx, [D.data(n) for n in D.NAMES])      # mixed sizes and samplings in one call
        for n, got in zip(D.NAMES, batch):
            _same(got, decoded[n], ("batch", n, bits))
    finally:
        ctx.set_jpeg_subseq_bits(0)
    for bad in (-32, 16, 48, 65536 + 32):
        with pytest.raises(hip.OpenPanoHipError, match="error -1: op_debug_set_jpeg_subseq_bits"):
            ctx.set_jpeg_subseq_bits(bad)


def test_more_subsequences_than_threads(ctx, decoded):
    name = "natural_400x600_q90_420"
    jpg = D.data(name)
    b0, e = D.scan_range(jpg)
    assert (e - b0) * 8 // 32 > 4 * 1024                    # k_jd_sync's 1024 threads stride over the subsequences
    ctx.set_jpeg_subseq_bits(32)
    try:
        _same(_decode(ctx, [jpg])[0], decoded[name], name)
        assert ctx.jpeg_last_rounds() > 1
        _same(_decode(ctx, [D.data("size_37x53_444")])[0], decoded["size_37x53_444"], "37 x 53 at 32 bits")
        assert ctx.jpeg_last_rounds() > 1                   # hundreds of subsequences, several rounds
    finally:
        ctx.set_jpeg_subseq_bits(0)


def _own_encoder(tmpdir, flags):
    """tests/harness/jpeg_ref.c (the project's serial ENCODER), optionally with other restart intervals"""
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("gcc not available")
    so = os.path.join(str(tmpdir), "libjpeg_enc_%d.so" % len(flags))
    subprocess.check_call([gcc, "-std=c11", "-O2", "-Wall", "-fPIC", "-shared", *flags, J.HARNESS, "-o", so])
    L = C.CDLL(so)
    L.jpeg_ref_bound.restype = C.c_long
    L.jpeg_ref_bound.argtypes = [C.c_int, C.c_int, C.c_int]
    L.jpeg_ref_encode.restype = C.c_long
    L.jpeg_ref_encode.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_long]
    return L


def test_files_of_the_projects_encoder(ctx, ref, tmp_path):
    with_rst = _own_encoder(tmp_path, ())
    unbroken = _own_encoder(tmp_path, ("-DOP_JPEG_RI_444=512", "-DOP_JPEG_RI_420=512"))      # above 136 x 136's 289 / 81 MCUs
    files = []
    for name in ("17x33", "chroma_bottom_40x56", "marker_wrap_136x136"):
        rgb = J.case(name)
        if name == "17x33":
            rgb = np.ascontiguousarray(rgb[:, :17])
        for q in (1, 100):
            for s in J.SUBSAMPLINGS:
                a, b = J.ref_encode(with_rst, rgb, q, s), J.ref_encode(unbroken, rgb, q, s)
                assert (b"\xff\xdd" in a[:700]) and a != b and b"\xff\xd0" not in b[623:]
                files += [a, b]
    want = [D.ref_decode(ref, f) for f in files]
    for f, w in zip(files, want):
        _same(_decode(ctx, [f])[0], w, "own encoder, alone")
    for got, w in zip(_decode(ctx, files), want):
        _same(got, w, "own encoder, batch")


def test_round_trip_feeds_sift_and_blend(ctx, ref):
    cfg = PanoConfig()
    views, homos = synth.pano_scene(3, 120, 160, seed=5, proj="flat")
    u8 = [np.ascontiguousarray((np.clip(v, 0, 1) * 255).astype(np.uint8)) for v in views]
    files = [hip.encode_jpeg_u8(ctx, a, 90, "420") for a in u8]
    want = [D.ref_decode(ref, f) for f in files]
    dv = hip.Views.decode_jpeg(ctx, files)
    uv = hip.Views.upload(ctx, want)
    try:
        assert dv.images()[0][1:] == uv.images()[0][1:] and dv.images()[0][3] == "u8"
        fa, fb = hip.sift_batch(ctx, cfg, dv.images()), hip.sift_batch(ctx, cfg, uv.images())
        try:
            for i in range(3):
                (da, ca), (db, cb) = fa.get(i), fb.get(i)
                assert len(da) > 20 and np.array_equal(da, db) and np.array_equal(ca, cb)
        finally:
            fa.free(); fb.free()
        ca, cb = hip.blend(ctx, cfg, dv, homos, 0, 1), hip.blend(ctx, cfg, uv, homos, 0, 1)
        try:
            assert np.array_equal(ca.numpy(), cb.numpy())
        finally:
            ca.free(); cb.free()
    finally:
        dv.free(); uv.free()


def test_deterministic_across_calls_and_contexts(ctx, decoded):
    names = ["natural_400x600_q50_422", "rst3_37x53_444", "grey_37x53"]
    files = [D.data(n) for n in names]
    a = _decode(ctx, files); b = _decode(ctx, files)
    other = hip.Context(0)
    try:
        c = _decode(other, files)
    finally:
        other.close()
    for n, x, y, z in zip(names, a, b, c):
        _same(x, decoded[n], n)
        assert np.array_equal(x, y) and np.array_equal(x, z)


def test_corrupt_streams_and_pool(ctx, decoded):
    good = D.data("size_17x17_420")
    _decode(ctx, [good])
    before = hip.pool_stats()[:2]
    for what in D.CORRUPT:
        bad, _ = D.corrupt(what)
        for files in ([bad], [good, bad, good]):
            with pytest.raises(hip.OpenPanoHipError, match=rf"error -1: op_views_decode_jpeg: file {len(files) // 2}: ") as e:
                hip.Views.decode_jpeg(ctx, files)
            assert hip.pool_stats()[:2] == before, (what, str(e.value))
        _same(_decode(ctx, [good])[0], decoded["size_17x17_420"], "after " + what)
    assert hip.pool_stats()[:2] == before


def test_refusal_in_a_batch_names_its_index(ctx):
    good = D.data("size_17x17_420")
    before = hip.pool_stats()
    with pytest.raises(hip.OpenPanoHipError, match=r"error -4: op_views_decode_jpeg: file 2: progressive JPEG") as e:
        hip.Views.decode_jpeg(ctx, [good, good, D.data("progressive_37x53"), good])
    assert hip.pool_stats() == before, str(e.value)         # nothing allocated, nothing returned to the cache either
    with pytest.raises(hip.OpenPanoHipError, match=r"error -1: op_views_decode_jpeg: file 1: .*EOI"):
        hip.Views.decode_jpeg(ctx, [good, D.patched(good, "no_eoi")])
    with pytest.raises(hip.OpenPanoHipError, match=r"error -1: op_views_decode_jpeg: bad argument"):
        hip.Views.decode_jpeg(ctx, [])
    assert hip.pool_stats() == before


def test_views_copy(ctx):
    rng = np.random.default_rng(3)
    f32 = rng.uniform(0, 1, (31, 47, 3)).astype(np.float32)
    u8 = rng.integers(0, 256, (20, 33, 3), dtype=np.uint8)
    v = hip.Views.upload(ctx, [f32, u8, f32[:9, :5].copy()])
    try:
        a, b, c = v.numpy(0), v.numpy(1), v.numpy(2)
        assert a.dtype == np.float32 and np.array_equal(a, f32)
        assert b.dtype == np.uint8 and np.array_equal(b, u8)
        assert np.array_equal(c, f32[:9, :5])
        with pytest.raises(hip.OpenPanoHipError, match="error -1: op_views_image"):
            v.numpy(3)
    finally:
        v.free()


def test_stitch_demo_jpeg_list(ctx, ref, tmp_path):
    assert os.path.exists(DEMO), "build it: make -C openpano_amd/csrc"
    views, _, _ = synth.rotating_views(5, 300, 400, seed=77, step_deg=22.0)
    u8 = [np.ascontiguousarray((np.clip(v, 0, 1) * 255).astype(np.uint8)) for v in views]
    paths = []
    for i, a in enumerate(u8):
        p = tmp_path / f"view{i}.jpg"
        p.write_bytes(hip.encode_jpeg_u8(ctx, a, 95, "444" if i % 2 else "420"))
        paths.append(str(p))
    (tmp_path / "list.txt").write_text("\n".join(paths) + "\n")
    pixels = [D.ref_decode(ref, open(p, "rb").read()) for p in paths]
    n = len(pixels); h, w, _ = pixels[0].shape
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("<3i", n, h, w))
        for a in pixels:
            f.write((a.astype(np.float32) / np.float32(255.0)).astype(np.float32).tobytes())
    outs = []
    for tag, extra in (("bin", ["--resident-views"]), ("jpeg", ["--jpeg-list", str(tmp_path / "list.txt")])):
        fout = tmp_path / f"out_{tag}.bin"
        r = subprocess.run([DEMO, str(tmp_path / "in.bin"), str(fout), "42", "camera_build"] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(open(fout, "rb").read())
    H, W = struct.unpack_from("<2i", outs[0], 0)
    assert H > 100 and W > 400 and outs[0] == outs[1]
