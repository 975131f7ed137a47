"""GPU: JPEG views decoded upright by their EXIF orientation (op_views_decode_jpeg_oriented, k_jd_rgb_oriented in
openpano_amd/csrc/jpeg_dec.hip).  The expected views are always the serial restatement's decode
(tests/harness/jpeg_dec_ref.c, which test_jpeg_dec_cpu.py holds equal to libjpeg) put through exif_craft.orient_map, the
table of the header restated with numpy index arrays.  Nothing here needs Pillow.

1. every decodable fixture of tests/golden/jpeg_dec x orientations 1..8 given explicitly, one file per call;
2. tile seams: files of the project's serial encoder with heights and widths T-1, T, T+1, 2T+1 in every combination (T read from
   the kernel's source), random pixels, 4:2:0 and 4:4:4, orientations 2..8;
3. a mixed batch whose files carry EXIF orientations 1..8 and two junk blocks, with orientation = [0, ...] and NULL, at
   subsequences of 32 bits and the default; an explicit 6 over an EXIF 3;
4. orientations all 1: byte for byte op_views_decode_jpeg, and k_jd_rgb_oriented is not launched;
5. decode_jpeg(orient=True) -> sift_batch / blend equals Views.upload of the turned bytes bit for bit; op_views_image and
   op_views_copy report the turned shape;
6. orientations -1 and 9 are OP_ERR_INVALID with a message and allocate nothing;
7. a corrupt file mid-batch names its index, and the context decodes a good oriented batch afterwards;
8. two decodes and two contexts agree;
9. the C++ layers: hip_read_jpeg_views(.., true) and hip_jpeg_exif from a stand-alone program, stitch_demo --jpeg-list --jpeg-orient."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import exif_craft as X
import jpeg_cases as J
import jpeg_dec_cases as D
from openpano_amd import hip, synth
from openpano_amd.config import PanoConfig

pytestmark = pytest.mark.gpu
DEMO = os.path.join(D.ROOT, "openpano_amd", "host", "stitch_demo")
KERNEL = os.path.join(D.CSRC, "jpeg_dec.hip")
ORIENTED_LABEL = "k_jd_rgb_oriented"
INVERSE = {1: 1, 2: 2, 3: 3, 4: 4, 5: 5, 6: 8, 7: 7, 8: 6}      # orient_map(orient_map(s, o), INVERSE[o]) == s


def tile():
    """the tile of the stored frame a workgroup of k_jd_rgb_oriented owns, read from the kernel's source"""
    return int(re.search(r"#define JD_OT (\d+)", open(KERNEL).read()).group(1))


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return D.build_ref(tmp_path_factory.mktemp("jpegorientref"))


@pytest.fixture(scope="module")
def enc(tmp_path_factory):
    return J.build_ref(tmp_path_factory.mktemp("jpegorientenc"))


@pytest.fixture(scope="module")
def decoded(ref):
    """the restatement's pixels of every fixture, computed once and shared"""
    out = {n: D.ref_decode(ref, D.data(n)) for n in D.NAMES}
    for n in D.NAMES:
        assert D.digest(out[n]) == D.DIGESTS[n]["sha256"], n
        out[n].setflags(write=False)
    return out


@pytest.fixture(scope="module")
def seam_files(ref, enc):
    """{sampling: [(file, the restatement's pixels)]} for every height x width of T-1, T, T+1, 2T+1"""
    T = tile()
    sizes = (T - 1, T, T + 1, 2 * T + 1)
    rng = np.random.default_rng(2024)
    out = {}
    for s in J.SUBSAMPLINGS:
        out[s] = []
        for h in sizes:
            for w in sizes:
                f = J.ref_encode(enc, rng.integers(0, 256, (h, w, 3), dtype=np.uint8), 90, s)
                px = D.ref_decode(ref, f)
                assert px.shape == (h, w, 3) and len({X.orient_map(px, o).tobytes() for o in range(1, 9)}) == 8
                px.setflags(write=False)
                out[s].append((f, px))
    return out


def _decode(ctx, files, orient):
    v = hip.Views.decode_jpeg(ctx, files, orient=orient)
    try:
        assert v.count == len(files)
        return [v.numpy(i) for i in range(v.count)]
    finally:
        v.free()


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == np.uint8, (what, got.shape, want.shape)
    diff = np.argwhere(got != want)
    assert len(diff) == 0, (what, len(diff), diff[:3].tolist())


def test_map_has_an_inverse():
    s = np.random.default_rng(1).integers(0, 256, (5, 7, 3), dtype=np.uint8)
    for o in range(1, 9):
        assert np.array_equal(X.orient_map(X.orient_map(s, o), INVERSE[o]), s)


@pytest.mark.parametrize("o", range(1, 9))
def test_every_fixture_alone(ctx, decoded, o):
    for n in D.NAMES:
        _same(_decode(ctx, [D.data(n)], [o])[0], X.orient_map(decoded[n], o), (n, o))


@pytest.mark.parametrize("o", range(2, 9))
@pytest.mark.parametrize("s", J.SUBSAMPLINGS, ids=["444", "420"])
def test_tile_seams(ctx, seam_files, s, o):
    files = [f for f, _ in seam_files[s]]
    assert len(files) == 16
    for got, (_, px) in zip(_decode(ctx, files, [o] * len(files)), seam_files[s]):
        _same(got, X.orient_map(px, o), (px.shape, s, o))


def _mixed(decoded):
    """files of mixed sizes and samplings that carry EXIF orientations 1..8, written eight different ways, and two junk blocks"""
    names = ["size_37x53_420", "size_40x56_420", "grey_37x53", "natural_400x600_q50_422", "size_9x9_422", "rst3_37x53_444",
             "size_17x17_420", "size_37x53_444", "size_8x8_444", "size_37x53_422"]
    how = ["II_short", "MM_long", "II_focal_sub", "MM_focal_ifd0", "orient_last", "orient_first", "II_long", "MM_short"]
    files, want, exif = [], [], []
    for k, n in enumerate(names):
        assert n in decoded, n
        if k < 8:
            f, (o, _) = X.WELL_FORMED[how[k]](D.data(n), k + 1, 35)
            assert o == k + 1
        else:
            f, (o, _) = X.JUNK[("ifd_offset_past", "orientation_9")[k - 8]](D.data(n), 6, 35)
            assert o == 1
        files.append(f); want.append(X.orient_map(decoded[n], o)); exif.append(o)
    return names, files, want, exif


@pytest.mark.parametrize("bits", [32, 0], ids=["S32", "default"])
def test_mixed_batch(ctx, decoded, bits):
    names, files, want, exif = _mixed(decoded)
    assert [hip.jpeg_exif(f)[0] for f in files] == exif
    ctx.set_jpeg_subseq_bits(bits)
    try:
        zeros = _decode(ctx, files, [0] * len(files))
        null = _decode(ctx, files, True)
        given = _decode(ctx, files, exif)
    finally:
        ctx.set_jpeg_subseq_bits(0)
    for n, a, b, c, w in zip(names, zeros, null, given, want):
        _same(a, w, ("orientation 0", n, bits)); _same(b, w, ("NULL", n, bits)); _same(c, w, ("explicit", n, bits))
    # an explicit orientation wins over the file's
    k = 2
    assert exif[k] == 3
    over = [0] * len(files); over[k] = 6
    got = _decode(ctx, files, over)
    _same(got[k], X.orient_map(decoded[names[k]], 6), "6 over EXIF 3")
    _same(got[k + 1], want[k + 1], "its neighbour")


def test_all_ones_is_the_plain_decode(ctx, decoded):
    names = ["size_37x53_420", "natural_400x600_q90_420", "grey_37x53", "size_2x2_444"]
    plain_files = [D.data(n) for n in names]
    tagged = [X.with_orientation(f, 1, order) for f, order in zip(plain_files, ("II", "MM", "II", "MM"))]
    plain = _decode(ctx, plain_files, False)
    ctx.set_profiling(True)
    try:
        for files, orient in ((plain_files, True), (plain_files, [1] * 4), (tagged, True), (tagged, [0, 1, 0, 1])):
            ctx.profile_reset()
            got = _decode(ctx, files, orient)
            labels = ctx.profile()
            assert "jpegdec rgb" in labels and not any(ORIENTED_LABEL in k for k in labels), sorted(labels)
            for n, a, b in zip(names, got, plain):
                _same(a, b, n); _same(a, decoded[n], n)
        ctx.profile_reset()
        _decode(ctx, plain_files, [1, 1, 2, 1])
        labels = ctx.profile()
        assert any(ORIENTED_LABEL in k for k in labels) and "jpegdec rgb" not in labels, sorted(labels)
    finally:
        ctx.set_profiling(False)


def test_oriented_views_feed_sift_and_blend(ctx, ref):
    cfg = PanoConfig()
    views, homos = synth.pano_scene(4, 120, 160, seed=5, proj="flat")
    u8 = [np.ascontiguousarray((np.clip(v, 0, 1) * 255).astype(np.uint8)) for v in views]
    orient = [6, 3, 8, 2]
    files = [X.with_orientation(hip.encode_jpeg_u8(ctx, X.orient_map(a, INVERSE[o]), 90, "420"), o) for a, o in zip(u8, orient)]
    want = [X.orient_map(D.ref_decode(ref, f), o) for f, o in zip(files, orient)]
    assert [w.shape for w in want] == [(120, 160, 3)] * 4
    dv = hip.Views.decode_jpeg(ctx, files, orient=True)
    uv = hip.Views.upload(ctx, want)
    try:
        for i in range(4):
            assert dv.images()[i][1:] == uv.images()[i][1:] == (120, 160, "u8")      # op_views_image: the turned shape
            _same(dv.numpy(i), want[i], ("op_views_copy", i))
        fa, fb = hip.sift_batch(ctx, cfg, dv.images()), hip.sift_batch(ctx, cfg, uv.images())
        try:
            for i in range(4):
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
    # a lone portrait view: 53 x 37 where the stored frame is 37 x 53
    pv = hip.Views.decode_jpeg(ctx, [D.data("size_37x53_420")], orient=[6])
    try:
        assert pv.images()[0][1:] == (53, 37, "u8") and pv.numpy(0).shape == (53, 37, 3)
    finally:
        pv.free()


def test_refusals_allocate_nothing(ctx):
    good = D.data("size_17x17_420")
    _decode(ctx, [good], [6])
    before = hip.pool_stats()
    for bad in (-1, 9):
        with pytest.raises(hip.OpenPanoHipError, match=rf"error -1: op_views_decode_jpeg_oriented: file 1: orientation {bad} ") as e:
            hip.Views.decode_jpeg(ctx, [good, good, good], orient=[6, bad, 0])
        assert hip.pool_stats() == before, str(e.value)
    with pytest.raises(hip.OpenPanoHipError, match=r"error -4: op_views_decode_jpeg_oriented: file 1: progressive JPEG"):
        hip.Views.decode_jpeg(ctx, [good, D.data("progressive_37x53")], orient=True)
    with pytest.raises(hip.OpenPanoHipError, match=r"error -1: op_views_decode_jpeg_oriented: bad argument"):
        hip.Views.decode_jpeg(ctx, [], orient=True)
    assert hip.pool_stats() == before


def test_corrupt_file_mid_batch(ctx, decoded):
    name = "size_17x17_420"
    good = X.with_orientation(D.data(name), 6)
    _decode(ctx, [good], True)
    before = hip.pool_stats()[:2]
    for what in D.CORRUPT:
        bad = X.with_orientation(D.corrupt(what)[0], 5)
        with pytest.raises(hip.OpenPanoHipError, match=r"error -1: op_views_decode_jpeg_oriented: file 1: ") as e:
            hip.Views.decode_jpeg(ctx, [good, bad, good], orient=True)
        assert hip.pool_stats()[:2] == before, (what, str(e.value))
        for got in _decode(ctx, [good, good], True):
            _same(got, X.orient_map(decoded[name], 6), "after " + what)
    assert hip.pool_stats()[:2] == before


def test_deterministic_across_calls_and_contexts(ctx, decoded):
    names = ["natural_400x600_q50_422", "rst3_37x53_444", "grey_37x53"]
    orient = [5, 6, 7]
    files = [D.data(n) for n in names]
    a = _decode(ctx, files, orient); b = _decode(ctx, files, orient)
    other = hip.Context(0)
    try:
        c = _decode(other, files, orient)
    finally:
        other.close()
    for n, o, x, y, z in zip(names, orient, a, b, c):
        _same(x, X.orient_map(decoded[n], o), n)
        assert np.array_equal(x, y) and np.array_equal(x, z)


def test_hip_read_jpeg_views_from_cpp(decoded, tmp_path):
    exe = tmp_path / "jpeg_orient_selftest"
    lib_dir = os.path.join(D.ROOT, "openpano_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fopenmp", "-I", os.path.join(D.ROOT, "include"), "-I", os.path.join(lib_dir, "host"),
                           "-o", str(exe), os.path.join(D.ROOT, "tests", "harness", "jpeg_orient_selftest.cc"),
                           "-L", lib_dir, "-lopenpano_hip", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib"])
    jobs = [("size_37x53_420", "MM_focal_sub", 6), ("size_40x56_420", "II_short", 3), ("grey_37x53", "orient_last", 8), ("size_17x17_420", "orient_absent", 4)]
    paths, want = [], []
    for k, (n, how, o) in enumerate(jobs):
        f, (eo, ef) = X.WELL_FORMED[how](D.data(n), o, 24 + k)
        p = tmp_path / f"v{k}.jpg"
        p.write_bytes(f)
        paths.append(str(p)); want.append((eo, ef, X.orient_map(decoded[n], eo)))
    fout = tmp_path / "out.bin"
    r = subprocess.run([str(exe), str(fout)] + paths, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    blob = open(fout, "rb").read()
    at = 0
    for (eo, ef, px), (n, how, _) in zip(want, jobs):
        o, f, h, w = struct.unpack_from("<4i", blob, at); at += 16
        assert (o, f, h, w) == (eo, ef) + px.shape[:2], (n, how)
        _same(np.frombuffer(blob, np.uint8, h * w * 3, at).reshape(h, w, 3), px, (n, how)); at += h * w * 3
    assert at == len(blob)


def test_stitch_demo_jpeg_orient(ctx, ref, tmp_path):
    assert os.path.exists(DEMO), "build it: make -C openpano_amd/csrc"
    views, _, _ = synth.rotating_views(5, 300, 400, seed=77, step_deg=22.0)
    u8 = [np.ascontiguousarray((np.clip(v, 0, 1) * 255).astype(np.uint8)) for v in views]
    orient = [6, 8, 5, 7, 6]                                # every file is stored 400 x 300 and shown 300 x 400
    paths = []
    for i, (a, o) in enumerate(zip(u8, orient)):
        stored = X.orient_map(a, INVERSE[o])
        assert stored.shape == (400, 300, 3)
        p = tmp_path / f"view{i}.jpg"
        p.write_bytes(X.with_orientation(hip.encode_jpeg_u8(ctx, stored, 95, "444" if i % 2 else "420"), o, "MM" if i % 2 else "II"))
        paths.append(str(p))
    (tmp_path / "list.txt").write_text("\n".join(paths) + "\n")
    pixels = [X.orient_map(D.ref_decode(ref, open(p, "rb").read()), o) for p, o in zip(paths, orient)]
    n = len(pixels); h, w, _ = pixels[0].shape
    assert (h, w) == (300, 400)
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("<3i", n, h, w))
        for a in pixels:
            f.write((a.astype(np.float32) / np.float32(255.0)).astype(np.float32).tobytes())
    outs = []
    for tag, extra in (("bin", ["--resident-views"]), ("jpeg", ["--jpeg-list", str(tmp_path / "list.txt"), "--jpeg-orient"])):
        fout = tmp_path / f"out_{tag}.bin"
        r = subprocess.run([DEMO, str(tmp_path / "in.bin"), str(fout), "42", "camera_build"] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(open(fout, "rb").read())
    H, W = struct.unpack_from("<2i", outs[0], 0)
    assert H > 100 and W > 400 and outs[0] == outs[1]
    r = subprocess.run([DEMO, str(tmp_path / "in.bin"), str(tmp_path / "x.bin"), "42", "camera_build", "--jpeg-orient"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--jpeg-orient goes with --jpeg-list" in r.stderr
