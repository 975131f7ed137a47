"""GPU: exposure (gain) compensation -- op_gain_overlap (csrc/overlap.hip) / op_gain_solve (photometric_solve.cc) / op_blend_gains (blend.hip).

1. the overlap statistics equal a CPU restatement (tests/harness/gain_overlap_ref.c, host libm for the map's trig, like
   the blend's tables) EXACTLY: counts and fixed-point int64 sums, for every projection, both LAZY_READ branches,
   strides 1 and 3, pixels covered by 3+ images and a 70-view scene whose pairs straddle the 64-image cover word;
2. gains off (NULL) and all-ones gains give op_blend's canvas bit for bit on every blend case of test_gpu_blend.py;
3. known exposures are recovered and the overlap residual drops, for both blenders;
4. two runs give bit-equal statistics and canvases;
5. the C++ path (stitch_demo --gain-compensation) matches the Python path."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from openpano_amd import hip, synth
from openpano_amd.config import PanoConfig

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "tests", "harness", "gain_overlap_ref.c")
DEMO = os.path.join(ROOT, "openpano_amd", "host", "stitch_demo")


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.close()


class GRefImage(C.Structure):
    _fields_ = [("data", C.c_void_p), ("h", C.c_int), ("w", C.c_int), ("mh", C.c_int), ("mw", C.c_int),
                ("hinv", C.c_double * 9), ("x0", C.c_int), ("y0", C.c_int), ("x1", C.c_int), ("y1", C.c_int)]


@pytest.fixture(scope="module")
def gref(tmp_path_factory):
    gcc = shutil.which("gcc") or shutil.which("cc")
    if not gcc:
        pytest.fail("a C compiler is needed for the CPU restatement")
    so = str(tmp_path_factory.mktemp("gref") / "libgain_overlap_ref.so")
    subprocess.check_call([gcc, "-std=c11", "-O2", "-ffp-contract=off", "-fPIC", "-shared", HARNESS, "-o", so, "-lm"])
    L = C.CDLL(so)
    L.gain_overlap_ref.argtypes = [C.c_int] + [C.c_double] * 4 + [C.c_int] * 3 + [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    return L


def _cfg(**kv):
    base = dict(ESTIMATE_CAMERA=1, ORDERED_INPUT=0, LAZY_READ=0, MULTIBAND=0)
    base.update(kv)
    return PanoConfig(**base)


def _ref_stats(gref, call, views, cfg, stride):
    """the restatement over the geometry / ROIs of a BlendCall"""
    g, n = call.geom, call.n
    arr = (GRefImage * n)()
    rois = []
    keep = []
    for k in range(n):
        v = np.ascontiguousarray(views[k], np.float32); keep.append(v)
        r = [call.arr[k].range[q] for q in range(4)]
        roi = [int((r[0] - g.proj_min[0]) / g.resolution[0]), int((r[1] - g.proj_min[1]) / g.resolution[1]),
               int((r[2] - g.proj_min[0]) / g.resolution[0]), int((r[3] - g.proj_min[1]) / g.resolution[1])]
        rois.append(roi)
        arr[k] = GRefImage(v.ctypes.data_as(C.c_void_p), v.shape[0], v.shape[1], v.shape[0], v.shape[1],
                           (C.c_double * 9)(*call.arr[k].homo_inv), *roi)
    H = max(r[3] for r in rois); W = max(r[2] for r in rois)
    P = n * (n - 1) // 2
    count = np.zeros(P, np.int64); sums = np.zeros((P, 6), np.int64)
    assert gref.gain_overlap_ref(g.proj_method, g.proj_min[0], g.proj_min[1], g.resolution[0], g.resolution[1], H, W, n, arr,
                                 int(stride), int(cfg.LAZY_READ), count.ctypes.data_as(C.c_void_p), sums.ctypes.data_as(C.c_void_p)) == 0
    return count, sums


# (n, h, w, seed, proj, method, step): step 0.3 puts 3+ views over some pixels
SCENES = [
    (5, 120, 160, 41, "flat", 0, 0.3),
    (5, 120, 160, 42, "camera", 1, 0.3),
    (5, 120, 160, 43, "camera", 2, 0.3),
    (6, 100, 140, 44, "camera", 2, 0.55),
]


@pytest.mark.parametrize("n,h,w,seed,proj,method,step", SCENES)
@pytest.mark.parametrize("lazy", [0, 1])
@pytest.mark.parametrize("stride", [1, 3])
def test_overlap_statistics_exact(ctx, gref, n, h, w, seed, proj, method, step, lazy, stride):
    views, homos = synth.pano_scene(n, h, w, seed=seed, proj=proj, step=step)
    cfg = _cfg(LAZY_READ=lazy)
    call = hip.BlendCall(ctx, cfg, views, homos, method, n // 2)
    count, sums = call.overlap_sums(stride)
    want_c, want_s = _ref_stats(gref, call, views, cfg, stride)
    assert count.sum() > 0
    assert np.array_equal(count, want_c), np.flatnonzero(count != want_c)
    assert np.array_equal(sums, want_s)
    if step < 0.34:                      # some pixel is covered by 3+ images: a pair (a, a + 2) overlaps
        assert any(count[hip.pair_index(n, a, a + 2)] > 0 for a in range(n - 2))


def test_overlap_statistics_exact_70_views(ctx, gref):
    """70 small views: pairs such as (62, 64) and (63, 65) straddle the first 64-image word of the cover bitmask"""
    n = 70
    views, homos = synth.pano_scene(n, 24, 40, seed=7, proj="flat", step=0.3)
    cfg = _cfg(ESTIMATE_CAMERA=0, TRANS=1, ORDERED_INPUT=1)
    call = hip.BlendCall(ctx, cfg, views, homos, 0, n // 2)
    for stride in (1, 3):
        count, sums = call.overlap_sums(stride)
        want_c, want_s = _ref_stats(gref, call, views, cfg, stride)
        assert np.array_equal(count, want_c) and np.array_equal(sums, want_s), stride
    count, _ = call.overlap_sums(1)
    assert all(count[hip.pair_index(n, a, b)] > 0 for a, b in ((62, 64), (63, 64), (63, 65)))


def test_overlap_statistics_exact_300_permuted_views(ctx, gref):
    """300 views on a permuted grid (tests/blend_cover_cases.py): the second pass of overlap_walk's marking loop, tiles met by
    far more images than one chunk holds, and overlapping pairs whose indices lie more than 256 apart"""
    import blend_cover_cases as bc
    views, homos, idx = bc.overlap_scene()
    n = len(views)
    a, b = bc.pair_arrays(n)
    for lazy in (0, 1):
        cfg = _cfg(ESTIMATE_CAMERA=0, TRANS=1, ORDERED_INPUT=1, LAZY_READ=lazy)
        call = hip.BlendCall(ctx, cfg, views, homos, 0, idx)
        for stride in (1, 3):
            count, sums = call.overlap_sums(stride)
            want_c, want_s = _ref_stats(gref, call, views, cfg, stride)
            assert np.array_equal(count, want_c) and np.array_equal(sums, want_s), (lazy, stride)
            assert ((count > 0) & (b - a > 256)).any() and ((count > 0) & (a < 64) & (b >= 64)).any(), (lazy, stride)


def test_gains_off_equals_op_blend(ctx):
    """every blend case of test_gpu_blend.py: gains NULL and all-ones gains give op_blend's canvas bit for bit"""
    from test_gpu_blend import CASES, _cfg as blend_cfg
    for proj, method, over, _ in CASES:
        cfg = blend_cfg(**over)
        views, homos = synth.pano_scene(5, 200, 280, seed=31 + method, proj=proj)
        call = hip.BlendCall(ctx, cfg, views, homos, method, 2)
        cv = call(); want = cv.numpy(); cv.free()
        cv = hip.BlendCall(ctx, cfg, views, homos, method, 2, gains=np.ones((5, 3), np.float32))(); ones = cv.numpy(); cv.free()
        h = C.c_void_p()
        hip.check(hip.lib().op_blend_gains(ctx.handle, C.byref(call.ccfg), C.byref(call.geom), call.arr, call.n, None, C.byref(h)))
        cv = hip.Canvas(ctx, h); null = cv.numpy(); cv.free()
        assert np.array_equal(null, want), (proj, method, over)
        assert np.array_equal(ones, want), (proj, method, over)


def _residual(count, means, gains, n):
    t = w = 0.0
    for a in range(n):
        for b in range(a + 1, n):
            p = hip.pair_index(n, a, b)
            if count[p]:
                t += count[p] * np.abs(gains[a] * means[p, :3] - gains[b] * means[p, 3:]).mean()
                w += count[p]
    return t / w


@pytest.mark.parametrize("proj,method,n", [("flat", 0, 5), ("rotating", 2, 7)])
@pytest.mark.parametrize("mb", [0, 4])
def test_known_exposures_recovered(ctx, proj, method, n, mb):
    """views scaled by e_k in [0.7, 1]: the solved gains undo them (g_a e_a / g_b e_b within 1%) and the residual over the
    overlaps drops 10x; the gained blend is valid and differs from the plain one.  sigma_g = 10: the default 0.1 holds the
    gains near 1 (measured: ratios off by up to ~25% on a chain) -- that trade-off is the prior's job, not the solver's."""
    if proj == "flat":
        views, homos = synth.pano_scene(n, 160, 220, seed=90 + n, proj=proj)
    else:                                # a rotating camera: both sides of an overlap see the same rays
        views, f, Rs = synth.rotating_views(n, 160, 220, seed=90 + n, step_deg=20.0)
        homos = np.stack([R.T @ np.diag([1.0 / f, 1.0 / f, 1.0]) for R in Rs])
    e = np.random.default_rng(n).uniform(0.7, 1.0, n)
    dark = [(v * np.float32(ek)).astype(np.float32) for v, ek in zip(views, e)]
    cfg = _cfg(MULTIBAND=mb) if method else _cfg(ESTIMATE_CAMERA=0, TRANS=1, ORDERED_INPUT=1, MULTIBAND=mb)
    count, means = hip.gain_overlap(ctx, cfg, dark, homos, method, n // 2)
    _, sums = hip.gain_overlap_sums(ctx, cfg, dark, homos, method, n // 2)
    gains = hip.gain_solve(n, count, sums, sigma_g=10.0)
    r = gains[:, 0] * e
    ratio = r[:, None] / r[None, :]
    assert ratio.min() >= 0.99 and ratio.max() <= 1.01, ratio
    assert _residual(count, means, gains, n) * 10 <= _residual(count, means, np.ones((n, 3)), n)
    cv = hip.blend(ctx, cfg, dark, homos, method, n // 2, gains=gains); got = cv.numpy(); cv.free()
    cv = hip.blend(ctx, cfg, dark, homos, method, n // 2); plain = cv.numpy(); cv.free()
    valid = got[..., 0] >= 0
    assert np.array_equal(valid, plain[..., 0] >= 0)
    assert got[valid].max() <= 1.0 and got[valid].min() >= 0.0
    assert not np.array_equal(got, plain)
    # per_channel = 0: one gain for all three channels
    grey = hip.gain_solve(n, count, sums, sigma_g=10.0, per_channel=False)
    assert np.array_equal(grey[:, 0], grey[:, 2])
    rg = grey[:, 0] * e
    assert (rg.max() / rg.min()) <= 1.01


@pytest.mark.parametrize("proj,method", [("flat", 0), ("camera", 2)])
@pytest.mark.parametrize("over", [dict(), dict(LAZY_READ=1), dict(MULTIBAND=3)], ids=["linear", "lazy", "multiband3"])
def test_gains_applied_per_image_and_channel(ctx, proj, method, over):
    """views divided by distinct power-of-two gains per image AND channel (exact in fp32, no clamp: the views are in
    [0, 0.75]) and blended with those gains give op_blend's canvas of the undivided views bit for bit -- a swapped channel or
    image index in either blender would not"""
    n = 5
    views, homos = synth.pano_scene(n, 120, 160, seed=61 + method, proj=proj, step=0.3)
    orig = [(v * np.float32(0.75)).astype(np.float32) for v in views]
    G = np.array([[2.0 ** (1 + (k + c) % 3) * (1 if k % 2 else 2) for c in range(3)] for k in range(n)], np.float32)
    dark = [(v / G[k]).astype(np.float32) for k, v in enumerate(orig)]
    assert all(np.array_equal(d * G[k], o) for k, (d, o) in enumerate(zip(dark, orig)))
    cfg = _cfg(**over) if method else _cfg(ESTIMATE_CAMERA=0, TRANS=1, ORDERED_INPUT=1, **over)
    cv = hip.blend(ctx, cfg, orig, homos, method, n // 2); want = cv.numpy(); cv.free()
    cv = hip.blend(ctx, cfg, dark, homos, method, n // 2, gains=G); got = cv.numpy(); cv.free()
    assert (want[..., 0] >= 0).mean() > 0.5
    assert np.array_equal(got, want)
    cv = hip.blend(ctx, cfg, dark, homos, method, n // 2, gains=G[:, ::-1].copy()); swapped = cv.numpy(); cv.free()
    assert not np.array_equal(swapped, want)


def test_gain_clamp_and_determinism(ctx):
    """a large gain saturates at 1 (never beyond); statistics and canvases of two runs are bit-equal"""
    n = 5
    views, homos = synth.pano_scene(n, 120, 160, seed=3, proj="camera", step=0.3)
    for mb in (0, 3):
        cfg = _cfg(MULTIBAND=mb)
        call = hip.BlendCall(ctx, cfg, views, homos, 2, 2, gains=np.full(n, 4.0, np.float32))
        a = call(); x = a.numpy(); a.free()
        b = call(); y = b.numpy(); b.free()
        assert np.array_equal(x, y)
        v = x[x[..., 0] >= 0]
        assert v.max() <= 1.0 and (v == 1.0).mean() > 0.3
        s1 = call.overlap_sums(1); s2 = call.overlap_sums(1)
        assert np.array_equal(s1[0], s2[0]) and np.array_equal(s1[1], s2[1])


def test_device_entry_points_reject_bad_arguments(ctx):
    n = 3
    views, homos = synth.pano_scene(n, 60, 80, seed=2, proj="flat")
    call = hip.BlendCall(ctx, _cfg(ESTIMATE_CAMERA=0, TRANS=1, ORDERED_INPUT=1), views, homos, 0, 1)
    L = hip.lib()
    count = np.zeros(3, np.int64); sums = np.zeros((3, 6), np.int64)
    cp, sp = count.ctypes.data_as(C.c_void_p), sums.ctypes.data_as(C.c_void_p)
    for stride, c, s in ((0, cp, sp), (-2, cp, sp), (1, None, sp), (1, cp, None)):
        assert L.op_gain_overlap(ctx.handle, C.byref(call.ccfg), C.byref(call.geom), call.arr, n, stride, c, s) == -1
    assert L.op_gain_overlap(ctx.handle, C.byref(call.ccfg), C.byref(call.geom), call.arr, 0, 1, cp, sp) == -1
    h = C.c_void_p()
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        g = np.ones((n, 3), np.float32); g[1, 2] = bad
        assert L.op_blend_gains(ctx.handle, C.byref(call.ccfg), C.byref(call.geom), call.arr, n,
                                g.ctypes.data_as(C.c_void_p), C.byref(h)) == -1, bad
        assert b"op_blend_gains" in L.op_last_error()


def _run_demo(tmp_path, views, mode, gain):
    n, h, w = len(views), views[0].shape[0], views[0].shape[1]
    fin, fout = tmp_path / "in.bin", tmp_path / ("out_%s_%d.bin" % (mode or "chain", gain))
    with open(fin, "wb") as f:
        f.write(struct.pack("<3i", n, h, w))
        for v in views:
            f.write(np.ascontiguousarray(v, np.float32).tobytes())
    args = [DEMO, str(fin), str(fout), "42"] + ([mode] if mode else []) + (["--gain-compensation"] if gain else [])
    r = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return open(fout, "rb").read()


def test_stitch_demo_gain_compensation(ctx, tmp_path):
    """stitch_demo camera mode (HipStitcher's stages + hip_gain_compensate + hip_blend(b, crop, gains)): without the flag
    nothing but the panorama follows the cameras and the output carries no gains; with it, everything before the panorama
    is byte-identical, the gains it appends match the Python path's on the same cameras, and its panorama matches
    blend(gains=).  (The program sets homo_inv = K R itself, the Python path inverts homo: the geometry agrees to
    rounding, hence tolerances -- the same ones test_gpu_host_cpp.py uses for this panorama.)"""
    assert os.path.exists(DEMO), "build it: make -C openpano_amd/csrc"
    n, h, w = 5, 300, 400
    views, _, _ = synth.rotating_views(n, h, w, seed=77, step_deg=22.0)
    e = np.random.default_rng(5).uniform(0.7, 1.0, n)
    dark = [(v * np.float32(ek)).astype(np.float32) for v, ek in zip(views, e)]
    off = _run_demo(tmp_path, dark, "camera", False)
    on = _run_demo(tmp_path, dark, "camera", True)
    cams = _cameras(off, n)
    assert np.array_equal(cams, _cameras(on, n))
    H0, W0, pano_off = _canvas(off, n, tail=0)
    H, W, pano_on = _canvas(on, n, tail=12 * n)
    assert (H, W) == (H0, W0)
    head = _skip_head(off, n) + 13 * n * 8
    assert on[:head] == off[:head]
    gains_demo = np.frombuffer(on, np.float32, count=3 * n, offset=len(on) - 12 * n).reshape(n, 3)
    homos = np.stack([_homo(c) for c in cams])
    cfg = _cfg()
    count, sums = hip.gain_overlap_sums(ctx, cfg, dark, homos, 2, n // 2)
    want_g = hip.gain_solve(n, count, sums)
    assert np.all(gains_demo != 1.0)
    assert np.abs(gains_demo / want_g - 1).max() < 1e-4, (gains_demo, want_g)
    cv = hip.blend(ctx, cfg, dark, homos, 2, n // 2, gains=gains_demo); want = cv.numpy(); cv.free()
    cv = hip.blend(ctx, cfg, dark, homos, 2, n // 2); want0 = cv.numpy(); cv.free()
    for got, ref in ((pano_on.reshape(H, W, 3), want), (pano_off.reshape(H, W, 3), want0)):
        assert ref.shape == got.shape
        valid = (ref[..., 0] >= 0) & (got[..., 0] >= 0)
        assert valid.mean() > 0.5 and np.mean((ref[..., 0] >= 0) != (got[..., 0] >= 0)) < 2e-3
        assert np.abs(got[valid] - ref[valid]).max() < 1e-4
    assert not np.array_equal(pano_on, pano_off)


def test_stitch_demo_chain_gain_compensation(ctx, tmp_path):
    """stitch_demo's TRANS mode (pairwise homographies chained to the middle image, flat projection): with the flag it
    appends n x 3 gains after the chain homographies; they equal the Python path's on those homographies exactly, and the
    panorama equals blend(gains=) bit for bit.  Without the flag nothing follows the homographies."""
    assert os.path.exists(DEMO), "build it: make -C openpano_amd/csrc"
    n, h, w = 4, 240, 320
    views = synth.image_set(n, h, w, seed=5, overlap=0.5)
    e = np.random.default_rng(11).uniform(0.8, 1.0, n)
    dark = [(v * np.float32(ek)).astype(np.float32) for v, ek in zip(views, e)]
    off = _run_demo(tmp_path, dark, None, False)
    on = _run_demo(tmp_path, dark, None, True)
    o = _skip_head(on, n)
    assert on[:o] == off[:o]
    H, W = struct.unpack_from("<2i", on, o)
    assert H > 200 and W > 600
    pano = np.frombuffer(on, np.float32, count=H * W * 3, offset=o + 8).reshape(H, W, 3)
    to_mid = np.frombuffer(on, np.float64, count=9 * n, offset=o + 8 + H * W * 12).reshape(n, 3, 3)
    tail = o + 8 + H * W * 12 + 72 * n
    assert len(off) == tail and len(on) == tail + 12 * n
    gains_demo = np.frombuffer(on, np.float32, count=3 * n, offset=tail).reshape(n, 3)
    cfg = PanoConfig(ESTIMATE_CAMERA=0, TRANS=1, ORDERED_INPUT=1, LAZY_READ=0)
    count, sums = hip.gain_overlap_sums(ctx, cfg, dark, to_mid, 0, n >> 1)
    want_g = hip.gain_solve(n, count, sums)
    assert np.array_equal(gains_demo, want_g) and np.all(want_g != 1.0)
    cv = hip.blend(ctx, cfg, dark, to_mid, 0, n >> 1, gains=want_g); want = cv.numpy(); cv.free()
    assert np.array_equal(pano, want)
    cv = hip.blend(ctx, cfg, dark, to_mid, 0, n >> 1); plain = cv.numpy(); cv.free()
    assert np.array_equal(np.frombuffer(off, np.float32, count=H * W * 3, offset=o + 8).reshape(H, W, 3), plain)


def test_stitcher_build_gain_compensation(tmp_path):
    """HipStitcher::build() itself (stitch_demo camera_build): with gain_compensation set its panorama and gains equal the
    staged camera mode's (which calls hip_gain_compensate + hip_blend by hand) bit for bit; without it, the panorama equals
    the staged mode's plain blend and build() reports no gains"""
    assert os.path.exists(DEMO), "build it: make -C openpano_amd/csrc"
    n, h, w = 5, 300, 400
    views, _, _ = synth.rotating_views(n, h, w, seed=77, step_deg=22.0)
    e = np.random.default_rng(5).uniform(0.7, 1.0, n)
    dark = [(v * np.float32(ek)).astype(np.float32) for v, ek in zip(views, e)]
    for gain in (True, False):
        staged = _run_demo(tmp_path, dark, "camera", gain)
        built = _run_demo(tmp_path, dark, "camera_build", gain)
        H, W, pano = _canvas(staged, n, tail=12 * n if gain else 0)
        bH, bW = struct.unpack_from("<2i", built, 0)
        assert (bH, bW) == (H, W)
        assert len(built) == 8 + H * W * 12 + (12 * n if gain else 0)
        assert np.array_equal(np.frombuffer(built, np.float32, count=H * W * 3, offset=8), pano)
        if gain:
            assert built[8 + H * W * 12:] == staged[len(staged) - 12 * n:]


def _skip_head(buf, n):
    """offset just past the features and pairs sections of stitch_demo's camera-mode output"""
    o = 0
    for _ in range(n):
        K = struct.unpack_from("<i", buf, o)[0]; o += 4 + K * 128 * 4 + K * 2 * 8
    npairs = struct.unpack_from("<i", buf, o)[0]; o += 4
    for _ in range(npairs):
        M = struct.unpack_from("<3i", buf, o)[2]; o += 12 + M * 8
        o += 4 + 4 + 9 * 8
        ninl = struct.unpack_from("<i", buf, o)[0]; o += 4 + ninl * 32
    return o


def _cameras(buf, n):
    o = _skip_head(buf, n)
    return np.frombuffer(buf, np.float64, count=13 * n, offset=o).reshape(n, 13).copy()


def _homo(c):
    """ImageComponent::homo = R^-1 K^-1 (stitcher.cc:154-158) of a camera (focal, aspect, ppx, ppy, R)"""
    f, aspect, ppx, ppy = c[:4]
    K = np.array([[f, 0, ppx], [0, f * aspect, ppy], [0, 0, 1]])
    R = c[4:].reshape(3, 3)
    return R.T @ np.linalg.inv(K)


def _canvas(buf, n, tail):
    o = _skip_head(buf, n) + 13 * n * 8
    H, W = struct.unpack_from("<2i", buf, o)
    o += 8
    assert o + H * W * 12 + tail == len(buf)
    return H, W, np.frombuffer(buf, np.float32, count=H * W * 3, offset=o)
