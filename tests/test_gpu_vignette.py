"""GPU: vignetting compensation -- op_vignette_overlap (csrc/overlap.hip) / op_vignette_solve (photometric_solve.cc) / op_blend_vignette (blend.hip).

1. the statistics equal a CPU restatement (tests/harness/vignette_overlap_ref.c) EXACTLY: counts and the 30 fixed-point
   int64 moments per pair, for every projection, both LAZY_READ branches, strides 1 and 3, clip 1 and 0.9, pixels covered
   by 3+ images and a 70-view scene whose pairs straddle the 64-image cover word;
2. a curve of 0 gives op_blend_gains(g)'s canvas, and with gains 1 op_blend's, bit for bit on every blend case of
   test_gpu_blend.py;
3. a non-zero curve gives the canvas of a C restatement of the linear blend bit for bit;
4. on views with exposure differences and ONE falloff 1 - alpha rho shared by all of them, the recovered curve is close to
   the truth and the canvas error against the clean views is far below the per-image gains' (linear and multiband);
   on vignetted()'s per-view falloffs (the model is wrong there on purpose) the error is reported and bounded;
5. two runs give bit-equal statistics, gains, curve and canvases;
6. the device entry points reject bad arguments and cylinder pre-warped views;
7. the C++ path (stitch_demo --vignetting) matches the Python path."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from openpano_amd import hip, synth
from openpano_amd.config import PanoConfig
from test_gpu_gain_blocks import GRefImage, _ref_geometry, canvas_error, vignetted, _skip_head, _homo

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "tests", "harness", "vignette_overlap_ref.c")
DEMO = os.path.join(ROOT, "openpano_amd", "host", "stitch_demo")
RHO = np.linspace(0.0, 1.0, 101)


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.close()


def build_ref(outdir):
    gcc = shutil.which("gcc") or shutil.which("cc")
    if not gcc:
        pytest.fail("a C compiler is needed for the CPU restatement")
    so = os.path.join(str(outdir), "libvignette_ref.so")
    subprocess.check_call([gcc, "-std=c11", "-O2", "-ffp-contract=off", "-fPIC", "-shared", HARNESS, "-o", so, "-lm"])
    L = C.CDLL(so)
    geo = [C.c_int] + [C.c_double] * 4 + [C.c_int] * 3 + [C.c_void_p]
    L.vignette_overlap_ref.argtypes = geo + [C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p]
    L.blend_linear_vig_ref.argtypes = geo + [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    return L


@pytest.fixture(scope="module")
def vref(tmp_path_factory):
    return build_ref(tmp_path_factory.mktemp("vigref"))


def _cfg(**kv):
    base = dict(ESTIMATE_CAMERA=1, ORDERED_INPUT=0, LAZY_READ=0, MULTIBAND=0)
    base.update(kv)
    return PanoConfig(**base)


def _flat_cfg(**kv):
    return _cfg(ESTIMATE_CAMERA=0, TRANS=1, ORDERED_INPUT=1, **kv)


def ref_stats(vref, call, views, cfg, stride, clip):
    head, keep = _ref_geometry(call, views)
    P = call.n * (call.n - 1) // 2
    count = np.zeros(P, np.int64); mom = np.zeros((P, 30), np.int64)
    assert vref.vignette_overlap_ref(*head, int(stride), int(cfg.LAZY_READ), float(clip), count.ctypes.data_as(C.c_void_p),
                                     mom.ctypes.data_as(C.c_void_p)) == 0
    return count, mom


def ref_blend_linear(vref, call, views, cfg, gains, poly):
    head, keep = _ref_geometry(call, views)
    H, W = head[5], head[6]
    g = np.ascontiguousarray(gains, np.float32); p = np.ascontiguousarray(poly, np.float32)
    out = np.zeros((H, W, 3), np.float32)
    assert vref.blend_linear_vig_ref(*head, int(cfg.LAZY_READ), int(cfg.ORDERED_INPUT), g.ctypes.data_as(C.c_void_p),
                                     p.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)) == 0
    return out


def _canvas(call):
    cv = call(); x = cv.numpy(); cv.free()
    return x


def curve(poly, rho):
    a1, a2, a3 = (float(x) for x in poly)
    return 1.0 + rho * (a1 + rho * (a2 + rho * a3))


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
def test_statistics_exact(ctx, vref, n, h, w, seed, proj, method, step, lazy, stride):
    views, homos = synth.pano_scene(n, h, w, seed=seed, proj=proj, step=step)
    views[1] = np.minimum(views[1] * np.float32(1.3), np.float32(1.0)).astype(np.float32)   # some saturated samples for clip
    cfg = _cfg(LAZY_READ=lazy) if method else _flat_cfg(LAZY_READ=lazy)
    call = hip.BlendCall(ctx, cfg, views, homos, method, n // 2)
    c_all = None
    for clip in (1.0, 0.9):
        count, mom = call.vignette_overlap_sums(stride, clip)
        want_c, want_m = ref_stats(vref, call, views, cfg, stride, clip)
        assert count.sum() > 0 and mom[:, 14].sum() > 0
        assert np.array_equal(count, want_c), (clip, np.argwhere(count != want_c)[:5])
        assert np.array_equal(mom, want_m), (clip, np.argwhere(mom != want_m)[:5])
        if c_all is None:
            c_all = count
        else:
            assert count.sum() < c_all.sum()          # clip 0.9 drops samples
    # op_gain_overlap's pairs, less the samples interpolated a hair above 1 in the saturated view
    c1, _ = call.overlap_sums(stride)
    assert np.all(c_all <= c1) and c_all.sum() > 0.9 * c1.sum()
    if step < 0.34:
        assert any(c_all[hip.pair_index(n, a, a + 2)] > 0 for a in range(n - 2))


def test_statistics_exact_70_views(ctx, vref):
    """70 small views: pairs such as (62, 64) and (63, 65) straddle the first 64-image word of the cover bitmask"""
    n = 70
    views, homos = synth.pano_scene(n, 24, 40, seed=7, proj="flat", step=0.3)
    cfg = _flat_cfg()
    call = hip.BlendCall(ctx, cfg, views, homos, 0, n // 2)
    for stride in (1, 3):
        for clip in (1.0, 0.9):
            count, mom = call.vignette_overlap_sums(stride, clip)
            want_c, want_m = ref_stats(vref, call, views, cfg, stride, clip)
            assert np.array_equal(count, want_c) and np.array_equal(mom, want_m), (stride, clip)
    count, _ = call.vignette_overlap_sums(1, 1.0)
    assert all(count[hip.pair_index(n, a, b)] > 0 for a, b in ((62, 64), (63, 64), (63, 65)))


def test_statistics_exact_300_permuted_views(ctx, vref):
    """300 views on a permuted grid (tests/blend_cover_cases.py): the second pass of overlap_walk's marking loop, tiles met by
    far more images than one chunk holds, and overlapping pairs whose indices lie more than 256 apart"""
    import blend_cover_cases as bc
    views, homos, idx = bc.overlap_scene()
    n = len(views)
    a, b = bc.pair_arrays(n)
    cfg = _flat_cfg()
    call = hip.BlendCall(ctx, cfg, views, homos, 0, idx)
    for stride in (1, 3):
        full = None
        for clip in (1.0, 0.6):
            count, mom = call.vignette_overlap_sums(stride, clip)
            want_c, want_m = ref_stats(vref, call, views, cfg, stride, clip)
            assert np.array_equal(count, want_c) and np.array_equal(mom, want_m), (stride, clip)
            assert ((count > 0) & (b - a > 256)).any() and ((count > 0) & (a < 64) & (b >= 64)).any(), (stride, clip)
            if full is None:
                full = count
            else:
                assert 0 < count.sum() < full.sum()            # clip 0.6 drops samples


def test_zero_curve_is_plain_gains(ctx):
    """every blend case of test_gpu_blend.py: a = 0 gives op_blend_gains(g)'s canvas bit for bit; a = 0 with g = 1 (and NULL
    gains and curve) op_blend's"""
    from test_gpu_blend import CASES, _cfg as blend_cfg
    n = 5
    zero = np.zeros(3, np.float32)
    for proj, method, over, _ in CASES:
        cfg = blend_cfg(**over)
        views, homos = synth.pano_scene(n, 200, 280, seed=31 + method, proj=proj)
        plain = _canvas(hip.BlendCall(ctx, cfg, views, homos, method, 2))
        G = np.repeat(np.random.default_rng(method + 7).uniform(0.6, 1.5, (n, 1)), 3, axis=1).astype(np.float32)
        G[1] = 1.0
        per_image = _canvas(hip.BlendCall(ctx, cfg, views, homos, method, 2, gains=G))
        assert not np.array_equal(per_image, plain)
        got = _canvas(hip.BlendCall(ctx, cfg, views, homos, method, 2, gains=G, vignette=zero))
        assert np.array_equal(got, per_image), (proj, method, over)
        ones = _canvas(hip.BlendCall(ctx, cfg, views, homos, method, 2, gains=np.ones((n, 3), np.float32), vignette=zero))
        assert np.array_equal(ones, plain), (proj, method, over)
        call = hip.BlendCall(ctx, cfg, views, homos, method, 2)
        h = C.c_void_p()
        hip.check(hip.lib().op_blend_vignette(ctx.handle, C.byref(call.ccfg), C.byref(call.geom), call.arr, call.n, None, None, C.byref(h)))
        cv = hip.Canvas(ctx, h); null = cv.numpy(); cv.free()
        assert np.array_equal(null, plain), (proj, method, over)
        # a real curve changes the canvas
        vig = _canvas(hip.BlendCall(ctx, cfg, views, homos, method, 2, gains=G, vignette=(-0.3, 0.05, 0.0)))
        assert not np.array_equal(vig, per_image)


@pytest.mark.parametrize("proj,method", [("flat", 0), ("camera", 1), ("camera", 2)])
@pytest.mark.parametrize("lazy", [0, 1])
@pytest.mark.parametrize("poly", [(-0.3, 0.0, 0.0), (-0.5, 0.4, -0.2)])
def test_curve_applied_per_sample(ctx, vref, proj, method, lazy, poly):
    """a non-zero curve and random gains (some exactly 1, some high enough to clamp) give the canvas of the C restatement of
    the linear blend bit for bit"""
    n = 5
    views, homos = synth.pano_scene(n, 120, 160, seed=71 + method, proj=proj, step=0.3)
    views = [(v * np.float32(0.8)).astype(np.float32) for v in views]
    rng = np.random.default_rng(method + 3 * lazy)
    G = np.repeat(rng.uniform(0.6, 1.5, (n, 1)), 3, axis=1).astype(np.float32)
    G[2] = 1.0
    P = np.array(poly, np.float32)
    for ordered in (0, 1):
        if not method and not ordered:
            continue                     # TRANS requires ORDERED_INPUT (main.cc:257-258)
        cfg = _cfg(LAZY_READ=lazy, ORDERED_INPUT=ordered) if method else _flat_cfg(LAZY_READ=lazy)
        call = hip.BlendCall(ctx, cfg, views, homos, method, n // 2, gains=G, vignette=P)
        got = _canvas(call)
        want = ref_blend_linear(vref, call, views, cfg, G, P)
        assert (want[..., 0] >= 0).mean() > 0.5
        assert np.array_equal(got, want), (np.argwhere(got != want)[:5], ordered)


# ---- quality: exposures + one falloff shared by all views ----
def rho_map(h, w):
    """the contract's rho at every pixel (r, c) = (row, column) of an h x w view -- the coordinates interpolate() reads
    a pixel at"""
    r, c = np.mgrid[0:h, 0:w].astype(np.float32)
    fw, fh = np.float32(w), np.float32(h)
    dx = c - np.float32(0.5) * fw; dy = r - np.float32(0.5) * fh
    return np.minimum((dx * dx + dy * dy) / (np.float32(0.25) * (fw * fw + fh * fh)), np.float32(1))


def shared_falloff(views, seed, alpha):
    """views x exposure e_k in [0.7, 1] x ONE falloff 1 - alpha rho"""
    rng = np.random.default_rng(seed)
    return [(v * (rng.uniform(0.7, 1.0) * (1.0 - alpha * rho_map(*v.shape[:2]).astype(np.float64)))[..., None]).astype(np.float32)
            for v in views]


def quality_scene(n=5, seed=13, alpha=0.3):
    """test_gpu_gain_blocks.py's rotating sweep, with a shared falloff instead of per-view ones"""
    views, f, Rs = synth.rotating_views(n, 160, 220, seed=seed, step_deg=20.0)
    homos = np.stack([R.T @ np.diag([1.0 / f, 1.0 / f, 1.0]) for R in Rs])
    return views, shared_falloff(views, seed + 1, alpha), homos


# Thresholds, with margin, from the C restatement of the statistics and the linear blend with the solve (seeds 13 and 3):
# the curve comes back within 0.0012 of 1 - 0.3 rho, and the canvas error is 0.013 / 0.027 of the per-image gains' (linear).
# On vignetted()'s per-view falloffs (alpha_k in [0.2, 0.35], per-axis radius: not the model) it was 0.40 / 0.43 of it.
# DESIGN section 10.2 has the measured ratios.
CURVE_TOL, CANVAS_RATIO, PER_VIEW_BOUND = 0.01, 0.25, 1.0


@pytest.mark.parametrize("mb", [0, 4])
@pytest.mark.parametrize("seed", [13, 3])
def test_shared_falloff_recovered(ctx, mb, seed):
    n, alpha = 5, 0.3
    clean, vig, homos = quality_scene(n, seed, alpha)
    cfg = _cfg(MULTIBAND=mb)
    g, poly = hip.vignette_compensate(ctx, cfg, vig, homos, 2, n // 2)
    g_img = hip.gain_compensate(ctx, cfg, vig, homos, 2, n // 2)
    verr = np.abs(curve(poly, RHO) - (1 - alpha * RHO)).max()
    want = _canvas(hip.BlendCall(ctx, cfg, clean, homos, 2, n // 2))
    e_none = canvas_error(_canvas(hip.BlendCall(ctx, cfg, vig, homos, 2, n // 2)), want)
    e_img = canvas_error(_canvas(hip.BlendCall(ctx, cfg, vig, homos, 2, n // 2, gains=g_img)), want)
    e_vig = canvas_error(_canvas(hip.BlendCall(ctx, cfg, vig, homos, 2, n // 2, gains=g, vignette=poly)), want)
    print(f"\nshared falloff seed={seed} MB={mb}: a = {poly}, V err {verr:.5f}; canvas error none {e_none:.5f} image {e_img:.5f} "
          f"vignetting {e_vig:.5f} ratio {e_vig / e_img:.3f}")
    assert verr < CURVE_TOL, (poly, verr)
    assert e_img < e_none
    assert e_vig < CANVAS_RATIO * e_img, (e_vig, e_img)


@pytest.mark.parametrize("mb", [0, 4])
def test_per_view_falloff_bounded(ctx, mb):
    """vignetted(): every view has its own falloff on a per-axis radius -- the shared model is wrong on purpose; the error
    is reported and must not exceed the per-image gains' times PER_VIEW_BOUND"""
    n, seed = 5, 13
    clean, f, Rs = synth.rotating_views(n, 160, 220, seed=seed, step_deg=20.0)
    homos = np.stack([R.T @ np.diag([1.0 / f, 1.0 / f, 1.0]) for R in Rs])
    vig = vignetted(clean, seed + 1)
    cfg = _cfg(MULTIBAND=mb)
    g, poly = hip.vignette_compensate(ctx, cfg, vig, homos, 2, n // 2)
    g_img = hip.gain_compensate(ctx, cfg, vig, homos, 2, n // 2)
    want = _canvas(hip.BlendCall(ctx, cfg, clean, homos, 2, n // 2))
    e_img = canvas_error(_canvas(hip.BlendCall(ctx, cfg, vig, homos, 2, n // 2, gains=g_img)), want)
    e_vig = canvas_error(_canvas(hip.BlendCall(ctx, cfg, vig, homos, 2, n // 2, gains=g, vignette=poly)), want)
    print(f"\nper-view falloff MB={mb}: a = {poly}; canvas error image {e_img:.5f} vignetting {e_vig:.5f} ratio {e_vig / e_img:.3f}")
    assert e_vig < PER_VIEW_BOUND * e_img, (e_vig, e_img)


def test_determinism(ctx):
    n = 5
    _, vig, homos = quality_scene(n, seed=3)
    for mb in (0, 3):
        cfg = _cfg(MULTIBAND=mb)
        call = hip.BlendCall(ctx, cfg, vig, homos, 2, n // 2)
        s1 = call.vignette_overlap_sums(1, 0.98); s2 = call.vignette_overlap_sums(1, 0.98)
        assert np.array_equal(s1[0], s2[0]) and np.array_equal(s1[1], s2[1])
        g1, p1 = hip.vignette_solve(n, *s1); g2, p2 = hip.vignette_solve(n, *s2)
        assert np.array_equal(g1, g2) and np.array_equal(p1, p2)
        c = hip.BlendCall(ctx, cfg, vig, homos, 2, n // 2, gains=g1, vignette=p1)
        assert np.array_equal(_canvas(c), _canvas(c))


def test_device_entry_points_reject_bad_arguments(ctx):
    n = 3
    views, homos = synth.pano_scene(n, 60, 80, seed=2, proj="flat")
    call = hip.BlendCall(ctx, _flat_cfg(), views, homos, 0, 1)
    L = hip.lib()
    count = np.zeros(3, np.int64); mom = np.zeros((3, 30), np.int64)
    cp, mp = count.ctypes.data_as(C.c_void_p), mom.ctypes.data_as(C.c_void_p)
    args = lambda n_, stride, clip, c, m: (ctx.handle, C.byref(call.ccfg), C.byref(call.geom), call.arr, n_, stride, clip, c, m)
    for bad in ((n, 0, 0.98, cp, mp), (n, -2, 0.98, cp, mp), (n, 1, 0.0, cp, mp), (n, 1, 1.5, cp, mp), (n, 1, float("nan"), cp, mp),
                (n, 1, 0.98, None, mp), (n, 1, 0.98, cp, None), (0, 1, 0.98, cp, mp)):
        assert L.op_vignette_overlap(*args(*bad)) == -1, bad
        assert b"op_vignette_overlap" in L.op_last_error()
    h = C.c_void_p()
    g = np.ones((n, 3), np.float32)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        gb = g.copy(); gb[2, 1] = bad
        assert L.op_blend_vignette(ctx.handle, C.byref(call.ccfg), C.byref(call.geom), call.arr, n, gb.ctypes.data_as(C.c_void_p),
                                   np.zeros(3, np.float32).ctypes.data_as(C.c_void_p), C.byref(h)) == -1, bad
        assert b"op_blend_vignette" in L.op_last_error()
    for poly in ((-1.0, 0.0, 0.0), (-4.0, 4.0, 0.0), (float("nan"), 0.0, 0.0), (0.0, 0.0, float("inf"))):
        p = np.array(poly, np.float32)
        assert L.op_blend_vignette(ctx.handle, C.byref(call.ccfg), C.byref(call.geom), call.arr, n, g.ctypes.data_as(C.c_void_p),
                                   p.ctypes.data_as(C.c_void_p), C.byref(h)) == -1, poly
        assert b"curve" in L.op_last_error()
    # a pixel buffer of the ImageRef's own size is accepted; a cylinder pre-warped one (mat_h / mat_w another size) is not in
    # the lens frame: refused by both device entry points, before anything is read
    call.arr[1].mat_h = call.arr[1].h; call.arr[1].mat_w = call.arr[1].w
    assert L.op_vignette_overlap(*args(n, 1, 0.98, cp, mp)) == 0
    call.arr[1].mat_h = call.arr[1].h + 4; call.arr[1].mat_w = call.arr[1].w - 6
    assert L.op_vignette_overlap(*args(n, 1, 0.98, cp, mp)) == -4
    assert b"pre-warped" in L.op_last_error()
    assert L.op_blend_vignette(ctx.handle, C.byref(call.ccfg), C.byref(call.geom), call.arr, n, None, None, C.byref(h)) == -4
    assert b"pre-warped" in L.op_last_error()
    with pytest.raises(ValueError):
        hip.BlendCall(ctx, _flat_cfg(), views, homos, 0, 1, gains=np.ones((n, 2, 2, 3), np.float32), vignette=(0, 0, 0))


# ---- the C++ path ----
def _run_demo(tmp_path, views, mode, extra):
    n, h, w = len(views), views[0].shape[0], views[0].shape[1]
    fin, fout = tmp_path / "in.bin", tmp_path / ("out_%s_%s.bin" % (mode or "chain", "_".join(extra) or "plain"))
    with open(fin, "wb") as f:
        f.write(struct.pack("<3i", n, h, w))
        for v in views:
            f.write(np.ascontiguousarray(v, np.float32).tobytes())
    args = [DEMO, str(fin), str(fout), "42"] + ([mode] if mode else []) + list(extra)
    r = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return open(fout, "rb").read()


def test_stitch_demo_chain_vignetting(ctx, tmp_path):
    """stitch_demo's TRANS mode with --vignetting appends n x 3 gains and a1..a3 after the chain homographies; they equal
    the Python path's on those homographies exactly, and the panorama equals blend(gains=, vignette=) bit for bit"""
    assert os.path.exists(DEMO), "build it: make -C openpano_amd/csrc"
    n, h, w = 4, 240, 320
    views = shared_falloff(synth.image_set(n, h, w, seed=5, overlap=0.5), 17, 0.3)
    on = _run_demo(tmp_path, views, None, ["--vignetting"])
    per_image = _run_demo(tmp_path, views, None, ["--gain-compensation"])
    o = _skip_head(on, n)
    assert on[:o] == per_image[:o]
    H, W = struct.unpack_from("<2i", on, o)
    pano = np.frombuffer(on, np.float32, count=H * W * 3, offset=o + 8).reshape(H, W, 3)
    to_mid = np.frombuffer(on, np.float64, count=9 * n, offset=o + 8 + H * W * 12).reshape(n, 3, 3)
    tail = o + 8 + H * W * 12 + 72 * n
    assert len(on) == tail + 12 * n + 12
    gains_demo = np.frombuffer(on, np.float32, count=3 * n, offset=tail).reshape(n, 3)
    poly_demo = np.frombuffer(on, np.float32, count=3, offset=tail + 12 * n)
    cfg = PanoConfig(ESTIMATE_CAMERA=0, TRANS=1, ORDERED_INPUT=1, LAZY_READ=0)
    want_g, want_p = hip.vignette_compensate(ctx, cfg, views, to_mid, 0, n >> 1)
    assert np.array_equal(gains_demo, want_g) and np.array_equal(poly_demo, want_p)
    assert poly_demo[0] < -0.1, poly_demo
    want = _canvas(hip.BlendCall(ctx, cfg, views, to_mid, 0, n >> 1, gains=want_g, vignette=want_p))
    assert np.array_equal(pano, want)


def test_stitcher_build_vignetting(ctx, tmp_path):
    """HipStitcher::build() (stitch_demo camera_build) with vignetting: its panorama, gains and curve equal the staged camera
    mode's (hip_vignette_compensate + hip_blend by hand) bit for bit; those match the Python path's on the same cameras to
    rounding (the program sets homo_inv = K R itself, the Python path inverts homo, as test_gpu_gain.py)"""
    assert os.path.exists(DEMO), "build it: make -C openpano_amd/csrc"
    n, h, w = 5, 300, 400
    views, _, _ = synth.rotating_views(n, h, w, seed=77, step_deg=22.0)
    views = shared_falloff(views, 23, 0.3)
    staged = _run_demo(tmp_path, views, "camera", ["--vignetting"])
    built = _run_demo(tmp_path, views, "camera_build", ["--vignetting"])
    nt = 3 * n + 3
    o = _skip_head(staged, n)
    cams = np.frombuffer(staged, np.float64, count=13 * n, offset=o).reshape(n, 13).copy()
    o += 13 * n * 8
    H, W = struct.unpack_from("<2i", staged, o)
    assert len(staged) == o + 8 + H * W * 12 + 4 * nt
    pano = np.frombuffer(staged, np.float32, count=H * W * 3, offset=o + 8)
    assert struct.unpack_from("<2i", built, 0) == (H, W)
    assert len(built) == 8 + H * W * 12 + 4 * nt
    assert np.array_equal(np.frombuffer(built, np.float32, count=H * W * 3, offset=8), pano)
    assert built[8 + H * W * 12:] == staged[len(staged) - 4 * nt:]
    tail = np.frombuffer(built, np.float32, count=nt, offset=8 + H * W * 12)
    gains_demo, poly_demo = tail[:3 * n].reshape(n, 3), tail[3 * n:]
    homos = np.stack([_homo(c) for c in cams])
    cfg = _cfg()
    want_g, want_p = hip.vignette_compensate(ctx, cfg, views, homos, 2, n // 2)
    assert np.abs(gains_demo / want_g - 1).max() < 1e-3, np.abs(gains_demo / want_g - 1).max()
    assert np.abs(curve(poly_demo, RHO) - curve(want_p, RHO)).max() < 1e-3
    # the cameras are estimated from features here, not exact as in quality_scene: the curve lands 0.0125 from the truth
    # (a = (-0.343, 0.105, -0.074) on MI355X); the bound only checks that the C++ path recovers the falloff at all
    assert np.abs(curve(poly_demo, RHO) - (1 - 0.3 * RHO)).max() < 2.5 * CURVE_TOL
    want = _canvas(hip.BlendCall(ctx, cfg, views, homos, 2, n // 2, gains=gains_demo, vignette=poly_demo))
    got = pano.reshape(H, W, 3)
    assert want.shape == got.shape
    valid = (want[..., 0] >= 0) & (got[..., 0] >= 0)
    assert valid.mean() > 0.5 and np.mean((want[..., 0] >= 0) != (got[..., 0] >= 0)) < 2e-3
    assert np.abs(got[valid] - want[valid]).max() < 1e-4
