"""GPU: blend, overlap passes and cylinder warp from decoder BYTES (OP_SRC_U8 / OP_U8) and from resident op_views.

The bar is bit equality everywhere: a byte b read as a source pixel is read_img's (float)b / 255.0 (lib/imgio.cc:55-57,78-80),
converted in the sampler, and everything after the four taps is the fp32 sequence of interpolate() -- so a canvas from byte
views equals the canvas from the fp32 views that conversion produces, which the C oracle computes.  The scene is 283 pixels
wide: 3 w is odd, so the sampler's two 6-byte runs land at every alignment mod 4."""
from openpano_amd.hip import Views          # the module needs the feature: without it, it fails here

import os
import struct
import subprocess

import numpy as np
import pytest

from openpano_amd import hip, synth
from openpano_amd.config import PanoConfig

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMO = os.path.join(ROOT, "openpano_amd", "host", "stitch_demo")
N, H, W, MID = 5, 200, 283, 2


def _cfg(**kv):
    base = dict(ESTIMATE_CAMERA=1, ORDERED_INPUT=0, LAZY_READ=0, MULTIBAND=0)
    base.update(kv)
    return PanoConfig(**base)


FLAT = dict(ESTIMATE_CAMERA=0, TRANS=1, ORDERED_INPUT=1)
# name -> (scene projection, proj_method, config overrides)
CASES = {
    "flat_linear": ("flat", 0, dict(FLAT)),
    "flat_lazy": ("flat", 0, dict(FLAT, LAZY_READ=1)),
    "flat_multiband4": ("flat", 0, dict(FLAT, MULTIBAND=4)),
    "cyl_linear": ("camera", 1, dict(ESTIMATE_CAMERA=0, CYLINDER=1, ORDERED_INPUT=1)),
    "sph_linear": ("camera", 2, dict()),
    "sph_multiband5": ("camera", 2, dict(MULTIBAND=5)),
}


def quantise(views):
    """(bytes b, the fp32 views f that read_img makes of them)"""
    b = [np.ascontiguousarray((np.asarray(v) * 255).astype(np.uint8)) for v in views]
    f = [(x.astype(np.float64) / 255).astype(np.float32) for x in b]
    return b, f


_scenes = {}


def scene(proj):
    """the module's scene of one projection: (bytes, fp32, homos), computed once and never modified"""
    if proj not in _scenes:
        views, homos = synth.pano_scene(N, H, W, seed=61 + (proj == "camera"), proj=proj)
        b, _ = quantise(views)
        b[1][40:56, 100:116] = np.arange(256, dtype=np.uint8).reshape(16, 16, 1)       # every byte value occurs
        f = [(x.astype(np.float64) / 255).astype(np.float32) for x in b]
        assert len(np.unique(np.concatenate([x.reshape(-1) for x in b]))) == 256
        for x in b + f:
            x.setflags(write=False)
        _scenes[proj] = (b, f, homos)
    return _scenes[proj]


def exposed_scene(proj):
    """the scene with a different exposure per view and a radial falloff, so that the solves return non-trivial gains"""
    key = proj + "+exposure"
    if key not in _scenes:
        _, f, homos = scene(proj)
        yy, xx = np.mgrid[0:H, 0:W]
        rho = ((xx - 0.5 * W) ** 2 + (yy - 0.5 * H) ** 2) / (0.25 * (W * W + H * H))
        fall = (1.0 - 0.3 * rho)[..., None]
        b, f = quantise([np.clip(v * e * fall, 0, 1) for v, e in zip(f, (0.85, 1.1, 0.95, 1.2, 0.9))])
        _scenes[key] = (b, f, homos)
    return _scenes[key]


_wants = {}


def want(name):
    """the oracle's canvas of a case, from the fp32 views; once per module"""
    if name not in _wants:
        from checkers import Oracle
        proj, method, over = CASES[name]
        cfg = _cfg(**over)
        _, f, homos = scene(proj)
        _wants[name] = Oracle(cfg).blend(f, homos, method, MID, cfg)[0]
        _wants[name].setflags(write=False)
    return _wants[name]


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.close()


def _canvas(ctx, cfg, images, homos, method, mid=MID, **kw):
    cv = hip.blend(ctx, cfg, images, homos, method, mid, **kw)
    got = cv.numpy(); cv.free()
    return got


def _device_bytes(b):
    """every view as device bytes at offset 1 of its own torch buffer of exactly nbytes + 1: unaligned, unpadded"""
    import torch
    keep, tuples = [], []
    for x in b:
        t = torch.empty(x.size + 1, dtype=torch.uint8, device="cuda")
        t[1:] = torch.from_numpy(x.reshape(-1).copy()).cuda()
        keep.append(t)
        tuples.append((t.data_ptr() + 1, x.shape[0], x.shape[1], "u8"))
    torch.cuda.synchronize()
    return tuples, keep


# ---- 1. blend against the oracle -------------------------------------------------------------------------------------
@pytest.mark.parametrize("source", ["host", "device_unaligned"])
@pytest.mark.parametrize("name", list(CASES))
def test_blend_from_bytes_equals_oracle(ctx, name, source):
    proj, method, over = CASES[name]
    b, _, homos = scene(proj)
    keep = None
    images = b
    if source == "device_unaligned":
        images, keep = _device_bytes(b)
    got = _canvas(ctx, _cfg(**over), images, homos, method)
    w = want(name)
    assert (w >= 0).mean() > 0.5
    assert np.array_equal(got, w)
    del keep


# ---- 2. the reference's own canvases -----------------------------------------------------------------------------------
def test_golden_fixture_from_its_bytes(ctx):
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "blend_sph_linear.npz"))
    views = [np.ascontiguousarray(v) for v in z["views"]]
    assert views[0].dtype == np.uint8
    for key, over in (("linear", dict()), ("multiband3", dict(MULTIBAND=3))):
        got = _canvas(ctx, _cfg(**over), views, z["homos"], 2, int(z["identity_idx"]))
        assert np.array_equal(got, z["canvas_" + key]), key


# ---- 3. mixed sets -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["flat_linear", "sph_multiband5"])
def test_mixed_set_equals_all_fp32(ctx, name):
    proj, method, over = CASES[name]
    b, f, homos = scene(proj)
    cfg = _cfg(**over)
    mixed = [b[k] if k in (0, 2) else f[k] for k in range(N)]
    assert np.array_equal(_canvas(ctx, cfg, mixed, homos, method), _canvas(ctx, cfg, f, homos, method))


# ---- 4. gain modes -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["flat_lazy", "sph_linear", "sph_multiband5"])
def test_overlap_passes_and_gained_blends(ctx, name):
    proj, method, over = CASES[name]
    b, f, homos = exposed_scene(proj)
    cfg = _cfg(**over)
    cb, cf = (hip.BlendCall(ctx, cfg, x, homos, method, MID) for x in (b, f))
    for a, c in ((cb.overlap_sums(), cf.overlap_sums()), (cb.block_overlap_sums(3, 2), cf.block_overlap_sums(3, 2)),
                 (cb.vignette_overlap_sums(), cf.vignette_overlap_sums())):
        assert a[0].dtype == np.int64 and a[1].dtype == np.int64 and a[0].sum() > 1000
        assert np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1])
    # non-trivial gains, from the fp32 solves
    gains = hip.gain_solve(N, *cf.overlap_sums())
    blocks = hip.gain_block_solve(N, 3, 2, *cf.block_overlap_sums(3, 2))
    vg, poly = hip.vignette_solve(N, *cf.vignette_overlap_sums())
    assert np.abs(gains - 1).max() > 1e-4 and np.abs(blocks - 1).max() > 1e-4 and np.abs(vg - 1).max() > 1e-6
    for kw in (dict(gains=gains), dict(gains=blocks), dict(gains=vg, vignette=poly)):
        assert np.array_equal(_canvas(ctx, cfg, b, homos, method, **kw), _canvas(ctx, cfg, f, homos, method, **kw)), list(kw)


# ---- 5. cylinder warp ----------------------------------------------------------------------------------------------------
def test_cyl_warp_from_bytes(ctx, cfg):
    world = synth.make_world(78, 130, 171)
    b, f = quantise([world[5:125, 5:166]])
    assert b[0].shape == (120, 161, 3)
    got, ref = (hip.cyl_warp(ctx, cfg, x, 1.0) for x in (b[0], f[0]))
    a, c = got.numpy(), ref.numpy(); got.free(); ref.free()
    assert (c >= 0).mean() > 0.5 and np.array_equal(a, c)
    dev, keep = _device_bytes(b)
    cv = hip.cyl_warp(ctx, cfg, dev[0], 1.0)
    a = cv.numpy(); cv.free()
    assert np.array_equal(a, c)
    del keep


# ---- 6. Views --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["u8", "f32"])
def test_views_feed_blend(ctx, dtype):
    b, f, homos = scene("flat")
    v = Views.upload(ctx, np.stack(b) if dtype == "u8" else f)      # a contiguous stack: one copy
    try:
        assert v.count == N and len(v) == N
        ims = v.images()
        assert [(i[1], i[2]) for i in ims] == [(H, W)] * N and all((len(i) == 4) == (dtype == "u8") for i in ims)
        arr = v.blend_images()
        assert [(arr[k].h, arr[k].w, arr[k].mat_h, arr[k].mat_w) for k in range(N)] == [(H, W, 0, 0)] * N
        assert all(arr[k].on_device == (hip.OP_SRC_DEVICE | (hip.OP_SRC_U8 if dtype == "u8" else 0)) for k in range(N))
        for name in ("flat_linear", "flat_multiband4"):
            _, method, over = CASES[name]
            assert np.array_equal(_canvas(ctx, _cfg(**over), v, homos, method), want(name)), name
    finally:
        v.free()


def test_views_feed_sift(ctx, cfg):
    world = synth.make_world(7, 200, 360, work_scale=1600.0 / (160 + 200), density=900.0)
    b, _ = quantise([world[10:170, 10:210], world[20:180, 120:320]])
    assert b[0].shape == (160, 200, 3)
    v = Views.upload(ctx, b)
    try:
        got = hip.sift_batch(ctx, cfg, v.images())
        ref = hip.sift_batch(ctx, cfg, b)
        for k in range(2):
            (d, c), (rd, rc) = got.get(k), ref.get(k)
            assert len(d) > 50 and np.array_equal(d, rd) and np.array_equal(c, rc), k
        got.free(); ref.free()
    finally:
        v.free()


def test_flag_word_is_checked(ctx):
    b, _, homos = scene("flat")
    call = hip.BlendCall(ctx, _cfg(**FLAT), b, homos, 0, MID)
    call.arr[3].on_device |= 4
    with pytest.raises(hip.OpenPanoHipError, match="error -1"):
        call()
    with pytest.raises(hip.OpenPanoHipError, match="error -1"):
        call.overlap_sums()


# ---- 7. stitch_demo --resident-views ----------------------------------------------------------------------------------------
def _demo(tmp_path, views, args, tag):
    n, (h, w) = len(views), views[0].shape[:2]
    fin = tmp_path / "in.bin"
    if not fin.exists():
        with open(fin, "wb") as f:
            f.write(struct.pack("<3i", n, h, w))
            for v in views:
                f.write(np.ascontiguousarray(v, np.float32).tobytes())
    fout = tmp_path / (tag + ".bin")
    pos, flags = [a for a in args if not a.startswith("--")], [a for a in args if a.startswith("--")]
    r = subprocess.run([DEMO] + flags[:1] + [str(fin), str(fout), "42"] + pos + flags[1:], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return open(fout, "rb").read()


@pytest.mark.parametrize("mode,flags,exact_bytes", [
    ("", [], True), ("camera_build", [], True), ("", ["--gain-compensation"], True), ("", [], False),
], ids=["chain", "camera_build", "chain_gain", "chain_fp32_fallback"])
def test_stitch_demo_resident_views(tmp_path, mode, flags, exact_bytes):
    assert os.path.exists(DEMO), "build it: make -C openpano_amd/csrc"
    if mode == "camera_build":
        views = synth.rotating_views(5, 300, 400, seed=77, step_deg=22.0)[0]
    else:
        views = synth.image_set(4, 240, 320, seed=5, overlap=0.5)
    if exact_bytes:
        views = quantise(views)[1]
    else:
        assert any(not np.array_equal(v, q) for v, q in zip(views, quantise(views)[1]))
    args = ([mode] if mode else []) + flags
    plain = _demo(tmp_path, views, args, "plain")
    resident = _demo(tmp_path, views, ["--resident-views"] + args, "resident")      # the flag first, the others after the positionals
    assert len(plain) > 240 * 320 * 3 * 4 and resident == plain


# ---- 8. smallest shapes ----------------------------------------------------------------------------------------------------
def _shift(dx, dy=0.0):
    return np.array([[1.0, 0, dx], [0, 1.0, dy], [0, 0, 1.0]])


@pytest.mark.parametrize("shapes,homos", [
    ([(2, 2), (3, 5)], [_shift(0), _shift(1.25, 0.5)]),
    ([(3, 5), (2, 2)], [_shift(0), _shift(-0.75, 0.25)]),
    ([(9, 13), (7, 6)], [_shift(0), _shift(3.5, 1.0)]),          # the second view's ROI ends on the canvas' right edge
], ids=["2x2_3x5", "3x5_2x2", "roi_on_canvas_edge"])
@pytest.mark.parametrize("mb", [0, 2])
def test_smallest_byte_views(ctx, shapes, homos, mb):
    from checkers import Oracle
    rng = np.random.default_rng(5)
    b = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in shapes]
    f = [(x.astype(np.float64) / 255).astype(np.float32) for x in b]
    cfg = _cfg(**dict(FLAT, MULTIBAND=mb))
    w, _ = Oracle(cfg).blend(f, np.stack(homos), 0, 0, cfg)
    got = _canvas(ctx, cfg, b, np.stack(homos), 0, mid=0)
    assert (w >= 0).any() and np.array_equal(got, w)
    dev, keep = _device_bytes(b)
    assert np.array_equal(_canvas(ctx, cfg, dev, np.stack(homos), 0, mid=0), w)
    del keep
