"""GPU: block gain compensation -- op_gain_block_overlap (csrc/overlap.hip) / op_gain_block_solve (photometric_solve.cc) / op_blend_block_gains (blend.hip).

1. the block statistics equal a CPU restatement (tests/harness/gain_block_overlap_ref.c) EXACTLY: counts and fixed-point
   int64 sums per unit pair, for every projection, both LAZY_READ branches, strides 1 and 3, grids 1 x 1, 3 x 2 and 4 x 4,
   pixels covered by 3+ images and a 70-view scene whose pairs straddle the 64-image cover word;
2. at 1 x 1 the block statistics are op_gain_overlap's and the block blend is op_blend_gains', bit for bit;
3. a uniform map G_k gives op_blend_gains(G)'s canvas, all-ones maps and NULL op_blend's, on every blend case of
   test_gpu_blend.py;
4. non-uniform maps give the canvas of a C restatement of the linear blend with the interpolated gains, bit for bit;
5. on views with vignetting and exposure differences, 4 x 4 block gains leave a much smaller overlap residual than
   per-image gains (the canvas error against the clean views is reported, and only bounded: see CANVAS_BOUND);
6. two runs give bit-equal statistics, gains and canvases;
7. the device entry points reject bad arguments and the statistics cap;
8. the C++ path (stitch_demo --gain-blocks) matches the Python path."""
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
HARNESS = os.path.join(ROOT, "tests", "harness", "gain_block_overlap_ref.c")
DEMO = os.path.join(ROOT, "openpano_amd", "host", "stitch_demo")
GRIDS = [(1, 1), (3, 2), (4, 4)]


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.close()


class GRefImage(C.Structure):
    _fields_ = [("data", C.c_void_p), ("h", C.c_int), ("w", C.c_int), ("mh", C.c_int), ("mw", C.c_int),
                ("hinv", C.c_double * 9), ("x0", C.c_int), ("y0", C.c_int), ("x1", C.c_int), ("y1", C.c_int)]


def build_ref(outdir):
    gcc = shutil.which("gcc") or shutil.which("cc")
    if not gcc:
        pytest.fail("a C compiler is needed for the CPU restatement")
    so = os.path.join(str(outdir), "libgain_block_ref.so")
    subprocess.check_call([gcc, "-std=c11", "-O2", "-ffp-contract=off", "-fPIC", "-shared", HARNESS, "-o", so, "-lm"])
    L = C.CDLL(so)
    geo = [C.c_int] + [C.c_double] * 4 + [C.c_int] * 3 + [C.c_void_p]
    L.gain_block_overlap_ref.argtypes = geo + [C.c_int] * 4 + [C.c_void_p, C.c_void_p]
    L.blend_linear_block_ref.argtypes = geo + [C.c_int] * 4 + [C.c_void_p, C.c_void_p]
    return L


@pytest.fixture(scope="module")
def gref(tmp_path_factory):
    return build_ref(tmp_path_factory.mktemp("gbref"))


def _cfg(**kv):
    base = dict(ESTIMATE_CAMERA=1, ORDERED_INPUT=0, LAZY_READ=0, MULTIBAND=0)
    base.update(kv)
    return PanoConfig(**base)


def _flat_cfg(**kv):
    return _cfg(ESTIMATE_CAMERA=0, TRANS=1, ORDERED_INPUT=1, **kv)


def _ref_geometry(call, views):
    """the restatement's image array, canvas size and geometry for a BlendCall"""
    g, n = call.geom, call.n
    arr = (GRefImage * n)()
    rois, keep = [], []
    for k in range(n):
        v = np.ascontiguousarray(views[k], np.float32); keep.append(v)
        r = [call.arr[k].range[q] for q in range(4)]
        roi = [int((r[0] - g.proj_min[0]) / g.resolution[0]), int((r[1] - g.proj_min[1]) / g.resolution[1]),
               int((r[2] - g.proj_min[0]) / g.resolution[0]), int((r[3] - g.proj_min[1]) / g.resolution[1])]
        rois.append(roi)
        arr[k] = GRefImage(v.ctypes.data_as(C.c_void_p), v.shape[0], v.shape[1], v.shape[0], v.shape[1],
                           (C.c_double * 9)(*call.arr[k].homo_inv), *roi)
    H = max(r[3] for r in rois); W = max(r[2] for r in rois)
    head = (g.proj_method, g.proj_min[0], g.proj_min[1], g.resolution[0], g.resolution[1], H, W, n, arr)
    return head, keep


def ref_block_stats(gref, call, views, cfg, stride, bx, by):
    head, keep = _ref_geometry(call, views)
    P, B = call.n * (call.n - 1) // 2, bx * by
    count = np.zeros((P, B, B), np.int64); sums = np.zeros((P, B, B, 6), np.int64)
    assert gref.gain_block_overlap_ref(*head, int(stride), int(cfg.LAZY_READ), bx, by, count.ctypes.data_as(C.c_void_p),
                                       sums.ctypes.data_as(C.c_void_p)) == 0
    return count, sums


def ref_blend_linear(gref, call, views, cfg, gains):
    """the linear blend with block gains (n, by, bx, 3)"""
    head, keep = _ref_geometry(call, views)
    H, W = head[5], head[6]
    g = np.ascontiguousarray(gains, np.float32)
    out = np.zeros((H, W, 3), np.float32)
    assert gref.blend_linear_block_ref(*head, int(cfg.LAZY_READ), int(cfg.ORDERED_INPUT), g.shape[2], g.shape[1],
                                       g.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)) == 0
    return out


def _canvas(call):
    cv = call(); x = cv.numpy(); cv.free()
    return x


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
def test_block_statistics_exact(ctx, gref, n, h, w, seed, proj, method, step, lazy, stride):
    views, homos = synth.pano_scene(n, h, w, seed=seed, proj=proj, step=step)
    cfg = _cfg(LAZY_READ=lazy) if method else _flat_cfg(LAZY_READ=lazy)
    call = hip.BlendCall(ctx, cfg, views, homos, method, n // 2)
    for bx, by in GRIDS:
        count, sums = call.block_overlap_sums(bx, by, stride)
        want_c, want_s = ref_block_stats(gref, call, views, cfg, stride, bx, by)
        assert count.sum() > 0
        assert np.array_equal(count, want_c), (bx, by, np.argwhere(count != want_c)[:5])
        assert np.array_equal(sums, want_s), (bx, by)
        if bx * by > 1:                  # the samples really spread over the blocks
            assert (count.sum(axis=0) > 0).sum() >= bx * by
    if step < 0.34:                      # some pixel is covered by 3+ images: a pair (a, a + 2) overlaps
        assert any(count[hip.pair_index(n, a, a + 2)].sum() > 0 for a in range(n - 2))


def test_block_statistics_exact_70_views(ctx, gref):
    """70 small views: pairs such as (62, 64) and (63, 65) straddle the first 64-image word of the cover bitmask"""
    n = 70
    views, homos = synth.pano_scene(n, 24, 40, seed=7, proj="flat", step=0.3)
    cfg = _flat_cfg()
    call = hip.BlendCall(ctx, cfg, views, homos, 0, n // 2)
    for bx, by in ((3, 2), (4, 4)):
        for stride in (1, 3):
            count, sums = call.block_overlap_sums(bx, by, stride)
            want_c, want_s = ref_block_stats(gref, call, views, cfg, stride, bx, by)
            assert np.array_equal(count, want_c) and np.array_equal(sums, want_s), (bx, by, stride)
    assert all(count[hip.pair_index(n, a, b)].sum() > 0 for a, b in ((62, 64), (63, 64), (63, 65)))


def test_block_statistics_exact_300_permuted_views(ctx, gref):
    """300 views on a permuted grid (tests/blend_cover_cases.py), 2 x 2 blocks: the second pass of overlap_walk's marking
    loop, tiles met by far more images than one chunk holds, and overlapping pairs whose indices lie more than 256 apart"""
    import blend_cover_cases as bc
    views, homos, idx = bc.overlap_scene()
    n = len(views)
    a, b = bc.pair_arrays(n)
    cfg = _flat_cfg()
    call = hip.BlendCall(ctx, cfg, views, homos, 0, idx)
    for stride in (1, 3):
        count, sums = call.block_overlap_sums(2, 2, stride)
        want_c, want_s = ref_block_stats(gref, call, views, cfg, stride, 2, 2)
        assert np.array_equal(count, want_c) and np.array_equal(sums, want_s), stride
        some = count.sum(axis=(1, 2)) > 0
        assert (some & (b - a > 256)).any() and (some & (a < 64) & (b >= 64)).any(), stride
        # neighbours lie 5, 10 pixels apart, a block is 6 x 5: a shared pixel falls into different blocks of the two views
        assert (count.sum(axis=0)[~np.eye(4, dtype=bool)] > 0).all()


@pytest.mark.parametrize("proj,method", [("flat", 0), ("camera", 1), ("camera", 2)])
@pytest.mark.parametrize("lazy", [0, 1])
def test_one_by_one_reduces_to_per_image(ctx, proj, method, lazy):
    n = 5
    views, homos = synth.pano_scene(n, 120, 160, seed=51 + method, proj=proj, step=0.3)
    G = np.random.default_rng(method).uniform(0.7, 1.4, (n, 3)).astype(np.float32)
    for mb in (0, 3):
        cfg = _cfg(LAZY_READ=lazy, MULTIBAND=mb) if method else _flat_cfg(LAZY_READ=lazy, MULTIBAND=mb)
        call = hip.BlendCall(ctx, cfg, views, homos, method, n // 2)
        for stride in (1, 2):
            c1, s1 = call.overlap_sums(stride)
            cb, sb = call.block_overlap_sums(1, 1, stride)
            assert np.array_equal(cb.reshape(-1), c1) and np.array_equal(sb.reshape(-1, 6), s1)
        want = _canvas(hip.BlendCall(ctx, cfg, views, homos, method, n // 2, gains=G))
        got = _canvas(hip.BlendCall(ctx, cfg, views, homos, method, n // 2, gains=G.reshape(n, 1, 1, 3)))
        assert np.array_equal(got, want), mb


def test_uniform_and_identity_maps(ctx):
    """every blend case of test_gpu_blend.py: a map whose blocks all equal G_k gives op_blend_gains(G)'s canvas bit for bit;
    all-ones maps and NULL give op_blend's"""
    from test_gpu_blend import CASES, _cfg as blend_cfg
    n = 5
    for proj, method, over, _ in CASES:
        cfg = blend_cfg(**over)
        views, homos = synth.pano_scene(n, 200, 280, seed=31 + method, proj=proj)
        plain = _canvas(hip.BlendCall(ctx, cfg, views, homos, method, 2))
        G = np.random.default_rng(method + 7).uniform(0.6, 1.5, (n, 3)).astype(np.float32)
        G[1, 1] = 1.0
        per_image = _canvas(hip.BlendCall(ctx, cfg, views, homos, method, 2, gains=G))
        assert not np.array_equal(per_image, plain)
        for bx, by in ((4, 4), (3, 2), (16, 1)):
            uni = np.ascontiguousarray(np.broadcast_to(G[:, None, None, :], (n, by, bx, 3)))
            got = _canvas(hip.BlendCall(ctx, cfg, views, homos, method, 2, gains=uni))
            assert np.array_equal(got, per_image), (proj, method, over, bx, by)
            ones = _canvas(hip.BlendCall(ctx, cfg, views, homos, method, 2, gains=np.ones((n, by, bx, 3), np.float32)))
            assert np.array_equal(ones, plain), (proj, method, over, bx, by)
        call = hip.BlendCall(ctx, cfg, views, homos, method, 2)
        h = C.c_void_p()
        hip.check(hip.lib().op_blend_block_gains(ctx.handle, C.byref(call.ccfg), C.byref(call.geom), call.arr, call.n, 4, 4, None, C.byref(h)))
        cv = hip.Canvas(ctx, h); null = cv.numpy(); cv.free()
        assert np.array_equal(null, plain), (proj, method, over)


@pytest.mark.parametrize("proj,method", [("flat", 0), ("camera", 1), ("camera", 2)])
@pytest.mark.parametrize("lazy", [0, 1])
@pytest.mark.parametrize("grid", [(4, 4), (3, 2), (1, 5)])
def test_block_gains_applied_per_sample(ctx, gref, proj, method, lazy, grid):
    """random non-uniform maps (some blocks exactly 1, some high enough to clamp) give the canvas of the C restatement of
    the linear blend with the interpolated gains bit for bit"""
    n = 5
    bx, by = grid
    views, homos = synth.pano_scene(n, 120, 160, seed=71 + method, proj=proj, step=0.3)
    views = [(v * np.float32(0.8)).astype(np.float32) for v in views]
    rng = np.random.default_rng(bx * 10 + by + method)
    G = rng.uniform(0.5, 1.6, (n, by, bx, 3)).astype(np.float32)
    G[rng.uniform(size=G.shape) < 0.15] = 1.0
    for ordered in (0, 1):
        if not method and not ordered:
            continue                     # TRANS requires ORDERED_INPUT (main.cc:257-258)
        cfg = _cfg(LAZY_READ=lazy, ORDERED_INPUT=ordered) if method else _flat_cfg(LAZY_READ=lazy)
        call = hip.BlendCall(ctx, cfg, views, homos, method, n // 2, gains=G)
        got = _canvas(call)
        want = ref_blend_linear(gref, call, views, cfg, G)
        assert (want[..., 0] >= 0).mean() > 0.5
        assert np.array_equal(got, want), (np.argwhere(got != want)[:5], ordered)
        per_image = _canvas(hip.BlendCall(ctx, cfg, views, homos, method, n // 2, gains=G.mean(axis=(1, 2))))
        assert not np.array_equal(got, per_image)


# ---- quality: vignetting + exposure ----
def vignetted(views, seed):
    """views x exposure e_k in [0.7, 1] x radial falloff 1 - alpha_k r^2 (alpha_k in [0.2, 0.35], r = 1 at the corners)"""
    rng = np.random.default_rng(seed)
    out = []
    for v in views:
        h, w = v.shape[:2]
        y, x = np.mgrid[0:h, 0:w].astype(np.float64)
        r2 = (((x + 0.5 - w / 2) / (w / 2)) ** 2 + ((y + 0.5 - h / 2) / (h / 2)) ** 2) / 2
        f = rng.uniform(0.7, 1.0) * (1 - rng.uniform(0.2, 0.35) * r2)
        out.append((v * f[..., None]).astype(np.float32))
    return out


def block_residual(count, sums, unit_gains, n, bx, by):
    """mean |g_{a,qa} I - g_{b,qb} I'| over the overlap samples (all channels), from the block statistics;
    unit_gains (n, B, 3)"""
    B = bx * by
    t = w = 0.0
    for a in range(n):
        for b in range(a + 1, n):
            p = hip.pair_index(n, a, b)
            N = count[p]
            if not N.any():
                continue
            qa, qb = np.nonzero(N)
            Nn = N[qa, qb].astype(np.float64)
            Ia = sums[p, qa, qb, :3] / (hip.GAIN_FIX * Nn[:, None]); Ib = sums[p, qa, qb, 3:] / (hip.GAIN_FIX * Nn[:, None])
            d = np.abs(unit_gains[a, qa] * Ia - unit_gains[b, qb] * Ib).mean(axis=1)
            t += (Nn * d).sum(); w += Nn.sum()
    return t / w


def canvas_error(got, clean):
    """RMS of got against the clean canvas after a least-squares global scale, over the pixels valid in both"""
    valid = (got[..., 0] >= 0) & (clean[..., 0] >= 0)
    x = got[valid].astype(np.float64); y = clean[valid].astype(np.float64)
    s = (x * y).sum() / (x * x).sum()
    return float(np.sqrt(((s * x - y) ** 2).mean()))


def quality_scene(n=5, seed=13):
    views, f, Rs = synth.rotating_views(n, 160, 220, seed=seed, step_deg=20.0)
    homos = np.stack([R.T @ np.diag([1.0 / f, 1.0 / f, 1.0]) for R in Rs])
    return views, vignetted(views, seed + 1), homos


# Thresholds, with margin, from the measured ratios: the overlap residual of 4 x 4 block gains is
# 0.61x the per-image one at the default sigmas.  The canvas error is NOT below the per-image one (1.14x, linear): a smooth
# field across the whole panorama -- the top / bottom falloff of a one-row sweep above all -- leaves every overlap
# unchanged, so the statistics cannot see it and the prior (1 - g)^2 chooses it; the bound below only keeps it from growing.
RESIDUAL_RATIO, CANVAS_BOUND = 0.75, 1.5


@pytest.mark.parametrize("mb", [0, 4])
def test_block_gains_reduce_overlap_residual(ctx, mb):
    n, bx, by = 5, 4, 4
    clean, vig, homos = quality_scene(n)
    cfg = _cfg(MULTIBAND=mb)
    count, sums = hip.BlendCall(ctx, cfg, vig, homos, 2, n // 2).block_overlap_sums(bx, by)
    c1, s1 = hip.gain_overlap_sums(ctx, cfg, vig, homos, 2, n // 2)
    g_img = hip.gain_solve(n, c1, s1)
    g_blk = hip.gain_block_solve(n, bx, by, count, sums)
    r_none = block_residual(count, sums, np.ones((n, bx * by, 3)), n, bx, by)
    r_img = block_residual(count, sums, np.repeat(g_img[:, None, :], bx * by, axis=1), n, bx, by)
    r_blk = block_residual(count, sums, g_blk.reshape(n, bx * by, 3), n, bx, by)
    want = _canvas(hip.BlendCall(ctx, cfg, clean, homos, 2, n // 2))
    e_none = canvas_error(_canvas(hip.BlendCall(ctx, cfg, vig, homos, 2, n // 2)), want)
    e_img = canvas_error(_canvas(hip.BlendCall(ctx, cfg, vig, homos, 2, n // 2, gains=g_img)), want)
    e_blk = canvas_error(_canvas(hip.BlendCall(ctx, cfg, vig, homos, 2, n // 2, gains=g_blk)), want)
    print(f"\nMB={mb} residual none {r_none:.5f} image {r_img:.5f} block {r_blk:.5f} ratio {r_blk / r_img:.3f}; "
          f"canvas error none {e_none:.5f} image {e_img:.5f} block {e_blk:.5f} ratio {e_blk / e_img:.3f}")
    assert r_img < r_none
    assert r_blk < RESIDUAL_RATIO * r_img, (r_blk, r_img)
    assert e_blk < CANVAS_BOUND * e_img, (e_blk, e_img)


def test_determinism(ctx):
    n, bx, by = 5, 4, 4
    _, vig, homos = quality_scene(n, seed=3)
    for mb in (0, 3):
        cfg = _cfg(MULTIBAND=mb)
        call = hip.BlendCall(ctx, cfg, vig, homos, 2, n // 2)
        s1 = call.block_overlap_sums(bx, by, 1); s2 = call.block_overlap_sums(bx, by, 1)
        assert np.array_equal(s1[0], s2[0]) and np.array_equal(s1[1], s2[1])
        g1 = hip.gain_block_solve(n, bx, by, *s1); g2 = hip.gain_block_solve(n, bx, by, *s2)
        assert np.array_equal(g1, g2)
        c = hip.BlendCall(ctx, cfg, vig, homos, 2, n // 2, gains=g1)
        assert np.array_equal(_canvas(c), _canvas(c))


def test_device_entry_points_reject_bad_arguments(ctx):
    n = 3
    views, homos = synth.pano_scene(n, 60, 80, seed=2, proj="flat")
    call = hip.BlendCall(ctx, _flat_cfg(), views, homos, 0, 1)
    L = hip.lib()
    count = np.zeros(3 * 16, np.int64); sums = np.zeros(3 * 16 * 6, np.int64)
    cp, sp = count.ctypes.data_as(C.c_void_p), sums.ctypes.data_as(C.c_void_p)
    args = lambda n_, stride, bx, by, c, s: (ctx.handle, C.byref(call.ccfg), C.byref(call.geom), call.arr, n_, stride, bx, by, c, s)
    for bad in ((n, 0, 2, 2, cp, sp), (n, -2, 2, 2, cp, sp), (n, 1, 0, 2, cp, sp), (n, 1, 2, 17, cp, sp), (n, 1, 2, 2, None, sp),
                (n, 1, 2, 2, cp, None), (0, 1, 2, 2, cp, sp)):
        assert L.op_gain_block_overlap(*args(*bad)) == -1, bad
        assert b"op_gain_block_overlap" in L.op_last_error()
    # the statistics cap: P * B^2 <= 2^22 entries (checked before anything is allocated or read)
    big_n = 70
    vb, hb = synth.pano_scene(big_n, 24, 40, seed=7, proj="flat", step=0.3)
    bcall = hip.BlendCall(ctx, _flat_cfg(), vb, hb, 0, big_n // 2)
    assert L.op_gain_block_overlap(ctx.handle, C.byref(bcall.ccfg), C.byref(bcall.geom), bcall.arr, big_n, 1, 16, 16, cp, sp) == -4
    assert b"exceed" in L.op_last_error()
    h = C.c_void_p()
    for bx, by in ((0, 1), (1, 0), (17, 2), (2, -1)):
        g = np.ones(3 * n * 4, np.float32)
        assert L.op_blend_block_gains(ctx.handle, C.byref(call.ccfg), C.byref(call.geom), call.arr, n, bx, by,
                                      g.ctypes.data_as(C.c_void_p), C.byref(h)) == -1, (bx, by)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        g = np.ones((n, 2, 2, 3), np.float32); g[2, 1, 0, 1] = bad
        assert L.op_blend_block_gains(ctx.handle, C.byref(call.ccfg), C.byref(call.geom), call.arr, n, 2, 2,
                                      g.ctypes.data_as(C.c_void_p), C.byref(h)) == -1, bad
        assert b"op_blend_block_gains" in L.op_last_error()


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


def test_stitch_demo_chain_gain_blocks(ctx, tmp_path):
    """stitch_demo's TRANS mode (flat projection, homographies chained to the middle image) with --gain-blocks 4x4 appends
    n x 4 x 4 x 3 gains after the chain homographies; they equal the Python path's on those homographies exactly, and the
    panorama equals blend(gains=) bit for bit.  --gain-blocks 1x1 is --gain-compensation byte for byte."""
    assert os.path.exists(DEMO), "build it: make -C openpano_amd/csrc"
    n, h, w = 4, 240, 320
    views = vignetted(synth.image_set(n, h, w, seed=5, overlap=0.5), 17)
    on = _run_demo(tmp_path, views, None, ["--gain-blocks", "4x4"])
    per_image = _run_demo(tmp_path, views, None, ["--gain-compensation"])
    assert _run_demo(tmp_path, views, None, ["--gain-blocks", "1x1"]) == per_image
    o = _skip_head(on, n)
    assert on[:o] == per_image[:o]
    H, W = struct.unpack_from("<2i", on, o)
    pano = np.frombuffer(on, np.float32, count=H * W * 3, offset=o + 8).reshape(H, W, 3)
    to_mid = np.frombuffer(on, np.float64, count=9 * n, offset=o + 8 + H * W * 12).reshape(n, 3, 3)
    tail = o + 8 + H * W * 12 + 72 * n
    assert len(on) == tail + 4 * 4 * 12 * n
    gains_demo = np.frombuffer(on, np.float32, count=n * 48, offset=tail).reshape(n, 4, 4, 3)
    cfg = PanoConfig(ESTIMATE_CAMERA=0, TRANS=1, ORDERED_INPUT=1, LAZY_READ=0)
    want_g = hip.gain_block_compensate(ctx, cfg, views, to_mid, 0, n >> 1, 4, 4)
    assert np.array_equal(gains_demo, want_g)
    assert np.ptp(want_g[..., 0].reshape(n, -1), axis=1).min() > 0.01
    want = _canvas(hip.BlendCall(ctx, cfg, views, to_mid, 0, n >> 1, gains=want_g))
    assert np.array_equal(pano, want)


def test_stitcher_build_gain_blocks(ctx, tmp_path):
    """HipStitcher::build() (stitch_demo camera_build) with gain_blocks 4 x 4: its panorama and gains equal the staged
    camera mode's (hip_gain_compensate_blocks + hip_blend by hand) bit for bit; those gains match the Python path's on the
    same cameras (the program sets homo_inv = K R itself, the Python path inverts homo: the geometry agrees to rounding,
    hence tolerances, as test_gpu_gain.py)"""
    assert os.path.exists(DEMO), "build it: make -C openpano_amd/csrc"
    n, h, w = 5, 300, 400
    views, _, _ = synth.rotating_views(n, h, w, seed=77, step_deg=22.0)
    views = vignetted(views, 23)
    extra = ["--gain-blocks", "4x4"]
    staged = _run_demo(tmp_path, views, "camera", extra)
    built = _run_demo(tmp_path, views, "camera_build", extra)
    ng = n * 16 * 3
    o = _skip_head(staged, n)
    cams = np.frombuffer(staged, np.float64, count=13 * n, offset=o).reshape(n, 13).copy()
    o += 13 * n * 8
    H, W = struct.unpack_from("<2i", staged, o)
    assert len(staged) == o + 8 + H * W * 12 + 4 * ng
    pano = np.frombuffer(staged, np.float32, count=H * W * 3, offset=o + 8)
    assert struct.unpack_from("<2i", built, 0) == (H, W)
    assert len(built) == 8 + H * W * 12 + 4 * ng
    assert np.array_equal(np.frombuffer(built, np.float32, count=H * W * 3, offset=8), pano)
    assert built[8 + H * W * 12:] == staged[len(staged) - 4 * ng:]
    gains_demo = np.frombuffer(built, np.float32, count=ng, offset=8 + H * W * 12).reshape(n, 4, 4, 3)
    homos = np.stack([_homo(c) for c in cams])
    cfg = _cfg()
    want_g = hip.gain_block_compensate(ctx, cfg, views, homos, 2, n // 2, 4, 4)
    assert np.abs(gains_demo / want_g - 1).max() < 1e-3, np.abs(gains_demo / want_g - 1).max()
    want = _canvas(hip.BlendCall(ctx, cfg, views, homos, 2, n // 2, gains=gains_demo))
    got = pano.reshape(H, W, 3)
    assert want.shape == got.shape
    valid = (want[..., 0] >= 0) & (got[..., 0] >= 0)
    assert valid.mean() > 0.5 and np.mean((want[..., 0] >= 0) != (got[..., 0] >= 0)) < 2e-3
    assert np.abs(got[valid] - want[valid]).max() < 1e-4


def _skip_head(buf, n):
    """offset just past the features and pairs sections of stitch_demo's output"""
    o = 0
    for _ in range(n):
        K = struct.unpack_from("<i", buf, o)[0]; o += 4 + K * 128 * 4 + K * 2 * 8
    npairs = struct.unpack_from("<i", buf, o)[0]; o += 4
    for _ in range(npairs):
        M = struct.unpack_from("<3i", buf, o)[2]; o += 12 + M * 8
        o += 4 + 4 + 9 * 8
        ninl = struct.unpack_from("<i", buf, o)[0]; o += 4 + ninl * 32
    return o


def _homo(c):
    """ImageComponent::homo = R^-1 K^-1 (stitcher.cc:154-158) of a camera (focal, aspect, ppx, ppy, R)"""
    f, aspect, ppx, ppy = c[:4]
    K = np.array([[f, 0, ppx], [0, f * aspect, ppy], [0, 0, 1]])
    R = c[4:].reshape(3, 3)
    return R.T @ np.linalg.inv(K)
