"""CPU: the gain modes of the C oracle's blenders (oracle/blend_oracle.c: orc_blend_linear_gained /
orc_blend_multiband_gained), which judge the device blend's gains in tests/test_gpu_blend_paths.py.

1. mode 0 is the old entry points bit for bit, on every blend case of test_gpu_blend.py;
2. the gained linear blend equals the independent C restatements of tests/harness (blend_linear_block_ref,
   blend_linear_vig_ref) bit for bit, with asymmetric block grids, gains that clamp and gains exactly 1;
3. identities of the gained multiband blend: a uniform block map is its per-image gains, a zero curve is the plain
   gains, and power-of-two gains on views divided by them give the ungained canvas."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from openpano_amd import synth
from openpano_amd.config import PanoConfig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "tests", "harness", "vignette_overlap_ref.c")     # includes the block and per-image forms


def _cfg(**kv):
    base = dict(ESTIMATE_CAMERA=1, ORDERED_INPUT=0, LAZY_READ=0, MULTIBAND=0)
    base.update(kv)
    return PanoConfig(**base)


def _flat_cfg(**kv):
    return _cfg(ESTIMATE_CAMERA=0, TRANS=1, ORDERED_INPUT=1, **kv)


class GRefImage(C.Structure):
    _fields_ = [("data", C.c_void_p), ("h", C.c_int), ("w", C.c_int), ("mh", C.c_int), ("mw", C.c_int),
                ("hinv", C.c_double * 9), ("x0", C.c_int), ("y0", C.c_int), ("x1", C.c_int), ("y1", C.c_int)]


@pytest.fixture(scope="module")
def gref(tmp_path_factory):
    gcc = shutil.which("gcc") or shutil.which("cc")
    if not gcc:
        pytest.fail("a C compiler is needed for the CPU restatement")
    so = os.path.join(str(tmp_path_factory.mktemp("vigref")), "libvig_ref.so")
    subprocess.check_call([gcc, "-std=c11", "-O2", "-ffp-contract=off", "-fPIC", "-shared", HARNESS, "-o", so, "-lm"])
    L = C.CDLL(so)
    geo = [C.c_int] + [C.c_double] * 4 + [C.c_int] * 3 + [C.c_void_p]
    L.blend_linear_block_ref.argtypes = geo + [C.c_int] * 4 + [C.c_void_p, C.c_void_p]
    L.blend_linear_vig_ref.argtypes = geo + [C.c_int] * 2 + [C.c_void_p, C.c_void_p, C.c_void_p]
    return L


def _harness_inputs(oracle, views, homos, method, idx, cfg):
    """the harness's geometry head (method, min, resolution, H, W, n, images) from the oracle's own preparation"""
    geom, arr, keep, (H, W), meta = oracle.blend_inputs(views, homos, method, idx, cfg)
    n = len(views)
    g = (GRefImage * n)()
    for k in range(n):
        r = meta["ranges"][k]
        roi = [int((r[0] - geom.proj_min[0]) / geom.resolution[0]), int((r[1] - geom.proj_min[1]) / geom.resolution[1]),
               int((r[2] - geom.proj_min[0]) / geom.resolution[0]), int((r[3] - geom.proj_min[1]) / geom.resolution[1])]
        v = keep[k]
        g[k] = GRefImage(v.ctypes.data_as(C.c_void_p), v.shape[0], v.shape[1], v.shape[0], v.shape[1],
                         (C.c_double * 9)(*meta["homo_inv"][k]), *roi)
    head = (geom.proj_method, geom.proj_min[0], geom.proj_min[1], geom.resolution[0], geom.resolution[1], H, W, n, g)
    return head, keep


def _block_map(n, by, bx, seed, ones=True):
    """block gains in [0.6, 2.2] (the larger ones clamp bright samples), one image with a block of exact 1s"""
    G = np.random.default_rng(seed).uniform(0.6, 2.2, (n, by, bx, 3)).astype(np.float32)
    if ones:
        G[1] = 1.0
        G[n - 1, 0, 0, :] = 1.0
    return G


GAIN_SCENES = [                  # (proj, method, seed, cfg overrides)
    ("flat", 0, 71, dict(ESTIMATE_CAMERA=0, TRANS=1, ORDERED_INPUT=1)),
    ("camera", 1, 72, dict(ESTIMATE_CAMERA=0, CYLINDER=1, ORDERED_INPUT=1)),
    ("camera", 2, 73, dict()),
]


def test_gain_mode_none_is_the_plain_blend(oracle):
    """orc_blend_linear / orc_blend_multiband are the mode-0 calls: same canvas, bit for bit, on every case of test_gpu_blend"""
    from test_gpu_blend import CASES
    for proj, method, over, _ in CASES:
        cfg = _cfg(**over)
        views, homos = synth.pano_scene(5, 200, 280, seed=31 + method, proj=proj)
        got, _ = oracle.blend(views, homos, method, 2, cfg)
        geom, arr, keep, (H, W), _ = oracle.blend_inputs(views, homos, method, 2, cfg)
        want = np.empty((H, W, 3), np.float32)
        if cfg.MULTIBAND > 0:
            oracle.lib.orc_blend_multiband(C.byref(geom), arr, len(views), cfg.MULTIBAND, cfg.GAUSS_WINDOW_FACTOR, want.reshape(-1))
        else:
            oracle.lib.orc_blend_linear(C.byref(geom), arr, len(views), int(cfg.ORDERED_INPUT), int(cfg.LAZY_READ), want.reshape(-1))
        assert (want >= 0).mean() > 0.5
        assert np.array_equal(got, want), (proj, method, over)
        ones, _ = oracle.blend(views, homos, method, 2, cfg, gains=np.ones((5, 3), np.float32))
        assert np.array_equal(ones, want), (proj, method, over)     # gains exactly 1 leave every sample as it is


@pytest.mark.parametrize("proj,method,seed,over", GAIN_SCENES)
@pytest.mark.parametrize("lazy", [0, 1])
def test_gained_linear_equals_harness(oracle, gref, proj, method, seed, over, lazy):
    """two restatements of the gained linear blender agree bit for bit: block maps on grids that are not square, and the
    vignetting curve with per-image gains"""
    n = 5
    views, homos = synth.pano_scene(n, 120, 160, seed=seed, proj=proj, step=0.3)
    cfg = _cfg(LAZY_READ=lazy, **over)
    head, keep = _harness_inputs(oracle, views, homos, method, n // 2, cfg)
    H, W = head[5], head[6]
    plain, _ = oracle.blend(views, homos, method, n // 2, cfg)
    for by, bx in ((2, 3), (5, 1), (3, 5), (1, 16)):
        G = _block_map(n, by, bx, seed + bx)
        got, _ = oracle.blend(views, homos, method, n // 2, cfg, gains=G)
        want = np.zeros((H, W, 3), np.float32)
        assert gref.blend_linear_block_ref(*head, lazy, int(cfg.ORDERED_INPUT), bx, by, G.ctypes.data_as(C.c_void_p),
                                           want.ctypes.data_as(C.c_void_p)) == 0
        assert np.array_equal(got, want), (bx, by)
        assert not np.array_equal(got, plain)
        valid = got[..., 0] >= 0
        assert (got[valid] == 1.0).any()                              # some samples clamp
    gains = np.array([[1.0, 1.3, 0.8], [1.7, 1.0, 1.0], [0.9, 2.0, 1.2], [1.0, 1.0, 1.0], [1.4, 0.7, 1.9]], np.float32)
    for poly in ((-0.5, 0.4, -0.2), (0.3, 0.0, 0.0), (0.0, 0.0, 0.0)):
        a = np.array(poly, np.float32)
        got, _ = oracle.blend(views, homos, method, n // 2, cfg, gains=gains, vignette=a)
        want = np.zeros((H, W, 3), np.float32)
        assert gref.blend_linear_vig_ref(*head, lazy, int(cfg.ORDERED_INPUT), gains.ctypes.data_as(C.c_void_p),
                                         a.ctypes.data_as(C.c_void_p), want.ctypes.data_as(C.c_void_p)) == 0
        assert np.array_equal(got, want), poly
        if not a.any():                                               # a = 0: the per-image gains
            assert np.array_equal(got, oracle.blend(views, homos, method, n // 2, cfg, gains=gains)[0])


MB_SCENES = [                    # (proj, method, seed, cfg overrides): shipped and other window factors
    ("flat", 0, 81, dict(ESTIMATE_CAMERA=0, TRANS=1, ORDERED_INPUT=1, MULTIBAND=4)),
    ("camera", 1, 82, dict(ESTIMATE_CAMERA=0, CYLINDER=1, ORDERED_INPUT=1, MULTIBAND=5, GAUSS_WINDOW_FACTOR=4)),
    ("camera", 2, 83, dict(MULTIBAND=3, GAUSS_WINDOW_FACTOR=9)),
]


@pytest.mark.parametrize("proj,method,seed,over", MB_SCENES)
def test_gained_multiband_identities(oracle, proj, method, seed, over):
    n = 5
    views, homos = synth.pano_scene(n, 120, 160, seed=seed, proj=proj, step=0.3)
    cfg = _cfg(**over)
    gains = np.array([[1.0, 1.3, 0.8], [1.7, 1.0, 1.0], [0.9, 2.0, 1.2], [1.0, 1.0, 1.0], [1.4, 0.7, 1.9]], np.float32)
    per_image, _ = oracle.blend(views, homos, method, n // 2, cfg, gains=gains)
    plain, _ = oracle.blend(views, homos, method, n // 2, cfg)
    assert (plain >= 0).mean() > 0.5 and not np.array_equal(per_image, plain)
    # a uniform block map is its per-image gains, on any grid
    for by, bx in ((2, 3), (1, 5), (4, 4)):
        U = np.ascontiguousarray(np.broadcast_to(gains[:, None, None, :], (n, by, bx, 3)), np.float32)
        assert np.array_equal(oracle.blend(views, homos, method, n // 2, cfg, gains=U)[0], per_image), (bx, by)
    # a zero curve is the plain gains; a non-zero one is not
    assert np.array_equal(oracle.blend(views, homos, method, n // 2, cfg, gains=gains, vignette=np.zeros(3))[0], per_image)
    assert not np.array_equal(oracle.blend(views, homos, method, n // 2, cfg, gains=gains, vignette=(-0.5, 0.4, -0.2))[0], per_image)
    # power-of-two gains undo views divided by them exactly (nothing clamps: the views are in [0, 0.75])
    orig = [(v * np.float32(0.75)).astype(np.float32) for v in views]
    P = np.array([[2.0 ** (1 + (k + c) % 3) * (1 if k % 2 else 2) for c in range(3)] for k in range(n)], np.float32)
    P[3] = 1.0
    dark = [(v / P[k]).astype(np.float32) for k, v in enumerate(orig)]
    assert all(np.array_equal(d * P[k], o) for k, (d, o) in enumerate(zip(dark, orig)))
    want, _ = oracle.blend(orig, homos, method, n // 2, cfg)
    got, _ = oracle.blend(dark, homos, method, n // 2, cfg, gains=P)
    assert np.array_equal(got, want)
    swapped, _ = oracle.blend(dark, homos, method, n // 2, cfg, gains=P[:, ::-1].copy())
    assert not np.array_equal(swapped, want)
