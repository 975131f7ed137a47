"""GPU: the SIFT step at the octave shapes and row-kernel segment heights that the aspect ratios of the other tests reach
only by accident (tests/sift_cases.py).  Every plane, list and descriptor equals the C oracle's, bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest

import sift_cases as sc

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
PINNED = (18, 24, 40)


@pytest.fixture(scope="module")
def ctx():
    from openpano_amd import hip
    c = hip.Context(0)
    yield c
    c.close()


def _oracle_stages(cfg, img):
    from checkers import Oracle
    return Oracle(cfg).sift_stages(img)


@pytest.mark.parametrize("h,w", sc.edge_shapes(16), ids=["%dx%d" % hw for hw in sc.edge_shapes(16)])
@pytest.mark.parametrize("texture", ["dense", "sparse"])
def test_edge_shapes_with_the_shipped_library(ctx, texture, h, w):
    """k_pyramid_rows at the segment height a single small image gets (16 rows): bands of 239, 240, 1 and 2 columns against
    last segments of 15, 16, 1 and 2 rows, odd and even widths, in every octave the shapes produce."""
    from openpano_amd import hip
    cfg = sc.cfg_for(h, w)
    img = getattr(sc, texture)(h, w, sc.shape_seed(h, w))
    o = _oracle_stages(cfg, img)
    assert o.dims[0] == (h, w) and len(o.desc) > 30
    sc._compare_stages(hip.sift_staged(ctx, cfg, img), o, cfg)


@pytest.fixture(scope="module")
def pinned_libs(tmp_path_factory):
    """one variant of the library per pinned segment height (-DOP_RW_SEG, csrc/sift_host.hip), built once for the module"""
    import variant_lib
    return {seg: variant_lib.build_variant(tmp_path_factory.mktemp("seg%d" % seg), "sift_host", ["-DOP_RW_SEG=%d" % seg]) for seg in PINNED}


CHILD = """import sys, numpy as np
sys.path[:0] = [%(root)r, %(tests)r]
from openpano_amd import hip
import sift_cases as sc
assert hip.LIB_PATH == %(lib)r
c = hip.Context(0)
for h, w in sc.edge_shapes(%(seg)d):
    st = hip.sift_staged(c, sc.cfg_for(h, w), sc.dense(h, w, sc.shape_seed(h, w)))
    sc.save_stages(%(out)r %% (h, w), st)
c.close()
"""


@pytest.mark.parametrize("seg", PINNED)
def test_edge_shapes_at_pinned_segment_heights(pinned_libs, tmp_path, seg):
    """The host layer picks the row kernel's segment height per batch (an even value in 16..40); the kernel keeps a four-row
    |DoG| ring indexed by row & 3, so heights with seg % 4 == 2 start their segments at another ring phase than 16, 24 and
    40.  A library compiled with the height pinned runs the dense images of edge_shapes(seg) in a child process; the planes
    are compared as well as the lists and descriptors, since a wrong row at a seam need not move a keypoint."""
    lib = pinned_libs[seg]
    out = str(tmp_path / "st_%dx%d.npz")
    code = CHILD % dict(root=os.path.dirname(HERE), tests=HERE, lib=lib, seg=seg, out=out)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, OPENPANO_HIP_LIB=lib), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    for h, w in sc.edge_shapes(seg):
        cfg = sc.cfg_for(h, w)
        o = _oracle_stages(cfg, sc.dense(h, w, sc.shape_seed(h, w)))
        g = sc.load_stages(out % (h, w))
        assert o.dims[0] == (h, w) and len(o.desc) > 1000
        octs = range(cfg.NUM_OCTAVE)                    # everything sift_staged returns came through the file
        assert sorted(g.grey) == list(octs) and sorted(g.dog) == [(oc, s) for oc in octs for s in range(cfg.NUM_SCALE - 1)]
        for kind in ("mag", "ort", "raw"):
            assert sorted(getattr(g, kind)) == [(oc, s) for oc in octs for s in range(1, cfg.NUM_SCALE - 2)], kind
        sc._compare_stages(g, o, cfg)


def test_batch_sizes_and_swizzle_tail(ctx):
    """k_pyramid_rows swizzles blockIdx over 8 XCDs and leaves the last gridDim.x % 8 blocks unswizzled; the item count, and
    with it the residue, follows the batch size: n copies of one dense 241 x 481 image, n = 1..9, 16 and 40, each image's
    features equal to the oracle's.  Which segment heights the chooser picks for these batches is not asserted here:
    test_edge_shapes_at_pinned_segment_heights carries that claim."""
    from checkers import Oracle
    from openpano_amd import hip
    h, w = sc.SEQ_H, sc.SEQ_W
    cfg = sc.cfg_for(h, w)
    img = sc.dense(h, w, 1)
    od, oc = Oracle(cfg).detect_feature(img)
    assert len(od) > 5000
    for n in list(range(1, 10)) + [16, 40]:
        f = hip.sift_batch(ctx, cfg, [img] * n)
        assert f.num_images == n and f.total == n * len(od), n
        for i in range(n):
            d, c = f.get(i)
            assert np.array_equal(d, od) and np.array_equal(c, oc), (n, i)
        f.free()


@pytest.mark.parametrize("name,kv,ndesc", sc.TINY, ids=[t[0] for t in sc.TINY])
def test_planes_smaller_than_the_kernels_units(ctx, name, kv, ndesc):
    """octaves below the 14-row window of the row kernel, below one 64 x 16 tile of the generic kernel, and below the Gaussian
    halo (15 over a 9 x 12 plane: every tap is a clamped one).  The last case has no descriptors: the planes are the check."""
    from openpano_amd import hip
    cfg = sc.tiny_cfg(kv)
    img = sc.dense(*sc.TINY_IMAGE)
    o = _oracle_stages(cfg, img)
    assert len(o.desc) == ndesc and len(o.dog) == cfg.NUM_OCTAVE * (cfg.NUM_SCALE - 1)
    sc._compare_stages(hip.sift_staged(ctx, cfg, img), o, cfg)


@pytest.mark.parametrize("h,w", sc.TILE_SHAPES, ids=["%dx%d" % hw for hw in sc.TILE_SHAPES])
@pytest.mark.parametrize("name,kv", sc.TILE_CONFIGS, ids=[t[0] for t in sc.TILE_CONFIGS])
def test_generic_tile_kernel_edges(ctx, name, kv, h, w):
    """k_pyramid<6> (NUM_SCALE=6) and k_pyramid<0> (GAUSS_WINDOW_FACTOR=4) on octave-0 sizes one short of, equal to and one past
    two 64-column and six 16-row tiles"""
    from openpano_amd import hip
    cfg = sc.cfg_for(h, w, **kv)
    img = sc.dense(h, w, sc.shape_seed(h, w))
    o = _oracle_stages(cfg, img)
    assert o.dims[0] == (h, w) and len(o.desc) > 100
    sc._compare_stages(hip.sift_staged(ctx, cfg, img), o, cfg)
