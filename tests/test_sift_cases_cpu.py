"""CPU: the shapes, configs and sequences of test_gpu_sift_shapes.py and test_gpu_sift_context_state.py (tests/sift_cases.py).
The C oracle equals the reference compiled in place at every one of them, stage by stage, and the oracle alone shows the
conditions the GPU tests rely on: extrema beside every seam of the row kernel, and the descriptor counts that decide which
batches outgrow the capacity predicted on the context."""
import numpy as np
import pytest

import sift_cases as sc
from openpano_amd.config import PanoConfig

SEGS = (16, 18, 40)
SHAPES = sorted({hw for seg in SEGS for hw in sc.edge_shapes(seg)})


def _fresh_ref(cfg):
    """a Ref of its own per config (the reference keeps its configuration in globals: set before the first run, put back after)"""
    from checkers import Ref, ref_available
    if not ref_available():
        pytest.skip("oracle/_ref not built (reference sources absent)")
    return Ref(cfg)


def _oracle_equals_ref(cfg, img):
    from checkers import Oracle
    ref = _fresh_ref(cfg)
    try:
        so = Oracle(cfg).sift_stages(img)
        sr = ref.sift_stages(img)
    finally:
        ref.set_config(**{k: v for k, v in PanoConfig().raw_items()})
    sc.compare_oracle_ref(so, sr)
    return so


@pytest.mark.parametrize("h,w", SHAPES, ids=["%dx%d" % hw for hw in SHAPES])
@pytest.mark.parametrize("texture", ["dense", "sparse"])
def test_oracle_equals_reference_at_edge_shapes(texture, h, w):
    cfg = sc.cfg_for(h, w)
    so = _oracle_equals_ref(cfg, getattr(sc, texture)(h, w, sc.shape_seed(h, w)))
    assert so.dims[0] == (h, w)
    assert len(so.desc) > (1000 if texture == "dense" else 30)


@pytest.mark.parametrize("name,kv,ndesc", sc.TINY, ids=[t[0] for t in sc.TINY])
def test_oracle_equals_reference_on_tiny_planes(name, kv, ndesc):
    so = _oracle_equals_ref(sc.tiny_cfg(kv), sc.dense(*sc.TINY_IMAGE))
    assert len(so.desc) == ndesc
    assert sum(v.size for v in so.dog.values()) > 0


def test_tiny_plane_sizes():
    """the octave sizes the tiny cases are there for: below the 14-row window, a 64 x 16 tile and the Gaussian halo"""
    from checkers import Oracle
    img = sc.dense(*sc.TINY_IMAGE)
    dims = {name: Oracle(sc.tiny_cfg(kv)).sift_stages(img, planes=False).dims for name, kv, _ in sc.TINY}
    assert dims["rows_20x27"][0] == (20, 27) and dims["rows_20x27"][-1] == (8, 10)
    assert dims["generic6_20x27"][0] == (20, 27)
    assert dims["halo15_5oct"][-1] == (9, 12) and len(dims["halo15_5oct"]) == 5
    assert dims["rows_13x18_3oct"][0] == (13, 18) and dims["rows_13x18_3oct"][-1] == (7, 9)


@pytest.mark.parametrize("name,kv", sc.TILE_CONFIGS, ids=[t[0] for t in sc.TILE_CONFIGS])
def test_oracle_equals_reference_around_the_generic_tile(name, kv):
    for h, w in sc.TILE_SHAPES:
        so = _oracle_equals_ref(sc.cfg_for(h, w, **kv), sc.dense(h, w, sc.shape_seed(h, w)))
        assert so.dims[0] == (h, w) and len(so.desc) > 100, (h, w)


@pytest.mark.parametrize("seg", (16, 18, 24, 40))
def test_dense_edge_shapes_have_extrema_beside_every_seam(seg):
    """what makes the plane and list comparisons of the GPU tests bite at the seams: octave 0 has raw extrema within 2 columns
    of the band seam at x = 240 (of the last scanned column where the plane ends before it) and within 2 rows of a segment seam
    (a multiple of ``seg`` inside the plane), at every dense edge shape"""
    from checkers import Oracle
    for h, w in sc.edge_shapes(seg):
        o = Oracle(sc.cfg_for(h, w)).sift_stages(sc.dense(h, w, sc.shape_seed(h, w)), planes=False)
        assert o.dims[0] == (h, w)
        xy = sc.raw_xy(o, 0)
        if w > sc.RW_OWN - 1:
            assert (np.abs(xy[:, 0] - sc.RW_OWN) <= 2).any(), (h, w)
        else:           # 239 columns: the scan ends at x = w - 2 = 237, out of reach of 240; the band's last two scanned columns instead
            assert (xy[:, 0] >= w - 3).any(), (h, w)
        seam = (xy[:, 1] + seg // 2) // seg * seg           # the nearest multiple of seg; rows 0 and h are edges, not seams
        assert ((np.abs(xy[:, 1] - seam) <= 2) & (seam > 0) & (seam < h)).any(), (h, w)


def test_descriptor_counts_of_the_context_sequences():
    """the counts test_gpu_sift_context_state.py reasons with (capK = max(2048 n, 1.25 x the previous batch's total))"""
    from checkers import Oracle
    im = sc.seq_images()
    orc = Oracle(sc.cfg_for(sc.SEQ_H, sc.SEQ_W))
    k = {name: len(orc.detect_feature(a)[0]) for name, a in im.items() if name not in ("Q1", "Q2")}
    raw = {name: len(sc.raw_xy(orc.sift_stages(im[name], planes=False))) for name in ("D1", "S")}
    assert 5000 < k["D1"] < 6000                                        # 1: > 2048
    assert k["D2"] + k["D3"] > max(4096, 1.25 * k["D1"]) and k["D2"] < max(4096, 1.25 * k["D1"])     # 2: the cut falls inside image 1
    assert k["F"] == 0                                                  # 3
    assert k["D1"] > 2048                                               # 4: capK back at its floor after the empty batch
    assert 30 < k["S"] < 1000 and 30 < k["S2"] < 1000                   # 5: no rerun, hints of a few hundred
    assert k["D2"] + k["S"] + k["D3"] > max(3 * 2048, 1.25 * k["S"])    # 6
    # 7: raw lists of 64 entries overflow, so the group reruns; the rerun's descriptors outgrow the floor of 2048 x 2, which
    # 1.25 x (the clamped first attempt's total, from at most 128 keypoints) does not lift
    assert raw["D1"] > 64 and raw["S"] > 64 and k["D1"] + k["S"] > 4096
    # 8: the second size group (under the call's config, so scaled up to 361 x 361) outgrows max(2048 x 2, 1.25 x the first
    # group's total), the first group stays below 2048 x 2
    first = k["S"] + k["S2"]
    second = sum(len(orc.detect_feature(im[q])[0]) for q in ("Q1", "Q2"))
    assert first <= 4096 and second > max(4096, 1.25 * first)
    # 9: chunk 0 (8 dense) outgrows 2048 x 8, chunk 1 (S / F) stays below max(2048 x 8, 1.25 x chunk 0)
    dense8 = sum(k["D%d" % (i % 3 + 1)] for i in range(8))
    assert dense8 > 8 * 2048 and 4 * k["S"] < 8 * 2048
