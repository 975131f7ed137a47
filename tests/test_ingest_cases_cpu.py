"""CPU: the cases of test_gpu_ingest.py (tests/ingest_cases.py), which run the SIFT ingest kernel off resize ratio 1.  The C
oracle equals the reference compiled in place at every one of them, stage by stage; the oracle alone shows what the GPU tests
rely on (working sizes on both sides of the tile seams, planes that carry information, indices that take the clamps of
resize_coord); and a numpy model of the octave section's candidate rectangle shows that it never misses an octave pixel and
never outgrows the kernel's coordinate tables."""
import numpy as np
import pytest

import ingest_cases as ic
import sift_cases as sc
from openpano_amd.config import PanoConfig

STAGED = ic.SEAM_CASES + ic.SMALL_SOURCES + ic.SCALE_ROWS + [ic.FALLBACK_CASE]
IDS = [c[0] for c in STAGED]


def _oracle_equals_ref(cfg, imgs, stages=True):
    """a Ref of its own per config (the reference keeps its configuration in globals: set before the first run, put back after)"""
    from checkers import Oracle, Ref, ref_available, sort_features
    if not ref_available():
        pytest.skip("oracle/_ref not built (reference sources absent)")
    ref = Ref(cfg)
    orc = Oracle(cfg)
    out = []
    try:
        for img in imgs:
            if stages:
                so = orc.sift_stages(img)
                sc.compare_oracle_ref(so, ref.sift_stages(img))
            else:
                so = sort_features(*orc.detect_feature(img))
                sr = sort_features(*ref.detect_feature(img))
                assert np.array_equal(so[0], sr[0]) and np.array_equal(so[1], sr[1])
            out.append(so)
    finally:
        ref.set_config(**{k: v for k, v in PanoConfig().raw_items()})
    return out


@pytest.mark.parametrize("case", STAGED, ids=IDS)
def test_oracle_equals_reference_off_ratio_one(case):
    """the fp32 image, the fp32 twin of its byte image and the twin of the three-channel byte image of every staged case"""
    imgs = [ic.f32_image(case), ic.twin(ic.u8_image(case)), ic.twin(ic.rgb_u8_image(case))]
    for so in _oracle_equals_ref(ic.cfg_of(case), imgs):
        assert so.dims[0] == ic.working_dims(*case[2])


@pytest.mark.parametrize("name,h,w,seed", ic.BIG_U8, ids=[b[0] for b in ic.BIG_U8])
def test_oracle_equals_reference_on_the_big_byte_images(name, h, w, seed):
    """default config: the thresholds leave noise next to no keypoints, so the planes are compared here as on the device"""
    so = _oracle_equals_ref(PanoConfig(), [ic.twin(ic.big_u8(h, w, seed))])[0]
    assert so.dims[0] == ic.working_dims(h, w, 800) and so.dims[0] != (h, w)
    assert all(so.gauss[(k, 0)].min() < so.gauss[(k, 0)].max() for k in range(4))


@pytest.mark.parametrize("cls,ws,shapes", ic.BATCHES, ids=[b[0] for b in ic.BATCHES])
def test_oracle_equals_reference_on_the_batch_images(cls, ws, shapes):
    """the images of test_batches_of_two_shapes_and_two_types: more than 100 descriptors each"""
    cfg = PanoConfig(SIFT_WORKING_SIZE=ws, **sc.LOOSE)
    for (wh, ww), src in zip(shapes, ic.batch_sources(cls, ws, shapes)):
        assert src is not None and ic.working_dims(*src) == (wh, ww) and src[0] + src[1] != 2 * ws
        case = ("batch", cls, src, {})
        for so in _oracle_equals_ref(cfg, [ic.f32_image(case), ic.twin(ic.u8_image(case))]):
            assert so.dims[0] == (wh, ww) and len(so.desc) > 100, (wh, ww, len(so.desc))


def test_fallback_case_outgrows_the_column_table():
    """SCALE_FACTOR = 0.9 makes octave 1 larger than the working image (43 x 128 -> 48 x 143).  The reference accepts it and
    the oracle equals it (the case is one of STAGED above), so the per-element branch of the octave section (tables == false)
    is live for an accepted config, and this is the case that runs it on the device: the candidate rectangle of a 64-column
    tile is longer than TC = 72 there, in the kernel's own arithmetic."""
    case = ic.FALLBACK_CASE
    wh, ww = ic.working_dims(*case[2])
    sf = ic.cfg_of(case).SCALE_FACTOR
    oh, ow = int(ic.octave_extent(wh, sf, 1)), int(ic.octave_extent(ww, sf, 1))
    assert (wh, ww) == (43, 128) and (oh, ow) == (48, 143)
    lo, hi = ic.candidate_rect(np.arange(0, ww, ic.WT), ic.WT, ww, ow)
    assert (hi - lo > ic.TC).any()
    lo, hi = ic.candidate_rect(np.arange(0, wh, ic.WR), ic.WR, wh, oh)
    assert (hi - lo <= ic.TR).all() and (hi - lo > 0).all()


@pytest.fixture(scope="module")
def oracle_runs():
    """id -> Oracle.sift_stages of the fp32 image, once per staged case"""
    from checkers import Oracle
    return {c[0]: Oracle(ic.cfg_of(c)).sift_stages(ic.f32_image(c)) for c in STAGED}


def test_working_sizes_reach_both_sides_of_the_tile_seams(oracle_runs):
    """from the oracle's dims, not from the search: per ratio class the seam cases reach 41, 42 and 43 rows (3 x 14 and one
    either side) and 127, 128 and 129 columns (2 x 64 and one either side); the large up-scale, whose source is 5 x 15 pixels,
    reaches 42 | 43 rows and 127 | 129 columns: a working image that ends at or before the seam, and one that needs a further
    tile, on both axes."""
    for cls, _ in ic.RATIOS:
        dims = [oracle_runs[c[0]].dims[0] for c in ic.SEAM_CASES if c[1] == cls]
        hs, ws = {d[0] for d in dims}, {d[1] for d in dims}
        if cls in ic.COARSE:
            assert hs <= set(ic.SEAM_H) and ws <= set(ic.SEAM_W), cls
            assert min(hs) <= 3 * ic.WR < max(hs) and min(ws) <= 2 * ic.WT < max(ws), (cls, hs, ws)
        else:
            assert hs == set(ic.SEAM_H) and ws == set(ic.SEAM_W), (cls, hs, ws)


def test_working_dims_and_resize_ratio(oracle_runs):
    for c in STAGED:
        sh, sw, ws = c[2]
        o = oracle_runs[c[0]]
        assert o.dims[0] == ic.working_dims(sh, sw, ws) and o.work.shape[:2] == o.dims[0], c[0]
        assert sh + sw != 2 * ws and o.dims[0] != (sh, sw), c[0]
        assert len(o.dims) == ic.cfg_of(c).NUM_OCTAVE and min(min(d) for d in o.dims) > 5, c[0]
        sf = ic.cfg_of(c).SCALE_FACTOR
        for k, d in enumerate(o.dims):
            assert d == (int(ic.octave_extent(o.dims[0][0], sf, k)), int(ic.octave_extent(o.dims[0][1], sf, k))) or k == 0, (c[0], k)


def test_every_grey_plane_carries_information(oracle_runs):
    """no grey plane of any case is constant (neither are its rows and columns at the border, which no extremum scan reaches)"""
    for c in STAGED:
        o = oracle_runs[c[0]]
        for k in range(len(o.dims)):
            g = o.gauss[(k, 0)]
            assert g.min() < g.max(), (c[0], k)
            for edge in (g[0], g[-1], g[:, 0], g[:, -1]):
                assert edge.min() < edge.max(), (c[0], k)


def test_clamps_of_resize_coord_per_ratio_class():
    """resize_coord in numpy fp32 on the sources of the seam cases.  The lower clamp (index -1 -> 0, weight 0) is taken where
    0.5 / f - 0.5 < 0 and the upper one (index srcn - 1 -> srcn - 2, weight 1) where the last destination index maps past
    srcn - 1.5: both happen exactly when the resize up-scales (f > 1).  So every up-scaling class has rows and columns on
    both clamps, in every case; a down-scaling class can take neither on any axis (asserted too: a clamp there would be an
    error of the restatement), and its first and last working rows / columns interpolate with weights strictly inside (0, 1)
    somewhere."""
    for cls, _ in ic.RATIOS:
        cases = [c for c in ic.SEAM_CASES if c[1] == cls]
        assert cases, cls
        for c in cases:
            sh, sw, ws = c[2]
            wh, ww = ic.working_dims(sh, sw, ws)
            for dn, sn in ((wh, sh), (ww, sw)):
                s, r, lo, hi = ic.resize_coord(np.arange(dn), ic.inv_factor(dn, sn), sn)
                assert s.min() >= 0 and s.max() <= sn - 2
                if cls in ic.UPSCALE:
                    assert lo.any() and hi.any() and not (lo & hi).any(), c[0]
                    assert lo[0] and hi[-1] and ((r > 0) & (r < 1)).any(), c[0]
                else:
                    assert not lo.any() and not hi.any(), c[0]
                    assert ((r > 0) & (r < 1)).any(), c[0]
    for c in ic.SMALL_SOURCES:          # a 2-pixel axis: EVERY index comes from a clamp
        sh, sw, ws = c[2]
        wh, ww = ic.working_dims(sh, sw, ws)
        for dn, sn in ((wh, sh), (ww, sw)):
            s, r, lo, hi = ic.resize_coord(np.arange(dn), ic.inv_factor(dn, sn), sn)
            assert lo.any() and hi.any(), c[0]
            if sn == 2:
                assert (lo | hi | (s == 0)).all() and (lo | hi).sum() > dn // 4, c[0]


MODEL_FACTORS = (2.0 ** 0.5, 2.0, 1.3, 1.2, 1.05)


def _rect_model(tile, scale_factor, o, lo_n=2, hi_n=2500):
    """every working extent n in [lo_n, hi_n] at once: every index d of octave o -> inside the rectangle of the tile that owns
    its top-left tap?  -> (misses, longest rectangle)"""
    n_all = np.arange(lo_n, hi_n + 1)
    on_all = ic.octave_extent(n_all, scale_factor, o)
    n = np.repeat(n_all, on_all)
    on = np.repeat(on_all, on_all)
    d = np.arange(on_all.sum()) - np.repeat(np.cumsum(on_all) - on_all, on_all)
    s, _, _, _ = ic.resize_coord(d, ic.inv_factor(on, n), n)
    assert (s >= 0).all() and (s + 1 < np.maximum(n, 2)).all()
    t0 = s // tile * tile
    lo, hi = ic.candidate_rect(t0, tile, n, on)
    # the longest rectangle over EVERY tile of every n, owners of no pixel included
    nt = -(-n_all // tile)
    tn = np.repeat(n_all, nt)
    tstart = (np.arange(nt.sum()) - np.repeat(np.cumsum(nt) - nt, nt)) * tile
    alo, ahi = ic.candidate_rect(tstart, tile, tn, np.repeat(on_all, nt))
    return int(((d < lo) | (d >= hi)).sum()), int((ahi - alo).max())


@pytest.mark.parametrize("scale_factor", MODEL_FACTORS, ids=["sf%.4g" % f for f in MODEL_FACTORS])
def test_candidate_rectangle_model(scale_factor):
    """The octave section of k_grey_octaves walks a "conservative candidate rectangle" of octave pixels per working tile and
    decides membership exactly inside it; a rectangle one pixel short would leave an octave pixel unwritten.  resize_coord,
    the rectangle (r_lo / r_hi / c_lo / c_hi) and the octave extent restated in numpy fp32 with the kernel's operation order,
    for tile extents 14 (rows) and 64 (columns), every working extent 2..2500, octaves 1..3 and SCALE_FACTOR sqrt(2), 2, 1.3,
    1.2 and 1.05: every octave index lies inside the rectangle of the tile that owns its top-left tap, and no rectangle is
    longer than the coordinate tables TR = 24 / TC = 72.  Longest rectangles found: 18 rows (SCALE_FACTOR 1.05, octave 1) and
    66 columns, so the kernel's per-element branch (tables == false) is out of reach of every SCALE_FACTOR >= 1
    (below 1 it is not: test_fallback_case_outgrows_the_column_table)."""
    longest = {}
    for tile, cap in ((ic.WR, ic.TR), (ic.WT, ic.TC)):
        for o in (1, 2, 3):
            miss, length = _rect_model(tile, scale_factor, o)
            assert miss == 0, (tile, o, miss)
            assert length <= cap, (tile, o, length)
            longest[tile] = max(longest.get(tile, 0), length)
    print("longest candidate rectangle at SCALE_FACTOR %.4g: %d rows, %d columns" % (scale_factor, longest[ic.WR], longest[ic.WT]))
    assert longest[ic.WR] <= 18 and longest[ic.WT] <= 66


def test_candidate_rectangle_outgrows_the_tables_below_scale_factor_one():
    """the model's own control: at SCALE_FACTOR 0.9 octave 3 is 1.37 x the working image and a 64-column tile's rectangle is
    longer than TC"""
    assert _rect_model(ic.WT, 0.9, 3, 200, 400)[1] > ic.TC
