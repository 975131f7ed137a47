"""CPU: the claims of tests/blend_cover_cases.py, without a device.

1. the table holds the view counts and modes it is meant to;
2. every case reaches what it is there for, computed from the ROIs the call's own geometry gives (meta["geom"] /
   meta["ranges"]): the pixels whose covering images lie in different 64-image words, 256-image passes and 4096-image
   rounds, the seam coordinates, the pixels where a duplicated pair ties, a mostly covered canvas;
3. the C oracle equals the reference bit for bit on every case (skipped where oracle/_ref is absent);
4. a numpy model of tile_cover + walk_cover marks and visits exactly what the brute-force per-pixel walk does on every
   case, and under each one-line slip it differs on a named case -- and on none of them for a scene off the seams, which is
   what the blend tests had before."""
import numpy as np
import pytest

import blend_cover_cases as bc
from openpano_amd.config import PanoConfig

_ORACLE = {}


def _call(oracle, case):
    """(canvas, meta, ROIs) of the oracle on a case, computed once"""
    if case.name not in _ORACLE:
        _, twins, homos, idx = case.scene()
        want, meta = oracle.blend(twins, homos, 0, idx, case.cfg, **case.gain_args())
        want.setflags(write=False)
        _ORACLE[case.name] = (want, meta, bc.rois(meta))
    return _ORACLE[case.name]


def _geometries():
    """the distinct (scene, LAZY_READ, multiband) of the table with one case name each: what the cover walk depends on"""
    out = {}
    for c in bc.CASES:
        out.setdefault((c.scene_key, int(c.cfg.LAZY_READ), int(c.cfg.MULTIBAND > 0)), c.name)
    return out


GEOMETRIES = _geometries()


def test_table_holds_the_counts_and_modes():
    assert sorted(bc.GRID) == [64, 65, 128, 129, 256, 257, 4096, 4097, 4200]
    names = {c.name for c in bc.CASES}
    for n in bc.GRID:
        modes = ("linear", "ordered", "lazy", "mb3", "mb7") if n <= 257 else ("linear", "lazy", "mb3")
        assert {"grid%d-%s" % (n, m) for m in modes} <= names
        assert ("grid%d-mb7" % n in names) == (n <= 257)
    for s in bc.SEAMS:
        assert 3 <= len(bc.SEAMS[s][0]) <= 6
        assert {"seam_%s-%s" % (s, m) for m in ("ordered", "lazy", "mb3")} <= names
    assert {"gains4200-linear", "vignette257-linear", "block257-linear", "mixed129-linear"} <= names
    assert bc.MODES["linear"].ORDERED_INPUT == 0 and bc.MODES["ordered"].ORDERED_INPUT == 1 and bc.MODES["lazy"].LAZY_READ == 1
    assert bc.MODES["mb3"].MULTIBAND == 3 and bc.MODES["mb7"].MULTIBAND == 7
    assert len(names) == len(bc.CASES)
    # duplicated pairs sit in different halves, words, passes and rounds
    pairs = {n: bc.GRID[n][1] for n in bc.GRID}
    assert all(a < 32 <= b < 64 for a, b in pairs[64])
    assert all((a >> 6) != (b >> 6) for n in pairs if n > 64 for a, b in pairs[n])
    assert any((a >> 8) != (b >> 8) for a, b in pairs[257])
    assert any((a >> 12) != (b >> 12) for a, b in pairs[4097]) and any((a >> 12) != (b >> 12) for a, b in pairs[4200])
    assert any(a >= 4096 and (a >> 6) != (b >> 6) for a, b in pairs[4200])           # both in the second round, different words
    views, twins, _, _ = bc.scene(("mixed", 129))
    assert [v.dtype for v in views[:4]] == [np.float32, np.uint8, np.float32, np.uint8] and all(t.dtype == np.float32 for t in twins)


# (view count, LAZY_READ) -> pixels of the canvas covered by a ROI, and those whose covering images lie in different
# words / passes / rounds.  The ROI of a 12 x 10 view holds 13 x 11 = 143 pixels, 12 x 10 = 120 under LAZY_READ.
SPANS = {
    (64, 0): (2155, 0, 0, 0), (64, 1): (2150, 0, 0, 0),
    (65, 0): (2314, 143, 0, 0), (65, 1): (2235, 120, 0, 0),
    (128, 0): (3915, 3370, 0, 0), (128, 1): (3915, 3190, 0, 0),
    (129, 0): (4044, 3145, 0, 0), (129, 1): (3960, 2945, 0, 0),
    (256, 0): (7395, 6986, 0, 0), (256, 1): (7395, 6865, 0, 0),
    (257, 0): (7534, 7125, 143, 0), (257, 1): (7455, 6910, 120, 0),
    (4096, 0): (106604, 106444, 106284, 0), (4096, 1): (106290, 106100, 105855, 0),
    (4097, 0): (106624, 106479, 106233, 143), (4097, 1): (106315, 106135, 105790, 120),
    (4200, 0): (109049, 108882, 108729, 13960), (4200, 1): (108925, 108710, 108495, 11875),
}


@pytest.mark.parametrize("n,lazy", sorted(SPANS))
def test_grid_case_reaches_its_branch(oracle, n, lazy):
    case = bc.CASE["grid%d-%s" % (n, "lazy" if lazy else "ordered" if n <= 257 else "linear")]
    want, meta, R = _call(oracle, case)
    H, W = want.shape[:2]
    views, _, homos, idx = case.scene()
    # integer translations: every ROI is exactly (w + 1) x (h + 1) at (L, T), the identity view at the origin
    L = (homos[:, 0, 2] - bc.VIEW_W / 2).astype(int); T = (homos[:, 1, 2] - bc.VIEW_H / 2).astype(int)
    assert np.array_equal(R, np.stack([L, T, L + bc.VIEW_W, T + bc.VIEW_H], axis=1)) and tuple(R[idx]) == (0, 0, bc.VIEW_W, bc.VIEW_H)
    assert (H, W) == (int(R[:, 3].max()), int(R[:, 2].max()))
    sp = bc.cover_spans(R, H, W, lazy)
    got = (sp["covered"], sp["words"], sp["passes"], sp["rounds"])
    print("grid %d lazy %d: covered, words, passes, rounds = %s; deepest cover %d" % (n, lazy, got, int(sp["count"].max())))
    assert got == SPANS[(n, lazy)]
    roi = 143 if not lazy else 120
    if n == 65:
        assert sp["words"] == roi                           # one whole ROI: image 64 is alone in the second word
    if n == 257:
        assert sp["passes"] == roi                          # image 256 alone in the second pass
    if n == 4097:
        assert sp["rounds"] == roi                          # image 4096 alone in the second round
    if n == 4200:
        assert sp["rounds"] > SPANS[(4097, lazy)][3]
    assert sp["covered"] > 0.85 * H * W and int(sp["count"].max()) >= 7
    assert (want >= 0).mean() > 0.5                         # the canvas is mostly covered


@pytest.mark.parametrize("name", sorted(bc.SEAMS))
def test_seam_scene_coordinates(oracle, name):
    specs, claims = bc.SEAMS[name]
    for mode in bc.SEAM_MODES:
        want, meta, R = _call(oracle, bc.CASE["seam_%s-%s" % (name, mode)])
        assert [tuple(r) for r in R] == [(L, T, L + w, T + h) for L, T, w, h in specs]
        assert tuple(R[0][:2]) == (0, 0)
        for axis, values in claims.items():
            have = set(int(v) for v in R[:, ("x0", "y0", "x1", "y1").index(axis)])
            assert set(values) <= have, (axis, sorted(have))
        assert (want >= 0).mean() > 0.5
    R = _call(oracle, bc.CASE["seam_%s-ordered" % name])[2]
    H, W = _call(oracle, bc.CASE["seam_%s-ordered" % name])[0].shape[:2]
    if name == "x1":
        # x1 == j0 = 64: as far as the tile starting at 64 sees them, views 2 and 4 are one column wide; under LAZY_READ
        # that tile skips them while column 63 still gets them
        for k in (2, 4):
            assert R[k][2] == 64
            assert k in bc.brute_marks(R, H, W, 0)[(0, 1)] and k not in bc.brute_marks(R, H, W, 1)[(0, 1)]
            lists, _ = bc.brute_lists(R, H, W, 1)
            assert k in lists[int(R[k][1]), 63] and k not in lists[int(R[k][1]), 64]
    if name == "x0":
        assert {1, 4} <= set(bc.brute_marks(R, H, W, 0)[(0, 0)]) | set(bc.brute_marks(R, H, W, 0)[(0, 1)])
        assert 1 in bc.brute_marks(R, H, W, 0)[(0, 0)] and 2 not in bc.brute_marks(R, H, W, 0)[(0, 0)]        # x0 = 63 / 64
        assert 4 in bc.brute_marks(R, H, W, 0)[(0, 1)] and 5 not in bc.brute_marks(R, H, W, 0)[(0, 1)]        # x0 = 127 / 128


# (view count, pair) -> pixels where the pair decides the winner-takes-all map between its two copies
# (25 = the 5 x 5 pixels around a view's centre that lie nearer to it than to any neighbour on the 5-pixel pitch; more where
# a neighbouring cell is empty)
TIES = {
    (64, (3, 40)): 25, (65, (3, 64)): 46, (128, (3, 70)): 25, (129, (3, 70)): 25, (129, (5, 128)): 35,
    (256, (3, 70)): 25, (256, (5, 200)): 35, (257, (3, 70)): 64, (257, (5, 256)): 25,
    (4096, (3, 70)): 25, (4096, (5, 4000)): 25, (4097, (3, 70)): 25, (4097, (5, 4096)): 25,
    (4200, (3, 70)): 25, (4200, (5, 4099)): 25, (4200, (4097, 4170)): 25,
}


@pytest.mark.parametrize("n", sorted(bc.GRID))
def test_duplicated_pairs_tie(oracle, n):
    case = bc.CASE["grid%d-mb3" % n]
    want, meta, R = _call(oracle, case)
    H, W = want.shape[:2]
    views, _, homos, _ = case.scene()
    shapes = [v.shape[:2] for v in views]
    got = {}
    for pair in bc.GRID[n][1]:
        a, b = pair
        assert np.array_equal(homos[a], homos[b]) and views[a].shape == views[b].shape and not np.array_equal(views[a], views[b])
        got[(n, pair)] = bc.tie_pixels(R, shapes, pair, H, W)
    print("ties %s" % (got,))
    assert got == {k: v for k, v in TIES.items() if k[0] == n} and min(got.values()) > 0
    if n <= 257:
        # the order among equals is part of the result: with the two copies' contents exchanged the oracle's winner shows
        # the other content on at least that many pixels' worth of canvas
        for a, b in bc.GRID[n][1]:
            swapped = list(case.scene()[1])
            swapped[a], swapped[b] = swapped[b], swapped[a]
            other, _ = oracle.blend(swapped, homos, 0, case.scene()[3], case.cfg)
            assert other.shape == want.shape and int((other != want).any(axis=2).sum()) >= got[(n, (a, b))]


def test_overlap_scene_has_far_pairs(oracle):
    """the 300-view scene of the overlap statistics: pairs (a, b) with b - a > 256, and with a < 64 <= b, share valid samples
    on the lattices of stride 1 and 3 (what test_gpu_gain.py, test_gpu_gain_blocks.py and test_gpu_vignette.py assert of the
    device's counts), and a tile of lattice points meets more images than one 8-image chunk of the walk holds"""
    views, homos, idx = bc.overlap_scene()
    n = len(views)
    assert n == 300 and n > bc.PASS
    _, _, _, (H, W), meta = oracle.blend_inputs(views, homos, 0, idx, bc.MODES["ordered"])
    R = bc.rois(meta)
    # integer translations: image k's samples are valid on x0 .. x0 + w - 2, y0 .. y0 + h - 2
    xa, ya, xb, yb = R[:, 0], R[:, 1], R[:, 0] + bc.VIEW_W - 2, R[:, 1] + bc.VIEW_H - 2
    a, b = bc.pair_arrays(n)
    for stride in (1, 3):
        first = lambda lo: -(-lo // stride) * stride                    # the first lattice coordinate >= lo
        shared = (first(np.maximum(xa[a], xa[b])) <= np.minimum(xb[a], xb[b])) & (first(np.maximum(ya[a], ya[b])) <= np.minimum(yb[a], yb[b]))
        far, straddle = int((shared & (b - a > 256)).sum()), int((shared & (a < 64) & (b >= 64)).sum())
        print("stride %d: %d pairs share samples, %d of them more than 256 apart, %d across the first word" % (stride, int(shared.sum()), far, straddle))
        assert far >= 10 and straddle >= 100
        marks = bc.brute_marks(np.stack([R[:, 0] // stride, R[:, 1] // stride, R[:, 2] // stride, R[:, 3] // stride], axis=1),
                               -(-H // stride), -(-W // stride))
        assert max(len(m) for m in marks.values()) > 8 * (3 if stride == 1 else 8)


def test_gained_cases_have_an_ungained_twin():
    """the reference has no gain modes (those of the oracle are pinned by test_blend_oracle_gains.py): what it can confirm of
    a gained case is the same call without gains, and that call is a case of its own"""
    plain = {(c.scene_key, c.mode) for c in bc.CASES if c.gains is None}
    gained = [c for c in bc.CASES if c.gains is not None]
    assert len(gained) == 6 and all((c.scene_key, c.mode) in plain for c in gained)


@pytest.mark.parametrize("name", [c.name for c in bc.CASES if c.gains is None])
def test_oracle_equals_reference(oracle, ref, name):
    """every call of the table (the byte views go in as the floats read_img makes of them)"""
    case = bc.CASE[name]
    _, twins, homos, idx = case.scene()
    ref.set_config(**{k: v for k, v in case.cfg.raw_items()})
    ref.lib.ref_set_threads(1)
    try:
        want, wmeta = ref.blend(twins, homos, 0, idx)
    finally:
        ref.set_config(**{k: v for k, v in PanoConfig().raw_items()})
    got, gmeta, _ = _call(oracle, case)
    for k in ("geom", "ranges", "homo_inv"):
        assert np.array_equal(wmeta[k], gmeta[k]), k
    assert want.shape == got.shape and (want >= 0).mean() > 0.5
    assert np.array_equal(want, got)


def _extent(oracle, key):
    scene_key, lazy, mb = key
    want, meta, R = _call(oracle, bc.CASE[GEOMETRIES[key]])
    H, W = want.shape[:2]
    return R, H + mb, W + mb              # the multiband first level covers (H + 1) x (W + 1)


@pytest.mark.parametrize("key", sorted(GEOMETRIES, key=str), ids=lambda k: "%s%s-lazy%d-mb%d" % (k[0] + k[1:]))
def test_model_visits_the_brute_force_lists(oracle, key):
    R, H, W = _extent(oracle, key)
    assert bc.model_differs(R, H, W, key[1], None) is None


# slip -> the (scene, LAZY_READ, multiband extent) that sees it
SEEN_BY = {
    "x0_lt": (("seam", "x0"), 0, 0),                  # x0 = 63 and 127: the image is gone from the tile that holds its first column
    "x1_lt": (("seam", "x1"), 0, 0),                  # x1 = 64 and 128: gone from the tile that holds its last column
    "y0_lt": (("seam", "y0"), 0, 0),                  # y0 = 3 and 7
    "y1_lt": (("seam", "y1"), 0, 0),                  # y1 = 4 and 8
    "excl_forgotten": (("seam", "x1"), 1, 0),         # x1 = 64 under LAZY_READ: the tile at 64 marks an image none of its pixels takes
    "excl_always": (("seam", "x1"), 0, 0),            # x1 = 64 without LAZY_READ: column 64 loses the image
    "walk_words_floor": (("grid", 65), 0, 0),         # image 64 is marked and never visited
    "mark_bound_floor": (("grid", 65), 0, 0),         # the wave that holds image 64 never ballots: the walk reads an unwritten word
    "k1_arms_swapped": (("grid", 4097), 0, 0),        # round 1 marks 4096 images of a table that has one left
    "hi_before_lo": (("grid", 64), 0, 0),             # the fp32 sums and the winner among equals change with the order
    "k0_dropped": (("grid", 4097), 0, 0),             # the second round visits image 0 for image 4096
}


@pytest.mark.parametrize("slip", bc.SLIPS)
def test_each_slip_is_seen_by_its_case(oracle, slip):
    key = SEEN_BY[slip]
    R, H, W = _extent(oracle, key)
    how = bc.model_differs(R, H, W, key[1], slip)
    print("%s on %s: %s" % (slip, GEOMETRIES[key], how))
    assert how is not None
    if slip == "k1_arms_swapped":
        # at exactly 4096 images both arms give k1 = n = k0 + 4096: neither `<` for `<=` nor the swapped arms change that
        # call, the counts on either side of it do (4097 above; every count below 4096 reads past the table as well)
        R, H, W = _extent(oracle, (("grid", 4096), 0, 0))
        assert bc.model_differs(R, H, W, 0, slip) is None
        R, H, W = _extent(oracle, (("grid", 64), 0, 0))
        assert bc.model_differs(R, H, W, 0, slip).startswith("fault")
    if slip in ("x0_lt", "x1_lt", "y0_lt", "y1_lt", "excl_always"):
        assert "pixels visit another number" in how            # a column or row of one image's contribution is gone
    if slip == "excl_forgotten":
        assert "tiles mark another set" in how                 # costs a tile's walk an image, changes no pixel


def test_no_slip_is_seen_off_the_seams():
    """three views as the older blend tests place them -- no border on a tile boundary, fewer than 32 images: every slip of
    the tile test and of the walk leaves the lists as they are (the ones that fault need a count no multiple of 64, which
    those tests have)"""
    R = np.array([(0, 0, 100, 30), (70, 1, 170, 31), (150, 2, 240, 30)])
    H, W = 31, 240
    loud = [s for s in bc.SLIPS if any(bc.model_differs(R, H, W, lazy, s) is not None for lazy in (0, 1))]
    assert set(loud) == {"walk_words_floor", "mark_bound_floor", "k1_arms_swapped"}, loud
    assert bc.model_differs(R, H, W, 0, None) is None and bc.model_differs(R, H, W, 1, None) is None
