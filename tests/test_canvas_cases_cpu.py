"""CPU: the cases of test_gpu_canvas.py (tests/canvas_cases.py), which hold the canvas stage (csrc/canvas.hip) at its edges.
Every crop family states what it is for -- which search of k_crop_lines it forces, which tie it sets up -- and that claim is
asserted here on the mask of the canvas the oracle blends, as the GPU tests assert it on the canvas they read back.  crop_model,
written from the definition of the reference's rule, equals a literal restatement of that definition, the C oracle (a
line-for-line port of the reference's pointer jumping) and, where oracle/_ref is built, the reference itself; the byte model
equals the oracle's quantisation at the values where fl32(v * 255) sits on an integer or one ulp below; the cylinder cases are
non-empty, carry Color::NO through and equal the reference off the default focal length.  No GPU is needed, but the cache-pair
test calls hip.cyl_warp_shape (host code of libopenpano_hip.so), so the library has to be built."""
import numpy as np
import pytest

import canvas_cases as cc
from openpano_amd.config import PanoConfig

NOPTS = np.zeros((0, 2))


@pytest.fixture(scope="module")
def orc():
    from checkers import Oracle
    return Oracle(cc.blend_cfg())


@pytest.fixture(scope="module")
def canvases(orc):
    """id -> the oracle's canvas of every crop case, blended once"""
    return {c.id: orc.blend([cc.view_of(c)], cc.HOMO, 0, 0)[0] for c in cc.CROP_CASES}


# ---- the model ---------------------------------------------------------------------------------------------------------------

def _literal_crop(mask):
    """the definition, one scan at a time: -> (x0, y0, w, h, n_ties)"""
    h, w = mask.shape
    height = cc.heights_of(mask)
    cands = []
    for line in range(h):
        for k in range(w):
            hk = height[line, k]
            if hk == 0:
                continue
            left = k
            while left > 0 and height[line, left - 1] >= hk:
                left -= 1
            right = k
            while right + 1 < w and height[line, right + 1] >= hk:
                right += 1
            cands.append(((right - left + 1) * hk, (left, line - hk + 1, right - left + 1, hk)))
    best, rect = 0, (0, 1, 1, 0)
    for area, r in cands:
        if area > best:
            best, rect = area, r
    return tuple(int(x) for x in rect) + (sum(1 for area, r in cands if area == best and r != rect),)


def _random_masks(n, max_h, max_w, seed):
    rng = np.random.default_rng(seed)
    for _ in range(n):
        h, w = int(rng.integers(1, max_h + 1)), int(rng.integers(1, max_w + 1))
        yield rng.random((h, w)) < rng.choice([0.5, 0.7, 0.85, 0.95])


def test_crop_model_equals_the_literal_definition():
    ties = 0
    for m in _random_masks(150, 9, 15, 11):
        want = _literal_crop(m)
        assert cc.crop_model(m) == want, m.astype(int)
        ties += want[4] > 0
    assert ties >= 30                        # a fifth of the masks at least
    assert cc.crop_model(np.zeros((4, 5), bool)) == (0, 1, 1, 0, 0) == _literal_crop(np.zeros((4, 5), bool))


def test_crop_model_equals_oracle_on_random_masks(orc):
    """300 masks up to 11 x 19, a fifth of them at least with a tie for the largest area"""
    ties = 0
    for m in _random_masks(300, 11, 19, 12):
        mat = np.where(m[..., None], np.float32(0.5), np.float32(-1)) * np.ones(3, np.float32)
        got, off = orc.crop(mat)
        x0, y0, w, h, n = cc.crop_model(m)
        assert off == (x0, y0) and got.shape[:2] == (h, w), m.astype(int)
        ties += n > 0
    assert ties >= 60, ties


# ---- the identity blend ------------------------------------------------------------------------------------------------------

def test_identity_blend_mask_transform(orc, canvases):
    """what canvas_cases.py builds on: the canvas has the view's shape; pixel (i, j) is valid exactly where the view's
    pixels (i..i+1, j..j+1) all are, and never in column 0, the last column or the last row; an invalid pixel is Color::NO in
    all three channels and a valid one is the view's colour to within one ulp"""
    for c in cc.CROP_CASES:
        view, cv = cc.view_of(c), canvases[c.id]
        assert cv.shape == view.shape, c.id
        v = c.vmask
        want = np.zeros(v.shape, bool)
        want[:-1, 1:-1] = (v[:-1, :-1] & v[:-1, 1:] & v[1:, :-1] & v[1:, 1:])[:, 1:]
        m = cc.canvas_mask(cv)
        assert np.array_equal(m, want), c.id
        assert (cv[~m] == -1).all() and (cv[m] >= 0).all(), c.id
        assert (np.abs(cv[m] - view[m]) <= np.spacing(view[m])).all(), c.id


# ---- crop: what each family claims, and oracle == model ---------------------------------------------------------------------

@pytest.mark.parametrize("case", cc.CROP_CASES, ids=[c.id for c in cc.CROP_CASES])
def test_crop_case_is_what_it_claims_and_oracle_equals_model(orc, canvases, case):
    cv = canvases[case.id]
    x0, y0, w, h = cc.check_family(case, cc.canvas_mask(cv))
    got, off = orc.crop(cv)
    assert off == (x0, y0) and got.shape == (h, w, 3)
    assert np.array_equal(got, cv[y0: y0 + h, x0: x0 + w]) and (got >= 0).all()


def test_tie_cases_cover_the_thread_layouts():
    """family D: the two first-maximum columns in one thread of k_crop_lines (k2 = k1 + 256), in neighbouring threads
    (k2 = k1 + 1, once across a multiple of 256) and with the later column at the lower thread id; family E: the two lines in
    neighbouring threads of k_crop_pick, in threads 255 and 0, and in one thread (l + 256)"""
    d = [(c.info["k1"], c.info["k2"]) for c in cc.FAMILY_D]
    assert any(k2 == k1 + cc.THREADS for k1, k2 in d) and any(k2 == k1 + 1 for k1, k2 in d)
    assert sum(k1 % cc.THREADS > k2 % cc.THREADS for k1, k2 in d) >= 3 and any(k2 % cc.THREADS == 0 for k1, k2 in d)
    e = [(c.info["line1"], c.info["line2"]) for c in cc.FAMILY_E]
    assert any(b == a + 1 for a, b in e) and any(b == a + cc.THREADS for a, b in e)
    assert any(b == a + 1 and a % cc.THREADS == cc.THREADS - 1 for a, b in e) and max(b for a, b in e) > cc.THREADS
    widths = {c.vmask.shape[1] for c in cc.CROP_SMALL}
    assert {2, 3, 63, 64, 65, 66, 128, 129, 255, 256, 257, 258, 513, 1030} <= widths


def test_wide_cases_sit_on_the_limits():
    assert [c.vmask.shape[1] for c in cc.FAMILY_H] == [16500, 37809, 37810]
    assert 64 * 1024 < cc.crop_lds_bytes(16500) == 67032 < cc.CROP_LDS_MAX
    assert cc.crop_lds_bytes(37809) == 4 * (37809 + 591) == cc.CROP_LDS_MAX < cc.crop_lds_bytes(37810) == 4 * (37810 + 591)


# ---- bytes -------------------------------------------------------------------------------------------------------------------

def test_byte_canvas_holds_the_values_it_aims_at(orc):
    cv = orc.blend([cc.byte_view()], cc.HOMO, 0, 0)[0]
    m = cc.canvas_mask(cv)
    assert m[:16, 1:81].all() and not m[16:].any() and cv[m].min() == 0 and cv[m].max() == 1
    want = cc.byte_model(cv)
    assert len(np.unique(want[m])) == 256 and (want[~m] == 255).all()
    on, below = cc.on_integer(cv[m])
    print("values on an integer: %d (%d distinct), one ulp below: %d (%d distinct)"
          % (on.sum(), len(np.unique(cv[m][on])), below.sum(), len(np.unique(cv[m][below]))))
    assert len(np.unique(cv[m][on])) >= 200 and len(np.unique(cv[m][below])) >= 200
    assert ((cv[m] > 0) & (cv[m] < np.finfo(np.float32).tiny)).any()          # a denormal (the blend's weights make 0 or 3e-45 of 1e-45)
    assert np.array_equal(orc.to_u8(cv), want)
    # the two edges disagree by one byte, so a product rounded another way shows: the values one ulp below truncate down
    p = cv[m][below] * np.float32(255)
    assert np.array_equal(want[m][below], np.ceil(p).astype(np.uint8) - 1)


@pytest.mark.parametrize("h,w", cc.COUNT_SHAPES)
def test_count_canvases_crop_to_their_shape(orc, h, w):
    cv = orc.blend([cc.count_view(h, w)], cc.HOMO, 0, 0)[0]
    got, off = orc.crop(cv)
    assert got.shape == (h, w, 3) and off == (1, 0) and cc.crop_model(cc.canvas_mask(cv))[:4] == (1, 0, w, h)
    assert np.array_equal(orc.to_u8(got), cc.byte_model(got))


# ---- cylinder ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("h,w", cc.CYL_SHAPES)
def test_cylinder_cases(orc, h, w):
    for (_, _, hf, fl) in [c for c in cc.CYL_CASES if c[:2] == (h, w)]:
        cfg = cc.cyl_cfg(fl)
        out, _ = orc.cyl_warp(cc.cyl_image(h, w), hf, NOPTS, cfg)
        assert out.shape[0] > 0 and out.shape[1] > 0
        valid = out[..., 0] >= 0
        assert 0.4 <= valid.mean() <= 1, (hf, fl, valid.mean())
        assert (out[~valid] == -1).all()
        holes, _ = orc.cyl_warp(cc.cyl_holes(h, w), hf, NOPTS, cfg)
        lost = valid & (holes[..., 0] < 0)
        assert lost.any() and (holes[lost] == -1).all() and np.array_equal(holes[~lost], out[~lost]), (hf, fl)


def test_cylinder_empty_case(orc):
    h, w, hf, fl = cc.CYL_EMPTY
    out, _ = orc.cyl_warp(cc.cyl_image(h, w), hf, NOPTS, cc.cyl_cfg(fl))
    assert out.shape[1] == 0


def test_cache_pair_shares_a_width_and_nothing_else(orc):
    """two focal lengths at which a 67 x 130 image warps to the same output width with another radius, so another table"""
    from openpano_amd import hip
    h, w, hf, fa, fb = cc.CACHE_PAIR
    a, b = (hip.cyl_warp_shape(cc.cyl_cfg(f), w, h, hf) for f in (fa, fb))
    assert a[0] == b[0] > 0 and a[1] == b[1] and a[2][0] != b[2][0]
    ra, rb = (int(np.hypot(float(w), float(h)) * (np.float32(f) / 43.266)) for f in (fa, fb))
    assert ra != rb
    oa, ob = (orc.cyl_warp(cc.cyl_image(h, w), hf, NOPTS, cc.cyl_cfg(f))[0] for f in (fa, fb))
    assert oa.shape == ob.shape == (a[1], a[0], 3) and not np.array_equal(oa, ob)


# ---- against the reference compiled in place ---------------------------------------------------------------------------------

REF_CROP = cc.CROP_SMALL + [cc.WIDE_LDS]


@pytest.mark.parametrize("case", REF_CROP, ids=[c.id for c in REF_CROP])
def test_reference_crop_equals_oracle(ref, orc, canvases, case):
    cv = canvases[case.id]
    want = ref.crop(cv)
    got, _ = orc.crop(cv)
    assert want.shape == got.shape and np.array_equal(want, got)


@pytest.mark.parametrize("h,w", cc.CYL_SHAPES)
def test_reference_cyl_warp_equals_oracle(ref, orc, h, w):
    """every fp32 cylinder case, with and without holes, at the case's focal length (a global of the reference: put back)"""
    try:
        for (_, _, hf, fl) in [c for c in cc.CYL_CASES if c[:2] == (h, w)]:
            cfg = cc.cyl_cfg(fl)
            ref.set_config(**{k: v for k, v in cfg.raw_items()})
            for img in (cc.cyl_image(h, w), cc.cyl_holes(h, w)):
                want, _ = ref.cyl_warp(img, hf, NOPTS)
                got, _ = orc.cyl_warp(img, hf, NOPTS, cfg)
                assert want.shape == got.shape and np.array_equal(want, got), (hf, fl)
    finally:
        ref.set_config(**{k: v for k, v in PanoConfig().raw_items()})
