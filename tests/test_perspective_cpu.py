"""CPU: cylinder mode's perspective correction off the device -- the numpy restatement of the pass (perspective_cases.perspective_ref)
has the properties its cases claim; the host geometry (hip.perspective_homography -> op_perspective_homography, csrc/blend_geom.cc)
returns the reference's corners bit for bit and a homography that maps the canvas rectangle onto them; and the same geometry runs
as a program of its own under AddressSanitizer and UndefinedBehaviorSanitizer (tests/harness/perspective_harness.cc).  Nothing is
loaded into Python under a sanitizer and nothing is preloaded."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import perspective_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "openpano_amd", "csrc")
F = np.float32


def _case(h, w, content, homo):
    return next(c for c in pc.CASES if (c.h, c.w, c.content, c.homo) == (h, w, content, homo))


def _valid(out):
    return out[..., 0] >= 0


def _ulps(a, b):
    """distance in units of the last place between fp32 arrays of one sign"""
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def test_case_list_is_complete():
    assert len(pc.CASES) == len(pc.SHAPES) * len(pc.CONTENTS) * len(pc.HOMOS) == 105 and len({c.id for c in pc.CASES}) == 105
    assert sorted(pc.FLAGS) == [(0, 0), (0, 1), (1, 0), (1, 1)]


@pytest.mark.parametrize("h,w", pc.SHAPES)
def test_identity_no_pixels_and_interior(h, w):
    """column 0 has weight 0, the last row and the last column have no taps, row 0 has weight 0 unless ORDERED_INPUT; everything
    else is the source to within 1 ulp under both branches"""
    case = _case(h, w, "random", "identity")
    src = pc.canvas_of(case)
    for ordered, lazy in pc.FLAGS:
        out = pc.perspective_ref(src, pc.homography_of(case), ordered, lazy)
        want = np.ones((h, w), bool)
        want[:, 0] = False; want[:, -1] = False; want[-1] = False
        if not ordered:
            want[0] = False
        assert np.array_equal(_valid(out), want), (ordered, lazy)
        assert (out[~want] == -1).all()
        if want.any():
            assert _ulps(out[want], src[want]).max() <= 1, (ordered, lazy, _ulps(out[want], src[want]).max())
    if (h, w) == (1, 7):
        assert not want.any()                                   # no second row: every pixel NO


@pytest.mark.parametrize("h,w", pc.SHAPES)
def test_shift_no_pixels(h, w):
    """a shift by (0.37, 0.61): only the last row and the last column lose their taps; a Color::NO border or hole grows by the
    pixels whose 2 x 2 taps touch it"""
    for content in pc.CONTENTS:
        case = _case(h, w, content, "shift")
        src = pc.canvas_of(case)
        ok = src[..., 0] >= 0
        want = np.zeros((h, w), bool)
        want[:-1, :-1] = ok[:-1, :-1] & ok[1:, :-1] & ok[:-1, 1:] & ok[1:, 1:]
        for ordered, lazy in pc.FLAGS:
            out = pc.perspective_ref(src, pc.homography_of(case), ordered, lazy)
            assert np.array_equal(_valid(out), want), (content, ordered, lazy)
        if content == "random" and h > 2 and w > 2:
            i, j = h // 2, w // 2           # one pixel by hand, in fp64: the bilinear sample itself, whatever the weight
            fy, fx = pc.SHIFT[1], pc.SHIFT[0]
            s = src.astype(np.float64)
            by_hand = ((1 - fy) * (1 - fx) * s[i, j] + fy * (1 - fx) * s[i + 1, j] + fy * fx * s[i + 1, j + 1] + (1 - fy) * fx * s[i, j + 1])
            # the fp32 coordinates carry half an ulp of 256 (1.5e-5) per axis, colours differ by less than 1 between taps
            assert np.abs(out[i, j] - by_hand).max() < 5e-5


def test_the_two_branches_differ():
    """(float)(1.0 / w) * s is not s / w: the lazy cases test something"""
    case = _case(37, 53, "random", "identity")
    src, m = pc.canvas_of(case), pc.homography_of(case)
    for ordered in (0, 1):
        a, b = pc.perspective_ref(src, m, ordered, 0), pc.perspective_ref(src, m, ordered, 1)
        assert np.array_equal(_valid(a), _valid(b)) and not np.array_equal(a, b)
        assert _ulps(a[_valid(a)], b[_valid(a)]).max() <= 2


def test_cases_are_what_they_claim():
    for case in pc.CASES:
        x, y, z = pc.map_of(case)
        src = pc.canvas_of(case)
        out = pc.perspective_ref(src, pc.homography_of(case), 1, 0)
        big = case.h >= 5 and case.content == "random"
        if case.homo == "z0":
            assert (z == 0).any() and not np.isfinite(x[z == 0]).any() and not _valid(out)[z == 0].any()
            if case.w > 2:
                assert np.isinf(x[z == 0]).any()
            if case.h >= 2:
                assert np.isnan(x[z == 0]).any()
        elif case.homo == "zneg":
            assert (z < 0).any() and (z > 0).any() and not (z == 0).any()
            if big:
                assert _valid(out)[z < 0].any() and _valid(out)[z > 0].any()       # z < 0 still samples
        elif case.homo == "tiny":
            assert (y[0] == -1e-50).all() and (y[0].astype(F) == 0).all() and np.signbit(y[0].astype(F)).all()
            assert not _valid(out)[0].any()
            if big:             # a bounds test on the floats would have sampled row 0
                assert _valid(pc.perspective_ref(src, np.array([[1, 0, 0.5], [0, 1, 0], [0, 0, 1.0]]), 1, 0))[0].any()
        elif case.homo == "outside":
            assert (out == -1).all()
        elif case.homo == "mild" and big:
            assert _valid(out).mean() > 0.5 and (np.abs(z - 1) > 1e-3).any()
        if case.content == "border":
            assert not (src[..., 0] >= 0)[:2].any() and not (src[..., 0] >= 0)[:, -2:].any()
        if case.content == "hole":
            assert (src[..., 0] < 0).any()


# ---- the corner geometry -------------------------------------------------------------------------------------------------------

def _solve(b):
    from openpano_amd import hip
    return hip.perspective_homography(b.proj_min, b.ref_wh, b.first_wh, b.first_homo, b.last_wh, b.last_homo, b.canvas_wh)


@pytest.mark.parametrize("b", pc.BUNDLES, ids=[b.id for b in pc.BUNDLES])
def test_perspective_homography(b):
    """corners bit-equal to the fp64 restatement of to_ref_coor; inv maps corners_std onto them within 1e-6 px (the system is
    exactly determined and the Givens solve backward stable: about eps |A| |h| = 1e-8 px at 1e4-px coordinates)"""
    inv, corners = _solve(b)
    want = pc.bundle_corners(b)
    assert b.first_wh != b.ref_wh or b.id == "two_views"            # stale sizes differ from the reference view's
    assert np.array_equal(corners, want), (corners - want)
    assert inv[2, 2] == 1.0 and np.isfinite(inv).all()
    got = pc.apply_homography(inv, pc.corners_std(b.canvas_wh))
    assert np.abs(got - corners).max() < 1e-6, np.abs(got - corners).max()
    # the geometry is a sweep: left corners left of the right ones, and upper above lower for a view that stands upright
    assert corners[0, 0] < corners[2, 0] and corners[1, 0] < corners[3, 0] and corners[2, 1] < corners[3, 1]
    assert corners[0, 1] < corners[1, 1] or b.id == "five_views_first_rotated"


def test_first_view_rotated_swaps_its_sides():
    b = pc.BUNDLES[2]
    assert b.first_wh == (b.ref_wh[1], b.ref_wh[0])
    _, corners = _solve(b)
    # through a quarter turn the first view's (-0.5, -0.5) and (-0.5, 0.5) corners lie w apart in x, not h apart in y
    assert abs(abs(corners[1, 0] - corners[0, 0]) - b.first_wh[1]) < 0.06 * b.first_wh[1]


def test_collinear_corners_are_refused():
    from openpano_amd import hip
    want = pc.bundle_corners(pc.COLLINEAR)
    assert len(set(want[:, 1])) == 1
    with pytest.raises(hip.OpenPanoHipError, match=r"error -1: op_perspective_homography: three corners on one line"):
        _solve(pc.COLLINEAR)


def test_bad_arguments_are_refused():
    from openpano_amd import hip
    b = pc.BUNDLES[0]
    with pytest.raises(hip.OpenPanoHipError, match=r"error -1: op_perspective_homography: a size below 1"):
        _solve(b._replace(first_wh=(0, 400)))
    with pytest.raises(hip.OpenPanoHipError, match=r"error -1: op_perspective_homography: a size below 1"):
        _solve(b._replace(canvas_wh=(1033, 0)))
    with pytest.raises(hip.OpenPanoHipError, match=r"error -1: op_perspective_homography"):
        _solve(b._replace(last_homo=np.full((3, 3), np.nan)))


def test_sanitizer_program(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ missing")
    exe = str(tmp_path / "perspective_harness")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                           "-Wall", "-Wno-unknown-pragmas", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                           os.path.join(ROOT, "tests", "harness", "perspective_harness.cc"), os.path.join(CSRC, "blend_geom.cc"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    m = re.search(r"perspective_harness: (\d+) checks passed", r.stdout)
    assert m and int(m.group(1)) > 300, r.stdout[-1000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
