"""CPU: the inputs of tests/keypoint_cases.py.  (a) The oracle's branch census shows that every case reaches the branches it is
here for -- and that the suite's older SIFT inputs do not; (b) the C oracle equals the reference compiled in place on every
case, stage by stage; (c) five one-line slips compiled into a copy of the oracle change the named case and are invisible
on the old input."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import keypoint_cases as kc
import sift_cases as sc
from openpano_amd.config import PanoConfig

OFF_DIAGONAL = ("pivot1_01", "pivot1_02", "pivot1_10", "pivot1_12", "pivot1_20", "pivot1_21")


@pytest.fixture(scope="module")
def runs():
    """name -> the oracle's stages of the case (lists and census, no planes), computed once and left unchanged"""
    from checkers import Oracle
    out = {}
    for name in kc.NAMES:
        img, cfg = kc.case(name)
        out[name] = Oracle(cfg).sift_stages(img, planes=False)
    return out


def _peaks_per_keypoint(st):
    """number of oriented keypoints per refined keypoint (oriented is the expansion of refined, in order)"""
    c = st.census
    return [c["ori_peaks_%s" % k] for k in ("0", "1", "2", "3", "4", "5plus")]


# ---- (a) preconditions: floors well under the measured counts, so that another seed does not break them while an
# input that lost its purpose does

def test_case_n_reaches_the_pivot_move_and_tie_branches(runs):
    for name in ("N", "N6"):
        st = runs[name]; c = st.census
        assert c["pivot1_01"] >= 1 and c["pivot1_02"] >= 1 and c["pivot1_12"] >= 1, name
        assert c["pivot2_12"] >= 5 and c["pivot2_21"] >= 5, name
        assert min(c["accepted_1"], c["accepted_2"], c["accepted_3"]) >= 30, name
        assert c["depth_exhausted"] >= 100 and c["scale_moves"] >= 100 and c["oob_moved_scale"] >= 20 and c["det_reject"] >= 20, name
        rows = np.concatenate([st.refined["ints"].astype(np.float64), st.refined["real"]], axis=1)
        assert len(np.unique(rows, axis=0)) < len(rows), name                # a pair of identical refined keypoints
        assert c["equal_cmp"] >= 1 and len(st.desc) > 5000, name
    assert runs["N6"].dims[0] == (kc.H, kc.W) and len(runs["N6"].raw) == 3 * 4          # NUM_SCALE = 6: three scanned layers


def test_case_s_reaches_the_pseudo_inverse_on_trajectories_that_survive(runs):
    for name, floor in (("S", 500), ("S241", 5000)):
        c = runs[name].census
        assert c["pinv_calls"] >= floor and c["lu_rank_2"] == c["pinv_calls"], name
        assert c["accepted_1"] + c["accepted_2"] + c["accepted_3"] >= 30, name
        assert len(runs[name].desc) > 500, name
    assert runs["S"].dims[0] == (121, 241)


def test_case_s0_is_all_candidates_and_no_keypoint(runs):
    st = runs["S0"]; c = st.census
    assert c["pinv_calls"] >= 5000 and len(st.desc) == 0 and len(st.refined["ints"]) == 0
    assert sum(len(v) for v in st.raw.values()) > 20000
    # more than 192 raw extrema in a 240 x 24 segment of octave 0: the shipped k_pyramid_rows leaves its LDS list for the
    # image's list (csrc/pyramid.hip), which test_gpu_sift.py reaches only through a variant build
    assert kc.segment_counts(st).max() > 192


def test_case_o_has_keypoints_without_a_peak(runs):
    st = runs["O"]; n = len(st.refined["ints"])
    peaks = _peaks_per_keypoint(st)
    assert sum(peaks) == n and n > 1000
    assert peaks[0] >= 0.9 * n and sum(peaks[1:]) >= 1
    assert len(st.desc) == sum(k * v for k, v in enumerate(peaks[:5])) and peaks[5] == 0
    assert len(runs["O6"].desc) > 1000


def test_case_z_has_only_nan_descriptors(runs):
    st = runs["Z"]
    assert len(st.desc) >= 1 and np.isnan(st.desc).all()
    assert st.census["desc_sum_le0"] == len(st.desc)
    assert not np.isnan(st.coor).any()


def test_case_h_wraps_the_histogram_bin(runs):
    assert runs["H"].census["desc_histbin_ge8"] >= 1


def test_old_inputs_reach_none_of_it():
    """the gap itself: the suite's everyday inputs never pivot off the diagonal, never call the pseudo-inverse and never move
    in scale -- a later change to them that does is noticed here"""
    from checkers import Oracle
    for img, cfg in ((kc.old_view(), PanoConfig()), (sc.dense(kc.H, kc.W, 1), sc.cfg_for(kc.H, kc.W))):
        c = Oracle(cfg).sift_stages(img, planes=False).census
        assert sum(c[k] for k in OFF_DIAGONAL) == 0 and c["pinv_calls"] == 0 and c["scale_moves"] == 0


def test_census_is_per_run_and_complete():
    """the counters belong to the run: two runs of one input report the same counts, and they add up"""
    from checkers import Oracle, CENSUS_NAMES
    img, cfg = kc.case("S")
    o = Oracle(cfg)
    a, b = o.sift_stages(img, planes=False), o.sift_stages(img, planes=False)
    assert a.census == b.census and list(a.census) == list(CENSUS_NAMES)
    c = a.census
    raw = sum(len(v) for v in a.raw.values())
    ended = sum(c["accepted_%d" % k] for k in range(8)) + c["depth_exhausted"] + c["oob_first"] + c["oob_moved"]
    assert ended == raw
    kept = sum(c["accepted_%d" % k] for k in range(8)) - c["contrast_reject"] - c["det_reject"] - c["edge_reject"]
    assert kept == len(a.refined["ints"])
    assert sum(c["pivot1_%d%d" % (r, k)] for r in range(3) for k in range(3)) >= sum(c["pivot2_%d%d" % (r, k)] for r in (1, 2) for k in (1, 2))


# ---- (b) the oracle equals the reference

@pytest.mark.parametrize("name", kc.NAMES)
def test_oracle_equals_reference_on_keypoint_cases(name):
    """Stage by stage, NaN descriptor elements by position.  The reference's pseudo_inverse is compiled against the project's
    own mini-Eigen stand-in (oracle/ref_shim), so on the rank-deficient Hessians of S, S0 and S241 this holds the oracle to
    that stand-in's JacobiSVD, not to Eigen's."""
    from checkers import Oracle, Ref, ref_available
    if not ref_available():
        pytest.skip("oracle/_ref not built (reference sources absent)")
    img, cfg = kc.case(name)
    ref = Ref(cfg)
    try:
        so = Oracle(cfg).sift_stages(img)
        sr = ref.sift_stages(img)
    finally:
        ref.set_config(**{k: v for k, v in PanoConfig().raw_items()})
    kc.compare_oracle_ref(so, sr)


# ---- (c) sensitivity

SLIPS = {1: ("N", "the column swap is skipped when the pivot is off the diagonal"),
         2: ("N", "a move leaves nows alone"),
         3: ("N", "a move truncates instead of round()"),
         4: ("O", "a keypoint without a peak emits the orientation 0"),
         5: ("N", "identical refined keypoints are merged")}


class _SiftOnly:
    """oracle/sift_oracle.c alone, compiled with extra flags: the staged interface of checkers.Oracle"""

    def __init__(self, so, cfg):
        from checkers import OrcCfg, _StagedBase

        class _B(_StagedBase):
            prefix = "orc_"
        self._b = _B()
        self.lib = C.CDLL(so)
        self._b._bind_staged(self.lib, with_cfg=True)
        self.cfg, self.ccfg = cfg, OrcCfg.from_config(cfg)

    def sift_stages(self, img):
        img = np.ascontiguousarray(img, np.float32)
        hd = self.lib.orc_sift_new(C.byref(self.ccfg), img.reshape(-1), img.shape[0], img.shape[1])
        try:
            return self._b._collect(self.lib, hd, self.cfg, planes=False)
        finally:
            self.lib.orc_sift_free(hd)


@pytest.fixture(scope="module")
def slipped(tmp_path_factory):
    """k -> path of sift_oracle.c compiled with -DORC_SLIP=k (0: none) under the flags of oracle/Makefile"""
    from checkers import ORACLE_DIR
    out = tmp_path_factory.mktemp("slips")
    jobs = {}
    for k in [0] + sorted(SLIPS):
        so = str(out / ("libsift_slip%d.so" % k))
        jobs[so] = subprocess.Popen([os.environ.get("CC", "gcc"), "-std=gnu11", "-O3", "-march=x86-64-v3", "-ffp-contract=off", "-fPIC", "-fopenmp",
                                     "-shared", "-DORC_SLIP=%d" % k, "-I" + ORACLE_DIR, "-o", so, os.path.join(ORACLE_DIR, "sift_oracle.c"), "-lm"])
    assert all(j.wait() == 0 for j in jobs.values())
    return dict(zip([0] + sorted(SLIPS), jobs))


def _lists_equal(a, b):
    if len(a.desc) != len(b.desc) or len(a.refined["ints"]) != len(b.refined["ints"]):
        return False
    return (all(kc.same(getattr(a, nm)[f], getattr(b, nm)[f]) for nm in ("refined", "oriented") for f in ("ints", "real", "fl"))
            and kc.same(a.desc, b.desc) and kc.same(a.coor, b.coor))


@pytest.mark.parametrize("k", sorted(SLIPS), ids=["slip%d" % k for k in sorted(SLIPS)])
def test_slip_changes_its_case_and_not_the_old_input(slipped, k):
    name = SLIPS[k][0]
    img, cfg = kc.case(name)
    good, bad = _SiftOnly(slipped[0], cfg).sift_stages(img), _SiftOnly(slipped[k], cfg).sift_stages(img)
    assert not (kc.same(good.desc, bad.desc) and kc.same(good.coor, bad.coor)), SLIPS[k][1]
    old, dflt = kc.old_view(), PanoConfig()
    good, bad = _SiftOnly(slipped[0], dflt).sift_stages(old), _SiftOnly(slipped[k], dflt).sift_stages(old)
    assert len(good.desc) > 500 and _lists_equal(good, bad), SLIPS[k][1]


def test_unslipped_copy_is_the_oracle(slipped, runs):
    """the copy built for the slips with ORC_SLIP=0 computes what liboracle.so computes"""
    for name in ("N", "O"):
        img, cfg = kc.case(name)
        assert _lists_equal(_SiftOnly(slipped[0], cfg).sift_stages(img), runs[name]), name
