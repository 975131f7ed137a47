"""CPU: the scene table of tests/ransac_scenes.py does what it says, and the oracle agrees with the reference on it.

The GPU test (tests/test_gpu_match_ransac_config.py) compares op_ransac_pairs with the oracle on these scenes; what that
comparison covers -- which exits of fill_inliers_to_matchinfo, which winner positions, which configurations -- is asserted
here, without a GPU: every scene reaches the exit it names, the exits reached are all of them but SINGULAR (see the
table's docstring), winners lie past the first workgroup and the first chunk of draws.  Where oracle/_ref is built the
oracle is held to the reference's own TransformEstimation under every configuration of the table, and the exact matcher to
the reference's under other MATCH_REJECT_NEXT_RATIO values."""
import os

import numpy as np
import pytest

import ransac_scenes as rs
from checkers import RANSAC_EXITS
from openpano_amd.config import PanoConfig
from test_ransac_vs_ref import _same_inliers

HERE = os.path.dirname(os.path.abspath(__file__))
RATIOS = (0.0, 0.5, 0.95, 1.0, 1.25)


def _run(oracle, s, **cfg):
    return oracle.ransac(s.match, s.kp1, s.kp2, s.shape1, s.shape2, s.seed, cfg=rs.config_of(rs.key_of(s.mode, **dict(dict(s.key), **cfg))))


@pytest.fixture(scope="module")
def results(oracle):
    return {s.id: _run(oracle, s) for s in rs.SCENES}


def _find(name, mode, **cfg):
    key = rs.key_of(mode, **cfg)
    (s,) = [s for s in rs.SCENES if s.name == name and s.key == key]
    return s


def _hyp_count(oracle, s, samples, k):
    """inlier count of hypothesis k of the scene (-1: unhealthy), from the oracle itself: see ransac_scenes.moved_to_front"""
    r = oracle.ransac(rs.moved_to_front(s, samples, k), s.kp1, s.kp2, s.shape1, s.shape2, s.seed,
                      cfg=rs.config_of(rs.key_of(s.mode, **dict(dict(s.key), RANSAC_ITERATIONS=1))))
    return r["best_count"]


def _samples(s, count):
    return rs.mt19937_samples(s.seed, len(s.match), 7 if s.mode == "affine" else 8, count)


def test_every_scene_reaches_the_exit_it_names(results):
    wrong = [(s.id, s.exit, results[s.id]["exit"]) for s in rs.SCENES if results[s.id]["exit"] != s.exit]
    assert not wrong, wrong
    for mode in rs.MODES:
        reached = {s.exit for s in rs.SCENES if s.mode == mode}
        assert reached == set(RANSAC_EXITS) - {"SINGULAR"}, (mode, sorted(set(RANSAC_EXITS) - reached))
    # the gates of the second image are reached past the first image's, not instead of them
    for name in ("second_image_crowded", "outliers_outside_first_overlap"):
        assert all(s.exit in ("POINT_RATIO_2", "MATCH_RATIO_2") for s in rs.SCENES if s.name == name)


def test_every_iteration_count_runs_on_every_list_size():
    for mode in rs.MODES:
        for it in rs.ITERATIONS:
            names = {s.name for s in rs.SCENES if s.key == rs.key_of(mode, RANSAC_ITERATIONS=it)}
            assert {"m8", "m13", "m14", "m64", "m65", "m300"} <= names, (mode, it)
        for th in rs.THRESHOLDS:
            assert any(s.key == rs.key_of(mode, RANSAC_INLIER_THRES=th) for s in rs.SCENES)
    # unequal shapes, both orders of one pair of images (the arrays themselves are shared: one image, two roles)
    for a, b in (("large_small_zoom", "small_large_zoom"), ("landscape_portrait", "portrait_landscape")):
        x, y = _find(a, "homo"), _find(b, "homo")
        assert x.kp1 is y.kp2 and x.kp2 is y.kp1 and x.shape1 == y.shape2 != x.shape2 == y.shape1
        assert np.array_equal(x.match, y.match[:, ::-1])


@pytest.mark.parametrize("mode", sorted(rs.MODES))
def test_winners_lie_past_the_first_workgroup_and_the_first_chunk(results, mode):
    def winners(**cfg):
        return [results[s.id]["best_hyp"] for s in rs.SCENES if s.key == rs.key_of(mode, **cfg)]
    assert max(winners(RANSAC_ITERATIONS=65536)) > 4096, winners(RANSAC_ITERATIONS=65536)
    assert max(winners()) > 256, winners()


@pytest.mark.parametrize("mode", sorted(rs.MODES))
def test_the_first_of_equal_counts_wins(oracle, results, mode):
    """tie_m14: hypothesis 0 loses, and a hypothesis after the winner reaches the winner's count.  Per-hypothesis counts come
    from the oracle: the match list is reordered so that the draws of hypothesis 0 pick hypothesis k's sample."""
    s = _find("tie_m14", mode)
    r = results[s.id]
    w, c = r["best_hyp"], r["best_count"]
    samples = _samples(s, 64)
    assert w > 0 and _hyp_count(oracle, s, samples, w) == c                   # the reordering reproduces the winner's count
    assert all(_hyp_count(oracle, s, samples, k) < c for k in range(w))
    later = [k for k in range(w + 1, 64) if _hyp_count(oracle, s, samples, k) == c]
    assert later, "no later hypothesis ties the winner"


@pytest.mark.parametrize("mode", sorted(rs.MODES))
def test_threshold_and_single_hypothesis_scenes(oracle, results, mode):
    # RANSAC_INLIER_THRES = 0: nothing is an inlier, the first healthy hypothesis wins with a count of 0
    late = 0
    for s in rs.SCENES:
        if s.key != rs.key_of(mode, RANSAC_INLIER_THRES=0.0):
            continue
        r = results[s.id]
        assert r["best_count"] == 0 and r["best_hyp"] >= 0 and len(r["inliers"]) == 0, s.id
        samples = _samples(s, r["best_hyp"] + 1)
        assert [_hyp_count(oracle, s, samples, k) for k in range(r["best_hyp"] + 1)] == [-1] * r["best_hyp"] + [0], s.id
        late += r["best_hyp"] > 0
    assert late or mode == "affine"          # (an affine sample is healthy unless it mirrors: the first one wins everywhere)
    # RANSAC_INLIER_THRES = 20: 12.5 px against 4 px of noise
    s = _find("noisy_4px", mode, RANSAC_INLIER_THRES=20.0)
    assert len(results[s.id]["inliers"]) >= 0.95 * len(s.match)
    # the inlier distance follows the first image: the same pair in the other order keeps other matches
    a, b = results[_find("large_small_zoom", mode).id], results[_find("small_large_zoom", mode).id]
    assert a["best_count"] > 80 and b["best_count"] > 80
    # RANSAC_ITERATIONS = 1: the only hypothesis decides
    one = rs.key_of(mode, RANSAC_ITERATIONS=1)
    r = results[_find("clean_m100", mode, RANSAC_ITERATIONS=1).id]
    assert r["ok"] and r["best_hyp"] == 0
    r = results[_find("mirrored", mode, RANSAC_ITERATIONS=1).id]
    assert not r["ok"] and r["best_hyp"] == -1 and r["best_count"] == -1 and r["exit"] == "NO_HEALTHY"
    assert {results[s.id]["best_hyp"] for s in rs.SCENES if s.key == one} <= {0, -1}


@pytest.mark.parametrize("mode", sorted(rs.MODES))
def test_edge_values_are_the_oracles_own(results, mode):
    e = _find("edge", mode)
    r = results[e.id]
    assert np.float32(r["confidence"]) == np.float32(rs.EDGE[mode]["confidence"])
    # every matched point lies inside both overlap polygons, so both match ratios are inliers / m in float
    ratio = np.float32(len(r["inliers"])) / np.float32(len(e.match))
    assert ratio == np.float32(rs.EDGE[mode]["match_ratio"])
    at = [s for s in rs.SCENES if s.name == "edge" and s.mode == mode and s is not e]
    assert sorted(s.exit for s in at) == ["ACCEPTED", "ACCEPTED", "CONFIDENCE", "MATCH_RATIO_1"]
    for s in at:
        assert results[s.id]["best_hyp"] == r["best_hyp"] and np.array_equal(results[s.id]["inliers"], r["inliers"])


@pytest.mark.parametrize("key", sorted(rs.by_config()), ids=lambda k: ",".join("%s=%.9g" % kv for kv in k) or "default")
def test_oracle_equals_reference_under_config(ref, results, key):
    scenes = [s for s in rs.by_config()[key] if s.reference]
    ref.set_config(**dict(rs.config_of(key).raw_items()))
    try:
        got = [ref.ransac(s.match, s.kp1, s.kp2, s.shape1, s.shape2, s.seed) for s in scenes]
    finally:
        ref.set_config(**dict(PanoConfig().raw_items()))
    for s, r in zip(scenes, got):
        o = results[s.id]
        assert o["ok"] == r["ok"], (s.id, o["exit"])
        assert abs(o["confidence"] - r["confidence"]) < 1e-6, s.id
        if o["ok"]:
            assert np.allclose(o["homo"], r["homo"], rtol=1e-7, atol=1e-9), s.id
            assert _same_inliers(s.match, s.kp1, s.kp2, r["inlier_pts"], o["inliers"]), s.id


def _ratio_sets():
    a = np.load(os.path.join(HERE, "golden", "sift_a_240x320.npz"))["desc"]
    b = np.load(os.path.join(HERE, "golden", "sift_b_240x320.npz"))["desc"]
    dup = np.concatenate([a[:100], a[:100]])
    return a, b, ((a, b), (b, a), (a[:200], dup), (dup, a[:200]))


_REF_MATCH = """import sys, numpy as np
sys.path[:0] = [%r, %r]
from checkers import Ref
from openpano_amd.config import PanoConfig
from test_ransac_config_cpu import _ratio_sets
ref = Ref(PanoConfig(MATCH_REJECT_NEXT_RATIO=float(sys.argv[1])))
np.savez(sys.argv[2], *[ref.match_exact(x, y) for x, y in _ratio_sets()[2]])
"""


@pytest.mark.parametrize("ratio", RATIOS)
def test_exact_matcher_equals_reference_under_ratio(ref, tmp_path, ratio):
    """The reference squares the ratio into a function-local static on the first match of a process (matcher.cc:16), so every
    ratio is asked of a process of its own; this process's reference never matches at another ratio than the shipped one."""
    import subprocess
    import sys
    from checkers import Oracle
    out = str(tmp_path / "ref.npz")
    subprocess.run([sys.executable, "-c", _REF_MATCH % (os.path.dirname(HERE), HERE), repr(ratio), out], check=True, timeout=300)
    wants = np.load(out)
    orc = Oracle(PanoConfig(MATCH_REJECT_NEXT_RATIO=ratio))
    a, b, sets = _ratio_sets()
    for k, (x, y) in enumerate(sets):
        want = wants["arr_%d" % k]
        want = want[np.lexsort((want[:, 1], want[:, 0]))]
        got = orc.match_exact(x, y)
        assert np.array_equal(got, want), (ratio, k, len(got), len(want))
        assert (len(got) > 0) == (ratio > 0 or k >= 2)       # exact duplicates match at every ratio: 0 > 0 is false
    # more rows pass a looser ratio, and past 1.0 the near-ties do
    assert ratio < 1.0 or len(orc.match_exact(a, b)) > 2 * len(Oracle(PanoConfig()).match_exact(a, b))
