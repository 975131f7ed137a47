"""GPU: op_match_pairs and op_ransac_pairs off the shipped configuration, at every exit of the acceptance epilogue, with
images of unequal shape and descriptors of unequal magnitude -- every comparison with the oracle exact.

RANSAC: the scene table of tests/ransac_scenes.py, one op_ransac_pairs call per configuration (what the scenes reach is
asserted on the CPU: tests/test_ransac_config_cpu.py).  Matcher: MATCH_REJECT_NEXT_RATIO 0 .. 1.25 (from 1.0 on the rows
that pass are the near-ties, whose candidate set the ranking margin has to get complete), descriptors scaled by powers of
two (exact in fp32: the lists may not change), one call mixing magnitudes (the margin uses the call's largest norm), and
DESC_INT_FACTOR end to end."""
import os

import numpy as np
import pytest

import ransac_scenes as rs
from openpano_amd import synth
from openpano_amd.config import PanoConfig
from test_gpu_match import _edge_sets, _near_tie_sets

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
RATIOS = (0.0, 0.5, 0.95, 1.0, 1.25)
MARGIN = 8.2e-5                 # OP_MATCH_MARGIN (csrc/match.hip): E = MARGIN * (|x|^2 + the call's largest |y|^2), on scores -d / 2


@pytest.fixture(scope="module")
def ctx():
    from openpano_amd import hip
    c = hip.Context(0)
    yield c
    c.close()


def _id(key):
    return ",".join("%s=%.9g" % kv for kv in key) or "default"


# ---- RANSAC -----------------------------------------------------------------------------------------------------------------

def _job(scenes):
    """the scenes of one configuration as one job: images (an array shared by two scenes is one image), shapes, pairs"""
    index, coors, shapes, pairs = {}, [], [], []
    for s in scenes:
        ij = []
        for kp, shape in ((s.kp1, s.shape1), (s.kp2, s.shape2)):
            if id(kp) not in index:
                index[id(kp)] = len(coors); coors.append(kp); shapes.append(shape)
            assert shapes[index[id(kp)]] == shape
            ij.append(index[id(kp)])
        pairs.append(tuple(ij))
    return coors, shapes, pairs


def _compare(oracle, scenes, res):
    for s, r in zip(scenes, res):
        want = rs.check(oracle, r, s.match, s.kp1, s.kp2, s.shape1, s.shape2, s.seed, cfg=s.cfg)
        assert want["exit"] == s.exit, s.id


@pytest.mark.parametrize("key", sorted(rs.by_config()), ids=_id)
def test_ransac_equals_oracle_under_config(ctx, oracle, key):
    from openpano_amd import hip
    scenes = rs.by_config()[key]
    coors, shapes, pairs = _job(scenes)
    f = hip.Features.from_host(ctx, [np.zeros((len(c), 128), np.float32) for c in coors], coors)
    mh = hip.Matches.from_host([s.match for s in scenes])
    try:
        res = hip.ransac_pairs(ctx, rs.config_of(key), f, mh, pairs, shapes, seeds=[s.seed for s in scenes])
        _compare(oracle, scenes, res)
    finally:
        mh.free(); f.free()


@pytest.mark.parametrize("iters", [0, -3, 65537])
def test_iteration_counts_outside_the_range_are_refused(ctx, iters):
    from openpano_amd import hip
    s = rs.SCENES[0]
    f = hip.Features.from_host(ctx, [np.zeros((len(c), 128), np.float32) for c in (s.kp1, s.kp2)], [s.kp1, s.kp2])
    mh = hip.Matches.from_host([s.match])
    try:
        with pytest.raises(hip.OpenPanoHipError, match="RANSAC_ITERATIONS"):
            hip.ransac_pairs(ctx, PanoConfig(RANSAC_ITERATIONS=iters), f, mh, [(0, 1)], [s.shape1, s.shape2], seeds=[1])
        for ok in (1, 65536):                  # the bounds themselves are served (the scene table runs both)
            assert any(k == rs.key_of("homo", RANSAC_ITERATIONS=ok) for k in rs.by_config())
    finally:
        mh.free(); f.free()


@pytest.mark.parametrize("mode", sorted(rs.MODES))
def test_mixed_shapes_over_a_device_group(ctx, oracle, mode):
    """op_ransac_pairs_multi under RANSAC_ITERATIONS = 257 with the unequal-shape scenes in the job.  Host-made lists run on
    the group's first context; lists matched by the group itself are dealt over its contexts, the pairs, shapes and seeds
    following the deal: every keypoint gets a descriptor of its own, matched keypoints the same one, so the matcher returns
    the scenes' lists."""
    from openpano_amd import hip
    key = rs.key_of(mode, RANSAC_ITERATIONS=257)
    cfg = rs.config_of(key)
    scenes = rs.by_config()[key]
    assert len({s.shape1 for s in scenes} | {s.shape2 for s in scenes}) >= 4
    coors, shapes, pairs = _job(scenes)
    rng = np.random.default_rng(9)
    descs = [(rng.random((len(c), 128)) * 40).astype(np.float32) for c in coors]
    for s, (i, j) in zip(scenes, pairs):
        descs[j][s.match[:, 1]] = descs[i][s.match[:, 0]]
    seeds = [s.seed for s in scenes]
    grp = hip.Group([0, 0])
    f = hip.Features.from_host(ctx, descs, coors)
    fg = hip.Features.from_host(grp.ctx0, descs, coors)
    mh = hip.Matches.from_host([s.match for s in scenes])
    mg = grp.match_pairs_handle(cfg, fg, pairs)
    try:
        for s, got in zip(scenes, mg.lists()):
            assert np.array_equal(got, s.match[np.lexsort((s.match[:, 1], s.match[:, 0]))]), s.id
            assert np.array_equal(s.match, s.match[np.lexsort((s.match[:, 1], s.match[:, 0]))]), s.id
        single = hip.ransac_pairs(ctx, cfg, f, mh, pairs, shapes, seeds=seeds)
        _compare(oracle, scenes, single)
        for handle in (mh, mg):
            multi = grp.ransac_pairs(cfg, fg, handle, pairs, shapes, seeds=seeds)
            for s, a, b in zip(scenes, single, multi):
                assert (a["ok"], a["best_hyp"], a["best_count"], a["confidence"]) == (b["ok"], b["best_hyp"], b["best_count"], b["confidence"]), s.id
                assert np.array_equal(a["inliers"], b["inliers"]) and np.array_equal(a["homo"], b["homo"]), s.id
    finally:
        mg.free(); mh.free(); fg.free(); f.free(); grp.close()


# ---- matcher: ratio -----------------------------------------------------------------------------------------------------------

def _dense_near_ties():
    """64 rows, each with three near-copies (|delta d^2| < 1 on |x|^2 = 512^2) in columns of its own: under a ratio of 1.0
    or more every row is accepted on a best and a second best far inside the margin"""
    rng = np.random.default_rng(5)
    a = np.load(os.path.join(HERE, "golden", "sift_d_500x700.npz"))["desc"]
    x = a[:64].copy(); y = a[200:200 + 192].copy()
    for r in range(64):
        for k in range(3):
            c = 3 * r + k
            y[c] = x[r]
            j = rng.choice(128, 3, replace=False)
            y[c, j] = np.maximum(y[c, j] + rng.choice([-0.25, 0.25, 0.5], 3).astype(np.float32), 0)
    return x, y


def _inside_margin(x, y, rows, gmax):
    """of the given rows of x: how many have their two smallest distances to y closer than the re-score margin"""
    x64, y64 = x.astype(np.float64), y.astype(np.float64)
    d = np.sort(((x64[rows, None, :] - y64[None, :, :]) ** 2).sum(2), 1)
    return int(((d[:, 1] - d[:, 0]) / 2 < MARGIN * ((x64[rows] ** 2).sum(1) + gmax)).sum())


@pytest.fixture(scope="module")
def sift5(ctx, cfg):
    from openpano_amd import hip
    f = hip.sift_batch(ctx, cfg, synth.image_set(5, 400, 600, seed=22, overlap=0.45))
    descs = [f.get(i)[0] for i in range(5)]
    yield f, descs
    f.free()


def _oracle_at(**kv):
    from checkers import Oracle
    return Oracle(PanoConfig(**kv))


@pytest.mark.parametrize("ratio", RATIOS)
def test_match_ratio_edge_sets(ctx, ratio):
    from openpano_amd import hip
    c, orc = PanoConfig(MATCH_REJECT_NEXT_RATIO=ratio), _oracle_at(MATCH_REJECT_NEXT_RATIO=ratio)
    sets = _edge_sets()
    f = hip.Features.from_host(ctx, sets)
    pairs = [(i, j) for i in range(len(sets)) for j in range(len(sets)) if i != j] + [(4, 4)]
    got = hip.match_pairs(ctx, c, f, pairs)
    f.free()
    total = 0
    for (i, j), g in zip(pairs, got):
        want = orc.match_exact(sets[i], sets[j])
        assert np.array_equal(g, want), (ratio, i, j, len(g), len(want))
        total += len(want)
    assert total > 0                           # exact duplicates (sets 4 / 5 / 9 / 10) match at every ratio, 0 included


@pytest.mark.parametrize("ratio", RATIOS)
def test_match_ratio_near_ties(ctx, ratio):
    from openpano_amd import hip
    c, orc = PanoConfig(MATCH_REJECT_NEXT_RATIO=ratio), _oracle_at(MATCH_REJECT_NEXT_RATIO=ratio)
    x, y = _near_tie_sets()
    p, q = _dense_near_ties()
    sets = [x, y, y[:40], x[:5], p, q]
    pairs = [(0, 1), (1, 0), (2, 0), (0, 2), (3, 1), (1, 3), (4, 5), (5, 4)]
    f = hip.Features.from_host(ctx, sets)
    got = hip.match_pairs(ctx, c, f, pairs)
    f.free()
    want = [orc.match_exact(sets[i], sets[j]) for i, j in pairs]
    if ratio >= 1.0:
        # what the oracle accepts here are rows whose best and second best the MFMA ranking cannot tell apart
        gmax = max(float((s.astype(np.float64) ** 2).sum(1).max()) for s in sets)
        assert len(want[6]) == 64 and _inside_margin(p, q, want[6][:, 0], gmax) == 64
        assert _inside_margin(x, y, want[0][:, 0], gmax) >= 10
    for (i, j), g, w in zip(pairs, got, want):
        assert np.array_equal(g, w), (ratio, i, j, len(g), len(w))


@pytest.mark.parametrize("ratio", RATIOS)
def test_match_ratio_all_pairs_of_a_sift_job(ctx, sift5, ratio):
    from openpano_amd import hip
    f, descs = sift5
    c, orc = PanoConfig(MATCH_REJECT_NEXT_RATIO=ratio), _oracle_at(MATCH_REJECT_NEXT_RATIO=ratio)
    pairs = [(i, j) for i in range(5) for j in range(i + 1, 5)]
    got = hip.match_pairs(ctx, c, f, pairs)
    n = 0
    for (i, j), g in zip(pairs, got):
        want = orc.match_exact(descs[i], descs[j])
        assert np.array_equal(g, want), (ratio, i, j, len(g), len(want))
        n += len(want)
    assert (n > 100) == (ratio > 0)


# ---- matcher: magnitude ------------------------------------------------------------------------------------------------------

def _golden_pair():
    return (np.load(os.path.join(HERE, "golden", "sift_a_240x320.npz"))["desc"], np.load(os.path.join(HERE, "golden", "sift_b_240x320.npz"))["desc"])


@pytest.fixture(scope="module")
def unscaled(oracle):
    a, b = _golden_pair()
    x, y = _near_tie_sets()
    sets = [a, b, x, y]
    pairs = [(0, 1), (1, 0), (2, 3), (3, 2)]
    return sets, pairs, [oracle.match_exact(sets[i], sets[j]) for i, j in pairs]


@pytest.mark.parametrize("log2", [-10, -3, 3, 10])
def test_power_of_two_scaling_changes_no_list(ctx, oracle, cfg, unscaled, log2):
    """every product, difference and sum of the exact distance scales by 4^log2 without rounding, both sides of the ratio
    test with it: the oracle's lists on the scaled sets are the unscaled ones, and so must the device's be"""
    from openpano_amd import hip
    sets, pairs, base = unscaled
    scaled = [(s * np.float32(2.0 ** log2)).astype(np.float32) for s in sets]
    f = hip.Features.from_host(ctx, scaled)
    got = hip.match_pairs(ctx, cfg, f, pairs)
    f.free()
    assert sum(len(w) for w in base) > 60
    for (i, j), g, w in zip(pairs, got, base):
        assert np.array_equal(oracle.match_exact(scaled[i], scaled[j]), w), (log2, i, j)
        assert np.array_equal(g, w), (log2, i, j, len(g), len(w))


def _tight_ties(rows=256, scale=2.0 ** -8):
    """rows of norm 2 against columns of norm 512: every row (a descriptor scaled down by 256) has three columns that are the
    unscaled descriptor with two elements moved along the sphere -- equal norms, true scores x.y - |y|^2 / 2 within 0.01 of each
    other, where the ranking keys of such columns are only good to a few tenths (their error goes with |y|^2, and their low
    bits carry the slot).  The margin E = 8.2e-5 (|x|^2 + the call's largest |y|^2) = 21 keeps all three as candidates;
    8.2e-5 * 2 |x|^2 = 7e-4 would keep only those whose keys happen to coincide
    (tests/test_matcher_margin_model.py::test_a_margin_from_the_rows_own_norm_loses_candidates)."""
    rng = np.random.default_rng(11)
    a = np.load(os.path.join(HERE, "golden", "sift_d_500x700.npz"))["desc"]
    base = a[:rows]
    x = (base * np.float32(scale)).astype(np.float32)
    y = a[400:400 + 3 * rows].copy()
    for r in range(rows):
        big = np.flatnonzero(base[r] > 8)
        for k in range(3):
            v = base[r].copy()
            if k:
                j1, j2 = rng.choice(big, 2, replace=False)
                d = np.float32(0.125 * k)
                v[j1] += d
                v[j2] = np.float32(np.sqrt(max(float(v[j2]) ** 2 - (2 * float(base[r][j1]) * float(d) + float(d) ** 2), 0.0)))
            y[3 * r + k] = v
    return x, y


@pytest.mark.parametrize("ratio", [0.8, 1.0, 1.25])
def test_one_call_mixing_magnitudes(ctx, ratio):
    """the largest norm of the call widens every pair's margin: with one set 16 times larger, rows of the other pairs
    fall back to the exact scan -- their lists stay the oracle's.  And the margin of a small-norm row against large-norm
    columns has to come from the columns' norm: the rows of _tight_ties are accepted (from a ratio of 1.0 on) on the exact
    best of three columns the keys cannot order."""
    from openpano_amd import hip
    c, orc = PanoConfig(MATCH_REJECT_NEXT_RATIO=ratio), _oracle_at(MATCH_REJECT_NEXT_RATIO=ratio)
    a, b = _golden_pair()
    x, y = _near_tie_sets()
    p, q = _tight_ties()
    sets = [a, a * np.float32(16), b * np.float32(2.0 ** -6), x, y, p, q]
    f = hip.Features.from_host(ctx, sets)
    pairs = [(i, j) for i in range(len(sets)) for j in range(len(sets)) if i != j]
    got = hip.match_pairs(ctx, c, f, pairs)
    f.free()
    for (i, j), g in zip(pairs, got):
        want = orc.match_exact(sets[i], sets[j])
        assert np.array_equal(g, want), (ratio, i, j, len(g), len(want))
    assert len(orc.match_exact(x, y)) > 10
    if ratio >= 1.0:
        w = orc.match_exact(p, q)
        assert len(w) >= 0.9 * len(p) and np.all(w[:, 1] // 3 == w[:, 0])


@pytest.mark.parametrize("factor", [64, 4096])
def test_desc_int_factor_end_to_end(ctx, factor):
    from openpano_amd import hip
    c, orc = PanoConfig(DESC_INT_FACTOR=factor), _oracle_at(DESC_INT_FACTOR=factor)
    views = synth.image_set(3, 240, 320, seed=5, overlap=0.5)
    f = hip.sift_batch(ctx, c, views)
    pairs = [(0, 1), (1, 2), (0, 2), (2, 0)]
    got = hip.match_pairs(ctx, c, f, pairs)
    descs = []
    for k, v in enumerate(views):
        od, oc = orc.detect_feature(v)
        d, co = f.get(k)
        assert len(d) > 50 and np.array_equal(d, od) and np.array_equal(co, oc), (factor, k)
        descs.append(od)
    f.free()
    for (i, j), g in zip(pairs, got):
        want = orc.match_exact(descs[i], descs[j])
        assert np.array_equal(g, want), (factor, i, j, len(g), len(want))
    assert len(got[0]) > 10
