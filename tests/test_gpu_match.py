"""GPU parity tests of the MFMA matcher (C-ABI op_match_pairs) against the exact-matcher oracle
(FeatureMatcher::match restated, oracle/match_oracle.c).  Match sets must be IDENTICAL."""
import os

import numpy as np
import pytest

from openpano_amd import synth

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def ctx():
    from openpano_amd import hip
    c = hip.Context(0)
    yield c
    c.close()


def test_match_golden(ctx, cfg):
    from openpano_amd import hip
    a = np.load(os.path.join(HERE, "golden", "sift_a_240x320.npz"))["desc"]
    b = np.load(os.path.join(HERE, "golden", "sift_b_240x320.npz"))["desc"]
    want = np.load(os.path.join(HERE, "golden", "match_ab.npz"))["pairs"]
    f = hip.Features.from_host(ctx, [a, b])
    got = hip.match_pairs(ctx, cfg, f, [(0, 1), (1, 0)])
    assert np.array_equal(got[0], want)
    assert sorted(map(tuple, got[1][:, ::-1])) == sorted(map(tuple, want))
    f.free()


def test_all_pairs_on_sift_features(ctx, oracle, cfg):
    """SIFT on device -> all-pairs match on device == oracle exact matcher on the same descriptors"""
    from openpano_amd import hip
    views = synth.image_set(5, 400, 600, seed=22, overlap=0.45)
    f = hip.sift_batch(ctx, cfg, views)
    descs = [f.get(i)[0] for i in range(5)]
    pairs = [(i, j) for i in range(5) for j in range(i + 1, 5)]
    got = hip.match_pairs(ctx, cfg, f, pairs)
    nmatch = 0
    for (i, j), g in zip(pairs, got):
        want = oracle.match_exact(descs[i], descs[j])
        assert np.array_equal(g, want), (i, j, len(g), len(want))
        nmatch += len(want)
    assert nmatch > 100
    f.free()


def _edge_sets():
    """the descriptor sets of test_edge_cases (also matched under other ratios: test_gpu_match_ransac_config.py)"""
    rng = np.random.default_rng(1)
    a = np.load(os.path.join(HERE, "golden", "sift_a_240x320.npz"))["desc"]
    sets = [
        a[:0],                      # 0: empty
        a[:1],                      # 1: single descriptor
        a[:3],                      # 2: fewer than the top-4 buffer
        a[:129],                    # 3: one row past a 128-row block
        a[:200].copy(),             # 4
        np.concatenate([a[:100], a[:100]]),        # 5: exact duplicates -> ties, nothing distinctive
        (rng.random((300, 128)) * 40).astype(np.float32),   # 6: un-normalised random vectors
        (a[:200] + rng.normal(0, 3.0, (200, 128)).astype(np.float32)).clip(0).astype(np.float32),  # 7: noisy copy of 4
        np.zeros((5, 128), np.float32),             # 8: all-zero descriptors
        # 9/10: more than 8 identical descriptors: every ranked candidate falls inside the error
        # margin, so the rows take the exact full-scan path (forward and reverse)
        np.concatenate([np.repeat(a[5:6], 12, axis=0), a[:60], np.repeat(a[70:71], 9, axis=0)]),
        np.concatenate([a[:40], np.repeat(a[5:6], 11, axis=0), a[60:90]]),
        # 11: a NaN descriptor (zero-weight window) never matches and never wins a ratio test
        np.concatenate([a[:30], np.full((1, 128), np.nan, np.float32), a[30:50]]),
    ]
    return sets


def test_edge_cases(ctx, oracle, cfg):
    from openpano_amd import hip
    sets = _edge_sets()
    f = hip.Features.from_host(ctx, sets)
    pairs = [(i, j) for i in range(len(sets)) for j in range(len(sets)) if i != j]
    got = hip.match_pairs(ctx, cfg, f, pairs)
    for (i, j), g in zip(pairs, got):
        want = oracle.match_exact(sets[i], sets[j])
        assert np.array_equal(g, want), (i, j, g.tolist()[:5], want.tolist()[:5])
    # a set against itself: every descriptor matches itself when all are distinct
    g = hip.match_pairs(ctx, cfg, f, [(4, 4)])[0]
    assert np.array_equal(g, oracle.match_exact(sets[4], sets[4]))
    f.free()


def _near_tie_sets():
    """x, y of test_near_ties_across_tiles_and_lane_halves: near-copies of x's rows planted at chosen columns of y"""
    rng = np.random.default_rng(77)
    a = np.load(os.path.join(HERE, "golden", "sift_d_500x700.npz"))["desc"]
    x = a[:96].copy()
    ky = 32 * 9
    y = a[200:200 + ky].copy()
    plans = [
        [0, 1],                      # two copies, same tile, same half
        [0, 4],                      # same tile, the two halves
        [3, 32 + 3, 64 + 3],         # three tiles, same slot, same half
        [2, 6, 32 + 9, 64 + 13],     # two per half
        [1, 2, 3, 5, 6, 7],          # 3 + 3 in one tile
        [0, 1, 2, 3],                # four in one half: overflow -> exact scan
        [8, 40, 72, 104, 136, 168],  # six tiles, one half
        [31, 63, 95, 287],           # last slots, last tile
    ]
    for r in range(len(x)):
        cols = [(c + 32 * (r % 3)) % ky for c in plans[r % len(plans)]]
        for k, c in enumerate(cols):
            y[c] = x[r]
            if k > 0 or r % 2:       # exact duplicate for even rows' first copy, otherwise a near-copy
                j = rng.integers(0, 128, 3)
                y[c, j] = np.maximum(y[c, j] + rng.choice([-0.25, 0.25, 0.5], 3).astype(np.float32), 0)
    return x, y


def test_near_ties_across_tiles_and_lane_halves(ctx, oracle, cfg):
    """The sweep keeps a top-4 of KEYS per lane half (column & 4 of every 32-column tile selects the half) and
    re-scores every kept entry within the error margin of the row's 2nd best.  Near-copies of a row (inside the
    margin: |delta d^2| of a few units on |x|^2 = 512^2) are planted at chosen columns -- same tile / different
    tiles, same half / both halves, 2 to 6 copies (up to 3 + 3 candidates; 4 in one half = exact full scan) --
    and the match sets must equal the exact matcher's, forward and reverse."""
    from openpano_amd import hip
    x, y = _near_tie_sets()
    f = hip.Features.from_host(ctx, [x, y, y[:40], x[:5]])
    pairs = [(0, 1), (1, 0), (2, 0), (0, 2), (3, 1), (1, 3)]
    sets = [x, y, y[:40], x[:5]]
    got = hip.match_pairs(ctx, cfg, f, pairs)
    for (i, j), g in zip(pairs, got):
        want = oracle.match_exact(sets[i], sets[j])
        assert np.array_equal(g, want), (i, j, len(g), len(want))
    f.free()


def test_reverse_exact_scan_uses_the_minimum(ctx, oracle, cfg):
    """The second ratio test compares the match's distance with the MINIMUM reverse distance over kk != k
    (matcher.cc:57-61).  A row whose reverse pass takes the exact full scan (four near-ties in one lane half) and
    whose smallest and second-smallest reverse distances straddle the ratio threshold: rounds 1-2 passed the
    second-smallest there and accepted one match in 740 k too many on the config-5 job (pair (2, 94))."""
    from openpano_amd import hip
    a_all = np.load(os.path.join(HERE, "golden", "sift_d_500x700.npz"))["desc"]
    A = a_all[:60].copy(); B = a_all[100:180].copy()
    v = a_all[300].copy()
    bstar = v.copy(); bstar[5] += np.float32(np.sqrt(40.0))             # d2(a, b*) = 40
    A[16] = v; B[33] = bstar
    for k, (row, m) in enumerate([(0, 50.0), (1, 70.0), (2, 72.0), (3, 74.0), (8, 76.0)]):   # near-copies of b* in lane half 0
        A[row] = bstar; A[row][20 + k] += np.float32(np.sqrt(m))
    sets = [A, B]
    f = hip.Features.from_host(ctx, sets)
    for (i, j) in [(0, 1), (1, 0)]:
        got = hip.match_pairs(ctx, cfg, f, [(i, j)])[0]
        want = oracle.match_exact(sets[i], sets[j])
        assert np.array_equal(got, want), (i, j, got.tolist(), want.tolist())
    # the construction does what it says: 0.64 * 50 < 40 <= 0.64 * 70, so row 16 must be rejected
    assert not any(g[0] == 16 and g[1] == 33 for g in hip.match_pairs(ctx, cfg, f, [(0, 1)])[0])
    f.free()


def test_full_size_properties(ctx, oracle, cfg):
    """config-4 sized descriptor sets: symmetry + spot oracle checks"""
    from openpano_amd import hip
    views = synth.image_set(6, 867, 1300, seed=38, overlap=0.45, rows=2)
    f = hip.sift_batch(ctx, cfg, views)
    pairs = [(i, j) for i in range(6) for j in range(6) if i != j]
    got = dict(zip(pairs, hip.match_pairs(ctx, cfg, f, pairs)))
    for i in range(6):
        for j in range(i + 1, 6):
            # match(i,j) and match(j,i) are the same set with swapped columns
            assert sorted(map(tuple, got[(i, j)])) == sorted(map(tuple, got[(j, i)][:, ::-1]))
            # one-to-one: an index appears at most once on either side
            if len(got[(i, j)]):
                assert len(set(got[(i, j)][:, 0])) == len(got[(i, j)]) == len(set(got[(i, j)][:, 1]))
    for (i, j) in [(0, 1), (2, 5), (4, 3)]:
        want = oracle.match_exact(f.get(i)[0], f.get(j)[0])
        assert np.array_equal(got[(i, j)], want)
    f.free()


def test_config5_sized_sets(ctx, oracle, cfg):
    """BASELINE config 5 scale for the matcher: K ~ 4000 descriptors per image (the MFMA
    match-matrix stress).  Properties over all pairs of 6 sets + exact oracle check of two pairs."""
    from openpano_amd import hip
    rng = np.random.default_rng(5)
    a = np.load(os.path.join(HERE, "golden", "sift_d_500x700.npz"))["desc"]
    base = np.concatenate([a] * (4000 // len(a) + 1))[:4000]
    sets = []
    for k in range(6):
        # RootSIFT-like rows: a noisy, shuffled copy of a common base so that true matches exist
        x = np.abs(base + rng.normal(0, 6.0 + 2 * k, base.shape)).astype(np.float32)
        x = (np.sqrt(x / x.sum(axis=1, keepdims=True)) * 512).astype(np.float32)
        sets.append(x[rng.permutation(len(x))[: 3600 + 80 * k]])
    f = hip.Features.from_host(ctx, sets)
    pairs = [(i, j) for i in range(6) for j in range(6) if i != j]
    got = dict(zip(pairs, hip.match_pairs(ctx, cfg, f, pairs)))
    for i in range(6):
        for j in range(i + 1, 6):
            assert sorted(map(tuple, got[(i, j)])) == sorted(map(tuple, got[(j, i)][:, ::-1]))
            if len(got[(i, j)]):
                assert len(set(got[(i, j)][:, 0])) == len(got[(i, j)]) == len(set(got[(i, j)][:, 1]))
    for (i, j) in [(0, 1), (5, 2)]:
        assert np.array_equal(got[(i, j)], oracle.match_exact(sets[i], sets[j]))
    f.free()
