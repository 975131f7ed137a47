"""CPU: the matcher's seam cases (tests/match_cases.py) do what they claim, and numpy restatements of the four index
computations behind the result lists see the slips the cases are there for ("The matcher at its seams").

1. Claims: every list a case writes down is what the oracle's exact matcher returns (and the reference's, where built);
   survivor counts from a float32 restatement of the first ratio test on the reference's four-partial-sum distance.
2. Queue lengths: the ranking-key model of test_matcher_margin_model.py over every sweep of the queue cases.  Planted rows
   overflow with half a margin to spare, every other row stays half a margin clear -- more than a different accumulation
   order on the device can move a key (see test_queue_lengths_are_exact).
3. An independent float64 matcher: outside a band around the ratio threshold that fp32 rounding explains, it lists what the
   oracle lists.
4. Index models with one slip each: the exact scan's work order, the chunked prefix, the rank sort, the top-4 attribution."""
import numpy as np
import pytest

import match_cases as mc
from test_matcher_margin_model import _bf16, _key_matrix

CASES = {c.name: c for c in mc.all_cases()}
QUEUE_CASES = [c.name for c in mc.queue_calls() + mc.image_tables() + mc.cap_calls()]
F32_MAX = np.finfo(np.float32).max


# ---- restatements ---------------------------------------------------------------------------------------------------------------

def d2_f32(x, y):
    """feature/dist.cc:22-57 in float32: four stride-4 partial sums walked in order, (v0 + v1) + (v2 + v3)"""
    out = np.empty((len(x), len(y)), np.float32)
    step = max(1, (1 << 22) // max(1, len(y) * 128))
    for r0 in range(0, len(x), step):
        d = x[r0:r0 + step, None, :] - y[None, :, :]
        d *= d
        v = np.zeros(d.shape[:2] + (4,), np.float32)
        for t in range(32):
            v += d[:, :, 4 * t:4 * t + 4]
        out[r0:r0 + step] = (v[:, :, 0] + v[:, :, 1]) + (v[:, :, 2] + v[:, :, 3])
    return out


def forward_f32(A, B):
    """first ratio test of every row of A against B (matcher.cc:33-55) -> (passes, best column, min, next_min)"""
    if len(A) == 0 or len(B) == 0:
        z = np.zeros(len(A), np.float32)
        return np.zeros(len(A), bool), np.full(len(A), -1), z, z
    D = d2_f32(A, B)
    idx = D.argmin(1)                                # the first index on equal minima, like the ascending scan
    mn = D[np.arange(len(A)), idx]
    if D.shape[1] > 1:
        D2 = D.copy(); D2[np.arange(len(A)), idx] = np.inf
        nx = D2.min(1).astype(np.float32)
    else:
        nx = np.full(len(A), F32_MAX, np.float32)
    return ~(mn > np.float32(mc.RR) * nx), idx, mn, nx


def key_matrix(x, y):
    """_key_matrix of test_matcher_margin_model.py without its temporaries (test_key_model_is_the_margin_models_own)"""
    xh = _bf16(x); xl = _bf16(x - xh)
    yh = _bf16(y); yl = _bf16(y - yh)
    ny = np.zeros(len(y), np.float32)
    for k in range(128):
        ny = (ny + y[:, k] * y[:, k]).astype(np.float32)
    acc = np.repeat((-(ny * np.float32(0.5))).astype(np.float32)[None], len(x), 0)
    tmp = np.empty_like(acc)
    for k in range(128):
        for a, b in ((xh, yh), (xh, yl), (xl, yh)):
            np.multiply(a[:, k, None], b[None, :, k], out=tmp)
            np.add(acc, tmp, out=acc)
    return (acc.view(np.uint32) & np.uint32(0xFFFFFFF0)).view(np.float32)


def key_rows(x, ycand):
    """the same model for row r of x against its own columns ycand[r] (n, c, 128) -> (n, c): a key depends on its row and its
    column only"""
    xh = _bf16(x); xl = _bf16(x - xh)
    yh = _bf16(ycand); yl = _bf16(ycand - yh)
    ny = np.zeros(ycand.shape[:2], np.float32)
    for k in range(128):
        ny = (ny + ycand[:, :, k] * ycand[:, :, k]).astype(np.float32)
    acc = (-(ny * np.float32(0.5))).astype(np.float32)
    for k in range(128):
        for a, b in ((xh, yh), (xh, yl), (xl, yh)):
            acc = (acc + (a[:, k, None] * b[:, :, k]).astype(np.float32)).astype(np.float32)
    return (acc.view(np.uint32) & np.uint32(0xFFFFFFF0)).view(np.float32)


TOP = 12         # columns per lane half whose keys are modelled; the rest is shown to be out of reach


def overflow_slack(X, Y, gmax):
    """per row of a sweep (rows X, columns Y): (a half's 4th largest key) - (the row's 2nd largest key - E), in units of E,
    the larger of the two lane halves.  >= 0: the row goes to the exact scan.  Keys are modelled for the TOP best columns
    of each half by float64 score; the best column left out is asserted to lie 4 E below the row's second best."""
    x64, y64 = X.astype(np.float64), Y.astype(np.float64)
    S = x64 @ y64.T - 0.5 * (y64 * y64).sum(1)[None]
    E = mc.MARGIN * ((x64 ** 2).sum(1) + gmax)
    second64 = np.sort(S, 1)[:, -2] if S.shape[1] >= 2 else np.full(len(X), -np.inf)
    half = np.array([mc.lane_half(c) for c in range(len(Y))])
    keys = []
    for h in (0, 1):
        cols = np.flatnonzero(half == h)
        if len(cols) > TOP:
            o = np.argsort(-S[:, cols], 1)
            assert np.all(S[np.arange(len(X)), cols[o[:, TOP]]] <= second64 - 4 * E)
            cols = cols[o[:, :TOP]]
        else:
            cols = np.tile(cols, (len(X), 1))
        keys.append(key_rows(X, Y[cols]).astype(np.float64) if cols.shape[1] else np.zeros((len(X), 0)))
    both = np.concatenate(keys, 1)
    second = np.sort(both, 1)[:, -2] if both.shape[1] >= 2 else np.full(len(X), -np.inf)
    slack = np.full(len(X), -np.inf)
    for K in keys:
        if K.shape[1] >= mc.NK:
            slack = np.maximum(slack, (np.sort(K, 1)[:, -mc.NK] - (second - E)) / E)
    return slack


def test_key_model_is_the_margin_models_own():
    rng = np.random.default_rng(3)
    x, y = mc.rootsift(rng, 37), mc.rootsift(rng, 70)
    y[5] = x[3]; y[9] = mc.bumped(x[3], 4, 2.0)
    want = _key_matrix(x, y).view(np.uint32)
    assert np.array_equal(key_matrix(x, y).view(np.uint32), want)
    cols = np.stack([rng.permutation(70)[:9] for _ in range(37)])
    assert np.array_equal(key_rows(x, y[cols]).view(np.uint32), np.take_along_axis(want, cols, 1))


# ---- 1. claims -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(CASES))
def test_claims_hold_on_the_oracle(oracle, name):
    case = CASES[name]
    got = mc.oracle_lists(oracle, case)
    fwd = {}
    for p, (g, want) in enumerate(zip(got, case.lists)):
        assert np.array_equal(g, want), (name, p, case.pairs[p], len(g), len(want))
        if case.survivors[p] is not None:
            ia, ib, _ = case.roles(p)
            if (ia, ib) not in fwd:
                fwd[ia, ib] = int(forward_f32(case.sets[ia], case.sets[ib])[0].sum())
            assert fwd[ia, ib] == case.survivors[p], (name, p, case.pairs[p])


def test_cases_reach_what_they_are_for():
    g = CASES["geometry"]
    sizes = {(len(g.sets[g.roles(p)[0]]), len(g.sets[g.roles(p)[1]])) for p in range(len(g.pairs))}
    for ka in mc.GEOM_KA:
        for kb in {ka} | {k for k in mc.GEOM_KB if k >= ka}:
            assert (ka, kb) in sizes
    cols = {}                                        # best matches per kb: column 0, 31, 32, the last valid one, the last of the last full tile
    rows = {}
    for p in range(0, len(g.pairs), 2):
        ia, ib, _ = g.roles(p)
        if g.survivors[p] == len(g.sets[ia]):
            cols.setdefault(len(g.sets[ib]), set()).update(g.lists[p][:, 1].tolist())
            rows.setdefault(len(g.sets[ia]), set()).update(g.lists[p][:, 0].tolist())
    for kb, seen in cols.items():
        if kb > 1:
            assert kb - 1 in seen
    assert {0, 31, 32, 384, 383} <= cols[385] and {0, 31, 32, 96, 95} <= cols[97] and {0, 31, 32, 64, 63} <= cols[65]
    assert {127, 128, 256} <= rows[257] and {127, 128} <= rows[129] and 127 in rows[128]
    assert sorted(g.survivors[p] for p in range(0, len(g.pairs), 2) if g.survivors[p] is not None and len(g.sets[g.roles(p)[0]]) == 257 and g.survivors[p] < 2) == [0, 1]
    # E: the carry of the prefix and the stride of the scatter
    counts = {c.name: sum(len(l) for l in c.lists) for c in mc.pair_lists()}
    assert counts["pairs_1025"] > mc.PLACE_THREADS and [len(c.pairs) for c in mc.pair_lists()] == [1023, 1024, 1025, 2049]
    for c in mc.pair_lists():
        for k in (1023, 1024):
            assert k >= len(c.pairs) or len(c.lists[k]) == 0
        assert any(i == j for i, j in c.pairs) or c.name == "pairs_1025"
    # F: both sides of kSortLds, both orders
    s = CASES["sort"]
    assert [len(l) for l in s.lists[0::2]] == list(mc.SORT_COUNTS) == [len(l) for l in s.lists[1::2]]
    assert mc.SORT_LDS in mc.SORT_COUNTS and mc.SORT_LDS + 1 in mc.SORT_COUNTS
    for l in s.lists:
        assert not np.array_equal(l[:, 1], np.sort(l[:, 1])) or len(l) < 3        # the second index is permuted
    # D: tables on both sides of kOrderBins, queued rows that scan the first and the last image
    for c in mc.image_tables():
        scanned_f = {c.roles(p)[1] for p, _ in c.fwd_rows}; scanned_r = {c.roles(p)[0] for p, _ in c.rev_rows}
        assert len(c.sets) in (mc.ORDER_BINS, mc.ORDER_BINS + 1) and len(scanned_f) >= 3 and len(scanned_r) >= 3
        assert (0 in scanned_f and len(c.sets) - 1 in scanned_r) or (0 in scanned_r and len(c.sets) - 1 in scanned_f)
    assert {4095} <= {c.roles(p)[1] for c in mc.image_tables() for p, _ in c.fwd_rows} | {c.roles(p)[0] for c in mc.image_tables() for p, _ in c.rev_rows}


def test_queue_sequence_meets_every_grid_condition():
    """the grids the calls of QUEUE_SEQUENCE run under, forward and backward through the list, from slow_grid()"""
    seq = mc.QUEUE_SEQUENCE
    grids = [mc.slow_grid(s) for s in (-1,) + seq[:-1]]
    assert grids == [2048, 2048, 64, 320, 72, 152, 256]
    ng = list(zip(seq, grids))
    assert ng[0][0] > 2048 and ng[0][0] % 8                                   # strides on the fresh context, with a tail the remap leaves alone
    assert (0, 2048) in ng                                                    # an empty queue under a full grid
    assert any(0 < n < 8 for n, _ in ng)                                      # per = 0: no remap at all
    assert any(n > 2 * g and n % 8 for n, g in ng[1:])                        # more than two rounds of a small grid
    for d in (-1, 0, 1):
        assert any(n == g + d for n, g in ng)
    back = [mc.slow_grid(s) for s in (-1,) + seq[::-1][:-1]]
    assert back != grids[::-1] and len(set(back)) >= 5                        # the other order really runs other grids
    for c in mc.queue_calls():
        assert len({c.roles(p)[1] for p, _ in c.fwd_rows}) in (0, 1, 3) and len({c.roles(p)[0] for p, _ in c.rev_rows}) in (0, 1, 3)
    big = CASES["queue_2051"]
    assert len({big.roles(p)[1] for p, _ in big.fwd_rows}) == 3 and len({big.roles(p)[0] for p, _ in big.rev_rows}) == 3


@pytest.mark.parametrize("name", list(CASES))
def test_oracle_equals_reference(oracle, ref, name):
    case = CASES[name]
    got = mc.oracle_lists(oracle, case)
    seen = set()
    for p, (i, j) in enumerate(case.pairs):
        if (i, j) not in seen:
            seen.add((i, j))
            assert np.array_equal(ref.match_exact(case.sets[i], case.sets[j]), got[p]), (name, p, i, j)


# ---- 2. queue lengths -----------------------------------------------------------------------------------------------------------

GAP = 0.5        # in units of E


@pytest.mark.parametrize("name", QUEUE_CASES)
def test_queue_lengths_are_exact(name):
    """A row is queued when the 4th key of one of its lane halves is within E of its 2nd best key.  The device sums the same
    384 products per key as the model, in another order.  Every product is >= 0 here up to the tiny lo terms (descriptors
    are non-negative), so a running sum stays inside [-|y|^2 / 2, |x|^2 / 2] and one fp32 addition rounds by at most
    2^-25 (|x|^2 + |y|^2): 385 of them move a key by at most 1.15e-5 (|x|^2 + |y|^2) = 0.14 E, the slot bits by another
    2^-20 (|x|^2 + |y|^2) = 0.012 E.  The comparison is between two keys: 0.31 E at the very worst.  Planted rows clear the
    condition by GAP = 0.5 E, all others miss it by at least as much, so the length of each queue is the planted count
    whatever the order."""
    case = CASES[name]
    gmax = case.gmax()
    sweeps = {}
    total = [0, 0]
    worst = [np.inf, -np.inf]
    for p in range(len(case.pairs)):
        ia, ib, _ = case.roles(p)
        A, B = case.sets[ia], case.sets[ib]
        if len(A) == 0 or len(B) == 0:
            continue
        if (ia, ib) not in sweeps:
            f_slack = overflow_slack(A, B, gmax)
            ok, idx, _, _ = forward_f32(A, B)
            surv = np.flatnonzero(ok)
            r_slack = np.full(len(A), -np.inf)
            if len(surv):
                r_slack[surv] = overflow_slack(B[idx[surv]], A, gmax)
            sweeps[ia, ib] = (f_slack, r_slack)
        for d, (slack, planted) in enumerate(zip(sweeps[ia, ib], (case.fwd_rows, case.rev_rows))):
            rows = np.array([r for q, r in planted if q == p], int)
            mask = np.zeros(len(A), bool); mask[rows] = True
            assert len(rows) == 0 or slack[mask].min() >= GAP, (name, p, d, "a planted row is not safely queued", float(slack[mask].min()))
            assert mask.all() or slack[~mask].max() <= -GAP, (name, p, d, "another row is not safely clear", float(slack[~mask].max()))
            total[d] += len(rows)
            if len(rows):
                worst[0] = min(worst[0], float(slack[mask].min()))
            if not mask.all():
                worst[1] = max(worst[1], float(slack[~mask].max()))
    print(name, "queue", total, "planted slack >= %.2f E, others <= %.1f E" % tuple(worst))
    assert tuple(total) == case.queue


def test_queued_rows_decide_lists():
    """the accepted matches among the queued rows: at least 64 distinct ones per call where the queue is that long -- a dropped,
    repeated or mis-addressed entry of the forward queue changes a list with probability 15 / 16 per entry"""
    for c in mc.queue_calls() + mc.image_tables():
        accepted = {(p, r) for p, r in c.fwd_rows + c.rev_rows if r in set(c.lists[p][:, 1 if c.roles(p)[2] else 0].tolist())}
        fwd_acc = sum((p, r) in accepted for p, r in c.fwd_rows)
        assert len(accepted) == c.queued_accepts
        assert c.queue[0] < 71 or len(accepted) >= 64, (c.name, len(accepted))
        assert c.queue[0] < 16 or fwd_acc >= 0.9 * c.queue[0], c.name
        partners = {(p, tuple(row)) for p, r in accepted for row in c.lists[p].tolist() if row[1 if c.roles(p)[2] else 0] == r}
        assert len(partners) == len(accepted)


# ---- 3. float64 ------------------------------------------------------------------------------------------------------------------

U = 2.0 ** -24
# A computed distance is sum_k fl(fl(x_k - y_k)^2) over four lanes of 32 terms: one rounding for the difference (squared: two
# factors), one for the square, at most 31 additions in the lane and two in (v0 + v1) + (v2 + v3) -- every term is >= 0, so
# the relative error is at most 36 u.  The test compares mn with fl(r^2 * next) (one more rounding, the same fp32 r^2 on both
# sides), two distances per comparison: it can only differ from the exact comparison where |mn / (r^2 next) - 1| <= 2 * 36 u
# + u + O(u^2).  BAND = 80 u.
BAND = 80 * U


def fp64_matcher(A, B):
    """exact matcher in float64, A queries -> (accepted, best column, inside the band) per row of A"""
    n, m = len(A), len(B)
    if n == 0 or m == 0:
        return np.zeros(n, bool), np.full(n, -1), np.zeros(n, bool)
    a, b = A.astype(np.float64), B.astype(np.float64)
    D = (a * a).sum(1)[:, None] + (b * b).sum(1)[None] - 2 * a @ b.T              # only ranks; the few smallest are recomputed from differences

    def smallest(D, rows, cols, k, skip_self):
        """per row the k smallest of D (ascending by exact distance, then by index), exact"""
        if skip_self:
            D = D.copy(); D[np.arange(len(D)), np.arange(len(D))] = np.inf
        k = min(k, D.shape[1])
        cand = np.sort(np.argpartition(D, k - 1, axis=1)[:, :k] if k < D.shape[1] else np.tile(np.arange(D.shape[1]), (len(D), 1)), 1)
        ex = ((rows[:, None, :] - cols[cand]) ** 2).sum(2)
        if skip_self:
            ex[cand == np.arange(len(D))[:, None]] = np.inf
        o = np.argsort(ex, 1, kind="stable")
        return np.take_along_axis(cand, o, 1), np.take_along_axis(ex, o, 1)

    c, e = smallest(D, a, b, 8, False)
    idx, mn = c[:, 0], e[:, 0]
    nx = e[:, 1] if e.shape[1] > 1 else np.full(n, float(F32_MAX))
    if n > 1:
        _, er = smallest(D[:, idx].T, b[idx], a, 8, True)
        nx2 = np.minimum(nx, er[:, 0])
    else:
        nx2 = nx
    accepted = ~(mn > mc.RR * nx) & ~(mn > mc.RR * nx2)
    band = (np.abs(mn - mc.RR * nx) < BAND * mc.RR * nx) | (np.abs(mn - mc.RR * nx2) < BAND * mc.RR * nx2)
    return accepted, idx, band


@pytest.mark.parametrize("name", list(CASES))
def test_float64_matcher_lists_the_same(oracle, name):
    case = CASES[name]
    got = mc.oracle_lists(oracle, case)
    done = {}
    rows = left_out = 0
    for p, (i, j) in enumerate(case.pairs):
        if (i, j) in done:
            continue
        done[i, j] = True
        ia, ib, swapped = case.roles(p)
        acc, idx, band = fp64_matcher(case.sets[ia], case.sets[ib])
        lst = got[p][:, ::-1] if swapped else got[p]
        listed = np.full(len(acc), -1)
        listed[lst[:, 0]] = lst[:, 1]
        assert len(set(lst[:, 0].tolist())) == len(lst)
        check = ~band
        assert np.array_equal(listed[check] >= 0, acc[check]), (name, p, "listed and accepted rows differ outside the band")
        both = check & acc
        assert np.array_equal(listed[both], idx[both]), (name, p, "a listed partner is not the float64 nearest column")
        rows += len(acc); left_out += int(band.sum())
    print(name, "rows", rows, "inside the band", left_out)
    assert left_out <= 0.01 * rows, (name, left_out, rows)


# ---- 4. index models --------------------------------------------------------------------------------------------------------------

def scan_order(n, slip=False):
    """queue entry that work item lin = 0 .. n - 1 of the exact scan takes.  Intent: workgroup lin runs on XCD lin & 7, and each
    XCD is to take a contiguous eighth of the (grouped) queue; the n % 8 entries that do not fill an eighth keep their place."""
    lin = np.arange(n)
    per = n >> 3
    whole = n if slip else per * 8
    return np.where(lin < whole, (lin & 7) * per + (lin >> 3), lin)


def grid_visits(n, grid):
    """work items in the order the workgroups of a grid take them: workgroup b takes b, b + grid, ..."""
    return np.concatenate([np.arange(b, n, grid) for b in range(grid)]) if n else np.arange(0)


def test_scan_order_is_a_permutation():
    for n in range(5001):
        assert np.array_equal(np.sort(scan_order(n)), np.arange(n)), n
    grids = sorted({mc.slow_grid(s) for s in range(-1, 4200)})
    assert grids[0] == 64 and grids[-1] == 2048 and all(g % 8 == 0 for g in grids) and len(grids) == 249
    for g in grids:
        for n in (0, 1, 7, g - 1, g, g + 1, 2 * g + 3, 5000):
            assert np.array_equal(np.sort(grid_visits(n, g)), np.arange(n)), (g, n)
    for n, g in ((2051, 2048), (203, 64)):          # each XCD's first `per` items are one contiguous eighth
        o = scan_order(n)
        for x in range(8):
            mine = o[np.arange(n) % 8 == x][:n >> 3]
            assert np.array_equal(mine, x * (n >> 3) + np.arange(n >> 3))


def test_slip_in_scan_order_is_seen_by_the_queue_cases():
    """`per * 8` replaced by `n`: the n % 8 last work items are remapped too, onto entries that were already taken.  Seen by
    every queue case with n % 8 != 0 -- queue_2051, queue_203, queue_5 (per = 0: every item takes entry 0), queue_71,
    queue_257 and the image tables (23 / 22 rows): entries are dropped and others scanned twice, and an accepted forward entry
    scanned twice is listed twice."""
    for c in mc.queue_calls() + mc.image_tables():
        for n, planted in zip(c.queue, (c.fwd_rows, c.rev_rows)):
            good, bad = scan_order(n), scan_order(n, slip=True)
            assert np.array_equal(good, bad) == (n % 8 == 0), (c.name, n)
            if n % 8:
                assert len(set(bad.tolist())) == n - n % 8 if n >= 8 else len(set(bad.tolist())) == 1
    c = CASES["queue_2051"]
    taken = [c.fwd_rows[i] for i in scan_order(2051, slip=True)]
    accepted = {(p, r) for p, r in c.fwd_rows if r in set(c.lists[p][:, 1 if c.roles(p)[2] else 0].tolist())}
    assert sorted(set(taken) & accepted) != sorted(accepted) or len([t for t in taken if t in accepted]) != len(accepted)


def chunked_offsets(counts, slip=False):
    """exclusive prefix of the per-pair counts as a workgroup of 1024 computes it: 1024 pairs per round, the total of the
    rounds before carried into the next -> npairs + 1 offsets"""
    counts = np.asarray(counts, np.int64)
    out = np.zeros(len(counts) + 1, np.int64)
    carry = 0
    for base in range(0, len(counts), 1024):
        c = counts[base:base + 1024]
        incl = np.cumsum(c)
        out[base:base + len(c)] = (0 if slip else carry) + incl - c
        carry = carry + int(incl[-1])
    out[len(counts)] = carry
    return out


def placed(case, offsets):
    """the flat list of a call when every pair's list is written at its offset"""
    flat = np.full((int(sum(len(l) for l in case.lists)) + 1, 2), -1, np.int64)
    for l, o in zip(case.lists, offsets):
        flat[o:o + len(l)] = l
    return flat


def test_chunked_prefix_and_its_slip():
    """the carry not added across rounds: pairs from 1024 on start at 0 again and overwrite the first pairs' segments.  Seen by
    pairs_2049 (matches on both sides of both carries) and by pairs_1025 only through the total, since its pair 1024 is empty on
    purpose -- which is why the 2049-pair list is in the set.  pairs_1023 / pairs_1024 are the last sizes that need no carry."""
    rng = np.random.default_rng(1)
    for n in (0, 1, 1023, 1024, 1025, 2048, 2049, 5000):
        counts = rng.integers(0, 9, n)
        assert np.array_equal(chunked_offsets(counts), np.concatenate([[0], np.cumsum(counts)]))
    for c in mc.pair_lists():
        counts = [len(l) for l in c.lists]
        good, bad = chunked_offsets(counts), chunked_offsets(counts, slip=True)
        differs = not np.array_equal(placed(c, good), placed(c, bad))
        assert differs == (c.name == "pairs_2049"), c.name
        assert np.array_equal(good[:-1], bad[:-1]) == (len(c.pairs) <= 1024), c.name


def rank_sort(seg, slip=False):
    """a pair's segment in arrival order -> sorted by (first, second): entry i goes to the number of entries below it (the
    (first, second) of a pair are distinct, so the ranks are a permutation).  One slot more than the segment is returned."""
    seg = np.asarray(seg, np.int64).reshape(-1, 2)
    out = np.full((len(seg) + 1, 2), -1, np.int64)
    if len(seg) == 1:
        out[0] = seg[0]
    elif len(seg) > 1:
        key = (seg[:, 0] << 32) | seg[:, 1]
        rank = (key[None, :] <= key[:, None]).sum(1) if slip else (key[None, :] < key[:, None]).sum(1)
        out[rank] = seg
    return out


def test_rank_sort_and_its_slip():
    """`<=` in the rank: every entry lands one slot late, the first slot keeps what was there and the last entry leaves the
    segment.  Seen by every pair with two or more matches: the m = 2 pair of `sort` is the smallest."""
    rng = np.random.default_rng(2)
    s = CASES["sort"]
    for l in s.lists:
        if len(l) > 600:
            continue                                 # (the model is quadratic in memory; the long lists sort the same way)
        arrival = l[rng.permutation(len(l))]
        good, bad = rank_sort(arrival), rank_sort(arrival, slip=True)
        assert np.array_equal(good[:len(l)], l) and np.all(good[len(l):] == -1)
        assert np.array_equal(bad[:len(l)], l) == (len(l) < 2), len(l)
    for c in (CASES["geometry"], CASES["equal_keys"]):
        for l in c.lists:
            assert np.array_equal(rank_sort(l[rng.permutation(len(l))])[:len(l)], l)


def slot_key(score, slot):
    return ((np.asarray(score, np.float32).view(np.uint32) & np.uint32(0xFFFFFFF0)) | np.asarray(slot, np.uint32)).view(np.float32)


def topk_tile(ts, tt, keys, t, slip=False):
    """One tile of one lane half for a batch of rows.  ts (S, 4): the kept keys, descending; tt (S, 4): the tile each came
    from; keys (S, 16): this tile's keys.  Intent of the attribution: the new list is a merge of the old list (order kept) and
    this tile's keys, so walk the new list with a cursor on the old one: a new-list entry equal to the old entry under the
    cursor is that old entry (keeps its tile, cursor moves on), anything else came from this tile."""
    old, old_t = ts.copy(), tt.copy()
    new = -np.sort(-np.concatenate([ts, keys], 1), 1)[:, :4]
    rows = np.arange(len(ts))
    cur = np.zeros(len(ts), int)                     # old entries used so far
    out_t = np.empty_like(tt)
    was_old = None
    for r in range(4):
        at = cur
        if slip and r == 3:
            at = np.where(was_old, 1, cur)           # THE SLIP: behind a matched slot 2 the cursor is taken to be 1, whatever slots 0 and 1 used
        is_old = new[:, r] == old[rows, at]
        out_t[:, r] = np.where(is_old, old_t[rows, at], t)
        was_old = is_old
        cur = cur + is_old
    return new, out_t


def sweep_half(keys, ky, h, slip=False):
    """the kept (key, column) list of lane half h after the sweep of a batch of rows: keys (S, ky) are the scores, the slot goes
    into their low bits, padded columns hold -FLT_MAX; -> ms (S, 4), mi (S, 4) with -1 for entries that are no column"""
    S = len(keys)
    ts = np.full((S, 4), -F32_MAX, np.float32); tt = np.full((S, 4), -1)
    regs = np.arange(16)
    cols = (regs & 3) + 8 * (regs >> 2) + 4 * h
    for t in range((ky + 31) // 32):
        c = t * 32 + cols
        tile = np.full((S, 16), -F32_MAX, np.float32)
        tile[:, c < ky] = keys[:, c[c < ky]]
        ts, tt = topk_tile(ts, tt, slot_key(tile, regs[None, :]), t, slip)
    reg = ts.view(np.uint32) & np.uint32(15)
    col = tt * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * h
    return ts, np.where((tt < 0) | (col >= ky), -1, col)


def sweep_overflow(X, Y, gmax, slip=False):
    """rows of the sweep that go to the exact scan, from the kept lists of the two halves as the epilogue reads them"""
    K = key_matrix(X, Y)
    E = mc.MARGIN * ((X.astype(np.float64) ** 2).sum(1) + gmax)
    (m0, i0), (m1, i1) = sweep_half(K, len(Y), 0, slip), sweep_half(K, len(Y), 1, slip)
    second = np.maximum(np.minimum(m0[:, 0], m1[:, 0]), np.maximum(m0[:, 1], m1[:, 1])).astype(np.float64)
    thr = second - E
    return ((i0[:, 3] >= 0) & (m0[:, 3] >= thr)) | ((i1[:, 3] >= 0) & (m1[:, 3] >= thr))


def test_topk_keeps_distinct_entries_on_equal_keys():
    """sequences of tiles whose keys come from a handful of values, so that equal keys from different tiles (same slot) and near
    keys abound: after every tile the kept keys are the four largest seen, every kept (key, tile) is an entry that exists, and
    no entry is kept twice.  With the slip some sequence breaks that."""
    S, T = 20000, 6
    base = np.float32(1000.0) + 16 * np.arange(12, dtype=np.float32)          # 16 apart: the slot bits never carry over
    broken = 0
    for slip in (False, True):
        ts = np.full((S, 4), -F32_MAX, np.float32); tt = np.full((S, 4), -1)
        seen = np.full((S, T, 16), -F32_MAX, np.float32)
        bad = np.zeros(S, bool)
        r = np.random.default_rng(4)
        for t in range(T):
            keys = slot_key(base[r.integers(0, 12, (S, 16))] * (r.random((S, 16)) < 0.4) - 5.0, np.arange(16)[None, :])
            seen[:, t] = keys
            ts, tt = topk_tile(ts, tt, keys, t, slip)
            top = -np.sort(-seen[:, :t + 1].reshape(S, -1), 1)[:, :4]
            bad |= (ts != top).any(1)
            slot = (ts.view(np.uint32) & np.uint32(15)).astype(int)
            exists = seen[np.arange(S)[:, None], np.maximum(tt, 0), slot] == ts
            bad |= ~(exists & (tt >= 0)).all(1)
            for a in range(4):
                for b in range(a + 1, 4):
                    bad |= (ts[:, a] == ts[:, b]) & (tt[:, a] == tt[:, b])
        if slip:
            broken = int(bad.sum())
        else:
            assert not bad.any(), int(bad.sum())
    assert broken > 0


def test_slip_in_topk_attribution_is_seen_by_the_queue_cases():
    """Only the fourth kept entry's tile depends on the selection the slip drops, and the epilogue reads that tile in one place:
    `mi[3] >= 0`, whether the fourth entry is a column at all.  With the slip, a tile that changes nothing in a full list
    (slots 0 .. 2 old) compares slot 3 with the wrong old entry and attributes it to that tile; the sweep of a queue unit ends
    on a padded tail tile (kb = 1 mod 32) in which only slot 0 of lane half 0 is a column, so the fourth of four near-ties
    ends up as "no column" and the row is not queued.  The forward queues of every queue_* and images_* call with planted
    rows come out short -- the first planted row of a unit, whose duplicate sits in that tail column, among them -- which
    the GPU test reads through op_debug_match_last_slow."""
    for name in ("queue_71", "images_4097a"):
        c = CASES[name]
        gmax = c.gmax()
        for p in sorted({p for p, _ in c.fwd_rows}):
            ia, ib, _ = c.roles(p)
            A, B = c.sets[ia], c.sets[ib]
            rows = np.array([r for q, r in c.fwd_rows if q == p])
            good, bad = sweep_overflow(A, B, gmax), sweep_overflow(A, B, gmax, slip=True)
            assert np.array_equal(np.flatnonzero(good), np.sort(rows)), (name, p)
            assert not np.any(bad & ~good)
            lost = set(np.flatnonzero(good & ~bad).tolist())
            tail = [int(r) for r in rows if np.array_equal(A[r], B[len(B) - 1])]
            assert len(tail) == 1 and tail[0] in lost, (name, p, lost, tail)
