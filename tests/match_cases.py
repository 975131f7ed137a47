"""Descriptor scenes for the seams of the matcher (openpano_amd/csrc/match.hip; DESIGN.md, "The matcher at its seams").

Every case is a seeded, deterministic call: descriptor sets, a pair list, and its own CLAIMS -- the lists the exact matcher
has to return (written down from the construction, not taken from a run), survivor counts, and for the queue cases the
exact-scan queue lengths of the call.  tests/test_match_cases_cpu.py proves the claims on the oracle, on an independent
float64 model and on the ranking-key model; tests/test_gpu_match_cases.py holds the device to the oracle on the same calls.

The smaller set of a pair queries (matcher.cc:21), so the rows of the sweep come from the smaller set; every pair is passed
in both orders.

  A  geometry     32-column tiles, padded tail, 128-row blocks, reverse strip: ka x kb at 31/32/33 ... 255/256/257
  B  equal_keys   bit-equal columns (and rows) a whole number of tiles apart: same slot, same lane half, equal keys
  C  queue_*      exact-scan queue lengths chosen against slow_grid(): calls made in sequence on one fresh context
  D  images_*     feature tables of 4096 / 4097 images (the grouped / ungrouped exact-scan queue)
  E  pairs_*      1023 / 1024 / 1025 / 2049 pairs, > 131 072 accepted matches in one call
  F  sort         pairs with exactly 0 .. 4097 matches: the rank sort from LDS and from global memory
"""
import functools

import numpy as np

MARGIN = 8.2e-5                  # OP_MATCH_MARGIN: E = MARGIN * (|x|^2 + the call's largest |y|^2), on scores x.y - |y|^2 / 2
NK = 4                           # kept keys per lane half
RR = float(np.float32(0.8) * np.float32(0.8))       # MATCH_REJECT_NEXT_RATIO^2 as the matcher forms it (fp32)
SORT_LDS = 4096                  # kSortLds
ORDER_BINS = 4096                # kOrderBins
PLACE_THREADS = 512 * 256        # k_match_place: at most 512 workgroups of 256


def slow_grid(seen):
    """workgroups of the exact scan after a call that queued `seen` rows (-1: a fresh context)"""
    if seen < 0:
        return 2048
    return min((seen + seen // 4 + 64 + 7) & ~7, 2048)


def lane_half(col):
    """the lane half that holds column (or, in the reverse sweep, row) `col` of its 32-wide tile"""
    return (col >> 2) & 1


def rootsift(rng, n):
    """RootSIFT-like rows of norm 512; two independent rows are about 1.7e5 apart (squared)"""
    h = rng.gamma(0.6, 1.0, (n, 128))
    h[:, 0] += 1e-3
    return (np.sqrt(h / h.sum(axis=1, keepdims=True)) * 512).astype(np.float32)


def noisy(rng, rows, sigma):
    """copies of rows with N(0, sigma^2) added to every element: squared distance about 128 sigma^2"""
    return np.maximum(rows + rng.normal(0, sigma, np.shape(rows)), 0).astype(np.float32)


def bumped(v, j, d2):
    """v with element j raised by sqrt(d2): at squared distance d2 (up to the rounding of one element)"""
    out = v.copy()
    out[j] = np.float32(out[j] + np.float32(np.sqrt(d2)))
    return out


def sorted_list(rows):
    a = np.asarray(rows, np.int32).reshape(-1, 2)
    return a[np.lexsort((a[:, 1], a[:, 0]))]


def flipped(lst):
    return sorted_list(lst[:, ::-1])


class Case:
    """One op_match_pairs call.  lists[p]: the claimed result of pair p; survivors[p]: rows that pass the first ratio test
    (None: no claim); queue: claimed (forward, reverse) exact-scan rows of the call (None: no claim); fwd_rows / rev_rows:
    the planted (pair index, A row) entries of the two queues; accepted_from_queue: accepted matches that went through a queue."""

    def __init__(self, name, seam, sets, pairs, lists, survivors=None, queue=None, fwd_rows=(), rev_rows=(), queued_accepts=0):
        self.name, self.seam, self.sets, self.pairs, self.lists = name, seam, sets, [tuple(p) for p in pairs], lists
        self.survivors = survivors or [None] * len(pairs)
        self.queue, self.fwd_rows, self.rev_rows, self.queued_accepts = queue, list(fwd_rows), list(rev_rows), queued_accepts
        assert len(self.lists) == len(self.pairs) == len(self.survivors)

    def roles(self, p):
        """(A image, B image, swapped) of pair p: the smaller set is A"""
        i, j = self.pairs[p]
        rev = len(self.sets[i]) > len(self.sets[j])
        return (j, i, True) if rev else (i, j, False)

    def gmax(self):
        return max(float((s.astype(np.float64) ** 2).sum(1).max()) for s in self.sets if len(s))


_ORACLE = {}


def oracle_lists(oracle, case):
    """oracle.match_exact of every pair of the case, computed once per distinct (i, j) and kept for the process"""
    todo = [p for p in dict.fromkeys(case.pairs) if (case.name,) + p not in _ORACLE]
    big = [p for p in todo if len(case.sets[p[0]]) * len(case.sets[p[1]]) > 1 << 20]
    if len(big) > 1:                                 # the library call releases the interpreter lock
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(min(8, len(big))) as pool:
            for p, r in zip(big, pool.map(lambda p: oracle.match_exact(case.sets[p[0]], case.sets[p[1]]), big)):
                _ORACLE[(case.name,) + p] = r
    for p in todo:
        if (case.name,) + p not in _ORACLE:
            _ORACLE[(case.name,) + p] = oracle.match_exact(case.sets[p[0]], case.sets[p[1]])
    return [_ORACLE[(case.name,) + p] for p in case.pairs]


# ---- A: tile and row-block geometry -------------------------------------------------------------------------------------------

GEOM_KA = (1, 31, 32, 33, 127, 128, 129, 255, 256, 257)
GEOM_KB = (31, 32, 33, 63, 64, 65, 95, 96, 97, 257, 385)


def special_columns(kb):
    """column 0, 31, 32, the last valid column and the last column of the last full tile"""
    return [c for c in dict.fromkeys((kb - 1, 0, 31, 32, 32 * (kb // 32) - 1)) if 0 <= c < kb]


def _tail_ties(rng, kb, variant):
    """x (8 rows), y (kb columns) in the scheme of test_gpu_match._near_tie_sets, around the padded tail tile (kb = 1 mod 32: the
    last column is the only valid one of its tile).  A plan is a list of columns; with dup its first column is bit-equal to the
    row (accepted on distance 0) and the others are near-copies, without dup all are near-copies at squared distances 0.5,
    0.5625, ... whose ratios the test refuses.  Row 0 carries the variant's plan with the tail column, rows 1 .. 3 fixed
    plans beside the tail."""
    last = kb - 1
    tail_plans = [(True, [last, 0]), (True, [last, last - 32]), (True, [3, last]), (False, [last, 4]), (True, [last, 1, 2]), (False, [last - 32, last])]
    plans = [tail_plans[variant], (True, [last - 1, last - 33]), (False, [last - 2, last - 34]), (True, [last - 3, last - 7, last - 39])]
    x = rootsift(rng, 8)
    y = rootsift(rng, kb)
    want = []
    for r, (dup, cols) in enumerate(plans):
        for k, c in enumerate(cols):
            y[c] = x[r] if dup and k == 0 else bumped(x[r], 17 + 9 * k, 0.5 + 0.0625 * k)
        if dup:
            want.append((r, cols[0]))
    return x, y, sorted_list(want)


@functools.lru_cache(None)
def geometry():
    rng = np.random.default_rng(101)
    sets, pairs, lists, surv = [], [], [], []

    def add(ia, ib, want, s):
        pairs.extend([(ia, ib), (ib, ia)])
        lists.extend([want, flipped(want)])
        surv.extend([s, s if len(sets[ia]) != len(sets[ib]) else None])      # equal sizes: the other set queries in the second order

    for ka in GEOM_KA:
        A = rootsift(rng, ka)
        ia = len(sets); sets.append(A)
        for kb in sorted({ka} | {k for k in GEOM_KB if k >= ka}):
            sp = special_columns(kb)
            rest = [c for c in rng.permutation(kb) if c not in sp]
            cols = np.array((sp + rest)[:ka])
            col_of_row = cols[rng.permutation(ka)]
            B = rootsift(rng, kb)
            B[col_of_row] = noisy(rng, A, 1.0)
            sets.append(B)
            add(ia, len(sets) - 1, sorted_list(np.stack([np.arange(ka), col_of_row], 1)), ka)
        if ka == 257:                                 # row blocks of the reverse strip that exit at once: 0 and 1 survivors
            sets.append(rootsift(rng, 385))
            add(ia, len(sets) - 1, sorted_list([]), 0)
            B = rootsift(rng, 385)
            B[384] = noisy(rng, A[200], 1.0)
            sets.append(B)
            add(ia, len(sets) - 1, sorted_list([(200, 384)]), 1)
    for kb in (65, 97):
        for variant in range(6):
            x, y, want = _tail_ties(rng, kb, variant)
            sets.extend([x, y])
            add(len(sets) - 2, len(sets) - 1, want, None)
    return Case("geometry", "tiles of 32 columns, padded tail, 128-row blocks, reverse strip", sets, pairs, lists, surv)


# ---- B: equal keys across tiles --------------------------------------------------------------------------------------------------

@functools.lru_cache(None)
def equal_keys():
    """Bit-equal columns 32 apart share slot and lane half, so their keys are bit-equal: topk_attribute has to tell the old
    entry from the new one.  X rows 7 / 39 and 11 / 43 are the A-side twins (equal keys in the reverse sweep)."""
    rng = np.random.default_rng(202)
    x = rootsift(rng, 48)
    y = rootsift(rng, 160)
    want = []

    def plant(r, cols, d2s, accept):
        for k, (c, d2) in enumerate(zip(cols, d2s)):
            y[c] = x[r] if d2 == 0 else bumped(x[r], 3 + 7 * k, d2)
        if accept is not None:
            want.append((r, accept))

    plant(0, [5, 37, 69], [0, 0, 0], 5)                 # three tiles, one slot of lane half 1
    plant(1, [2, 66], [0, 0], 2)                        # c and c + 64
    plant(2, [7, 39, 71, 103], [0, 0, 0, 0], 7)         # four in one lane half: the exact scan, first index wins
    plant(3, [31, 63, 95], [0, 0, 0], 31)               # the last slot of a tile
    plant(4, [64, 128], [0, 0], 64)                     # the first slot
    plant(5, [10, 42, 74], [1.0, 1.5, 3.0], None)       # near-copy twins: 1 > 0.64 * 1.5
    plant(6, [12, 76], [1.0, 4.0], 12)                  # 1 <= 0.64 * 4
    plant(8, [44, 108], [3.0, 4.0], None)
    plant(9, [13, 45, 77, 109], [1.0, 5.0, 6.0, 7.0], 13)          # four near-copies in one half, accepted by the exact scan
    plant(10, [17, 49, 81, 113], [5.0, 6.5, 9.0, 10.0], None)      # ... refused by it: 5 > 0.64 * 6.5 (the third would accept: 5 <= 0.64 * 9)
    x[7] = y[20]; x[39] = y[20]                          # bit-equal A rows 32 apart, equal to one B column: both accepted (0 > 0.64 * 0 is false)
    want += [(7, 20), (39, 20)]
    x[11] = bumped(y[24], 9, 1.0); x[43] = bumped(y[24], 30, 4.0)   # near twins: row 43 is refused by the reverse test (4 > 0.64 * 1)
    want += [(11, 24)]
    want = sorted_list(want)
    return Case("equal_keys", "topk_attribute on bit-equal keys from different tiles", [x, y], [(0, 1), (1, 0)], [want, flipped(want)])


# ---- C / D: the exact-scan queue ---------------------------------------------------------------------------------------------------
# A unit is a pair of sets (A smaller, B larger) and a small set P, built so that the queues hold exactly the planted rows:
#   forward   row a = v, columns 4 r .. 4 r + 3 of B (one lane half) = v bumped to squared distances (2, 8, 9, 10): four keys
#             inside the margin in one half -> exact scan, accepted on the exact minimum; every 16th row instead
#             (5, 6.5, 9, 10): refused on the exact minimum and second minimum (5 > 0.64 * 6.5; the third would accept).
#             Row 0 of a unit has its exact duplicate in the LAST column of B (kb = 1 mod 32: alone in the padded tail tile,
#             lane half 0) and three near-copies at distances 30, 31, 32 in columns 0 .. 2.
#   reverse   s >= 4 rows of A in lane half 0 = one column v of B bumped to (2, 8, 9, ...): each survives the first test on
#             v, and the row v of the reverse sweep finds s keys inside the margin in one half -> s queued rows, the closest
#             one accepted; every 8th cluster instead (5, 6.5, 9, 10, ...): all refused, the closest only by the exact minimum.
# Every other row is kept clear of the overflow condition by construction, not by luck: each row of A has a companion
# row in A at sigma = 12 (squared distance about 18 000) and two columns of its own in B (sigma 1 and 5: about 128 and
# 3200), so the second-best key of every sweep row that is not planted is thousands above the third -- the margin E is 43.

FWD_ACCEPT, FWD_STRADDLE, FWD_TAIL = (2.0, 8.0, 9.0, 10.0), (5.0, 6.5, 9.0, 10.0), (30.0, 31.0, 32.0)
REV_ACCEPT, REV_STRADDLE = (2.0, 8.0, 9.0, 10.0, 11.0, 12.0, 13.0), (5.0, 6.5, 9.0, 10.0, 11.0, 12.0, 13.0)


def cluster_sizes(n):
    """n reverse rows as clusters of 4 .. 7"""
    if n == 0:
        return []
    assert n >= 4
    q, rem = divmod(n, 4)
    return [4 + (1 if k < rem % q else 0) + rem // q for k in range(q)]




def queue_unit(rng, nf, nr, n_ord=8):
    """-> dict(A, B, P, Q, ab / pa / qb: the claimed lists of (A, B), (P, A), (Q, B), fwd / rev: the planted forward and reverse
    rows of (A, B), accepts: accepted matches among them).  P and Q are near-copies of the ordinary rows of A and columns
    of B: (P, A) and (Q, B) are ordinary pairs on the same images that queue nothing."""
    sizes = cluster_sizes(nr)
    n_ord += n_ord & 1
    while True:                                       # enough other rows for the clusters to find their lane-half-0 positions
        ka = 2 * nf + n_ord + sum(sizes)
        if sum(1 for p in range(ka) if not lane_half(p)) >= sum(sizes):
            break
        n_ord += 2
    base_f = rootsift(rng, nf)                       # planted forward rows ...
    base_o = rootsift(rng, n_ord // 2)
    ordinary = np.concatenate([noisy(rng, base_f, 12.0), base_o, noisy(rng, base_o, 12.0)])      # ... their companions, and pairs of companions
    vs = rootsift(rng, len(sizes))                   # the B columns the reverse clusters copy
    half0 = [p for p in range(ka) if not lane_half(p)][:sum(sizes)]
    others = sorted(set(range(ka)) - set(half0))
    others = [others[k] for k in rng.permutation(len(others))]
    f_pos, o_pos = others[:nf], others[nf:]
    A = np.zeros((ka, 128), np.float32)
    ncol = 4 * nf + 2 * len(sizes) + 2 * len(ordinary)
    kb = max(ncol + 1, ka + 33)
    kb += (1 - kb) % 32                              # kb = 1 (mod 32): the last column is alone in its tile
    B = rootsift(rng, kb)
    ab, fwd, rev = [], [], []
    accepts = 0
    for r in range(nf):
        A[f_pos[r]] = base_f[r]
        fwd.append(f_pos[r])
        if r == 0:
            B[kb - 1] = base_f[0]
            for k, d2 in enumerate(FWD_TAIL):
                B[k] = bumped(base_f[0], 11 + 5 * k, d2)
            ab.append((f_pos[0], kb - 1)); accepts += 1
            continue
        d2s = FWD_STRADDLE if r % 16 == 15 else FWD_ACCEPT
        order = rng.permutation(4)
        for k in range(4):
            B[4 * r + order[k]] = bumped(base_f[r], 11 + 5 * k, d2s[k])
        if d2s is FWD_ACCEPT:
            ab.append((f_pos[r], 4 * r + order[0])); accepts += 1
    c = 4 * nf
    at = 0
    for g, s in enumerate(sizes):
        B[c] = vs[g]; B[c + 1] = noisy(rng, vs[g], 5.0)
        d2s = REV_STRADDLE if g % 8 == 7 else REV_ACCEPT
        order = rng.permutation(s)
        for k in range(s):
            p = half0[at + order[k]]
            A[p] = bumped(vs[g], 11 + 5 * k, d2s[k])
            rev.append(p)
            if k == 0 and d2s is REV_ACCEPT:
                ab.append((p, c)); accepts += 1
        at += s; c += 2
    o_cols = []
    for k, p in enumerate(o_pos):
        A[p] = ordinary[k]
        B[c] = noisy(rng, ordinary[k], 1.0); B[c + 1] = noisy(rng, ordinary[k], 5.0)
        ab.append((p, c)); o_cols += [c, c + 1]
        c += 2
    prow = f_pos + o_pos                             # every row of A outside the clusters: its companion is among them
    P = noisy(rng, A[prow], 1.0)
    Q = noisy(rng, B[o_cols], 1.0)
    return dict(A=A, B=B, P=P, Q=Q, ab=sorted_list(ab), pa=sorted_list(list(enumerate(prow))), qb=sorted_list(list(enumerate(o_cols))),
                fwd=sorted(fwd), rev=sorted(rev), accepts=accepts)


def split_queue(n):
    """n queued rows over three units, the first two listed in both orders: 2 a + 2 a + c = n"""
    a = n // 5 if n // 5 >= 4 else 0
    return a, a, n - 4 * a


def queue_call(name, seed, nf, nr, seam, images=None, where=None):
    """A call whose forward / reverse queues hold exactly nf / nr rows, spread over three units (three scanned images each
    way).  images / where: the size of the feature table and the image index of every set (default: 12 sets, packed)."""
    rng = np.random.default_rng(seed)
    units = [queue_unit(rng, f, r) for f, r in zip(split_queue(nf), split_queue(nr))]
    order = [(u, k) for u in range(3) for k in "ABPQ"]
    where = where or {uk: n for n, uk in enumerate(order)}
    sets = [np.zeros((0, 128), np.float32) for _ in range(images or len(order))]
    for u, k in order:
        sets[where[u, k]] = units[u][k]
    pairs, lists, fwd_rows, rev_rows = [], [], [], []
    accepts = 0
    for u, unit in enumerate(units):
        a, b, p, q = (where[u, k] for k in "ABPQ")
        todo = [((a, b), unit["ab"], True)] + ([((b, a), flipped(unit["ab"]), True)] if u < 2 else [])
        todo += [((p, a), unit["pa"], False), ((a, p), flipped(unit["pa"]), False), ((q, b), unit["qb"], False), ((b, q), flipped(unit["qb"]), False)]
        for pr, want, planted in todo:
            if planted:
                fwd_rows += [(len(pairs), r) for r in unit["fwd"]]
                rev_rows += [(len(pairs), r) for r in unit["rev"]]
                accepts += unit["accepts"]
            pairs.append(pr); lists.append(want)
    assert (len(fwd_rows), len(rev_rows)) == (nf, nr)
    return Case(name, seam, sets, pairs, lists, queue=(nf, nr), fwd_rows=fwd_rows, rev_rows=rev_rows, queued_accepts=accepts)


# queue lengths of consecutive calls on one fresh context, forward and reverse alike.  The grid of a call comes from the call
# before it: 2048 (fresh), 2048, 64, 320, 72, 152, 256 -- test_match_cases_cpu.py checks this list against slow_grid() and
# against what the sequence is for (n > 2048 with n % 8 != 0; 0; n > 2 grids with n % 8 != 0; n < 8; grid - 1, grid, grid + 1)
QUEUE_SEQUENCE = (2051, 0, 203, 5, 71, 152, 257)


@functools.lru_cache(None)
def queue_calls():
    return [queue_call("queue_%d" % n, 300 + k, n, n, "exact-scan queue of %d rows: grid, stride and XCD remap of k_match_slow" % n)
            for k, n in enumerate(QUEUE_SEQUENCE)]


@functools.lru_cache(None)
def image_tables():
    """tables of 4096 images (the queue is grouped by scanned image, one LDS counter each: images 0 and 4095 are the first and
    the last) and of 4097 (not grouped: k_match_slow reads the queue in arrival order), nearly all empty"""
    out = []
    for name, n, spots in (("images_4096a", 4096, (4095, 0, 2000, 1)), ("images_4096b", 4096, (0, 4095, 1, 2000)),
                           ("images_4097a", 4097, (4096, 0, 4095, 1)), ("images_4097b", 4097, (0, 4096, 1, 4095))):
        a0, b0, a1, b1 = spots
        where = {(0, "A"): a0, (0, "B"): b0, (0, "P"): 7, (0, "Q"): 8, (1, "A"): a1, (1, "B"): b1, (1, "P"): 9, (1, "Q"): 10,
                 (2, "A"): 11, (2, "B"): 12, (2, "P"): 13, (2, "Q"): 14}
        out.append(queue_call(name, 400 + len(out), 23, 22, "a feature table of %d images: %s exact-scan queue" % (n, "grouped" if n <= ORDER_BINS else "ungrouped"),
                              images=n, where=where))
    return out


# ---- E: pair-count and match-count seams -------------------------------------------------------------------------------------------

@functools.lru_cache(None)
def pair_lists():
    """1023 / 1024 / 1025 / 2049 pairs over five small sets.  k_match_offsets scans 1024 pairs per round with a carry;
    k_match_place has 131 072 threads and strides over more accepted matches than that (1025 pairs, 1023 of them the
    all-matching 129-row pair)."""
    rng = np.random.default_rng(505)
    s0 = rootsift(rng, 129)
    perm = rng.permutation(129)
    s1 = np.zeros_like(s0); s1[perm] = noisy(rng, s0, 1.0)
    s3 = rootsift(rng, 40)
    rows = rng.permutation(129)[:20]
    s4 = noisy(rng, s0[rows], 1.0)
    sets = [s0, s1, np.zeros((0, 128), np.float32), s3, s4]
    full = sorted_list(np.stack([np.arange(129), perm], 1))
    part = sorted_list(np.stack([np.arange(20), rows], 1))                  # (4, 0): 20 rows query 129
    ident = sorted_list(np.stack([np.arange(129)] * 2, 1))
    none = sorted_list([])
    want = {(0, 1): full, (1, 0): flipped(full), (0, 0): ident, (1, 1): ident, (0, 2): none, (2, 0): none, (0, 3): none, (3, 0): none,
            (4, 0): part, (0, 4): flipped(part), (3, 4): none, (2, 2): none}
    cycle = [(0, 1), (1, 0), (0, 0), (4, 0), (0, 2), (0, 1), (0, 4), (3, 0), (1, 1), (0, 1), (2, 0), (0, 3), (3, 4), (2, 2)]
    out = []
    for n in (1023, 1024, 1025, 2049):
        pairs = [cycle[k % len(cycle)] for k in range(n)]
        if n == 1025:
            pairs = [(0, 1) if k % 2 == 0 else (1, 0) for k in range(n)]
        for k, pr in ((1023, (0, 3)), (1024, (2, 0))):                      # zero-match pairs on either side of the carry
            if k < n:
                pairs[k] = pr
        out.append(Case("pairs_%d" % n, "%d pairs: chunked prefix of k_match_offsets%s" % (n, ", stride of k_match_place" if n == 1025 else ""),
                        sets, pairs, [want[p] for p in pairs]))
    return out


# ---- F: the list sort --------------------------------------------------------------------------------------------------------------

SORT_COUNTS = (0, 1, 2, 255, 256, 257, 4095, 4096, 4097)


@functools.lru_cache(None)
def sort_case():
    """one call, pairs with exactly m matches, the B rows permuted: up to kSortLds = 4096 matches a pair is ranked from LDS, beyond
    from global memory.  The large pairs query with all 4097 rows, the small ones with 600 of them."""
    rng = np.random.default_rng(606)
    big = rootsift(rng, 4097)
    sets = [big, big[:600].copy()]
    ca = np.stack([rng.uniform(-250, 250, 4097), rng.uniform(-170, 170, 4097)], 1)
    coors = [ca, ca[:600].copy()]
    pairs, lists = [], []
    for m in SORT_COUNTS:
        b = np.concatenate([noisy(rng, big[:m], 1.0), rootsift(rng, 200)])
        cb = np.concatenate([ca[:m] * 0.98 + (31.0, -7.0) + rng.normal(0, 0.4, (m, 2)), np.stack([rng.uniform(-300, 300, 200), rng.uniform(-200, 200, 200)], 1)])
        wrong = np.flatnonzero(rng.random(m) < 0.3)                          # outliers: the inlier set names entries of the list
        cb[wrong] = np.stack([rng.uniform(-300, 300, len(wrong)), rng.uniform(-200, 200, len(wrong))], 1)
        perm = rng.permutation(len(b))
        B = np.zeros_like(b); B[perm] = b
        cB = np.zeros_like(cb); cB[perm] = cb
        sets.append(B); coors.append(cB)
        ia, ib = (0 if m > 600 else 1), len(sets) - 1
        want = sorted_list(np.stack([np.arange(m), perm[:m]], 1))
        pairs += [(ia, ib), (ib, ia)]
        lists += [want, flipped(want)]
    case = Case("sort", "k_match_sort: rank from LDS up to 4096 matches of a pair, from global memory beyond", sets, pairs, lists)
    case.coors, case.shape = coors, (600, 400)       # keypoints under which the copies are one similarity apart: the lists feed RANSAC
    return case


# ---- the queue cap under a variant build (-DOP_MATCH_SLOW_CAP=64) -----------------------------------------------------------------

SLOW_CAP_VARIANT = 64


@functools.lru_cache(None)
def cap_calls():
    """in this order on one context: 65 forward rows (refused), 64 and 64 (served), 65 reverse rows (refused), an ordinary call"""
    seam = "exact-scan queue against its cap"
    return [queue_call("cap_forward_65", 701, 65, 0, seam), queue_call("cap_64", 702, 64, 64, seam),
            queue_call("cap_reverse_65", 703, 12, 65, seam), queue_call("cap_after", 704, 0, 0, seam)]


def all_cases():
    return [geometry(), equal_keys()] + queue_calls() + image_tables() + pair_lists() + [sort_case()] + cap_calls()
