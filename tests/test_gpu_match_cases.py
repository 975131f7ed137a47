"""GPU: the matcher at its seams (tests/match_cases.py; DESIGN.md, "The matcher at its seams").  Every call of every case
has to return the oracle's lists, pair by pair and in order; the queue cases also have to queue exactly the rows they were
built to queue (op_debug_match_last_slow), checked apart from the lists: a length that is off means the scene missed its
seam.  What each case is for, and that its claims hold, is tests/test_match_cases_cpu.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

import match_cases as mc
import ransac_scenes as rs
import variant_lib

pytestmark = pytest.mark.gpu

PLAIN = [mc.geometry, mc.equal_keys] + [(lambda k=k: mc.pair_lists()[k]) for k in range(4)]
PLAIN_IDS = ["geometry", "equal_keys", "pairs_1023", "pairs_1024", "pairs_1025", "pairs_2049"]


@pytest.fixture(scope="module")
def ctx():
    from openpano_amd import hip
    c = hip.Context(0)
    yield c
    c.close()


def assert_lists(case, got, want, what=""):
    assert len(got) == len(want) == len(case.pairs)
    for p, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), "%s%s: pair %d %r: %d matches on the device, %d in the oracle%s" % (
            case.name, what, p, case.pairs[p], len(g), len(w),
            "" if len(g) != len(w) else ", first difference at entry %d" % int(np.flatnonzero((g != w).any(1))[0]))


def run_call(ctx, cfg, oracle, case):
    """the call on ctx -> its lists, read through the handle (all at once and pair by pair) and held to the oracle"""
    from openpano_amd import hip
    want = mc.oracle_lists(oracle, case)
    f = hip.Features.from_host(ctx, case.sets)
    try:
        mh = hip.match_pairs_handle(ctx, cfg, f, case.pairs)
        try:
            got = [a.copy() for a in mh.lists()]
            assert mh.total == sum(len(g) for g in got)
            for p in sorted({0, len(case.pairs) // 2, len(case.pairs) - 1}):
                assert np.array_equal(mh.get(p), got[p]), (case.name, p)
        finally:
            mh.free()
    finally:
        f.free()
    assert_lists(case, got, want)
    return got


def assert_queue(ctx, case):
    got = ctx.match_last_slow()
    assert got == case.queue, "%s missed its seam: the call queued %r (forward, reverse) rows for the exact scan, the scene was built for %r" % (
        case.name, got, case.queue)


@pytest.mark.parametrize("make", PLAIN, ids=PLAIN_IDS)
def test_case_equals_oracle(ctx, cfg, oracle, make):
    case = make()
    got = run_call(ctx, cfg, oracle, case)
    assert_lists(case, got, case.lists, " (claimed lists)")
    from openpano_amd import hip
    f = hip.Features.from_host(ctx, case.sets)
    try:
        assert_lists(case, hip.match_pairs(ctx, cfg, f, case.pairs), got, " (match_pairs)")
    finally:
        f.free()


_SEQUENCE = {}


@pytest.mark.parametrize("order", ["forward", "backward"])
def test_queue_sequence_on_a_fresh_context(cfg, oracle, order):
    """the calls of QUEUE_SEQUENCE on a context of their own: every call's exact scans run on the grid the call before left
    (2048, 2048, 64, 320, 72, 152, 256 going forward, other grids going backward), the lists are the oracle's either way
    and the queues hold the planted rows"""
    from openpano_amd import hip
    calls = mc.queue_calls()
    c = hip.Context(0)
    try:
        assert c.match_last_slow() == (-1, -1)
        for case in (calls if order == "forward" else calls[::-1]):
            got = run_call(c, cfg, oracle, case)
            assert_queue(c, case)
            _SEQUENCE.setdefault(case.name, []).append(got)
    finally:
        c.close()
    for name, runs in _SEQUENCE.items():              # the same lists whatever grid the call ran on
        for other in runs[1:]:
            assert all(np.array_equal(a, b) for a, b in zip(runs[0], other)), name


@pytest.mark.parametrize("k", range(4), ids=["images_4096a", "images_4096b", "images_4097a", "images_4097b"])
def test_image_count_seam(cfg, oracle, k):
    from openpano_amd import hip
    case = mc.image_tables()[k]
    c = hip.Context(0)
    try:
        run_call(c, cfg, oracle, case)
        assert_queue(c, case)
        run_call(c, cfg, oracle, case)                # and on the grid that call left
        assert_queue(c, case)
    finally:
        c.close()


def test_sorted_lists_on_the_device(ctx, cfg, oracle):
    """case F through the handle: joined with a second result (two device-to-device copies of the sorted buffers) and fed to
    one op_ransac_pairs call, which reads the lists on the device -- an order other than the oracle's draws other samples"""
    from openpano_amd import hip
    case = mc.sort_case()
    want = mc.oracle_lists(oracle, case)
    extra = [(1, 3), (4, 1)]
    want_extra = [oracle.match_exact(case.sets[i], case.sets[j]) for i, j in extra]
    f = hip.Features.from_host(ctx, case.sets, case.coors)
    a = b = j = None
    try:
        a = hip.match_pairs_handle(ctx, cfg, f, case.pairs)
        b = hip.match_pairs_handle(ctx, cfg, f, extra)
        j = hip.Matches.concat(ctx, a, b)             # before anything is read: the joined lists exist on the device only
        pairs = case.pairs + extra
        seeds = [1000 + p for p in range(len(pairs))]
        res = hip.ransac_pairs(ctx, cfg, f, j, pairs, [case.shape] * len(case.sets), seeds=seeds)
        joined = [x.copy() for x in j.lists()]
        first = [x.copy() for x in a.lists()]
    finally:
        for h in (j, b, a):
            if h:
                h.free()
        f.free()
    assert_lists(case, first, want)
    assert_lists(case, joined[:len(case.pairs)], want, " (joined)")
    assert all(np.array_equal(g, w) for g, w in zip(joined[len(case.pairs):], want_extra))
    accepted = 0
    for p, ((i, k), r, m) in enumerate(zip(pairs, res, want + want_extra)):
        w = rs.check(oracle, r, m, case.coors[i], case.coors[k], case.shape, case.shape, seeds[p])
        accepted += bool(w["ok"])
    assert accepted >= 10                             # the long lists are accepted pairs, with inliers that index the lists


# ---- the queue cap, under a variant build ---------------------------------------------------------------------------------------

CHILD = """
import sys
import numpy as np
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
from openpano_amd import hip
from openpano_amd.config import PanoConfig
import match_cases as mc
assert hip.LIB_PATH == %(lib)r, hip.LIB_PATH
cfg = PanoConfig()
ctx = hip.Context(0)
out = {}
for k, case in enumerate(mc.cap_calls()):
    f = hip.Features.from_host(ctx, case.sets)
    before = hip.pool_stats()[0]
    try:
        got = hip.match_pairs(ctx, cfg, f, case.pairs)
        out["n%%d" %% k] = np.array([len(g) for g in got])
        out["l%%d" %% k] = np.concatenate(got + [np.zeros((0, 2), np.int32)])
        out["e%%d" %% k] = np.array("")
    except hip.OpenPanoHipError as e:
        out["e%%d" %% k] = np.array(str(e))
    out["b%%d" %% k] = np.array([before, hip.pool_stats()[0]])
    out["q%%d" %% k] = np.array(ctx.match_last_slow())
    f.free()
ctx.close()
np.savez(%(fout)r, **out)
"""


def test_queue_cap_refuses_and_recovers(cfg, oracle, tmp_path):
    """match.hip rebuilt with a queue cap of 64 rows, in a process of its own: a call that queues 65 forward rows is refused
    with OP_ERR_CAPACITY and its counts, a call that queues 64 and 64 is served, 65 reverse rows are refused, and an ordinary
    call on the same context is served again; a refused call leaves no pool block behind.  (An over-full queue is counted,
    never written: the store is guarded by slot < slow_cap, the scans clamp their count to the cap.)"""
    lib = variant_lib.build_variant(tmp_path, "match", ["-DOP_MATCH_SLOW_CAP=%d" % mc.SLOW_CAP_VARIANT])
    fout = str(tmp_path / "out.npz")
    code = CHILD % dict(root=variant_lib.ROOT, tests=os.path.join(variant_lib.ROOT, "tests"), lib=lib, fout=fout)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, OPENPANO_HIP_LIB=lib), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    z = np.load(fout)
    for k, case in enumerate(mc.cap_calls()):
        err = str(z["e%d" % k])
        assert tuple(z["q%d" % k]) == case.queue, "%s missed its seam: queued %r, built for %r" % (case.name, tuple(z["q%d" % k]), case.queue)
        if max(case.queue) > mc.SLOW_CAP_VARIANT:
            assert "error -3:" in err and "exact-scan queue overflow (65 rows > 64)" in err, (case.name, err)
            assert z["b%d" % k][0] == z["b%d" % k][1], (case.name, z["b%d" % k])
        else:
            assert err == "", (case.name, err)
            ends = np.cumsum(z["n%d" % k])
            assert_lists(case, np.split(z["l%d" % k], ends[:-1]), mc.oracle_lists(oracle, case))
