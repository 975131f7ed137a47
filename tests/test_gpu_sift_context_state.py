"""GPU: the state run_group keeps on the context between batches (csrc/sift_host.hip).  The descriptor output is sized from the
previous batch (capK = max(2048 n, 1.25 x its total)) and the last two stages run again when a batch outgrows it; the refine,
sort and peak launches are sized from the previous batch's longest lists, grid-stride loops covering the rest; the raw list
capacity grows and reruns the whole group.  Sequences of batches on one context walk through every such transition -- dense
after sparse after empty, a rerun inside a rerun, two size groups and two chunks in one call -- and every batch's features
equal the oracle's.  Each sequence runs a second time with profiling on, where the call count of a stage label says which path
ran: "sift descriptor" twice when the last two stages were repeated, "build pyramid" twice when the group was rerun.  The
oracle's counts that make these the expected paths are asserted on the CPU (test_sift_cases_cpu.py)."""
import numpy as np
import pytest

import sift_cases as sc

pytestmark = pytest.mark.gpu
MODES = [False, True]
MODE_IDS = ["plain", "profiled"]


@pytest.fixture(scope="module")
def cfg():
    return sc.cfg_for(sc.SEQ_H, sc.SEQ_W)


@pytest.fixture(scope="module")
def images():
    return sc.seq_images()


@pytest.fixture(scope="module")
def want(cfg, images):
    """name -> (desc, centred coordinates, real coordinates in [0, 1)) of the oracle, computed once"""
    from checkers import Oracle
    orc = Oracle(cfg)
    out = {}
    for name, img in images.items():
        d, c = orc.detect_feature(img)
        st = orc.sift_stages(img, planes=False)
        assert np.array_equal(st.desc, d)
        out[name] = (d, c, st.coor)
    return out


def _new_ctx(profiled):
    from openpano_amd import hip
    c = hip.Context(0)
    if profiled:
        c.set_profiling(True)
    return c


def _check(f, names, want):
    assert f.num_images == len(names)
    tot = 0
    for i, name in enumerate(names):
        d, c = f.get(i)
        wd, wc, wr = want[name]
        assert np.array_equal(d, wd) and np.array_equal(c, wc), (i, name, len(d), len(wd))
        assert np.array_equal(f.get_real(i), wr), (i, name)
        assert f.offset(i) == tot, (i, name)
        tot += len(wd)
    assert f.total == tot


def _calls(ctx):
    prof = ctx.profile()
    return prof.get("build pyramid", (0, 0))[1], prof.get("sift descriptor", (0, 0))[1]


def _batch(ctx, cfg, images, want, names, profiled, pyramid=1, descriptor=1, at_least=False):
    """one op_sift_batch of the named images: features against the oracle, and (profiled) the paths taken"""
    from openpano_amd import hip
    if profiled:
        ctx.profile_reset()
    f = hip.sift_batch(ctx, cfg, [images[n] for n in names])
    try:
        _check(f, names, want)
    finally:
        f.free()
    if profiled:
        got = _calls(ctx)
        assert got[0] == pyramid and (got[1] >= descriptor if at_least else got[1] == descriptor), (names, got)


@pytest.mark.parametrize("profiled", MODES, ids=MODE_IDS)
def test_capacity_and_launch_hints_across_batches(cfg, images, want, profiled):
    ctx = _new_ctx(profiled)
    try:
        run = lambda names, descriptor: _batch(ctx, cfg, images, want, names, profiled, descriptor=descriptor)    # noqa: E731
        run(["D1"], 2)                   # fresh context: more than 2048 descriptors, the last two stages run again
        run(["D2", "D3"], 2)             # about twice 1.25 x the last total: the cut falls inside image 1
        run(["F"], 1)                    # no features at all: every hint drops to 0
        run(["D1"], 2)                   # full-size lists on launches sized from zero hints, capK back at its floor
        run(["S"], 1)                    # the hints shrink to a few hundred
        run(["D2", "S", "D3"], 2)        # launches sized for ~100 keypoints against ~4000 per image
        run(["D2", "S", "D3"], 1)        # steady state: the same batch fits its own prediction
    finally:
        ctx.close()


@pytest.mark.parametrize("profiled", MODES, ids=MODE_IDS)
def test_descriptor_rerun_inside_the_raw_capacity_rerun(cfg, images, want, profiled):
    ctx = _new_ctx(profiled)
    try:
        ctx.set_raw_capacity(64)
        # lists of 64 overflow: the group runs again with grown lists, and that second run outgrows capK (still at its floor
        # after the clamped first attempt), so its last two stages run a second time as well
        _batch(ctx, cfg, images, want, ["D1", "S"], profiled, pyramid=2, descriptor=3, at_least=True)
        _batch(ctx, cfg, images, want, ["D1", "S"], profiled)
    finally:
        ctx.close()


@pytest.mark.parametrize("profiled", MODES, ids=MODE_IDS)
def test_two_size_groups_in_one_call(cfg, images, want, profiled):
    """[241 x 481, 240 x 240, 241 x 481, 240 x 240]: two groups run one after the other on the same context state; the second
    outgrows the capacity the first one left.  Offsets and order follow the input order, not the groups'."""
    ctx = _new_ctx(profiled)
    try:
        _batch(ctx, cfg, images, want, ["S", "Q1", "S2", "Q2"], profiled, pyramid=2, descriptor=3)
    finally:
        ctx.close()


@pytest.mark.parametrize("profiled", MODES, ids=MODE_IDS)
def test_pipelined_host_call_reruns_one_chunk_of_two(cfg, images, want, profiled):
    """op_sift_batch_host over 16 stacked images = two chunks of 8 through run_group: the dense chunk outgrows 2048 x 8 and
    repeats its last two stages while the next chunk's upload is in flight, the sparse / flat chunk fits what the first left.
    Resident features and the caller's host buffers both equal the oracle's."""
    from openpano_amd import hip
    names = ["D%d" % (i % 3 + 1) for i in range(8)] + ["S", "F"] * 4
    stack = np.ascontiguousarray(np.stack([images[n] for n in names]))
    total = sum(len(want[n][0]) for n in names)
    hd = np.zeros((total + 8, 128), np.float32); hc = np.zeros((total + 8, 2), np.float64)
    ctx = _new_ctx(profiled)
    try:
        if profiled:
            ctx.profile_reset()
        f = hip.SiftHostCall(ctx, cfg, [stack[i] for i in range(16)], hd.ctypes.data, hc.ctypes.data, total + 8)()
        try:
            _check(f, names, want)
            for i, n in enumerate(names):
                o, k = f.offset(i), len(want[n][0])
                assert np.array_equal(hd[o: o + k], want[n][0]) and np.array_equal(hc[o: o + k], want[n][1]), (i, n)
            assert not hd[total:].any() and not hc[total:].any()
        finally:
            f.free()
        if profiled:
            assert _calls(ctx) == (2, 3)
    finally:
        ctx.close()
