"""GPU: the inputs of tests/keypoint_cases.py through the HIP path, bit for bit against the C oracle (NaN descriptor elements by
position): off-diagonal pivots and rank-deficient Hessians in k_refine, candidates that move and leave, identical keypoints in
the rank sort, keypoints without a peak in k_orient_peaks / k_expand_oriented, bin 8 and weightless windows in k_descriptor.
test_keypoint_cases_cpu.py shows on the oracle alone that each case reaches what it is here for."""
import numpy as np
import pytest

import keypoint_cases as kc
import sift_cases as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def want():
    """(case or image name, config name) -> the oracle's (desc, coor), computed on first use and left unchanged"""
    from checkers import Oracle
    cache = {}

    def get(img_name, img, cfg_name, cfg):
        key = (img_name, cfg_name)
        if key not in cache:
            cache[key] = Oracle(cfg).detect_feature(img)
        return cache[key]
    return get


def _batch_equals(ctx, cfg, cfg_name, named, want):
    """one hip.sift_batch of the named images: every image's features are the oracle's of that image alone"""
    from openpano_amd import hip
    f = hip.sift_batch(ctx, cfg, [im for _, im in named])
    try:
        counts = []
        for i, (nm, im) in enumerate(named):
            d, c = f.get(i)
            od, oc = want(nm, im, cfg_name, cfg)
            assert kc.same(d, od) and np.array_equal(c, oc), (cfg_name, [n for n, _ in named], i, nm, len(d), len(od))
            counts.append(len(d))
        return counts
    finally:
        f.free()


@pytest.mark.parametrize("name", kc.NAMES)
def test_staged_case_equals_oracle(name):
    """every plane, list and descriptor of the case on a fresh context (S0 and S241 hold more raw extrema than the lists of a
    fresh context: the group runs again with grown lists)"""
    from checkers import Oracle
    from openpano_amd import hip
    img, cfg = kc.case(name)
    o = Oracle(cfg).sift_stages(img)
    ctx = hip.Context(0)
    try:
        g = hip.sift_staged(ctx, cfg, img)
    finally:
        ctx.close()
    assert len(g.desc) == len(o.desc) and len(g.refined["ints"]) == len(o.refined["ints"])
    kc.compare_stages(g, o, cfg)
    if name == "Z":
        assert len(g.desc) > 0 and np.isnan(g.desc).all()


def test_nan_descriptors_match_nothing(want):
    """case Z's descriptors, as the device made them, through the device matcher against themselves and against N's: every
    list is empty, as the exact matcher's"""
    from checkers import Oracle
    from openpano_amd import hip
    zimg, zcfg = kc.case("Z")
    nimg, ncfg = kc.case("N")
    ctx = hip.Context(0)
    try:
        fz = hip.sift_batch(ctx, zcfg, [zimg]); zd, zc = fz.get(0); fz.free()
        fn = hip.sift_batch(ctx, ncfg, [nimg]); nd, nc = fn.get(0); fn.free()
        assert len(zd) > 1000 and np.isnan(zd).all() and len(nd) > 5000 and not np.isnan(nd).any()
        feats = hip.Features.from_host(ctx, [zd, zd, nd], [zc, zc, nc])
        pairs = [(0, 1), (0, 2), (2, 0)]
        got = hip.match_pairs(ctx, ncfg, feats, pairs)
        feats.free()
    finally:
        ctx.close()
    descs = [zd, zd, nd]
    orc = Oracle(ncfg)
    for (i, j), m in zip(pairs, got):
        assert len(m) == 0 and np.array_equal(m.reshape(-1, 2), orc.match_exact(descs[i], descs[j]).reshape(-1, 2)), (i, j)


@pytest.mark.parametrize("cfg_name", ["N", "O"])
def test_features_do_not_depend_on_the_neighbours_in_a_batch(want, cfg_name):
    """N's image (which is O's too), S's and another dense one beside plain sparse() images of both sizes in one call (two size
    groups), under N's config and under O's, then the same images in reversed order on the same context.  Under O's config
    nearly every keypoint is without a peak: k_expand_oriented's per-image offsets stand behind images whose counts are
    nearly zero."""
    from openpano_amd import hip
    _, (h, w), kv = kc.CASES[cfg_name]
    named = [("N", kc.case("N")[0]), ("sparse241", sc.sparse(kc.H, kc.W, 4)), ("S", kc.case("S")[0]),
             ("sparse121", sc.sparse(121, 241, 6)), ("dense2", sc.dense(kc.H, kc.W, 2))]
    # one config per call, with the working size of the larger images: the smaller ones are scaled up (resize ratio 722 / 362)
    cfg = sc.cfg_for(h, w, **kv)
    ctx = hip.Context(0)
    try:
        counts = _batch_equals(ctx, cfg, cfg_name, named, want)
        back = _batch_equals(ctx, cfg, cfg_name, named[::-1], want)
    finally:
        ctx.close()
    assert back == counts[::-1]
    if cfg_name == "N":
        assert counts[0] > 5000 and 30 < counts[1] < 2000 and counts[2] > 500
    else:
        assert counts[0] < 50 and counts[4] < 50 and max(counts) >= 1


def test_case_n_through_the_rerun_with_grown_lists(want):
    """N on a fresh context whose raw / refined lists hold 64 entries: the first attempt clamps, the group runs again with
    lists for its eleven thousand raw candidates"""
    from openpano_amd import hip
    img, cfg = kc.case("N")
    ctx = hip.Context(0)
    try:
        ctx.set_raw_capacity(64)
        assert _batch_equals(ctx, cfg, "N", [("N", img)], want)[0] > 5000
        _batch_equals(ctx, cfg, "N", [("N", img)], want)                      # and again on the grown lists
    finally:
        ctx.close()


def test_all_candidates_and_no_keypoint_between_two_full_images(want):
    """S0 -- thirty thousand raw candidates, every one rejected -- between two N images in one batch"""
    from openpano_amd import hip
    img, cfg = kc.case("N")
    s0, cfg0 = kc.case("S0")
    assert cfg0.raw_items() == cfg.raw_items()
    ctx = hip.Context(0)
    try:
        counts = _batch_equals(ctx, cfg, "N", [("N", img), ("S0", s0), ("N", img)], want)
    finally:
        ctx.close()
    assert counts[1] == 0 and counts[0] == counts[2] > 5000
