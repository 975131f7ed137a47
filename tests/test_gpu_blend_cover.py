"""GPU: the blend's image-cover walk (csrc/blend_sample.hpp: tile_cover / walk_cover, under k_blend_linear, k_mb_first_fused
and k_mb_bands of csrc/blend.hip) past 64, 256 and 4096 views, against the C oracle, bit for bit.

Every case of tests/blend_cover_cases.py: the permuted grid at 64 ... 4200 views (second ballot word, second pass of the
marking loop, both arms of the round bound, a second round with the accumulators carried into it, duplicated placements
whose equal weights leave the order to decide), ROI borders at, one short of and one past the tile boundaries with and
without LAZY_READ, and the gain tables, the vignette row and the byte sampler at large image index.  What each case reaches
and which one-line slip it would show is proved without a device in test_blend_cover_cases_cpu.py.

The views go in as host arrays, 4200 of them in the largest calls: op_blend uploads each (the device-input path is
test_gpu_blend.py's)."""
import time

import numpy as np
import pytest

import blend_cover_cases as bc
from openpano_amd import hip

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.close()


def _compare(got, want, what):
    assert got.shape == want.shape, what
    if not np.array_equal(got, want):
        no_g, no_w = got[..., 0] < 0, want[..., 0] < 0
        both = ~(no_g | no_w)
        diff = np.abs(got[both] - want[both])
        raise AssertionError("%s: canvas differs: mask flips %d, max |d| %g, unequal pixels %d"
                             % (what, int((no_g != no_w).sum()), float(diff.max()) if diff.size else 0.0, int((diff != 0).sum())))


@pytest.mark.parametrize("name", [c.name for c in bc.CASES])
def test_case_equals_oracle(ctx, oracle, name):
    case = bc.CASE[name]
    views, twins, homos, idx = case.scene()
    gk = case.gain_args()
    t0 = time.perf_counter()
    want, _ = oracle.blend(twins, homos, 0, idx, case.cfg, **gk)
    t1 = time.perf_counter()
    cv = hip.blend(ctx, case.cfg, views, homos, 0, idx, **gk)
    got = cv.numpy(); cv.free()
    t2 = time.perf_counter()
    print("%s: %d views, canvas %d x %d, oracle %.2f s, device call %.2f s" % (name, len(views), want.shape[0], want.shape[1], t1 - t0, t2 - t1))
    assert (want >= 0).mean() > 0.5
    if gk and case.mode == "linear":         # the table is read: the gained canvas is not the plain one
        plain, _ = oracle.blend(twins, homos, 0, idx, case.cfg)
        assert plain.shape == want.shape and not np.array_equal(plain, want)
    _compare(got, want, name)

