"""CPU model of the matcher's ranking keys (openpano_amd/csrc/match.hip): two-term bf16 split of both operands, the three
bf16 x bf16 products per element accumulated in fp32 from -|y|^2 / 2, four low mantissa bits given to the slot index.
DESIGN.md section 1.8 bounds the distance of such a key from the true score x.y - |y|^2 / 2 by e = 3.3e-5 (|x|^2 + |y|^2)
and builds the re-score margin E = 8.2e-5 (|x|^2 + max |y|^2) on it.  This test measures that distance on RootSIFT-like
and on adversarial descriptor sets (near-duplicates, sparse, saturated) in numpy -- the bound is about the arithmetic,
not about the hardware; what the hardware does with it is checked by the whole-job GPU tests."""
import numpy as np


def _bf16(v):
    """round-to-nearest-even to bfloat16, returned as float32"""
    u = np.ascontiguousarray(v, np.float32).view(np.uint32)
    r = ((u >> np.uint32(16)) & np.uint32(1)) + np.uint32(0x7FFF)
    return ((u + r) & np.uint32(0xFFFF0000)).view(np.float32)


def _keys(x, y, order):
    xh = _bf16(x); xl = _bf16(x - xh)
    yh = _bf16(y); yl = _bf16(y - yh)
    ny = np.zeros(len(y), np.float32)
    for k in range(128):
        ny = (ny + y[:, k] * y[:, k]).astype(np.float32)
    acc = (-(ny * np.float32(0.5))).astype(np.float32)
    for k in order:                                    # any order: the bound does not depend on it
        for a, b in ((xh, yh), (xh, yl), (xl, yh)):
            acc = (acc + (a[:, k] * b[:, k]).astype(np.float32)).astype(np.float32)      # bf16 x bf16 is exact in fp32
    key = (acc.view(np.uint32) & np.uint32(0xFFFFFFF0)).view(np.float32)                # slot bits
    return key


def _rootsift(rng, n, sparsity):
    h = rng.gamma(0.6, 1.0, (n, 128)) * (rng.random((n, 128)) > sparsity)
    h[:, 0] += 1e-3
    return (np.sqrt(h / h.sum(axis=1, keepdims=True)) * 512).astype(np.float32)


def test_key_error_stays_inside_the_budget():
    rng = np.random.default_rng(5)
    worst = 0.0
    for sparsity in (0.0, 0.5, 0.9):
        x = _rootsift(rng, 4000, sparsity); y = _rootsift(rng, 4000, sparsity)
        cases = [(x, y), (x, x.copy()), (x, (x * np.float32(1.0009765625)).astype(np.float32)), (x, y[::-1].copy())]
        for a, b in cases:
            for order in (range(128), range(127, -1, -1), rng.permutation(128)):
                key = _keys(a, b, order).astype(np.float64)
                a64, b64 = a.astype(np.float64), b.astype(np.float64)
                true = (a64 * b64).sum(axis=1) - 0.5 * (b64 * b64).sum(axis=1)
                scale = (a64 * a64).sum(axis=1) + (b64 * b64).sum(axis=1)
                worst = max(worst, float(np.max(np.abs(key - true) / scale)))
    assert worst <= 3.3e-5, worst
    assert worst > 1e-7                                  # the model really rounds


def _key_matrix(x, y):
    """_keys for every row of x against every row of y"""
    xh = _bf16(x); xl = _bf16(x - xh)
    yh = _bf16(y); yl = _bf16(y - yh)
    ny = np.zeros(len(y), np.float32)
    for k in range(128):
        ny = (ny + y[:, k] * y[:, k]).astype(np.float32)
    acc = np.repeat((-(ny * np.float32(0.5))).astype(np.float32)[None], len(x), 0)
    for k in range(128):
        for a, b in ((xh, yh), (xh, yl), (xl, yh)):
            acc = (acc + (a[:, k, None] * b[None, :, k]).astype(np.float32)).astype(np.float32)
    return (acc.view(np.uint32) & np.uint32(0xFFFFFFF0)).view(np.float32)


def test_a_margin_from_the_rows_own_norm_loses_candidates():
    """E uses the largest norm of the CALL, not the row's: the key error goes with |y|^2.  On the small-norm rows against
    large-norm columns that tests/test_gpu_match_ransac_config.py::test_one_call_mixing_magnitudes matches on the device,
    the shipped margin keeps the exact best and second best of every row among the candidates (keys within E of the
    second-largest key); 8.2e-5 * 2 |x|^2 drops one of them for several rows -- so that test can tell the two apart."""
    from test_gpu_match_ransac_config import MARGIN, _tight_ties
    x, y = _tight_ties()
    key = _key_matrix(x, y).astype(np.float64)
    x64, y64 = x.astype(np.float64), y.astype(np.float64)
    dist = (x64 ** 2).sum(1)[:, None] + (y64 ** 2).sum(1)[None] - 2 * x64 @ y64.T
    nx, gmax = (x64 ** 2).sum(1), float((y64 ** 2).sum(1).max())
    lost = {}
    for name, E in (("call", MARGIN * (nx + gmax)), ("row", MARGIN * 2 * nx)):
        n = 0
        for r in range(len(x)):
            kept = key[r] >= np.sort(key[r])[-2] - E[r]
            n += not kept[np.argsort(dist[r], kind="stable")[:2]].all()
        lost[name] = n
    assert lost["call"] == 0 and lost["row"] >= 5, lost
