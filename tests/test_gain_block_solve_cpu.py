"""CPU: op_gain_block_solve -- the host solve of block gain compensation -- against a numpy restatement of its normal
equations (data term over unit pairs, smoothness over 4-neighbour blocks), its exact reduction to op_gain_solve at 1 x 1,
and the argument and cap checks of the three block-gain entry points that need no device.

The gains come back as float32: each must be the float32 rounding of a value within 1e-12 (relative) of numpy's fp64
solution."""
import ctypes as C

import numpy as np
import pytest

from openpano_amd import hip

FIX = 2.0 ** 32
SN, SG, SS = 10.0 / 255.0, 0.1, 0.1


def _np_block_gains(n, bx, by, count, sums, sigma_n=SN, sigma_g=SG, sigma_s=SS, per_channel=True):
    """the normal equations of
    e = 1/2 sum_{ordered unit pairs} N [(g_{a,qa} I - g_{b,qb} I')^2 / sn^2 + (1 - g_{a,qa})^2 / sg^2]
      + 1/2 sum_k sum_{ordered 4-neighbours q ~ q'} (M_k / B) (g_{k,q} - g_{k,q'})^2 / ss^2"""
    B = bx * by
    count = np.asarray(count).reshape(-1, B, B)
    sums = np.asarray(sums).reshape(-1, B, B, 6)
    M = np.zeros(n)
    for a in range(n):
        for b in range(a + 1, n):
            N = count[hip.pair_index(n, a, b)].sum()
            M[a] += N; M[b] += N
    act = [k for k in range(n) if M[k] > 0]
    out = np.ones((n, B, 3))
    for ch in range(3 if per_channel else 1):
        A = np.zeros((n * B, n * B)); rhs = np.zeros(n * B)
        for a in range(n):
            for b in range(a + 1, n):
                p = hip.pair_index(n, a, b)
                for qa in range(B):
                    for qb in range(B):
                        N = float(count[p, qa, qb])
                        if N <= 0:
                            continue
                        S = sums[p, qa, qb]
                        if per_channel:
                            Iab, Iba = S[ch] / (FIX * N), S[3 + ch] / (FIX * N)
                        else:
                            Iab = (float(S[0] + S[1] + S[2]) / 3.0) / (FIX * N)
                            Iba = (float(S[3] + S[4] + S[5]) / 3.0) / (FIX * N)
                        i, j = a * B + qa, b * B + qb
                        A[i, i] += N * (2 * Iab * Iab / sigma_n ** 2 + 1 / sigma_g ** 2)
                        A[j, j] += N * (2 * Iba * Iba / sigma_n ** 2 + 1 / sigma_g ** 2)
                        A[i, j] -= N * 2 * Iab * Iba / sigma_n ** 2
                        A[j, i] -= N * 2 * Iab * Iba / sigma_n ** 2
                        rhs[i] += N / sigma_g ** 2
                        rhs[j] += N / sigma_g ** 2
        for k in act:
            w = 2 * (M[k] / B) / sigma_s ** 2
            for v in range(by):
                for u in range(bx):
                    q = k * B + v * bx + u
                    for q2 in ([q + 1] if u + 1 < bx else []) + ([q + bx] if v + 1 < by else []):
                        A[q, q] += w; A[q2, q2] += w; A[q, q2] -= w; A[q2, q] -= w
        idx = np.concatenate([np.arange(k * B, (k + 1) * B) for k in act]) if act else np.zeros(0, int)
        g = np.ones(n * B)
        if len(idx):
            g[idx] = np.linalg.solve(A[np.ix_(idx, idx)], rhs[idx])
        if per_channel:
            out[:, :, ch] = g.reshape(n, B)
        else:
            out[:] = g.reshape(n, B)[:, :, None]
    return out.reshape(n, by, bx, 3)


def _assert_f32_of(got, want):
    want = np.asarray(want, np.float64)
    half_ulp = np.spacing(want.astype(np.float32)).astype(np.float64) / 2
    err = np.abs(got.astype(np.float64) - want)
    assert np.all(err <= half_ulp + 1e-12 * np.abs(want)), float((err - half_ulp).max())


def _random_block_stats(n, bx, by, seed, isolated=(), empty_blocks=()):
    """unit-pair statistics of images with a smooth brightness field each: a connected graph of overlapping pairs, every
    pair touching a random subset of block pairs; `empty_blocks` (q) of every image overlap nothing"""
    rng = np.random.default_rng(seed)
    B = bx * by
    P = n * (n - 1) // 2
    count = np.zeros((P, B, B), np.int64); sums = np.zeros((P, B, B, 6), np.int64)
    live = [k for k in range(n) if k not in isolated]
    edges = set(zip(live[:-1], live[1:]))
    for _ in range(2 * n):
        if len(live) >= 2:
            a, b = sorted(rng.choice(live, 2, replace=False))
            edges.add((int(a), int(b)))
    field = rng.uniform(0.6, 1.0, (n, B, 3))
    ok = [q for q in range(B) if q not in empty_blocks]
    for a, b in edges:
        p = hip.pair_index(n, a, b)
        for _ in range(max(2, B)):
            qa, qb = int(rng.choice(ok)), int(rng.choice(ok))
            N = int(rng.integers(1, 50000))
            base = rng.uniform(0.1, 0.9, 3)
            count[p, qa, qb] += N
            sums[p, qa, qb, :3] += np.rint(base * field[a, qa] * N * FIX).astype(np.int64)
            sums[p, qa, qb, 3:] += np.rint(base * field[b, qb] * N * FIX * rng.uniform(0.98, 1.02)).astype(np.int64)
    return count, sums


@pytest.mark.parametrize("n,bx,by,seed", [(2, 2, 2, 1), (5, 4, 4, 2), (7, 3, 2, 3), (12, 1, 3, 4), (20, 4, 4, 5)])
@pytest.mark.parametrize("per_channel", [True, False])
def test_block_solve_equals_normal_equations(n, bx, by, seed, per_channel):
    count, sums = _random_block_stats(n, bx, by, seed)
    got = hip.gain_block_solve(n, bx, by, count, sums, per_channel=per_channel)
    assert got.shape == (n, by, bx, 3) and got.dtype == np.float32
    want = _np_block_gains(n, bx, by, count, sums, per_channel=per_channel)
    _assert_f32_of(got, want)
    if not per_channel:
        assert np.array_equal(got[..., 0], got[..., 1]) and np.array_equal(got[..., 0], got[..., 2])
    # the blocks differ: a block gain is not an image gain
    assert np.ptp(got[..., 0].reshape(n, -1), axis=1).max() > 1e-3


@pytest.mark.parametrize("per_channel", [True, False])
def test_isolated_images_and_empty_blocks(per_channel):
    """an image without overlap keeps 1 everywhere; blocks that overlap nothing are solved through the smoothness term
    (finite, not 1, and between their neighbours' range)"""
    n, bx, by = 9, 4, 4
    iso = (0, 6)
    centre = (5, 6, 9, 10)
    count, sums = _random_block_stats(n, bx, by, 21, isolated=iso, empty_blocks=centre)
    got = hip.gain_block_solve(n, bx, by, count, sums, per_channel=per_channel)
    assert np.all(got[list(iso)] == 1.0)
    _assert_f32_of(got, _np_block_gains(n, bx, by, count, sums, per_channel=per_channel))
    live = [k for k in range(n) if k not in iso]
    g = got[live].reshape(len(live), bx * by, 3)
    inner, outer = g[:, list(centre)], np.delete(g, list(centre), axis=1)
    assert np.all(np.isfinite(inner)) and np.all(inner != 1.0)
    assert np.all(inner >= outer.min(axis=1, keepdims=True) - 1e-6) and np.all(inner <= outer.max(axis=1, keepdims=True) + 1e-6)
    # no overlap anywhere: all ones; a single image: ones
    assert np.all(hip.gain_block_solve(4, 2, 2, np.zeros((6, 4, 4), np.int64), np.zeros((6, 4, 4, 6), np.int64)) == 1.0)
    assert np.all(hip.gain_block_solve(1, 3, 2, np.zeros(0, np.int64), np.zeros(0, np.int64)) == 1.0)


@pytest.mark.parametrize("n,seed", [(2, 1), (7, 2), (20, 3), (65, 5), (128, 6)])
@pytest.mark.parametrize("per_channel", [True, False])
def test_one_by_one_is_op_gain_solve_bit_for_bit(n, seed, per_channel):
    rng = np.random.default_rng(seed)
    P = n * (n - 1) // 2
    count = np.where(rng.uniform(size=P) < 0.3, rng.integers(1, 300000, P), 0).astype(np.int64)
    count[[hip.pair_index(n, a, a + 1) for a in range(n - 1)]] += 7
    sums = (rng.uniform(0.05, 0.95, (P, 6)) * count[:, None] * FIX).astype(np.int64)
    want = hip.gain_solve(n, count, sums, per_channel=per_channel)
    for ss in (SS, 1e-3, 1e3):               # no edges at 1 x 1: sigma_s plays no part
        got = hip.gain_block_solve(n, 1, 1, count.reshape(P, 1, 1), sums.reshape(P, 1, 1, 6), sigma_s=ss, per_channel=per_channel)
        assert np.array_equal(got.reshape(n, 3), want)


def test_sigmas_are_honoured():
    count, sums = _random_block_stats(6, 3, 3, 13)
    for sn, sg, ss in ((0.01, 0.05, 0.02), (0.2, 1.0, 1.0)):
        got = hip.gain_block_solve(6, 3, 3, count, sums, sigma_n=sn, sigma_g=sg, sigma_s=ss)
        _assert_f32_of(got, _np_block_gains(6, 3, 3, count, sums, sigma_n=sn, sigma_g=sg, sigma_s=ss))
    # a stiffer smoothness term pulls the blocks of an image together
    loose = hip.gain_block_solve(6, 3, 3, count, sums, sigma_s=1.0)
    stiff = hip.gain_block_solve(6, 3, 3, count, sums, sigma_s=0.001)
    assert np.ptp(stiff.reshape(6, 9, 3), axis=1).max() < 0.1 * np.ptp(loose.reshape(6, 9, 3), axis=1).max()


def test_block_entry_points_reject_bad_arguments():
    L = hip.lib()
    n, bx, by = 3, 2, 2
    count = np.ones((3, 4, 4), np.int64); sums = np.full((3, 4, 4, 6), 1 << 31, np.int64)
    gains = np.zeros((n, by, bx, 3), np.float32)
    cp, sp, gp = (a.ctypes.data_as(C.c_void_p) for a in (count, sums, gains))
    bad = [
        (0, bx, by, cp, sp, SN, SG, SS, 1, gp), (-1, bx, by, cp, sp, SN, SG, SS, 1, gp),
        (n, 0, by, cp, sp, SN, SG, SS, 1, gp), (n, bx, 0, cp, sp, SN, SG, SS, 1, gp),
        (n, 17, by, cp, sp, SN, SG, SS, 1, gp), (n, bx, 17, cp, sp, SN, SG, SS, 1, gp),
        (n, bx, by, None, sp, SN, SG, SS, 1, gp), (n, bx, by, cp, None, SN, SG, SS, 1, gp), (n, bx, by, cp, sp, SN, SG, SS, 1, None),
        (n, bx, by, cp, sp, 0.0, SG, SS, 1, gp), (n, bx, by, cp, sp, SN, -0.1, SS, 1, gp), (n, bx, by, cp, sp, SN, SG, 0.0, 1, gp),
        (n, bx, by, cp, sp, SN, SG, float("nan"), 1, gp), (n, bx, by, cp, sp, SN, SG, float("inf"), 1, gp),
        (n, bx, by, cp, sp, SN, SG, SS, 2, gp),
    ]
    for args in bad:
        assert L.op_gain_block_solve(*args) == -1, args
        assert L.op_last_error().decode().startswith("op_gain_block_solve")
    count[1, 2, 3] = -5
    assert L.op_gain_block_solve(n, bx, by, cp, sp, SN, SG, SS, 1, gp) == -1
    assert b"negative" in L.op_last_error()
    # the dense solve's cap: n * bx * by <= 4096 units (checked before the statistics are read)
    assert L.op_gain_block_solve(17, 16, 16, cp, sp, SN, SG, SS, 1, gp) == -4
    assert b"4096" in L.op_last_error()
    # the device entry points check their arguments before touching a device
    out = C.c_void_p()
    assert L.op_gain_block_overlap(None, None, None, None, n, 1, bx, by, cp, sp) == -1
    assert b"op_gain_block_overlap" in L.op_last_error()
    assert L.op_blend_block_gains(None, None, None, None, n, bx, by, gp, C.byref(out)) == -1
    assert b"op_blend_block_gains" in L.op_last_error()
    with pytest.raises(ValueError):
        hip.gain_block_solve(4, bx, by, count, sums)
