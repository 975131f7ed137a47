"""CPU: op_gain_solve -- the host solve of exposure (gain) compensation (Brown & Lowe, IJCV 2007, section 6) -- against a
numpy restatement of its normal equations, and the argument checks of the three gain entry points that need no device.

The gains come back as float32: the check is that each one is the float32 rounding of a value within 1e-12 (relative)
of numpy's fp64 solution."""
import ctypes as C

import numpy as np
import pytest

from openpano_amd import hip

FIX = 2.0 ** 32
SN, SG = 10.0 / 255.0, 0.1


def _np_gains(n, count, sums, sigma_n=SN, sigma_g=SG, per_channel=True):
    """the normal equations of e = 1/2 sum_a sum_{b!=a} N_ab [(g_a I_ab - g_b I_ba)^2 / sn^2 + (1 - g_a)^2 / sg^2]"""
    out = np.ones((n, 3))
    for ch in range(3 if per_channel else 1):
        A = np.zeros((n, n)); rhs = np.zeros(n)
        for a in range(n):
            for b in range(a + 1, n):
                p = hip.pair_index(n, a, b)
                N = float(count[p])
                if N <= 0:
                    continue
                S = sums[p]
                if per_channel:
                    Iab, Iba = S[ch] / (FIX * N), S[3 + ch] / (FIX * N)
                else:
                    Iab, Iba = (float(S[0] + S[1] + S[2]) / 3.0) / (FIX * N), (float(S[3] + S[4] + S[5]) / 3.0) / (FIX * N)
                A[a, a] += N * (2 * Iab * Iab / sigma_n ** 2 + 1 / sigma_g ** 2)
                A[b, b] += N * (2 * Iba * Iba / sigma_n ** 2 + 1 / sigma_g ** 2)
                A[a, b] -= N * 2 * Iab * Iba / sigma_n ** 2
                A[b, a] -= N * 2 * Iab * Iba / sigma_n ** 2
                rhs[a] += N / sigma_g ** 2
                rhs[b] += N / sigma_g ** 2
        act = np.flatnonzero(np.diag(A) > 0)
        g = np.ones(n)
        if len(act):
            g[act] = np.linalg.solve(A[np.ix_(act, act)], rhs[act])
        if per_channel:
            out[:, ch] = g
        else:
            out[:] = g[:, None]
    return out


def _assert_f32_of(got, want):
    want = np.asarray(want, np.float64)
    half_ulp = np.spacing(want.astype(np.float32)).astype(np.float64) / 2
    err = np.abs(got.astype(np.float64) - want)
    assert np.all(err <= half_ulp + 1e-12 * np.abs(want)), float((err - half_ulp).max())


def _random_graph(n, seed, isolated=()):
    rng = np.random.default_rng(seed)
    P = n * (n - 1) // 2
    count = np.zeros(P, np.int64); sums = np.zeros((P, 6), np.int64)
    live = [k for k in range(n) if k not in isolated]
    edges = set(zip(live[:-1], live[1:]))                   # a chain keeps the graph connected
    for _ in range(2 * n):
        a, b = sorted(rng.choice(live, 2, replace=False))
        edges.add((int(a), int(b)))
    expo = rng.uniform(0.6, 1.0, (n, 3))
    for a, b in edges:
        p = hip.pair_index(n, a, b)
        N = int(rng.integers(1, 200000))
        base = rng.uniform(0.1, 0.9, 3)
        count[p] = N
        sums[p, :3] = np.rint(base * expo[a] * N * FIX).astype(np.int64)
        sums[p, 3:] = np.rint(base * expo[b] * N * FIX * rng.uniform(0.98, 1.02)).astype(np.int64)
    return count, sums


def test_two_images_closed_form():
    N = 12345
    Iab, Iba = np.array([0.5, 0.31, 0.7]), np.array([0.4, 0.35, 0.5])
    count = np.array([N], np.int64)
    sums = np.rint(np.concatenate([Iab, Iba]) * N * FIX).astype(np.int64)[None, :]
    got = hip.gain_solve(2, count, sums)
    want = np.zeros((2, 3))
    for c in range(3):
        ia, ib = sums[0, c] / (FIX * N), sums[0, 3 + c] / (FIX * N)
        # per image a: (2 ia^2/sn^2 + 1/sg^2) g_a - (2 ia ib/sn^2) g_b = 1/sg^2 (N cancels)
        a11, a22, a12 = 2 * ia * ia / SN ** 2 + 1 / SG ** 2, 2 * ib * ib / SN ** 2 + 1 / SG ** 2, -2 * ia * ib / SN ** 2
        r = 1 / SG ** 2
        det = a11 * a22 - a12 * a12
        want[0, c] = (r * a22 - a12 * r) / det
        want[1, c] = (a11 * r - a12 * r) / det
    _assert_f32_of(got, want)
    _assert_f32_of(got, _np_gains(2, count, sums))
    # the darker image is brightened, the brighter one dimmed
    assert got[0, 0] < 1 < got[1, 0]


@pytest.mark.parametrize("n,seed", [(3, 1), (7, 2), (20, 3), (64, 4), (65, 5), (128, 6)])
@pytest.mark.parametrize("per_channel", [True, False])
def test_random_graphs_equal_normal_equations(n, seed, per_channel):
    count, sums = _random_graph(n, seed)
    got = hip.gain_solve(n, count, sums, per_channel=per_channel)
    _assert_f32_of(got, _np_gains(n, count, sums, per_channel=per_channel))
    if not per_channel:
        assert np.array_equal(got[:, 0], got[:, 1]) and np.array_equal(got[:, 0], got[:, 2])


@pytest.mark.parametrize("per_channel", [True, False])
def test_isolated_images_keep_gain_one(per_channel):
    n = 12
    iso = (0, 5, 11)
    count, sums = _random_graph(n, 9, isolated=iso)
    got = hip.gain_solve(n, count, sums, per_channel=per_channel)
    assert np.all(got[list(iso)] == 1.0)
    _assert_f32_of(got, _np_gains(n, count, sums, per_channel=per_channel))
    # no overlap anywhere: all ones; a single image: one
    assert np.all(hip.gain_solve(4, np.zeros(6, np.int64), np.zeros((6, 6), np.int64)) == 1.0)
    assert np.all(hip.gain_solve(1, np.zeros(0, np.int64), np.zeros((0, 6), np.int64)) == 1.0)


def test_sigmas_are_honoured():
    count, sums = _random_graph(9, 13)
    for sn, sg in ((0.01, 0.05), (0.2, 1.0)):
        got = hip.gain_solve(9, count, sums, sigma_n=sn, sigma_g=sg)
        _assert_f32_of(got, _np_gains(9, count, sums, sigma_n=sn, sigma_g=sg))


def test_gain_entry_points_reject_bad_arguments():
    L = hip.lib()
    n = 3
    count = np.ones(3, np.int64); sums = np.full((3, 6), 1 << 31, np.int64); gains = np.zeros((n, 3), np.float32)
    cp, sp, gp = (a.ctypes.data_as(C.c_void_p) for a in (count, sums, gains))
    bad = [
        (0, cp, sp, SN, SG, 1, gp), (-1, cp, sp, SN, SG, 1, gp),
        (n, None, sp, SN, SG, 1, gp), (n, cp, None, SN, SG, 1, gp), (n, cp, sp, SN, SG, 1, None),
        (n, cp, sp, 0.0, SG, 1, gp), (n, cp, sp, SN, -0.1, 1, gp), (n, cp, sp, float("nan"), SG, 1, gp),
        (n, cp, sp, SN, float("inf"), 1, gp), (n, cp, sp, SN, SG, 2, gp),
    ]
    for args in bad:
        assert L.op_gain_solve(*args) == -1, args
        assert L.op_last_error().decode().startswith("op_gain_solve")
    count[1] = -5
    assert L.op_gain_solve(n, cp, sp, SN, SG, 1, gp) == -1
    assert b"negative" in L.op_last_error()
    # the device entry points check their pointers before touching a device
    out = C.c_void_p()
    assert L.op_gain_overlap(None, None, None, None, n, 1, cp, sp) == -1
    assert b"op_gain_overlap" in L.op_last_error()
    assert L.op_blend_gains(None, None, None, None, n, gp, C.byref(out)) == -1
    assert b"op_blend_gains" in L.op_last_error()
    with pytest.raises(ValueError):
        hip.gain_solve(4, count, sums)
