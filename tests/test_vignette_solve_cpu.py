"""CPU: op_vignette_solve -- the host solve of vignetting compensation (gains plus one radial curve shared by all views) --
against an independent numpy restatement of its alternation, its recovery of a known curve and known exposures from
moments of the exact observation model, and the argument checks of the three vignetting entry points that need no device.

The moments are formed here as include/openpano_hip.h states them: rho and the grey level in fp32 from the contract's
expressions, every product in fp64 in the stated order, summed as rint(x * 2^32) in int64."""
import ctypes as C

import numpy as np
import pytest

from openpano_amd import hip

FIX = 2.0 ** 32
SN, SG, SV = 10.0 / 255.0, 1.0, 100.0
MAX_ROUNDS, TOL = 100, 1e-12          # op_vignette_solve's alternation (include/openpano_hip.h)


def rho_of(r, c, w, h):
    """the contract's normalised squared radius, fp32"""
    r = np.asarray(r, np.float32); c = np.asarray(c, np.float32)
    fw, fh = np.float32(w), np.float32(h)
    dx = c - np.float32(0.5) * fw; dy = r - np.float32(0.5) * fh
    return np.minimum((dx * dx + dy * dy) / (np.float32(0.25) * (fw * fw + fh * fh)), np.float32(1))


def moments_of(Ya, ra, Yb, rb):
    """(N, 30 moments) of one pair's samples (fp32 arrays), as k_vignette_overlap forms them"""
    Ya, ra, Yb, rb = (np.asarray(x, np.float32).astype(np.float64) for x in (Ya, ra, Yb, rb))
    aa, bb, ab = Ya * Ya, Yb * Yb, Ya * Yb
    pa, pb = [np.ones_like(ra)], [np.ones_like(rb)]
    for _ in range(6):
        pa.append(pa[-1] * ra); pb.append(pb[-1] * rb)
    terms = [aa * pb[k] for k in range(7)] + [bb * pa[k] for k in range(7)] + [(ab * pa[i]) * pb[j] for i in range(4) for j in range(4)]
    return len(Ya), np.array([np.rint(t * FIX).astype(np.int64).sum() for t in terms], np.int64)


def sweep_moments(n=5, w=220, h=160, pan=130, poly=(-0.3, 0.0, 0.0), seed=0, stride=2):
    """a one-row sweep: view k sees world columns [pan k, pan k + w); every lattice point of an overlap observes
    Y = e_k V(rho) L with L uniform in [0.2, 0.9] and exposures e_k in [0.7, 1].  -> (count, moments, exposures)"""
    rng = np.random.default_rng(seed)
    e = rng.uniform(0.7, 1.0, n)
    a1, a2, a3 = poly
    V = lambda rho: 1.0 + rho * (a1 + rho * (a2 + rho * a3))
    P = n * (n - 1) // 2
    count = np.zeros(P, np.int64); mom = np.zeros((P, 30), np.int64)
    for a in range(n):
        for b in range(a + 1, n):
            x0, x1 = pan * b, pan * a + w
            if x1 <= x0:
                continue
            y, x = np.mgrid[0:h:stride, x0:x1:stride].astype(np.float64)
            y, x = y.ravel() + 0.25, x.ravel() + 0.25
            L = rng.uniform(0.2, 0.9, len(x))
            ra, rb = rho_of(y, x - pan * a, w, h), rho_of(y, x - pan * b, w, h)
            Ya = (e[a] * V(ra.astype(np.float64)) * L).astype(np.float32)
            Yb = (e[b] * V(rb.astype(np.float64)) * L).astype(np.float32)
            p = hip.pair_index(n, a, b)
            count[p], mom[p] = moments_of(Ya, ra, Yb, rb)
    return count, mom, e


def np_vignette_solve(n, count, mom, degree=3, sigma_n=SN, sigma_g=SG, sigma_v=SV):
    """the alternation of op_vignette_solve, written with numpy matrices -> (g (n,), a (3,), rounds)"""
    pairs = [(a, b) for a in range(n) for b in range(a + 1, n) if count[hip.pair_index(n, a, b)] > 0]
    act = sorted({k for ab in pairs for k in ab})
    g, a = np.ones(n), np.array([1.0, 0.0, 0.0, 0.0])
    if not pairs:
        return g, a[1:], 0
    hank = lambda h: np.array([[h[i + j] for j in range(4)] for i in range(4)])
    st = []
    for pa_, pb_ in pairs:
        p = hip.pair_index(n, pa_, pb_)
        m = mom[p].astype(np.float64) / FIX
        st.append((pa_, pb_, float(count[p]), hank(m[:7]), hank(m[7:14]), m[14:].reshape(4, 4)))
    Mtot = sum(s[2] for s in st)

    def energy():
        e = Mtot * (a[1:] @ a[1:]) / sigma_v ** 2
        for i, j, N, HA, HB, Cm in st:
            e += (g[i] ** 2 * (a @ HA @ a) - 2 * g[i] * g[j] * (a @ Cm @ a) + g[j] ** 2 * (a @ HB @ a)) / sigma_n ** 2
            e += N * ((1 - g[i]) ** 2 + (1 - g[j]) ** 2) / sigma_g ** 2
        return e

    e_prev, rounds = energy(), 0
    for rounds in range(1, MAX_ROUNDS + 1):
        A = np.zeros((n, n)); rhs = np.zeros(n)
        for i, j, N, HA, HB, Cm in st:
            A[i, i] += (a @ HA @ a) / sigma_n ** 2 + N / sigma_g ** 2
            A[j, j] += (a @ HB @ a) / sigma_n ** 2 + N / sigma_g ** 2
            A[i, j] -= (a @ Cm @ a) / sigma_n ** 2
            A[j, i] -= (a @ Cm @ a) / sigma_n ** 2
            rhs[i] += N / sigma_g ** 2; rhs[j] += N / sigma_g ** 2
        g[act] = np.linalg.solve(A[np.ix_(act, act)], rhs[act])
        Q = sum(g[i] ** 2 * HA - g[i] * g[j] * (Cm + Cm.T) + g[j] ** 2 * HB for i, j, N, HA, HB, Cm in st) / sigma_n ** 2
        d = degree
        a[1:] = 0.0
        a[1:1 + d] = np.linalg.solve(Q[1:1 + d, 1:1 + d] + np.eye(d) * Mtot / sigma_v ** 2, -Q[1:1 + d, 0])
        e = energy()
        done = not (e_prev - e > TOL * e_prev)
        e_prev = e
        if done:
            break
    s = sum(N * (g[i] + g[j]) for i, j, N, HA, HB, Cm in st) / (2 * Mtot)     # overlap-weighted mean gain 1
    g[act] /= s
    return g, a[1:].copy(), rounds


def curve(poly, rho):
    a1, a2, a3 = (float(x) for x in poly)
    return 1.0 + rho * (a1 + rho * (a2 + rho * a3))


RHO = np.linspace(0.0, 1.0, 101)


def assert_f32_of(got, want, atol=0.0):
    """got (float32) is the float32 rounding of a value within 1e-12 (relative) + atol of want (float64)"""
    want = np.asarray(want, np.float64)
    half_ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64) / 2
    err = np.abs(np.asarray(got).astype(np.float64) - want)
    assert np.all(err <= half_ulp + 1e-12 * np.abs(want) + atol), (got, want)


# The curve step solves a degree x degree system in the moments of rho up to rho^6: a Hankel-like matrix whose condition
# number reaches ~1e6, so two correct fp64 solvers that add in different orders agree on a1..a3 to ~1e-11 absolute, not
# 1e-12 relative.  The coefficients are compared to CURVE_ATOL (1e-9 on a curve of order 1), the gains to 1e-12 relative.
CURVE_ATOL = 1e-9


@pytest.mark.parametrize("seed,poly", [(0, (-0.3, 0.0, 0.0)), (1, (-0.15, -0.2, 0.05)), (2, (0.0, 0.0, 0.0)), (3, (-0.45, 0.1, 0.0))])
@pytest.mark.parametrize("degree", [1, 2, 3])
def test_solve_equals_numpy_alternation(seed, poly, degree):
    n = 5
    count, mom, _ = sweep_moments(n, poly=poly, seed=seed)
    g, p = hip.vignette_solve(n, count, mom, degree)
    assert g.shape == (n, 3) and g.dtype == np.float32 and p.shape == (3,) and p.dtype == np.float32
    assert np.array_equal(g[:, 0], g[:, 1]) and np.array_equal(g[:, 0], g[:, 2])
    wg, wa, rounds = np_vignette_solve(n, count, mom, degree)
    assert rounds >= 2
    assert_f32_of(g[:, 0], wg)
    assert_f32_of(p, wa, CURVE_ATOL)
    assert np.all(p[degree:] == 0.0)                  # the unused coefficients are exactly 0


def test_solve_equals_numpy_on_a_graph_with_gaps():
    """pairs beyond neighbours (a, a + 2 overlaps), an isolated view, and other sigmas"""
    n = 7
    count, mom, _ = sweep_moments(n, pan=90, poly=(-0.25, -0.05, 0.0), seed=9)
    iso = 6
    for b in range(n):
        if b != iso:
            p = hip.pair_index(n, min(b, iso), max(b, iso))
            count[p] = 0; mom[p] = 0
    assert count[hip.pair_index(n, 0, 2)] > 0
    for sn, sg, sv in ((SN, SG, SV), (0.02, 0.5, 1e3), (0.1, 3.0, 10.0)):
        g, p = hip.vignette_solve(n, count, mom, 3, sn, sg, sv)
        wg, wa, _ = np_vignette_solve(n, count, mom, 3, sn, sg, sv)
        assert_f32_of(g[:, 0], wg)
        assert_f32_of(p, wa, CURVE_ATOL)
        assert np.all(g[iso] == 1.0)


@pytest.mark.parametrize("poly", [(-0.3, 0.0, 0.0), (-0.15, -0.2, 0.05), (-0.4, 0.25, -0.1)])
def test_recovery_under_weak_priors(poly):
    """moments of the exact model: weak priors (sigma_g = 10 or 100, sigma_v = 1e3) give back the curve and the exposure
    ratios within 1e-4.  (At sigma_g = 1 Brown & Lowe's prior itself pulls the ratios towards 1 by a few 0.1 %: see
    test_recovery_at_the_defaults.)"""
    n = 5
    count, mom, e = sweep_moments(n, poly=poly, seed=4)
    for sg, sv in ((10.0, 1e3), (100.0, 1e3)):
        g, p = hip.vignette_solve(n, count, mom, 3, SN, sg, sv)
        assert np.abs(curve(p, RHO) - curve(poly, RHO)).max() < 1e-4, (p, poly)
        ratio = (g[:, 0].astype(np.float64) * e) / (g[0, 0] * e[0])     # g_k = c / e_k for one common c
        assert np.abs(ratio - 1).max() < 1e-4, ratio


@pytest.mark.parametrize("seed", [0, 4])
def test_recovery_at_the_defaults(seed):
    """the default priors (sigma_g = 1, sigma_v = 100) on the sweep of DESIGN 10.2's table: a1 within 0.005 of -0.3, the
    higher terms near 0, V within 1e-3 of the truth, exposure ratios within 1 %.  A stiffer curve prior (sigma_v = 10, 1)
    shrinks the coefficients and moves V away from the truth step by step, and a strong gain prior (sigma_g = 0.1) lets the curve absorb the exposures."""
    n = 5
    count, mom, e = sweep_moments(n, poly=(-0.3, 0.0, 0.0), seed=seed)
    verr = lambda p: np.abs(curve(p, RHO) - curve((-0.3, 0, 0), RHO)).max()
    g, p = hip.vignette_solve(n, count, mom)
    print("\ndefaults a =", p, "V err", verr(p), "ratios", (g[:, 0] * e) / (g[0, 0] * e[0]))
    assert abs(p[0] + 0.3) < 5e-3 and np.abs(p[1:]).max() < 5e-3, p
    assert verr(p) < 1e-3
    assert np.abs((g[:, 0] * e) / (g[0, 0] * e[0]) - 1).max() < 1e-2
    _, p10 = hip.vignette_solve(n, count, mom, 3, SN, SG, 10.0)
    _, p1 = hip.vignette_solve(n, count, mom, 3, SN, SG, 1.0)
    print("sigma_v = 10: a =", p10, "sigma_v = 1: a =", p1)
    assert verr(p) < verr(p10) < verr(p1)
    assert np.linalg.norm(p1) < np.linalg.norm(p10) < np.linalg.norm(p)       # the prior shrinks the coefficients
    _, pg = hip.vignette_solve(n, count, mom, 3, SN, 0.1, SV)
    print("sigma_g = 0.1: a =", pg)
    assert verr(pg) > 0.05


def test_gains_keep_the_panorama_brightness():
    """overlaps that disagree with the model (uncorrelated content) pull every gain towards 0 under the weak default gain
    prior; the solve keeps their overlap-weighted mean at 1"""
    n, k = 4, 5000
    rng = np.random.default_rng(8)
    P = n * (n - 1) // 2
    count = np.zeros(P, np.int64); mom = np.zeros((P, 30), np.int64)
    for a in range(n - 1):
        p = hip.pair_index(n, a, a + 1)
        count[p], mom[p] = moments_of(rng.uniform(0.1, 0.9, k), rng.uniform(0, 1, k), rng.uniform(0.1, 0.9, k), rng.uniform(0, 1, k))
    g, p = hip.vignette_solve(n, count, mom)
    wg, wa, _ = np_vignette_solve(n, count, mom)
    assert_f32_of(g[:, 0], wg)
    N = count[[hip.pair_index(n, a, a + 1) for a in range(n - 1)]].astype(np.float64)
    mean = sum(N[a] * (g[a, 0] + g[a + 1, 0]) for a in range(n - 1)) / (2 * N.sum())
    assert abs(mean - 1) < 1e-6, (mean, g[:, 0], p)


@pytest.mark.parametrize("degree", [1, 2])
def test_lower_degrees_zero_the_unused_coefficients(degree):
    n = 5
    count, mom, _ = sweep_moments(n, poly=(-0.2, -0.1, 0.0), seed=5)
    _, p = hip.vignette_solve(n, count, mom, degree)
    assert np.all(p[degree:] == 0.0) and np.all(p[:degree] != 0.0), p


def test_no_overlap():
    n = 4
    g, p = hip.vignette_solve(n, np.zeros(6, np.int64), np.zeros((6, 30), np.int64))
    assert np.all(g == 1.0) and np.all(p == 0.0)
    g, p = hip.vignette_solve(1, np.zeros(0, np.int64), np.zeros((0, 30), np.int64))
    assert np.all(g == 1.0) and np.all(p == 0.0)


@pytest.mark.parametrize("degree", [2, 3])
def test_non_positive_curve_is_refused(degree):
    """statistics whose best curve dips below zero on [0, 1] -- samples that put V(0.5) and V(0.7) at 0 and V(1) at 1, each
    seen from both sides so that the exposures are equal: OP_ERR_UNSUPPORTED, gains 1 and a curve of 0 written"""
    n, k = 2, 3000
    rng = np.random.default_rng(3)
    N, M = 0, np.zeros(30, np.int64)
    for r, t in ((0.5, 0.0), (0.7, 0.0), (1.0, 1.0)):
        L = rng.uniform(0.3, 0.9, k)
        zero, rr = np.zeros(k, np.float32), np.full(k, r, np.float32)
        for Ya, ra, Yb, rb in (((0.8 * L), zero, (0.8 * t * L), rr), ((0.8 * t * L), rr, (0.8 * L), zero)):
            dn, dm = moments_of(Ya.astype(np.float32), ra, Yb.astype(np.float32), rb)
            N += dn; M += dm
    count = np.array([N], np.int64); mom = M.reshape(1, 30)
    L_ = hip.lib()
    gains = np.zeros((n, 3), np.float32); poly = np.full(3, 7.0, np.float32)
    rc = L_.op_vignette_solve(n, count.ctypes.data_as(C.c_void_p), mom.ctypes.data_as(C.c_void_p), degree, SN, SG, 1e4,
                              gains.ctypes.data_as(C.c_void_p), poly.ctypes.data_as(C.c_void_p))
    assert rc == -4, (rc, poly)
    assert b"not positive" in L_.op_last_error()
    assert np.all(gains == 1.0) and np.all(poly == 0.0)
    with pytest.raises(hip.OpenPanoHipError):
        hip.vignette_solve(n, count, mom, degree, SN, SG, 1e4)


def test_entry_points_reject_bad_arguments():
    L = hip.lib()
    n = 3
    count = np.ones(3, np.int64); mom = np.full((3, 30), 1 << 31, np.int64)
    gains = np.zeros((n, 3), np.float32); poly = np.zeros(3, np.float32)
    cp, mp, gp, pp = (a.ctypes.data_as(C.c_void_p) for a in (count, mom, gains, poly))
    bad = [
        (0, cp, mp, 3, SN, SG, SV, gp, pp), (-1, cp, mp, 3, SN, SG, SV, gp, pp),
        (n, None, mp, 3, SN, SG, SV, gp, pp), (n, cp, None, 3, SN, SG, SV, gp, pp),
        (n, cp, mp, 3, SN, SG, SV, None, pp), (n, cp, mp, 3, SN, SG, SV, gp, None),
        (n, cp, mp, 0, SN, SG, SV, gp, pp), (n, cp, mp, 4, SN, SG, SV, gp, pp),
        (n, cp, mp, 3, 0.0, SG, SV, gp, pp), (n, cp, mp, 3, SN, -1.0, SV, gp, pp), (n, cp, mp, 3, SN, SG, 0.0, gp, pp),
        (n, cp, mp, 3, float("nan"), SG, SV, gp, pp), (n, cp, mp, 3, SN, float("inf"), SV, gp, pp),
        (n, cp, mp, 3, SN, SG, float("inf"), gp, pp),
    ]
    for args in bad:
        assert L.op_vignette_solve(*args) == -1, args
        assert L.op_last_error().decode().startswith("op_vignette_solve")
    count[1] = -5
    assert L.op_vignette_solve(n, cp, mp, 3, SN, SG, SV, gp, pp) == -1
    assert b"negative" in L.op_last_error()
    # the device entry points check their arguments before touching a device
    out = C.c_void_p()
    assert L.op_vignette_overlap(None, None, None, None, n, 2, 0.98, cp, mp) == -1
    assert b"op_vignette_overlap" in L.op_last_error()
    assert L.op_blend_vignette(None, None, None, None, n, gp, pp, C.byref(out)) == -1
    assert b"op_blend_vignette" in L.op_last_error()
    with pytest.raises(ValueError):
        hip.vignette_solve(4, count, mom)
    assert L.op_abi_version() >= 11
