"""The two 3 x 3 solvers of the refine step, as functions.  Images reach an off-diagonal pivot of the LU a few dozen times and
cannot observe the pseudo-inverse at all (every rank-deficient site is rejected later, test_keypoint_cases_cpu.py), so the
device's inverse3_fullpiv -- a register-only network of conditional swaps, not the oracle's loop -- and pinv3_jacobi run here on
six thousand matrices (keypoint_cases.solver_matrices) through a probe kernel that only a variant build contains
(-DOP_KP_SOLVER_PROBE, csrc/keypoints.hip), bit for bit against the oracle's orc_solve3.  CPU: the oracle's census shows that the
matrices reach every pivot position, every rank and both sides of the rank threshold, and its LU inverse is held to a cofactor
inverse in extended precision, which shares nothing with the restatement."""
import os
import subprocess
import sys

import numpy as np
import pytest

import keypoint_cases as kc

HERE = os.path.dirname(os.path.abspath(__file__))
EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def solved():
    """matrices, classes and the oracle's answers, made once: dict(m, cls, ok, lu, pinv, where)"""
    from checkers import Oracle
    img, cfg = kc.case("S0")
    o = Oracle(cfg)
    m, cls = kc.solver_matrices(o.sift_stages(img))
    ok, lu, pinv, where = o.solve3(m)
    return dict(m=m, cls=cls, ok=ok, lu=lu, pinv=pinv, where=where)


def _inverse_extended(m):
    """cofactor inverse in np.longdouble (a 64-bit significand here; numpy's linalg has no extended-precision inverse): for a
    condition number below 1e6 its own error stays below 1e6 x 2^-63, a thousandth of what an fp64 inverse can reach"""
    a = m.astype(np.longdouble)
    c = np.empty_like(a)
    for i in range(3):
        for j in range(3):
            r = [k for k in range(3) if k != i]; s = [k for k in range(3) if k != j]
            c[:, j, i] = (-1) ** (i + j) * (a[:, r[0], s[0]] * a[:, r[1], s[1]] - a[:, r[0], s[1]] * a[:, r[1], s[0]])
    det = a[:, 0, 0] * c[:, 0, 0] + a[:, 0, 1] * c[:, 1, 0] + a[:, 0, 2] * c[:, 2, 0]
    return c / det[:, None, None]


def _well_conditioned(s):
    """indices of the finite matrices the LU inverted whose 2-norm condition number is below 1e6, and those numbers"""
    idx = np.array([i for i in np.flatnonzero(s["ok"]) if np.isfinite(s["m"][i]).all()])
    cond = np.linalg.cond(s["m"][idx])
    keep = cond < 1e6
    return idx[keep], cond[keep]


def _relative_errors(inv, m):
    want = _inverse_extended(m)
    return np.asarray(np.abs(inv - want).max(axis=(1, 2)) / np.abs(want).max(axis=(1, 2)), np.float64)


def test_solver_matrices_reach_every_pivot_rank_and_threshold_side(solved):
    s = solved; where, cls, ok = s["where"], s["cls"], s["ok"]
    assert len(s["m"]) > 3000

    def count(i_list, name):
        return sum(name in where[i] for i in i_list)
    # symmetric: each upper-triangle first pivot by each second pivot by each sign, as the ORACLE pivots
    for r in range(3):
        for c in range(r, 3):
            for q in ("11", "12", "21", "22"):
                for sg in ("pos", "neg"):
                    idx = cls["sym_p%d%d_q%s_%s" % (r, c, q, sg)]
                    assert len(idx) >= 20 and count(idx, "pivot1_%d%d" % (r, c)) == len(idx) and count(idx, "pivot2_" + q) == len(idx), (r, c, q, sg)
                    assert (np.sign(s["m"][idx, r, c]) == (1 if sg == "pos" else -1)).all()
    for p in ("10", "20", "21"):                             # the lower triangle: general matrices only
        assert count(cls["general_lower"], "pivot1_" + p) >= 50
        assert sum(count(v, "pivot1_" + p) for k, v in cls.items() if k.startswith("sym_")) == 0
    # ties: the strict > scan keeps the first of equal magnitudes in row-major order
    assert all(int(np.argmax(np.abs(s["m"][i]))) == int([k for k in where[i] if k.startswith("pivot1_")][0][-2]) * 3 + int([k for k in where[i] if k.startswith("pivot1_")][0][-1])
               for name in ("tie_in_row", "tie_across_diagonal", "tie_all_nine") for i in cls[name])
    assert count(cls["tie_all_nine"], "pivot1_00") == 512
    # exact zeros end the elimination at k = 0 (no pivot at all), k = 1 (no second pivot), k = 2
    assert not where[cls["zero_k0"][0]].keys() - {"lu_rank_0"} and "lu_rank_0" in where[cls["zero_k0"][0]]
    assert all("lu_rank_1" in where[i] and not any(k.startswith("pivot2_") for k in where[i]) for i in cls["zero_k1"])
    assert all("lu_rank_2" in where[i] for i in cls["zero_k2"]) and not ok[cls["zero_k2"]].any()
    # both sides of the rank threshold |pivot| > |maxpivot| * 3 eps
    t3 = cls["threshold_third"]
    assert 0.3 * len(t3) < ok[t3].sum() < 0.5 * len(t3) and count(t3, "lu_rank_2") == len(t3) - ok[t3].sum()
    t2 = cls["threshold_second"]                              # the second pivot above the threshold leaves rank 2, on or below it rank 1
    assert count(t2, "lu_rank_1") >= 0.3 * len(t2) and count(t2, "lu_rank_2") >= 0.3 * len(t2) and not ok[t2].any()
    # the pseudo-inverse's inputs: ranks 0, 1, 2 as the LU sees them, and case S0's own Hessians
    assert count(cls["rank1"], "lu_rank_1") + count(cls["rank1"], "lu_rank_2") == len(cls["rank1"])
    assert count(cls["rank2"], "lu_rank_2") >= 0.9 * len(cls["rank2"])
    h = cls["s0_hessians"]
    xconst = (s["m"][h][:, 0, :] == 0).all(axis=1) & (s["m"][h][:, :, 0] == 0).all(axis=1)       # dxx = dxy = dsx = 0 exactly
    assert len(h) >= 200 and xconst.sum() >= 100 and count(h[xconst], "lu_rank_2") == xconst.sum()
    assert not np.isfinite(s["m"][cls["nonfinite"]]).all(axis=(1, 2)).any()


def test_pseudo_inverse_of_the_oracle_has_the_rank_it_is_given(solved):
    """Moore-Penrose conditions on the rank-deficient classes, where the rank is clear of the cut (every singular value above
    1e-5 or below 1e-12), to 1e-9 relative (the Jacobi sweeps stop at 1e-15); and the cut itself at 1e-6: a singular value
    below it is dropped, one above it is inverted"""
    s = solved
    for name in ("rank1", "rank2", "zero_k2", "s0_hessians"):
        checked = 0
        for i in s["cls"][name]:
            a, p = s["m"][i], s["pinv"][i]
            sv = np.linalg.svd(a, compute_uv=False)
            if ((sv > 1e-12) & (sv < 1e-5)).any():
                continue
            checked += 1
            assert np.abs(a @ p @ a - a).max() <= 1e-9 * np.abs(a).max(), (name, i)
            assert np.abs(p @ a @ p - p).max() <= 1e-9 * np.abs(p).max(), (name, i)
            assert np.abs(a @ p - (a @ p).T).max() <= 1e-9, (name, i)
        assert checked >= 50, name
    assert (s["pinv"][s["cls"]["zero_k0"][0]] == 0).all()
    near = s["cls"]["sigma_near_eps"]
    norms = np.abs(s["pinv"][near]).max(axis=(1, 2))
    assert (norms > 4e5).sum() >= 10 and (norms < 10).sum() >= 10           # 1 / s kept for s > 1e-6, dropped below: both happen


def test_lu_inverse_of_the_oracle_against_extended_precision(solved):
    """On the well-conditioned subset (condition number below 1e6, about 4000 matrices) the oracle's inverse differs from the
    extended-precision cofactor inverse by at most 1.09e-13 relative to the inverse's largest entry (measured; that matrix
    has a condition number of 4.4e3).  Per matrix the error is held to 16 x condition x eps (measured worst: 1.03 x):
    complete pivoting is backward stable with a growth factor of at most 4 at n = 3, so the forward error of a solved
    column is a small multiple of condition x eps.  The GPU test allows the device the first figure, recomputed there."""
    idx, cond = _well_conditioned(solved)
    assert len(idx) > 3000
    err = _relative_errors(solved["lu"][idx], solved["m"][idx])
    print("worst relative error %.3g at condition %.3g; worst err / (cond eps) %.3g" % (err.max(), cond[err.argmax()], (err / (cond * EPS)).max()))
    assert (err <= 16 * cond * EPS).all()


@pytest.mark.gpu
def test_device_solvers_equal_the_oracle_bit_for_bit(solved, tmp_path):
    import variant_lib
    root = os.path.dirname(HERE)
    lib = variant_lib.build_variant(tmp_path, "keypoints", ["-DOP_KP_SOLVER_PROBE"])
    m = solved["m"]
    np.save(tmp_path / "in.npy", m)
    code = ("import sys, ctypes as C, numpy as np; sys.path.insert(0, %r)\n"
            "from openpano_amd import hip\n"
            "assert hip.LIB_PATH == %r\n"
            "m = np.ascontiguousarray(np.load(%r)); n = len(m)\n"
            "v = np.zeros(n, np.int32); lu = np.zeros((n, 3, 3)); pv = np.zeros((n, 3, 3))\n"
            "f = hip.lib().op_debug_kp_solver_probe; f.restype = C.c_int; f.argtypes = [C.c_void_p] * 1 + [C.c_int] + [C.c_void_p] * 3\n"
            "rc = f(m.ctypes.data, n, v.ctypes.data, lu.ctypes.data, pv.ctypes.data)\n"
            "assert rc == 0, rc\n"
            "np.savez(%r, v=v, lu=lu, pv=pv)\n") % (root, lib, str(tmp_path / "in.npy"), str(tmp_path / "out.npz"))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, OPENPANO_HIP_LIB=lib), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    got = np.load(tmp_path / "out.npz")
    bad = {}
    for name, idx in solved["cls"].items():
        nv = int((got["v"][idx] != solved["ok"][idx]).sum())
        nl = sum(not kc.same(got["lu"][i], solved["lu"][i]) for i in idx)
        npv = sum(not kc.same(got["pv"][i], solved["pinv"][i]) for i in idx)
        if nv or nl or npv:
            bad[name] = (nv, nl, npv, len(idx))
    assert not bad, "classes whose (verdicts, LU inverses, pseudo-inverses, of) differ from the oracle: %r" % bad
    # independent of the oracle's restatement: the device's inverse against extended precision, held to the oracle's own worst
    idx, _ = _well_conditioned(solved)
    allowed = _relative_errors(solved["lu"][idx], m[idx]).max()
    assert _relative_errors(got["lu"][idx], m[idx]).max() <= allowed
