"""Inputs that put the keypoint chain (k_refine, the rank sort of k_orientation, k_orient_peaks, k_expand_oriented, k_descriptor)
on the branches that images "with many keypoints" never reach: off-diagonal pivots of the 3 x 3 LU, rank-deficient Hessians
(the pseudo-inverse), candidates that move, also in scale, and leave the plane or the scale range, keypoints without a peak,
identical keypoints, descriptors whose window holds no weight.  test_keypoint_cases_cpu.py holds each case to the purpose it
is here for (the oracle's branch census), to the reference, and shows what the old inputs could not see;
test_gpu_keypoint_cases.py runs them on the device.  No tests here.

The lever of N, S and S0 is a negative JUDGE_EXTREMA_DIFF_THRES (a user-editable float that neither the reference nor
build_plan refuses): plateau pixels and near-ties pass the 26-neighbour test, so candidates arrive that a strict extremum
never produces."""
import numpy as np

import sift_cases as sc
from openpano_amd import synth

NEG = dict(JUDGE_EXTREMA_DIFF_THRES=-1e-4)
H, W = 241, 481


def stripes(h=H, w=W):
    """row y = float32(0.5 + 0.3 sin(y / 3.1) + 0.15 sin(y / 7.3)), evaluated in float64 and cast once; constant along x, grey:
    every Hessian has dxx = dxy = dsx = 0 exactly"""
    y = np.arange(h, dtype=np.float64)
    col = (0.5 + 0.3 * np.sin(y / 3.1) + 0.15 * np.sin(y / 7.3)).astype(np.float32)
    return np.ascontiguousarray(np.broadcast_to(col[:, None, None], (h, w, 3)))


def stripes_noise():
    """the stripes with columns 0..199 replaced by noise: trajectories that start on an x-constant site can end on a keypoint"""
    img = stripes().copy()
    img[:, :200] = sc.dense(H, 200, 5)
    return img


def _n():
    return sc.dense(H, W, 1)


def _s():
    return np.ascontiguousarray(stripes_noise()[:121, 80:321])


def _z():
    return sc.dense(121, 241, 1)


def old_view():
    """_view(400, 600, 1) of test_gpu_sift.py: the suite's everyday SIFT input, under the default config"""
    world = synth.make_world(1, 400 + 48, 600 + 48, work_scale=1600.0 / (400 + 600))
    return synth.cut_view(world, 24, 24, 400, 600, 1)


# name -> (image maker, (h, w), config keys on top of sift_cases.cfg_for(h, w))
CASES = {
    "N": (_n, (H, W), NEG),
    "N6": (_n, (H, W), dict(NEG, NUM_SCALE=6)),             # the generic k_pyramid<6> and its is_raw_extremum, not the row kernel's ring_extremum
    "S0": (stripes, (H, W), NEG),
    "S": (_s, (121, 241), NEG),
    "S241": (stripes_noise, (H, W), NEG),
    "O": (_n, (H, W), dict(ORI_RADIUS=0.3)),
    "O6": (_n, (H, W), dict(ORI_RADIUS=0.6)),
    "Z": (_z, (121, 241), dict(DESC_HIST_SCALE_FACTOR=0)),
    # found by a search over seeds 1..40 of dense(241, 481, seed) under N's config: one descriptor sample whose
    # now_ort rounds to exactly 2 pi, so floorf(hist_bin) is 8 and the bin index wraps through hbinf % 8
    "H": (lambda: sc.dense(H, W, 26), (H, W), NEG),
}
NAMES = list(CASES)


def case(name):
    """-> (image, config)"""
    make, (h, w), kv = CASES[name]
    img = make()
    assert img.shape == (h, w, 3) and img.dtype == np.float32
    return img, sc.cfg_for(h, w, **kv)


def same(a, b):
    """array equality in which NaNs are equal by position: the sign and payload of a NaN are not part of the contract"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na], b[~nb]))


class _NanBlind:
    """the view of a stage result that sift_cases' comparisons see: NaN descriptor elements replaced by one fixed finite
    value (-1: no descriptor element is negative), so that np.array_equal compares NaNs by position and the rest bit for bit"""

    def __init__(self, st):
        self.__dict__.update(st.__dict__)
        self.desc = np.where(np.isnan(st.desc), np.float32(-1), st.desc)


def compare_stages(g, o, cfg):
    """sift_cases._compare_stages with NaN descriptor elements compared by position"""
    assert not (g.desc[~np.isnan(g.desc)] < 0).any() and not (o.desc[~np.isnan(o.desc)] < 0).any()
    sc._compare_stages(_NanBlind(g), _NanBlind(o), cfg)


def compare_oracle_ref(so, sr):
    """sift_cases.compare_oracle_ref with NaN descriptor elements compared by position"""
    assert not (so.desc[~np.isnan(so.desc)] < 0).any() and not (sr.desc[~np.isnan(sr.desc)] < 0).any()
    sc.compare_oracle_ref(_NanBlind(so), _NanBlind(sr))


def segment_counts(o, seg=24, band=sc.RW_OWN):
    """raw extrema of octave 0 per 240 x 24 segment of k_pyramid_rows, counted as test_dense_extrema_fill_the_workgroup_lists does"""
    h0, w0 = o.dims[0]
    per_item = np.zeros(((h0 + seg - 1) // seg, (w0 + band - 1) // band), np.int64)
    for (oc, _), v in o.raw.items():
        if oc == 0:
            xy = np.asarray(v).reshape(-1, 2)
            np.add.at(per_item, (xy[:, 1] // seg, xy[:, 0] // band), 1)
    return per_item


# ---- matrices for the two 3 x 3 solvers of the refine step (test_gpu_keypoint_solvers.py)

def lu_pivots(m):
    """(first, second) pivot position of complete pivoting on a 3 x 3 (row * 3 + col; the second inside the trailing 2 x 2 as
    row * 2 + col, None where the first pivot is zero): the strict > scan in row-major order keeps the FIRST largest entry,
    as np.argmax does.  Used to sort candidates into classes; the tests count the classes with the oracle's own census."""
    a = np.array(m, np.float64)
    p1 = int(np.argmax(np.abs(a)))
    r, c = divmod(p1, 3)
    a[[0, r]] = a[[r, 0]]
    a[:, [0, c]] = a[:, [c, 0]]
    if not np.isfinite(a[0, 0]) or a[0, 0] == 0:
        return p1, None
    s = a[1:, 1:] - np.outer(a[1:, 0] / a[0, 0], a[0, 1:])
    return p1, int(np.argmax(np.abs(s)))


def hessians_of(st, limit):
    """the fp64 Hessians calc_kp_offset_iter (feature/extrema.cc:108-150) builds at the first raw extrema of an oracle run with
    planes: fp32 differences of the DoG stack, each widened once"""
    out = []
    f4 = np.float32(4)
    for (o, s), xy in sorted(st.raw.items()):
        lo, d, hi = st.dog[(o, s - 1)], st.dog[(o, s)], st.dog[(o, s + 1)]
        for x, y in np.asarray(xy).reshape(-1, 2)[:limit]:
            v = d[y, x]
            dxx = d[y, x + 1] + d[y, x - 1] - v - v
            dyy = d[y + 1, x] + d[y - 1, x] - v - v
            dss = hi[y, x] + lo[y, x] - v - v
            dxy = (d[y + 1, x + 1] - d[y - 1, x + 1] - d[y + 1, x - 1] + d[y - 1, x - 1]) / f4
            dys = (hi[y + 1, x] - hi[y - 1, x] - lo[y + 1, x] + lo[y - 1, x]) / f4
            dsx = (hi[y, x + 1] - hi[y, x - 1] - lo[y, x + 1] + lo[y, x - 1]) / f4
            out.append(np.array([[dxx, dxy, dsx], [dxy, dyy, dys], [dsx, dys, dss]], np.float64))
    return out


def solver_matrices(s0=None):
    """-> (mats (n, 3, 3) float64, classes: name -> index array).  Built from one fixed seed.  ``s0``: the oracle's stages of
    case S0 with planes; its x-constant Hessians join the class "s0_hessians"."""
    rng = np.random.default_rng(20240)
    mats, cls = [], {}

    def add(name, m):
        cls.setdefault(name, []).append(len(mats))
        mats.append(np.array(m, np.float64).reshape(3, 3))

    def sym(scale):
        a = rng.uniform(-1, 1, (3, 3)) * scale
        return np.triu(a) + np.triu(a, 1).T

    # symmetric, Hessian-like (1e-4 .. 1): the largest |entry| at each upper-triangle position, of either sign, by each of
    # the four second-pivot positions.  ((2, 1) behind a diagonal first pivot takes the two mirrored Schur entries rounding
    # apart, since the scan meets (1, 2) first: rarer, but common enough to fill its classes too.)
    PER = 40
    want = {(r * 3 + c, p2, sg): 0 for r in range(3) for c in range(r, 3) for p2 in range(4) for sg in (1, -1)}
    for _ in range(400000):
        if min(want.values()) >= PER:
            break
        a = sym(10.0 ** rng.uniform(-4, 0))
        r, c = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)][rng.integers(6)]
        sg = 1 if rng.integers(2) else -1
        a[r, c] = a[c, r] = sg * np.abs(a).max() * rng.uniform(1.0, 3.0)
        p1, p2 = lu_pivots(a)
        key = (p1, p2, sg)
        if p1 == r * 3 + c and key in want and want[key] < PER:
            want[key] += 1
            add("sym_p%d%d_q%d%d_%s" % (r, c, 1 + p2 // 2, 1 + p2 % 2, "pos" if sg > 0 else "neg"), a)

    # general matrices: FullPivLU of any 3 x 3, first pivot anywhere -- those in the lower triangle no product Hessian makes
    for k in range(900):
        a = rng.uniform(-1, 1, (3, 3)) * 10.0 ** rng.uniform(-4, 2)
        r, c = divmod(k % 9, 3)
        a[r, c] = (1 if k % 2 else -1) * np.abs(a).max() * rng.uniform(1.0, 3.0)
        add("general_lower" if r > c else "general", a)

    # exact ties in magnitude: within a row, across the diagonal, and all nine entries equal under every pattern of signs
    # (most of those are singular: exact zeros end the elimination at k = 1 and k = 2)
    for k in range(120):
        a = sym(0.5); big = 1.0 + k % 3
        r = k % 3; c0, c1 = [(0, 1), (0, 2), (1, 2)][(k // 3) % 3]
        a[r, c0] = big; a[r, c1] = -big if k % 2 else big
        add("tie_in_row", a)
        a = sym(0.5); a[c0, c1] = big; a[c1, c0] = -big if k % 2 else big
        add("tie_across_diagonal", a)
    for bits in range(512):
        add("tie_all_nine", np.array([1.0 if bits >> i & 1 else -1.0 for i in range(9)]) * (0.375 if bits % 3 else 1.0))

    # exact zeros that end the elimination at k = 0, 1, 2; small integers keep every quotient and product exact
    add("zero_k0", np.zeros((3, 3)))
    for i in range(3):
        for j in range(3):
            a = np.zeros((3, 3)); a[i, j] = -2.5 if (i + j) % 2 else 0.75
            add("zero_k1", a)
    for _ in range(60):
        u, v = rng.integers(-2, 3, 3), rng.integers(-2, 3, 3)
        if u.any() and v.any():
            add("zero_k1", np.outer(u, v).astype(np.float64) * 2.0 ** rng.integers(-8, 3))
    for _ in range(600):
        add("small_integers", rng.integers(-2, 3, (3, 3)).astype(np.float64))
    for _ in range(150):                                   # x-constant Hessians: a zero row and column, rank <= 2
        a = sym(10.0 ** rng.uniform(-4, 0)); k = rng.integers(3)
        a[k, :] = 0; a[:, k] = 0
        add("zero_k2", a)

    # the third (and the second) pivot just above, on and just below maxpivot * 3 * eps, the rank threshold
    eps3 = np.finfo(np.float64).eps * 3
    perms = [[0, 1, 2], [0, 2, 1], [1, 0, 2], [1, 2, 0], [2, 0, 1], [2, 1, 0]]
    for big in (1.0, 0.8125, 3.0e-3, 7.0):
        thr = abs(big) * eps3
        for t in (np.nextafter(thr, np.inf), thr, np.nextafter(thr, 0.0), 2 * thr, 0.5 * thr):
            for pr in perms[::2]:
                for pc in perms[1::2]:
                    add("threshold_third", np.diag([big, 0.5 * big, t])[pr][:, pc])
                    add("threshold_second", np.diag([big, t, 0.25 * t])[pr][:, pc])
                    add("threshold_third", np.diag([-big, 0.5 * big, -t])[pr][:, pc])

    # rank 0, 1, 2 for the pseudo-inverse: outer products, sums of two, singular values on both sides of 1e-6, and dense
    # symmetric matrices (several Jacobi sweeps)
    for _ in range(150):
        u = rng.standard_normal(3)
        add("rank1", np.outer(u, u) * 10.0 ** rng.uniform(-3, 0))
        v = rng.standard_normal(3)
        add("rank2", (np.outer(u, u) - np.outer(v, v)) * 10.0 ** rng.uniform(-3, 0))
    for s in (1e-6, np.nextafter(1e-6, 1), np.nextafter(1e-6, 0), 2e-6, 5e-7, 1.001e-6, 0.999e-6):
        for pr in perms:
            add("sigma_near_eps", np.diag([1.0, s, 0.0])[pr][:, pr])
            add("sigma_near_eps", np.diag([s, s, 0.25])[pr][:, perms[0]])
        for _ in range(8):
            q, _r = np.linalg.qr(rng.standard_normal((3, 3)))
            add("sigma_near_eps_rotated", q @ np.diag([0.5, s, 0.0]) @ q.T)
    for _ in range(300):
        add("dense_symmetric", sym(10.0 ** rng.uniform(-4, 0)))

    # an entry that is NaN, +inf or -inf
    for k in range(9):
        for bad in (np.nan, np.inf, -np.inf):
            a = sym(1.0); a[k // 3, k % 3] = bad
            add("nonfinite", a)
            a = rng.uniform(-1, 1, (3, 3)); a[k // 3, k % 3] = bad; a[(k + 4) % 9 // 3, (k + 4) % 9 % 3] = bad
            add("nonfinite", a)

    if s0 is not None:
        for m in hessians_of(s0, 60):
            add("s0_hessians", m)
    return np.stack(mats), {k: np.asarray(v) for k, v in cls.items()}
