"""Planted-homography scenes for the RANSAC stage off its default configuration -- TEST INFRASTRUCTURE ONLY.

One table, read by tests/test_ransac_config_cpu.py (the oracle reaches the exit each scene names; oracle == reference)
and tests/test_gpu_match_ransac_config.py (op_ransac_pairs == oracle, one call per configuration).  Seeded numpy only: no
SIFT, no images.  A scene is a pair of keypoint sets (centred coordinates, as op_features holds them), a match list, the
two image shapes (w, h), an mt19937 seed, the configuration it runs under and the exit of fill_inliers_to_matchinfo
(checkers.RANSAC_EXITS) it was built to reach.

Geometry: `common` points lie in both images, p1 = Ht p2 (+ Gaussian noise); every image also holds keypoints nobody
matches.  The match list draws from the common points; an `outlier` keeps its keypoint in the second image and gets a
uniformly drawn one in the first.

SINGULAR (the refit on the inliers has no inverse, transform_estimate.cc:182-184) is not in the table: no input reached it
in the oracle.  Tried: all matches on one line y = const in both images, all matches at one point of the second image
(every sample's DLT loses a column, ls_solve zeroes it, Homography::health refuses m[4] = 0: NO_HEALTHY); 8 exact
matches on a line among noisy off-line ones with RANSAC_INLIER_THRES 0.25, 2000 seeds (a healthy sample holds off-line
points, which the refit then keeps: its rank is 3).  A rank-deficient refit needs >= 8 inliers of a healthy hypothesis
whose second-image points are collinear to 1e-15 relative, and a healthy hypothesis cannot come from such points alone.
"""
from __future__ import annotations

import numpy as np

from openpano_amd.config import PanoConfig

HOMO = ()                                                                        # configuration keys: sorted (key, value) tuples
AFFINE = (("CYLINDER", 1), ("ESTIMATE_CAMERA", 0), ("ORDERED_INPUT", 1))
MODES = {"homo": HOMO, "affine": AFFINE}
ITERATIONS = (1, 2, 255, 256, 257, 1024, 1499, 4097, 65536)
THRESHOLDS = (0.0, 0.25, 1.0, 20.0)
RAISED_MATCH_RATIO = 0.8
NO_REFERENCE = ("DEAD", "NO_HEALTHY")       # get_transform on such input reads uninitialised members in the reference


def key_of(mode, **kv):
    return tuple(sorted(dict(MODES[mode], **kv).items()))


def config_of(key):
    return PanoConfig(**dict(key))


class Scene:
    def __init__(self, name, mode, kp1, kp2, match, shape1, shape2, seed, exit, reference=True, **cfg):
        self.name, self.mode, self.key = name, mode, key_of(mode, **cfg)
        self.kp1, self.kp2 = kp1, kp2
        self.match = np.ascontiguousarray(match, np.int32).reshape(-1, 2)
        self.shape1, self.shape2, self.seed, self.exit = shape1, shape2, seed, exit
        self.reference = reference and exit not in NO_REFERENCE     # False: the reference cannot take the scene (see where it is set)

    @property
    def cfg(self):
        return config_of(self.key)

    @property
    def id(self):
        return self.name + "|" + ",".join("%s=%.9g" % kv for kv in self.key)

    def under(self, exit, reference=True, **cfg):
        """the same arrays under another configuration"""
        base = {k: v for k, v in self.key if (k, v) not in AFFINE}
        return Scene(self.name, self.mode, self.kp1, self.kp2, self.match, self.shape1, self.shape2, self.seed, exit,
                     reference, **dict(base, **cfg))

    def swapped(self, name, exit):
        """the pair in the other order: (j, i), the shapes following their images"""
        s = Scene(name, self.mode, self.kp2, self.kp1, self.match[:, ::-1], self.shape2, self.shape1, self.seed + 1, exit)
        s.key = self.key
        return s


def _apply(H, p):
    q = np.concatenate([p, np.ones((len(p), 1))], 1) @ np.asarray(H, np.float64).T
    return q[:, :2] / q[:, 2:3]


def _uniform(rng, n, shape, box=None):
    w, h = shape
    x0, x1, y0, y1 = box or (-w / 2, w / 2, -h / 2, h / 2)
    return np.stack([rng.uniform(x0, x1, n), rng.uniform(y0, y1, n)], 1)


def _inside(p, shape):
    w, h = shape
    return (p[:, 0] >= -w / 2) & (p[:, 0] < w / 2) & (p[:, 1] >= -h / 2) & (p[:, 1] < h / 2)


def shift(mode, tx=210.0, ty=-12.0, scale=1.0):
    """p1 = Ht p2: a small rotation and zoom on a translation, with a perspective row in homography mode"""
    H = np.array([[1.01 * scale, 0.02 * scale, tx], [-0.015 * scale, 0.99 * scale, ty], [0.0, 0.0, 1.0]])
    if mode == "homo":
        H[2, :2] = (4e-5 * scale, -2e-5 * scale)
    return H


def planted(seed, shape1, shape2, Ht, common, m, noise=0.4, outliers=0.0, extra1=0, extra2=0, repeat=1,
            outlier_box=None, extra2_box=None, margin=0.0):
    """-> kp1, kp2, match.  `common` points of image 2 whose image under Ht lies in image 1 (at least `margin` pixels from
    both borders); `m` of them matched (each `repeat` times), a fraction `outliers` of those with a wrong keypoint in
    image 1 (drawn from outlier_box, default all of image 1); extra1 / extra2 unmatched keypoints."""
    rng = np.random.default_rng(seed)
    k2 = np.zeros((0, 2))
    while len(k2) < common:
        c = _uniform(rng, 4 * common, (shape2[0] - 2 * margin, shape2[1] - 2 * margin))
        k2 = np.concatenate([k2, c[_inside(_apply(Ht, c), (shape1[0] - 2 * margin, shape1[1] - 2 * margin))]])
    k2 = k2[:common]
    k1 = _apply(Ht, k2) + rng.normal(0, noise, (common, 2))
    a = np.sort(rng.choice(common, m, replace=False))
    bad = a[rng.random(m) < outliers]
    k1[bad] = _uniform(rng, len(bad), shape1, outlier_box)
    kp1 = np.concatenate([k1, _uniform(rng, extra1, shape1)])
    kp2 = np.concatenate([k2, _uniform(rng, extra2, shape2, extra2_box)])
    a = np.repeat(a, repeat)
    return kp1, kp2, np.stack([a, a], 1).astype(np.int32)


S = (600, 400)


def _gate_scenes(mode):
    """default iterations and threshold: one scene per exit, the three causes of POINT_RATIO_1, the unequal shapes"""
    H = shift(mode)
    sc = []

    def add(name, exit, seed, arrays, shape1=S, shape2=S, reference=True, **cfg):
        sc.append(Scene(name, mode, *arrays, shape1, shape2, seed, exit, reference, **cfg))
        return sc[-1]
    add("accepted", "ACCEPTED", 101, planted(1, S, S, H, 260, 120, outliers=0.3, extra1=140, extra2=140))
    add("dead_m7", "DEAD", 102, planted(2, S, S, H, 100, 7, extra1=50, extra2=50))
    mirror = np.diag([-1.0, 1.0, 1.0]) @ shift(mode, tx=0.0)                    # x2x <= x1x in every hypothesis (homography.hh:106-127)
    add("mirrored", "NO_HEALTHY", 103, planted(3, S, S, mirror, 200, 60, extra1=50, extra2=50))
    add("random_matches", "FEW_INLIERS", 104, planted(4, S, S, H, 200, 40, outliers=1.0, extra1=50, extra2=50))
    # POINT_RATIO_1, rp > 1: 30 keypoints matched three times each -- 90 inliers over ~30 keypoints in the overlap
    add("repeated_keypoints", "POINT_RATIO_1", 105, planted(5, S, S, H, 30, 30, repeat=3))
    # POINT_RATIO_1, rp < 0.01: 14 matches among 4000 keypoints
    add("sparse_matches", "POINT_RATIO_1", 106, planted(6, S, S, H, 2600, 14, extra1=1400, extra2=1400))
    # POINT_RATIO_1, no polygon: the translation moves image 2 off image 1 (keypoints outside their frame are accepted by the
    # API); the reference asserts in PointInPolygon's constructor here (polygon.hh:32), so it is not asked
    kp1, kp2, mt = planted(7, S, S, shift(mode, tx=0.0), 200, 60, extra1=50, extra2=50)
    add("disjoint_images", "POINT_RATIO_1", 107, (kp1 + np.array([1800.0, 0.0]), kp2, mt), reference=False)
    # POINT_RATIO_2 past image 1's gates: 4000 keypoints that only image 2 has, all inside its overlap with image 1
    add("second_image_crowded", "POINT_RATIO_2", 108, planted(8, S, S, H, 40, 20, extra1=40, extra2=4000, extra2_box=(-280, 60, -180, 180)))
    add("low_confidence", "CONFIDENCE", 109, planted(9, S, S, H, 1000, 20, extra1=500, extra2=500))
    # unequal shapes.  Image 1 three times the size of image 2 and Ht a zoom by 3: image 2 covers image 1, the overlap polygon
    # measured in image 2 is a ninth of the larger area (AREA); in the other order it is all of it.  The inlier distance
    # follows the FIRST image's shape: with 2.5 px of noise about a sixth of the true matches miss (1200 + 900) / 1600 * 3.5 =
    # 4.6 px, and five in six would miss the 1.5 px of the smaller image.
    big, small = (1200, 900), (400, 300)
    zoom = planted(10, big, small, shift(mode, tx=8.0, ty=-5.0, scale=3.0), 300, 150, noise=2.5, outliers=0.2, extra1=100, extra2=60)
    a = add("large_small_zoom", "AREA", 110, zoom, big, small)
    sc.append(a.swapped("small_large_zoom", "ACCEPTED"))
    land, port = (600, 400), (400, 600)
    lp = add("landscape_portrait", "ACCEPTED", 112, planted(12, land, port, shift(mode, tx=100.0, ty=6.0), 250, 110, noise=0.8, outliers=0.3, extra1=120, extra2=150), land, port)
    sc.append(lp.swapped("portrait_landscape", "ACCEPTED"))
    # 12 clean matches and 2 gross outliers (matches 5 and 13): a sample without the outliers counts 12, every later such
    # sample ties it
    kp1, kp2, mt = planted(13, S, S, H, 12, 12, noise=0.05, extra1=30, extra2=30)
    far = np.array([[250.0, -150.0], [-200.0, 120.0]])
    kp1, kp2 = np.concatenate([kp1, far]), np.concatenate([kp2, far[::-1] * 0.5])
    n1, n2 = len(kp1), len(kp2)
    add("tie_m14", "ACCEPTED", 113, (kp1, kp2, np.concatenate([mt[:5], [[n1 - 2, n2 - 2]], mt[5:], [[n1 - 1, n2 - 1]]])))
    return sc


def _raised_ratio_scenes(mode):
    """INLIER_IN_MATCH_RATIO = 0.8"""
    H = shift(mode)
    r = dict(INLIER_IN_MATCH_RATIO=RAISED_MATCH_RATIO)
    return [
        Scene("clean", mode, *planted(21, S, S, H, 200, 100, outliers=0.04, extra1=100, extra2=100), S, S, 201, "ACCEPTED", **r),
        Scene("outliers_everywhere", mode, *planted(22, S, S, H, 260, 120, outliers=0.45, extra1=140, extra2=140), S, S, 202, "MATCH_RATIO_1", **r),
        # MATCH_RATIO_2 past image 1's gates: the outliers' keypoints in image 1 lie left of x = -110, outside the overlap
        # (image 2 covers x > -90 of image 1); in image 2 they are ordinary points of the overlap
        Scene("outliers_outside_first_overlap", mode, *planted(23, S, S, H, 260, 120, outliers=0.4, extra1=140, extra2=140, outlier_box=(-300, -110, -200, 200)),
              S, S, 203, "MATCH_RATIO_2", **r),
    ]


def _sweep_scenes(mode):
    """the lists every RANSAC_ITERATIONS value runs on: m = 8 (about 22 draws per sample), 13 | 14 (the two launch
    groups), 64 | 65 (bit-mask walk | compare walk), a few hundred"""
    H = shift(mode)
    sc = []
    for k, (m, noise, out) in enumerate([(8, 0.6, 0.0), (13, 0.8, 0.15), (14, 0.8, 0.15), (64, 0.9, 0.25), (65, 0.9, 0.25), (300, 1.1, 0.45)]):
        sc.append(Scene("m%d" % m, mode, *planted(30 + k, S, S, H, max(m, 40) * 2, m, noise=noise, outliers=out, extra1=60, extra2=60), S, S, 300 + k, None))
    return sc


def _edge_scene(mode):
    """every matched point at least 40 px inside both images' overlap: the match counts of both polygons are m, so the
    oracle's match ratios are float32(inliers) / float32(m) on both sides"""
    H = shift(mode, tx=14.0, ty=-6.0)
    return Scene("edge", mode, *planted(41, S, S, H, 240, 157, noise=0.7, outliers=0.3, extra1=90, extra2=120, margin=40.0,
                                        outlier_box=(-240, 240, -150, 150)), S, S, 401, "ACCEPTED")


# float32 values the oracle returns for the edge scene (asserted in tests/test_ransac_config_cpu.py): its confidence and its
# match ratio float32(inliers) / float32(157)
EDGE = {"homo": dict(confidence="0.32975692", match_ratio="0.7133758"), "affine": dict(confidence="0.33172348", match_ratio="0.7197452")}

# exits of the sweep scenes where they differ from the scene's own: (mode, scene, configuration override) -> exit.
# No point is an inlier at RANSAC_INLIER_THRES 0, fewer than eight are at 0.25 (a distance of 0.16 px under 0.4 to 4 px of noise)
_THRES_GROUP = ("noisy_4px", "m13", "m300", "large_small_zoom", "small_large_zoom", "landscape_portrait", "portrait_landscape")
SWEEP_EXITS = {(mode, name, (("RANSAC_INLIER_THRES", th),)): "FEW_INLIERS" for mode in MODES for th in (0.0, 0.25) for name in _THRES_GROUP}
SWEEP_EXITS.update({
    # one or two hypotheses: a sample that holds an outlier is unhealthy (homography) or fits nothing (affine)
    ("homo", "m13", (("RANSAC_ITERATIONS", 1),)): "NO_HEALTHY",
    ("homo", "m300", (("RANSAC_ITERATIONS", 1),)): "NO_HEALTHY",
    ("homo", "m13", (("RANSAC_ITERATIONS", 2),)): "NO_HEALTHY",
    ("homo", "m300", (("RANSAC_ITERATIONS", 2),)): "NO_HEALTHY",
    ("affine", "m13", (("RANSAC_ITERATIONS", 1),)): "FEW_INLIERS",
    ("affine", "m300", (("RANSAC_ITERATIONS", 1),)): "FEW_INLIERS",
    ("affine", "m13", (("RANSAC_ITERATIONS", 2),)): "FEW_INLIERS",
    ("affine", "m300", (("RANSAC_ITERATIONS", 2),)): "FEW_INLIERS",
    ("homo", "noisy_4px", (("RANSAC_INLIER_THRES", 1.0),)): "FEW_INLIERS",
    ("homo", "m13", (("RANSAC_INLIER_THRES", 1.0),)): "FEW_INLIERS",
    ("homo", "m300", (("RANSAC_INLIER_THRES", 1.0),)): "MATCH_RATIO_2",
    ("affine", "noisy_4px", (("RANSAC_INLIER_THRES", 1.0),)): "FEW_INLIERS",
    ("affine", "m13", (("RANSAC_INLIER_THRES", 1.0),)): "FEW_INLIERS",
    ("affine", "m300", (("RANSAC_INLIER_THRES", 1.0),)): "MATCH_RATIO_2",
})


def _up(v):
    return float(np.nextafter(np.float32(v), np.float32(np.inf)))


def build():
    out = []
    for mode in MODES:
        gates = _gate_scenes(mode)
        sweep = _sweep_scenes(mode)
        out += gates + _raised_ratio_scenes(mode)
        by_name = {s.name: s for s in gates}
        # without outliers: under RANSAC_ITERATIONS = 1 the only hypothesis decides, and it is a good one
        clean = Scene("clean_m100", mode, *planted(61, S, S, shift(mode), 200, 100, extra1=80, extra2=80), S, S, 601, "ACCEPTED")
        shapes = [by_name[n] for n in ("large_small_zoom", "small_large_zoom", "landscape_portrait", "portrait_landscape")]
        out += [s.under(SWEEP_EXITS.get((mode, s.name, ()), "ACCEPTED")) for s in sweep]
        for it in ITERATIONS:
            ov = (("RANSAC_ITERATIONS", it),)
            # 257 and 4097: unequal shapes and a dead pair among the live ones
            group = sweep + (shapes + [by_name["dead_m7"]] if it in (257, 4097) else []) + ([clean, by_name["mirrored"]] if it == 1 else [])
            out += [s.under(SWEEP_EXITS.get((mode, s.name, ov), s.exit or "ACCEPTED"), RANSAC_ITERATIONS=it) for s in group]
        noisy = Scene("noisy_4px", mode, *planted(51, S, S, shift(mode), 220, 150, noise=4.0, extra1=80, extra2=80), S, S, 501, None)
        for th in THRESHOLDS:
            ov = (("RANSAC_INLIER_THRES", th),)
            group = [noisy, sweep[1], sweep[5]] + shapes
            out += [s.under(SWEEP_EXITS.get((mode, s.name, ov), s.exit or "ACCEPTED"), RANSAC_INLIER_THRES=th) for s in group]
        e = _edge_scene(mode)
        c, r = EDGE[mode]["confidence"], EDGE[mode]["match_ratio"]
        out.append(e)
        # a gate value equal to the measured figure keeps the pair (the gates are `<`), one ulp above rejects it.  Judged
        # against the oracle only: one ulp from a threshold the reference's SVD solution need not land on the same side
        out += [e.under("ACCEPTED", reference=False, INLIER_IN_POINTS_RATIO=float(np.float32(c))),
                e.under("CONFIDENCE", reference=False, INLIER_IN_POINTS_RATIO=_up(c)),
                e.under("ACCEPTED", reference=False, INLIER_IN_MATCH_RATIO=float(np.float32(r))),
                e.under("MATCH_RATIO_1", reference=False, INLIER_IN_MATCH_RATIO=_up(r))]
    ids = [s.id for s in out]
    assert len(set(ids)) == len(ids), [i for i in ids if ids.count(i) > 1]
    return out


SCENES = build()


def by_config():
    """{configuration key: its scenes}: one op_ransac_pairs call each"""
    groups = {}
    for s in SCENES:
        groups.setdefault(s.key, []).append(s)
    return groups


def check(oracle, got, m, ca, cb, s1, s2, seed, cfg=None):
    """one pair of op_ransac_pairs against the oracle: winner, acceptance, confidence and inliers equal, the homography
    bit for bit when accepted"""
    want = oracle.ransac(m, ca, cb, s1, s2, seed, cfg=cfg)
    assert got["best_hyp"] == want["best_hyp"] and got["best_count"] == want["best_count"]
    assert got["ok"] == want["ok"]
    assert got["confidence"] == want["confidence"]
    assert np.array_equal(got["inliers"], want["inliers"])
    if want["ok"]:
        assert np.array_equal(got["homo"], want["homo"])
    return want


def mt19937_samples(seed, m, nsample, count):
    """the first `count` samples TransformEstimation::get_transform draws (transform_estimate.cc:64-77): std::mt19937(seed),
    rng() % m until `nsample` distinct indices"""
    bg = np.random.MT19937()
    bg._legacy_seeding(int(seed))
    out = []
    raw = iter(())
    while len(out) < count:
        sel = []
        while len(sel) < nsample:
            r = next(raw, None)
            if r is None:
                raw = iter((bg.random_raw(4096) % m).tolist())
                continue
            if r not in sel:
                sel.append(r)
        out.append(sel)
    return out


def moved_to_front(scene, samples, k):
    """the scene's match list reordered so that hypothesis 0 of the same seed draws the points hypothesis k drew, in the
    same order: the oracle's best_count with RANSAC_ITERATIONS = 1 on it is hypothesis k's inlier count (-1: unhealthy)"""
    m = len(scene.match)
    new = np.full(m, -1)
    new[samples[0]] = samples[k]
    rest = [i for i in range(m) if i not in set(samples[k])]
    new[new < 0] = rest
    return scene.match[new]
