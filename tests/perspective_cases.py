"""The perspective correction of cylinder mode (CylinderStitcher::perspective_correction, stitch/cylstitcher.cc:139-180) in numpy,
and the cases its kernel (k_canvas_perspective, csrc/canvas.hip) is held to.  No tests here: test_perspective_cpu.py proves that
the restatement and the cases are what they claim, test_gpu_perspective.py and test_gpu_cylinder_stitch.py hold the device to them.

perspective_ref restates the pass from the reference's semantics, one operation per numpy call so that nothing is fused:
  the map          Homography::trans2d(Vec2D(j, i)) (homography.hh:53-76): three fp64 dot products with z = 1, denom = 1.0 / z,
                   x * denom, y * denom; no centre offset, no z < 0 test
  the bounds       ImageToAdd::map_coor (blender.hh:39-44) on the doubles: x < 0 || x >= w || y < 0 || y >= h skips, then
                   isNaN() (blender.cc:29), which looks at x
  the sample       interpolate (lib/imgproc.cc:135-156) in fp32, Color::NO when a tap is NO
  the weight       (float)(0.5 - fabs((double)(c / (float)W) - 0.5)), times the row term unless ORDERED_INPUT (blender.cc:33-35)
  the division     non-lazy: (0 + col * w) * (float)(1.0 / (double)w) when wsum > 0 (blender.cc:83-91, lib/geometry.hh:123-124);
                   lazy: (0 + col * w) / w when wsum != 0 (:56-59, :70-71); -1 otherwise

to_ref_coor restates the corner geometry of :140-161 in fp64 with + - * / only."""
import collections
import itertools
import zlib

import numpy as np

F = np.float32
D = np.float64


def perspective_ref(canvas, inv, ordered_input=1, lazy=0):
    src = np.ascontiguousarray(canvas, F)
    H, W = src.shape[:2]
    d = np.asarray(inv, D).reshape(9)
    out = np.full((H, W, 3), F(-1), F)
    if H == 0 or W == 0:
        return out
    i, j = np.meshgrid(np.arange(H, dtype=D), np.arange(W, dtype=D), indexing="ij")
    with np.errstate(all="ignore"):
        def row(a, b, c):
            t = d[a] * j
            u = d[b] * i
            t = t + u
            return t + d[c] * 1.0
        rx, ry, rz = row(0, 1, 2), row(3, 4, 5), row(6, 7, 8)
        denom = 1.0 / rz
        ox = rx * denom
        oy = ry * denom
        ok = ~((ox < 0) | (ox >= W) | (oy < 0) | (oy >= H))        # map_coor, on the doubles
        ok &= ~np.isnan(ox)                                        # isNaN()
        r = oy.astype(F)
        c = ox.astype(F)
        fr = np.floor(r)
        fc = np.floor(c)
        ok &= (fr >= 0) & (fc >= 0) & (fc + 1 < W) & (fr + 1 < H)  # interpolate's bounds; NaN fails them
        ir = np.where(ok, fr, 0).astype(np.int64)
        ic = np.where(ok, fc, 0).astype(np.int64)
        ir1 = np.minimum(ir + 1, H - 1)
        ic1 = np.minimum(ic + 1, W - 1)
        r = r - fr.astype(F)
        c = c - fc.astype(F)
        one = F(1)
        nr = one - r
        nc = one - c
        p00, p10, p11, p01 = src[ir, ic], src[ir1, ic], src[ir1, ic1], src[ir, ic1]
        ok &= (p00[..., 0] >= 0) & (p10[..., 0] >= 0) & (p11[..., 0] >= 0) & (p01[..., 0] >= 0)
        col = np.zeros((H, W, 3), F)
        for p, wt in ((p00, nr * nc), (p10, r * nc), (p11, r * c), (p01, nr * c)):
            t = p * wt[..., None]
            col = col + t
        ok &= ~(col[..., 0] < 0)
        # the weight reads the sample's coordinates, not their fractions
        r, c = oy.astype(F), ox.astype(F)
        t = c / F(W)
        t = t.astype(D) - 0.5
        t = np.abs(t)
        w = (0.5 - t).astype(F)
        if not ordered_input:
            u = r / F(H)
            u = u.astype(D) - 0.5
            u = np.abs(u)
            u = 0.5 - u
            w = (w.astype(D) * u).astype(F)
        s = col * w[..., None]
        s = F(0) + s
        wsum = F(0) + w
        if lazy:
            good = ok & (wsum != 0)
            res = s / wsum[..., None]
        else:
            good = ok & (wsum > 0)
            iw = (1.0 / wsum.astype(D)).astype(F)
            res = s * iw[..., None]
    out[good] = res[good]
    return out


def to_ref_coor(proj_min, ref_wh, wh, homo, v):
    """one corner of cylstitcher.cc:148-156: v scaled by the component's ImageRef size, homo.trans, / ref size, the flat
    homo2proj, * ref size, - proj_min"""
    h = np.asarray(homo, D).reshape(9)
    x = D(v[0]) * D(wh[0])
    y = D(v[1]) * D(wh[1])
    hx = h[0] * x + h[1] * y + h[2] * D(1)
    hy = h[3] * x + h[4] * y + h[5] * D(1)
    hz = h[6] * x + h[7] * y + h[8] * D(1)
    hx = hx / D(ref_wh[0])
    hy = hy / D(ref_wh[1])
    with np.errstate(all="ignore"):
        tx = hx / hz
        ty = hy / hz
    tx = tx * D(ref_wh[0])
    ty = ty * D(ref_wh[1])
    return np.array([tx - D(proj_min[0]), ty - D(proj_min[1])], D)


def corners_ref(proj_min, ref_wh, first_wh, first_homo, last_wh, last_homo):
    return np.stack([to_ref_coor(proj_min, ref_wh, first_wh, first_homo, (-0.5, -0.5)),
                     to_ref_coor(proj_min, ref_wh, first_wh, first_homo, (-0.5, 0.5)),
                     to_ref_coor(proj_min, ref_wh, last_wh, last_homo, (0.5, -0.5)),
                     to_ref_coor(proj_min, ref_wh, last_wh, last_homo, (0.5, 0.5))])


def corners_std(canvas_wh):
    w, h = canvas_wh
    return np.array([[0, 0], [0, h], [w, 0], [w, h]], D)


def apply_homography(m, pts):
    m = np.asarray(m, D).reshape(3, 3)
    p = np.concatenate([np.asarray(pts, D), np.ones((len(pts), 1))], axis=1) @ m.T
    return p[:, :2] / p[:, 2:]


# ---- the cases -------------------------------------------------------------------------------------------------------------
# the smallest shapes at which the kernel can still go wrong: one tile and less, no second row (every pixel NO), a width one past
# four 64-column tiles, odd sizes, more than one tile both ways
SHAPES = [(2, 2), (1, 7), (5, 257), (37, 53), (67, 130)]
CONTENTS = ("random", "border", "hole")
HOMOS = ("identity", "mild", "shift", "z0", "zneg", "tiny", "outside")
FLAGS = list(itertools.product((0, 1), (0, 1)))                 # (ORDERED_INPUT, LAZY_READ)
SHIFT = (0.37, 0.61)

Case = collections.namedtuple("Case", "id h w content homo")
CASES = [Case("%dx%d_%s_%s" % (h, w, c, m), h, w, c, m) for (h, w), c, m in itertools.product(SHAPES, CONTENTS, HOMOS)]


def canvas_of(case):
    """random colours in [0, 1); "border": Color::NO two pixels wide all round; "hole": a block of Color::NO inside"""
    h, w = case.h, case.w
    v = np.random.default_rng(zlib.crc32(("%dx%d" % (h, w)).encode())).random((h, w, 3), dtype=F)
    if case.content == "border":
        keep = np.zeros((h, w), bool)
        keep[2:-2, 2:-2] = True
        v[~keep] = -1
    elif case.content == "hole":
        v[h // 3: h // 3 + max(1, h // 4), w // 3: w // 3 + max(1, w // 4)] = -1
    return v


def homography_of(case):
    h, w = case.h, case.w
    if case.homo == "identity":        # column 0 has weight 0, the last row and column have no taps
        return np.eye(3)
    if case.homo == "mild":            # like a real correction: a little shear and scale, a horizon tilted over the width
        return np.array([[1.02, 0.03, -0.4], [0.01, 0.98, 0.3], [0.05 / w, -0.03 / h, 1.0]])
    if case.homo == "shift":
        return np.array([[1, 0, SHIFT[0]], [0, 1, SHIFT[1]], [0, 0, 1.0]])
    if case.homo == "z0":              # z = j + i - k is 0 on a diagonal of pixels: x = +-inf there, NaN where j = w // 2 too
        return np.array([[1, 0, -(w // 2)], [0, 1, 0.5], [1, 1, -(w // 2 + 1.0)]])
    if case.homo == "zneg":            # z = j0 - j changes sign at the non-integer j0; x = w / 2 + 1.5 / z, y = 0.4 on both sides
        j0 = w / 2 - 0.75
        return np.array([[-w / 2, 0, w / 2 * j0 + 1.5], [-0.4, 0, 0.4 * j0], [-1, 0, j0]])
    if case.homo == "tiny":            # row 0 maps to y = -1e-50: below 0 as a double, -0.f as a float
        return np.array([[1, 0, 0.5], [0, 1, -1e-50], [0, 0, 1.0]])
    if case.homo == "outside":
        return np.array([[1, 0, w + 3.0], [0, 1, 0], [0, 0, 1.0]])
    raise AssertionError(case.homo)


def map_of(case):
    """(x, y, z) of every pixel, as the restatement computes them"""
    d = homography_of(case).reshape(9)
    i, j = np.meshgrid(np.arange(case.h, dtype=D), np.arange(case.w, dtype=D), indexing="ij")
    with np.errstate(all="ignore"):
        z = d[6] * j + d[7] * i + d[8]
        return (d[0] * j + d[1] * i + d[2]) * (1.0 / z), (d[3] * j + d[4] * i + d[5]) * (1.0 / z), z


# ---- synthetic bundles for the corner geometry -------------------------------------------------------------------------------
Bundle = collections.namedtuple("Bundle", "id n proj_min ref_wh first_wh first_homo last_wh last_homo canvas_wh")


def _rot(deg, tx, ty, g=0.0, h=0.0):
    a = np.deg2rad(deg)
    return np.array([[np.cos(a), -np.sin(a), tx], [np.sin(a), np.cos(a), ty], [g, h, 1.0]])


# ImageRef sizes (stale after the pre-warp) that differ from what a warped Mat would have; the homographies act on centred pixel
# coordinates as CylinderStitcher::build_warp leaves them
BUNDLES = [
    Bundle("two_views", 2, (-301.5, -203.25), (600, 400), (600, 400), np.eye(3), (600, 400), _rot(0.4, 431.7, 6.2, 1e-5, -2e-6), (1033, 412)),
    Bundle("four_views", 4, (-1290.125, -260.5), (640, 480), (612, 470), _rot(-1.1, -872.4, 11.3, -3e-5, 4e-6), (655, 491),
           _rot(0.8, 460.9, -7.7, 2e-5, 1e-6), (2101, 533)),
    Bundle("five_views_first_rotated", 5, (-9480.75, -1410.5), (4000, 3000), (3000, 4000), _rot(91.5, -7400.2, 40.6, -4e-6, 1e-6), (4000, 3000),
           _rot(-0.7, 7613.4, -55.1, 3e-6, -5e-7), (18803, 3390)),
]
# every corner on the line y = -proj_min.y: no homography maps a rectangle there
COLLINEAR = Bundle("collinear", 3, (-10.0, -20.0), (600, 400), (600, 400), np.array([[1, 0, -300.0], [0, 0, 0], [0, 0, 1.0]]), (600, 400),
                   np.array([[1, 0, 300.0], [0, 0, 0], [0, 0, 1.0]]), (900, 400))


def bundle_corners(b):
    return corners_ref(b.proj_min, b.ref_wh, b.first_wh, b.first_homo, b.last_wh, b.last_homo)
