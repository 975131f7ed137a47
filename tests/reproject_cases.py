"""The re-projection of a finished equirectangular panorama (op_canvas_reproject, csrc/reproject.hip) in numpy, and the cases its
kernel is held to.  No tests here: test_reproject_cpu.py proves that the restatement and the cases are what they claim,
test_gpu_reproject.py holds the device to them with np.array_equal.

Every function restates the kernel one operation per numpy call, so that nothing is fused, in float64 where the kernel is fp64
and np.float32 where it is fp32:
  pano_atan2            csrc/pano_angle.hpp: + - * / only; the kernel's angle IS this function
  interpolate_ref       interpolate (lib/imgproc.cc:135-156), Color::NO when a tap is NO
  interpolate_wrap_ref  the same for columns that close a full turn: bound c <= W, the right tap of column W - 1 reads column 0,
                        a c that narrowed to exactly W reads column 0 with fraction 0
  planet_ref            planet (main.cc:297-329) operation by operation; atan(q) is pano_atan2(q, 1)
  rectilinear_ref       a pinhole camera: d = rot (u, v, focal), lon = atan2(dx, dz), lat = atan2(dy, sqrt(dx dx + dz dz))
A frame is (lon0, lat0, step_lon, step_lat, wrap); a view is (out_h, out_w, rot[9], focal)."""
import collections
import zlib

import numpy as np

F = np.float32
D = np.float64
PI = D(float.fromhex("0x1.921fb54442d18p+1"))
PI_2 = D(float.fromhex("0x1.921fb54442d18p+0"))
TWO_PI = D(float.fromhex("0x1.921fb54442d18p+2"))

ATAN_TABLE = np.array([float.fromhex(s) for s in (
    "0x0p+0", "0x1.fd5ba9aac2f6ep-4", "0x1.f5b75f92c80ddp-3", "0x1.6f61941e4def1p-2", "0x1.dac670561bb4fp-2",
    "0x1.1e00babdefeb4p-1", "0x1.4978fa3269ee1p-1", "0x1.700a7c5784634p-1", "0x1.921fb54442d18p-1")], D)
# -1/15, 1/13, -1/11, 1/9, -1/7, 1/5, -1/3 as the correctly rounded doubles, then 1
ATAN_POLY = [D(float.fromhex(s)) for s in (
    "-0x1.1111111111111p-4", "0x1.3b13b13b13b14p-4", "-0x1.745d1745d1746p-4", "0x1.c71c71c71c71cp-4", "-0x1.2492492492492p-3",
    "0x1.999999999999ap-3", "-0x1.5555555555555p-2", "0x1p+0")]


def pano_atan2(y, x):
    y, x = np.broadcast_arrays(np.asarray(y, D), np.asarray(x, D))
    with np.errstate(all="ignore"):
        ax = np.where(x < 0, -x, x)
        ay = np.where(y < 0, -y, y)
        zero = (ax == 0) & (ay == 0)
        swap = ay > ax
        mn = np.where(swap, ax, ay)
        mx = np.where(swap, ay, ax)
        a = mn / np.where(zero, D(1), mx)
        k8 = a * D(8)
        k8 = k8 + D(0.5)
        k = np.where(np.isfinite(k8), np.floor(k8), 0).astype(np.int64)
        k = np.clip(k, 0, 8)                             # (a NaN in: any table entry, the result is NaN anyway)
        c = k.astype(D) * D(0.125)
        num = a - c
        den = a * c
        den = D(1) + den
        t = num / den
        s = t * t
        p = np.full(t.shape, ATAN_POLY[0], D)
        for coef in ATAN_POLY[1:]:
            p = p * s
            p = p + coef
        tp = t * p
        r = ATAN_TABLE[k] + tp
        r = np.where(swap, PI_2 - r, r)
        r = np.where(x < 0, PI - r, r)
        r = np.where(y < 0, -r, r)
        return np.where(zero, D(0), r)


def _taps(src, ir, ic, ir1, ic1, r, c, ok):
    one = F(1)
    nr = one - r
    nc = one - c
    p00, p10, p11, p01 = src[ir, ic], src[ir1, ic], src[ir1, ic1], src[ir, ic1]
    ok = ok & (p00[..., 0] >= 0) & (p10[..., 0] >= 0) & (p11[..., 0] >= 0) & (p01[..., 0] >= 0)
    col = np.zeros(r.shape + (3,), F)
    for p, wt in ((p00, nr * nc), (p10, r * nc), (p11, r * c), (p01, nr * c)):
        t = p * wt[..., None]
        col = col + t
    return col, ok


def interpolate_ref(src, r, c):
    """-> (colours, ok) at float32 coordinates r (row), c (column)"""
    H, W = src.shape[:2]
    r, c = np.asarray(r, F), np.asarray(c, F)
    with np.errstate(all="ignore"):
        ok = (r >= 0) & (c >= 0) & (r < F(H - 1)) & (c < F(W - 1))
        fr = np.floor(np.where(ok, r, 0))
        fc = np.floor(np.where(ok, c, 0))
        ir, ic = fr.astype(np.int64), fc.astype(np.int64)
        ir1, ic1 = np.minimum(ir + 1, H - 1), np.minimum(ic + 1, W - 1)         # (reached only where ok is False)
        return _taps(src, ir, ic, ir1, ic1, np.where(ok, r, 0) - fr, np.where(ok, c, 0) - fc, ok)


def interpolate_wrap_ref(src, r, c):
    H, W = src.shape[:2]
    r, c = np.asarray(r, F), np.asarray(c, F)
    with np.errstate(all="ignore"):
        ok = (r >= 0) & (c >= 0) & (r < F(H - 1)) & (c <= F(W))
        r, c = np.where(ok, r, F(0)), np.where(ok, c, F(0))
        fr = np.floor(r)
        fc = np.floor(c)
        r = r - fr
        c = c - fc
        ir, ic = fr.astype(np.int64), fc.astype(np.int64)
        full = ic >= W
        ic = np.where(full, 0, ic)
        c = np.where(full, F(0), c)
        ic1 = np.where(ic + 1 == W, 0, ic + 1)
        ir1 = np.minimum(ir + 1, H - 1)
        return _taps(src, ir, ic, ir1, ic1, r, c, ok)


def _finish(col, ok, shape):
    out = np.full(shape + (3,), F(-1), F)
    out[ok] = col[ok]
    return out


def planet_coords(H, W, n):
    """(r, c, live): the float32 coordinates planet hands to interpolate, and where it does (dist < center, dist != 0)"""
    center = n // 2
    i, j = np.meshgrid(np.arange(n, dtype=np.int64), np.arange(n, dtype=np.int64), indexing="ij")
    di, dj = center - i, center - j
    with np.errstate(all="ignore"):
        dist = np.sqrt((di * di + dj * dj).astype(D))
        live = ~((dist >= D(center)) | (dist == 0))
        dist = dist / D(center)
        t = dist * D(H)
        dist = D(H) - t
        q = di.astype(D) / dj.astype(D)
        theta = pano_atan2(q, D(1))
        theta = np.where(theta < 0, theta + PI, theta)
        theta = np.where((theta == 0) & (j > center), theta + PI, theta)
        theta = np.where(center < i, theta + PI, theta)
        three_half = D(3) * PI
        three_half = three_half / D(2)
        theta = np.where(j == center, np.where(i < center, PI / D(2), three_half), theta)
        theta = theta / (PI * D(2))
        theta = theta * D(W)
        dist = np.where(D(H - 1) < dist, D(H - 1), dist)
        return dist.astype(F), theta.astype(F), live


def planet_ref(src, n, wrap):
    src = np.ascontiguousarray(src, F)
    H, W = src.shape[:2]
    if H == 0 or W == 0:
        return np.full((n, n, 3), F(-1), F)
    r, c, live = planet_coords(H, W, n)
    col, ok = (interpolate_wrap_ref if wrap else interpolate_ref)(src, r, c)
    return _finish(col, ok & live, (n, n))


def rectilinear_coords(H, W, frame, view):
    """(py, px, live): the doubles the kernel narrows, and where its own bounds let them through"""
    lon0, lat0, step_lon, step_lat, wrap = frame
    out_h, out_w, rot, focal = view
    R = np.asarray(rot, D).reshape(9)
    focal = D(focal)
    i, j = np.meshgrid(np.arange(out_h, dtype=D), np.arange(out_w, dtype=D), indexing="ij")
    with np.errstate(all="ignore"):
        u = j - D(0.5) * D(out_w - 1)
        v = i - D(0.5) * D(out_h - 1)

        def row(a, b, c):
            t = R[a] * u
            t = t + R[b] * v
            return t + R[c] * focal
        dx, dy, dz = row(0, 1, 2), row(3, 4, 5), row(6, 7, 8)
        lon = pano_atan2(dx, dz)
        hyp = dx * dx
        hyp = hyp + dz * dz
        hyp = np.sqrt(hyp)
        lat = pano_atan2(dy, hyp)
        py = lat - D(lat0)
        py = py / D(step_lat)
        if wrap:
            d = lon - D(lon0)
            d = np.where(d < 0, d + TWO_PI, d)
            d = np.where(d >= TWO_PI, d - TWO_PI, d)
            px = d / (PI * D(2))
            px = px * D(W)
            live = ~((py < 0) | (py >= H)) & ~np.isnan(px)
        else:
            px = lon - D(lon0)
            px = px / D(step_lon)
            live = ~((px < 0) | (px >= W) | (py < 0) | (py >= H)) & ~np.isnan(px)
    return py, px, live


def rectilinear_ref(src, frame, view):
    src = np.ascontiguousarray(src, F)
    H, W = src.shape[:2]
    out_h, out_w = view[0], view[1]
    if H == 0 or W == 0:
        return np.full((out_h, out_w, 3), F(-1), F)
    py, px, live = rectilinear_coords(H, W, frame, view)
    col, ok = (interpolate_wrap_ref if frame[4] else interpolate_ref)(src, py.astype(F), px.astype(F))
    return _finish(col, ok & live, (out_h, out_w))


def look_rot(yaw, pitch, roll):
    """op_view_look's matrix with numpy's cos / sin: R_yaw (about y) R_pitch (about x) R_roll (about z)"""
    cy, sy, cp, sp, cr, sr = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]], D)
    Rx = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]], D)
    Rz = np.array([[cr, -sr, 0], [sr, cr, 0], [0, 0, 1]], D)
    return Ry @ Rx @ Rz


# face 0..5 = +x, -x, +y, -y, +z, -z: (the matrix, the direction of the picture's centre, the direction of its top)
CUBE = [
    ([0, 0, 1, 0, 1, 0, -1, 0, 0], (1, 0, 0), (0, -1, 0)),
    ([0, 0, -1, 0, 1, 0, 1, 0, 0], (-1, 0, 0), (0, -1, 0)),
    ([1, 0, 0, 0, 0, 1, 0, -1, 0], (0, 1, 0), (0, 0, 1)),
    ([1, 0, 0, 0, 0, -1, 0, 1, 0], (0, -1, 0), (0, 0, -1)),
    ([1, 0, 0, 0, 1, 0, 0, 0, 1], (0, 0, 1), (0, -1, 0)),
    ([-1, 0, 0, 0, 1, 0, 0, 0, -1], (0, 0, -1), (0, -1, 0)),
]


def cube_view(face, n):
    return (n, n, np.array(CUBE[face][0], D), D(0.5) * D(n))


# ---- the cases -------------------------------------------------------------------------------------------------------------
# sources: one tile and less, no second row (every pixel NO), a width one past four 64-column tiles, odd sizes, and a full sphere
SOURCES = [(2, 2), (1, 7), (5, 257), (37, 53), (16, 32)]
SPHERE = (16, 32)
CONTENTS = ("random", "border", "hole")
# outputs: tile edges either side (64 x 4 tiles)
OUTPUTS = [(1, 1), (2, 2), (4, 64), (5, 65), (63, 130)]
PLANETS = [1, 2, 7, 64]
CUBE_N = 8
TINY = 1e-9                      # a longitude this far left of lon0 lies at px = W (1 - 1.6e-10): it narrows to exactly W


def source_of(hw, content):
    """random colours in [0, 1); "border": Color::NO one pixel wide all round; "hole": a block of Color::NO inside"""
    h, w = hw
    v = np.random.default_rng(zlib.crc32(("reproject %dx%d" % (h, w)).encode())).random((h, w, 3), dtype=F)
    if content == "border":
        keep = np.zeros((h, w), bool)
        keep[1:-1, 1:-1] = True
        v[~keep] = -1
    elif content == "hole":
        v[h // 3: h // 3 + max(1, h // 4), w // 3: w // 3 + max(1, w // 4)] = -1
    return v


def frame_of(hw, wrap, lon0=None):
    """the sphere covers every direction (lat0 = -pi/2, step_lat = pi/15, a turn of columns from -pi); the others are partial
    panoramas of 1.4 x 0.8 rad about the forward direction.  lon0 overrides where column 0 lies."""
    h, w = hw
    if hw == SPHERE:
        f = [-PI, -PI_2, TWO_PI / D(w), PI / D(15), int(wrap)]
    else:
        f = [D(-0.7), D(-0.4), D(1.4) / D(w), D(0.8) / D(h), int(wrap)]
    if lon0 is not None:
        f[0] = D(lon0)
    return tuple(f)


# name -> (yaw, pitch, roll, hfov, lon0 override or None); "seam_*" are built from the frame's lon0 in looks_of
LOOKS = collections.OrderedDict([
    ("identity", (0.0, 0.0, 0.0, 1.2, None)),
    ("yaw_pi", (np.pi, 0.0, 0.0, 1.2, None)),                    # the +-pi seam of atan2 runs down the middle
    ("up", (0.0, np.pi / 2, 0.0, 1.2, None)),                     # dx = dz = 0 at the centre pixel of an odd output
    ("down", (0.0, -np.pi / 2, 0.0, 1.2, None)),
    ("roll", (0.2, 0.1, 0.7, 1.0, None)),
    ("narrow", (0.1, -0.05, 0.0, 0.1, None)),
    ("wide", (-0.2, 0.1, 0.0, 3.0, None)),
    ("outside", (2.5, 0.0, 0.0, 0.3, None)),                      # wholly outside a partial panorama
    ("lon0_plus_pi", (np.pi, 0.0, 0.0, 1.2, float(PI))),
    ("lon0_minus_pi", (-np.pi, 0.1, 0.0, 1.2, -float(PI))),
    ("seam_last_column", None),                                   # the centre looks at px = W - 0.5: in [W - 1, W)
    ("seam_exactly_w", None),                                     # the centre looks TINY left of lon0: px narrows to W
])


def looks_of(hw, wrap):
    """[(name, yaw, pitch, roll, hfov, frame)] for a source"""
    out = []
    for name, spec in LOOKS.items():
        if spec is None:
            f = frame_of(hw, wrap)
            step = TWO_PI / D(hw[1]) if wrap else f[2]
            first = f[0] if wrap else f[0] + D(hw[1]) * f[2]       # the longitude of column W: lon0 again under wrap
            yaw = float(first - D(0.5) * step) if name == "seam_last_column" else float(first - D(TINY))
            pitch = 0.0 if hw != SPHERE else 0.0
            out.append((name, yaw, pitch, 0.0, 0.2, f))
        else:
            yaw, pitch, roll, hfov, lon0 = spec
            out.append((name, yaw, pitch, roll, hfov, frame_of(hw, wrap, lon0)))
    return out
