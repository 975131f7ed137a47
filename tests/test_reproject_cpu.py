"""CPU: the re-projection's angle function, host helpers and numpy restatement (tests/reproject_cases.py) are what they claim.

The C side -- csrc/pano_angle.hpp and the host-only entry points of csrc/blend_geom.cc -- runs as a program of its own under
AddressSanitizer and UndefinedBehaviorSanitizer (tests/harness/reproject_harness.cc); nothing here needs a device.  The same
program holds a C++ twin of the kernel's per-pixel code, which must equal the restatement bit for bit."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import reproject_cases as rc
from openpano_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "openpano_amd", "csrc")
CLI_CPU = os.path.join(ROOT, "oracle", "_ref", "image-stitching")
D, F = np.float64, np.float32
ANGLE_BOUND = 4e-15                     # the contract of pano_atan2 (csrc/pano_angle.hpp)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ missing")
    exe = str(tmp_path_factory.mktemp("reproject") / "reproject_harness")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                           "-Wall", "-Wno-unknown-pragmas", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                           os.path.join(ROOT, "tests", "harness", "reproject_harness.cc"), os.path.join(CSRC, "blend_geom.cc"), "-o", exe])

    def run(*args):
        r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
        assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
        return r.stdout
    return run


def angle_inputs():
    """(y, x): a million random pairs over many magnitudes, the axes, tiny magnitudes, the integer grid"""
    rng = np.random.default_rng(20)
    n = 1 << 20
    parts = [rng.standard_normal((n // 2, 2)),
             rng.standard_normal((n // 4, 2)) * 10.0 ** rng.uniform(-12, 12, (n // 4, 2)),
             rng.standard_normal((n // 8, 2)) * 1e-300,                                  # tiny, subnormal quotients included
             rng.standard_normal((n // 8, 2)) * np.array([1e-308, 1.0])]
    v = np.array([0.0, 1.0, -1.0, 2.5, -2.5, 1e-310, -1e-310, 1e300, -1e300])
    parts.append(np.stack(np.meshgrid(v, v), -1).reshape(-1, 2))                      # the axes and (0, 0)
    g = np.arange(-500, 501, dtype=D)
    parts.append(np.stack(np.meshgrid(g, g), -1).reshape(-1, 2))                      # the 1001^2 integer grid
    yx = np.concatenate(parts)
    return np.ascontiguousarray(yx[:, 0]), np.ascontiguousarray(yx[:, 1])


def test_pano_atan2_is_within_its_bound_of_atan2():
    y, x = angle_inputs()
    assert len(y) >= 1 << 20
    got = rc.pano_atan2(y, x)
    err = np.abs(got - np.arctan2(y, x))
    print("pano_atan2: max |error| = %.3g rad over %d pairs" % (err.max(), len(y)))
    assert err.max() <= ANGLE_BOUND
    assert rc.pano_atan2(0.0, 0.0) == 0 and not np.signbit(rc.pano_atan2(0.0, 0.0))
    assert rc.pano_atan2(0.0, -1.0) == rc.PI and rc.pano_atan2(1.0, 0.0) == rc.PI_2 and rc.pano_atan2(-1.0, 0.0) == -rc.PI_2
    assert rc.pano_atan2(1.0, 1.0) == rc.ATAN_TABLE[8]


def test_c_pano_atan2_equals_numpy_bit_for_bit(harness, tmp_path):
    y, x = angle_inputs()
    np.stack([y, x], 1).tofile(str(tmp_path / "in.bin"))
    harness("atan2", tmp_path / "in.bin", tmp_path / "out.bin")
    got = np.fromfile(str(tmp_path / "out.bin"), D)
    want = rc.pano_atan2(y, x)
    assert got.shape == want.shape and got.tobytes() == want.tobytes()


def _hex(v):
    return float(v).hex() if np.isfinite(v) else str(float(v))


def _spec_line(frame, view, mode):
    out_h, out_w, rot, focal = view
    return [_hex(frame[0]), _hex(frame[1]), _hex(frame[2]), _hex(frame[3]), int(frame[4]), mode, out_h, out_w, _hex(focal)] + [_hex(r) for r in np.asarray(rot).reshape(9)]


def _helpers(harness, tmp_path, lines):
    p = tmp_path / "helpers.txt"
    p.write_text("\n".join(" ".join(str(t) for t in ln) for ln in lines) + "\n")
    out = harness("helpers", p).splitlines()
    assert out[-1] == "reproject_harness: helpers done" and len(out) == len(lines) + 1
    return [ln.split(" ") for ln in out[:-1]]


def _parse_spec(w):
    return dict(rc=int(w[0]), mode=int(w[1]), out_h=int(w[2]), out_w=int(w[3]), focal=float.fromhex(w[4]), rot=np.array([float.fromhex(t) for t in w[5:14]]))


LOOK_ARGS = [(0.0, 0.0, 0.0, 1.2, 64, 48), (np.pi, 0.0, 0.0, 1.2, 5, 65), (0.3, -0.4, 0.7, 0.1, 130, 63), (-2.9, 1.5, -3.0, 3.0, 1, 1),
             (0.0, np.pi / 2, 0.0, 1.0, 7, 7)]


def test_view_helpers_against_numpy(harness, tmp_path):
    lines = [["look"] + [_hex(a) for a in args[:4]] + list(args[4:]) for args in LOOK_ARGS]
    lines += [["cube", f, rc.CUBE_N] for f in range(6)] + [["planet", 64]]
    res = [_parse_spec(w) for w in _helpers(harness, tmp_path, lines)]
    for args, s in zip(LOOK_ARGS, res):
        yaw, pitch, roll, hfov, w, h = args
        assert (s["rc"], s["mode"], s["out_h"], s["out_w"]) == (0, hip.VIEW_RECTILINEAR, h, w)
        R = s["rot"].reshape(3, 3)
        assert np.abs(R - rc.look_rot(yaw, pitch, roll)).max() <= 1e-15
        assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-15 and abs(np.linalg.det(R) - 1) <= 1e-15
        assert abs(s["focal"] - 0.5 * w / np.tan(0.5 * hfov)) <= 4e-16 * s["focal"]
        # the optical axis: positive yaw looks right, positive pitch looks up (-y)
        assert np.abs(R[:, 2] - [np.sin(yaw) * np.cos(pitch), -np.sin(pitch), np.cos(yaw) * np.cos(pitch)]).max() <= 1e-15
    for f, s in enumerate(res[len(LOOK_ARGS):-1]):
        assert (s["rc"], s["mode"], s["out_h"], s["out_w"], s["focal"]) == (0, hip.VIEW_RECTILINEAR, rc.CUBE_N, rc.CUBE_N, 0.5 * rc.CUBE_N)
        R = s["rot"].reshape(3, 3)
        assert np.array_equal(s["rot"], np.array(rc.CUBE[f][0], D))             # exact: entries 0, 1, -1
        assert np.array_equal(R @ R.T, np.eye(3)) and np.linalg.det(R) == 1
        assert np.array_equal(R[:, 2], rc.CUBE[f][1]) and np.array_equal(-R[:, 1], rc.CUBE[f][2])   # centre and top of the picture
    s = res[-1]
    assert (s["rc"], s["mode"], s["out_h"], s["out_w"]) == (0, hip.VIEW_PLANET, 64, 64) and np.array_equal(s["rot"].reshape(3, 3), np.eye(3))


def test_pano_frame_of_is_its_formula(harness, tmp_path):
    minx, miny, resx, resy = -2.7182818284590451, -0.61803398874989479, 0.0007853981633974483, 0.00078125
    lines = [["frame", 2, _hex(minx), _hex(miny), _hex(resx), _hex(resy), x0, y0] for x0, y0 in ((0, 0), (17, 3), (7998, 762))]
    lines += [["frame", m, _hex(minx), _hex(miny), _hex(resx), _hex(resy), 0, 0] for m in (0, 1)]
    res = _helpers(harness, tmp_path, lines)
    for (x0, y0), w in zip(((0, 0), (17, 3), (7998, 762)), res):
        got = [float.fromhex(t) for t in w[1:5]]
        assert int(w[0]) == 0 and int(w[5]) == 0                            # wrap is never guessed
        assert got == [D(minx) + D(x0) * D(resx), D(miny) + D(y0) * D(resy), resx, resy]
    assert [int(w[0]) for w in res[3:]] == [-4, -4]                          # OP_ERR_UNSUPPORTED: flat, cylindrical


def test_every_refusal_is_refused(harness, tmp_path):
    nan, inf = float("nan"), float("inf")
    lines = [["look", _hex(nan), 0, 0, 1, 4, 4], ["look", 0, _hex(inf), 0, 1, 4, 4], ["look", 0, 0, _hex(-inf), 1, 4, 4],
             ["look", 0, 0, 0, 0, 4, 4], ["look", 0, 0, 0, _hex(np.pi), 4, 4], ["look", 0, 0, 0, _hex(nan), 4, 4], ["look", 0, 0, 0, -1, 4, 4],
             ["look", 0, 0, 0, 1, 0, 4], ["look", 0, 0, 0, 1, 4, 0],
             ["cube", -1, 4], ["cube", 6, 4], ["cube", 0, 0], ["planet", 0], ["planet", -3]]
    assert [int(w[0]) for w in _helpers(harness, tmp_path, lines)] == [-1] * len(lines)
    good_f = (-0.7, -0.4, 0.01, 0.02, 0)
    good_v = (4, 4, np.eye(3), 2.0)
    bad = []
    for k in range(4):
        for v in (nan, inf):
            f = list(good_f); f[k] = v
            bad.append((f, good_v, 1, "not finite"))
    bad.append((good_f, (4, 4, np.eye(3), nan), 1, "not finite"))
    for k in range(9):
        r = np.eye(3).reshape(9).copy(); r[k] = -inf
        bad.append((good_f, (4, 4, r, 2.0), 1, "not finite"))
    bad += [(good_f, (4, 4, np.eye(3), 0.0), 1, "focal"), (good_f, (4, 4, np.eye(3), -1.0), 1, "focal"),
            (good_f, (0, 4, np.eye(3), 2.0), 1, "size below 1"), (good_f, (4, 0, np.eye(3), 2.0), 0, "size below 1"),
            (good_f, (4, 5, np.eye(3), 2.0), 0, "square"), (good_f, good_v, 2, "unknown mode"), (good_f, good_v, -1, "unknown mode"),
            ((-0.7, -0.4, 0.0, 0.02, 0), good_v, 1, "step is zero"), ((-0.7, -0.4, 0.01, 0.0, 0), good_v, 1, "step is zero"),
            ((-0.7, -0.4, 0.01, 0.0, 1), good_v, 1, "step is zero"), ((-0.7, -0.4, 0.01, 0.02, 2), good_v, 1, "wrap is neither"),
            ((3.1415926535897936, -0.4, 0.01, 0.02, 1), good_v, 1, "lon0 outside"), ((-3.2, -0.4, 0.01, 0.02, 1), good_v, 1, "lon0 outside")]
    res = _helpers(harness, tmp_path, [["check"] + _spec_line(f, v, m) for f, v, m, _ in bad])
    for (f, v, m, what), w in zip(bad, res):
        assert int(w[0]) == -1 and what in " ".join(w[1:]), (f, m, w)
    ok = [(good_f, good_v, 0), (good_f, good_v, 1), ((-0.7, -0.4, 0.0, 0.02, 1), good_v, 1), ((float(rc.PI), -0.4, 0.01, 0.02, 1), good_v, 1),
          ((-float(rc.PI), -0.4, 0.01, -0.02, 1), good_v, 0), ((7.0, -0.4, -0.01, 0.02, 0), good_v, 1)]
    assert [int(w[0]) for w in _helpers(harness, tmp_path, [["check"] + _spec_line(f, v, m) for f, v, m in ok])] == [0] * len(ok)


def test_struct_layouts_match_header(tmp_path):
    """OpPanoFrame and OpViewSpec against the header, as test_binding_header_cpu.py::test_struct_layouts_match_header does"""
    cc = shutil.which("gcc") or shutil.which("cc")
    if not cc:
        pytest.skip("no C compiler")
    structs = [("op_pano_frame", hip.OpPanoFrame, ["lon0", "lat0", "step_lon", "step_lat", "wrap"]),
               ("op_view_spec", hip.OpViewSpec, ["mode", "out_h", "out_w", "rot", "focal"])]
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "openpano_hip.h"', "int main(void) {"]
    for cname, _, members in structs:
        lines.append('printf("%s sizeof %%zu\\n", sizeof(%s));' % (cname, cname))
        for m in members:
            lines.append('printf("%s %s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));' % (cname, m, cname, m, cname, m))
    lines += ['printf("modes %d %d\\n", OP_VIEW_PLANET, OP_VIEW_RECTILINEAR);', "return 0;", "}"]
    src, exe = str(tmp_path / "layout.c"), str(tmp_path / "layout")
    with open(src, "w") as f:
        f.write("\n".join(lines) + "\n")
    subprocess.check_call([cc, "-std=c99", "-I" + os.path.join(ROOT, "include"), src, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60, check=True).stdout.split("\n")
    want = {}
    for line in out:
        w = line.split()
        if len(w) == 3:
            want[w[0]] = (int(w[1]), int(w[2])) if w[0] == "modes" else int(w[2])
        elif len(w) == 4:
            want[w[0], w[1]] = (int(w[2]), int(w[3]))
    assert want["modes"] == (hip.VIEW_PLANET, hip.VIEW_RECTILINEAR)
    for cname, cls, members in structs:
        assert [n for n, _ in cls._fields_] == members, cname
        assert C.sizeof(cls) == want[cname], cname
        for m in members:
            field = getattr(cls, m)
            assert (field.offset, field.size) == want[cname, m], (cname, m)


# ---- properties of the restatement ---------------------------------------------------------------------------------------------
def test_cube_faces_cover_a_full_sphere():
    """16 x 32 full sphere with wrap: every cube-face pixel whose latitude row has both taps is sampled"""
    src = rc.source_of(rc.SPHERE, "random")
    frame = rc.frame_of(rc.SPHERE, 1)
    H, W = rc.SPHERE
    seen = 0
    for face in range(6):
        view = rc.cube_view(face, rc.CUBE_N)
        py, px, live = rc.rectilinear_coords(H, W, frame, view)
        inside = (py.astype(F) >= 0) & (py.astype(F) < F(H - 1))
        assert live.all() and (px >= 0).all() and (px <= W).all()
        out = rc.rectilinear_ref(src, frame, view)
        assert np.array_equal(out[..., 0] >= 0, inside)
        assert inside.all()                               # an even face has no pixel at a pole
        seen += inside.sum()
    assert seen == 6 * rc.CUBE_N * rc.CUBE_N


def test_cube_face_centres_look_along_the_axes():
    frame = rc.frame_of(rc.SPHERE, 1)
    H, W = rc.SPHERE
    want = [(rc.PI_2, 0.0), (-rc.PI_2, 0.0), (None, rc.PI_2), (None, -rc.PI_2), (0.0, 0.0), (rc.PI, 0.0)]     # (lon, lat); y is down
    for face, (lon, lat) in enumerate(want):
        py, px, _ = rc.rectilinear_coords(H, W, frame, rc.cube_view(face, 9))
        assert py[4, 4] == (D(lat) - frame[1]) / frame[3]
        if lon is not None:
            d = D(lon) - frame[0]
            d = d - rc.TWO_PI if d >= rc.TWO_PI else d
            assert px[4, 4] == d / rc.TWO_PI * W


def test_planet_seam_without_wrap_and_none_with():
    src = rc.source_of((37, 53), "random")
    H, W = src.shape[:2]
    n = 64
    r, c, live = rc.planet_coords(H, W, n)
    rows = live & (r >= 0) & (r < F(H - 1))
    assert rows.sum() > 0.7 * 3.14 * 32 * 32
    plain = rc.planet_ref(src, n, 0)[..., 0] >= 0
    wrapped = rc.planet_ref(src, n, 1)[..., 0] >= 0
    seam = rows & (c >= F(W - 1))
    assert seam.sum() > 10                                       # the reference's one-column seam of Color::NO
    assert np.array_equal(plain, rows & ~seam)
    assert np.array_equal(wrapped, rows)
    # outside the seam both samplers read the same taps
    both = rows & ~seam
    assert np.array_equal(rc.planet_ref(src, n, 0)[both], rc.planet_ref(src, n, 1)[both])


def test_seam_cases_are_what_they_claim():
    for hw in rc.SOURCES:
        for wrap in (0, 1):
            looks = {lk[0]: lk for lk in rc.looks_of(hw, wrap)}
            for name, lo, hi in (("seam_last_column", hw[1] - 1, hw[1]), ("seam_exactly_w", hw[1], hw[1])):
                _, yaw, pitch, roll, hfov, frame = looks[name]
                view = (5, 65, rc.look_rot(yaw, pitch, roll).reshape(9), 0.5 * 65 / np.tan(0.5 * hfov))
                py, px, live = rc.rectilinear_coords(hw[0], hw[1], frame, view)
                c = px.astype(F)[2, 32]
                assert px[2, 32] < hw[1] and lo <= c <= hi and (c == hw[1]) == (name == "seam_exactly_w"), (hw, wrap, name, px[2, 32])
    # the wrapped sampler at c = W reads column 0 alone, and right of the last column it blends with column 0
    src = rc.source_of((5, 257), "random")
    col, ok = rc.interpolate_wrap_ref(src, np.array([1.0], F), np.array([257.0], F))
    assert ok[0] and np.array_equal(col[0], src[1, 0])
    col, ok = rc.interpolate_wrap_ref(src, np.array([1.0], F), np.array([256.5], F))
    assert ok[0] and np.array_equal(col[0], F(0.5) * src[1, 256] + F(0.5) * src[1, 0])
    assert not rc.interpolate_ref(src, np.array([1.0], F), np.array([256.5], F))[1][0]
    assert not rc.interpolate_wrap_ref(src, np.array([1.0], F), np.array([257.5], F))[1][0]


def test_outside_view_sees_nothing_of_a_partial_panorama():
    looks = {lk[0]: lk for lk in rc.looks_of((37, 53), 0)}
    _, yaw, pitch, roll, hfov, frame = looks["outside"]
    view = (63, 130, rc.look_rot(yaw, pitch, roll).reshape(9), 0.5 * 130 / np.tan(0.5 * hfov))
    assert not rc.rectilinear_coords(37, 53, frame, view)[2].any()
    _, yaw, pitch, roll, hfov, frame = looks["identity"]
    view = (63, 130, rc.look_rot(yaw, pitch, roll).reshape(9), 0.5 * 130 / np.tan(0.5 * hfov))
    assert (rc.rectilinear_ref(rc.source_of((37, 53), "random"), frame, view)[..., 0] >= 0).mean() > 0.3


# ---- the C++ twin of the kernel equals the restatement ---------------------------------------------------------------------------
def _render(harness, tmp_path, src, frame, view, mode):
    src.tofile(str(tmp_path / "src.bin"))
    harness("render", tmp_path / "src.bin", src.shape[0], src.shape[1], tmp_path / "out.bin", *_spec_line(frame, view, mode))
    return np.fromfile(str(tmp_path / "out.bin"), F).reshape(view[0], view[1], 3)


def test_host_twin_equals_the_restatement(harness, tmp_path):
    for hw, content in (((37, 53), "hole"), (rc.SPHERE, "border"), ((5, 257), "random")):
        src = rc.source_of(hw, content)
        for wrap in (0, 1):
            for n in (7, 64):
                view = (n, n, np.eye(3).reshape(9), 1.0)
                assert np.array_equal(_render(harness, tmp_path, src, rc.frame_of(hw, wrap), view, 0), rc.planet_ref(src, n, wrap)), (hw, wrap, n)
            for name, yaw, pitch, roll, hfov, frame in rc.looks_of(hw, wrap):
                view = (5, 65, rc.look_rot(yaw, pitch, roll).reshape(9), 0.5 * 65 / np.tan(0.5 * hfov))
                assert np.array_equal(_render(harness, tmp_path, src, frame, view, 1), rc.rectilinear_ref(src, frame, view)), (hw, wrap, name)
            for face in range(6):
                view = rc.cube_view(face, rc.CUBE_N)
                assert np.array_equal(_render(harness, tmp_path, src, rc.frame_of(hw, wrap), view, 1), rc.rectilinear_ref(src, rc.frame_of(hw, wrap), view))


# ---- against the reference's own planet -------------------------------------------------------------------------------------------
def test_planet_against_the_reference_cli(tmp_path):
    """image-stitching planet pano.png on a 64 x 256 random-byte panorama: its planet.png (1000 x 1000) against planet_ref
    quantised by the library's rule (NO -> white, v * 255 truncated).  The two differ only in the last ulp of atan / hypot: every
    byte within one level and more than 0.999 of them equal, the bound the project holds between two builds that differ in the
    last digits of a coordinate."""
    if not os.path.exists(CLI_CPU):
        pytest.skip("oracle/_ref/image-stitching not built (reference sources absent at build time)")
    from PIL import Image
    from openpano_amd.config import DEFAULTS
    pano = np.random.default_rng(64256).integers(0, 256, (64, 256, 3), dtype=np.uint8)
    Image.fromarray(pano).save(str(tmp_path / "pano.png"))
    with open(tmp_path / "config.cfg", "w") as f:
        for k, v in DEFAULTS.items():
            f.write(f"{k} {v}\n")
    env = dict(os.environ)
    env["OMP_NUM_THREADS"] = "1"
    r = subprocess.run([CLI_CPU, "planet", str(tmp_path / "pano.png")], capture_output=True, text=True, env=env, timeout=900, cwd=str(tmp_path))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    ref = np.asarray(Image.open(tmp_path / "planet.png").convert("RGB"))
    assert ref.shape == (1000, 1000, 3)
    src = (pano.astype(D) / 255.0).astype(F)                    # read_img (lib/imgio.cc:78-80)
    want = rc.planet_ref(src, 1000, 0)
    want = (np.where(want < 0, F(1), want) * F(255)).astype(np.uint8)       # canvas_byte
    diff = np.abs(ref.astype(int) - want.astype(int))
    share = (diff == 0).mean()
    print("planet against the reference: %d of %d bytes differ, largest difference %d" % ((diff != 0).sum(), diff.size, diff.max()))
    assert diff.max() <= 1 and share > 0.999
