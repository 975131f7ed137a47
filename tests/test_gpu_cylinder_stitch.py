"""GPU: CYLINDER mode standalone -- `stitch_demo ... cylinder` (HipCylinderStitcher, openpano_amd/host/pano_hip.hh) on natural-texture
views: BASELINE config 1 (2 views), 4 views of config 2 and a 5-view ordered sweep.  Per case: the panorama is the numpy restatement
of the perspective correction applied to the blend the program wrote (bit for bit), the corners are the restated to_ref_coor's, the
run with resident views and the run from JPEG files equal the plain run byte for byte, the cropped JPEG has the oracle's crop size,
`cylinder_build` (build(), the Mat32f hook, build_canvas(crop)) gives the staged run's panorama and files,
and -- where the reference's own CLI was built -- size, h-factor search, crop and pixels are the reference's."""
import os
import struct
import subprocess

import numpy as np
import pytest

import natural
import perspective_cases as pc
from openpano_amd.config import PanoConfig

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMO = os.path.join(ROOT, "openpano_amd", "host", "stitch_demo")
CLI_CPU = os.path.join(ROOT, "oracle", "_ref", "image-stitching")
SEED = 38
CFG = dict(CYLINDER=1, ESTIMATE_CAMERA=0, ORDERED_INPUT=1, LAZY_READ=0)


# The 5-view ordered sweep: on the first five views of config 2 the reference CPU CLI prints three `slope:` lines (0.014949,
# -0.009283, 0.002835: the first h-factor leaves a slope above SLOPE_PLAIN, the step overshoots, the third attempt wins at 0.9);
# the first four views take two attempts.
CASES = {"config1_2": lambda: natural.config_views(1, 2), "config2_4": lambda: natural.config_views(2, 4), "sweep_5": lambda: natural.config_views(2, 5)}
SEARCHES = "sweep_5"            # the case that must take two or more update_h_factor attempts


class _Reader:
    def __init__(self, buf):
        self.b = buf; self.o = 0

    def take(self, dtype, n):
        a = np.frombuffer(self.b, dtype=dtype, count=n, offset=self.o).copy()
        self.o += a.nbytes
        return a


def _parse(buf):
    rd = _Reader(buf)
    out = {}
    n = out["n"] = int(rd.take(np.int32, 1)[0])
    out["kp"] = []
    for _ in range(n):
        k = int(rd.take(np.int32, 1)[0])
        out["kp"].append(rd.take(np.float64, 2 * k).reshape(k, 2))
    na = int(rd.take(np.int32, 1)[0])
    out["attempts"] = []
    for _ in range(na):
        factor, slope = (float(x) for x in rd.take(np.float32, 2))
        out["attempts"].append((factor, slope, int(rd.take(np.int32, 1)[0])))
    out["best"] = float(rd.take(np.float32, 1)[0])
    out["homo"] = rd.take(np.float64, 9 * n).reshape(n, 3, 3)
    h, w = (int(x) for x in rd.take(np.int32, 2))
    out["pre"] = rd.take(np.float32, h * w * 3).reshape(h, w, 3)
    out["corners"] = rd.take(np.float64, 8).reshape(4, 2)
    out["inv"] = rd.take(np.float64, 9).reshape(3, 3)
    h, w = (int(x) for x in rd.take(np.int32, 2))
    out["final"] = rd.take(np.float32, h * w * 3).reshape(h, w, 3)
    assert rd.o == len(buf)
    return out


def _write_in_bin(path, views_u8):
    h, w = views_u8[0].shape[:2]
    with open(path, "wb") as f:
        f.write(struct.pack("<3i", len(views_u8), h, w))
        for v in views_u8:
            f.write(natural.u8_to_f32(v).tobytes())


def _demo(args):
    assert os.path.exists(DEMO), "build it: make -C openpano_amd/csrc"
    r = subprocess.run([DEMO] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stderr


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """the plain run of every case, once: (views, out.bin bytes, stderr, directory)"""
    if not natural.available():
        pytest.skip("tests/golden/natural or PIL missing")
    cache = {}

    def get(name):
        if name not in cache:
            d = tmp_path_factory.mktemp(name)
            views = CASES[name]()
            _write_in_bin(d / "in.bin", views)
            err = _demo([d / "in.bin", d / "out.bin", SEED, "cylinder", "--png", d / "plain.png"])
            cache[name] = (views, open(d / "out.bin", "rb").read(), err, d)
        return cache[name]
    return get


@pytest.mark.parametrize("name", list(CASES))
def test_panorama_is_the_restated_correction_of_the_blend(runs, name):
    from openpano_amd import hip
    views, buf, err, d = runs(name)
    o = _parse(buf)
    n, (h, w) = len(views), views[0].shape[:2]
    assert o["n"] == n and all(len(k) > 100 for k in o["kp"])
    assert o["pre"].shape == o["final"].shape and o["pre"].shape[0] > 100 and o["pre"].shape[1] > w
    want = pc.perspective_ref(o["pre"], o["inv"], 1, 0)
    assert np.array_equal(o["final"], want), int((o["final"] != want).any(axis=2).sum())
    valid = o["final"][..., 0] >= 0
    assert valid.mean() > 0.5 and (o["pre"][..., 0] >= 0).mean() > 0.5
    # the corners: to_ref_coor restated, on the geometry the bundle's homographies give
    mid = n >> 1
    assert np.array_equal(o["homo"][mid], np.eye(3))
    cfg = PanoConfig(**CFG)
    g, _, _ = hip.blend_prepare(cfg, [(w, h)] * n, o["homo"], 0, mid)
    proj_min = (g.proj_min[0], g.proj_min[1])
    ch, cw = o["pre"].shape[:2]
    assert np.array_equal(o["corners"], pc.corners_ref(proj_min, (w, h), (w, h), o["homo"][0], (w, h), o["homo"][-1]))
    inv, corners = hip.perspective_homography(g, (w, h), (w, h), o["homo"][0], (w, h), o["homo"][-1], (cw, ch))
    assert np.array_equal(inv, o["inv"]) and np.array_equal(corners, o["corners"])
    assert np.abs(pc.apply_homography(o["inv"], pc.corners_std((cw, ch))) - o["corners"]).max() < 1e-6
    # the search: none for two views, and the attempts the program reports are the lines it printed
    slopes = [ln for ln in err.splitlines() if ln.startswith("slope:")]
    assert len(slopes) == len([a for a in o["attempts"] if a[2]])
    if n == 2:
        assert o["attempts"] == [] and o["best"] == 1.0
    else:
        assert o["attempts"] and o["attempts"][0][0] == 1.0 and o["best"] in [a[0] for a in o["attempts"]]
        ok = [a for a in o["attempts"] if a[2]]
        assert abs(dict((a[0], a[1]) for a in ok)[o["best"]]) == min(abs(a[1]) for a in ok)
    if name == SEARCHES:
        assert len(o["attempts"]) >= 2, o["attempts"]
    assert "Final Image Size: (%d, %d)" % (cw, ch) in err


@pytest.mark.parametrize("name", list(CASES))
def test_resident_views_and_cropped_jpeg(runs, name):
    """--resident-views changes no byte of out.bin; the file of --crop --jpeg decodes to the size the oracle's crop() gives the
    panorama, and the cropped PNG holds the oracle's crop of its bytes"""
    from PIL import Image
    from checkers import Oracle
    views, buf, _, d = runs(name)
    _demo([d / "in.bin", d / "resident.bin", SEED, "cylinder", "--resident-views", "--crop", "--jpeg", d / "crop.jpg", "--png", d / "crop.png"])
    assert open(d / "resident.bin", "rb").read() == buf
    orc = Oracle(PanoConfig(**CFG))
    want, _ = orc.crop(_parse(buf)["final"])
    assert want.shape[0] > 100 and want.shape[1] > views[0].shape[1]
    jpg = np.asarray(Image.open(d / "crop.jpg").convert("RGB"))
    assert jpg.shape == want.shape
    png = np.asarray(Image.open(d / "crop.png").convert("RGB"))
    assert np.array_equal(png, orc.to_u8(want))
    full = np.asarray(Image.open(d / "plain.png").convert("RGB"))
    assert np.array_equal(full, orc.to_u8(_parse(buf)["final"]))


@pytest.mark.parametrize("name", list(CASES))
def test_jpeg_list_equals_in_bin_of_the_decoded_files(runs, name):
    """from JPEG files (decoded on the device, always resident) the program writes what it writes from an in.bin that holds
    Pillow's decode of the same files"""
    from PIL import Image
    views, _, _, d = runs(name)
    files, decoded = [], []
    for k, v in enumerate(views):
        p = str(d / ("%02d.jpg" % k))
        Image.fromarray(v).save(p, quality=92)
        files.append(p)
        decoded.append(np.asarray(Image.open(p).convert("RGB")).copy())
    with open(d / "files.txt", "w") as f:
        f.write("\n".join(files) + "\n")
    _write_in_bin(d / "decoded.bin", decoded)
    _demo(["--jpeg-list", d / "files.txt", d / "unused.bin", d / "from_jpeg.bin", SEED, "cylinder", "--jpeg", d / "pano.jpg"])
    _demo([d / "decoded.bin", d / "from_decoded.bin", SEED, "cylinder"])
    a, b = open(d / "from_jpeg.bin", "rb").read(), open(d / "from_decoded.bin", "rb").read()
    assert a == b
    o = _parse(a)
    assert np.asarray(Image.open(d / "pano.jpg")).shape == o["final"].shape


def _parse_build(buf):
    """out.bin of `cylinder_build`: three times int32 H, W and the fp32 pixels"""
    rd = _Reader(buf)
    out = []
    for _ in range(3):
        h, w = (int(x) for x in rd.take(np.int32, 2))
        out.append(rd.take(np.float32, h * w * 3).reshape(h, w, 3))
    assert rd.o == len(buf)
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_build_and_build_canvas_are_the_staged_run(runs, name):
    """`cylinder_build` goes through the public entries -- HipCylinderStitcher::build(), hip_perspective_correction(bundle, Mat32f)
    and build_canvas(crop), twice on one object -- and every one of them gives the panorama of the staged run bit for bit: the
    Mat32f of build(), the Mat32f the hook returns for the blend, the canvas of build_canvas() (cropped: the oracle's crop of
    it), and the files encoded from that canvas byte for byte.  Each build prints the search of the staged run."""
    from checkers import Oracle
    views, buf, err, d = runs(name)
    final = _parse(buf)["final"]
    search = _lines(err, "Best hfactor", "slope:")
    _demo([d / "in.bin", d / "staged.bin", SEED, "cylinder", "--crop", "--png", d / "staged.png", "--jpeg", d / "staged.jpg"])
    e = _demo([d / "in.bin", d / "build.bin", SEED, "cylinder_build", "--crop", "--png", d / "build.png", "--jpeg", d / "build.jpg"])
    built, hooked, canvas = _parse_build(open(d / "build.bin", "rb").read())
    assert built.shape == final.shape and built.tobytes() == final.tobytes()
    assert hooked.shape == final.shape and hooked.tobytes() == final.tobytes()
    want, _ = Oracle(PanoConfig(**CFG)).crop(final)
    assert canvas.shape == want.shape and canvas.tobytes() == np.ascontiguousarray(want).tobytes()
    for ext in ("png", "jpg"):
        assert open(d / ("build." + ext), "rb").read() == open(d / ("staged." + ext), "rb").read(), ext
    assert _lines(e, "Best hfactor", "slope:") == search + search
    assert "Final Image Size: (%d, %d)" % (final.shape[1], final.shape[0]) in e
    # resident views, no crop: all three are the panorama
    _demo([d / "in.bin", d / "build_res.bin", SEED, "cylinder_build", "--resident-views"])
    for got in _parse_build(open(d / "build_res.bin", "rb").read()):
        assert got.shape == final.shape and got.tobytes() == final.tobytes()


def _write_config_cfg(path, **over):
    """config.cfg as ConfigParser reads it (lib/config.cc:13-29): the shipped defaults with overrides"""
    from openpano_amd.config import DEFAULTS
    vals = dict(DEFAULTS); vals.update(over)
    with open(path, "w") as f:
        for k, v in vals.items():
            f.write(f"{k} {v}\n")


def _run_cli(d, views, crop):
    from PIL import Image
    d.mkdir()
    files = []
    for k, v in enumerate(views):
        p = str(d / f"{k:02d}.png")
        Image.fromarray(v).save(p)
        files.append(p)
    _write_config_cfg(str(d / "config.cfg"), CROP=crop, **CFG)
    env = dict(os.environ)
    env["OPENPANO_TEST_SEED"] = str(SEED)                 # oracle/cli_seed_seam.cc: what random_device returns
    env["OMP_NUM_THREADS"] = "1"
    r = subprocess.run([CLI_CPU] + files, capture_output=True, text=True, env=env, timeout=900, cwd=str(d))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    out = r.stdout + r.stderr                              # print_debug goes to stderr, GuardedTimer to stdout
    return out, np.asarray(Image.open(d / "out.png").convert("RGB")).copy()


def _lines(text, *keys):
    """the lines that hold one of the keys, from the key on (the reference puts a coloured [function@file:line] in front)"""
    return [ln[ln.index(k):].strip() for ln in text.splitlines() for k in keys if k in ln]


@pytest.mark.parametrize("name", list(CASES))
def test_against_the_reference_cli(runs, tmp_path, name):
    """the reference's own CPU CLI on the same views as PNG files under CYLINDER 1, seeded alike, one thread: the same Final
    Image Size, the same `Best hfactor` and `slope:` lines as printed, the same crop, and out.png within one quantisation level
    of --png with more than 0.999 of the bytes equal (the bounds test_reference_cli_dropin holds between the CPU CLI and the
    hooked cylinder CLI: the two sides solve the 4-point system with different fp64 routines)"""
    if not os.path.exists(CLI_CPU):
        pytest.skip("oracle/_ref/image-stitching not built (reference sources absent at build time)")
    from PIL import Image
    views, buf, err, d = runs(name)
    if not os.path.exists(d / "crop.png"):
        _demo([d / "in.bin", d / "again.bin", SEED, "cylinder", "--crop", "--png", d / "crop.png"])
    for crop, mine in ((0, d / "plain.png"), (1, d / "crop.png")):
        out, ref = _run_cli(tmp_path / ("crop%d" % crop), views, crop)
        assert _lines(out, "Final Image Size:") == _lines(err, "Final Image Size:") and len(_lines(out, "Final Image Size:")) == 1
        assert _lines(out, "Best hfactor", "slope:") == _lines(err, "Best hfactor", "slope:"), (_lines(out, "Best hfactor", "slope:"), _lines(err, "Best hfactor", "slope:"))
        if name == SEARCHES:
            assert len(_lines(out, "slope:")) >= 2
        got = np.asarray(Image.open(mine).convert("RGB"))
        assert got.shape == ref.shape, (crop, got.shape, ref.shape)       # CROP 1: the same crop size
        diff = np.abs(got.astype(np.int16) - ref.astype(np.int16))
        assert diff.max() <= 1, int(diff.max())
        assert (diff == 0).mean() > 0.999, float((diff == 0).mean())
