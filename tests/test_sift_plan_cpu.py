"""CPU: the plan of a SIFT batch (openpano_amd/csrc/sift_plan.cc: working and octave sizes, the Gaussian bank, the choice of the
scale-space kernel and of the row kernel's segment height), compiled with tests/harness/sift_plan_harness.cc into a program of
its own under AddressSanitizer and UndefinedBehaviorSanitizer.  Nothing is loaded into Python and nothing is preloaded.  The
program prints every plan as text; the sizes and the bank are checked against the C oracle, the refusals against the ABI's
codes, and the per-batch segment heights against the choices recorded from the code before build_plan became a unit of its own."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import ingest_cases
import sift_cases as sc
from openpano_amd.config import PanoConfig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "openpano_amd", "csrc")
OP_OK, OP_ERR_INVALID, OP_ERR_UNSUPPORTED = 0, -1, -4         # include/openpano_hip.h
RW_SEG_MIN, RW_SEG_MAX, MAX_KCENTER = 16, 40, 15              # csrc/sift_plan.hpp, op_base.hpp

SHIPPED = {}
BENCH_SHAPES = [(867, 1300), (400, 600), (3000, 4000)]
DIM_CASES = ([(dict(sc.LOOSE, SIFT_WORKING_SIZE=(h + w) // 2), h, w) for h, w in sc.edge_shapes(16)] +
             [(dict(sc.LOOSE, **kv), sc.TINY_IMAGE[0], sc.TINY_IMAGE[1]) for _, kv, _ in sc.TINY] +
             [(SHIPPED, h, w) for h, w in BENCH_SHAPES])
BANK_CONFIGS = [("shipped", SHIPPED, 1), ("scales6", dict(NUM_SCALE=6), 0), ("window4", dict(GAUSS_WINDOW_FACTOR=4), 0)]
REFUSALS = [("octaves0", dict(NUM_OCTAVE=0), 240, 320, OP_ERR_UNSUPPORTED), ("octaves9", dict(NUM_OCTAVE=9), 240, 320, OP_ERR_UNSUPPORTED),
            ("scales3", dict(NUM_SCALE=3), 240, 320, OP_ERR_UNSUPPORTED), ("scales13", dict(NUM_SCALE=13), 240, 320, OP_ERR_UNSUPPORTED),
            ("halfwidth16", dict(GAUSS_WINDOW_FACTOR=16), 240, 320, OP_ERR_UNSUPPORTED),         # scale 4: 2 x 16 + 1 taps
            ("1xN", SHIPPED, 1, 320, OP_ERR_INVALID),
            ("octave5px", dict(SIFT_WORKING_SIZE=16), 60, 80, OP_ERR_INVALID)]                   # 13 x 18, fourth octave 5 x 7
BATCHES = (1, 5, 8, 38, 128)
# source shape -> per batch size (rw_seg, rw_items) with the shipped config on 256 compute units, as build_plan chose them
# while it was part of sift_host.hip (read from that code, not from the unit under test)
CHOSEN = {(867, 1300): [(16, 317), (26, 198), (40, 128), (24, 213), (40, 128)],
          (241, 481): [(16, 341), (28, 200), (22, 254), (24, 231), (24, 231)]}
PINS = (18, 24, 40)


def _f32_hex(v):
    return "%x" % int(np.float32(v).view(np.uint32))


def _case(kv, sh, sw, n=1, num_cu=256, pin=0):
    return (tuple(sorted(kv.items())), sh, sw, n, num_cu, pin)


def _line(case):
    kv, sh, sw, n, num_cu, pin = case
    c = PanoConfig(**dict(kv))
    return "%d %d %d %s %s %d %d %d %d %d %d" % (c.SIFT_WORKING_SIZE, c.NUM_OCTAVE, c.NUM_SCALE, _f32_hex(c.SCALE_FACTOR), _f32_hex(c.GAUSS_SIGMA),
                                                  c.GAUSS_WINDOW_FACTOR, n, sh, sw, num_cu, pin)


def _all_cases():
    out = [_case(kv, h, w) for kv, h, w in DIM_CASES]
    out += [_case(kv, 240, 320) for _, kv, _ in BANK_CONFIGS]
    out += [_case(kv, h, w) for _, kv, h, w, _ in REFUSALS]
    out += [_case(SHIPPED, h, w, n, 256) for (h, w) in CHOSEN for n in BATCHES]
    out += [_case(SHIPPED, h, w, n, cu) for (h, w) in BENCH_SHAPES for n in BATCHES for cu in (64, 0)]
    out += [_case(SHIPPED, 867, 1300, n, 256, pin) for n in (1, 5) for pin in PINS]
    return list(dict.fromkeys(out))


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    """every plan of the module from one run of the sanitizer program: case -> the plan it printed"""
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ missing")
    tmp = tmp_path_factory.mktemp("sift_plan")
    exe = str(tmp / "sift_plan_harness")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                           "-Wall", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                           os.path.join(ROOT, "tests", "harness", "sift_plan_harness.cc"), os.path.join(CSRC, "sift_plan.cc"), "-o", exe])
    cases = _all_cases()
    (tmp / "cases.txt").write_text("".join(_line(c) + "\n" for c in cases))
    r = subprocess.run([exe, str(tmp / "cases.txt")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == "sift_plan_harness: %d plans" % len(cases), lines[-1]
    return dict(zip(cases, (json.loads(ln) for ln in lines[:-1])))


def _octaves(p):
    return [dict(zip(("h", "w", "tiles_x", "tiles_y", "tile_begin", "rw_nb", "rw_nseg", "off", "plane"), o)) for o in p["oct"]]


@pytest.mark.parametrize("kv,h,w", DIM_CASES, ids=["%d_%dx%d" % (i, h, w) for i, (_, h, w) in enumerate(DIM_CASES)])
def test_dimensions_equal_the_oracle(plans, kv, h, w):
    from checkers import Oracle
    cfg = PanoConfig(**kv)
    p = plans[_case(kv, h, w)]
    assert p["rc"] == OP_OK, p
    o = Oracle(cfg).sift_stages(sc.flat(h, w), planes=False)            # orc_sift_working_dims, orc_sift_octave_dims
    assert (p["wh"], p["ww"]) == o.work.shape[:2] == ingest_cases.working_dims(h, w, cfg.SIFT_WORKING_SIZE)
    octs = _octaves(p)
    assert [(q["h"], q["w"]) for q in octs] == o.dims and len(octs) == cfg.NUM_OCTAVE
    off = 0
    for q in octs:                                                      # the workspace: NUM_SCALE planes per octave, back to back
        assert q["plane"] == q["h"] * q["w"] and q["off"] == off
        off += cfg.NUM_SCALE * q["plane"]
    assert p["ws_stride"] == (off + 63) // 64 * 64


@pytest.mark.parametrize("name,kv,rows_ok", BANK_CONFIGS, ids=[b[0] for b in BANK_CONFIGS])
def test_gauss_bank_equals_the_oracle_bit_for_bit(plans, name, kv, rows_ok):
    from checkers import Oracle
    cfg = PanoConfig(**kv)
    orc = Oracle(cfg)
    p = plans[_case(kv, 240, 320)]
    assert p["rc"] == OP_OK, p
    kern = np.array(p["kern"], np.uint32).reshape(-1, 2 * MAX_KCENTER + 1)
    want = np.zeros_like(kern)
    centers = [0] * len(kern)
    sigma = np.float32(cfg.GAUSS_SIGMA)
    for s in range(1, cfg.NUM_SCALE):                                   # feature/gaussian.hh:96-103
        taps = orc.gauss_kernel(sigma)
        centers[s] = len(taps) // 2
        want[s, MAX_KCENTER - centers[s]: MAX_KCENTER + centers[s] + 1] = taps.view(np.uint32)
        sigma = np.float32(sigma * np.float32(cfg.SCALE_FACTOR))
    assert p["kcenter"] == centers and p["halo"] == max(centers)
    assert np.array_equal(kern, want)
    assert p["rows_ok"] == rows_ok
    kpair = np.array(p["kpair"], np.uint32).reshape(3, 7, 2)
    if rows_ok:                                                         # taps at distance d of the scales 2 pl + 1 and 2 pl + 2, zero-extended
        for pl in range(3):
            for e in range(2):
                s = 2 * pl + 1 + e
                assert np.array_equal(kpair[pl, :, e], np.concatenate([kern[s, MAX_KCENTER: MAX_KCENTER + centers[s] + 1], np.zeros(6 - centers[s], np.uint32)]))
    else:
        assert not kpair.any() and p["rw_seg"] == 0 and p["rw_items"] == 0


@pytest.mark.parametrize("name,kv,h,w,code", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals(plans, name, kv, h, w, code):
    p = plans[_case(kv, h, w)]
    assert p["rc"] == code and p["error"], p


def _check_split(p, seg):
    assert p["rows_ok"] == 1 and p["rw_seg"] == seg and seg % 2 == 0 and RW_SEG_MIN <= seg <= RW_SEG_MAX
    octs = _octaves(p)
    assert [q["rw_nb"] for q in octs] == [-(-q["w"] // sc.RW_OWN) for q in octs]
    assert [q["rw_nseg"] for q in octs] == [-(-q["h"] // seg) for q in octs]
    assert p["rw_items"] == sum(q["rw_nb"] * q["rw_nseg"] for q in octs)


def test_segment_height_is_chosen_per_batch(plans):
    for (h, w), want in CHOSEN.items():
        got = [plans[_case(SHIPPED, h, w, n, 256)] for n in BATCHES]
        assert [(p["rw_seg"], p["rw_items"]) for p in got] == want, (h, w)
    for case, p in plans.items():
        if p["rc"] == OP_OK and p["rows_ok"]:
            _check_split(p, case[5] or p["rw_seg"])
    for n in BATCHES:                                                   # an unknown compute-unit count (0) plans like 256
        assert plans[_case(SHIPPED, 867, 1300, n, 0)] == plans[_case(SHIPPED, 867, 1300, n, 256)]


def test_pinned_segment_height_is_obeyed(plans):
    for n in (1, 5):
        for pin in PINS:
            _check_split(plans[_case(SHIPPED, 867, 1300, n, 256, pin)], pin)
