"""GPU: the SIFT ingest kernel (k_grey_octaves, csrc/pyramid.hip) off resize ratio 1 (tests/ingest_cases.py), from fp32 and
from decoder bytes.  At ratio 1, where the other shape tests run, the working-tile half of the kernel is a copy; here bilerp,
both clamps of resize_coord, the row and column tables, the six-element source runs and the byte LUT all do arithmetic, with
the working image ending one short of, at and one past a multiple of the 64 x 14 tile.  The working image, every grey plane and
everything built on them equal the C oracle's, bit for bit; test_ingest_cases_cpu.py shows the oracle equal to the reference
at every case used here."""
import numpy as np
import pytest

import ingest_cases as ic
import sift_cases as sc

pytestmark = pytest.mark.gpu
KINDS = ("f32", "u8", "rgb_u8")


@pytest.fixture(scope="module")
def ctx():
    from openpano_amd import hip
    c = hip.Context(0)
    yield c
    c.close()


def _source(case, kind):
    """(what the device gets, the fp32 image the oracle gets)"""
    if kind == "f32":
        img = ic.f32_image(case)
        return img, img
    u8 = ic.u8_image(case) if kind == "u8" else ic.rgb_u8_image(case)
    return u8, ic.twin(u8)


def _staged_equals_oracle(ctx, case, kind):
    from checkers import Oracle
    from openpano_amd import hip
    cfg = ic.cfg_of(case)
    src, f32 = _source(case, kind)
    o = Oracle(cfg).sift_stages(f32)
    assert o.dims[0] == ic.working_dims(*case[2]) and o.dims[0] != src.shape[:2]
    sc._compare_stages(hip.sift_staged(ctx, cfg, src), o, cfg)


def _same_stages(a, b):
    """two hip.sift_staged results, field by field"""
    assert a.dims == b.dims and np.array_equal(a.work, b.work)
    for kind in ("grey", "dog", "mag", "ort", "raw"):
        x, y = getattr(a, kind), getattr(b, kind)
        assert x.keys() == y.keys() and len(x) > 0
        for k in x:
            assert np.array_equal(x[k], y[k]), (kind, k)
    for nm in ("refined", "oriented"):
        for f in ("ints", "real", "fl"):
            assert np.array_equal(getattr(a, nm)[f], getattr(b, nm)[f]), (nm, f)
    assert np.array_equal(a.desc, b.desc) and np.array_equal(a.coor, b.coor)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", ic.SEAM_CASES, ids=[c[0] for c in ic.SEAM_CASES])
def test_seam_cases(ctx, case, kind):
    """working images of 41 | 42 | 43 rows and 127 | 128 | 129 columns (3 x 14 and 2 x 64, one short and one past) resized
    from the source at ratios 0.23, 0.5, 0.74, 1.6, 2.86 and 8.5: the fp32 image, its byte image (the first case's holds every
    byte value in every channel) against the oracle on the fp32 twin, and bytes with three independent channels"""
    _staged_equals_oracle(ctx, case, kind)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", ic.SMALL_SOURCES, ids=[c[0] for c in ic.SMALL_SOURCES])
def test_smallest_sources(ctx, case, kind):
    """2 x 2, 2 x 9, 9 x 2 and 3 x 3 sources up-scaled to a working size of 48: on a two-pixel axis every index is a clamped
    one, neighbouring lanes read the same run, and the run at the image's end is the image's last six elements"""
    _staged_equals_oracle(ctx, case, kind)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", ic.SCALE_ROWS + [ic.FALLBACK_CASE], ids=[c[0] for c in ic.SCALE_ROWS + [ic.FALLBACK_CASE]])
def test_octave_section_at_other_scale_factors(ctx, case, kind):
    """the octave section resizing at 1 / 1.2 and 1 / 1.3 instead of 1 / sqrt(2), through eight octaves, and at
    SCALE_FACTOR 0.9, where octave 1 is larger than the working image and the candidate rectangle outgrows the column table:
    the one case that runs the per-element branch (test_ingest_cases_cpu.py::test_fallback_case_outgrows_the_column_table)"""
    _staged_equals_oracle(ctx, case, kind)


@pytest.mark.parametrize("name,h,w,seed", ic.BIG_U8, ids=[b[0] for b in ic.BIG_U8])
def test_byte_images_at_job_shapes(ctx, cfg, oracle, name, h, w, seed):
    """867 x 1300 and 400 x 600 decoder bytes under the default config, every plane against the oracle on the fp32 twin"""
    from openpano_amd import hip
    u8 = ic.big_u8(h, w, seed)
    o = oracle.sift_stages(ic.twin(u8))
    assert o.dims[0] == ic.working_dims(h, w, cfg.SIFT_WORKING_SIZE)
    sc._compare_stages(hip.sift_staged(ctx, cfg, u8, planes=True), o, cfg)


ALIGN_CASES = [c for c in ic.SEAM_CASES if c[0] in ("r0.74_43x129", "r2.86_41x128")]


@pytest.mark.parametrize("kind", ("f32", "u8"))
@pytest.mark.parametrize("case", ALIGN_CASES, ids=[c[0] for c in ALIGN_CASES])
def test_device_sources_that_are_only_element_aligned(ctx, case, kind):
    """a resident fp32 source 4 bytes past a 16-byte boundary (the runs are fetched as 16-byte + 8-byte loads declared
    4-aligned) and a resident byte source at an odd address: the same planes as from the host array"""
    import torch
    from openpano_amd import hip
    assert len(ALIGN_CASES) == 2
    cfg = ic.cfg_of(case)
    src, _ = _source(case, kind)
    h, w = src.shape[:2]
    flat = torch.from_numpy(src.reshape(-1))
    buf = torch.zeros(flat.numel() + 1, dtype=flat.dtype, device="cuda")
    view = buf[1:]
    view.copy_(flat)
    torch.cuda.synchronize()
    ptr = view.data_ptr()
    assert ptr % 16 == 4 if kind == "f32" else ptr % 2 == 1
    got = hip.sift_staged(ctx, cfg, (ptr, h, w, "u8") if kind == "u8" else (ptr, h, w))
    _same_stages(got, hip.sift_staged(ctx, cfg, src))
    del buf


@pytest.fixture(scope="module")
def batch_images():
    """per BATCHES row: config, the four sources (two shapes x fp32 / bytes), their working shapes and the oracle's features"""
    from checkers import Oracle
    from openpano_amd.config import PanoConfig
    out = {}
    for cls, ws, shapes in ic.BATCHES:
        cfg = PanoConfig(SIFT_WORKING_SIZE=ws, **sc.LOOSE)
        orc = Oracle(cfg)
        srcs, dims, want = [], [], []
        for (wh, ww), src in zip(shapes, ic.batch_sources(cls, ws, shapes)):
            assert ic.working_dims(*src) == (wh, ww)
            case = ("batch", cls, src, {})
            for s, f32 in ((ic.f32_image(case),) * 2, (ic.u8_image(case), ic.twin(ic.u8_image(case)))):
                d, c = orc.detect_feature(f32)
                assert len(d) > 100, (cls, wh, ww, len(d))
                srcs.append(s); dims.append((wh, ww)); want.append((d, c))
        out[cls] = (cfg, srcs, dims, want)
    return out


def test_batches_of_two_shapes_and_two_types(ctx, batch_images):
    """op_sift_batch (write_work = 0) with four groups per call -- two working shapes around 7 x 14 rows and 3 x 64 columns,
    each as fp32 and as bytes -- of n = 1..9 copies each, at a down-scaling and an up-scaling ratio.  The kernel deals
    ntile = tiles x n workgroups over 8 XCDs, rounds the grid up to a multiple of 8 and drops the padding blocks
    (lin >= ntile); image = lin / tiles.  The tile counts reached cover ntile % 8 == 0 and at least three other residues;
    every image's features equal the oracle's on its fp32 twin."""
    from openpano_amd import hip
    residues = set()
    for cls, ws, shapes in ic.BATCHES:
        cfg, srcs, dims, want = batch_images[cls]
        for n in range(1, 10):
            order = [k for _ in range(n) for k in range(4)]           # interleaved: the groups are gathered from all over the call
            f = hip.sift_batch(ctx, cfg, [srcs[k] for k in order])
            try:
                assert f.num_images == 4 * n
                for i, k in enumerate(order):
                    d, c = f.get(i)
                    assert np.array_equal(d, want[k][0]) and np.array_equal(c, want[k][1]), (cls, n, i, k)
            finally:
                f.free()
            residues |= {ic.ntile(wh, ww, n) % 8 for wh, ww in dims}
    assert 0 in residues and len(residues - {0}) >= 3, residues


def test_alternating_types_and_sizes_on_one_context(ctx):
    """the LUT and the coordinate tables are per launch, the staging block and the source table per context: a byte case,
    an fp32 case of another size, the byte case again -- the third result equals the first (and the oracle's)"""
    from openpano_amd import hip
    by = {c[0]: c for c in ic.SEAM_CASES}
    a, b = by["r0.23_41x128"], by["r1.6_43x129"]
    first = hip.sift_staged(ctx, ic.cfg_of(a), ic.u8_image(a))
    _staged_equals_oracle(ctx, b, "f32")
    _same_stages(hip.sift_staged(ctx, ic.cfg_of(a), ic.u8_image(a)), first)
    _staged_equals_oracle(ctx, a, "u8")
