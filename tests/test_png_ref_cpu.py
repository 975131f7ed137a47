"""PNG encoder, the parts that need no GPU:

1. the library is ABI 12 and exports the encoder's entry points (it loads without a device);
2. the serial restatement of the device encoder (tests/harness/png_ref.c) writes files that an independent decoder -- struct,
   binascii.crc32 and zlib.decompressobj, nothing else -- accepts and un-filters to exactly the input, for every input of
   png_cases.CASES; PIL, where present, reads the same pixels;
3. sizes: never above the stored form plus framing; the all-background canvas of config 4 at least 100-fold;
4. the deflate stage against zlib level 1 on the same filtered bytes, on photographic content (measured bounds)."""
import ctypes as C
import io
import zlib

import numpy as np
import pytest

import png_cases
from openpano_amd import hip

# len(IDAT payload) / len(zlib.compress(filtered, 1)) as measured on this encoder, rounded up to the next 0.05 (DESIGN 11.5;
# also in profiles/png_probe_latest.json).  Above 1.30 would be an encoder defect, not a bound.
# Measured: natural crop 259118 / 238493 = 1.0865, blended canvas 86808 / 88139 = 0.9849.
RATIO_BOUND = {"natural_400x600": 1.10, "blended": 1.00}


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return png_cases.build_ref(tmp_path_factory.mktemp("pngref"))


def test_abi_12_and_symbols():
    L = hip.lib()
    assert L.op_abi_version() == 12
    for name in ("op_canvas_encode_png", "op_png_encode_u8", "op_png_size", "op_png_copy", "op_png_free"):
        assert hasattr(L, name), name


@pytest.mark.parametrize("name", list(png_cases.CASES))
def test_reference_file_decodes_to_input(ref, name):
    rgb = png_cases.case(name)
    h, w, _ = rgb.shape
    png = png_cases.ref_encode(ref, rgb)
    d = png_cases.decode(png)
    assert (d["h"], d["w"]) == (h, w)
    assert np.array_equal(d["pixels"], rgb)
    assert d["n_idat"] == -(-(h * (1 + 3 * w)) // png_cases.SEG) + 2      # zlib header, one per segment, Adler-32
    assert len(png) <= png_cases.stored_bound(h, w), (len(png), png_cases.stored_bound(h, w))
    try:
        from PIL import Image
    except ImportError:
        return
    Image.MAX_IMAGE_PIXELS = None
    im = Image.open(io.BytesIO(png))
    assert im.mode == "RGB" and np.array_equal(np.asarray(im), rgb)


def test_reference_is_deterministic(ref):
    rgb = png_cases.case("blended")
    assert png_cases.ref_encode(ref, rgb) == png_cases.ref_encode(ref, rgb.copy())


@pytest.mark.parametrize("name", ["random_97x211", "random_one_segment_60x341"])
def test_incompressible_input_is_stored(ref, name):
    rgb = png_cases.case(name)
    h, w, _ = rgb.shape
    d = png_cases.decode(png_cases.ref_encode(ref, rgb))
    n = h * (1 + 3 * w)
    nseg = -(-n // png_cases.SEG)
    assert len(d["payload"]) == 2 + n + 5 * nseg + 4            # zlib header, one stored block per segment, Adler-32


def test_background_canvas_compresses_100_fold(ref):
    rgb = png_cases.case("all255_763x7999")
    png = png_cases.ref_encode(ref, rgb)
    ratio = rgb.size / len(png)
    print(f"all-255 763 x 7999: {rgb.size} -> {len(png)} bytes, {ratio:.1f}-fold")
    assert ratio >= 100, ratio


@pytest.mark.parametrize("name", list(RATIO_BOUND))
def test_deflate_stage_against_zlib_level_1(ref, name):
    rgb = png_cases.case(name)
    d = png_cases.decode(png_cases.ref_encode(ref, rgb))
    ours, theirs = len(d["payload"]), len(zlib.compress(d["filtered"], 1))
    ratio = ours / theirs
    print(f"{name}: IDAT payload {ours}, zlib level 1 {theirs}, ratio {ratio:.4f}")
    assert RATIO_BOUND[name] <= 1.30
    assert ratio <= RATIO_BOUND[name], ratio
