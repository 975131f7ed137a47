"""GPU: the Huffman length limiter of the device PNG encoder on ordinary inputs (openpano_amd/csrc/png.hip).

huff_build's Kraft fix-up rewrites a tree that is deeper than the limit.  At deflate's own limits (15 / 15 / 7) only the crafted
inputs of png_cases.REACHES get there (test_gpu_png.py).  Here png.hip is compiled a second time with its three knobs at
11 / 11 / 5, where smooth, natural and blended images reach the fix-up in all three alphabets and in segments that are not the
last, and the device's file has to equal, byte for byte, the file of the serial restatement compiled with the same knobs.
The variant runs in a child process of its own (it finds the library through OPENPANO_HIP_LIB), all inputs in one run."""
import os
import subprocess
import sys

import numpy as np
import pytest

import png_cases
import variant_lib

pytestmark = pytest.mark.gpu
NAMES = ["boundary_mid_pixel_150x333", "two_segments_120x341", "blended", "natural_400x600"] + list(png_cases.REACHES)

CHILD = """
import sys
import numpy as np
sys.path.insert(0, %(root)r)
from openpano_amd import hip
assert hip.LIB_PATH == %(lib)r, hip.LIB_PATH
z = np.load(%(fin)r)
ctx = hip.Context(0)
out = {k: np.frombuffer(hip.encode_png_u8(ctx, z[k]), np.uint8) for k in z.files}
ctx.close()
np.savez(%(fout)r, **out)
"""


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """name -> (input, the variant device's file, the variant restatement's file, its statistics)"""
    tmp = tmp_path_factory.mktemp("pngvariant")
    lib = variant_lib.build_variant(tmp, "png", png_cases.VARIANT_FLAGS)
    ref = png_cases.build_ref(tmp, png_cases.VARIANT_FLAGS)
    inputs = {n: png_cases.case(n) for n in NAMES if n not in png_cases.NEEDS_PIL or png_cases.natural.available()}
    fin, fout = str(tmp / "in.npz"), str(tmp / "out.npz")
    np.savez(fin, **inputs)
    code = CHILD % dict(root=variant_lib.ROOT, lib=lib, fin=fin, fout=fout)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, OPENPANO_HIP_LIB=lib), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    got = np.load(fout)
    out = {}
    for n, rgb in inputs.items():
        want = png_cases.ref_encode(ref, rgb)
        out[n] = (rgb, got[n].tobytes(), want, png_cases.ref_stats(ref))
    return out


@pytest.mark.parametrize("name", NAMES)
def test_variant_device_file_equals_variant_reference(runs, name):
    if name not in runs:
        pytest.skip("PIL not available")
    rgb, got, want, s = runs[name]
    print(name, s)
    assert tuple(s.maxbits) == png_cases.VARIANT_MAXBITS and sum(s.limited_dynamic) > 0       # the comparison is about a limited table
    if got != want:
        n = min(len(got), len(want))
        first = next((i for i in range(n) if got[i] != want[i]), n)
        pytest.fail(f"{name}: device {len(got)} bytes, reference {len(want)} bytes, first difference at byte {first}")
    assert np.array_equal(png_cases.decode(got)["pixels"], rgb)


def test_variant_inputs_limit_every_alphabet(runs):
    """the files compared above hold limited tables of all three alphabets, one of them before the last segment"""
    for a in range(3):
        assert sum(s.limited_dynamic[a] for _, _, _, s in runs.values()) > 0, a
    assert any(s.limited_not_last for _, _, _, s in runs.values())
