"""Writes the JPEG files of this directory and digests.json (sha256 of each file's expected RGB) with Pillow / libjpeg.

    python tests/golden/jpeg_dec/make_jpeg_dec_fixtures.py [--check]

The files are inputs of the device JPEG decoder's tests: the GPU machine may have no Pillow, and the
project's own encoder writes only the standard tables with restart markers.  `fixtures()` returns {name: file bytes} and is
what tests/test_jpeg_dec_cpu.py regenerates and compares with the committed bytes; --check does the same from the command line.
The expected RGB is Pillow's: Image.open(f).convert("RGB")."""
import hashlib
import io
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(os.path.dirname(HERE))
SAMPLINGS = {"444": 0, "422": 1, "420": 2}      # Pillow's subsampling argument
SIZES = ((2, 2), (8, 8), (9, 9), (16, 16), (17, 17), (15, 33), (37, 53), (40, 56))


def _smooth(h, w, seed):
    """a colour gradient plus low-amplitude noise (png_cases._smooth)"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([(x * 3 + y) % 256, (x + y * 2) % 256, (x * y // 7) % 256], axis=-1)
    return ((base + rng.integers(0, 4, (h, w, 3))) % 256).astype(np.uint8)


def _rand(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _checker01(h, w):
    """saturated one-pixel checker: AC category 10 at quality 100"""
    y, x = np.mgrid[0:h, 0:w]
    return np.repeat((((y + x) & 1) * 255).astype(np.uint8)[..., None], 3, axis=2)


def _block_steps(h, w):
    """8 x 8 blocks alternately black and white: DC category 11 at quality 100"""
    y, x = np.mgrid[0:h, 0:w]
    return np.repeat(((((y >> 3) + (x >> 3)) & 1) * 255).astype(np.uint8)[..., None], 3, axis=2)


def _save(Image, arr, **kw):
    b = io.BytesIO()
    Image.fromarray(arr).save(b, "JPEG", **kw)
    return b.getvalue()


def _natural():
    sys.path.insert(0, TESTS)
    import natural
    return natural.crop_u8("uav", 300, 900, 400, 600)


def fixtures():
    from PIL import Image
    out = {}
    qt = [[(3 + (7 * i) % 61) for i in range(64)], [(5 + (11 * i) % 97) for i in range(64)]]
    for name, sub in SAMPLINGS.items():
        for k, (h, w) in enumerate(SIZES):
            out[f"size_{h}x{w}_{name}"] = _save(Image, _smooth(h, w, 100 + k), quality=90, subsampling=sub)
        for q in (1, 50, 100):
            out[f"q{q}_37x53_{name}"] = _save(Image, _smooth(37, 53, 7), quality=q, subsampling=sub)
        out[f"qtables_37x53_{name}"] = _save(Image, _smooth(37, 53, 8), qtables=qt, subsampling=sub)
        out[f"opt_random_37x53_{name}"] = _save(Image, _rand(37, 53, 9), quality=100, subsampling=sub, optimize=True)
        out[f"opt_flat_17x17_{name}"] = _save(Image, np.full((17, 17, 3), (90, 160, 30), np.uint8), quality=90, subsampling=sub, optimize=True)
        out[f"checker01_32x32_{name}"] = _save(Image, _checker01(32, 32), quality=100, subsampling=sub)
        out[f"block_steps_16x64_{name}"] = _save(Image, _block_steps(16, 64), quality=100, subsampling=sub)
        # 37 x 53: 35 MCUs at 4:4:4 (5 x 7), 20 at 4:2:2 (5 x 4), 12 at 4:2:0 (3 x 4): more than eight intervals, and with 3
        # MCUs per interval a last one that is partial at 4:4:4 and 4:2:2
        out[f"rst1_37x53_{name}"] = _save(Image, _smooth(37, 53, 10), quality=90, subsampling=sub, restart_marker_blocks=1)
        out[f"rst3_37x53_{name}"] = _save(Image, _smooth(37, 53, 11), quality=90, subsampling=sub, restart_marker_blocks=3)
        out[f"rstrow_37x53_{name}"] = _save(Image, _smooth(37, 53, 12), quality=90, subsampling=sub, restart_marker_rows=1)
        thumb = _save(Image, _smooth(16, 24, 13), quality=60)
        exif = b"Exif\x00\x00II*\x00\x08\x00\x00\x00\x00\x00\x00\x00\x00\x00" + thumb
        out[f"exif_com_37x53_{name}"] = _save(Image, _smooth(37, 53, 14), quality=90, subsampling=sub, exif=exif, comment=b"FF D8 FF DA in a comment: \xff\xd8\xff\xda\xff\xd9")
    out["grey_9x9"] = _save(Image, _smooth(9, 9, 15)[..., 1].copy(), quality=90)
    out["grey_37x53"] = _save(Image, _smooth(37, 53, 16)[..., 1].copy(), quality=90)
    nat = _natural()
    out["natural_400x600_q90_420"] = _save(Image, nat, quality=90, subsampling=2)
    out["natural_400x600_q50_422"] = _save(Image, nat, quality=50, subsampling=1)
    out["progressive_37x53"] = _save(Image, _smooth(37, 53, 17), quality=90, progressive=True)      # refused: SOF2
    return out


def expected_rgb(data):
    from PIL import Image
    return np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(data)).convert("RGB")))


def main():
    fx = fixtures()
    if "--check" in sys.argv:
        bad = [n for n, b in fx.items() if open(os.path.join(HERE, n + ".jpg"), "rb").read() != b]
        print("differ:", bad) if bad else print("all", len(fx), "files regenerate to the committed bytes")
        sys.exit(1 if bad else 0)
    digests = {}
    for n, b in sorted(fx.items()):
        open(os.path.join(HERE, n + ".jpg"), "wb").write(b)
        rgb = expected_rgb(b)
        digests[n] = {"h": int(rgb.shape[0]), "w": int(rgb.shape[1]), "bytes": len(b), "sha256": hashlib.sha256(rgb.tobytes()).hexdigest()}
    with open(os.path.join(HERE, "digests.json"), "w") as f:
        json.dump(digests, f, indent=1, sort_keys=True)
        f.write("\n")
    print(len(fx), "files,", sum(len(b) for b in fx.values()), "bytes")


if __name__ == "__main__":
    main()
