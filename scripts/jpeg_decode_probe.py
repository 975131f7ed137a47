#!/usr/bin/env python3
"""Timing of the device JPEG decoder (GPU box).  Inputs: 38 natural 867 x 1300 views (shifts of
tests/golden/nat_uav_867x1300.npz, so no Pillow is needed to make them) and one 3000 x 4000 view (the same image tiled), each
encoded at quality 90, 4:2:0, two ways: with restart intervals by the device encoder, and as one unbroken scan by
tests/harness/jpeg_ref.c built with -DOP_JPEG_RI_420 above the MCU count.  Per row: kernel time per stage from the context's
HIP-event profile (mean of `--steps` calls after one warm-up), the call's wall times, the pass-B rounds, and next to them the
parent path on the same pixels -- Views.upload of already-decoded bytes -- and, where Pillow imports, Pillow's decode on one
host thread plus Views.upload: the path the decoder replaces.  One JSON object on stdout, with the library's hash.

    python scripts/jpeg_decode_probe.py [--steps 10] [--out profiles/jpeg_decode_probe_latest.json]"""
import argparse
import ctypes as C
import hashlib
import io
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def unbroken_encoder(tmp):
    """tests/harness/jpeg_ref.c with one restart interval for the whole image (DRI holds 16 bits: up to 65535 MCUs)"""
    so = os.path.join(tmp, "libjpeg_ref_unbroken.so")
    subprocess.check_call([shutil.which("gcc"), "-std=c11", "-O2", "-fPIC", "-shared", "-DOP_JPEG_RI_444=65535", "-DOP_JPEG_RI_420=65535",
                           os.path.join(ROOT, "tests", "harness", "jpeg_ref.c"), "-o", so])
    L = C.CDLL(so)
    L.jpeg_ref_bound.restype = C.c_long
    L.jpeg_ref_bound.argtypes = [C.c_int, C.c_int, C.c_int]
    L.jpeg_ref_encode.restype = C.c_long
    L.jpeg_ref_encode.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_long]
    return L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import jpeg_cases
    from openpano_amd import hip
    try:
        from PIL import Image
    except ImportError:
        Image = None
    ctx = hip.Context(0)

    def spread(ms):
        return {"mean": round(float(np.mean(ms)), 4), "min": round(float(np.min(ms)), 4), "max": round(float(np.max(ms)), 4)}

    def wall(fn, steps):
        fn()
        ms = []
        for _ in range(steps):
            ctx.sync(); t0 = time.perf_counter()
            fn()
            ctx.sync(); ms.append((time.perf_counter() - t0) * 1e3)
        return spread(ms)

    def decode(files):
        hip.Views.decode_jpeg(ctx, files).free()

    def probe(files, pixels):
        r = {"files": len(files), "file_bytes": sum(len(f) for f in files), "rgb_bytes": sum(p.size for p in pixels),
             "intervals_per_file": len(jpeg_cases.walk(files[0])["intervals"]) if b"\xff\xd0" in files[0] else 1}
        v = hip.Views.decode_jpeg(ctx, files)                     # warm-up (pool, code objects), and the check
        r["equals_source_decode"] = all(np.array_equal(v.numpy(i), pixels[i]) for i in range(len(files)))
        r["pass_b_rounds"] = ctx.jpeg_last_rounds()
        v.free()
        ctx.set_profiling(True); ctx.profile_reset()
        for _ in range(a.steps):
            decode(files)
        r["kernel_ms"] = {k: round(val[0] / a.steps, 4) for k, val in ctx.profile().items() if k.startswith("jpegdec")}
        ctx.set_profiling(False)
        r["decode_wall_ms"] = wall(lambda: decode(files), a.steps)
        r["upload_decoded_bytes_wall_ms"] = wall(lambda: hip.Views.upload(ctx, pixels).free(), a.steps)
        if Image is not None:
            def host():
                px = [np.asarray(Image.open(io.BytesIO(f)).convert("RGB")) for f in files]
                hip.Views.upload(ctx, px).free()
            r["host_libjpeg_decode_plus_upload_wall_ms"] = wall(host, max(2, a.steps // 4))
        else:
            r["host_libjpeg_decode_plus_upload_wall_ms"] = "not measured: Pillow not available"
        return r

    base = np.load(os.path.join(ROOT, "tests", "golden", "nat_uav_867x1300.npz"))["img"]
    views = [np.ascontiguousarray(np.roll(base, (13 * i, 29 * i), axis=(0, 1))) for i in range(38)]
    big = np.ascontiguousarray(np.tile(base, (4, 4, 1))[:3000, :4000])
    out = {"_meta": {"lib_sha256_16": hashlib.sha256(open(hip.LIB_PATH, "rb").read()).hexdigest()[:16], "steps": a.steps, "host_threads": 1,
                     "quality": 90, "sampling": "420", "subsequence_bits": 1024, "pillow": Image is not None}}
    with tempfile.TemporaryDirectory() as tmp:
        U = unbroken_encoder(tmp)
        ref = __import__("jpeg_dec_cases").build_ref(tmp)
        for name, imgs in (("views_38x867x1300", views), ("view_3000x4000", [big])):
            for kind in ("restart_intervals", "unbroken_scan"):
                if kind == "restart_intervals":
                    files = [hip.encode_jpeg_u8(ctx, im, 90, "420") for im in imgs]
                else:
                    files = [jpeg_cases.ref_encode(U, im, 90, jpeg_cases.S420) for im in imgs]
                # the pixels the files hold, from the serial restatement (equal to libjpeg's: tests/test_jpeg_dec_cpu.py)
                pixels = [__import__("jpeg_dec_cases").ref_decode(ref, f) for f in files]
                out[f"{name}_{kind}"] = probe(files, pixels)
    ctx.close()
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
