#!/usr/bin/env python3
"""Timing of the oriented JPEG decode (GPU box).  Inputs as scripts/jpeg_decode_probe.py: 38 natural
867 x 1300 views (shifts of tests/golden/nat_uav_867x1300.npz) and one 3000 x 4000 view (the same image tiled), encoded at
quality 90, 4:2:0 with restart intervals by the device encoder, then given an EXIF orientation tag (tests/exif_craft.py).
Per input and orientation 1, 3, 6, 5: the last stage's kernel time from the context's HIP-event profile -- k_jd_rgb for
orientation 1, the yardstick, k_jd_rgb_oriented otherwise -- and their ratio, all stages' kernel time, the call's wall time
(mean of `--steps` calls after one warm-up, all in one process), and the path the call replaces: Pillow's decode and
ImageOps.exif_transpose on one host thread plus Views.upload.  The views are checked against the plain decode put through
the index map.  One JSON object on stdout, with the library's hash.

    python scripts/jpeg_orient_probe.py [--steps 10] [--out profiles/jpeg_orient_probe_latest.json]"""
import argparse
import hashlib
import io
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
ORIENTATIONS = (1, 3, 6, 5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import exif_craft
    from openpano_amd import hip
    try:
        from PIL import Image, ImageOps
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

    def probe(plain_files, stored, o):
        files = [exif_craft.with_orientation(f, o) for f in plain_files]
        r = {"files": len(files), "rgb_bytes": sum(p.size for p in stored)}
        v = hip.Views.decode_jpeg(ctx, files, orient=True)        # warm-up (pool, code objects), and the check
        r["equals_index_map_of_plain_decode"] = all(np.array_equal(v.numpy(i), exif_craft.orient_map(stored[i], o)) for i in range(len(files)))
        v.free()
        ctx.set_profiling(True); ctx.profile_reset()
        for _ in range(a.steps):
            hip.Views.decode_jpeg(ctx, files, orient=True).free()
        prof = {k: round(val[0] / a.steps, 4) for k, val in ctx.profile().items() if k.startswith("jpegdec")}
        ctx.set_profiling(False)
        last = [k for k in prof if k.startswith("jpegdec rgb")]
        assert len(last) == 1 and (last[0] == "jpegdec rgb") == (o == 1), prof
        r["last_stage"] = last[0]
        r["last_stage_kernel_ms"] = prof[last[0]]
        r["all_kernels_ms"] = round(sum(val for k, val in prof.items() if "H2D" not in k and "host" not in k), 4)
        r["kernel_ms"] = prof
        r["decode_wall_ms"] = wall(lambda: hip.Views.decode_jpeg(ctx, files, orient=True).free(), a.steps)
        if Image is not None:
            def host():
                px = [np.asarray(ImageOps.exif_transpose(Image.open(io.BytesIO(f))).convert("RGB")) for f in files]
                hip.Views.upload(ctx, px).free()
            r["host_libjpeg_decode_transpose_plus_upload_wall_ms"] = wall(host, max(2, a.steps // 4))
        else:
            r["host_libjpeg_decode_transpose_plus_upload_wall_ms"] = "not measured: Pillow not available"
        return r

    base = np.load(os.path.join(ROOT, "tests", "golden", "nat_uav_867x1300.npz"))["img"]
    views = [np.ascontiguousarray(np.roll(base, (13 * i, 29 * i), axis=(0, 1))) for i in range(38)]
    big = np.ascontiguousarray(np.tile(base, (4, 4, 1))[:3000, :4000])
    out = {"_meta": {"lib_sha256_16": hashlib.sha256(open(hip.LIB_PATH, "rb").read()).hexdigest()[:16], "steps": a.steps, "host_threads": 1,
                     "quality": 90, "sampling": "420", "orientations": list(ORIENTATIONS), "pillow": Image is not None,
                     "note": "one run on one machine"}}
    for name, imgs in (("views_38x867x1300", views), ("view_3000x4000", [big])):
        plain_files = [hip.encode_jpeg_u8(ctx, im, 90, "420") for im in imgs]
        v = hip.Views.decode_jpeg(ctx, plain_files)
        stored = [v.numpy(i) for i in range(len(plain_files))]
        v.free()
        rows = {}
        for o in ORIENTATIONS:
            rows[str(o)] = probe(plain_files, stored, o)
        for o in ORIENTATIONS:
            rows[str(o)]["last_stage_over_k_jd_rgb"] = round(rows[str(o)]["last_stage_kernel_ms"] / rows["1"]["last_stage_kernel_ms"], 3)
        out[name] = rows
    ctx.close()
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
