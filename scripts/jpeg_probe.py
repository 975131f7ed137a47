#!/usr/bin/env python3
"""Timing of the device JPEG encoder (GPU box) on two canvases: config 4's blend (38 resident 1300 x 867 views, spherical,
bench.py's blend section -- mostly Color::NO background) and a 3000 x 4000 canvas of natural texture (tests/golden/natural
tiled; needs PIL).  Per canvas and setting (quality 90 at 4:2:0, the default; quality 100 at 4:2:0, the reference's out.jpg):
kernel time per stage from the context's HIP-event profile (mean of `--steps` calls after one warm-up), the per-call wall
times, bytes out, and next to them what a caller would otherwise do in the same process: Canvas.numpy_u8() alone, and
numpy_u8() + Pillow's libjpeg at the same settings (same restart interval, so the same bytes) on one host thread.
One JSON object on stdout, with the library's hash.

    python scripts/jpeg_probe.py [--steps 10] [--out profiles/jpeg_probe_latest.json]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import bench
    import natural
    import jpeg_cases
    from openpano_amd import hip, synth
    from openpano_amd.config import PanoConfig
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(stream)
    ctx = hip.Context(0, stream.cuda_stream)
    Image = jpeg_cases.pillow()

    def spread(ms):
        return {"mean": round(float(np.mean(ms)), 4), "min": round(float(np.min(ms)), 4), "max": round(float(np.max(ms)), 4)}

    def wall(fn, steps):
        fn()
        ms = []
        for _ in range(steps):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(); ms.append((time.perf_counter() - t0) * 1e3)
        return spread(ms)

    def probe(cv):
        r = {"canvas_hw": [cv.h, cv.w], "rgb_bytes": cv.h * cv.w * 3}
        r["copy_u8_wall_ms"] = wall(cv.numpy_u8, a.steps)
        for q, name in ((90, "420"), (100, "420"), (90, "444")):
            s = jpeg_cases.S420 if name == "420" else jpeg_cases.S444
            e = {}
            jpg = cv.jpeg_bytes(q, name)                             # warm-up (pool, code objects)
            e["jpeg_bytes"] = len(jpg)
            e["intervals"] = len(jpeg_cases.walk(jpg)["intervals"])
            ctx.set_profiling(True); ctx.profile_reset()
            for _ in range(a.steps):
                cv.jpeg_bytes(q, name)
            e["kernel_ms"] = {k: round(v[0] / a.steps, 4) for k, v in ctx.profile().items() if k.startswith("jpeg")}
            ctx.set_profiling(False)
            e["encode_wall_ms"] = wall(lambda: cv.jpeg_bytes(q, name), a.steps)
            if Image is not None:
                def host():
                    return jpeg_cases.pillow_encode(Image, cv.numpy_u8(), q, s, jpeg_cases.RI[s])
                e["host_copy_u8_libjpeg_wall_ms"] = wall(host, max(2, a.steps // 4))
                e["equals_libjpeg"] = host() == jpg
                e["libjpeg_no_restart_bytes"] = len(jpeg_cases.pillow_encode(Image, cv.numpy_u8(), q, s, 0))
            else:
                e["host_copy_u8_libjpeg_wall_ms"] = "not measured: Pillow's JPEG codec not available"
            r[f"q{q}_{name}"] = e
        return r

    out = {"_meta": {"lib_sha256_16": hashlib.sha256(open(hip.LIB_PATH, "rb").read()).hexdigest()[:16],
                     "device": torch.cuda.get_device_name(0), "steps": a.steps, "host_threads": 1,
                     "restart_interval_mcus": {"444": jpeg_cases.RI[jpeg_cases.S444], "420": jpeg_cases.RI[jpeg_cases.S420]}}}
    # config 4's canvas
    H, W, n = 867, 1300, 38
    views = synth.image_set(n, H, W, seed=38, overlap=0.45, rows=2, shuffle=True)
    d_imgs = [torch.from_numpy(v).to(dev) for v in views]
    inputs = [(t.data_ptr(), H, W) for t in d_imgs]
    homos = bench.run_blend(hip, ctx, PanoConfig(), inputs, H, W, argparse.Namespace(steps=1), lambda m: None)["_homos"]
    cv = hip.BlendCall(ctx, PanoConfig(MULTIBAND=0), inputs, homos, 2, n // 2)()
    out["config4_canvas"] = probe(cv)
    cv.free()
    del d_imgs
    # natural texture, 3000 x 4000
    if natural.available():
        src = natural.u8_to_f32(natural.load("uav"))
        reps = (-(-3000 // src.shape[0]), -(-4000 // src.shape[1]), 1)
        img = np.ascontiguousarray(np.tile(src, reps)[:3000, :4000])
        cv = hip.blend(ctx, PanoConfig(LAZY_READ=0), [img], np.eye(3)[None], 0, 0)
        out["natural_3000x4000"] = probe(cv)
        cv.free()
    else:
        out["natural_3000x4000"] = "not measured: PIL not available"
    ctx.close()
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
