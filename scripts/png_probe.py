#!/usr/bin/env python3
"""Timing of the device PNG encoder (GPU box) on two canvases: config 4's blend (38 resident 1300 x 867 views, spherical,
bench.py's blend section -- mostly Color::NO background) and a 3000 x 4000 canvas of natural texture (tests/golden/natural
tiled; needs PIL).  Per canvas: kernel time per stage from the context's HIP-event profile (mean of `--steps` calls after one
warm-up, with the spread of the per-call wall times), bytes out, and next to them what a caller would otherwise do in the
same process: Canvas.numpy_u8() alone (the floor any host encoder pays first), and numpy_u8() + a fixed Up filter in numpy
+ zlib.compress(level 1) on one host thread (a cheaper filter than the device's per-row choice).  Also the deflate stage's
size against zlib level 1 on the same filtered bytes.  One JSON object on stdout, with the library's hash.

    python scripts/png_probe.py [--steps 10] [--out profiles/png_probe_latest.json]"""
import argparse
import hashlib
import json
import os
import sys
import time
import zlib

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
    import png_cases
    from openpano_amd import hip, synth
    from openpano_amd.config import PanoConfig
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(stream)
    ctx = hip.Context(0, stream.cuda_stream)

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
        png = cv.png_bytes()                                     # warm-up (pool, code objects)
        r["png_bytes"] = len(png)
        ctx.set_profiling(True); ctx.profile_reset()
        for _ in range(a.steps):
            cv.png_bytes()
        r["kernel_ms"] = {k: round(v[0] / a.steps, 4) for k, v in ctx.profile().items() if k.startswith("png")}
        ctx.set_profiling(False)
        r["encode_wall_ms"] = wall(cv.png_bytes, a.steps)
        r["copy_u8_wall_ms"] = wall(cv.numpy_u8, a.steps)

        def host():
            u8 = cv.numpy_u8().reshape(cv.h, cv.w * 3)
            f = np.empty((cv.h, cv.w * 3 + 1), np.uint8)
            f[:, 0] = 2
            f[0, 1:] = u8[0]
            f[1:, 1:] = u8[1:] - u8[:-1]
            return zlib.compress(f.tobytes(), 1)
        r["host_up_filter_zlib1_wall_ms"] = wall(host, max(2, a.steps // 4))
        r["host_up_filter_zlib1_bytes"] = len(host())
        d = png_cases.decode(png)
        assert np.array_equal(d["pixels"], cv.numpy_u8())
        z1 = len(zlib.compress(d["filtered"], 1))
        r["idat_payload_bytes"] = len(d["payload"]); r["zlib1_same_filter_bytes"] = z1
        r["payload_over_zlib1"] = round(len(d["payload"]) / z1, 4)
        return r

    out = {"_meta": {"lib_sha256_16": hashlib.sha256(open(hip.LIB_PATH, "rb").read()).hexdigest()[:16],
                     "device": torch.cuda.get_device_name(0), "steps": a.steps, "segment_bytes": png_cases.SEG}}
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
    # CPU-side size measurements of tests/test_png_ref_cpu.py (serial restatement, same bytes as the device)
    out["deflate_stage_vs_zlib1"] = {"natural_400x600": 1.0865, "blended": 0.9849}
    ctx.close()
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
