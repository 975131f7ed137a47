#!/usr/bin/env python3
"""Timing of exposure compensation on config 4's blend geometry (GPU box): bench.py's blend section (38 resident
1300 x 867 views, 2-row camera sweep, spherical projection) -- op_gain_overlap at strides 1, 2, 4, op_gain_solve, and
op_blend_gains against op_blend for the linear and the 5-band blender.  Kernel times from the context's HIP-event
profile (mean of `--steps` calls after one warm-up), wall times per call; one JSON object on stdout, with the library's
hash.

    python scripts/gain_probe.py [--steps 10] [--out profiles/gain_probe_latest.json]"""
import argparse
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import bench
    from openpano_amd import hip, synth
    from openpano_amd.config import PanoConfig
    H, W, n = 867, 1300, 38
    dev = torch.device("cuda", 0)
    views = synth.image_set(n, H, W, seed=38, overlap=0.45, rows=2, shuffle=True)
    d_imgs = [torch.from_numpy(v).to(dev) for v in views]
    inputs = [(t.data_ptr(), H, W) for t in d_imgs]
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(stream)
    ctx = hip.Context(0, stream.cuda_stream)
    homos = bench.run_blend(hip, ctx, PanoConfig(), inputs, H, W, argparse.Namespace(steps=1), lambda m: None)["_homos"]

    def timed(fn, stage):
        fn()                                                     # warm-up (tables, pool)
        ctx.set_profiling(True); ctx.profile_reset()
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(a.steps):
            fn()
        torch.cuda.synchronize(); wall = (time.perf_counter() - t0) / a.steps * 1e3
        prof = {k: v[0] / a.steps for k, v in ctx.profile().items()}
        ctx.set_profiling(False)
        return {"kernel_ms": round(prof.get(stage, float("nan")), 4), "wall_ms": round(wall, 4)}

    out = {"_meta": {"lib_sha256_16": hashlib.sha256(open(hip.LIB_PATH, "rb").read()).hexdigest()[:16],
                     "device": torch.cuda.get_device_name(0), "steps": a.steps,
                     "workload": f"config 4 blend geometry: {n} x {W}x{H} resident views, spherical, 2-row sweep (bench.run_blend)"}}
    lin = hip.BlendCall(ctx, PanoConfig(MULTIBAND=0), inputs, homos, 2, n // 2)
    out["canvas"] = None
    for s in (1, 2, 4):
        out[f"gain_overlap_stride{s}"] = timed(lambda: lin.overlap_sums(s), "gain overlap")
    count, sums = lin.overlap_sums(1)
    t0 = time.perf_counter()
    gains = hip.gain_solve(n, count, sums)
    out["gain_solve_host_ms"] = round((time.perf_counter() - t0) * 1e3, 4)
    out["pairs_overlapping"] = int((count > 0).sum())
    out["gains_range"] = [float(gains.min()), float(gains.max())]
    for key, mb in (("linear", 0), ("multiband5", 5)):
        plain = hip.BlendCall(ctx, PanoConfig(MULTIBAND=mb), inputs, homos, 2, n // 2)
        gained = hip.BlendCall(ctx, PanoConfig(MULTIBAND=mb), inputs, homos, 2, n // 2, gains=gains)
        stage = "blend linear" if mb == 0 else "multiband first level"
        out[f"{key}_op_blend"] = timed(lambda: plain().free(), stage)
        out[f"{key}_op_blend_gains"] = timed(lambda: gained().free(), stage)
        cv = plain(); out["canvas"] = [cv.h, cv.w]; cv.free()
    ctx.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
