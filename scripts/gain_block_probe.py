#!/usr/bin/env python3
"""Timing of block gain compensation on config 4's blend geometry (GPU box), next to gain_probe.py's per-image numbers:
op_gain_block_overlap at strides 1, 2, 4 for 4 x 4 blocks (and 8 x 8 at stride 1 and 2) against op_gain_overlap,
op_gain_block_solve on the host, and op_blend_block_gains against op_blend_gains for the linear and the 5-band blender.
Kernel times from the context's HIP-event profile (mean of `--steps` calls after one warm-up), wall times per call; one
JSON object on stdout, with the library's hash.

    python scripts/gain_block_probe.py [--steps 10] [--out profiles/gain_block_probe_latest.json]"""
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
    for s in (1, 2, 4):
        out[f"gain_overlap_stride{s}"] = timed(lambda: lin.overlap_sums(s), "gain overlap")
        out[f"gain_block_overlap_4x4_stride{s}"] = timed(lambda: lin.block_overlap_sums(4, 4, s), "gain block overlap")
    for s in (1, 2):
        out[f"gain_block_overlap_8x8_stride{s}"] = timed(lambda: lin.block_overlap_sums(8, 8, s), "gain block overlap")
    count1, sums1 = lin.overlap_sums(1)
    t0 = time.perf_counter()
    g_img = hip.gain_solve(n, count1, sums1)
    out["gain_solve_host_ms"] = round((time.perf_counter() - t0) * 1e3, 4)
    count, sums = lin.block_overlap_sums(4, 4, 1)
    for pc in (True, False):
        t0 = time.perf_counter()
        gains = hip.gain_block_solve(n, 4, 4, count, sums, per_channel=pc)
        out[f"gain_block_solve_4x4_host_ms_{'per_channel' if pc else 'grey'}"] = round((time.perf_counter() - t0) * 1e3, 4)
    out["block_unknowns_4x4"] = int(n * 16)
    out["unit_pairs_overlapping_4x4"] = int((count > 0).sum())
    out["block_gains_range"] = [float(gains.min()), float(gains.max())]
    gains = hip.gain_block_solve(n, 4, 4, count, sums)
    for key, mb in (("linear", 0), ("multiband5", 5)):
        per_image = hip.BlendCall(ctx, PanoConfig(MULTIBAND=mb), inputs, homos, 2, n // 2, gains=g_img)
        blocks = hip.BlendCall(ctx, PanoConfig(MULTIBAND=mb), inputs, homos, 2, n // 2, gains=gains)
        stage = "blend linear" if mb == 0 else "multiband first level"
        out[f"{key}_op_blend_gains"] = timed(lambda: per_image().free(), stage)
        out[f"{key}_op_blend_block_gains"] = timed(lambda: blocks().free(), stage)
    # config 5's size at 4 x 4: 128 images, 2048 unknowns -- the dense solve on synthetic statistics (a chain + random pairs)
    import numpy as np
    rng = np.random.default_rng(5)
    n5, B = 128, 16
    P5 = n5 * (n5 - 1) // 2
    c5 = np.zeros((P5, B, B), np.int64); s5 = np.zeros((P5, B, B, 6), np.int64)
    for a_ in range(n5 - 1):
        for b_ in (a_ + 1, min(a_ + 8, n5 - 1)):
            p = hip.pair_index(n5, a_, b_) if b_ > a_ else None
            if p is None:
                continue
            N = rng.integers(1, 5000, (B, B)); N[rng.uniform(size=(B, B)) < 0.6] = 0
            c5[p] = N
            s5[p] = (rng.uniform(0.2, 0.8, (B, B, 6)) * N[..., None] * hip.GAIN_FIX).astype(np.int64)
    t0 = time.perf_counter()
    hip.gain_block_solve(n5, 4, 4, c5, s5, per_channel=False)
    out["gain_block_solve_config5_size_grey_host_ms"] = round((time.perf_counter() - t0) * 1e3, 4)
    ctx.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
