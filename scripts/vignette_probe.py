#!/usr/bin/env python3
"""Timing of vignetting compensation on config 4's blend geometry (GPU box), next to the per-image gain numbers:
op_vignette_overlap at strides 1, 2, 4 against op_gain_overlap, op_vignette_solve on the host, and op_blend_vignette
against op_blend_gains for the linear and the 5-band blender.  Kernel times from the context's HIP-event profile (mean of
`--steps` calls after one warm-up), wall times per call; one JSON object on stdout, with the library's hash.

    python scripts/vignette_probe.py [--steps 10] [--out profiles/vignette_probe_latest.json]"""
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
        out[f"vignette_overlap_stride{s}"] = timed(lambda: lin.vignette_overlap_sums(s, hip.VIG_CLIP), "vignette overlap")
    count1, sums1 = lin.overlap_sums(1)
    g_img = hip.gain_solve(n, count1, sums1)
    count, mom = lin.vignette_overlap_sums(hip.VIG_STRIDE, hip.VIG_CLIP)
    out["pairs_overlapping"] = int((count > 0).sum())
    for deg in (1, 3):
        t0 = time.perf_counter()
        gains, poly = hip.vignette_solve(n, count, mom, deg)
        out[f"vignette_solve_degree{deg}_host_ms"] = round((time.perf_counter() - t0) * 1e3, 4)
    out["vignette_curve"] = [float(x) for x in poly]          # synthetic views without falloff: a stays near 0
    out["vignette_gains_range"] = [float(gains.min()), float(gains.max())]
    for key, mb in (("linear", 0), ("multiband5", 5)):
        per_image = hip.BlendCall(ctx, PanoConfig(MULTIBAND=mb), inputs, homos, 2, n // 2, gains=g_img)
        vig = hip.BlendCall(ctx, PanoConfig(MULTIBAND=mb), inputs, homos, 2, n // 2, gains=gains, vignette=(-0.3, 0.05, -0.01))
        stage = "blend linear" if mb == 0 else "multiband first level"
        out[f"{key}_op_blend_gains"] = timed(lambda: per_image().free(), stage)
        out[f"{key}_op_blend_vignette"] = timed(lambda: vig().free(), stage)
    ctx.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
