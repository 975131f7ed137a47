#!/usr/bin/env python3
"""Timing of the blend from decoder bytes and from resident views (GPU box) on a config-4-shaped scene:
synth.pano_scene(38, 867, 1300, proj="camera"), spherical projection, the linear and the 5-band blender, with the views
quantised to bytes b and the fp32 views f = b / 255 those bytes stand for.  Four legs per blender:

    host_f32       numpy fp32 views in pageable memory: 12 h w bytes per view uploaded by every call (the path before views)
    host_u8        numpy bytes: 3 h w per view uploaded by every call, converted in the sampler
    resident_f32   fp32 views already on the device (device pointers)
    resident_u8    one hip.Views upload of the bytes, read by every call

Per leg: 2 warm-up calls, then `--steps` calls timed ONE BY ONE -- wall time around the call (op_blend synchronises its
stream before it returns) and the kernel time of the context's HIP-event profile -- reported as median, min and max.
`kernel_ms` is the kernel that reads the sources ("blend linear" / "multiband first level"); `all_kernels_ms` every
bracketed device stage of the call.  The canvases of the four legs are compared (they must be equal).

    python scripts/views_probe.py [--steps 10] [--out profiles/views_probe_latest.json] [--scene-cache /tmp/scene.npz]"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--n", type=int, default=38)
    ap.add_argument("--out", default=None)
    ap.add_argument("--modes", default="linear,multiband5", help="blenders to time (a library from before this probe faults in "
                    "the multiband first level on this scene -- DESIGN section 12 -- so it is given linear alone)")
    ap.add_argument("--scene-cache", default=None, help="npz to keep the scene's bytes in between runs (20 s of CPU to render)")
    a = ap.parse_args()
    import numpy as np
    import torch
    from openpano_amd import hip, synth
    from openpano_amd.config import PanoConfig
    H, W, n = 867, 1300, a.n
    dev = torch.device("cuda", 0)
    if a.scene_cache and os.path.exists(a.scene_cache):
        z = np.load(a.scene_cache)
        b, homos = list(z["b"]), z["homos"]
        assert len(b) == n and b[0].shape == (H, W, 3)
    else:
        views, homos = synth.pano_scene(n, H, W, seed=38, proj="camera")
        b = [np.ascontiguousarray((v * 255).astype(np.uint8)) for v in views]
        del views
        if a.scene_cache:
            np.savez(a.scene_cache, b=np.stack(b), homos=homos)
    f = [(x.astype(np.float64) / 255).astype(np.float32) for x in b]
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(stream)
    ctx = hip.Context(0, stream.cuda_stream)
    d_f = [torch.from_numpy(v).to(dev) for v in f]
    resident = hip.Views.upload(ctx, np.stack(b))
    legs = {"host_f32": f, "resident_f32": [(t.data_ptr(), H, W) for t in d_f], "host_u8": b, "resident_u8": resident}
    torch.cuda.synchronize()

    def stat(xs):
        return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}

    def timed(call, stage):
        for _ in range(2):
            call().free()                                         # warm-up: code objects, tables, pool
        wall, kern, allk = [], [], []
        ctx.set_profiling(True)
        for _ in range(a.steps):
            ctx.profile_reset()
            torch.cuda.synchronize(); t0 = time.perf_counter()
            cv = call()
            wall.append((time.perf_counter() - t0) * 1e3)
            cv.free()
            prof = ctx.profile()
            kern.append(prof[stage][0])
            allk.append(sum(v[0] for k, v in prof.items() if not k.endswith("(host)")))
        ctx.set_profiling(False)
        return {"wall_ms": stat(wall), "kernel_ms": stat(kern), "all_kernels_ms": stat(allk)}

    out = {"_meta": {"lib_sha256_16": hashlib.sha256(open(hip.LIB_PATH, "rb").read()).hexdigest()[:16],
                     "device": torch.cuda.get_device_name(0), "steps": a.steps,
                     "workload": f"synth.pano_scene({n}, {H}, {W}, seed=38, proj='camera'), spherical",
                     "view_bytes": {"f32": 12 * H * W * n, "u8": 3 * H * W * n}}}
    for key, mb in (("linear", 0), ("multiband5", 5)):
        if key not in a.modes.split(","):
            continue
        cfg = PanoConfig(MULTIBAND=mb)
        stage = "blend linear" if mb == 0 else "multiband first level"
        ref = None
        out[key] = {}
        for leg, images in legs.items():
            call = hip.BlendCall(ctx, cfg, images, homos, 2, n // 2)
            out[key][leg] = timed(call, stage)
            cv = call(); got = cv.numpy(); out["canvas"] = [cv.h, cv.w]; cv.free()
            if ref is None:
                ref = got
            out[key][leg]["equals_host_f32"] = bool(np.array_equal(got, ref))
    resident.free()
    ctx.close()
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as fo:
            fo.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
