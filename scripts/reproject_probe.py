#!/usr/bin/env python3
"""Timing of the re-projection of a finished panorama on the device (GPU box).  From a synthetic 763 x 7999
canvas (config 4's size) that spans one turn: a 1000 x 1000 planet, one 1920 x 1080 view, and the six 1024 x 1024 faces of a cube
-- the kernel time from the context's HIP-event profile (stage "reproject") and the wall time of the calls; and the path they
replace, in this process: op_canvas_copy of the canvas plus the same loops on one host thread (tests/harness/reproject_harness.cc
--time, the C++ twin of tests/reproject_cases.py, built with -O3).  Back-to-back calls read the canvas from the last-level cache,
as section 18.5 says of its own numbers.  One JSON object on stdout, with the library's hash.

    python scripts/reproject_probe.py [--steps 10] [--host-exe PATH] [--out profiles/reproject_probe_latest.json]"""
import argparse
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
CSRC = os.path.join(ROOT, "openpano_amd", "csrc")
H, W = 763, 7999


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--host-exe", default=None, help="reproject_harness built with -O3 (built here when absent and g++ exists)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import reproject_cases as rc
    from openpano_amd import hip
    ctx = hip.Context(0)
    tmp = tempfile.mkdtemp(prefix="reproject_probe")

    def spread(ms):
        return {"mean": round(float(np.mean(ms)), 4), "min": round(float(np.min(ms)), 4), "max": round(float(np.max(ms)), 4)}

    host_exe = a.host_exe
    if not host_exe and shutil.which("g++"):
        host_exe = os.path.join(tmp, "reproject_harness")
        subprocess.check_call(["g++", "-std=c++17", "-O3", "-ffp-contract=off", "-Wno-unknown-pragmas", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                               os.path.join(ROOT, "tests", "harness", "reproject_harness.cc"), os.path.join(CSRC, "blend_geom.cc"), "-o", host_exe])

    rng = np.random.default_rng(19)
    pano = rng.random((H, W, 3), dtype=np.float32)
    frame = (-rc.PI, -rc.PI_2 * 0.2, rc.TWO_PI / W, rc.PI * 0.2 / H, 1)         # what the harness's --time uses
    cframe = hip.OpPanoFrame(*[float(v) for v in frame[:4]], 1)
    cv = hip.Canvas.upload(ctx, pano)
    jobs = {"planet_1000": [hip.view_planet(1000)], "view_1920x1080": [hip.view_look(0.3, 0.02, 0.0, 1.2, 1920, 1080)],
            "cube_6x1024": [hip.view_cube_face(f, 1024) for f in range(6)]}
    out = {"_meta": {"lib_sha256_16": hashlib.sha256(open(hip.LIB_PATH, "rb").read()).hexdigest()[:16], "steps": a.steps, "host_threads": 1,
                     "canvas": [H, W], "canvas_fp32_bytes": int(pano.nbytes), "note": "one run on one machine; back-to-back calls"}}
    ms = []
    for _ in range(a.steps):
        t0 = time.perf_counter()
        cv.numpy()
        ms.append((time.perf_counter() - t0) * 1e3)
    out["replaced_op_canvas_copy_wall_ms"] = spread(ms)
    for name, specs in jobs.items():
        r = {"outputs": [[s.out_h, s.out_w] for s in specs]}
        first = cv.reproject(cframe, specs[0])                  # warm-up (pool, code object), and the check of the first output
        view = (specs[0].out_h, specs[0].out_w, np.array(list(specs[0].rot)), specs[0].focal)
        want = rc.planet_ref(pano, specs[0].out_h, 1) if specs[0].mode == hip.VIEW_PLANET else rc.rectilinear_ref(pano, frame, view)
        r["equals_restatement"] = bool(np.array_equal(first.numpy(), want))
        r["sampled_share"] = round(float((want[..., 0] >= 0).mean()), 4)
        first.free()
        for s in specs[1:]:
            cv.reproject(cframe, s).free()
        ctx.set_profiling(True); ctx.profile_reset()
        for _ in range(a.steps):
            for s in specs:
                cv.reproject(cframe, s).free()
        r["reproject_kernel_ms"] = round(ctx.profile()["reproject"][0] / a.steps, 4)
        ctx.set_profiling(False)
        ms = []
        for _ in range(a.steps):
            ctx.sync(); t0 = time.perf_counter()
            for s in specs:
                cv.reproject(cframe, s).free()
            ctx.sync(); ms.append((time.perf_counter() - t0) * 1e3)
        r["op_canvas_reproject_wall_ms"] = spread(ms)
        if host_exe:
            what = name.split("_")[0]
            txt = subprocess.run([host_exe, "--time", what, str(H), str(W), str(max(2, a.steps // 3))], capture_output=True, text=True, check=True, timeout=900).stdout
            r["replaced_host_loop_one_thread_ms"] = float(re.search(r"([0-9.]+) ms", txt).group(1))
        else:
            r["replaced_host_loop_one_thread_ms"] = "not measured: g++ not available"
        out[name] = r
    cv.free()
    ctx.close()
    shutil.rmtree(tmp, ignore_errors=True)
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
