#!/usr/bin/env python3
"""Timing of cylinder mode's perspective correction on the device (GPU box).  With the context's HIP-event
profile: the kernel time of op_canvas_perspective on the panorama of the 4-view case (natural.config_views(2, 4)) and on one
synthetic 900 x 8000 canvas; a whole HipCylinderStitcher::build_canvas(true) on the 4-view case, as `stitch_demo ... cylinder_build
--crop --profile` reports it for its second build on a warm context (every stage of the context's profile, their sum over the
device stages and over the host ones, and the wall time of the call); the fp32 bytes that no longer cross PCIe; and the path
the device pass replaces, in this process: op_canvas_copy of the blended canvas plus the pass on one host thread
(tests/harness/perspective_harness.cc --time, the C++ twin of perspective_cases.perspective_ref, built here with -O3).
One JSON object on stdout, with the library's hash.

    python scripts/cylinder_probe.py [--steps 10] [--out profiles/cylinder_probe_latest.json]"""
import argparse
import hashlib
import json
import os
import re
import shutil
import struct
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
CSRC = os.path.join(ROOT, "openpano_amd", "csrc")
DEMO = os.path.join(ROOT, "openpano_amd", "host", "stitch_demo")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import natural
    import perspective_cases as pc
    from openpano_amd import hip
    from openpano_amd.config import PanoConfig
    cfg = PanoConfig(CYLINDER=1, ESTIMATE_CAMERA=0, ORDERED_INPUT=1, LAZY_READ=0)
    ctx = hip.Context(0)
    tmp = tempfile.mkdtemp(prefix="cylinder_probe")

    def spread(ms):
        return {"mean": round(float(np.mean(ms)), 4), "min": round(float(np.min(ms)), 4), "max": round(float(np.max(ms)), 4)}

    host_exe = None
    if shutil.which("g++"):
        host_exe = os.path.join(tmp, "perspective_harness")
        subprocess.check_call(["g++", "-std=c++17", "-O3", "-ffp-contract=off", "-Wno-unknown-pragmas", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                               os.path.join(ROOT, "tests", "harness", "perspective_harness.cc"), os.path.join(CSRC, "blend_geom.cc"), "-o", host_exe])

    def probe(canvas, inv):
        h, w = canvas.shape[:2]
        cv = hip.Canvas.upload(ctx, canvas)
        out = cv.perspective(inv, cfg)                       # warm-up (pool, code object), and the check
        r = {"h": h, "w": w, "fp32_bytes": int(canvas.nbytes), "equals_restatement": bool(np.array_equal(out.numpy(), pc.perspective_ref(canvas, inv, 1, 0)))}
        out.free()
        ctx.set_profiling(True); ctx.profile_reset()
        for _ in range(a.steps):
            cv.perspective(inv, cfg).free()
        r["perspective_kernel_ms"] = round(ctx.profile()["perspective"][0] / a.steps, 4)
        ctx.set_profiling(False)
        ms = []
        for _ in range(a.steps):
            ctx.sync(); t0 = time.perf_counter()
            cv.perspective(inv, cfg).free()
            ctx.sync(); ms.append((time.perf_counter() - t0) * 1e3)
        r["op_canvas_perspective_wall_ms"] = spread(ms)
        ms = []
        for _ in range(a.steps):
            t0 = time.perf_counter()
            cv.numpy()
            ms.append((time.perf_counter() - t0) * 1e3)
        r["replaced_op_canvas_copy_wall_ms"] = spread(ms)
        if host_exe:
            txt = subprocess.run([host_exe, "--time", str(h), str(w), str(max(2, a.steps // 3))], capture_output=True, text=True, check=True, timeout=600).stdout
            r["replaced_host_pass_one_thread_ms"] = float(re.search(r": ([0-9.]+) ms", txt).group(1))
        else:
            r["replaced_host_pass_one_thread_ms"] = "not measured: g++ not available"
        # what no longer crosses PCIe per panorama: the blended canvas coming back as fp32 (the corrected one goes out as the
        # encoder's file instead of fp32 as well, which hip_write_png / hip_write_jpeg already spared camera mode)
        r["fp32_bytes_no_longer_over_pcie"] = int(canvas.nbytes)
        cv.free()
        return r

    out = {"_meta": {"lib_sha256_16": hashlib.sha256(open(hip.LIB_PATH, "rb").read()).hexdigest()[:16], "steps": a.steps, "host_threads": 1,
                     "note": "one run on one machine"}}
    # the 4-view case through the program: out.bin holds the blend before the correction and the map
    views = natural.config_views(2, 4)
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<3i", len(views), *views[0].shape[:2]))
        for v in views:
            f.write(natural.u8_to_f32(v).tobytes())
    subprocess.run([DEMO, fin, fout, "38", "cylinder"], capture_output=True, check=True, timeout=300)
    builds = []
    for _ in range(max(2, a.steps // 3)):
        err = subprocess.run([DEMO, fin, os.path.join(tmp, "build.bin"), "38", "cylinder_build", "--crop", "--profile"], capture_output=True,
                             text=True, check=True, timeout=300).stderr
        m = re.search(r"build_canvas: ([0-9.]+) ms device stages, ([0-9.]+) ms host stages, ([0-9.]+) ms wall", err)
        builds.append({"device_stages_ms": float(m.group(1)), "host_stages_ms": float(m.group(2)), "wall_ms": float(m.group(3)),
                       "stages_ms": {lab: float(ms) for ms, lab in re.findall(r"profile: ([0-9.]+) ms, [0-9]+ calls: (.*)", err)}})
    buf = open(fout, "rb").read()
    o = 4
    for _ in range(len(views)):
        k = struct.unpack_from("<i", buf, o)[0]; o += 4 + 16 * k
    na = struct.unpack_from("<i", buf, o)[0]; o += 4 + 12 * na + 4 + 72 * len(views)
    h, w = struct.unpack_from("<2i", buf, o); o += 8
    pre = np.frombuffer(buf, np.float32, h * w * 3, o).reshape(h, w, 3).copy(); o += pre.nbytes + 64
    inv = np.frombuffer(buf, np.float64, 9, o).reshape(3, 3).copy()
    out["views_4x400x600"] = probe(pre, inv)
    out["views_4x400x600"]["build_canvas_crop"] = {"device_stages_ms": spread([b["device_stages_ms"] for b in builds]),
                                                   "host_stages_ms": spread([b["host_stages_ms"] for b in builds]),
                                                   "wall_ms": spread([b["wall_ms"] for b in builds]), "stages_ms_last_run": builds[-1]["stages_ms"]}
    out["views_4x400x600"]["update_h_factor_attempts"] = na
    # one synthetic panorama-sized canvas under a mild correction
    rng = np.random.default_rng(18)
    big = rng.random((900, 8000, 3), dtype=np.float32)
    big[:20] = -1; big[-20:] = -1
    mild = np.array([[1.02, 0.03, -0.4], [0.01, 0.98, 0.3], [0.05 / 8000, -0.03 / 900, 1.0]])
    out["synthetic_900x8000"] = probe(big, mild)
    ctx.close()
    shutil.rmtree(tmp, ignore_errors=True)
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
