"""A variant of libopenpano_hip.so: one translation unit recompiled with extra -D flags, linked with the objects the build left
next to the sources.  Tests reach branches this way that the shipped constants keep out of reach (test_gpu_sift.py: the raw-extrema
overflow of the row kernel; test_gpu_png_variant.py: the Huffman length limiter), and run the variant in a child process that
finds it through OPENPANO_HIP_LIB."""
import glob
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "openpano_amd", "csrc")


def build_variant(out_dir, stem, flags):
    """csrc/<stem>.hip compiled with ``flags`` (a list), every other unit taken prebuilt (or compiled as the Makefile does where
    its object is missing) -> path of the variant library in ``out_dir``.  Skips without hipcc."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available on this box")
    base = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fopenmp", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC]
    objs = []
    jobs = []
    for src in sorted(glob.glob(os.path.join(CSRC, "*.hip"))):
        name = os.path.basename(src)[:-4]
        prebuilt = os.path.join(CSRC, name + ".o")
        if name != stem and os.path.exists(prebuilt):
            objs.append(prebuilt)
            continue
        o = os.path.join(str(out_dir), name + ".o")
        jobs.append(subprocess.Popen(base + (list(flags) if name == stem else []) + ["-c", src, "-o", o]))
        objs.append(o)
    for src in sorted(glob.glob(os.path.join(CSRC, "*.cc"))):           # host-only translation units of the library (plain g++, csrc/Makefile)
        name = os.path.basename(src)[:-3]
        prebuilt = os.path.join(CSRC, name + ".o")
        if os.path.exists(prebuilt):
            objs.append(prebuilt)
            continue
        o = os.path.join(str(out_dir), name + ".o")
        jobs.append(subprocess.Popen(["g++", "-std=c++17", "-O3", "-ffp-contract=off", "-fPIC", "-Wno-psabi", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-c", src, "-o", o]))
        objs.append(o)
    assert all(j.wait() == 0 for j in jobs)
    lib = os.path.join(str(out_dir), "libopenpano_hip_variant.so")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-fopenmp", "-o", lib] + objs)
    return lib
