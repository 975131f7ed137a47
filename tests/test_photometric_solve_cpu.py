"""CPU: the host-only units of the blend stage -- the photometric solvers (openpano_amd/csrc/photometric_solve.cc) and the
canvas geometry (blend_geom.cc) -- compiled with tests/harness/photometric_solve_harness.cc into a program of its own under
AddressSanitizer and UndefinedBehaviorSanitizer: every accepted size class of op_gain_solve / op_gain_block_solve up to the
largest, one over it, op_vignette_solve into each of its refusals, op_blend_prepare / op_blend_canvas_dims /
op_cyl_warp_shape and the blur taps at their limit.  Nothing is loaded into Python and nothing is preloaded.  The numbers
these functions return are checked by test_gain_solve_cpu.py, test_gain_block_solve_cpu.py, test_vignette_solve_cpu.py and
test_blend_host_cpu.py."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "openpano_amd", "csrc")


def test_sanitizer_program(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ missing")
    exe = str(tmp_path / "photometric_solve_harness")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                           "-Wall", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                           os.path.join(ROOT, "tests", "harness", "photometric_solve_harness.cc"),
                           os.path.join(CSRC, "photometric_solve.cc"), os.path.join(CSRC, "blend_geom.cc"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    m = re.search(r"photometric_solve_harness: (\d+) checks passed", r.stdout)
    assert m and int(m.group(1)) > 300, r.stdout[-1000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
