"""GPU: a plain `bench.py` run (no --full) in a fresh process: set-up, warm-up, the timed steps, --dump-outputs and the
line -- the headline and nothing else."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_bench_run_measures_the_headline_only(tmp_path):
    detail = os.path.join(ROOT, "bench_detail.json")
    before = os.stat(detail).st_mtime_ns if os.path.exists(detail) else None
    dump = tmp_path / "outputs"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "2", "--dump-outputs", str(dump)],
                       capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == 5 and d["warmup"] == 2 and d["n_gpus"] == 1
    assert d["unit"] == "keypoints+descriptors/s" and d["higher_is_better"] is True and d["dtype"] == "f32" and d["metric"]
    # value = descriptors of one step / the step's time: the same descriptors the dump holds
    k = np.load(dump / "keypoints_per_image.npy")
    assert len(k) == d["config"]["images_per_gpu"] == 38 and k.min() > 0
    assert np.load(dump / "descriptors.npy").shape == (int(k.sum()), 128)
    assert abs(d["value"] - k.sum() / (d["ms_per_step"] * 1e-3)) < 1e-4 * d["value"]
    assert d["roofline"]["frac"] > 0 and d["stage_ms"]
    # nothing beyond the headline ran, and no record was written
    assert not {"match", "ransac", "blend", "ingest", "stitch_e2e", "configs", "config5", "parity", "detail"} & set(d)
    assert d["cpu_baseline"] is None and d["parity_checked"] is None
    assert (os.stat(detail).st_mtime_ns if os.path.exists(detail) else None) == before
