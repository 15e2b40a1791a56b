"""The plain benchmark run (``bench.py --gpus 1 --steps K --warmup W``): the contract keys, none of the ``--full`` legs, and
``--dump-outputs DIR``: the last timed step's attention output and evicted indices, identical from run to run of the same
arguments (the inputs are seeded and the pre-warm is a step count, not a wall time)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plain_run(out_dir, steps):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "2",
           "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_bench_run_dumps_reproducible_outputs(tmp_path):
    runs = [(_plain_run(tmp_path / f"run{i}", 16), tmp_path / f"run{i}") for i in range(2)]
    for line, _ in runs:
        for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "config"):
            assert key in line, key
        assert line["metric"] == "decode_tokens_per_sec" and line["steps"] == 16 and line["value"] > 0
        assert abs(line["value"] - 1e3 / line["ms_per_step"]) < 1e-6 * line["value"]
        for key in ("cpu_baseline", "strided_prefill", "strided_prefill_more", "boundary_kernels", "per_layer_launches",
                    "configs", "stage_workloads"):
            assert key not in line, key       # --full only
    (_, a), (_, b) = runs
    out_a, out_b = np.load(a / "attn_out.npy"), np.load(b / "attn_out.npy")
    ids_a, ids_b = np.load(a / "evict_ids.npy"), np.load(b / "evict_ids.npy")
    assert out_a.dtype == np.float32 and out_a.shape == (32, 32, 1, 128) and np.isfinite(out_a).all()
    assert ids_a.dtype == np.float64 and ids_a.shape == (32, 32, 1)
    assert ids_a.min() >= 0 and ids_a.max() <= 2048          # one victim per (layer, head) among the T = 2049 slots
    assert np.array_equal(out_a, out_b) and np.array_equal(ids_a, ids_b)
