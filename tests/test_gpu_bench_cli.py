"""bench.py as a command on the GPU: a plain run times only its steps and says so in its
line, and --dump-outputs writes what the last timed step returned (one small workload, one
process)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_bench_run_times_its_steps_and_dumps_its_outputs(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--workload", "resnet18_ddp", "--dump-outputs", str(out)],
                       cwd=REPO, env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1
    d = lines[0]
    assert d["steps"] == 3 and d["warmup"] == 1 and d["n_gpus"] == 1 and d["full"] is False
    assert d["unit"] == "GB/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["ms_per_step"] > 0
    # value = bucket bytes of the step / its time
    step_bytes = d["config"]["bucket_bytes"] * d["config"]["buckets_per_step"]
    assert d["value"] == pytest.approx(step_bytes / d["ms_per_step"] / 1e6, rel=1e-2)
    # nothing beyond the headline figure ran
    assert d["forced_exchange"] is None and d["emulated_wire"] is None and d["roofline"] is None
    assert d["cpu_baseline"] is None and d["phase_ms"] == {}
    # the dump: each of the 3 DDP buckets' output and EF14 residual, float32, seeded sample
    names = sorted(f for f in os.listdir(out) if not f.endswith("_sums.npy"))
    assert names == sorted([f"out_b{i}.npy" for i in range(3)] + [f"residual_b{i}.npy" for i in range(3)])
    assert sum(os.path.getsize(out / f) for f in os.listdir(out)) <= 64 * 10**6
    for f in names:
        a, s = np.load(out / f), np.load(out / f.replace(".npy", "_sums.npy"))
        info = d["dumped_outputs"][f[:-4]]
        assert a.dtype == np.float32 and a.shape == (info["saved"],) and np.isfinite(a).all()
        assert s.dtype == np.float64 and s.shape == (3,) and 0 < s[2] <= info["elements"]
    # EF14 keeps about compress_ratio of each bucket's elements and zeroes them in the residual:
    # every element is non-zero in exactly one of the two (but for a normal draw of exactly 0.0,
    # which millions of float32 draws can hold a few of)
    for i in range(3):
        n = d["dumped_outputs"][f"out_b{i}"]["elements"]
        kept = np.load(out / f"out_b{i}_sums.npy")[2]
        left = np.load(out / f"residual_b{i}_sums.npy")[2]
        assert 0.1 * n < kept < 0.3 * n and n - 4 <= kept + left <= n
