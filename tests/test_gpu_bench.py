"""A plain `bench.py --gpus 1 --steps K --warmup W` on the GPU: the headline line and nothing else, within 30 s outside its steps."""
import json
import os
import subprocess
import sys
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_a_plain_bench_run_prints_the_headline_and_spends_under_30_s_outside_its_steps(tmp_path):
    """The whole run in a new process, from start to exit, less (K + W) x ms_per_step, at the default workload (measured: 3.1-4.1 s; the bound
    is the one the run is held to).  None of the --full legs ran: their keys are null.  --dump-outputs still writes its six arrays."""
    steps, warmup = 3, 1
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    t0 = time.monotonic()
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                        "--dump-outputs", str(tmp_path / "dump")], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    wall = time.monotonic() - t0
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert sum(ln.startswith('{"metric"') for ln in lines) == 1
    rec = json.loads(lines[-1])                      # the record is the LAST stdout line
    assert rec["unit"] == "frames/s" and rec["higher_is_better"] is True and rec["dtype"] == "bf16" and rec["full"] is False
    assert (rec["n_gpus"], rec["steps"], rec["warmup"]) == (1, steps, warmup)
    assert rec["ms_per_step"] > 0 and abs(rec["value"] - 128 / rec["ms_per_step"] * 1e3) < 1e-6 * rec["value"]
    outside = wall - (steps + warmup) * rec["ms_per_step"] / 1e3
    print("whole run %.2f s, ms_per_step %.3f, outside the steps %.2f s" % (wall, rec["ms_per_step"], outside))
    assert outside <= 30.0, (wall, rec["ms_per_step"])
    for key in ("graph_equals_eager", "sharded_equals_unsharded", "strong", "kernels", "roofline", "calibration", "cpu_baseline", "gpu_stock_baseline",
                "latency", "configs", "training", "host_streaming"):
        assert rec[key] is None, key
    assert sorted(os.listdir(tmp_path / "dump")) == ["cls_a_sample.npy", "cls_b_sample.npy", "cls_item0.npy", "loc_a_sample.npy", "loc_b_sample.npy", "loc_item0.npy"]
