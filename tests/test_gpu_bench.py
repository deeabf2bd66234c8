"""-m gpu: a plain `bench.py` run -- set-up, warm-up, exactly K timed steps, one JSON line -- and what it writes with
--dump-outputs: the network output of the last timed step, the same in every launch form, and the same as the network
gives when fed the bench's frames in the bench's order."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS, WARMUP = 7, 3


def _plain_bench(out_dir, mode):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "CBINFER_FORCE_DIST")}
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", str(STEPS), "--warmup",
           str(WARMUP), "--mode", mode, "--dump-outputs", str(out_dir)]
    out = subprocess.run(cmd, env=env, cwd=REPO, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert out.returncode == 0, out.stderr.decode()[-3000:]
    lines = [l for l in out.stdout.decode().splitlines() if l.startswith("{")]
    assert len(lines) == 1, lines            # the record alone: no details line
    r = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in r, k
    assert r["steps"] == STEPS and r["warmup"] == WARMUP and r["config"]["launch"] == mode
    assert r["ms_per_step"] == pytest.approx(1e3 * r["timed_region_s"] / STEPS, rel=1e-6)
    assert r["value"] == pytest.approx(STEPS / r["timed_region_s"], rel=1e-6)
    assert "roofline" not in r and "cpu_baseline" not in r and "literal_regions_s" not in r     # (--full only)
    assert os.listdir(out_dir) == ["output.npy"]
    return np.load(os.path.join(out_dir, "output.npy"))


def test_plain_bench_times_k_steps_and_dumps_the_last_output(tmp_path):
    import bench
    got = {m: _plain_bench(tmp_path / m, m) for m in ("eager", "program")}
    assert got["eager"].dtype == np.float32 and np.isfinite(got["eager"]).all()
    assert np.array_equal(got["eager"], got["program"])
    # the bench's walk (run_sequences): two priming frames, then W warm-up and K timed steps back and forth over the
    # frames behind them
    _, net = bench.build_bench_model()
    allframes = bench.bench_video(1234).frames(2 + max(8, min(max(STEPS, WARMUP), 256)))
    walk = allframes[2:]
    with torch.no_grad():
        for f in allframes[:2]:
            net(f)
        for i in range(WARMUP + STEPS):
            y = net(walk[bench.pingpong(i, len(walk))])
    torch.cuda.synchronize()
    assert np.array_equal(y.float().cpu().numpy(), got["eager"])
