"""A plain bench.py run on the GPU: --steps sets the timed steps, the result line carries the headline
fields and none of what --full adds, and --dump-outputs writes what the last timed step left with the
caller -- equal, bit for bit, to the same seeded steps run in this process (the step's sums are
integer sums, so a rerun on the same inputs is bit-identical)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
from helpers import CONFIG_HASH

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_dumps_what_the_timed_steps_computed(tmp_path):
    import torch
    from tinycudann import Trainer
    steps, warmup, log2_b = 3, 2, 14
    d = tmp_path / "dump"
    out = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                          "--batch-log2", str(log2_b), "--dump-outputs", str(d)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    res = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in res, k
    for k in ("phase_ms", "roofline", "cpu_baseline"):  # these take runs of their own: --full
        assert k not in res, k
    assert res["steps"] == steps and res["warmup"] == warmup
    assert res["ms_per_step"] > 0 and res["value"] == pytest.approx(1000.0 / res["ms_per_step"], rel=1e-9)

    B = 1 << log2_b
    t = Trainer(2, 3, CONFIG_HASH, seed=1337)
    g = torch.Generator(device="cuda")
    g.manual_seed(1337)
    batches = []
    for _ in range(4):
        pos = torch.rand(B, 2, device="cuda", generator=g).contiguous()
        batches.append((pos, bench.rgb_field_torch(pos)))
    for i in list(range(warmup)) + list(range(steps)):
        t.training_step(*batches[i % 4])
    want = {"params": t.params().float().cpu().numpy(), "params_fp32": t.params_fp32().cpu().numpy(),
            "loss": np.array([t.loss()], dtype=np.float64)}
    assert sorted(os.listdir(d)) == sorted(k + ".npy" for k in want)
    assert res["dumped_outputs"] == {k: list(v.shape) for k, v in want.items()}
    for k, v in want.items():
        got = np.load(d / (k + ".npy"))
        assert got.dtype == v.dtype and got.dtype in (np.float32, np.float64), (k, got.dtype)
        assert np.isfinite(got).all(), k
        np.testing.assert_array_equal(got, v, err_msg=k)
    assert not np.array_equal(want["params_fp32"], Trainer(2, 3, CONFIG_HASH, seed=1337).params_fp32().cpu().numpy())  # it trained
