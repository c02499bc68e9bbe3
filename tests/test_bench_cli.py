"""bench.py's command line without a GPU: the options a plain and a --full run take, and the files
--dump-outputs writes (dump_outputs: float arrays, a fixed seeded sample above the size cap)."""
import os
import subprocess
import sys

import numpy as np

import bench

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_help_lists_full_and_dump_outputs():
    out = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--help"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    for opt in ("--gpus", "--steps", "--warmup", "--full", "--dump-outputs"):
        assert opt in out.stdout, opt


def test_dump_outputs_writes_float_arrays(tmp_path):
    arrays = {"params": np.arange(10, dtype=np.float32), "loss": np.array([0.25], dtype=np.float64)}
    shapes = bench.dump_outputs(str(tmp_path / "d"), arrays)
    assert shapes == {"params": [10], "loss": [1]}
    assert sorted(os.listdir(tmp_path / "d")) == ["loss.npy", "params.npy"]
    p, l = np.load(tmp_path / "d" / "params.npy"), np.load(tmp_path / "d" / "loss.npy")
    assert p.dtype == np.float32 and l.dtype == np.float64
    np.testing.assert_array_equal(p, arrays["params"])
    np.testing.assert_array_equal(l, arrays["loss"])


def test_dump_outputs_samples_large_arrays_the_same_way_every_time(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_ELEMS", 64)
    a = np.arange(1000, dtype=np.float32)
    assert bench.dump_outputs(str(tmp_path / "a"), {"x": a}) == {"x": [64]}
    bench.dump_outputs(str(tmp_path / "b"), {"x": a + 1})
    xa, xb = np.load(tmp_path / "a" / "x.npy"), np.load(tmp_path / "b" / "x.npy")
    assert xa.shape == (64,) and len(set(xa.tolist())) == 64 and np.all(np.diff(xa) > 0)  # distinct, in order
    np.testing.assert_array_equal(xb, xa + 1)  # the same indices in both runs


def test_dump_stays_under_64_mb_for_three_arrays():
    assert 3 * bench.DUMP_MAX_ELEMS * 4 + 8 < 64 * 10 ** 6
