"""Store policy at the kernel boundaries (csrc/wt_store.h, TCNN_WT_STORES): the training step's bulk
hand-off buffers written through L2 instead of left dirty in it. Only where the bytes sit when a kernel
ends changes -- every result must stay bit-identical to TCNN_WT_STORES=0 (all plain stores)."""
import numpy as np
import pytest

from helpers import CONFIG_HASH, bits, make_batch, trainer_arrays

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


def _trainer(monkeypatch, default_policy):
    """the switch is read when the engine is built (as TCNN_GRID_BWD_STREAM in test_gpu_grid_bwd_stream.py)"""
    from tinycudann import Trainer
    if default_policy:
        monkeypatch.delenv("TCNN_WT_STORES", raising=False)
    else:
        monkeypatch.setenv("TCNN_WT_STORES", "0")
    t = Trainer(2, 3, CONFIG_HASH, seed=1337)
    monkeypatch.delenv("TCNN_WT_STORES", raising=False)
    assert t.engine == "fused"
    return t


def _batch(B, step, outside):
    pos, tgt = make_batch(B, step=step)
    if outside:  # 0.2 % of the positions outside [0, 1]: the generic per-corner path
        rng = np.random.default_rng(7 + step)
        idx = rng.choice(B, max(1, B // 500), replace=False)
        pos[idx] += rng.choice(np.array([-0.7, 1.5], np.float32), (idx.size, 1))
    return pos, tgt


def _assert_same(a, b, what, names=("w32", "w16", "g16", "g32")):
    for k in names:
        x, y = bits(a[k]), bits(b[k])
        bad = np.flatnonzero(x != y)
        assert bad.size == 0, (what, k, int(bad.size), int(bad[0]), hex(int(x[bad[0]])), hex(int(y[bad[0]])))


@pytest.mark.parametrize("outside", [False, True])
@pytest.mark.parametrize("B", [256, 16384, 65792])
def test_three_steps_bit_identical_to_plain_stores(torch_mod, monkeypatch, B, outside):
    """B = 256: one chunk, two fused workgroups, waves without a second slice; 16384: two chunks (Adam sums
    two slabs); 65792: eight chunks of 257 slices (partial last batch, waves with two slices)."""
    torch = torch_mod
    new, old = _trainer(monkeypatch, True), _trainer(monkeypatch, False)
    for s in range(3):
        pos, tgt = _batch(B, s, outside)
        p, g = torch.from_numpy(pos).cuda(), torch.from_numpy(tgt).cuda()
        old.training_step(p, g)
        new.training_step(p, g)
        assert np.float32(new.loss()).view(np.uint32) == np.float32(old.loss()).view(np.uint32)
        _assert_same(trainer_arrays(new), trainer_arrays(old), (B, outside, s))


MODE2_ENC = {"otype": "HashGrid", "n_levels": 6, "n_features_per_level": 4, "log2_hashmap_size": 14, "base_resolution": 16,
             "per_level_scale": 2.0}


@pytest.mark.parametrize("B", [256, 16384])
@pytest.mark.parametrize("case", ["mode2_d2_f4", "mode1_feature_plan"])
def test_module_grid_grad_bit_identical_to_plain_stores(torch_mod, monkeypatch, case, B):
    """The unpacked slab writers (write_slab, PACKED = false), which the config_hash step's packed pairs
    never reach: a D = 2, F = 4 grid (all F features per entry, mode 2: whole dense levels and entry
    ranges of the hashed ones) and config_hash under the feature plan (one feature per item, mode 1).
    B = 256: one chunk, replicas on the coarse levels; 16384: two chunks."""
    from test_gpu_grid_large import _module_grad, _random_dy
    enc = MODE2_ENC
    if case == "mode1_feature_plan":
        enc = CONFIG_HASH["encoding"]
        monkeypatch.setenv("TCNN_GRID_BWD_PLAN", "feature")
    pos, _ = _batch(B, 0, True)
    dy = _random_dy(B, enc["n_levels"], enc["n_features_per_level"], 5)
    monkeypatch.delenv("TCNN_WT_STORES", raising=False)
    new = _module_grad(torch_mod, enc, 2, pos, dy)
    monkeypatch.setenv("TCNN_WT_STORES", "0")
    old = _module_grad(torch_mod, enc, 2, pos, dy)
    assert np.count_nonzero(new) > new.size // 100
    bad = np.flatnonzero(new.view(np.uint32) != old.view(np.uint32))
    assert bad.size == 0, (case, B, int(bad.size), int(bad[0]), float(new[bad[0]]), float(old[bad[0]]))


def test_sequential_readers_of_the_slabs(torch_mod, monkeypatch):
    """training_step(run_optimizer=False) + optimizer_step() read the slabs through the sequential
    reductions (launch_column_sums, reduce_items) instead of the tail and k_adam: with the default
    policy they give the one-call step's parameters and fp16 gradients bit for bit. (The loss is summed
    in another order there -- the bar of test_overlapped_step_bit_identical_to_sequential.)"""
    torch = torch_mod
    one, seq = _trainer(monkeypatch, True), _trainer(monkeypatch, True)
    B = 16384
    for s in range(3):
        pos, tgt = _batch(B, s, False)
        p, g = torch.from_numpy(pos).cuda(), torch.from_numpy(tgt).cuda()
        one.training_step(p, g, run_optimizer=True)
        seq.training_step(p, g, run_optimizer=False)
        seq.optimizer_step()
        assert abs(one.loss() - seq.loss()) <= 1e-6 * abs(seq.loss())
        _assert_same(trainer_arrays(one), trainer_arrays(seq), ("sequential", s), names=("w32", "w16", "g16"))
