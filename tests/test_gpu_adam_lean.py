"""Lean Adam over the grid slabs (TCNN_ADAM_LEAN, csrc/kernels.hip k_adam<LEAN>): the one-call training
step stores no grid gradients (bit 1: they are summed again from the slabs when a caller asks) and keeps
one step count per 256-parameter block while the block's parameters agree on it (bit 2; not in the default
mask, so the tests of the block counts build their trainer with both bits). Only the bytes
moved change: parameters, Adam state, gradients and loss must be bit-identical to TCNN_ADAM_LEAN=0 on
twin trainers (config_hash, seed 1337), whenever and however often the getters are called.

Batch sizes: 256 -- one chunk, most fine-level entries untouched, so blocks diverge; 16384 -- two slabs;
65792 -- eight chunks, about eight hits per fine-level entry: most blocks uniform, some not."""
import ctypes

import numpy as np
import pytest

from helpers import CONFIG_HASH, adam_arrays, assert_adam_bits, make_batch, trainer_arrays

pytestmark = pytest.mark.gpu

BATCHES = (256, 16384, 65792)
ALL = ("w32", "w16", "m1", "m2", "steps", "g16", "g32")
BLOCK = 256
MASKS = [None, 3]  # the default switch, and both bits


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


def _trainer(monkeypatch, mask=None):
    """the switch is read when the trainer is built (as TCNN_WT_STORES in test_gpu_store_policy.py);
    None: the default"""
    from tinycudann import Trainer
    if mask is None:
        monkeypatch.delenv("TCNN_ADAM_LEAN", raising=False)
    else:
        monkeypatch.setenv("TCNN_ADAM_LEAN", str(mask))
    t = Trainer(2, 3, CONFIG_HASH, seed=1337)
    monkeypatch.delenv("TCNN_ADAM_LEAN", raising=False)
    assert t.engine == "fused"
    return t


_batches = {}


def _batch(torch, B, step):
    """device batch (B, step), made once and shared by every test (never written)"""
    if (B, step) not in _batches:
        pos, tgt = make_batch(B, step=step)
        _batches[(B, step)] = (torch.from_numpy(pos).cuda(), torch.from_numpy(tgt).cuda())
    return _batches[(B, step)]


def _arrays(t):
    """everything the getters hand out (this makes the trainer eager / per-parameter from here on)"""
    a = adam_arrays(t)
    a["g32"] = trainer_arrays(t)["g32"]
    return a


def _same_loss(a, b, what):
    la, lb = np.float32(a.loss()).view(np.uint32), np.float32(b.loss()).view(np.uint32)
    assert la == lb, (what, hex(int(la)), hex(int(lb)))


def _blocks(t):
    """(uniform blocks, blocks) of the trainer's grid range -- the debug entry (csrc/debug_adam.h), no getter"""
    from tinycudann import _lib as L
    f = L.lib().tcnn_debug_adam_uniform_blocks
    f.restype, f.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    u, n = ctypes.c_uint32(0), ctypes.c_uint32(0)
    L.check(f(t.h, ctypes.byref(u), ctypes.byref(n)))
    return u.value, n.value


def _equal_count_blocks(t, steps):
    """256-blocks (aligned to the first grid parameter, the last one partial) of the grid range of the
    per-parameter counts `steps` whose counts are all equal"""
    s = np.asarray(steps, np.uint32)[t.n_network_params:]
    n_blocks = (s.size + BLOCK - 1) // BLOCK
    pad = np.full(n_blocks * BLOCK - s.size, s[(n_blocks - 1) * BLOCK], np.uint32)  # the last block: its own parameters only
    b = np.concatenate([s, pad]).reshape(n_blocks, BLOCK)
    return int(np.count_nonzero((b == b[:, :1]).all(axis=1))), n_blocks


def _steps_of(t):
    return t.optimizer_state()[2].cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("B", BATCHES)
def test_four_steps_without_getters_then_one_read_out(torch_mod, monkeypatch, B, mask):
    """the lazy materialisation of the gradients and the expansion of the block counts"""
    lean, full = _trainer(monkeypatch, mask), _trainer(monkeypatch, 0)
    for s in range(4):
        p, g = _batch(torch_mod, B, s)
        lean.training_step(p, g)
        full.training_step(p, g)
        _same_loss(lean, full, (B, s))
    assert_adam_bits(_arrays(lean), _arrays(full), ("read-out", B), names=ALL)


@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("B", BATCHES)
def test_getters_after_every_step(torch_mod, monkeypatch, B, mask):
    """the first call is lazy; the later steps store eagerly and count per parameter, and the pointers
    handed out the first time keep seeing fresh values"""
    lean, full = _trainer(monkeypatch, mask), _trainer(monkeypatch, 0)
    cached = None
    for s in range(4):
        p, g = _batch(torch_mod, B, s)
        lean.training_step(p, g)
        full.training_step(p, g)
        _same_loss(lean, full, (B, s))
        ref = _arrays(full)
        assert_adam_bits(_arrays(lean), ref, ("every step", B, s), names=ALL)
        if cached is None:
            cached = (lean.param_gradients(), lean.gradients_fp32(), lean.optimizer_state()[2])
        else:  # views made after step 0, never asked for again
            torch_mod.cuda.synchronize()
            got = {"g16": cached[0].cpu().numpy().view(np.uint16), "g32": cached[1].cpu().numpy(),
                   "steps": cached[2].cpu().numpy().view(np.uint32)}
            assert_adam_bits(got, ref, ("cached pointers", B, s), names=("g16", "g32", "steps"))


@pytest.mark.parametrize("B", BATCHES)
def test_block_is_uniform_exactly_when_its_counts_are_equal(torch_mod, monkeypatch, B):
    lean, full = _trainer(monkeypatch, 3), _trainer(monkeypatch, 0)
    assert _blocks(lean)[0] == _blocks(lean)[1] > 0  # every block starts uniform at count 0
    for s in range(4):
        p, g = _batch(torch_mod, B, s)
        lean.training_step(p, g)
        full.training_step(p, g)
        want, n_blocks = _equal_count_blocks(full, _steps_of(full))
        got, n = _blocks(lean)
        print(f"B={B} step={s}: uniform blocks {got} of {n}, equal-count blocks in the twin {want} of {n_blocks}")
        assert n == n_blocks
        assert got == want, (B, s, got, want)
        if B == 65792:  # both paths of the kernel run
            assert 0 < got < n, (s, got, n)
    assert_adam_bits(_arrays(lean), _arrays(full), ("invariant", B), names=ALL)


def test_recompaction_after_small_batches_and_after_a_snapshot(torch_mod, monkeypatch):
    """two steps at B = 256 leave most blocks diverged; steps at B = 65792 then run on both kinds of
    block. A snapshot save + load marks every block diverged; the next step's vote makes the blocks whose
    counts are all equal uniform again (the invariant), with the twin's parameters."""
    lean, full = _trainer(monkeypatch, 3), _trainer(monkeypatch, 0)
    plan = [(256, 0), (256, 1), (65792, 0), (65792, 1)]
    seen = []
    for B, s in plan:
        p, g = _batch(torch_mod, B, s)
        lean.training_step(p, g)
        full.training_step(p, g)
        want, n_blocks = _equal_count_blocks(full, _steps_of(full))
        got, n = _blocks(lean)
        print(f"B={B} step={s}: uniform blocks {got} of {n}, twin {want}")
        assert (got, n) == (want, n_blocks), (B, s)
        seen.append(got)
    # (counts that once differ inside a block differ for good: the large batches add no uniform blocks,
    # they only keep the invariant on both kinds)
    assert 0 < seen[3] < n_blocks, seen
    # the snapshot between two steps, on both twins (loading rounds the masters through fp16)
    snap_lean, snap_full = lean.serialize(optimizer=True), full.serialize(optimizer=True)
    assert snap_lean == snap_full
    assert _blocks(lean)[0] == seen[3]  # saving expands the counts without switching
    lean.deserialize(snap_lean)
    full.deserialize(snap_full)
    assert _blocks(lean)[0] == 0
    p, g = _batch(torch_mod, 65792, 2)
    lean.training_step(p, g)
    full.training_step(p, g)
    _same_loss(lean, full, "after load")
    want, n_blocks = _equal_count_blocks(full, _steps_of(full))
    assert _blocks(lean) == (want, n_blocks)
    assert want > 0
    assert_adam_bits(_arrays(lean), _arrays(full), "after load", names=ALL)


def test_one_call_step_against_gradient_pass_and_optimizer_step(torch_mod, monkeypatch):
    """both under the default switch: the bar of test_sequential_readers_of_the_slabs"""
    one, seq = _trainer(monkeypatch), _trainer(monkeypatch)
    B = 16384
    for s in range(3):
        p, g = _batch(torch_mod, B, s)
        one.training_step(p, g, run_optimizer=True)
        seq.training_step(p, g, run_optimizer=False)
        seq.optimizer_step()
    assert_adam_bits(trainer_arrays(one), trainer_arrays(seq), "sequential", names=("w32", "w16", "g16"))


def test_lean_then_sequential_on_one_trainer(torch_mod, monkeypatch):
    """a lean step followed by the two-call step on the same trainer: optimizer_step reads per-parameter
    counts, which the lean step left in the block words"""
    mix, full = _trainer(monkeypatch, 3), _trainer(monkeypatch, 0)
    B = 16384
    for s in range(4):
        p, g = _batch(torch_mod, B, s)
        for t in (mix, full):
            if s % 2 == 0:
                t.training_step(p, g)
            else:
                t.training_step(p, g, run_optimizer=False)
                t.optimizer_step()
    assert_adam_bits(_arrays(mix), _arrays(full), "mixed schedules", names=ALL)


@pytest.mark.parametrize("mask", MASKS)
def test_graph_replay_of_lean_steps(torch_mod, monkeypatch, mask):
    torch = torch_mod
    graph, eager = _trainer(monkeypatch, mask), _trainer(monkeypatch, 0)
    graph.set_graph(True)
    B = 16384
    pos_d, tgt_d = torch.empty(B, 2, device="cuda"), torch.empty(B, 3, device="cuda")

    def run(first, n):
        for s in range(first, first + n):
            p, g = _batch(torch, B, s)
            pos_d.copy_(p)
            tgt_d.copy_(g)
            graph.training_step(pos_d, tgt_d)
            eager.training_step(pos_d, tgt_d)
            _same_loss(graph, eager, ("graph", s))

    run(0, 5)
    captures, replays = graph.graph_stats()
    assert captures >= 1 and replays >= 2, (captures, replays)
    want, n_blocks = _equal_count_blocks(eager, _steps_of(eager))
    if mask == 3:
        assert _blocks(graph) == (want, n_blocks)  # replays leave the block words like eager steps
    assert_adam_bits(_arrays(graph), _arrays(eager), "graph replay", names=ALL)
    # the getters switched the trainer to eager stores: the captured lean kernel must not be replayed
    run(5, 3)
    assert graph.graph_stats()[0] > captures
    assert_adam_bits(_arrays(graph), _arrays(eager), "graph replay after the getters", names=ALL)


@pytest.mark.parametrize("mask", [1, 2])
def test_each_bit_alone(torch_mod, monkeypatch, mask):
    lean, full = _trainer(monkeypatch, mask), _trainer(monkeypatch, 0)
    B = 16384
    for s in range(3):
        p, g = _batch(torch_mod, B, s)
        lean.training_step(p, g)
        full.training_step(p, g)
        _same_loss(lean, full, (mask, s))
    if mask & 2:
        assert _blocks(lean) == _equal_count_blocks(full, _steps_of(full))
    assert_adam_bits(_arrays(lean), _arrays(full), ("mask", mask), names=ALL)
