"""Adam's options on every path of the engine that applies the update, bit for bit against the oracle's Adam
(O.adam_step, itself checked against float64 in tests/test_adam_reference.py) fed the GPU's own fp16 gradients:
fp32 masters, fp16 copies, both moments, the per-parameter step counts and the fp16 gradients. No tolerance.

The five paths and the tests that reach them (cases: tests/adam_cases.py):
  1. k_adam over the whole vector (optimizer_step): test_standalone_kernel_* on the crafted state, every case;
     test_sequential_engines (tile and layer-wise step) and the training_step(False) + optimizer_step() twin of
     test_fused_step; test_graph_replay on the tile model.
  2. grid_bwd_mlp_tail (network parameters + the next step's weight image) and
  3. k_adam over the LDS levels' slabs: test_fused_step, every case, on config_hash; test_graph_replay.
  4. adam_store4 in the binned accumulate pass: test_binned_pass (a 2^16-entry table: levels on both sides of
     the LDS budget, test_binned_model_has_levels_on_both_passes).
  5. optimizer_step_range: test_optimizer_step_range.
"""
import json

import msgpack
import numpy as np
import pytest

import adam_cases as AC
from helpers import CONFIG_HASH, adam_arrays, assert_adam_bits, fresh_adam_state, make_batch, oracle_adam_step
from oracle import oracle as O

pytestmark = pytest.mark.gpu

ALL = ("w32", "w16", "m1", "m2", "steps", "g16")


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


def make_trainer(cfg, case):
    from tinycudann import Trainer
    t = Trainer(2, 3, AC.with_optimizer(cfg, case), seed=1337)
    t.set_loss_scale(AC.loss_scale(case))
    return t


def load_state(t, state, global_step, learning_rate):
    """masters (full precision), moments, per-parameter step counts and the optimizer's step count into the
    trainer, as a snapshot"""
    blob = msgpack.packb({"n_params": t.n_params, "params_type": "float", "params_binary": state["w32"].tobytes(),
                          "optimizer": {"current_step": int(global_step), "base_learning_rate": float(learning_rate),
                                        "first_moments_binary": state["m1"].tobytes(), "second_moments_binary": state["m2"].tobytes(),
                                        "param_steps_binary": state["steps"].astype(np.uint32).tobytes()}}, use_bin_type=True)
    t.deserialize(blob)
    assert t.optimizer_step_count == global_step


def learning_rate(case):
    return AC.optimizer_block(case).get("learning_rate", 1e-3)


def crafted_trainer(torch, cfg, case, steps=None, global_step=AC.CRAFT_GLOBAL_STEP):
    """a trainer of cfg holding the crafted state tiled over its parameters; returns (trainer, the same state on
    the host, the crafted fp16 gradients)"""
    t = make_trainer(cfg, case)
    ref = AC.tiled_state(t.n_params)
    g16 = ref.pop("g16")
    if steps is not None:
        ref["steps"] = steps(t.n_params)
    ref["w16"] = O.f2h(ref["w32"])
    load_state(t, ref, global_step, learning_rate(case))
    got = adam_arrays(t)
    assert_adam_bits(got, ref, "loaded state")
    return t, ref, g16


def set_gradients(torch, t, g16):
    """fp32 gradient sums that round to the fp16 gradients g16 (bits), zero signs included"""
    t.gradients_fp32().copy_(torch.from_numpy(O.h2f(g16)))


def step_and_compare(torch, t, case, ref, T, g16, what):
    """optimizer_step() on the fp32 gradients of g16 against one oracle step (global step T) of ref"""
    set_gradients(torch, t, g16)
    t.optimizer_step()
    oracle_adam_step(AC.optimizer_block(case), t.n_network_params, AC.loss_scale(case), T, ref, g16)
    assert t.optimizer_step_count == T
    assert_adam_bits(adam_arrays(t), dict(ref, g16=g16), what, names=ALL)


# ---------------------------------------------------------------------------------------------
# (a) the standalone kernel on the crafted state
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", AC.CASE_NAMES)
@pytest.mark.parametrize("model", ["matrix_only", "small_grid"])
def test_standalone_kernel_crafted_state(torch_mod, model, case):
    """optimizer_step() three times on the crafted state (signed zero, largest and subnormal fp16 gradients,
    zero masters of both signs, fresh parameters, step counts unlike the optimizer's) tiled over a model without
    non-matrix parameters and over a small grid model with the class boundary inside."""
    cfg = AC.CFG_SMALL_ONEBLOB if model == "matrix_only" else AC.CFG_SMALL_GRID
    t, ref, g16 = crafted_trainer(torch_mod, cfg, case)
    assert (t.n_network_params == t.n_params) == (model == "matrix_only")
    for k in range(3):
        step_and_compare(torch_mod, t, case, ref, AC.CRAFT_GLOBAL_STEP + 1 + k, np.roll(g16, 5 * k), (model, case, k))


@pytest.mark.parametrize("global_step,first", [(1026, 1022), (1023, 1019)], ids=["table_filled_past_1024", "table_grows_at_1024"])
def test_standalone_kernel_bias_table_boundary(torch_mod, global_step, first):
    """Per-parameter step counts first .. first + 4 around the 1024-step granule in which the bias-correction
    table is filled: with 1026 steps behind it the optimizer fills 2048 entries at once and the updates read both
    sides of entry 1024; with 1023 it fills 1024 entries, and the next step has to extend the table."""
    case = "combined"
    t, ref, g16 = crafted_trainer(torch_mod, AC.CFG_SMALL_GRID, case, steps=lambda n: (first + np.arange(n) % 5).astype(np.uint32),
                                  global_step=global_step)
    for k in range(3):
        step_and_compare(torch_mod, t, case, ref, global_step + 1 + k, np.roll(g16, 5 * k), (global_step, k))
    assert ref["steps"].min() <= 1024 < ref["steps"].max()


# ---------------------------------------------------------------------------------------------
# (b) optimizer_step_range
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", AC.RANGE_CASES)
def test_optimizer_step_range(torch_mod, case):
    """One range with unaligned ends across n_network_params: the oracle's update inside, every array
    bit-identical to its state before the call outside, one optimizer step counted per call."""
    torch = torch_mod
    t, ref, g16 = crafted_trainer(torch, AC.CFG_SMALL_GRID, case)
    n, nm = t.n_params, t.n_network_params
    begin, end = nm - 37, nm + 131
    assert 0 < begin < nm < end < n and begin % 4 and end % 4
    inside = (np.arange(n) >= begin) & (np.arange(n) < end)
    for k in range(2):
        T = AC.CRAFT_GLOBAL_STEP + 1 + k
        g = np.roll(g16, 5 * k)
        set_gradients(torch, t, g)
        before = adam_arrays(t)
        t.optimizer_step_range(begin, end)
        assert t.optimizer_step_count == T
        full = {k_: v.copy() for k_, v in ref.items()}
        oracle_adam_step(AC.optimizer_block(case), nm, AC.loss_scale(case), T, full, g)
        for name in ref:
            ref[name][inside] = full[name][inside]
        got = adam_arrays(t)
        assert_adam_bits(got, dict(ref, g16=g), (case, k, "inside"), names=ALL, where=inside)
        assert_adam_bits(got, before, (case, k, "outside"), names=ALL, where=~inside)
        assert_adam_bits(got, ref, (case, k))


# ---------------------------------------------------------------------------------------------
# training steps against the oracle
# ---------------------------------------------------------------------------------------------
def opt_step(t, pos_d, tgt_d):
    t.training_step(pos_d, tgt_d, run_optimizer=True)


def train_and_compare(torch, t, case, n_steps, B, what, step=opt_step, opt_at=None):
    """n_steps training steps of t on the batches make_batch(B, step=s); after each, one oracle step on the
    GPU's fp16 gradients from the state before it must give the GPU's arrays. opt_at: {step: optimizer keys to
    change before it} (applied to both). Returns the oracle's state."""
    from tinycudann import _lib as L
    opt = AC.optimizer_block(case)
    first = adam_arrays(t)
    ref = fresh_adam_state(first["w32"])
    assert_adam_bits(first, ref, (what, "initial state"))
    pos_d, tgt_d = torch.empty(B, 2, device="cuda"), torch.empty(B, 3, device="cuda")  # fixed buffers (graph keys)
    for s in range(n_steps):
        if opt_at and s in opt_at:
            opt = dict(opt, **opt_at[s])
            L.check(L.lib().tcnn_trainer_update_hyperparams(t.h, json.dumps({"optimizer": opt_at[s]}).encode()))
        pos, tgt = make_batch(B, step=s)
        pos_d.copy_(torch.from_numpy(pos))
        tgt_d.copy_(torch.from_numpy(tgt))
        step(t, pos_d, tgt_d)
        got = adam_arrays(t)
        assert np.isfinite(O.h2f(got["g16"])).all(), (what, s)
        oracle_adam_step(opt, t.n_network_params, AC.loss_scale(case), s + 1, ref, got["g16"])
        assert t.optimizer_step_count == s + 1
        assert_adam_bits(got, ref, (what, case, s))
    return ref


@pytest.mark.parametrize("case", AC.CASE_NAMES)
def test_fused_step(torch_mod, case):
    """config_hash on the fused engine: the network parameters' Adam in the grid backward's spare workgroups,
    the grid's over the LDS levels' slabs; 4 steps. Then the weight image the epilogue wrote: inference on a fresh
    batch equals that of a new trainer given the same masters. For two cases training_step(False) +
    optimizer_step() (the standalone kernel) gives the same bits."""
    torch = torch_mod
    cfg, B, _ = AC.TRAINED["fused"]
    t = make_trainer(cfg, case)
    assert t.engine == "fused"
    ref = train_and_compare(torch, t, case, 4, B, "fused")
    pos, _ = make_batch(B, seed=9)
    pos_d = torch.from_numpy(pos).cuda()
    out = t.inference(pos_d)
    t2 = make_trainer(cfg, case)
    t2.set_params_full_precision(ref["w32"])
    assert np.array_equal(adam_arrays(t2)["w16"], ref["w16"])
    out2 = t2.inference(pos_d)
    assert torch.equal(out, out2), (case, float((out - out2).abs().max()))
    if case in ("combined", "freeze_matrix"):
        def two_calls(tr, p, q):
            tr.training_step(p, q, run_optimizer=False)
            tr.optimizer_step()
        t3 = make_trainer(cfg, case)
        ref3 = train_and_compare(torch, t3, case, 4, B, "fused, optimizer_step()", step=two_calls)
        assert_adam_bits(ref3, ref, (case, "two calls against the fused step"))


def test_binned_model_has_levels_on_both_passes(torch_mod):
    """The 2^16-entry table of test_binned_pass: a fused step with the optimizer writes the fp32 gradient sums of
    the levels it keeps in the LDS (their Adam kernel sums the slabs into gradients_fp32()) and leaves those of
    the binned levels alone (the accumulate pass applies Adam from its registers and writes only the fp16
    gradients), so a sentinel survives exactly on the binned levels: a suffix of whole levels, at least one level
    on either side. config_hash's own 2^15-entry table keeps every level in the LDS."""
    torch = torch_mod
    for cfg, want_binned in ((AC.CFG_BINNED, True), (CONFIG_HASH, False)):
        t = make_trainer(cfg, "default")
        assert t.engine == "fused"
        g = O.grid_cfg(cfg["encoding"], 2)
        F, nm = g.n_features_per_level, t.n_network_params
        sentinel = 12345.0
        t.gradients_fp32().fill_(sentinel)
        pos, tgt = make_batch(256)
        t.training_step(torch.from_numpy(pos).cuda(), torch.from_numpy(tgt).cuda(), run_optimizer=True)
        kept = t.gradients_fp32().cpu().numpy()[nm:] == sentinel
        level_kept = [bool(kept[g.offsets[l] * F:g.offsets[l + 1] * F].all()) for l in range(g.n_levels)]
        level_none = [not kept[g.offsets[l] * F:g.offsets[l + 1] * F].any() for l in range(g.n_levels)]
        assert all(a != b for a, b in zip(level_kept, level_none)), (level_kept, level_none)  # whole levels
        n_lds = level_kept.index(True) if True in level_kept else g.n_levels
        assert level_kept == [False] * n_lds + [True] * (g.n_levels - n_lds), level_kept  # the binned levels are a suffix
        if want_binned:
            assert 1 <= n_lds < g.n_levels, level_kept
            assert g.offsets[n_lds] - g.offsets[n_lds - 1] <= 1 << 15 < g.offsets[n_lds + 1] - g.offsets[n_lds]
        else:
            assert n_lds == g.n_levels


@pytest.mark.parametrize("case", AC.BINNED_CASES)
def test_binned_pass(torch_mod, case):
    """Adam in the binned accumulate pass (groups of 4 parameters; a group without an updated parameter writes
    nothing): 2 steps of 256 points on the 2^16-entry table, where most groups see no gradient."""
    torch = torch_mod
    cfg, B, _ = AC.TRAINED["binned"]
    t = make_trainer(cfg, case)
    assert t.engine == "fused"
    train_and_compare(torch, t, case, 2, B, "binned")
    g = O.grid_cfg(cfg["encoding"], 2)
    binned_from = next(l for l in range(g.n_levels) if g.offsets[l + 1] - g.offsets[l] > 1 << 15)
    g16 = adam_arrays(t)["g16"][t.n_network_params + g.offsets[binned_from] * g.n_features_per_level:]
    live = (O.h2f(g16).reshape(-1, 4) != 0).any(axis=1)
    assert 0.001 < live.mean() < 0.5, live.mean()  # groups with and (mostly) without a gradient


@pytest.mark.parametrize("case", AC.SEQUENTIAL_CASES)
@pytest.mark.parametrize("engine", ["tile", "layered"])
def test_sequential_engines(torch_mod, engine, case):
    """The tile engine (HashGrid + W128/H2) and the layer-wise engine (OneBlob + CutlassMLP W64/H2): the step
    ends in the standalone kernel over the whole vector."""
    cfg, B, _ = AC.TRAINED[engine]
    t = make_trainer(cfg, case)
    assert t.engine == ("fused" if engine == "tile" else "layered")
    train_and_compare(torch_mod, t, case, 3, B, engine)


# ---------------------------------------------------------------------------------------------
# (f) graph replay
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["fused", "tile"])
def test_graph_replay(torch_mod, model):
    """The step replayed as a graph, against the oracle after every step: 6 steps of `combined`; before the
    fourth, beta1, beta2 and the clip change (the bias-correction table is rebuilt, the step captured again)."""
    cfg, B, _ = AC.TRAINED[model]
    t = make_trainer(cfg, "combined")
    t.set_graph(True)
    change = {3: {"beta1": 0.7, "beta2": 0.9, "clipping_magnitude": 0.04}}
    train_and_compare(torch_mod, t, "combined", 6, B, ("graph", model), opt_at=change)
    captures, replays = t.graph_stats()
    assert captures >= 2 and replays >= 2, (captures, replays)


@pytest.mark.parametrize("model", ["fused", "tile"])
def test_graph_adabound_runs_eagerly(torch_mod, model):
    """AdaBound's bounds move with the optimizer's step, so its steps are never replayed -- and match the oracle."""
    cfg, B, _ = AC.TRAINED[model]
    t = make_trainer(cfg, "adabound_upper")
    t.set_graph(True)
    train_and_compare(torch_mod, t, "adabound_upper", 4, B, ("graph", model))
    assert t.graph_stats()[1] == 0, t.graph_stats()
