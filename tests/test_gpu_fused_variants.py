"""The register-resident fused training kernel (k_fused_train_grid, k_fused_train_grid_loss) and the fused forward
(k_fused_fwd_grid) against the CPU oracle on what no other Trainer test runs: 3-D grids, the Prime and ReversedPrime
hashes, Dense and Tiled grids (hash_grid = 0), Smoothstep and Nearest, each of the kernel's gather paths at D = 3 (the
per-level pair gather, the general index for out-of-range waves and for inrange_index = 0), the four fused shapes x
hidden None / ReLU at D = 3, and the D = 3 step as a whole (the fused kernel's dL/d(encoding) into the 3-D grid
backward with the network's column sums and Adam in its spare workgroups, lean grid Adam afterwards).

Cases, inputs and the CPU proof that these assertions can fail: tests/fused_variant_cases.py and
tests/test_fused_variants_reference.py. Tolerances are the project's: loss and gradient vectors 1e-3 relative
(test_gpu_parity.py), per element helpers.trainer_grad_bounds, outputs 4 fp16 ulps of the output scale
(helpers.assert_within_fp16_ulps), Adam and the halves bit for bit.

TCNN_VARIANT_RATIOS=<file>: every test appends its measured figures (profiles/fused_variants_ratios.txt is that
file behind fused_variant_cases.RATIOS_HEADER)."""
import copy
import functools
import json
import os

import numpy as np
import pytest

import fused_variant_cases as C
import loss_reference as R
import test_gpu_losses as TL
from helpers import (adam_arrays, assert_adam_bits, assert_trainer_grads_per_element, assert_within_fp16_ulps, fresh_adam_state,
                     oracle_adam_step, rel_err, trainer_arrays, trainer_grad_bounds)
from oracle import oracle as O

pytestmark = pytest.mark.gpu

INFER_IDS = [c.id for c in C.INFERENCE_CASES]
STEP_IDS = [c.id for c in C.ALL_CASES]
OTHER_LOSSES = [o for o in R.LOSSES if o not in ("RelativeL2", "L2")]
LOSS_SCALE = 128.0


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


def _record(case_id, kind, **figures):
    line = f"{case_id} [{kind}] " + " ".join(f"{k}={v:.3g}" for k, v in figures.items())
    print(line)
    path = os.environ.get("TCNN_VARIANT_RATIOS")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


@functools.lru_cache(maxsize=None)
def _register_kernel(case_id):
    """the kernel family the network's backward without dL/dinput runs (NetworkHost::fused_ok decides both this and
    the Trainer's engine, whose name "fused" also covers the tile kernel)"""
    from tinycudann import _lib as L
    case, lib = C.BY_ID[case_id], L.lib()
    m = L.check_ptr(lib.tcnn_create_network_with_input_encoding(case.D, C.N_OUT, json.dumps(case.enc).encode(),
                                                                 json.dumps(case.cfg["network"]).encode()))
    try:
        return lib.tcnn_module_backward_kernel(m, 0).decode()
    finally:
        lib.tcnn_module_destroy(m)


def _trainer(case, from_trainer=True):
    """a Trainer of the case on the fused engine at the test parameters. from_trainer: the parameters are made from
    the trainer's own initial ones (and must be the CPU file's); else set without reading a trainer buffer (the
    getters switch lean Adam off)"""
    from tinycudann import Trainer
    t = Trainer(case.D, C.N_OUT, case.cfg, seed=C.SEED)
    assert t.engine == "fused" and t.inference_engine == "fused", (case.id, t.engine, t.inference_engine)
    assert _register_kernel(case.id) == "register", case.id
    w = C.cpu_params(case.id)
    if from_trainer:
        w_own = C.test_params(case, trainer_arrays(t)["w32"])
        np.testing.assert_array_equal(w_own.view(np.uint32), w.view(np.uint32))  # what the CPU file proved sound
    t.set_params_full_precision(w)
    return t, w


def _pair(case):
    """one Trainer and one OracleModel at the same parameters (w16 bit-equal, asserted)"""
    t, w = _trainer(case)
    om = C.oracle_model(case, w)
    np.testing.assert_array_equal(trainer_arrays(t)["w16"], om.w16)
    return t, om, w


def _gpu_step(torch, t, pos, tgt):
    t.training_step(torch.from_numpy(pos).cuda(), torch.from_numpy(tgt).cuda(), run_optimizer=False)
    return t.loss(), trainer_arrays(t)["g32"]


def _assert_step(case, torch, t, om, pos, tgt, n_threads=4):
    """loss and the two gradient vectors of one step without the optimizer against the oracle's; returns the figures"""
    loss_gpu, g32 = _gpu_step(torch, t, pos, tgt)
    loss_ref = om.train_step(pos, tgt, run_optimizer=False, n_threads=n_threads)
    nm = case.n_mlp
    fig = dict(loss_rel=abs(loss_gpu - loss_ref) / abs(loss_ref), mlp_rel=rel_err(g32[:nm], om.grad32[:nm]),
               grid_rel=rel_err(g32[nm:], om.grad32[nm:]))
    print(case.id, fig)
    assert np.isfinite(g32).all()
    assert fig["loss_rel"] <= 1e-3, (loss_gpu, loss_ref)
    assert fig["mlp_rel"] <= 1e-3, fig
    assert fig["grid_rel"] <= 1e-3, fig
    return fig, g32


# ---------------------------------------------------------------------------------------------
# a: one step against the oracle
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_id", STEP_IDS)
def test_one_step_matches_oracle(torch_mod, case_id):
    case = C.BY_ID[case_id]
    t, om, w = _pair(case)
    (pos_all, tgt_all), (pos, tgt), _ = C.batches(case, w)
    fig, _ = _assert_step(case, torch_mod, t, om, pos_all, tgt_all)  # every sample, safe or not
    if case.loss != "RelativeL2":  # helpers.trainer_grad_bounds is RelativeL2's
        _record(case_id, "step", **fig)
        return
    fig, g32 = _assert_step(case, torch_mod, t, om, pos, tgt)  # the samples clear of the branches: per element too
    mag, gb = trainer_grad_bounds(case.cfg, trainer_arrays(t)["w16"], pos, tgt)
    fig["pe_mlp"], fig["pe_grid"] = assert_trainer_grads_per_element(g32, om.grad32, case.n_mlp, mag, gb)
    _record(case_id, "step", **fig)


# ---------------------------------------------------------------------------------------------
# b: in-range, edge and out-of-range waves in one batch
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_id", C.MIXED_RANGE_CASES)
def test_mixed_in_range_and_out_of_range_waves(torch_mod, case_id):
    case = C.BY_ID[case_id]
    t, om, _ = _pair(case)
    pos, tgt = C.mixed_range_batch(case)
    fig, _ = _assert_step(case, torch_mod, t, om, pos, tgt)
    _record(case_id, "mixed-range", **fig)


# ---------------------------------------------------------------------------------------------
# c: more than one sweep of the persistent grid
# ---------------------------------------------------------------------------------------------
def test_second_sweep_of_the_persistent_grid(torch_mod):
    case = C.BY_ID[C.SWEEP_CASE]
    n_cu = torch_mod.cuda.get_device_properties(0).multi_processor_count
    n = 256 * n_cu + 256  # 2 n_cu workgroups x 4 slices, then two workgroups take a second one (the batch granularity is 256)
    t, om, _ = _pair(case)
    pos, tgt = C.pool(case, n, seed=3)
    fig, _ = _assert_step(case, torch_mod, t, om, pos, tgt, n_threads=8)
    _record(case.id, f"sweep-B{n}", **fig)


# ---------------------------------------------------------------------------------------------
# d: three optimizer steps
# ---------------------------------------------------------------------------------------------
def _step_batches(case, n_steps):
    return [C.pool(case, C.B, seed=20 + s) for s in range(n_steps)]


@pytest.mark.parametrize("case_id", C.ADAM_CASES)
def test_adam_steps_match_oracle_on_same_gradients(torch_mod, case_id):
    """as test_gpu_parity.py::test_adam_step_matches_oracle_on_same_gradients, on a 3-D table: the oracle's Adam on the
    GPU's own fp16 gradients (the network's in the 3-D grid backward's spare workgroups, the grid's in k_adam; the first
    step lean, the later ones eager since the getters were called)"""
    torch = torch_mod
    case = C.BY_ID[case_id]
    t, w = _trainer(case, from_trainer=False)
    state = fresh_adam_state(w)
    for s, (pos, tgt) in enumerate(_step_batches(case, 3)):
        t.training_step(torch.from_numpy(pos).cuda(), torch.from_numpy(tgt).cuda(), run_optimizer=True)
        got = adam_arrays(t)
        assert np.any(got["g16"][:case.n_mlp]) and np.any(got["g16"][case.n_mlp:]), s
        oracle_adam_step(case.cfg["optimizer"], case.n_mlp, LOSS_SCALE, s + 1, state, got["g16"])
        assert_adam_bits(got, state, (case_id, s))
    assert np.any(state["w16"] != O.f2h(w))  # the parameters moved


@pytest.mark.parametrize("case_id", C.ADAM_CASES)
def test_one_call_step_bit_identical_to_gradient_pass_and_optimizer_step(torch_mod, case_id):
    """as test_gpu_parity.py::test_overlapped_step_bit_identical_to_sequential: no getter before the end, so every
    one-call step runs lean grid Adam"""
    torch = torch_mod
    case = C.BY_ID[case_id]
    (ta, w), (tb, _) = _trainer(case, from_trainer=False), _trainer(case, from_trainer=False)
    for pos, tgt in _step_batches(case, 3):
        p, g = torch.from_numpy(pos).cuda(), torch.from_numpy(tgt).cuda()
        ta.training_step(p, g, run_optimizer=True)
        tb.training_step(p, g, run_optimizer=False)
        tb.optimizer_step()
        assert abs(ta.loss() - tb.loss()) <= 1e-6 * abs(tb.loss())
    a, b = adam_arrays(ta), adam_arrays(tb)
    assert_adam_bits(a, b, case_id, names=("w32", "w16", "m1", "m2", "steps", "g16"))
    assert np.any(a["w16"] != O.f2h(w))


# ---------------------------------------------------------------------------------------------
# e: inference through k_fused_fwd_grid
# ---------------------------------------------------------------------------------------------
def _assert_inference(torch, case, t, om, pos, kind):
    out = t.inference(torch.from_numpy(pos).cuda()).cpu().numpy()
    ref = O.h2f(om.inference(pos, n_threads=4))[:, :C.N_OUT]
    assert out.shape == ref.shape and np.abs(ref).max() > 0.5
    _record(case.id, kind, ulps=assert_within_fp16_ulps(out, ref))


@pytest.mark.parametrize("case_id", INFER_IDS)
def test_inference_matches_oracle(torch_mod, case_id):
    case = C.BY_ID[case_id]
    t, om, _ = _pair(case)
    pos, _ = C.pool(case, C.B_INFER, seed=5)
    _assert_inference(torch_mod, case, t, om, pos, "infer")
    if case_id == "d3-dense":
        pos[130] = [1.25, 0.5, -0.125]
        pos[287] = [-0.5, 1.5, 0.75]
        _assert_inference(torch_mod, case, t, om, pos, "infer-out-of-range")


# ---------------------------------------------------------------------------------------------
# f: the other seven losses at D = 3 (k_fused_train_grid_loss<.., 3, ..>), with test_gpu_losses.py's helpers
# ---------------------------------------------------------------------------------------------
def _loss_case(otype):
    """the W32/H1 shape case under test_gpu_losses.py's helpers (CrossEntropy and Variance at a learning rate of 1e-4:
    test_gpu_losses._slow)"""
    slow = otype in ("CrossEntropy", "Variance")
    name = "variants_d3_w32h1" + ("_slow" if slow else "")
    if name not in TL.OTHER_CASES:
        cfg = copy.deepcopy(C.BY_ID[C.LOSS_SHAPE].cfg)
        TL.OTHER_CASES[name] = (TL._slow(cfg) if slow else cfg, "fused")
    return name


@pytest.mark.parametrize("otype", OTHER_LOSSES)
def test_other_losses_forward_matches_restatement(torch_mod, otype):
    name = _loss_case(otype)
    assert _register_kernel(C.LOSS_SHAPE) == "register"
    t = TL._trainer(name, C.N_OUT, otype, n_dims=3)
    x, y = TL._batch(torch_mod, name, C.N_OUT, C.B, n_dims=3)
    TL._check_context(otype, t.forward(x, y), y.cpu().numpy(), C.B, C.N_OUT, (name, otype))


@pytest.mark.parametrize("otype", OTHER_LOSSES)
def test_other_losses_halves_reproduce_training_step(torch_mod, otype):
    """as test_gpu_losses.py::test_halves_reproduce_training_step, over two steps"""
    name = _loss_case(otype)
    a, b = TL._trainer(name, C.N_OUT, otype, n_dims=3), TL._trainer(name, C.N_OUT, otype, n_dims=3)
    w0 = O.f2h(TL._setup(name, C.N_OUT, 3)[0])  # (no getter on a or b before the steps: they switch lean Adam off)
    for s in range(2):
        x, y = TL._batch(torch_mod, name, C.N_OUT, C.B, s, n_dims=3)
        a.training_step(x, y)
        ctx = b.forward(x, y)
        b.backward(ctx, x)
        b.optimizer_step()
        la, lb = a.loss(), ctx.loss()
        assert np.isfinite(la) and abs(la - lb) <= 1e-6 * abs(la), (otype, s, la, lb)
    ra, rb = trainer_arrays(a), trainer_arrays(b)
    np.testing.assert_array_equal(ra["w16"], rb["w16"])
    np.testing.assert_array_equal(ra["w32"], rb["w32"])
    assert np.isfinite(ra["w32"]).all() and np.any(ra["w16"] != w0)
