"""GPU tests of the reference's nine losses (src/loss.cu:57-65) on the three training engines, against
the numpy restatement tests/loss_reference.py (pinned on the CPU by tests/test_loss_reference.py).

  1. the stand-alone kernel (tcnn_loss_evaluate) against the restatement: gradients bit-equal for the
     six losses without an FMA, within 1 fp16 ulp and at most 1 element in 10^4 different for the three
     with one (the restatement's fmaf is float64 arithmetic rounded twice); values within 2 fp32 ulps
     (1e-6 relative for CrossEntropy's logf); padded columns zero; with and without data_pdf
  2. forward() on every engine: dL_doutput and loss() are the restatement of the context's own output
  3. the loss inside the fused and tile kernels: forward + backward + optimizer_step reproduce
     training_step bit for bit (the halves evaluate the loss in the stand-alone kernel of 1 and 2)
  4. interfaces: otypes in any letter case, hyperparams, refusals, negative losses, snapshots, C++
  5. L1 and Smape train

Inputs. The seed-1337 initialisation gives outputs of about 1e-5: useless for CrossEntropy / Variance
(log and 1 / p of a prediction that may be <= 0) and fragile for the sign losses. The tests start from the
trainer's initial fp32 parameters, multiply the encoding's part by 1e4 and replace the 16 x W output
matrix by its absolute values; the predictions are then positive (asserted, computed with the CPU
oracle). Samples are drawn clear of the ReLU boundaries (helpers.relu_safe_grid_batch, grid encodings)
and samples with any |p - t| < 8 * 2^-10 are dropped (a sign loss flips there on one fp16 ulp of p).
"""
import copy
import ctypes
import functools
import json
import os
import subprocess

import numpy as np
import pytest

import loss_reference as R
from helpers import CONFIG_HASH, make_batch, relu_safe_grid_batch, rgb_field, trainer_arrays
from oracle import oracle as O

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOSS_SCALE = 128.0  # the trainer's default
FMA_ULPS, FMA_SHARE = 1, 1e-4


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


# ---------------------------------------------------------------------------------------------
# networks and inputs
# ---------------------------------------------------------------------------------------------
def _net(base, **kw):
    cfg = copy.deepcopy(base)
    cfg["network"] = dict(cfg["network"], **kw)
    return cfg


def _slow(cfg):
    """learning rate 1e-4: behind an Exponential output CrossEntropy and Variance fall without bound as the prediction
    grows, and at 1e-2 the third step's predictions overflow fp16"""
    cfg["optimizer"] = dict(cfg["optimizer"], learning_rate=1e-4)
    return cfg


# name -> (config, engine). The tile kernels hold the 16 outputs in one of two register layouts
# (mlp_tile.h: OP = !(W >= 128 && NH >= 4)): W64 / 4 layers has OP, W128 / 4 layers has not.
CASES = {
    "fused_w64": (_net(CONFIG_HASH), "fused"),                                        # register-resident fused kernel
    "fused_w32h1": (_net(CONFIG_HASH, n_neurons=32, n_hidden_layers=1), "fused"),
    "tile_op": (_net(CONFIG_HASH, n_neurons=64, n_hidden_layers=4), "fused"),         # tile kernel (not a fused shape), OP layout
    "tile_exp": (_slow(_net(CONFIG_HASH, n_neurons=128, n_hidden_layers=4, output_activation="Exponential")), "fused"),  # tile, !OP
    "layered": (_net(CONFIG_HASH, otype="CutlassMLP"), "layered"),
}
# name -> (config, engine) of other test modules that use the helpers below (tests/test_gpu_fused_variants.py: a 3-D
# grid); not part of this module's parametrisations
OTHER_CASES = {}


def _case(case):
    return CASES[case] if case in CASES else OTHER_CASES[case]


def _with_loss(cfg, otype):
    cfg = copy.deepcopy(cfg)
    cfg["loss"] = {"otype": otype}
    return cfg


def scaled_params(cfg, w32, n_mlp):
    """the test parameters from a trainer's initial ones: encoding x 1e4, |output matrix|"""
    w = np.array(w32, np.float32)
    W = cfg["network"]["n_neurons"]
    w[n_mlp:] *= np.float32(1e4)
    w[n_mlp - 16 * W:n_mlp] = np.abs(w[n_mlp - 16 * W:n_mlp])
    return w


def targets_for(pos, dims):
    rgb = rgb_field(pos)
    return np.ascontiguousarray(np.tile(rgb, (1, (dims + 2) // 3))[:, :dims])


def select_samples(cfg, w32, dims, n_want, n_dims=2):
    """n_want (positions [n_want, n_dims], targets) for the network of cfg at fp32 parameters w32: positive oracle predictions
    (asserted), clear of the ReLU boundaries (grid encodings) and of |p - t| < 8 * 2^-10 (at most 10 % dropped, asserted)"""
    w16 = O.f2h(w32)
    if cfg["encoding"]["otype"].lower() == "hashgrid":
        pos, _ = relu_safe_grid_batch(cfg, w16, 2 * n_want, n_dims=n_dims)
    else:
        pos, _ = make_batch(2 * n_want, n_dims=n_dims)
    tgt = targets_for(pos, dims)
    om = O.OracleModel({k: v for k, v in cfg.items() if k != "loss"}, n_dims, dims)
    om.w32[:] = w32
    om.w16[:] = w16
    pred = O.h2f(om.inference(pos, n_threads=4))[:, :dims]
    assert pred.min() > 0, float(pred.min())
    keep = np.all(np.abs(pred - tgt) >= 8 * 2.0 ** -10, axis=1)
    assert (~keep).mean() <= 0.10, float((~keep).mean())
    assert keep.sum() >= n_want
    idx = np.nonzero(keep)[0][:n_want]
    return np.ascontiguousarray(pos[idx]), np.ascontiguousarray(tgt[idx])


def _setup(case, dims, n_dims=2):
    """(test parameters fp32, positions [1024, n_dims], targets [1024, dims]) of a case, computed once"""
    return _setup_once(case, dims, n_dims)


@functools.lru_cache(maxsize=None)
def _setup_once(case, dims, n_dims):
    from tinycudann import Trainer
    cfg, _ = _case(case)
    t = Trainer(n_dims, dims, cfg, seed=1337)
    w = scaled_params(cfg, trainer_arrays(t)["w32"], t.n_network_params)
    pos, tgt = select_samples(cfg, w, dims, 1024, n_dims)
    for a in (w, pos, tgt):
        a.setflags(write=False)
    return w, pos, tgt


def _trainer(case, dims, otype, n_dims=2):
    from tinycudann import Trainer
    cfg, engine = _case(case)
    t = Trainer(n_dims, dims, _with_loss(cfg, otype), seed=1337)
    assert t.engine == engine, (case, t.engine)
    t.set_params_full_precision(_setup(case, dims, n_dims)[0])
    return t


def _batch(torch, case, dims, B, step=0, n_dims=2):
    _, pos, tgt = _setup(case, dims, n_dims)
    s = slice(step * B % 1024, step * B % 1024 + B)
    return torch.from_numpy(pos[s].copy()).cuda(), torch.from_numpy(tgt[s].copy()).cuda()


def _assert_grads(otype, got16, ref16, what):
    got16, ref16 = np.asarray(got16, np.uint16), np.asarray(ref16, np.uint16)
    bad = got16 != ref16
    if R.canonical(otype) not in R.FMA_LOSSES:
        assert not bad.any(), (what, otype, int(bad.sum()), got16[bad][:4], ref16[bad][:4])
        return
    assert bad.mean() <= FMA_SHARE, (what, otype, float(bad.mean()))
    if bad.any():
        assert R.ulp_diff16(got16[bad], ref16[bad]).max() <= FMA_ULPS, (what, otype)


# ---------------------------------------------------------------------------------------------
# 1: the stand-alone kernel against the restatement
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _kernel_inputs(n, dims):
    rng = np.random.default_rng(1000 * n + dims)
    pred16 = O.f2h(rng.uniform(0.2, 2.0, size=(n, 16)).astype(np.float32))  # padded columns too: the luminance reads them
    tgt = rng.uniform(0.05, 1.5, size=(n, dims)).astype(np.float32)
    tgt[::7] = O.h2f(pred16)[::7, :dims]  # differences of exactly 0: copysignf gives +scale
    pdf = rng.uniform(0.25, 4.0, size=(n, dims)).astype(np.float32)
    return pred16, tgt, pdf


def _loss_evaluate(torch, otype, pred16, tgt, pdf, want_values=True):
    from tinycudann import _lib as L
    n, stride = pred16.shape
    dims = tgt.shape[1]
    p = torch.from_numpy(pred16.view(np.float16)).cuda()
    t = torch.from_numpy(tgt).cuda()
    q = torch.from_numpy(pdf).cuda() if pdf is not None else None
    vals = torch.full((n, stride), float("nan"), device="cuda") if want_values else None
    grads = torch.full((n, stride), float("nan"), dtype=torch.float16, device="cuda")
    ptr = lambda x: ctypes.c_void_p(x.data_ptr() if x is not None else 0)
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    L.check(L.lib().tcnn_loss_evaluate(otype.encode(), s, n, stride, dims, LOSS_SCALE, ptr(p), ptr(t), ptr(vals), ptr(grads), ptr(q)))
    torch.cuda.synchronize()
    return (vals.cpu().numpy() if want_values else None), grads.cpu().numpy().view(np.uint16)


# RelativeL2 first: the kernel that existed before the other losses, expected bit-equal to oracle.relative_l2
@pytest.mark.parametrize("otype", ("RelativeL2",) + tuple(o for o in R.LOSSES if o != "RelativeL2"))
def test_standalone_kernel_matches_restatement(torch_mod, otype):
    for n in (256, 768):  # 768: more than one workgroup's worth of a grid-stride sum
        for dims in (1, 3, 4, 6, 16):
            for with_pdf in (False, True):
                pred16, tgt, pdf = _kernel_inputs(n, dims)
                pdf = pdf if with_pdf else None
                what = (n, dims, with_pdf)
                vals, grads = _loss_evaluate(torch_mod, otype, pred16, tgt, pdf)
                v_ref, g_ref = R.evaluate(otype, pred16, tgt, LOSS_SCALE, pdf)
                if otype == "RelativeL2" and not with_pdf:
                    _, g_orc, _ = O.relative_l2(pred16, tgt, loss_scale=LOSS_SCALE)
                    np.testing.assert_array_equal(grads[:, :dims], g_orc[:, :dims])
                _assert_grads(otype, grads, g_ref, what)
                assert not grads[:, dims:].any() and not vals[:, dims:].any(), what
                assert np.isfinite(vals).all(), what
                if otype == "CrossEntropy":
                    np.testing.assert_allclose(vals, v_ref, rtol=1e-6, atol=0, err_msg=str(what))
                else:
                    assert R.ulp_diff32(vals, v_ref).max() <= 2, (what, int(R.ulp_diff32(vals, v_ref).max()))
                # without a values buffer: the same gradients
                _, g2 = _loss_evaluate(torch_mod, otype, pred16, tgt, pdf, want_values=False)
                np.testing.assert_array_equal(g2, grads)


def test_loss_evaluate_refuses_unknown_otypes(torch_mod):
    from tinycudann import _lib as L
    pred16, tgt, _ = _kernel_inputs(256, 3)
    for bad in ("Huber", ""):
        with pytest.raises(L.TcnnError, match="RelativeL2Luminance.*Variance"):
            _loss_evaluate(torch_mod, bad, pred16, tgt, None)


# ---------------------------------------------------------------------------------------------
# 2: forward() on every engine
# ---------------------------------------------------------------------------------------------
LOSS_DIMS = [(o, 3) for o in R.LOSSES] + [("RelativeL2Luminance", 4), ("RelativeL2Luminance", 6)]


def _check_context(otype, ctx, tgt, B, dims, what):
    out16 = ctx.output.cpu().numpy().view(np.uint16).reshape(B, 16)
    d16 = ctx.dL_doutput.cpu().numpy().view(np.uint16).reshape(B, 16)
    v_ref, g_ref = R.evaluate(otype, out16, tgt, LOSS_SCALE)
    assert O.h2f(out16)[:, :dims].min() > 0, what
    _assert_grads(otype, d16, g_ref, what)
    assert not d16[:, dims:].any()
    v64 = v_ref.astype(np.float64)
    # the summed loss: fp32 partial sums of values within 2 ulps of v_ref
    assert abs(ctx.loss() - v64.sum()) <= B * 2.0 ** -24 * np.abs(v64).sum(), (what, ctx.loss(), v64.sum())


@pytest.mark.parametrize("otype,dims", LOSS_DIMS)
@pytest.mark.parametrize("case", list(CASES))
def test_forward_matches_restatement(torch_mod, case, otype, dims):
    B = 256
    t = _trainer(case, dims, otype)
    x, y = _batch(torch_mod, case, dims, B)
    ctx = t.forward(x, y)
    _check_context(otype, ctx, y.cpu().numpy(), B, dims, (case, otype, dims))


def test_forward_loss_sum_over_several_workgroups(torch_mod):
    B = 768
    for otype in ("L1", "CrossEntropy"):
        t = _trainer("fused_w64", 3, otype)
        x, y = _batch(torch_mod, "fused_w64", 3, B)
        _check_context(otype, t.forward(x, y), y.cpu().numpy(), B, 3, otype)


# ---------------------------------------------------------------------------------------------
# 3: the loss inside the fused and tile kernels
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("otype,dims", LOSS_DIMS)
@pytest.mark.parametrize("case", list(CASES))
def test_halves_reproduce_training_step(torch_mod, case, otype, dims):
    for B in (256, 512):
        a, b = _trainer(case, dims, otype), _trainer(case, dims, otype)
        for s in range(3):
            x, y = _batch(torch_mod, case, dims, B, s)
            a.training_step(x, y)
            ctx = b.forward(x, y)
            b.backward(ctx, x)
            b.optimizer_step()
            la, lb = a.loss(), ctx.loss()
            assert np.isfinite(la) and abs(la - lb) <= 1e-6 * abs(la), (case, otype, B, s, la, lb)
        ra, rb = trainer_arrays(a), trainer_arrays(b)
        np.testing.assert_array_equal(ra["w16"], rb["w16"])
        np.testing.assert_array_equal(ra["w32"], rb["w32"])
        assert np.isfinite(ra["w32"]).all()


# ---------------------------------------------------------------------------------------------
# 4: interfaces
# ---------------------------------------------------------------------------------------------
def test_otypes_construct_in_any_case_and_round_trip(torch_mod):
    from tinycudann import Trainer, _lib as L
    for otype in R.LOSSES:
        for spelled in (otype, otype.lower(), otype.upper()):
            t = Trainer(2, 3, _with_loss(CONFIG_HASH, spelled), seed=1337)
            hp = json.loads(L.lib().tcnn_trainer_hyperparams(t.h).decode())
            assert hp["loss"]["otype"] == spelled
            assert R.canonical(hp["loss"]["otype"]) == otype
        # the type is fixed at construction
        with pytest.raises(L.TcnnError):
            other = "L2" if otype != "L2" else "L1"
            L.check(L.lib().tcnn_trainer_update_hyperparams(t.h, json.dumps({"loss": {"otype": other}}).encode()))
        L.check(L.lib().tcnn_trainer_update_hyperparams(t.h, json.dumps({"loss": {"otype": otype}}).encode()))


@pytest.mark.parametrize("bad", ["Huber", ""])
def test_other_otypes_are_refused_with_the_list(bad):
    from tinycudann import Trainer, _lib as L
    with pytest.raises(L.TcnnError) as e:
        Trainer(2, 3, _with_loss(CONFIG_HASH, bad), seed=1337)
    for o in R.LOSSES:
        assert o in str(e.value), (o, str(e.value))


def test_negative_loss_is_returned_not_raised(torch_mod):
    torch = torch_mod
    t = _trainer("fused_w64", 3, "CrossEntropy")
    w = np.array(_setup("fused_w64", 3)[0])
    n_mlp = t.n_network_params
    w[n_mlp - 16 * 64:n_mlp] *= 8  # predictions 8 x larger: above 1
    t.set_params_full_precision(w)
    x, y = _batch(torch, "fused_w64", 3, 256)
    ctx = t.forward(x, y)
    assert float(ctx.output.float().reshape(256, 16)[:, :3].min()) > 1
    assert ctx.loss() < 0
    t.training_step(x, y, run_optimizer=False)
    assert t.loss() < 0
    assert t.loss() == pytest.approx(ctx.loss(), rel=1e-6)


def test_snapshot_round_trip_keeps_l1_training_bit_identical(torch_mod):
    """as tests/test_gpu_snapshot.py asserts for RelativeL2: the loaded trainer has the saved fp16 parameters and step
    count, and its next step computes the same loss and gradients, bit for bit (the fp32 masters become (float)half
    on load, as in the reference, so the parameters after that step may differ in the last fp16 place)"""
    torch = torch_mod
    a = _trainer("fused_w64", 3, "L1")
    for s in range(2):
        a.training_step(*_batch(torch, "fused_w64", 3, 256, s))
    b = _trainer("fused_w64", 3, "L1")
    b.deserialize(a.serialize(optimizer=True))
    np.testing.assert_array_equal(trainer_arrays(a)["w16"], trainer_arrays(b)["w16"])
    assert a.optimizer_step_count == b.optimizer_step_count == 2
    x, y = _batch(torch, "fused_w64", 3, 256, 2)
    a.training_step(x, y)
    b.training_step(x, y)
    assert a.loss() == b.loss()
    np.testing.assert_array_equal(trainer_arrays(a)["g32"], trainer_arrays(b)["g32"])


def test_cpp_loss_api_consumer():
    """tests/cpp/loss_api_consumer.cpp (built by the Makefile): create_loss for the nine, Loss::evaluate against
    Trainer::forward's dL_doutput, create_from_config with Smape"""
    exe = os.path.join(REPO, "neuralbtf-tiny-cuda-nn_amd", "bin", "loss_api_consumer")
    assert os.path.exists(exe), "build it with make -C neuralbtf-tiny-cuda-nn_amd"
    r = subprocess.run([exe, os.path.join(REPO, "tests", "golden", "config_hash.json")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "loss api ok" in r.stdout, r.stdout


# ---------------------------------------------------------------------------------------------
# 5: it trains
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("otype", ["L1", "Smape"])
def test_it_trains(torch_mod, otype):
    torch = torch_mod
    from tinycudann import Trainer
    t = Trainer(2, 3, _with_loss(CONFIG_HASH, otype), seed=1337)
    assert t.engine == "fused"
    losses = []
    for s in range(60):
        pos, tgt = make_batch(4096, step=s)
        t.training_step(torch.from_numpy(pos).cuda(), torch.from_numpy(tgt).cuda())
        losses.append(t.loss())
    assert np.isfinite(losses).all()
    assert np.mean(losses[-10:]) < np.mean(losses[:10]), (losses[:10], losses[-10:])
