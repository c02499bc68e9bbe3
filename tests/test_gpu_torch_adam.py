"""tinycudann.optim.Adam on the GPU, bit for bit against the oracle's Adam (O.adam_step, itself checked against
float64 in tests/test_adam_reference.py), called as tests/test_gpu_adam_options.py calls it.

  5. every optimizer block of tests/adam_cases.py on the crafted state (n = 4099, class boundary at 2050: inside a
     thread's 8 parameters; signed-zero, largest and subnormal gradients, fresh parameters), three steps, with fp32
     gradients float32(h2f(g16)) / loss_scale -- the oracle's own (float)g16 / loss_scale -- and with fp16 gradients
     against the oracle at loss scale 1: masters, both moments and the per-element step counts
  6. the optimizer's behaviour: groups, missing gradients, lr written between steps, state_dict round trip, refusals,
     param_groups
  7. one training step of config_btf's model with tinycudann.Loss, and 30 steps that reduce the loss
"""
import copy
import json
import os

import numpy as np
import pytest

import adam_cases as AC
import loss_reference as R
from helpers import CONFIG_HASH, assert_adam_bits, oracle_adam_step
from oracle import oracle as O

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CONFIG_BTF = json.load(open(os.path.join(GOLD, "config_btf.json")))
NAMES = ("w32", "m1", "m2", "steps")


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(params=[False, True], ids=["cpp_ext", "ctypes"])
def path(request, monkeypatch):
    """the C++ extension's plain function and the ctypes fallback, selected as the autograd nodes are"""
    from tinycudann import modules
    if request.param:
        monkeypatch.setattr(modules, "_EXT", None)
    elif modules._EXT is None:
        pytest.fail("the C++ extension (lib/_tcnn_torch) is not built")
    return "ctypes" if request.param else "cpp"


def options(case):
    opt = AC.optimizer_block(case)
    return {k: v for k, v in opt.items() if k != "otype"}


def crafted(torch, block, n_matrix=AC.CRAFT_N_MATRIX, seed=20, n=AC.CRAFT_N):
    """(parameter, optimizer holding the crafted state, the same state on the host, the crafted fp16 gradients)"""
    import tinycudann as tcnn
    ref = AC.crafted_state(n, seed)
    g16 = ref.pop("g16")
    ref["w16"] = O.f2h(ref["w32"])
    p = torch.nn.Parameter(torch.from_numpy(ref["w32"].copy()).cuda())
    opt = tcnn.optim.Adam([dict(block, params=[p], n_matrix=n_matrix)])
    load(torch, opt, p, ref)
    return p, opt, ref, g16


def load(torch, opt, p, ref, step=AC.CRAFT_GLOBAL_STEP):
    opt.state[p] = {"step": step, "exp_avg": torch.from_numpy(ref["m1"].copy()).cuda(),
                    "exp_avg_sq": torch.from_numpy(ref["m2"].copy()).cuda(),
                    "param_steps": torch.from_numpy(ref["steps"].view(np.int32).copy()).cuda()}


def arrays(opt, p):
    s = opt.state[p]
    return {"w32": p.detach().cpu().numpy(), "m1": s["exp_avg"].cpu().numpy(), "m2": s["exp_avg_sq"].cpu().numpy(),
            "steps": s["param_steps"].cpu().numpy().view(np.uint32)}


def grad32(torch, g16, loss_scale):
    g = O.h2f(g16) / np.float32(loss_scale)
    assert g.dtype == np.float32
    return torch.from_numpy(g).cuda()


def grad16(torch, g16):
    return torch.from_numpy(np.ascontiguousarray(g16).view(np.float16).copy()).cuda()


# ---------------------------------------------------------------------------------------------
# 5: bit for bit against the oracle
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp16_grad", [False, True], ids=["grad32", "grad16"])
@pytest.mark.parametrize("case", AC.CASE_NAMES)
def test_crafted_state_against_the_oracle(torch_mod, path, case, fp16_grad):
    torch = torch_mod
    block = options(case)
    ls = 1.0 if fp16_grad else AC.loss_scale(case)
    p, opt, ref, g16 = crafted(torch, block)
    if fp16_grad:
        p.grad_dtype = torch.float16  # torch keeps a gradient in its tensor's dtype unless told otherwise
    assert_adam_bits(arrays(opt, p), ref, (case, "loaded state"), names=NAMES)
    for k in range(3):
        g = np.roll(g16, 5 * k)
        p.grad = grad16(torch, g) if fp16_grad else grad32(torch, g, ls)
        opt.step()
        T = AC.CRAFT_GLOBAL_STEP + 1 + k
        before = {name: ref[name].copy() for name in NAMES}
        oracle_adam_step(dict(block, otype="Adam"), AC.CRAFT_N_MATRIX, ls, T, ref, g)
        assert opt.state[p]["step"] == T
        assert_adam_bits(arrays(opt, p), ref, (case, fp16_grad, k), names=NAMES)
        # the skipped parameters (a non-matrix parameter with a +-0 gradient, a frozen class) kept everything
        skipped = ref["steps"] == before["steps"]
        assert skipped.any() or case not in ("default", "freeze_matrix", "freeze_nonmatrix")
        assert_adam_bits(arrays(opt, p), before, (case, fp16_grad, k, "skipped"), names=NAMES, where=skipped)


# ---------------------------------------------------------------------------------------------
# 6: optimizer behaviour
# ---------------------------------------------------------------------------------------------
def test_two_groups_missing_grad_and_lr(torch_mod, path):
    """two tensors in two groups with different options follow their own oracles; a tensor without a gradient is
    untouched; lr written between steps (as a scheduler does) holds from the next step"""
    torch = torch_mod
    import tinycudann as tcnn
    blocks = [options("combined"), options("l2_nonmat")]
    n_matrix = [AC.CRAFT_N_MATRIX, 7]
    refs, params, g16s = [], [], []
    for i in range(2):
        ref = AC.crafted_state(AC.CRAFT_N - 3 * i, seed=20 + i)
        g16s.append(ref.pop("g16"))
        ref["w16"] = O.f2h(ref["w32"])
        refs.append(ref)
        params.append(torch.nn.Parameter(torch.from_numpy(ref["w32"].copy()).cuda()))
    idle = torch.nn.Parameter(torch.ones(100, device="cuda"))
    opt = tcnn.optim.Adam([dict(blocks[0], params=[params[0], idle], n_matrix=n_matrix[0]),
                           dict(blocks[1], params=[params[1]], n_matrix=n_matrix[1])])
    for i in range(2):
        load(torch, opt, params[i], refs[i])
    for k in range(3):
        if k == 1:
            opt.param_groups[0]["lr"] = 0.05
            blocks[0] = dict(blocks[0], learning_rate=0.05)
        if k == 2:
            opt.param_groups[1]["learning_rate"] = 3e-3
            blocks[1] = dict(blocks[1], learning_rate=3e-3)
        for i in range(2):
            params[i].grad = grad32(torch, np.roll(g16s[i], k), 1.0)
        opt.step()
        for i in range(2):
            oracle_adam_step(dict(blocks[i], otype="Adam"), n_matrix[i], 1.0, AC.CRAFT_GLOBAL_STEP + 1 + k, refs[i], np.roll(g16s[i], k))
            assert_adam_bits(arrays(opt, params[i]), refs[i], (i, k), names=NAMES)
    assert opt.param_groups[0]["lr"] == opt.param_groups[0]["learning_rate"] == 0.05
    assert opt.param_groups[1]["lr"] == opt.param_groups[1]["learning_rate"] == 3e-3
    assert bool((idle == 1).all()) and idle not in opt.state


def test_state_dict_round_trip(torch_mod, path):
    torch = torch_mod
    import tinycudann as tcnn
    block = options("combined")
    p, opt, ref, g16 = crafted(torch, block)
    p.grad = grad32(torch, g16, 1.0)
    opt.step()
    sd = copy.deepcopy(opt.state_dict())  # (load_state_dict keeps the tensors it is given)
    assert set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq", "param_steps"} and sd["state"][0]["param_steps"].dtype == torch.int32
    p2 = torch.nn.Parameter(p.detach().clone())
    opt2 = tcnn.optim.Adam([dict(params=[p2])])  # default options: the loaded groups carry the saved ones
    opt2.load_state_dict(sd)
    assert opt2.param_groups[0]["n_matrix"] == AC.CRAFT_N_MATRIX and opt2.param_groups[0]["beta1"] == block["beta1"]
    g = np.roll(g16, 3)
    p.grad, p2.grad = grad32(torch, g, 1.0), grad32(torch, g, 1.0)
    opt.step()
    opt2.step()
    assert_adam_bits(arrays(opt2, p2), arrays(opt, p), "after load_state_dict", names=NAMES)
    oracle_adam_step(dict(block, otype="Adam"), AC.CRAFT_N_MATRIX, 1.0, AC.CRAFT_GLOBAL_STEP + 1, ref, g16)
    oracle_adam_step(dict(block, otype="Adam"), AC.CRAFT_N_MATRIX, 1.0, AC.CRAFT_GLOBAL_STEP + 2, ref, g)
    assert_adam_bits(arrays(opt2, p2), ref, "the oracle's second step", names=NAMES)


def test_refusals(torch_mod):
    torch = torch_mod
    import tinycudann as tcnn
    with pytest.raises(ValueError, match="fp32"):
        tcnn.optim.Adam([torch.nn.Parameter(torch.zeros(8, device="cuda", dtype=torch.float16))])
    with pytest.raises(ValueError, match="GPU"):
        tcnn.optim.Adam([torch.nn.Parameter(torch.zeros(8))])
    with pytest.raises(ValueError, match="contiguous"):
        tcnn.optim.Adam([torch.nn.Parameter(torch.zeros(8, 8, device="cuda").t()[:, :4])])
    with pytest.raises(TypeError, match="unknown options"):
        tcnn.optim.Adam([torch.nn.Parameter(torch.zeros(8, device="cuda"))], weight_decay=0.1)
    with pytest.raises(ValueError, match="n_matrix"):
        tcnn.optim.Adam([torch.nn.Parameter(torch.zeros(8, device="cuda"))], n_matrix=-1)
    # lr is learning_rate
    opt = tcnn.optim.Adam([torch.nn.Parameter(torch.zeros(8, device="cuda"))], lr=0.5)
    assert opt.param_groups[0]["learning_rate"] == opt.param_groups[0]["lr"] == 0.5 and opt.param_groups[0]["beta2"] == 0.999


def test_param_groups(torch_mod):
    torch = torch_mod
    import tinycudann as tcnn
    enc_cfg, net_cfg = CONFIG_HASH["encoding"], CONFIG_HASH["network"]

    class Both(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.nwie = tcnn.NetworkWithInputEncoding(2, 3, enc_cfg, net_cfg)
            self.enc = tcnn.Encoding(2, enc_cfg)
            self.net = tcnn.Network(32, 3, net_cfg)
            self.lin = torch.nn.Linear(3, 5).cuda()

    model = Both()
    groups = tcnn.optim.param_groups(model, learning_rate=0.02)
    by_param = {id(g["params"][0]): g for g in groups}
    n_network = tcnn.Trainer(2, 3, CONFIG_HASH).n_network_params
    assert 0 < n_network < model.nwie.params.numel()
    assert by_param[id(model.nwie.params)]["n_matrix"] == n_network
    assert by_param[id(model.enc.params)]["n_matrix"] == 0
    assert by_param[id(model.net.params)]["n_matrix"] == model.net.params.numel()
    rest = groups[-1]
    assert {id(p) for p in rest["params"]} == {id(model.lin.weight), id(model.lin.bias)} and rest["n_matrix"] is None  # None: all
    assert all(g["learning_rate"] == 0.02 for g in groups) and len(groups) == 4
    opt = tcnn.optim.Adam(groups)
    assert [g["lr"] for g in opt.param_groups] == [0.02] * 4
    # a tinycudann module on its own
    (only,) = tcnn.optim.param_groups(model.nwie)
    assert only["n_matrix"] == n_network and only["params"][0] is model.nwie.params


# ---------------------------------------------------------------------------------------------
# 7: end to end
# ---------------------------------------------------------------------------------------------
def _btf(torch):
    import tinycudann as tcnn
    B = 256
    model = tcnn.NetworkWithInputEncoding(8, 3, CONFIG_BTF["encoding"], CONFIG_BTF["network"], seed=1337)
    rng = np.random.default_rng(5)
    x = rng.uniform(0, 1, (B, 8)).astype(np.float32)
    tgt = np.stack([0.5 + 0.4 * np.sin(6 * x[:, 0]) * x[:, 2], 0.3 + 0.5 * x[:, 1] * x[:, 3], 0.2 + 0.6 * x[:, 0] * x[:, 1]],
                   axis=1).astype(np.float32)
    block = {k: v for k, v in CONFIG_BTF["optimizer"].items() if k != "otype"}
    opt = tcnn.optim.Adam(tcnn.optim.param_groups(model, **block))
    return model, opt, tcnn.Loss("RelativeL2"), torch.from_numpy(x).cuda(), torch.from_numpy(tgt).cuda(), tgt, block


def test_one_training_step_end_to_end(torch_mod, path):
    torch = torch_mod
    model, opt, loss, x, tgt_d, tgt, block = _btf(torch)
    n_matrix = opt.param_groups[0]["n_matrix"]
    assert 0 < n_matrix < model.params.numel()
    out = model(x)
    seen = []
    out.register_hook(seen.append)
    value = loss(out, tgt_d)
    value.backward()
    # the loss from the module's actual output
    pred16 = np.zeros((256, 16), np.uint16)
    pred16[:, :3] = out.detach().cpu().numpy().view(np.uint16)
    v_ref, g_ref = R.evaluate("RelativeL2", pred16, tgt, 1.0)
    np.testing.assert_array_equal(seen[0].cpu().numpy().view(np.uint16), g_ref[:, :3])
    v64 = v_ref[:, :3].astype(np.float64)
    assert abs(float(value.item()) - v64.sum()) <= v64.size * 2.0 ** -24 * np.abs(v64).sum()
    # the step from the parameters before and the actual .grad
    w32 = model.params.detach().cpu().numpy().copy()
    g = model.params.grad.cpu().numpy()
    g16 = O.f2h(g)
    assert np.array_equal(O.h2f(g16), g)  # the module's gradients are fp16 values: the oracle reads them exactly
    assert (g[:n_matrix] != 0).any() and (g[n_matrix:] != 0).any() and (g[n_matrix:] == 0).mean() > 0.5
    ref = {"w32": w32, "w16": O.f2h(w32), "m1": np.zeros_like(w32), "m2": np.zeros_like(w32), "steps": np.zeros(w32.size, np.uint32)}
    opt.step()
    oracle_adam_step(dict(block, otype="Adam"), n_matrix, 1.0, 1, ref, g16)
    assert_adam_bits(arrays(opt, model.params), ref, "end to end", names=NAMES)
    untouched = g[n_matrix:] == 0  # the zero-gradient skip: untouched grid entries are not moved and not counted
    assert np.array_equal(ref["w32"][n_matrix:][untouched], w32[n_matrix:][untouched]) and not ref["steps"][n_matrix:][untouched].any()


def test_thirty_steps_reduce_the_loss(torch_mod, path):
    torch = torch_mod
    model, opt, loss, x, tgt_d, _, _ = _btf(torch)
    values = []
    for _ in range(30):
        opt.zero_grad()
        value = loss(model(x), tgt_d)
        value.backward()
        opt.step()
        values.append(value.detach())
    v = torch.stack(values).cpu().numpy()
    assert np.isfinite(v).all()
    print("loss", v[:5], v[-5:])
    assert v[-5:].mean() < v[:5].mean(), (v[:5], v[-5:])
