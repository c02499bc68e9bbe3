"""The torch front end of fp32 network modules: tinycudann.Network / NetworkWithInputEncoding with
dtype=torch.float32, on both autograd nodes (the C++ extension's and the Python autograd.Function). Gradients are
held to the float64 reference and bounds of tests/mlp_f32_reference.py; Adam to the oracle's Adam bit for bit (the
tolerance tests/test_gpu_torch_adam.py holds fp32 parameters to; the oracle is checked against a float64 Adam in
tests/test_adam_reference.py), on gradients rounded to fp16 values, which is what that oracle reads.
"""
import pickle

import numpy as np
import pytest

import mlp_f32_reference as F
from helpers import assert_adam_bits, oracle_adam_step
from oracle import oracle as O

pytestmark = pytest.mark.gpu

NET = {"otype": "CutlassMLP", "activation": "Tanh", "output_activation": "None", "n_neurons": 48, "n_hidden_layers": 2}
ENC = {"otype": "OneBlob", "n_bins": 4}
U = 2.0 ** -24


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(params=[False, True], ids=["cpp_node", "py_node"])
def node(request, monkeypatch):
    """the C++ autograd node and the Python one (what TCNN_TORCH_PY=1 selects)"""
    from tinycudann import modules
    if request.param:
        monkeypatch.setattr(modules, "_EXT", None)
    elif modules._EXT is None:
        pytest.fail("the C++ extension (lib/_tcnn_torch) is not built")
    return "py" if request.param else "cpp"


def test_network_dtypes(torch_mod, node):
    import tinycudann as tcnn
    torch = torch_mod
    m = tcnn.Network(3, 4, NET, dtype=torch.float32)
    assert m.params.dtype == torch.float32 and m.dtype == torch.float32 and m.loss_scale == 1.0
    assert m.precision == tcnn.modules.PRECISION_FP32
    x = torch.rand(300, 3, device="cuda")
    y = m(x)
    assert y.dtype == torch.float32 and tuple(y.shape) == (300, 4) and bool(torch.isfinite(y).all())
    with torch.no_grad():
        assert m(x).dtype == torch.float32
    # the fp16 module of the same config starts from the same fp32 values
    h = tcnn.Network(3, 4, NET)
    assert h.params.dtype == torch.float32 and h.dtype == torch.float16  # fp32 masters of an fp16 module
    assert torch.equal(h.params.detach(), m.params.detach())
    assert h(x).dtype == torch.float16
    assert tcnn.Network(3, 4, NET, dtype=torch.float16).dtype == torch.float16


def test_network_with_input_encoding_dtypes(torch_mod, node):
    import tinycudann as tcnn
    torch = torch_mod
    m = tcnn.NetworkWithInputEncoding(2, 3, ENC, NET, dtype=torch.float32)
    assert m.params.dtype == torch.float32 and m.dtype == torch.float32 and m.loss_scale == 1.0
    x = torch.rand(256, 2, device="cuda", requires_grad=True)
    y = m(x)
    assert y.dtype == torch.float32 and tuple(y.shape) == (256, 3)
    y.sum().backward()
    assert m.params.grad.dtype == torch.float32 and x.grad.dtype == torch.float32
    assert bool(torch.isfinite(m.params.grad).all()) and float(m.params.grad.abs().max()) > 0
    assert tcnn.NetworkWithInputEncoding(2, 3, ENC, NET).dtype == torch.float16


def _reference(m, x, w, n_in, n_out):
    """float64 truth and bounds of a Network(n_in, n_out, NET) at its parameters for the loss sum(y * w)"""
    case = F.Case("torch", NET["n_neurons"], NET["n_hidden_layers"], n_in=n_in, n_out=n_out, act=NET["activation"])
    rows = F.identity_rows(case, x)
    dout = np.zeros((x.shape[0], case.OUTP), np.float32)
    dout[:, :n_out] = w
    p = m.params.detach().cpu().numpy()
    return case, F.reference(case.W, case.IN, case.NH, case.OUTP, case.act, case.out_act, p, rows, dout)


def test_backward_against_float64(torch_mod, node):
    """loss = sum(y * w): params.grad, x.grad and y within the bounds (loss scale 1: nothing is scaled)"""
    import tinycudann as tcnn
    torch = torch_mod
    rng = np.random.default_rng(2)
    m = tcnn.Network(5, 3, NET, dtype=torch.float32)
    with torch.no_grad():
        m.params.mul_(1.5)
    xn, wn = rng.uniform(-1, 1, (256, 5)).astype(np.float32), rng.uniform(-1, 1, (256, 3)).astype(np.float32)
    x = torch.from_numpy(xn).cuda().requires_grad_(True)
    y = m(x)
    (y * torch.from_numpy(wn).cuda()).sum().backward()
    case, ref = _reference(m, xn, wn, 5, 3)
    q = np.abs(y.detach().cpu().numpy() - ref["out"][:, :3]) / ref["e_out"][:, :3]
    assert q.max() <= 1.0, q.max()
    r = F.check(ref, None, m.params.grad.cpu().numpy(), None, case.NH, node)
    qx = np.abs(x.grad.cpu().numpy() - ref["dinput"][:, :5]) / ref["e_in"][:, :5]
    assert qx.max() <= 1.0, qx.max()
    print(node, r, "out", q.max(), "dinput", qx.max())


def test_module_called_twice_in_one_graph(torch_mod, node):
    """y = m(x1) + 2 m(x2): torch adds the two calls' fp32 gradients -- the sum of the two references within the
    sum of their bounds plus the addition's rounding"""
    import tinycudann as tcnn
    torch = torch_mod
    rng = np.random.default_rng(3)
    m = tcnn.Network(5, 3, NET, dtype=torch.float32)
    xs = [rng.uniform(-1, 1, (256, 5)).astype(np.float32) for _ in range(2)]
    wn = rng.uniform(-1, 1, (256, 3)).astype(np.float32)
    x1, x2 = (torch.from_numpy(v).cuda().requires_grad_(True) for v in xs)
    y = m(x1) + 2.0 * m(x2)
    (y * torch.from_numpy(wn).cuda()).sum().backward()
    refs = [_reference(m, xs[0], wn, 5, 3)[1], _reference(m, xs[1], 2.0 * wn, 5, 3)[1]]
    want = np.concatenate([(a + b).ravel() for a, b in zip(refs[0]["wgrad"], refs[1]["wgrad"])])
    bound = np.concatenate([(a + b).ravel() for a, b in zip(refs[0]["e_w"], refs[1]["e_w"])]) + U * np.abs(want)
    q = np.abs(m.params.grad.cpu().numpy() - want) / bound
    assert q.max() <= 1.0, q.max()
    for xg, ref in ((x1.grad, refs[0]), (x2.grad, refs[1])):
        qx = np.abs(xg.cpu().numpy() - ref["dinput"][:, :5]) / ref["e_in"][:, :5]
        assert qx.max() <= 1.0, qx.max()


def test_pickle_keeps_the_precision(torch_mod, node):
    import tinycudann as tcnn
    torch = torch_mod
    x = torch.rand(256, 2, device="cuda")
    for m in (tcnn.NetworkWithInputEncoding(2, 3, ENC, NET, dtype=torch.float32), tcnn.Network(2, 3, NET, dtype=torch.float32)):
        c = pickle.loads(pickle.dumps(m))
        assert c.precision == tcnn.modules.PRECISION_FP32 and c.params.dtype == torch.float32
        assert c.native_tcnn_module.param_precision() == tcnn.modules.PRECISION_FP32
        with torch.no_grad():
            a, b = m(x), c(x)
        assert b.dtype == torch.float32 and torch.equal(a, b)
    h = pickle.loads(pickle.dumps(tcnn.Network(2, 3, NET)))
    assert h.native_tcnn_module.param_precision() == tcnn.modules.PRECISION_FP16


def test_param_groups_and_adam_steps(torch_mod, node):
    """optim.param_groups finds the matrix / non-matrix boundary of an fp32 model (a grid in front: the network's
    parameters are the matrix class), and three steps of tinycudann.optim.Adam move its fp32 parameters exactly as
    the oracle's Adam does from the same gradients (each step's gradient rounded to an fp16 value first, the
    oracle's input format; loss scale 1)."""
    import tinycudann as tcnn
    torch = torch_mod
    grid = {"otype": "HashGrid", "n_levels": 4, "n_features_per_level": 2, "log2_hashmap_size": 12, "base_resolution": 8,
            "per_level_scale": 1.5}
    net = dict(NET, n_neurons=32, otype="FullyFusedMLP", activation="ReLU")
    m = tcnn.NetworkWithInputEncoding(2, 3, grid, net, dtype=torch.float32)
    block = {"learning_rate": 1e-2, "non_matrix_learning_rate_factor": 0.5}
    groups = tcnn.optim.param_groups(m, **block)
    n_matrix = 32 * 16 + 32 * 32 + 16 * 32
    assert len(groups) == 1 and groups[0]["n_matrix"] == n_matrix and groups[0]["params"][0] is m.params
    assert 0 < n_matrix < m.params.numel()
    opt = tcnn.optim.Adam(groups)
    w0 = m.params.detach().cpu().numpy().copy()
    n = w0.size
    ref = {"w32": w0.copy(), "w16": O.f2h(w0), "m1": np.zeros(n, np.float32), "m2": np.zeros(n, np.float32), "steps": np.zeros(n, np.uint32)}
    x = torch.rand(256, 2, device="cuda")
    t = torch.rand(256, 3, device="cuda")
    for k in range(3):
        opt.zero_grad()
        ((m(x) - t) ** 2).mean().backward()
        assert m.params.grad.dtype == torch.float32
        g16 = m.params.grad.half()
        assert float(g16.float().abs().max()) > 0
        m.params.grad = g16.float()
        opt.step()
        oracle_adam_step(dict(block, otype="Adam"), n_matrix, 1.0, k + 1, ref, g16.cpu().numpy().view(np.uint16))
        s = opt.state[m.params]
        got = {"w32": m.params.detach().cpu().numpy(), "m1": s["exp_avg"].cpu().numpy(), "m2": s["exp_avg_sq"].cpu().numpy(),
               "steps": s["param_steps"].cpu().numpy().view(np.uint32)}
        assert_adam_bits(got, ref, (node, k), names=("w32", "m1", "m2", "steps"))
    assert np.any(m.params.detach().cpu().numpy()[:n_matrix] != w0[:n_matrix])
    assert np.any(m.params.detach().cpu().numpy()[n_matrix:] != w0[n_matrix:])


def test_other_dtypes_raise(torch_mod):
    import tinycudann as tcnn
    torch = torch_mod
    with pytest.raises(ValueError, match="only supports fp32 or fp16 precision"):
        tcnn.Network(3, 4, NET, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="only supports fp32 or fp16 precision"):
        tcnn.NetworkWithInputEncoding(2, 3, ENC, NET, dtype=torch.float64)
    with pytest.raises(ValueError, match="only supports fp32 or fp16 precision"):
        tcnn.Encoding(2, ENC, dtype=torch.bfloat16)


def test_default_dtype_is_fp16(torch_mod):
    import tinycudann as tcnn
    torch = torch_mod
    m = tcnn.Network(3, 4, NET, dtype=None)
    assert m.native_tcnn_module.param_precision() == tcnn.modules.PRECISION_FP16
    assert m.native_tcnn_module._param_dtype == torch.float16 and m.loss_scale == 128.0
    y = m(torch.rand(256, 3, device="cuda"))
    assert y.dtype == torch.float16
