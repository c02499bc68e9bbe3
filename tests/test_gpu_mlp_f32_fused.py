"""GPU tests of the fused fp32 MLP kernels (csrc/mlp_f32_fused.hip): an fp32 network module with "otype":
"FullyFusedMLP", at least one hidden layer and a width of 16, 32, 64 or 128 runs its forward and its backward's delta
chain in one launch each, out of registers. Two checks per shape: against float64 within the bounds of
tests/mlp_f32_reference.py (no tolerance of this file's own), and against the layer kernels (the same config as
"CutlassMLP") bit for bit -- the fused kernels keep every element's accumulation order, so nothing may differ.

The shapes are the smallest that reach each way the kernels can go wrong: every width's instantiation, one hidden layer
(no hidden-to-hidden matrix) and three (more than one hand-over), a first layer narrower (IN 16 under W 64) and wider
(IN 48 over W 16) than the rest, 1 / 2 / 5 output tiles (5: a group of four and a rest), an out-of-line activation with
an output transfer, and a grid in front whose dL/dparams reads D_0. Batches: 256 and 768, the smallest and a
non-power-of-two count of the 256-row granules a network module accepts (two and six workgroups of 128 rows, one and
three weight-gradient slabs); the single workgroup of B 128 cannot be asked for through the module interface.
"""
import numpy as np
import pytest

import mlp_f32_reference as F
import test_gpu_mlp_f32 as T

pytestmark = pytest.mark.gpu

FF = dict(otype="FullyFusedMLP")
SMOOTH = dict(act="Tanh", out_act="Sigmoid", **FF)
ROWS = [  # (case, batch)
    (F.Case("w16h2", 16, 2, n_in=16, n_out=1, **FF), 256),
    (F.Case("w16h2in48o65", 16, 2, n_in=48, n_out=65, **SMOOTH), 768),
    (F.Case("w32h1", 32, 1, n_in=3, n_out=17, **SMOOTH), 256),
    (F.Case("w32h2o17", 32, 2, n_in=16, n_out=17, **FF), 768),
    (F.Case("grid-w32h2", 32, 2, n_in=2, n_out=3, enc=F.GRID2_L4, **FF), 768),
    (F.Case("w64h2in16", 64, 2, n_in=3, n_out=3, **FF), 256),
    (F.Case("w64h2in32o65", 64, 2, n_in=32, n_out=65, **FF), 768),
    (F.Case("w64h3o17", 64, 3, n_in=16, n_out=17, **SMOOTH), 768),
    (F.Case("w64h3none", 64, 3, n_in=16, n_out=1, act="None", **FF), 256),
    (F.Case("w128h2", 128, 2, n_in=16, n_out=3, **FF), 256),
    (F.Case("w128h2o65", 128, 2, n_in=48, n_out=65, **SMOOTH), 768),
]
IDS = [f"{c.id}-B{B}" for c, B in ROWS]
_setups = {}


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


def shared_setup(torch, i):
    """inputs, parameters and the float64 reference of row i: computed once, read by both tests"""
    if i not in _setups:
        _setups[i] = T.setup(torch, *ROWS[i])
    return _setups[i]


def kernels(net):
    lib = net.lib
    return [lib.tcnn_module_engine(net.h).decode(), lib.tcnn_module_inference_engine(net.h).decode(),
            lib.tcnn_module_backward_kernel(net.h, 0).decode(), lib.tcnn_module_backward_kernel(net.h, 1).decode()]


def run_all(torch, case, x, dout, p):
    """forward, backward with and without dL/dparams, inference of one module; and the kernels it names"""
    net = T.make_net(torch, case)
    out = net.forward(x, p)
    dx, grad = net.backward(dout)
    dx_only, none = net.backward(dout, want_params=False)
    inf = net.inference(x, p)
    names = kernels(net)
    net.close()
    assert none is None
    return dict(out=out, dx=dx, grad=grad, dx_only=dx_only, inf=inf), names


@pytest.mark.parametrize("i", range(len(ROWS)), ids=IDS)
def test_fused_against_float64(torch_mod, i):
    """The module names the fused kernels, and its forward, inference, network dL/dparams and (Identity in front)
    dL/dinput are within the per-element bounds of tests/mlp_f32_reference.py. The grid row's dL/dinput and grid
    gradient are held by the bit-for-bit test below to the layer path, which tests/test_gpu_mlp_f32.py holds to float64."""
    case, B = ROWS[i]
    x, rows, dout, p, ref, g = shared_setup(torch_mod, i)
    got, names = run_all(torch_mod, case, x, dout, p)
    assert names == ["fused", "fused", "chain", "chain"]
    for v in got.values():
        assert not np.isnan(v).any()
    ratios = F.check(ref, got["out"], got["grad"][:case.n_mlp], None, case.NH, case.id)
    ratios["inference"] = F.check(ref, got["inf"], None, None, case.NH, case.id)["out"]
    if case.enc is None:  # Identity, scale 1: dL/dinput is dL/d(encoding)'s first columns
        for k in ("dx", "dx_only"):
            q = np.abs(got[k] - ref["dinput"][:, :case.n_in]) / ref["e_in"][:, :case.n_in]
            ratios[k] = float(q.max())
            assert q.max() <= 1.0, (case.id, k, q.max())
    print(case.id, B, ratios)


@pytest.mark.parametrize("i", range(len(ROWS)), ids=IDS)
def test_fused_equals_layer_kernels_bit_for_bit(torch_mod, i):
    """The same config as "CutlassMLP" (the layer kernels), same parameters and inputs: forward, inference, dL/dinput
    (with and without dL/dparams asked for) and the FULL dL/dparams are equal as uint32. The grid row's grid part is
    included: the fp32 grid backward accumulates in fixed point (csrc/grid_f32.hip: integer LDS adds, order-independent)
    and is bit-reproducible, so equal D_0 bits give equal grid gradients."""
    case, B = ROWS[i]
    x, rows, dout, p, ref, g = shared_setup(torch_mod, i)
    twin = F.Case(case.name, case.W, case.NH, case.n_in, case.n_out, case.act, case.out_act, case.enc, "CutlassMLP")
    got, _ = run_all(torch_mod, case, x, dout, p)
    want, names = run_all(torch_mod, twin, x, dout, p)
    assert names == ["layered"] * 4
    assert got["grad"].size == p.size
    for k, v in want.items():
        np.testing.assert_array_equal(got[k].view(np.uint32), v.view(np.uint32), err_msg=f"{case.id} {k}")


@pytest.mark.parametrize("otype,W,NH", [("CutlassMLP", 64, 2), ("FullyFusedMLP", 64, 0), ("CutlassMLP", 48, 2)])
def test_dispatch_stays_put_elsewhere(torch_mod, otype, W, NH):
    """the layer kernels everywhere else; FullyFusedMLP without a hidden layer is no module at all (refused when it
    is built, as on the fp16 side), so the fused kernels never see NH 0"""
    case = F.Case("other", W, NH, otype=otype)
    if otype == "FullyFusedMLP":
        with pytest.raises(Exception, match="FullyFusedMLP requires at least 1 hidden layer"):
            T.make_net(torch_mod, case)
        return
    net = T.make_net(torch_mod, case)
    assert kernels(net) == ["layered"] * 4
    net.close()


def test_torch_front_end_matches_its_layered_twin(torch_mod):
    torch = torch_mod
    import tinycudann as tcnn
    cfg = {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": 64, "n_hidden_layers": 2}
    a = tcnn.Network(16, 3, cfg, dtype=torch.float32)
    b = tcnn.Network(16, 3, dict(cfg, otype="CutlassMLP"), dtype=torch.float32)
    assert a.native_tcnn_module.engine() == "fused" and b.native_tcnn_module.engine() == "layered"
    with torch.no_grad():
        b.params.copy_(a.params)
    gen = torch.Generator(device="cuda").manual_seed(5)
    x0 = torch.rand(256, 16, device="cuda", generator=gen) * 2 - 1
    w = torch.rand(256, 3, device="cuda", generator=gen) - 0.5
    res = []
    for m in (a, b):
        with torch.no_grad():
            y_inf = m(x0)
        x = x0.clone().requires_grad_(True)
        y = m(x)
        (y * w).sum().backward()
        res.append((y_inf, y.detach(), x.grad, m.params.grad))
    for u, v in zip(*res):
        assert u.abs().max() > 0 and torch.equal(u, v)
