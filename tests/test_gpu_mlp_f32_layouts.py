"""GPU tests of batch-contiguous (SoA) matrices on fp32 FullyFusedMLP network modules: tcnn_module_inference_layout /
_forward_layout / _backward_layout (csrc/mlp_f32_fused.hip's layout variants). A SoA matrix is [width][B] at its
unpadded width. The accumulation order of the kernels does not depend on the layout, so every result must be the AoS
entry's bits, transposed and with the padding dropped: no tolerance. One shape per width is also held to float64
within the bounds of tests/mlp_f32_reference.py, so the check does not rest on the AoS path alone.

Every SoA result buffer is exactly its unpadded size followed by a guard of sentinels, which must come back untouched:
the padded neurons are never written. Batches are 256 and 768, the smallest and a non-power-of-two count of the 256-row
granules a network module accepts (two and six workgroups; B 128 cannot be asked for through the module interface).
"""
import numpy as np
import pytest

import mlp_f32_reference as F
import test_gpu_mlp_f32 as T
from test_gpu_encoding_f32 import FP16, Mod, _vp

pytestmark = pytest.mark.gpu

IN_, OUT_, DOUT_, DIN_ = 1, 2, 4, 8  # TCNN_LAYOUT_SOA_*
GUARD, SENTINEL = 64, -7.5
GRID3 = {"otype": "HashGrid", "n_levels": 4, "n_features_per_level": 2, "log2_hashmap_size": 10, "base_resolution": 4,
         "per_level_scale": 1.5}
FRONTS = {"in16": dict(n_in=16), "in48": dict(n_in=48), "grid3d": dict(n_in=3, enc=GRID3)}
MESSAGE = r"batch-contiguous matrices are not implemented by the MI355X engine yet \(fp32 FullyFusedMLP network modules only\)"


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


def make_case(W, NH, n_out, out_act, front):
    return F.Case(f"w{W}h{NH}o{n_out}-{front}", W, NH, n_out=n_out, out_act=out_act, otype="FullyFusedMLP", **FRONTS[front])


def inputs(case, B):
    x, dout = F.case_inputs(case, B)
    table = None
    if case.enc is not None:
        table = np.random.default_rng(7).uniform(-1, 1, T.O.grid_cfg(case.enc, case.n_in).n_params).astype(np.float32)
    return x[:B], dout, F.case_params(case, table)


def call(torch, net, case, x, dout, p, mask):
    """forward, backward and inference of one module under one mask; every result as unpadded AoS [B][width]"""
    B, lib, L = x.shape[0], net.lib, net.L

    def to_dev(a, soa, width):  # an [B][>= width] host matrix as the call reads it
        return torch.from_numpy(np.ascontiguousarray(a[:, :width].T if soa else a)).cuda()

    def result(soa, width, padded):  # a result buffer; SoA: exactly width * B floats, then the guard
        return torch.full((width * B + GUARD if soa else B * padded,), SENTINEL, dtype=torch.float32, device="cuda")

    def to_host(t, soa, width, padded):
        a = t.cpu().numpy()
        if not soa:
            return a.reshape(B, padded)[:, :width].copy()
        assert np.all(a[width * B:] == SENTINEL), "a SoA result was written past its unpadded size"
        return a[:width * B].reshape(width, B).T.copy()

    xd, pd = to_dev(x, mask & IN_, case.n_in), torch.from_numpy(p).cuda()
    dd = to_dev(dout, mask & DOUT_, case.n_out)
    out, inf = (result(mask & OUT_, case.n_out, case.OUTP) for _ in range(2))
    dx, grad = result(mask & DIN_, case.n_in, case.n_in), torch.full((p.size,), SENTINEL, dtype=torch.float32, device="cuda")
    ctx = L.check_ptr(lib.tcnn_module_forward_layout(net.h, None, B, _vp(xd), _vp(out), _vp(pd), 1, mask))
    L.check(lib.tcnn_module_backward_layout(net.h, None, ctx, B, _vp(dx), _vp(dd), _vp(grad), _vp(xd), _vp(out), _vp(pd), mask))
    L.check(lib.tcnn_module_inference_layout(net.h, None, B, _vp(xd), _vp(inf), _vp(pd), mask))
    torch.cuda.synchronize()
    lib.tcnn_context_destroy(ctx)
    return dict(out=to_host(out, mask & OUT_, case.n_out, case.OUTP), inf=to_host(inf, mask & OUT_, case.n_out, case.OUTP),
                dx=to_host(dx, mask & DIN_, case.n_in, case.n_in), grad=grad.cpu().numpy())


def assert_same_bits(got, want, label):
    for k, v in want.items():
        assert np.abs(v).max() > 0, (label, k)
        np.testing.assert_array_equal(got[k].view(np.uint32), v.view(np.uint32), err_msg=f"{label} {k}")


@pytest.mark.parametrize("B", [256, 768])
@pytest.mark.parametrize("front", list(FRONTS))
@pytest.mark.parametrize("out_act", ["None", "Sigmoid"])
@pytest.mark.parametrize("n_out", [1, 3, 16, 20])
@pytest.mark.parametrize("NH", [1, 3])
@pytest.mark.parametrize("W", [16, 32, 64, 128])
def test_soa_equals_aos_bit_for_bit(torch_mod, W, NH, n_out, out_act, front, B):
    """all four matrices SoA against the existing AoS entries (mask 0 forwards to them): output, inference, dL/dinput
    and the full dL/dparams, a grid's table gradient included (fixed-point sums, bit-reproducible)"""
    case = make_case(W, NH, n_out, out_act, front)
    x, dout, p = inputs(case, B)
    net = T.make_net(torch_mod, case)
    assert net.lib.tcnn_module_engine(net.h) == b"fused"
    want = call(torch_mod, net, case, x, dout, p, 0)
    got = call(torch_mod, net, case, x, dout, p, 15)
    net.close()
    assert_same_bits(got, want, case.id)


@pytest.mark.parametrize("front", ["in48", "grid3d"])
def test_every_mask_on_one_shape(torch_mod, front):
    """the sixteen masks one by one (every mix of layouts between the four matrices), two output tiles, Sigmoid"""
    case = make_case(64, 2, 20, "Sigmoid", front)
    x, dout, p = inputs(case, 256)
    net = T.make_net(torch_mod, case)
    want = call(torch_mod, net, case, x, dout, p, 0)
    for mask in range(1, 16):
        assert_same_bits(call(torch_mod, net, case, x, dout, p, mask), want, f"{case.id} mask {mask}")
    net.close()


@pytest.mark.parametrize("W,NH,n_out,out_act,n_in,B", [(16, 3, 20, "Sigmoid", 48, 768), (32, 1, 3, "None", 16, 256),
                                                       (64, 3, 1, "None", 16, 256), (128, 1, 16, "Sigmoid", 48, 768)])
def test_soa_against_float64(torch_mod, W, NH, n_out, out_act, n_in, B):
    """the SoA call alone against the float64 reference, within the bounds of tests/mlp_f32_reference.py"""
    case = F.Case(f"w{W}h{NH}o{n_out}in{n_in}", W, NH, n_in=n_in, n_out=n_out, out_act=out_act, otype="FullyFusedMLP")
    x, rows, dout, p, ref, _ = T.setup(torch_mod, case, B)
    net = T.make_net(torch_mod, case)
    got = call(torch_mod, net, case, x, dout, p, 15)
    net.close()
    pad = lambda a, w: np.concatenate([a, np.zeros((B, w - a.shape[1]), np.float32)], axis=1)  # noqa: E731
    ref_cols = {k: (v[:, :n_out] if k in ("out", "e_out") else v) for k, v in ref.items()}
    ratios = F.check(ref_cols, got["out"], got["grad"], pad(got["dx"], case.IN), case.NH, case.id)
    ratios["inference"] = F.check(ref_cols, got["inf"], None, None, case.NH, case.id)["out"]
    print(case.id, B, ratios)


def test_other_modules_refuse(torch_mod):
    """an fp16 module, an fp32 CutlassMLP module and a stand-alone encoding answer a non-zero mask with the message,
    and mask 0 with the existing entry's bits"""
    torch = torch_mod
    case = F.Case("refuse", 64, 2)
    x, dout, p = inputs(case, 256)
    for m in (T.make_net(torch, case, FP16, "plain"), T.make_net(torch, case), Mod(torch, 16, {"otype": "Identity"})):
        params = None if not m.n_params else p if m.f32 else p.astype(np.float16).view(np.uint16)
        want = m.forward(x, params)
        out = torch.full(want.shape, float("nan"), dtype=m.dt, device="cuda")
        ctx = m.L.check_ptr(m.lib.tcnn_module_forward_layout(m.h, None, 256, _vp(m.x), _vp(out), _vp(m.p), 1, 0))
        torch.cuda.synchronize()
        m.lib.tcnn_context_destroy(ctx)
        np.testing.assert_array_equal(m._host(out).view(np.uint8), want.view(np.uint8))
        for mask in (IN_, OUT_, 15):
            with pytest.raises(m.L.TcnnError, match=MESSAGE):
                m.L.check(m.lib.tcnn_module_inference_layout(m.h, None, 256, _vp(m.x), _vp(out), _vp(m.p), mask))
            assert not m.lib.tcnn_module_forward_layout(m.h, None, 256, _vp(m.x), _vp(out), _vp(m.p), 1, mask)
            with pytest.raises(m.L.TcnnError, match=MESSAGE):
                m.L.check(m.lib.tcnn_module_backward_layout(m.h, None, m.ctx, 256, None, _vp(out), None, _vp(m.x), _vp(out), _vp(m.p), mask))
        m.close()


def test_torch_front_end_soa(torch_mod):
    """module(x, layout="soa"): [D, B] -> [n_out, B] with first-order autograd, the AoS call's values transposed"""
    torch = torch_mod
    import tinycudann as tcnn
    cfg = {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": 64, "n_hidden_layers": 2}
    m = tcnn.NetworkWithInputEncoding(3, 3, GRID3, cfg, dtype=torch.float32)
    gen = torch.Generator(device="cuda").manual_seed(5)
    x0 = torch.rand(200, 3, device="cuda", generator=gen)  # padded to 256 inside
    w = torch.rand(200, 3, device="cuda", generator=gen) - 0.5
    res = []
    for soa in (False, True):
        m.params.grad = None
        x = (x0.T.contiguous() if soa else x0.clone()).requires_grad_(True)
        y = m(x, layout="soa") if soa else m(x)
        (y * (w.T if soa else w)).sum().backward()
        res.append([t.T if soa else t for t in (y.detach(), x.grad)] + [m.params.grad.clone()])
    assert res[1][0].shape == (200, 3)
    for u, v in zip(*res):
        assert u.abs().max() > 0 and torch.equal(u, v)
    with pytest.raises(RuntimeError, match=MESSAGE):
        tcnn.Network(16, 3, cfg)(x0.new_zeros(16, 256), layout="soa")
