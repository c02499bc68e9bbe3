"""GPU tests of tcnn_module_inference_jacobian (csrc/mlp_f32_jacobian.hip): the value and the input Jacobian of an fp32
FullyFusedMLP network module in one forward-mode launch, against float64.

Truth for row o of J is tests/mlp_f32_reference.py's dL/dinput for a one-hot dL/dy, times the Identity scale, and the
bound is that call's e_in times the scale, derived there from operation counts for the same contractions in reverse
order; forward mode has K = W terms where the reverse has N = W or OUTP, and no first-layer contraction: where e_in
allots W u (|D_1| |W0|) to that product, forward mode spends one rounding, u scale (|D_1| |W0|), on scale W0[n][d]
(none for a power of two), so its count is not larger. One case has scale 1.7, where the fma of the Identity row and
that product do round. y must be tcnn_module_inference's bits. Batches 128 and 384 are one and three pairs of the
kernel's 64-row workgroups; inference takes 256-row granules, so its batch is the same rows padded with zeros.
"""
import functools
from fractions import Fraction

import numpy as np
import pytest

import mlp_f32_reference as F
import test_gpu_mlp_f32 as T
from test_gpu_encoding_f32 import FP16, FP32, _vp

pytestmark = pytest.mark.gpu

GUARD, SENTINEL = 64, -7.5
IDENTITY = {"otype": "Identity", "scale": 2, "offset": -1}
ACTS = ("None", "ReLU", "LeakyReLU", "Exponential", "Sigmoid", "Squareplus", "Softplus", "Tanh")


def ff(name, W, NH, n_in, n_out, act, out_act="None", scale=1.5):
    return F.Case(name, W, NH, n_in=n_in, n_out=n_out, act=act, out_act=out_act, otype="FullyFusedMLP", scale=scale)


# (case, encoding in front or None for a network alone)
CASES = [(ff("sdf-w16h1", 16, 1, 3, 1, "ReLU"), None), (ff("w64h3o17", 64, 3, 3, 17, "Tanh", "Sigmoid"), None),
         (ff("w128h2d16", 128, 2, 16, 3, "Tanh"), None)]
# each of the eight as hidden and output activation. Exponential on Exponential at scale 1.5 leaves the range over which
# its accuracy was measured (pre-activations down to -22, mlp_f32_reference.reference asserts [-8, 32]): as in
# mlp_f32_reference.CASES it runs at scale 0.6, and at 1.5 Exponential is the output activation behind ReLU
CASES += [(ff("identity-w32h2", 32, 2, 2, 3, "ReLU" if a == "Exponential" else a, a), IDENTITY) for a in ACTS]
CASES += [(ff("identity-w32h2-s0.6", 32, 2, 2, 3, "Exponential", "Exponential", scale=0.6), IDENTITY),
          (ff("identity1.7-w32h2", 32, 2, 2, 3, "Tanh", "Tanh"), {"otype": "Identity", "scale": 1.7, "offset": -1})]
IDS = [c.id for c, _ in CASES]


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


def truth(case, p, rows, scale):
    """(J [B][n_out][D], its bound) in float64: one reference backward per output"""
    B, D = rows.shape[0], case.n_in
    J, E = np.empty((B, case.n_out, D)), np.empty((B, case.n_out, D))
    for o in range(case.n_out):
        dout = np.zeros((B, case.OUTP), np.float32)
        dout[:, o] = 1.0
        ref = F.reference(case.W, case.IN, case.NH, case.OUTP, case.act, case.out_act, p, rows, dout)
        J[:, o], E[:, o] = ref["dinput"][:, :D] * scale, ref["e_in"][:, :D] * abs(scale)
    return J, E


def fma32(x, scale, offset):
    """float32(x scale + offset) with one rounding, as the Identity encoding's fma: the exact rational, then the nearest
    of the float32 around it"""
    s, o, out = Fraction(float(np.float32(scale))), Fraction(float(np.float32(offset))), np.empty_like(x)
    for k, v in enumerate(x.flat):
        e = Fraction(float(v)) * s + o
        c = np.float32(float(e))
        out.flat[k] = min((c, np.nextafter(c, np.float32(np.inf)), np.nextafter(c, np.float32(-np.inf))), key=lambda t: abs(Fraction(float(t)) - e))
    return out


@functools.lru_cache(maxsize=None)
def setup(i, B):
    """inputs clear of the ReLU branches, parameters, and the float64 truth of case i, computed once"""
    case, enc = CASES[i]
    scale, offset = (enc["scale"], enc["offset"]) if enc else (1, 0)
    x2, _ = F.case_inputs(case, B)
    rows2 = np.ones((x2.shape[0], case.IN), np.float32)
    rows2[:, :case.n_in] = fma32(x2, scale, offset)
    p = F.case_params(case)
    x, rows = F.keep_clear(case, p, x2, rows2, B)
    return x, p, truth(case, p, rows, float(np.float32(scale)))


def make(torch, i, precision=FP32):
    case, enc = CASES[i]
    return T.Net(torch, case.n_in, case.n_out, case.net, enc, precision)


def call(torch, net, case, x, p, mask):
    """one call under a layout mask; (y [B][OUTP] or [B][n_out] under the output bit, J [B][n_out][D]), each result
    buffer exactly its size plus a guard that must come back untouched"""
    B, D, n = x.shape[0], case.n_in, case.n_out
    xd = torch.from_numpy(np.ascontiguousarray(x.T if mask & 1 else x)).cuda()
    pd = torch.from_numpy(p).cuda()
    ny = n * B if mask & 2 else B * case.OUTP
    y = torch.full((ny + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    J = torch.full((B * n * D + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    net.L.check(net.lib.tcnn_module_inference_jacobian(net.h, None, B, _vp(xd), _vp(y), _vp(J), _vp(pd), mask))
    torch.cuda.synchronize()
    y, J = y.cpu().numpy(), J.cpu().numpy()
    assert np.all(y[ny:] == SENTINEL) and np.all(J[B * n * D:] == SENTINEL), "written past the unpadded size"
    assert not np.any(J[:B * n * D] == SENTINEL), "a Jacobian element was not written"
    if mask & 2:
        return y[:ny].reshape(n, B).T.copy(), J[:B * n * D].reshape(n, D, B).transpose(2, 0, 1).copy()
    return y[:ny].reshape(B, case.OUTP), J[:B * n * D].reshape(B, n, D)


def inference(net, x, p):
    """tcnn_module_inference on the rows of x, padded with zero rows to its 256-row granule"""
    pad = -x.shape[0] % 256
    return net.inference(np.concatenate([x, np.zeros((pad, x.shape[1]), np.float32)]), p)[:x.shape[0]]


@pytest.mark.parametrize("B", [128, 384])
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_against_float64(torch_mod, i, B):
    case = CASES[i][0]
    x, p, (Jt, Et) = setup(i, B)
    net = make(torch_mod, i)
    assert net.lib.tcnn_module_engine(net.h) == b"fused" and net.n_params == p.size
    y, J = call(torch_mod, net, case, x, p, 0)
    want = inference(net, x, p)
    net.close()
    q = np.abs(J.astype(np.float64) - Jt) / Et
    q = np.where(np.isnan(q), np.inf, q)
    print(f"jacobian-ratio {case.id} B={B} worst |J - truth| / bound = {q.max():.4f}")
    assert np.abs(Jt).max() > 0 and q.max() <= 1.0, (case.id, float(q.max()), np.unravel_index(int(np.argmax(q)), q.shape))
    np.testing.assert_array_equal(y.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("i", [0, 1], ids=IDS[:2])
def test_soa_is_aos_transposed(torch_mod, i):
    case = CASES[i][0]
    x, p, _ = setup(i, 128)
    net = make(torch_mod, i)
    y0, J0 = call(torch_mod, net, case, x, p, 0)
    for mask in (1, 2, 3):
        y, J = call(torch_mod, net, case, x, p, mask)
        np.testing.assert_array_equal(y.view(np.uint32), y0[:, :y.shape[1]].view(np.uint32), err_msg=f"y, mask {mask}")
        np.testing.assert_array_equal(J.view(np.uint32), J0.view(np.uint32), err_msg=f"J, mask {mask}")
    net.close()


def test_torch_front_end(torch_mod):
    torch = torch_mod
    import tinycudann as tcnn
    case = ff("torch-w64h2", 64, 2, 3, 3, "Tanh")
    m = tcnn.Network(3, 3, case.net, dtype=torch.float32)
    x = torch.rand(200, 3, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5)) * 2 - 1
    y, J = m.value_and_jacobian(x)
    assert y.shape == (200, 3) and J.shape == (200, 3, 3) and not y.requires_grad and not J.requires_grad
    with torch.no_grad():
        assert torch.equal(y, m(x))
    ys, Js = m.value_and_jacobian(x.T.contiguous(), layout="soa")
    assert torch.equal(ys.T, y) and torch.equal(Js.permute(2, 0, 1), J)
    rows = np.ones((200, 16), np.float32)
    rows[:, :3] = x.cpu().numpy()
    Jt, Et = truth(case, m.params.detach().cpu().numpy(), rows, 1)
    xg = x.clone().requires_grad_(True)
    yg = m(xg)
    for o in range(3):
        g = torch.autograd.grad(yg[:, o].sum(), xg, retain_graph=True)[0].cpu().numpy().astype(np.float64)
        j = J[:, o].cpu().numpy().astype(np.float64)
        assert np.all(np.abs(j - Jt[:, o]) <= Et[:, o]) and np.all(np.abs(g - Jt[:, o]) <= Et[:, o])
        assert np.all(np.abs(j - g) <= 2 * Et[:, o])


@pytest.mark.parametrize("what", ["fp16", "cutlass", "grid", "sine"])
def test_refusals(torch_mod, what):
    torch = torch_mod
    net = dict(ff("refuse", 64, 2, 3, 3, "Sine" if what == "sine" else "ReLU").net, otype="CutlassMLP" if what == "cutlass" else "FullyFusedMLP")
    m = T.Net(torch, 3, 3, net, F.GRID2_L4 if what == "grid" else None, FP16 if what == "fp16" else FP32)
    p = m.initial_params(3)
    p = p if m.f32 else p.astype(np.float16).view(np.uint16)
    x = np.random.default_rng(2).uniform(0, 1, (256, 3)).astype(np.float32)
    xd, pd = torch.from_numpy(x).cuda(), m._dev(p)
    y = torch.zeros(256 * 16, dtype=m.dt, device="cuda")
    J = torch.zeros(256 * 9, dtype=torch.float32, device="cuda")
    name = m.lib.tcnn_module_name(m.h).decode()
    message = (rf"{name}: Sine has no backward from its forward value" if what == "sine" else
               rf"{name}.*: inference_jacobian is not implemented by the MI355X engine yet \(fp32 FullyFusedMLP network modules alone or "
               r"behind a lone Identity encoding only\)")
    with pytest.raises(m.L.TcnnError, match=message):
        m.L.check(m.lib.tcnn_module_inference_jacobian(m.h, None, 256, _vp(xd), _vp(y), _vp(J), _vp(pd), 0))
    out = m.inference(x, p)
    assert np.isfinite(out.astype(np.float32) if m.f32 else out.view(np.float16).astype(np.float32)).all()
    m.close()
