"""GPU tests of tcnn_module_forward_jvp / tcnn_module_backward_jvp (csrc/mlp_f32_jvp_train.hip): dL/dparams of a loss
L = sum C_y o y + sum C_J o Jv on the value and the directional input derivatives of an fp32 FullyFusedMLP network module
behind a lone grid or a lone Identity, against float64. The truth (torch.float64 autograd on the CPU) and the per-element
bound (every computed quantity carried as value and error bound through the kernels' operations, by the rules of
mlp_f32_reference.py and mlp_f32_second_order_reference.py) are tests/mlp_f32_jvp_train_reference.py; nothing in the bound
comes from a GPU result. The worst |got - truth| / bound of every case is printed (pytest -s) and recorded in
profiles/mlp_f32_jvp_train_ratios.txt.
"""
import functools

import numpy as np
import pytest

import mlp_f32_jvp_train_reference as TR
import test_gpu_mlp_f32 as T
import test_gpu_mlp_f32_jacobian as JT
import test_gpu_mlp_f32_jvp as V
from test_gpu_encoding_f32 import _vp

pytestmark = pytest.mark.gpu

GUARD, SENTINEL = JT.GUARD, JT.SENTINEL
I_ID = JT.IDS.index("identity-w32h2-Softplus-Softplus")
# (case, encoding, index into V.CASES or None for the Identity case)
CASES = [(c, c.enc, i) for i, c in enumerate(V.CASES)] + [(JT.CASES[I_ID][0], JT.CASES[I_ID][1], None)]
IDS = [c.id for c, _, _ in CASES]


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


@functools.lru_cache(maxsize=None)
def setup(i, B):
    """(grid config or None, parameters, inputs) of case i"""
    case, enc, vi = CASES[i]
    if vi is None:
        x, p, _ = JT.setup(I_ID, B)
        return None, p, x
    g, _, p, x, _ = V.setup(vi, B)
    return g, p, x


def cotangents(case, B, K, seed=11):
    r = np.random.default_rng(seed)
    Cy = np.zeros((B, case.OUTP), np.float32)
    Cy[:, :case.n_out] = r.uniform(-1, 1, (B, case.n_out))
    return Cy, r.uniform(-1, 1, (B, case.n_out, K)).astype(np.float32)


def truth_and_bound(torch, i, B, v, Cy, CJ):
    """(dL/dparams float64 [n_params], its bound)"""
    case, enc, _ = CASES[i]
    g, p, x = setup(i, B)
    return TR.truth(torch, case, enc, g, p, x, v, Cy, CJ), TR.bound(case, enc, g, p, x, v, Cy, CJ)


def run(torch, net, case, x, p, v, Cy, CJ, K):
    """forward_jvp + backward_jvp; (y, Jv, dL/dparams), the gradient buffer guarded"""
    B, n = x.shape[0], case.n_out
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    xd, vd, pd, cy, cj = dev(x), dev(v), dev(p), dev(Cy), dev(CJ)
    y = torch.empty(B * case.OUTP, dtype=torch.float32, device="cuda")
    J = torch.empty(B * n * K, dtype=torch.float32, device="cuda")
    grad = torch.full((p.size + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    ctx = net.L.check_ptr(net.lib.tcnn_module_forward_jvp(net.h, None, B, _vp(xd), _vp(vd), 0 if v is None else K, _vp(y), _vp(J), _vp(pd)))
    try:
        net.L.check(net.lib.tcnn_module_backward_jvp(net.h, None, ctx, B, _vp(cy), _vp(cj), _vp(grad), _vp(xd), _vp(vd), _vp(pd)))
        torch.cuda.synchronize()
    finally:
        net.lib.tcnn_context_destroy(ctx)
    grad = grad.cpu().numpy()
    assert np.all(grad[p.size:] == SENTINEL), "written past dL/dparams"
    return y.cpu().numpy().reshape(B, case.OUTP), J.cpu().numpy().reshape(B, n, K), grad[:p.size]


def worst(label, got, want, bound):
    q = np.abs(got.astype(np.float64) - want) / bound
    q = np.where(np.isnan(q), np.inf, q)
    print(f"jvp-train-ratio {label} worst |dL/dparams - truth| / bound = {q.max():.2e}")
    assert np.abs(want).max() > 0 and q.max() <= 1.0, (label, float(q.max()), int(np.argmax(q)))


def make(torch, i):
    case, enc, _ = CASES[i]
    return T.Net(torch, case.n_in, case.n_out, case.net, enc)


def unit_or_one(case, x):
    """null directions, except where the width forces K = 1"""
    return V.directions(x, 1) if case.W == 128 else None


@pytest.mark.parametrize("B", [256, 768])
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_against_float64(torch_mod, i, B):
    case = CASES[i][0]
    _, p, x = setup(i, B)
    v = unit_or_one(case, x)
    K = x.shape[1] if v is None else 1
    Cy, CJ = cotangents(case, B, K)
    net = make(torch_mod, i)
    y, Jv, grad = run(torch_mod, net, case, x, p, v, Cy, CJ, K)
    y0, J0 = V.call(torch_mod, net, case, x, p, v)
    net.close()
    np.testing.assert_array_equal(y.view(np.uint32), y0.view(np.uint32))
    np.testing.assert_array_equal(Jv.view(np.uint32), J0.view(np.uint32))
    ve = np.broadcast_to(np.eye(x.shape[1], dtype=np.float32), (B, K, K)) if v is None else v
    worst(f"{case.id} B={B}", grad, *truth_and_bound(torch_mod, i, B, ve, Cy, CJ))


@pytest.mark.parametrize("zero", ["none", "dL_doutput", "dL_djvp"])
@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("i", [0, 2], ids=[IDS[0], IDS[2]])
def test_directions(torch_mod, i, K, zero):
    case, B = CASES[i][0], 256
    _, p, x = setup(i, B)
    v = V.directions(x, K)
    Cy, CJ = cotangents(case, B, K)
    net = make(torch_mod, i)
    _, _, grad = run(torch_mod, net, case, x, p, v, None if zero == "dL_doutput" else Cy, None if zero == "dL_djvp" else CJ, K)
    net.close()
    Cy, CJ = (np.zeros_like(Cy) if zero == "dL_doutput" else Cy), (np.zeros_like(CJ) if zero == "dL_djvp" else CJ)
    worst(f"{case.id} K={K} zero={zero}", grad, *truth_and_bound(torch_mod, i, B, v, Cy, CJ))


def test_network_part_is_bit_reproducible(torch_mod):
    case, B = CASES[2][0], 768
    _, p, x = setup(2, B)
    Cy, CJ = cotangents(case, B, 3)
    net = make(torch_mod, 2)
    a = run(torch_mod, net, case, x, p, None, Cy, CJ, 3)[2]
    b = run(torch_mod, net, case, x, p, None, Cy, CJ, 3)[2]
    net.close()
    np.testing.assert_array_equal(a[:case.n_mlp].view(np.uint32), b[:case.n_mlp].view(np.uint32))


def test_matches_double_backward_route(torch_mod):
    """one output, null directions: tcnn_module_backward (C_y) plus tcnn_module_backward_backward_input
    (dL_ddLdinput = C_J, dL_doutput = 1), code this feature does not touch, within the sum of the two paths' bounds (both
    are bounded by the bound above: the double-backward route runs the same contractions layer by layer)"""
    torch = torch_mod
    i, B = 0, 256
    case = CASES[i][0]
    _, p, x = setup(i, B)
    D = x.shape[1]
    Cy, CJ = cotangents(case, B, D)
    net = make(torch, i)
    grad = run(torch, net, case, x, p, None, Cy, CJ, D)[2]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    xd, pd, cy, cj = dev(x), dev(p), dev(Cy), dev(CJ.reshape(B, D))
    ones = torch.zeros(B, case.OUTP, device="cuda")
    ones[:, 0] = 1.0
    y = torch.empty(B, case.OUTP, device="cuda")
    g1, g2 = torch.empty(p.size, device="cuda"), torch.empty(p.size, device="cuda")
    ctx = net.L.check_ptr(net.lib.tcnn_module_forward(net.h, None, B, _vp(xd), _vp(y), _vp(pd), 1))
    net.L.check(net.lib.tcnn_module_backward(net.h, None, ctx, B, None, _vp(cy), _vp(g1), _vp(xd), _vp(y), _vp(pd)))
    net.L.check(net.lib.tcnn_module_backward_backward_input(net.h, None, ctx, B, _vp(cj), _vp(xd), _vp(ones), _vp(g2), None, None, _vp(pd)))
    torch.cuda.synchronize()
    net.lib.tcnn_context_destroy(ctx)
    net.close()
    other = (g1 + g2).cpu().numpy()
    _, bound = truth_and_bound(torch, i, B, np.broadcast_to(np.eye(D, dtype=np.float32), (B, D, D)), Cy, CJ)
    assert np.all(np.abs(grad.astype(np.float64) - other) <= 2 * bound)


def test_torch_front_end(torch_mod):
    torch = torch_mod
    import tinycudann as tcnn
    i, B = 1, 256
    case = CASES[i][0]
    g, p, x = setup(i, B)
    m = tcnn.NetworkWithInputEncoding(2, 3, case.enc, case.net, dtype=torch.float32)
    with torch.no_grad():
        m.params.copy_(torch.from_numpy(p))
    xd = torch.from_numpy(x).cuda()
    y, J = m.value_and_jacobian(xd, differentiable=True)
    assert y.requires_grad and J.requires_grad and y.shape == (B, 3) and J.shape == (B, 3, 2)
    y0, J0 = m.value_and_jacobian(xd)
    assert not y0.requires_grad and not J0.requires_grad and torch.equal(y0, y.detach()) and torch.equal(J0, J.detach())
    loss = y.mean() + ((J.norm(dim=-1) - 1) ** 2).mean()
    loss.backward()
    Jd = J.detach().double().cpu()
    nrm = Jd.norm(dim=-1, keepdim=True)
    Cy = np.zeros((B, case.OUTP), np.float32)
    Cy[:, :3] = 1.0 / (3 * B)
    CJ = (2 * (nrm - 1) * Jd / nrm / (3 * B)).numpy().astype(np.float32)
    want, bound = truth_and_bound(torch, i, B, np.broadcast_to(np.eye(2, dtype=np.float32), (B, 2, 2)), Cy, CJ)
    worst("torch eikonal", m.params.grad.cpu().numpy(), want, bound)
    with pytest.raises(ValueError, match="layout='aos' only"):
        m.value_and_jacobian(xd.T.contiguous(), layout="soa", differentiable=True)
    with pytest.raises(ValueError, match="must not require grad"):
        m.value_and_jacobian(xd.clone().requires_grad_(True), differentiable=True)
    y, J = m.value_and_jacobian(xd, differentiable=True)
    with pytest.raises(ValueError, match="double backward"):
        torch.autograd.grad(J.sum(), m.params, create_graph=True)


REFUSED = {  # what: (case index, batch, K, what the message names)
    "k4-w64": (2, 256, 4, r": 4 directions at width 64 \(at most 3 are served"),
    "k3-w128": (3, 256, 3, r": 3 directions at width 128 \(at most 1 are served"),
    "b128": (0, 128, 3, r": a batch of 128 \(a multiple of 256 is served\)"),
    "max_level": (0, 256, 3, ": a grid with max_level or stochastic interpolation in effect"),
}


@pytest.mark.parametrize("what", list(REFUSED))
def test_refusals(torch_mod, what):
    torch = torch_mod
    i, B, K, why = REFUSED[what]
    case = CASES[i][0]
    _, p, x = setup(i, 256)
    net = make(torch, i)
    if what == "max_level":
        net.L.check(net.lib.tcnn_module_set_max_level(net.h, 0.5))
    xd, pd = torch.from_numpy(x).cuda(), torch.from_numpy(p).cuda()
    vd = torch.from_numpy(V.directions(x, K)).cuda()
    y = torch.zeros(256 * case.OUTP, device="cuda")
    J = torch.zeros(256 * case.n_out * K, device="cuda")
    message = (r"^NetworkWithInputEncoding behind GridEncoding: forward_jvp / backward_jvp are not implemented by the MI355X engine yet "
               r"\(.*\)" + why)
    with pytest.raises(net.L.TcnnError, match=message):
        net.L.check_ptr(net.lib.tcnn_module_forward_jvp(net.h, None, B, _vp(xd), _vp(vd), K, _vp(y), _vp(J), _vp(pd)))
    if what == "max_level":
        net.L.check(net.lib.tcnn_module_set_max_level(net.h, 1000.0))
    assert np.isfinite(net.inference(x, p)).all()
    net.close()
