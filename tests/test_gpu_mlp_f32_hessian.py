"""GPU tests of tcnn_module_inference_hessian (csrc/mlp_f32_hessian.hip): the value, the directional input derivatives and
H[k][k'] = v_k^T (d^2 y / dx^2) v_k' of an fp32 FullyFusedMLP network module, in one forward-mode launch, against float64.

Truth. test_gpu_mlp_f32_jvp_second.f64, the module's function in float64 torch: per output one
autograd.grad(create_graph=True), then one grad per direction, dotted with the directions. Inputs stay 2^-10 of a cell
clear of the cell boundaries (test_gpu_mlp_f32_jvp.clear_of_boundaries; at most a quarter of the candidates may go).

Bound. max|H - H64| <= TOL[case] max|H64|, TOL four times the worst ratio measured on an MI355X over both batches
(profiles/mlp_f32_hessian_ratios.txt, and beside each case). The same modules' q sits at about 4e-7
(profiles/mlp_f32_jvp2_ratios.txt); ten times that would be a defect, not a bound.
"""
import functools

import numpy as np
import pytest

import mlp_f32_reference as F
import test_gpu_mlp_f32 as T
import test_gpu_mlp_f32_jvp as V
import test_gpu_mlp_f32_jvp_second as S
from test_gpu_encoding_f32 import FP16, FP32, _vp

pytestmark = pytest.mark.gpu

LINEAR3 = dict(F.GRID2_L4, interpolation="Linear")
CASES = [  # (case, front, K or None for the unit directions, TOL)
    (V.gc("identity-w16h1", 16, 1, 3, 1, "None", "None", None), S.IDENTITY, None, 0.0),  # H exactly zero, J not
    (V.gc("alone-w32h2", 32, 2, 3, 3, "Tanh", "None", None), None, None, 4 * 6.230e-7),  # six pairs from the activation's curvature
    (V.gc("dense2-l8f4-smooth-w32h2", 32, 2, 2, 3, "Tanh", "None", V.DENSE2_F4), V.DENSE2_F4, None, 4 * 3.450e-7),  # three pairs, the grid's own terms
    (V.gc("hash3-l4f2-linear-w32h2", 32, 2, 3, 3, "Tanh", "None", LINEAR3), LINEAR3, None, 4 * 2.785e-7),  # off-diagonals from the mixed term alone
    (V.gc("tiled3-l8f8-w64h2o17", 64, 2, 3, 17, "Tanh", "Sigmoid", V.TILED3_F8), V.TILED3_F8, 3, 4 * 5.354e-7),  # two output tiles, the output gate
    (S.HASH3_W64, V.HASH3_L16, 2, 4 * 4.499e-7),  # Softplus, hashed levels, two of three pair rows' directions
    (S.HASH3_W64, V.HASH3_L16, 1, 4 * 2.465e-7),  # one pair, an unused tangent row
]
IDS = [f"{c[0].id}-k{c[2]}" for c in CASES]
K3, K2 = 4, 5


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


@functools.lru_cache(maxsize=None)
def setup(i, B):
    """(parameters, inputs clear of the cell boundaries, directions or None, H in float64 [B][n_out][K][K]) of case i, once"""
    import torch
    case, _, K, _ = CASES[i]
    g = S.grid_of(case)
    p = F.case_params(case, None if g is None else np.random.default_rng(7).uniform(-1, 1, g.n_params).astype(np.float32))
    x = F.case_inputs(case, B)[0]
    if g is not None:
        ok = V.clear_of_boundaries(g, x)
        assert ok.mean() >= 0.75, (case.id, "the boundary filter rejects", 1 - ok.mean())
        x = x[ok]
    x = np.ascontiguousarray(x[:B])
    v = None if K is None else V.directions(x, K)
    xt = torch.from_numpy(x.astype(np.float64)).requires_grad_(True)
    vt = torch.eye(case.n_in, dtype=torch.float64).expand(B, -1, -1) if v is None else torch.from_numpy(v.astype(np.float64))
    y, H = S.f64(torch, case, g, p, xt), np.zeros((B, case.n_out, vt.shape[1], vt.shape[1]))
    for o in range(case.n_out):
        g1 = torch.autograd.grad(y[:, o].sum(), xt, create_graph=True)[0]
        for k in range(vt.shape[1] if g1.requires_grad else 0):  # a function linear in x has a constant gradient
            hv = torch.autograd.grad((g1 * vt[:, k]).sum(), xt, retain_graph=True)[0]
            H[:, o, k] = torch.einsum("bd,bld->bl", hv, vt).numpy()
    return p, x, v, H


def call_h(torch, net, case, x, p, v=None, mask=0):
    """(y, Jv, H [B][n_out][K][K]) of one call under a layout mask; H's buffer is exactly its size plus a guard"""
    B, D, n = x.shape[0], case.n_in, case.n_out
    K = D if v is None else v.shape[1]
    xd = torch.from_numpy(np.ascontiguousarray(x.T if mask & 1 else x)).cuda()
    vd = None if v is None else torch.from_numpy(np.ascontiguousarray(v.transpose(1, 2, 0) if mask & 1 else v)).cuda()
    pd = torch.from_numpy(p).cuda()
    y = torch.zeros(n * B if mask & 2 else B * case.OUTP, dtype=torch.float32, device="cuda")
    J = torch.zeros(B * n * K, dtype=torch.float32, device="cuda")
    nh = B * n * K * K
    H = torch.full((nh + V.GUARD,), V.SENTINEL, dtype=torch.float32, device="cuda")
    net.L.check(net.lib.tcnn_module_inference_hessian(net.h, None, B, _vp(xd), _vp(vd), 0 if v is None else K, _vp(y), _vp(J), _vp(H),
                                                      _vp(pd), mask))
    torch.cuda.synchronize()
    y, J, H = y.cpu().numpy(), J.cpu().numpy(), H.cpu().numpy()
    assert np.all(H[nh:] == V.SENTINEL) and not np.any(H[:nh] == V.SENTINEL), "H written past its size, or not everywhere"
    if mask & 2:
        return y.reshape(n, B).T.copy(), J.reshape(n, K, B).transpose(2, 0, 1).copy(), H[:nh].reshape(n, K, K, B).transpose(3, 0, 1, 2).copy()
    return y.reshape(B, case.OUTP), J.reshape(B, n, K), H[:nh].reshape(B, n, K, K)


def make(torch, i):
    case, front = CASES[i][:2]
    return T.Net(torch, case.n_in, case.n_out, case.net, front)


@pytest.mark.parametrize("B", [128, 384])
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_against_float64(torch_mod, i, B):
    case, _, _, tol = CASES[i]
    p, x, v, Ht = setup(i, B)
    net = make(torch_mod, i)
    assert net.lib.tcnn_module_engine(net.h) == b"fused" and net.n_params == p.size
    _, Jv, H = call_h(torch_mod, net, case, x, p, v)
    net.close()
    if tol == 0.0:
        assert np.all(H == 0) and np.all(Ht == 0) and np.abs(Jv).max() > 0
        return
    ratio = np.abs(H.astype(np.float64) - Ht).max() / np.abs(Ht).max()
    off = np.abs(Ht[:, :, 0, 1:]).max() if Ht.shape[2] > 1 else 1.0
    print(f"hessian-ratio {IDS[i]} B={B} max|H - H64| / max|H64| = {ratio:.3e} (max|H64| = {np.abs(Ht).max():.3e}, off-diagonal {off:.3e})")
    assert off > 0 and ratio <= tol, (IDS[i], ratio)


@pytest.mark.parametrize("i", [K3, K2], ids=[IDS[K3], IDS[K2]])
def test_bits(torch_mod, i):
    case = CASES[i][0]
    p, x, v, _ = setup(i, 128)
    net = make(torch_mod, i)
    y, Jv, H = call_h(torch_mod, net, case, x, p, v)  # call_h checks the guard and that every element is written
    y0, Jv0 = V.call(torch_mod, net, case, x, p, v)
    np.testing.assert_array_equal(y.view(np.uint32), y0.view(np.uint32))
    np.testing.assert_array_equal(Jv.view(np.uint32), Jv0.view(np.uint32))
    np.testing.assert_array_equal(H.view(np.uint32), H.transpose(0, 1, 3, 2).view(np.uint32))
    for k in range(v.shape[1]):
        q = S.call2(torch_mod, net, case, x, p, np.ascontiguousarray(v[:, k:k + 1]))[2]
        np.testing.assert_array_equal(H[:, :, k, k].view(np.uint32), q.view(np.uint32), err_msg=f"direction {k}")
    net.close()


def test_soa_is_aos_transposed(torch_mod):
    case = CASES[K3][0]
    p, x, v, _ = setup(K3, 128)
    net = make(torch_mod, K3)
    r0 = call_h(torch_mod, net, case, x, p, v)
    for mask in (1, 2, 3):
        r = call_h(torch_mod, net, case, x, p, v, mask)
        for name, a, b in zip(("y", "Jv", "H"), r, (r0[0][:, :r[0].shape[1]],) + r0[1:]):
            np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32), err_msg=f"{name}, mask {mask}")
    net.close()


def test_torch_front_end(torch_mod):
    torch = torch_mod
    import tinycudann as tcnn
    case, B = CASES[2][0], 200
    m = tcnn.NetworkWithInputEncoding(2, 3, case.enc, case.net, dtype=torch.float32)
    x = torch.rand(B, 2, device="cuda")
    y, J, H = m.value_jacobian_and_hessian(x)
    y2, Jv, Hv = m.value_jvp_and_hessian(x, torch.eye(2, device="cuda").expand(B, -1, -1))
    assert y.shape == (B, 3) and J.shape == (B, 3, 2) and H.shape == (B, 3, 2, 2) and Hv.shape == (B, 3, 2, 2)
    assert not any(t.requires_grad for t in (y, J, H, y2, Jv, Hv))
    assert torch.equal(y, y2) and H.abs().max() > 0
    assert (H - Hv).abs().max() <= CASES[2][3] * H.abs().max()


@pytest.mark.parametrize("what", ["fp16", "oneblob", "w128", "k4", "sine"])
def test_refusals(torch_mod, what):
    torch = torch_mod
    enc, W = (F.ONEBLOB4 if what == "oneblob" else V.HASH3_L16), (128 if what == "w128" else 64)
    net = V.gc("refuse", W, 2, 3, 1, "Sine" if what == "sine" else "Softplus", "None", None).net
    m = T.Net(torch, 3, 1, net, enc, FP16 if what == "fp16" else FP32)
    p = m.initial_params(3)
    xd, pd = torch.rand(256, 3, device="cuda"), m._dev(p if m.f32 else p.astype(np.float16).view(np.uint16))
    vd = torch.rand(256, 4, 3, device="cuda") if what == "k4" else None
    y, J, H = (torch.zeros(256 * n, dtype=torch.float32, device="cuda") for n in (16, 4, 16))
    name = m.lib.tcnn_module_name(m.h).decode()
    front, why = {"fp16": ("", ""), "oneblob": (" behind OneBlobEncoding", ""), "sine": ("", ""),
                  "w128": (" behind GridEncoding", r": a width of 128 \(16, 32 and 64 are served\)"),
                  "k4": (" behind GridEncoding", r": 4 directions \(at most 3 are served\)")}[what]
    message = (rf"^{name}: Sine has no backward from its forward value: inference_hessian serves the other eight activations "
               rf"\(use inference for the value\)$" if what == "sine" else
               rf"^{name}{front}: inference_hessian is not implemented by the MI355X engine yet \(fp32 FullyFusedMLP network modules "
               rf"alone, behind a lone Identity encoding or behind a lone grid encoding only\){why}$")
    with pytest.raises(m.L.TcnnError, match=message):
        m.L.check(m.lib.tcnn_module_inference_hessian(m.h, None, 256, _vp(xd), _vp(vd), 4 if what == "k4" else 0, _vp(y), _vp(J), _vp(H),
                                                      _vp(pd), 0))
    if what in ("w128", "k4"):  # the first-order call serves the module
        m.L.check(m.lib.tcnn_module_inference_jvp(m.h, None, 256, _vp(xd), None, 0, _vp(y), _vp(J), _vp(pd), 0))
    else:
        out = torch.zeros(256 * 16, dtype=torch.float32 if m.f32 else torch.float16, device="cuda")
        m.L.check(m.lib.tcnn_module_inference(m.h, None, 256, _vp(xd), _vp(out), _vp(pd)))
    torch.cuda.synchronize()
    m.close()
