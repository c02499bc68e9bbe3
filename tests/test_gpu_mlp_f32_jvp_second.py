"""GPU tests of tcnn_module_inference_jvp_second (csrc/mlp_f32_jvp2.hip): the value, the directional input derivatives
and q = sum_k v_k^T H v_k of an fp32 FullyFusedMLP network module, in one forward-mode launch, against float64.

Truth. The module's function restated in float64 torch on the CPU: the matrices from the module's parameters, a grid
front from test_grid_f32_reference.level_corners' entries with the interpolation written in torch at the fraction the
kernel sees (the single-rounded fmaf, as test_gpu_mlp_f32_jvp.fractions has it, with slope scale), and q from two
applications of torch.autograd.grad along each v_k. No case has a ReLU, so only the cell boundaries are kept clear
(2^-10 of a cell, test_gpu_mlp_f32_jvp.clear_of_boundaries; at most a quarter of the candidates may go).

Bound. |q - q64| <= TOL[case] max|q64|, TOL four times the worst ratio measured on an MI355X over both batches
(profiles/mlp_f32_jvp2_ratios.txt); every one is far below 1e-3, and each case's own term (in its comment) is of order
one when dropped. y and Jv must be tcnn_module_inference_jvp's bits.
"""
import functools

import numpy as np
import pytest

import mlp_f32_reference as F
import test_gpu_mlp_f32 as T
import test_gpu_mlp_f32_jvp as V
import test_grid_f32_reference as G
from oracle import oracle as O
from test_gpu_encoding_f32 import FP16, FP32, _vp

pytestmark = pytest.mark.gpu

HASH3_W64 = V.gc("hash3-l16f2-w64h2", 64, 2, 3, 1, "Softplus", "None", V.HASH3_L16)
IDENTITY = {"otype": "Identity"}  # in front of a case without an encoding: a lone Identity, where None is the network alone
CASES = [  # (case, K or None for the unit directions, TOL)
    (V.gc("identity-w16h1", 16, 1, 3, 1, "None", "None", None), None, 0.0),  # behind an Identity; q is exactly zero
    (V.gc("alone-w32h2", 32, 2, 3, 3, "Tanh", "None", None), None, 4 * 3.856e-7),  # the activation's curvature
    (V.gc("dense2-l8f4-smooth-w32h2", 32, 2, 2, 3, "Tanh", "None", V.DENSE2_F4), None, 4 * 2.556e-7),  # the grid's diagonal second derivatives
    (V.gc("tiled3-l8f8-w64h2o17", 64, 2, 3, 17, "Tanh", "Sigmoid", V.TILED3_F8), 4, 4 * 3.900e-7),  # mixed terms, two passes, two output tiles
    (HASH3_W64, 2, 4 * 3.866e-7),  # two levels per lane, hashed levels, Softplus (width 128 is refused: test_refusals)
]
IDS = [c[0].id for c in CASES]
ACT = {"None": lambda z: z, "Tanh": lambda z: z.tanh(), "Sigmoid": lambda z: z.sigmoid(),
       "Softplus": lambda z: (1 + (10 * z).exp()).log() / 10}


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


def grid_of(case):
    return O.grid_cfg(case.enc, case.n_in) if case.enc else None


def make(torch, i):
    case = CASES[i][0]
    return T.Net(torch, case.n_in, case.n_out, case.net, IDENTITY if i == 0 else case.enc)


def f64(torch, case, g, p, x):
    """y [B][n_out] in float64 torch from x (float64, requires grad) and the parameters p"""
    B, D = x.shape
    if g is None:
        rows = torch.cat([x, torch.ones(B, case.IN - D, dtype=torch.float64)], 1)
    else:
        xh = x.detach().numpy().astype(np.float32)
        table, cols = torch.from_numpy(p[case.n_mlp:].astype(np.float64)).reshape(-1, g.n_features_per_level), []
        for l in range(g.n_levels):
            idx = torch.from_numpy(G.level_corners(g, l, xh)[0])
            f = torch.from_numpy(V.fractions(g, l, xh)) + (x - x.detach()) * float(np.float32(g.scales[l]))
            s = f * f * (3 - 2 * f) if g.interpolation == 2 else f
            w = [torch.stack([s[:, d] if c >> d & 1 else 1 - s[:, d] for d in range(D)]).prod(0) for c in range(1 << D)]
            cols.append(sum(w[c][:, None] * table[idx[:, c]] for c in range(1 << D)))
        rows = torch.cat(cols + [torch.zeros(B, case.IN - g.n_levels * g.n_features_per_level, dtype=torch.float64)], 1)
    mats = [torch.from_numpy(m.astype(np.float64)) for m in F.split(case.W, case.IN, case.NH, case.OUTP, p[:case.n_mlp])]
    for m in mats[:-1]:
        rows = ACT[case.act](rows @ m.T)
    return ACT[case.out_act](rows @ mats[-1].T)[:, :case.n_out]


@functools.lru_cache(maxsize=None)
def setup(i, B):
    """(parameters, inputs clear of the cell boundaries, directions or None, q in float64 [B][n_out]) of case i, once"""
    import torch
    case, K, _ = CASES[i]
    g = grid_of(case)
    table = None if g is None else np.random.default_rng(7).uniform(-1, 1, g.n_params).astype(np.float32)
    p = F.case_params(case, table)
    x = F.case_inputs(case, B)[0]
    if g is not None:
        ok = V.clear_of_boundaries(g, x)
        assert ok.mean() >= 0.75, (case.id, "the boundary filter rejects", 1 - ok.mean())
        x = x[ok]
    x = np.ascontiguousarray(x[:B])
    v = None if K is None else V.directions(x, K)
    xt = torch.from_numpy(x.astype(np.float64)).requires_grad_(True)
    vt = torch.eye(case.n_in, dtype=torch.float64).expand(B, -1, -1) if v is None else torch.from_numpy(v.astype(np.float64))
    y, q = f64(torch, case, g, p, xt), np.zeros((B, case.n_out))
    for o in range(case.n_out):
        g1 = torch.autograd.grad(y[:, o].sum(), xt, create_graph=True)[0]
        for k in range(vt.shape[1] if g1.requires_grad else 0):  # a function linear in x has a constant gradient
            q[:, o] += (torch.autograd.grad((g1 * vt[:, k]).sum(), xt, retain_graph=True)[0] * vt[:, k]).sum(1).numpy()
    return p, x, v, q


def call2(torch, net, case, x, p, v=None, mask=0):
    """(y, Jv, q [B][n_out]) of one call under a layout mask; q's buffer is exactly its size plus a guard"""
    B, D, n = x.shape[0], case.n_in, case.n_out
    K = D if v is None else v.shape[1]
    xd = torch.from_numpy(np.ascontiguousarray(x.T if mask & 1 else x)).cuda()
    vd = None if v is None else torch.from_numpy(np.ascontiguousarray(v.transpose(1, 2, 0) if mask & 1 else v)).cuda()
    pd = torch.from_numpy(p).cuda()
    y = torch.zeros(n * B if mask & 2 else B * case.OUTP, dtype=torch.float32, device="cuda")
    J = torch.zeros(B * n * K, dtype=torch.float32, device="cuda")
    q = torch.full((B * n + V.GUARD,), V.SENTINEL, dtype=torch.float32, device="cuda")
    net.L.check(net.lib.tcnn_module_inference_jvp_second(net.h, None, B, _vp(xd), _vp(vd), 0 if v is None else K, _vp(y), _vp(J), _vp(q),
                                                         _vp(pd), mask))
    torch.cuda.synchronize()
    y, J, q = y.cpu().numpy(), J.cpu().numpy(), q.cpu().numpy()
    assert np.all(q[B * n:] == V.SENTINEL) and not np.any(q[:B * n] == V.SENTINEL), "q written past its size, or not everywhere"
    if mask & 2:
        return y.reshape(n, B).T.copy(), J.reshape(n, K, B).transpose(2, 0, 1).copy(), q[:B * n].reshape(n, B).T.copy()
    return y.reshape(B, case.OUTP), J.reshape(B, n, K), q[:B * n].reshape(B, n)


@pytest.mark.parametrize("B", [128, 384])
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_against_float64(torch_mod, i, B):
    case, _, tol = CASES[i]
    p, x, v, qt = setup(i, B)
    net = make(torch_mod, i)
    assert net.lib.tcnn_module_engine(net.h) == b"fused" and net.n_params == p.size
    y, Jv, q = call2(torch_mod, net, case, x, p, v)
    y0, Jv0 = V.call(torch_mod, net, case, x, p, v)
    net.close()
    np.testing.assert_array_equal(y.view(np.uint32), y0.view(np.uint32))
    np.testing.assert_array_equal(Jv.view(np.uint32), Jv0.view(np.uint32))
    if tol == 0.0:
        assert np.all(q == 0) and np.all(qt == 0) and np.abs(Jv).max() > 0
        return
    ratio = np.abs(q.astype(np.float64) - qt).max() / np.abs(qt).max()
    print(f"jvp2-ratio {case.id} B={B} max|q - q64| / max|q64| = {ratio:.3e} (max|q64| = {np.abs(qt).max():.3e})")
    assert np.abs(qt).max() > 0 and ratio <= tol, (case.id, ratio)


def test_soa_is_aos_transposed(torch_mod):
    case = CASES[3][0]
    p, x, v, _ = setup(3, 128)
    net = make(torch_mod, 3)
    y0, J0, q0 = call2(torch_mod, net, case, x, p, v)
    for mask in (1, 2, 3):
        y, J, q = call2(torch_mod, net, case, x, p, v, mask)
        for name, a, b in (("y", y, y0[:, :y.shape[1]]), ("Jv", J, J0), ("q", q, q0)):
            np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32), err_msg=f"{name}, mask {mask}")
    net.close()


def test_torch_front_end(torch_mod):
    torch = torch_mod
    import tinycudann as tcnn
    case, B = CASES[2][0], 200
    m = tcnn.NetworkWithInputEncoding(2, 3, case.enc, case.net, dtype=torch.float32)
    x = torch.rand(B, 2, device="cuda")
    v = torch.rand(B, 2, 2, device="cuda")
    y, J, lap = m.value_jacobian_and_laplacian(x)
    y2, Jv, q = m.value_jvp_and_second(x, v)
    _, Jv1, q1 = m.value_jvp_and_second(x, v[:, 0])
    ys, Js, ls = m.value_jvp_and_second(x.T.contiguous(), layout="soa")
    assert lap.shape == (B, 3) and q.shape == (B, 3) and Jv1.shape == (B, 3) and ls.shape == (3, B)
    assert not any(t.requires_grad for t in (y, J, lap, y2, Jv, q))
    y0, J0 = m.value_and_jacobian(x)
    y3, Jv0 = m.value_and_jvp(x, v)
    assert torch.equal(y, y0) and torch.equal(J, J0) and torch.equal(y2, y3) and torch.equal(Jv, Jv0)
    assert torch.equal(Jv1, m.value_and_jvp(x, v[:, 0])[1]) and torch.equal(ls, lap.T) and torch.equal(Js, J.permute(1, 2, 0))
    assert lap.abs().max() > 0 and q1.abs().max() > 0


@pytest.mark.parametrize("what", ["fp16", "oneblob", "w128"])
def test_refusals(torch_mod, what):
    torch = torch_mod
    enc, W = (F.ONEBLOB4 if what == "oneblob" else V.HASH3_L16), (128 if what == "w128" else 64)
    m = T.Net(torch, 3, 1, V.gc("refuse", W, 2, 3, 1, "Softplus", "None", None).net, enc, FP16 if what == "fp16" else FP32)
    p = m.initial_params(3)
    xd, pd = torch.rand(256, 3, device="cuda"), m._dev(p if m.f32 else p.astype(np.float16).view(np.uint16))
    y, J, q = (torch.zeros(256 * n, dtype=torch.float32, device="cuda") for n in (16, 3, 1))
    name = m.lib.tcnn_module_name(m.h).decode()
    front, why = {"fp16": ("", ""), "oneblob": (" behind OneBlobEncoding", ""),
                  "w128": (" behind GridEncoding", r": a width of 128 \(16, 32 and 64 are served\)")}[what]
    message = (rf"^{name}{front}: inference_jvp_second is not implemented by the MI355X engine yet \(fp32 FullyFusedMLP network modules "
               rf"alone, behind a lone Identity encoding or behind a lone grid encoding only\){why}$")
    with pytest.raises(m.L.TcnnError, match=message):
        m.L.check(m.lib.tcnn_module_inference_jvp_second(m.h, None, 256, _vp(xd), None, 0, _vp(y), _vp(J), _vp(q), _vp(pd), 0))
    if what == "w128":  # the first-order call serves the module
        m.L.check(m.lib.tcnn_module_inference_jvp(m.h, None, 256, _vp(xd), None, 0, _vp(y), _vp(J), _vp(pd), 0))
        torch.cuda.synchronize()
    m.close()
