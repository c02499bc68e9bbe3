"""GPU tests of tcnn_module_forward_jvp_second / tcnn_module_backward_jvp_second (csrc/mlp_f32_jvp2_train.hip):
dL/dparams of a loss L = sum C_y o y + sum C_J o Jv + sum C_q o q on the value, the directional input derivatives and
q = sum_k v_k^T H v_k of an fp32 FullyFusedMLP network module, against float64.

Truth. The module's function restated in float64 torch on the CPU as test_gpu_mlp_f32_jvp_second.f64 has it, with the
parameters a float64 tensor that requires grad; q from two autograd.grad(create_graph=True) along each v_k, then
autograd.grad(L, p). The cotangents are folded in before the input derivatives are taken (the rows are independent),
so the cost does not grow with the outputs.

Bound. Separately for the network block and the table block, max|g - g64| / max|g64| <= TOL[case][block]: four times
the worst ratio measured on an MI355X over both batches (profiles/mlp_f32_jvp2_train_ratios.txt, which also records
how far each truth moves when C_q is zeroed: more than 100 times the tolerance). Each case's comment names the term
that is of order one when dropped.
"""
import functools

import numpy as np
import pytest

import mlp_f32_reference as F
import test_gpu_mlp_f32 as T
import test_gpu_mlp_f32_jvp as V
import test_gpu_mlp_f32_jvp_second as S
import test_gpu_mlp_f32_jvp_train as TT
import test_grid_f32_reference as G
from test_gpu_encoding_f32 import _vp

pytestmark = pytest.mark.gpu

GUARD, SENTINEL = TT.GUARD, TT.SENTINEL
ACT = dict(S.ACT, Squareplus=lambda z: (10 * z + (100 * z * z + 4).sqrt()) / 20, Exponential=lambda z: z.exp())
CASES = [  # (case, K explicit directions or None for the unit vectors, front, (TOL network, TOL table))
    (S.CASES[1][0], None, None, (4 * 5.611e-7, None)),  # alone-w32h2 Tanh: chi and the psi r Ub term
    (S.CASES[2][0], None, V.DENSE2_F4, (4 * 6.131e-7, 4 * 7.364e-7)),  # the diagonal d^2 w_c term of the table gradient
    (S.CASES[3][0], 3, V.TILED3_F8, (4 * 5.523e-7, 4 * 6.743e-7)),  # mixed d^2 w_c, five rows at W 64, two output tiles, Sigmoid's curvature
    (S.HASH3_W64, None, V.HASH3_L16, (4 * 5.842e-7, 4 * 3.612e-7)),  # the Laplacian behind a hash grid, two levels per lane
    (S.CASES[0][0], None, S.IDENTITY, (4 * 6.001e-7, None)),  # identity-w16h1 None: q = 0, C_q contributes exactly nothing
    (V.gc("alone-w16h1", 16, 1, 3, 1, "Squareplus", "None", None), None, None, (4 * 7.074e-7, None)),  # Squareplus' chi
    (V.gc("alone-w16h1", 16, 1, 3, 1, "Exponential", "None", None), None, None, (4 * 1.327e-6, None)),  # Exponential's chi
]
IDS = [c[0].id for c in CASES]
I_ALONE, I_DENSE2, I_HASH, I_IDENTITY = 0, 1, 3, 4


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


def make(torch, i):
    case, _, front, _ = CASES[i]
    return T.Net(torch, case.n_in, case.n_out, case.net, front)


@functools.lru_cache(maxsize=None)
def setup(i, B):
    """(grid config or None, parameters, exactly B inputs clear of the cell boundaries, directions or None) of case i"""
    case, K, _, _ = CASES[i]
    g = S.grid_of(case)
    table = None if g is None else np.random.default_rng(7).uniform(-1, 1, g.n_params).astype(np.float32)
    p = F.case_params(case, table)
    x = F.case_inputs(case, B)[0]
    if g is not None:
        ok = V.clear_of_boundaries(g, x)
        assert ok.mean() >= 0.75, (case.id, "the boundary filter rejects", 1 - ok.mean())
        x = x[ok]
    x = np.ascontiguousarray(x[:B])
    assert x.shape[0] == B, (case.id, x.shape)
    return g, p, x, (None if K is None else V.directions(x, K))


def cotangents(case, B, K):
    Cy, CJ = TT.cotangents(case, B, K)
    return Cy, CJ, np.random.default_rng(13).uniform(-1, 1, (B, case.n_out)).astype(np.float32)


def f64(torch, case, g, p, x):
    """S.f64 with the parameters p a float64 tensor: y [B][n_out] from x (float64, requires grad)"""
    B, D = x.shape
    if g is None:
        rows = torch.cat([x, torch.ones(B, case.IN - D, dtype=torch.float64)], 1)
    else:
        xh = x.detach().numpy().astype(np.float32)
        table, cols = p[case.n_mlp:].reshape(-1, g.n_features_per_level), []
        for l in range(g.n_levels):
            idx = torch.from_numpy(G.level_corners(g, l, xh)[0])
            f = torch.from_numpy(V.fractions(g, l, xh)) + (x - x.detach()) * float(np.float32(g.scales[l]))
            s = f * f * (3 - 2 * f) if g.interpolation == 2 else f
            w = [torch.stack([s[:, d] if c >> d & 1 else 1 - s[:, d] for d in range(D)]).prod(0) for c in range(1 << D)]
            cols.append(sum(w[c][:, None] * table[idx[:, c]] for c in range(1 << D)))
        rows = torch.cat(cols + [torch.zeros(B, case.IN - g.n_levels * g.n_features_per_level, dtype=torch.float64)], 1)
    off = 0
    for j, (r, c) in enumerate(F.shapes(case.W, case.IN, case.NH, case.OUTP)):
        rows = ACT[case.act if j < case.NH else case.out_act](rows @ p[off:off + r * c].reshape(r, c).T)
        off += r * c
    return rows[:, :case.n_out]


def truth(torch, i, B, Cy, CJ, Cq):
    """dL/dparams in float64 [n_params]; a cotangent None counts as zero"""
    case = CASES[i][0]
    g, p, x, v = setup(i, B)
    grad, t64 = torch.autograd.grad, lambda a: torch.from_numpy(np.asarray(a, np.float64))
    pt, xt = t64(p).requires_grad_(True), t64(x).requires_grad_(True)
    vt = torch.eye(case.n_in, dtype=torch.float64).expand(B, -1, -1) if v is None else t64(v)
    y = f64(torch, case, g, pt, xt)
    L = 0 if Cy is None else (t64(Cy[:, :case.n_out]) * y).sum()
    for k in range(vt.shape[1] if CJ is not None else 0):
        L = L + (grad((t64(CJ[:, :, k]) * y).sum(), xt, create_graph=True)[0] * vt[:, k]).sum()
    if Cq is not None:
        g1 = grad((t64(Cq) * y).sum(), xt, create_graph=True)[0]
        for k in range(vt.shape[1]):
            g2 = grad((g1 * vt[:, k]).sum(), xt, create_graph=True, allow_unused=True)[0]  # None: a function linear in x
            L = L + (0 if g2 is None else (g2 * vt[:, k]).sum())
    return grad(L, pt)[0].numpy()


def run(torch, net, case, x, p, v, Cy, CJ, Cq, vb="same"):
    """forward_jvp_second + backward_jvp_second; (y, Jv, q, dL/dparams), the gradient buffer guarded. vb: the
    backward's directions where they are not the forward's"""
    B, n = x.shape[0], case.n_out
    K = case.n_in if v is None else v.shape[1]
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    xd, vd, pd, cy, cj, cq = dev(x), dev(v), dev(p), dev(Cy), dev(CJ), dev(Cq)
    y, J, q = (torch.empty(B * m, dtype=torch.float32, device="cuda") for m in (case.OUTP, n * K, n))
    grad = torch.full((p.size + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    ctx = net.L.check_ptr(net.lib.tcnn_module_forward_jvp_second(net.h, None, B, _vp(xd), _vp(vd), 0 if v is None else K, _vp(y), _vp(J),
                                                                 _vp(q), _vp(pd)))
    try:
        net.L.check(net.lib.tcnn_module_backward_jvp_second(net.h, None, ctx, B, _vp(cy), _vp(cj), _vp(cq), _vp(grad), _vp(xd),
                                                            _vp(vd if vb == "same" else dev(vb)), _vp(pd)))
        torch.cuda.synchronize()
    finally:
        net.lib.tcnn_context_destroy(ctx)
    grad = grad.cpu().numpy()
    assert np.all(grad[p.size:] == SENTINEL), "written past dL/dparams"
    return y.cpu().numpy().reshape(B, case.OUTP), J.cpu().numpy().reshape(B, n, K), q.cpu().numpy().reshape(B, n), grad[:p.size]


def check(label, i, got, want):
    case, tol = CASES[i][0], CASES[i][3]
    for block, sl, t in (("network", slice(0, case.n_mlp), tol[0]), ("table", slice(case.n_mlp, None), tol[1])):
        if t is None:
            assert got[sl].size == 0
            continue
        ratio = np.abs(got[sl].astype(np.float64) - want[sl]).max() / np.abs(want[sl]).max()
        print(f"jvp2-train-ratio {label} {block} max|g - g64| / max|g64| = {ratio:.3e} (max|g64| = {np.abs(want[sl]).max():.3e})")
        assert np.abs(want[sl]).max() > 0 and ratio <= t, (label, block, ratio)


@pytest.mark.parametrize("B", [256, 768])
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_against_float64(torch_mod, i, B):
    case = CASES[i][0]
    _, p, x, v = setup(i, B)
    Cy, CJ, Cq = cotangents(case, B, case.n_in if v is None else v.shape[1])
    net = make(torch_mod, i)
    y, Jv, q, grad = run(torch_mod, net, case, x, p, v, Cy, CJ, Cq)
    y0, Jv0, q0 = S.call2(torch_mod, net, case, x, p, v)
    if i == I_IDENTITY:  # q = 0 in every layer: C_q meets zeros alone
        assert np.all(q == 0) and np.array_equal(grad, run(torch_mod, net, case, x, p, v, Cy, CJ, None)[3])
    net.close()
    for a, b in ((y, y0), (Jv, Jv0), (q, q0)):
        np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
    check(f"{case.id} B={B}", i, grad, truth(torch_mod, i, B, Cy, CJ, None if i == I_IDENTITY else Cq))


@pytest.mark.parametrize("zero", ["dL_doutput", "dL_djvp", "dL_dsecond"])
@pytest.mark.parametrize("i", [I_ALONE, I_DENSE2], ids=[IDS[I_ALONE], IDS[I_DENSE2]])
def test_cotangents(torch_mod, i, zero):
    case, B = CASES[i][0], 256
    _, p, x, v = setup(i, B)
    C = [None if zero == name else c for name, c in zip(("dL_doutput", "dL_djvp", "dL_dsecond"), cotangents(case, B, case.n_in))]
    net = make(torch_mod, i)
    grad = run(torch_mod, net, case, x, p, v, *C)[3]
    net.close()
    check(f"{case.id} zero={zero}", i, grad, truth(torch_mod, i, B, *C))


def test_network_part_is_bit_reproducible(torch_mod):
    case, B = CASES[I_HASH][0], 768
    _, p, x, v = setup(I_HASH, B)
    C = cotangents(case, B, 3)
    net = make(torch_mod, I_HASH)
    a, b = (run(torch_mod, net, case, x, p, v, *C)[3][:case.n_mlp] for _ in range(2))
    net.close()
    np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))


def test_torch_front_end(torch_mod):
    torch = torch_mod
    import tinycudann as tcnn
    i, B = I_DENSE2, 256
    case = CASES[i][0]
    _, p, x, _ = setup(i, B)
    m = tcnn.NetworkWithInputEncoding(2, 3, case.enc, case.net, dtype=torch.float32)
    with torch.no_grad():
        m.params.copy_(torch.from_numpy(p))
    xd = torch.from_numpy(x).cuda()
    f = torch.from_numpy(cotangents(case, B, 2)[2]).cuda()
    y, J, lap = m.value_jacobian_and_laplacian(xd, differentiable=True)
    assert all(t.requires_grad for t in (y, J, lap)) and lap.shape == (B, 3)
    for a, b in zip((y, J, lap), m.value_jacobian_and_laplacian(xd)):
        assert not b.requires_grad and torch.equal(a.detach(), b)
    (((lap - f) ** 2).mean() + y.mean()).backward()
    Cy = np.zeros((B, case.OUTP), np.float32)
    Cy[:, :3] = 1.0 / (3 * B)
    Cq = (2 * (lap.detach() - f) / (3 * B)).cpu().numpy()
    check("torch poisson", i, m.params.grad.cpu().numpy(), truth(torch, i, B, Cy, None, Cq))
    with pytest.raises(ValueError, match="layout='aos' only"):
        m.value_jacobian_and_laplacian(xd.T.contiguous(), layout="soa", differentiable=True)
    with pytest.raises(ValueError, match="must not require grad"):
        m.value_jacobian_and_laplacian(xd.clone().requires_grad_(True), differentiable=True)
    lap = m.value_jacobian_and_laplacian(xd, differentiable=True)[2]
    with pytest.raises(ValueError, match="double backward"):
        torch.autograd.grad(lap.sum(), m.params, create_graph=True)


REFUSED = {  # what: (case, front, batch, K, what the message names)
    "w128": (V.CASES[3], V.HASH3_L16, 256, 3, r": a width of 128 \(16, 32 and 64 are served\)"),
    "k4": (S.HASH3_W64, V.HASH3_L16, 256, 4, r": 4 directions at width 64 \(at most 3 are served"),
    "b128": (S.HASH3_W64, V.HASH3_L16, 128, 3, r": a batch of 128 \(a multiple of 256 is served\)"),
    "max_level": (S.HASH3_W64, V.HASH3_L16, 256, 3, ": a grid with max_level or stochastic interpolation in effect"),
    "mismatch": (S.HASH3_W64, V.HASH3_L16, 256, 2, ": the forward ran 2 directions and the backward was given none"),
}


@pytest.mark.parametrize("what", list(REFUSED))
def test_refusals(torch_mod, what):
    torch = torch_mod
    case, front, B, K, why = REFUSED[what]
    net = T.Net(torch, case.n_in, case.n_out, case.net, front)
    p = net.initial_params(3)
    x = np.random.default_rng(5).uniform(0, 1, (256, 3)).astype(np.float32)
    v = V.directions(x, K)
    if what == "max_level":
        net.L.check(net.lib.tcnn_module_set_max_level(net.h, 0.5))
    message = (r"^NetworkWithInputEncoding behind GridEncoding: forward_jvp_second / backward_jvp_second are not implemented by the MI355X "
               r"engine yet \(.*\)" + why)
    with pytest.raises(net.L.TcnnError, match=message):
        if what == "mismatch":
            run(torch, net, case, x, p, v, *cotangents(case, 256, K), vb=None)
        else:
            xd, vd, pd = (torch.from_numpy(a).cuda() for a in (x, v, p))
            y, J, q = (torch.zeros(256 * m, device="cuda") for m in (case.OUTP, case.n_out * K, case.n_out))
            net.L.check_ptr(net.lib.tcnn_module_forward_jvp_second(net.h, None, B, _vp(xd), _vp(vd), K, _vp(y), _vp(J), _vp(q), _vp(pd)))
    if what == "max_level":
        net.L.check(net.lib.tcnn_module_set_max_level(net.h, 1000.0))
    assert np.isfinite(net.inference(x, p)).all()
    net.close()
