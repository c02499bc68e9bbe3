"""GPU tests of the second-order input gradient of fp32 network modules through the torch front end, on both autograd
nodes (the C++ node of csrc/torch_ext.cpp and the Python node of tinycudann/modules.py): the eikonal step

    gx = autograd.grad(y.sum(), x, create_graph=True);  loss = (y w).sum() + ((gx.norm(dim=-1) - 1)^2).mean()

with one backward() of the loss, against the float64 truth and the bounds of tests/mlp_f32_second_order_reference.py.

What the step computes, in the engine's terms: params.grad = first-order dL/dparams for dL/dy = w, plus the
second-order dL2/dparams for dL/dy = 1 and u_x = d loss / d gx = (2 / B)(1 - 1 / |gx|) gx; x.grad likewise. u_x is
itself computed (torch fp32 arithmetic on the engine's gx), so it carries a bound of its own: with e_g the bound of gx
(rule (4), tests/mlp_f32_reference.py), |du| <= (2 / B)(1 + 1 / |gx|) |dg|_1 per row (d/dg of g - g / |g| is I - (I - n n^T) /
|g|, of norm <= 1 + 1 / |g|) plus 16 roundings of the elementwise formula on magnitudes (2 / B)(|gx| + 1). torch adds the
two gradients in fp32: one more rounding of their magnitudes."""
import numpy as np
import pytest

import mlp_f32_reference as F
import mlp_f32_second_order_reference as S
from oracle import oracle as O
from test_gpu_mlp_f32 import encoded_rows
from test_gpu_mlp_f32_second_order import GRID, grid_case, grid_truth

pytestmark = pytest.mark.gpu

U = S.U
NET = {"otype": "FullyFusedMLP", "activation": "Softplus", "output_activation": "None", "n_neurons": 64, "n_hidden_layers": 2}


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(params=["cpp", "python"])
def node(request, monkeypatch, torch_mod):
    from tinycudann import modules
    if request.param == "python":
        monkeypatch.setattr(modules, "_EXT", None)
    elif modules._EXT is None:
        pytest.fail("the C++ autograd node (lib/_tcnn_torch) is not built")
    return request.param


def eikonal_step(torch, model, x_np, w_np):
    """(y, gx, params.grad, x.grad) of one eikonal step, numpy"""
    model.params.grad = None
    x = torch.from_numpy(x_np).cuda().requires_grad_(True)
    w = torch.from_numpy(w_np).cuda()
    y = model(x)
    gx = torch.autograd.grad(y.sum(), x, create_graph=True)[0]
    loss = (y * w).sum() + ((gx.norm(dim=-1) - 1) ** 2).mean()
    loss.backward()
    torch.cuda.synchronize()
    assert y.dtype == torch.float32 and model.params.grad.dtype == torch.float32 and x.grad.dtype == torch.float32
    return y.detach().cpu().numpy(), gx.detach().cpu().numpy(), model.params.grad.cpu().numpy().copy(), x.grad.cpu().numpy().copy()


def eikonal_u(gx, e_g, B):
    """u_x = d loss / d gx in float64 and its bound (module docstring)"""
    n = np.linalg.norm(gx, axis=1, keepdims=True)
    u = (2.0 / B) * (1.0 - 1.0 / n) * gx
    e = (2.0 / B) * (1.0 + 1.0 / n) * e_g.sum(axis=1, keepdims=True) + 16 * U * (2.0 / B) * (np.abs(gx) + 1.0)
    return u, e * np.ones_like(gx)


def _douts(B, OUTP, w):
    ones = np.zeros((B, OUTP), np.float32)
    ones[:, :w.shape[1]] = 1.0
    dw = np.zeros((B, OUTP), np.float32)
    dw[:, :w.shape[1]] = w
    return ones, dw


def _check(name, got, want, bound):
    return S.check_one(name, got, want, bound, "eikonal")


def network_truth(case, p, x, w):
    """the float64 truth of the eikonal step on a Network alone: (params.grad, its bound, x.grad, its bound)"""
    B = x.shape[0]
    rows = F.identity_rows(case, x)
    ones, dw = _douts(B, case.OUTP, w)
    data = F.reference(case.W, case.IN, case.NH, case.OUTP, case.act, case.out_act, p, rows, dw)
    grad = F.reference(case.W, case.IN, case.NH, case.OUTP, case.act, case.out_act, p, rows, ones)
    gx, e_g = grad["dinput"][:, :case.n_in], grad["e_in"][:, :case.n_in]
    u_x, e_ux = eikonal_u(gx, e_g, B)
    u0 = S.identity_u0(u_x, case.IN)
    e_u0 = np.zeros_like(u0)
    e_u0[:, :case.n_in] = e_ux + U * np.abs(u_x)
    sec = S.reference(case.W, case.IN, case.NH, case.OUTP, case.act, case.out_act, p, rows, ones, u0, e_u0=e_u0)
    g1 = np.concatenate([v.ravel() for v in data["wgrad"]])
    g2 = np.concatenate([v.ravel() for v in sec["wgrad"]])
    e1 = np.concatenate([v.ravel() for v in data["e_w"]])
    e2 = np.concatenate([v.ravel() for v in sec["e_w"]])
    dx2, e_dx2 = S.identity_dinput(sec, case.n_in)
    dx1, e_dx1 = data["dinput"][:, :case.n_in], data["e_in"][:, :case.n_in]
    return (g1 + g2, e1 + e2 + U * (np.abs(g1) + e1 + np.abs(g2) + e2), dx1 + dx2,
            e_dx1 + e_dx2 + U * (np.abs(dx1) + e_dx1 + np.abs(dx2) + e_dx2), gx, e_g)


def _network(torch, tcnn):
    model = tcnn.Network(3, 1, NET, dtype=torch.float32)
    case = F.Case("eikonal", 64, 2, n_in=3, n_out=1, act="Softplus", otype="FullyFusedMLP")
    assert model.params.numel() == case.n_mlp
    return model, case


def test_eikonal_step_network(torch_mod, node):
    torch = torch_mod
    import tinycudann as tcnn
    model, case = _network(torch, tcnn)
    p = model.params.detach().cpu().numpy()
    rng = np.random.default_rng(23)
    B = 256
    x = rng.uniform(-1, 1, (B, 3)).astype(np.float32)
    w = rng.uniform(-1, 1, (B, 1)).astype(np.float32)
    y, gx, pg, xg = eikonal_step(torch, model, x, w)
    want_pg, e_pg, want_xg, e_xg, want_gx, e_gx = network_truth(case, p, x, w)
    r = {"gx": _check("gx", gx, want_gx, e_gx), "params.grad": _check("params.grad", pg, want_pg, e_pg), "x.grad": _check("x.grad", xg, want_xg, e_xg)}
    # the second-order part is really there: the data term alone misses
    data_only = np.concatenate([v.ravel() for v in F.reference(case.W, case.IN, case.NH, case.OUTP, case.act, case.out_act, p,
                                                                 F.identity_rows(case, x), _douts(B, case.OUTP, w)[1])["wgrad"]])
    assert np.any(np.abs(pg - data_only) > e_pg)
    print(node, "eikonal network", r)


def test_eikonal_step_grid(torch_mod, node):
    """NetworkWithInputEncoding over the small HashGrid: the truth of tests/test_gpu_mlp_f32_second_order.py's
    grid_truth (tolerances derived there), the first-order parts from the oracle's grid_bwd_input / grid_bwd on the
    float64 dL/d(encoding) with test_gpu_grid_input's rtol = atol = 1e-5 and, for the table, the relative L2 1e-3 of
    test_gpu_encoding_f32's oracle comparison"""
    torch = torch_mod
    import tinycudann as tcnn
    from test_gpu_mlp_f32_second_order import _linear, _per_point_abs_jacobian
    from helpers import rel_err
    D, B = 2, 256
    case = grid_case(1)
    model = tcnn.NetworkWithInputEncoding(D, 1, GRID, NET, dtype=torch.float32)
    g = O.grid_cfg(GRID, D)
    LF = g.n_levels * g.n_features_per_level
    assert model.params.numel() == case.n_mlp + g.n_params
    rng = np.random.default_rng(29)
    t16 = O.f2h(rng.uniform(-1, 1, g.n_params).astype(np.float32))
    with torch.no_grad():
        model.params[case.n_mlp:].copy_(torch.from_numpy(O.h2f(t16)).cuda())
    p = model.params.detach().cpu().numpy()
    x = rng.uniform(0, 1, (B, D)).astype(np.float32)
    w = O.h2f(O.f2h(rng.uniform(-1, 1, (B, 1)).astype(np.float32)))
    y, gx, pg, xg = eikonal_step(torch, model, x, w)
    rows = encoded_rows(torch, case, x, p[case.n_mlp:])
    ones, dw = _douts(B, case.OUTP, w)
    pm = p[:case.n_mlp]
    data = F.reference(case.W, case.IN, case.NH, case.OUTP, case.act, case.out_act, pm, rows, dw)
    grad = F.reference(case.W, case.IN, case.NH, case.OUTP, case.act, case.out_act, pm, rows, ones)
    first = lambda dy: O.grid_bwd_input(g, x, t16, dy)
    J1 = _per_point_abs_jacobian(first, B, LF, D)

    def through_grid(ref):  # (dL/dx, its bound) of a first-order pass
        denc, e = ref["dinput"][:, :LF], ref["e_in"][:, :LF] + 2.0 ** -22 * np.abs(ref["dinput"][:, :LF])
        v = _linear(first, denc)
        return v, 1e-5 * np.abs(v) + 1e-5 + np.einsum("bdf,bf->bd", J1, e)

    want_gx, e_gx = through_grid(grad)
    r = {"gx": _check("gx", gx, want_gx, e_gx)}
    u_x, e_ux = eikonal_u(want_gx, e_gx, B)
    t = grid_truth(case, g, x, t16, rows, pm, ones, u_x.astype(np.float32), e_ux=e_ux + U * np.abs(u_x))
    dx1, e_dx1 = through_grid(data)
    want_xg = dx1 + t["dx"]
    e_xg = e_dx1 + t["tol_dx"] + U * (np.abs(dx1) + e_dx1 + np.abs(t["dx"]) + t["tol_dx"])
    r["x.grad"] = _check("x.grad", xg, want_xg, e_xg)
    g1 = np.concatenate([v.ravel() for v in data["wgrad"]])
    g2 = np.concatenate([v.ravel() for v in t["ref"]["wgrad"]])
    e1 = np.concatenate([v.ravel() for v in data["e_w"]])
    e2 = np.concatenate([v.ravel() for v in t["ref"]["e_w"]])
    r["params.grad"] = _check("params.grad", pg[:case.n_mlp], g1 + g2, e1 + e2 + U * (np.abs(g1) + e1 + np.abs(g2) + e2))
    tab1 = _linear(lambda dy: O.grid_bwd(g, x, dy), data["dinput"][:, :LF])
    import test_grid_f32_reference as G
    slack1 = float(np.linalg.norm(G.grid_gradient(g, x, data["e_in"][:, :LF] + 2.0 ** -22 * np.abs(data["dinput"][:, :LF]))[0]))
    want_tab = tab1 + t["table"]
    err = np.linalg.norm(pg[case.n_mlp:].astype(np.float64) - want_tab)
    bound = 1e-3 * np.linalg.norm(tab1) + slack1 + t["tol_table"] + U * (np.linalg.norm(tab1) + np.linalg.norm(t["table"]))
    r["table"] = float(err / bound)
    assert err <= bound, ("table gradient", err, bound)
    assert rel_err(pg[case.n_mlp:], tab1) > 1e-2  # the second-order terms are there
    print(node, "eikonal grid", r)


def test_module_called_twice_in_one_graph(torch_mod, node):
    """the same module called at B = 256 and B = 512 in one graph, one backward of the summed eikonal losses: the
    gradients are the sums of the two calls' truths (one more fp32 addition per element)"""
    torch = torch_mod
    import tinycudann as tcnn
    model, case = _network(torch, tcnn)
    p = model.params.detach().cpu().numpy()
    rng = np.random.default_rng(31)
    xs = [rng.uniform(-1, 1, (B, 3)).astype(np.float32) for B in (256, 512)]
    ws = [rng.uniform(-1, 1, (B, 1)).astype(np.float32) for B in (256, 512)]
    model.params.grad = None
    xt = [torch.from_numpy(x).cuda().requires_grad_(True) for x in xs]
    loss = 0
    for x, w in zip(xt, ws):
        y = model(x)
        gx = torch.autograd.grad(y.sum(), x, create_graph=True)[0]
        loss = loss + (y * torch.from_numpy(w).cuda()).sum() + ((gx.norm(dim=-1) - 1) ** 2).mean()
    loss.backward()
    torch.cuda.synchronize()
    truths = [network_truth(case, p, x, w) for x, w in zip(xs, ws)]
    want = truths[0][0] + truths[1][0]
    bound = truths[0][1] + truths[1][1] + U * (np.abs(truths[0][0]) + truths[0][1] + np.abs(truths[1][0]) + truths[1][1])
    # torch may add the four gradients (two per call) in any order: two more roundings of the whole magnitude
    bound = bound + 2 * U * (np.abs(truths[0][0]) + np.abs(truths[1][0]) + truths[0][1] + truths[1][1])
    r = {"params.grad": _check("params.grad", model.params.grad.cpu().numpy(), want, bound)}
    for i, (x, t) in enumerate(zip(xt, truths)):
        r["x%d.grad" % i] = _check("x.grad", x.grad.cpu().numpy(), t[2], t[3])
    print(node, "two calls", r)


def test_cpp_and_python_nodes_agree_bit_for_bit(torch_mod, monkeypatch):
    """the Network alone: both nodes make the same engine calls on the same values"""
    torch = torch_mod
    import tinycudann as tcnn
    from tinycudann import modules
    if modules._EXT is None:
        pytest.fail("the C++ autograd node (lib/_tcnn_torch) is not built")
    model, case = _network(torch, tcnn)
    rng = np.random.default_rng(37)
    x = rng.uniform(-1, 1, (256, 3)).astype(np.float32)
    w = rng.uniform(-1, 1, (256, 1)).astype(np.float32)
    a = eikonal_step(torch, model, x, w)
    monkeypatch.setattr(modules, "_EXT", None)
    b = eikonal_step(torch, model, x, w)
    for u, v in zip(a, b):
        np.testing.assert_array_equal(u.view(np.uint32), v.view(np.uint32))
