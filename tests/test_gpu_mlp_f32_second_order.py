"""GPU tests of the second-order input gradient of fp32 network modules through the C-ABI
(tcnn_module_backward_backward_input on a module created with TCNN_PRECISION_FP32): csrc/mlp_f32.hip's tangent and
curvature kernels under NetworkF32Host::backward_backward_input, against the float64 truth and the per-element
bounds of tests/mlp_f32_second_order_reference.py (derived there from the operation count; its CPU test is their
proof). Every output buffer is pre-filled with NaN: what is asked for must be written whole."""
import numpy as np
import pytest

import mlp_f32_reference as F
import mlp_f32_second_order_reference as S
import test_grid_f32_reference as G
from helpers import rel_err
from oracle import oracle as O
from test_gpu_encoding_f32 import _vp
from test_gpu_mlp_f32 import Net, encoded_rows, make_net

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


def bbi(net, u_x, dout, want=("params", "ddout", "dx"), x=None, p=None, expect_fail=False):
    """tcnn_module_backward_backward_input on net's last forward: {"params", "ddout", "dx"} -> arrays (NaN pre-filled).
    dout None: a NULL dL_doutput. x / p: device tensors passed instead of the forward's (a foreign context)."""
    torch = net.torch
    n = net.x.shape[0]
    g_d = torch.from_numpy(np.ascontiguousarray(u_x, np.float32)).cuda()
    d = None if dout is None else torch.from_numpy(np.ascontiguousarray(dout, np.float32)).cuda()
    nan = float("nan")
    bufs = {"params": torch.full((net.n_params,), nan, dtype=torch.float32, device="cuda") if "params" in want else None,
            "ddout": torch.full((n, net.width), nan, dtype=torch.float32, device="cuda") if "ddout" in want else None,
            "dx": torch.full((n, net.n_in), nan, dtype=torch.float32, device="cuda") if "dx" in want else None}
    rc = net.lib.tcnn_module_backward_backward_input(net.h, None, net.ctx, n, _vp(g_d), _vp(net.x if x is None else x), _vp(d),
                                                     _vp(bufs["params"]), _vp(bufs["ddout"]), _vp(bufs["dx"]), _vp(net.p if p is None else p))
    torch.cuda.synchronize()
    if expect_fail:
        assert rc != 0
        return net.lib.tcnn_last_error().decode()
    net.L.check(rc)
    return {k: v.cpu().numpy() for k, v in bufs.items() if v is not None}


_SETUPS = {}


def setup(case, B):
    """the float64 reference of a case, computed once and shared (never modified)"""
    if (case.id, B) not in _SETUPS:
        _SETUPS[(case.id, B)] = S.setup_identity(case, B)
    return _SETUPS[(case.id, B)]


@pytest.mark.parametrize("B", S.BATCHES)
@pytest.mark.parametrize("case", S.CASES, ids=[c.id for c in S.CASES])
def test_network_alone_against_float64(torch_mod, case, B):
    """dL2/d(dL/dy), every matrix's dL2/dparams and dL2/dinput per element within the derived bounds. ReLU / LeakyReLU:
    on the rows clear_of_branches keeps (setup fails if fewer than B of the 2 B candidates stay); without curvature
    dL2/dinput is written as zeros."""
    x, rows, dout, u_x, p, ref = setup(case, B)
    net = make_net(torch_mod, case)
    assert net.n_params == p.size == case.n_mlp
    net.forward(x, p)
    got = bbi(net, u_x, dout)
    net.close()
    ratios = S.check(ref, got["ddout"], got["params"], case.NH, case.id)
    want_dx, e_dx = S.identity_dinput(ref, case.n_in)
    ratios["dinput"] = S.check_one("dinput", got["dx"], want_dx, e_dx, case.id)
    if ref["top"] < 0:
        assert not got["dx"].any() and not np.isnan(got["dx"]).any()
    else:
        assert np.abs(got["dx"]).max() > 0
    print(case.id, B, ratios)


def _softplus():
    return next(c for c in S.CASES if c.name == "w64in32h2" and c.act == "Softplus")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_power_of_two_scaling(torch_mod):
    """Every pass is linear in u_x and in dL/dy, and fp32 arithmetic commutes with a power of two away from underflow
    (inputs are O(1), the factor 2^-20 leaves every value above 2^-60): u_x * 2^-20 gives 2^-20 times every output bit
    for bit; dL/dy * 2^-20 the same for dL2/dparams and dL2/dinput and leaves dL2/d(dL/dy) unchanged."""
    case = _softplus()
    x, rows, dout, u_x, p, ref = setup(case, 256)
    s = np.float32(2.0 ** -20)
    net = make_net(torch_mod, case)
    net.forward(x, p)
    base = bbi(net, u_x, dout)
    a = bbi(net, u_x * s, dout)
    b = bbi(net, u_x, dout * s)
    net.close()
    for k in ("params", "ddout", "dx"):
        assert np.abs(base[k]).max() > 0
        np.testing.assert_array_equal(_bits(a[k]), _bits(base[k] * s), err_msg="u_x scaled: " + k)
    for k in ("params", "dx"):
        np.testing.assert_array_equal(_bits(b[k]), _bits(base[k] * s), err_msg="dL/dy scaled: " + k)
    np.testing.assert_array_equal(_bits(b["ddout"]), _bits(base["ddout"]))


def test_two_calls_give_equal_bits(torch_mod):
    """the Network alone at B = 768 (three slabs per term, six per sum): no atomics anywhere"""
    case = _softplus()
    x, rows, dout, u_x, p, ref = setup(case, 768)
    net = make_net(torch_mod, case)
    net.forward(x, p)
    a, b = bbi(net, u_x, dout), bbi(net, u_x, dout)
    net.close()
    for k in a:
        np.testing.assert_array_equal(_bits(a[k]), _bits(b[k]), err_msg=k)


def test_null_outputs(torch_mod):
    """all three outputs NULL: no work, no error. Each output alone, and the tangent pass with a NULL dL/dy, give the
    full call's bits. dL/dy NULL with dL_dparams or dL_dinput asked for is refused with a clear message."""
    case = _softplus()
    x, rows, dout, u_x, p, ref = setup(case, 256)
    net = make_net(torch_mod, case)
    net.forward(x, p)
    full = bbi(net, u_x, dout)
    assert bbi(net, u_x, dout, want=()) == {}
    assert bbi(net, u_x, None, want=()) == {}
    for k in ("params", "ddout", "dx"):
        np.testing.assert_array_equal(_bits(bbi(net, u_x, dout, want=(k,))[k]), _bits(full[k]), err_msg=k)
    np.testing.assert_array_equal(_bits(bbi(net, u_x, None, want=("ddout",))["ddout"]), _bits(full["ddout"]))
    for want in (("params",), ("dx",), ("params", "ddout", "dx")):
        msg = bbi(net, u_x, None, want=want, expect_fail=True)
        assert "dL_doutput may be null only when dL_dparams and dL_dinput are" in msg, msg
    net.close()


def test_foreign_context_recomputes(torch_mod):
    """a context whose forward saw other input / parameter pointers: the forward is recomputed from the pointers of
    this call, the same bits come out"""
    case = _softplus()
    x, rows, dout, u_x, p, ref = setup(case, 256)
    net = make_net(torch_mod, case)
    net.forward(x, p)
    full = bbi(net, u_x, dout)
    x2, p2 = net.x.clone(), net.p.clone()
    assert x2.data_ptr() != net.x.data_ptr() and p2.data_ptr() != net.p.data_ptr()
    for kw in (dict(x=x2), dict(p=p2), dict(x=x2, p=p2)):
        other = bbi(net, u_x, dout, **kw)
        for k in full:
            np.testing.assert_array_equal(_bits(other[k]), _bits(full[k]), err_msg=k)
    net.close()


# ---- a grid in front ----
GRID = {"otype": "HashGrid", "n_levels": 4, "n_features_per_level": 2, "log2_hashmap_size": 10, "base_resolution": 8, "per_level_scale": 1.5}


def _split16(v):
    """v [B][LF] float64 as two fp16-representable pieces, v = (a + b 2^-12) sc up to 2^-22 |v|: what lets the
    fp16 oracle evaluate a map that is linear in v"""
    sc = 2.0 ** np.ceil(np.log2(max(np.abs(v).max(), 1e-30)))
    a16 = O.f2h((v / sc).astype(np.float32))
    b16 = O.f2h(((v / sc - O.h2f(a16).astype(np.float64)) * 2.0 ** 12).astype(np.float32))
    return sc, np.ascontiguousarray(a16.T), np.ascontiguousarray(b16.T)


def _linear(fn, v):
    sc, a, b = _split16(v)
    return (fn(a).astype(np.float64) + fn(b).astype(np.float64) * 2.0 ** -12) * sc


def _per_point_abs_jacobian(fn, B, LF, D):
    """|J| [B][D][LF] of a map dx[b] = J[b] dy[b] that is linear and independent per point: one-hot columns"""
    J = np.zeros((B, D, LF))
    for f in range(LF):
        dy = np.zeros((LF, B), np.float32)
        dy[f] = 1.0
        J[:, :, f] = np.abs(fn(O.f2h(dy)).astype(np.float64))
    return J


def _per_point_abs_jacobian_u(fn, B, D, width):
    """the same for a map that is linear in u_x [B][D]: |J| [B][width][D]"""
    J = np.zeros((B, width, D))
    for d in range(D):
        u = np.zeros((B, D), np.float32)
        u[:, d] = 1.0
        J[:, :, d] = np.abs(fn(u).astype(np.float64))
    return J


def grid_truth(case, g, x, t16, rows, p_mlp, dout, u_x, e_ux=None):
    """The float64 truth of the second-order call with a grid in front, built compositionally, and its tolerances.
    U_0 = the oracle's grid_bwd_bwd dL/d(dL/dy); the float64 MLP passes on the module's own encoded rows; dL2/dx =
    grid_bwd_bwd's dL/dx for dL/dy = D_0 plus grid_bwd_input(P_0); dL2/dtable = grid_bwd_bwd's dL/dgrid for D_0 plus
    grid_bwd(P_0). The oracle reads fp16: D_0 and P_0 go in as two fp16 pieces each (the maps are linear in them;
    residual 2^-22). Tolerances: the grid's parts carry those of tests/test_gpu_grid_second_order.py -- U_0 rtol 2e-3 +
    1e-4 max, which enters the MLP bounds as e_u0 and is propagated through |W| by the reference; dL/dx rtol 1e-4 +
    1e-4 max per grid term, plus the MLP's own e_d0 / e_p0 through the per-point |Jacobians| (one-hot oracle calls);
    dL/dtable relative L2 2e-3 of each term, plus the L2 norm of the first-order gradient of e_p0 (its weights are
    non-negative) and, for e_d0 through the second-order term, sum_b sum_l 2 s_l |u_x[b]|_1 sum_f e_d0[b, l, f]
    (|A_c| <= s_l sum_e |u_x[b, e]| prod_{d != e} w_d, and the weights of the four corners sum to 2 per e in 2-D; an L1
    bound, which dominates the L2 norm). e_ux [B][D]: a bound on the error of u_x itself (a caller that computes it
    from engine outputs); every term above is linear in u_x and carries it the same way.
    Returns dict(ref, dx, tol_dx, table, tol_table (L2), g_a, g_b)."""
    B, D = x.shape
    LF = g.n_levels * g.n_features_per_level
    e_ux = np.zeros((B, D)) if e_ux is None else np.asarray(e_ux, np.float64)
    u_x = np.asarray(u_x, np.float32)
    tangent = lambda u: O.grid_bwd_bwd(g, x, t16, u, None, want_grad=False, want_dx=False)[1]
    u0v = tangent(u_x).astype(np.float64)
    u0 = np.zeros((B, case.IN))
    u0[:, :LF] = u0v
    e_u0 = np.zeros_like(u0)
    e_u0[:, :LF] = 2e-3 * np.abs(u0v) + 1e-4 * np.abs(u0v).max() + np.einsum("bfd,bd->bf", _per_point_abs_jacobian_u(tangent, B, D, LF), e_ux)
    ref = S.reference(case.W, case.IN, case.NH, case.OUTP, case.act, case.out_act, p_mlp, rows, dout, u0, e_u0=e_u0)
    d0, p0 = ref["d0"][:, :LF], ref["p0"][:, :LF]
    e_d0, e_p0 = ref["e_d0"][:, :LF] + 2.0 ** -22 * np.abs(d0), ref["e_p0"][:, :LF] + 2.0 ** -22 * np.abs(p0)
    # dL2/dx
    second = lambda dy: O.grid_bwd_bwd(g, x, t16, u_x, dy, want_grad=False, want_ddLdy=False)[2]
    first = lambda dy: O.grid_bwd_input(g, x, t16, dy)
    dx_a, dx_b = _linear(second, d0), _linear(first, p0)
    J2, J1 = _per_point_abs_jacobian(second, B, LF, D), _per_point_abs_jacobian(first, B, LF, D)
    # (linear in u_x per point for the dL/dy at hand: one-hot u_x gives the Jacobian itself; its product with e_d0 is second order)
    Ju = _per_point_abs_jacobian_u(lambda u: _linear(lambda dy: O.grid_bwd_bwd(g, x, t16, u, dy, want_grad=False, want_ddLdy=False)[2], d0), B, D, D)
    tol_dx = (1e-4 * np.abs(dx_a) + 1e-4 * np.abs(dx_a).max() + 1e-4 * np.abs(dx_b) + 1e-4 * np.abs(dx_b).max()
              + np.einsum("bdf,bf->bd", J2, e_d0) + np.einsum("bdf,bf->bd", J1, e_p0) + np.einsum("bed,bd->be", Ju, e_ux))
    # dL2/dtable: both contributors
    g_a = _linear(lambda dy: O.grid_bwd_bwd(g, x, t16, u_x, dy, want_ddLdy=False, want_dx=False)[0], d0)
    g_b = _linear(lambda dy: O.grid_bwd(g, x, dy), p0)
    # s_l <= base_resolution per_level_scale^l (grid.h's scale is that minus 1)
    scales = np.array([GRID["base_resolution"] * GRID["per_level_scale"] ** l for l in range(g.n_levels)])
    per_level = lambda v: v.reshape(B, g.n_levels, -1).sum(axis=2)
    slack_a = float((2.0 * scales[None, :] * (np.abs(u_x).sum(axis=1)[:, None] * per_level(e_d0)
                                               + e_ux.sum(axis=1)[:, None] * per_level(np.abs(d0) + e_d0))).sum())
    slack_b = float(np.linalg.norm(G.grid_gradient(g, x, e_p0)[0]))
    tol_table = 2e-3 * (np.linalg.norm(g_a) + np.linalg.norm(g_b)) + slack_a + slack_b
    return dict(ref=ref, dx=dx_a + dx_b, tol_dx=tol_dx, table=g_a + g_b, tol_table=tol_table, g_a=g_a, g_b=g_b, dx_a=dx_a, dx_b=dx_b)


def grid_case(n_out=1):
    return F.Case("grid-w64h2", 64, 2, n_in=2, n_out=n_out, act="Softplus", enc=GRID, otype="FullyFusedMLP", scale=1.0)


def test_grid_in_front(torch_mod):
    """NetworkWithInputEncoding fp32 over a small HashGrid (2-D, 4 levels, F 2, 2^10 entries), Softplus W 64 NH 2, the
    table and dL/dy fp16-representable, against grid_truth. The grid's table gradient has two contributors, which
    must add; the network's part of dL2/dparams is bit-reproducible, the grid's (fp32 atomics) is not held to that."""
    torch = torch_mod
    B, D, n_out = 256, 2, 1
    case = grid_case(n_out)
    g = O.grid_cfg(GRID, D)
    rng = np.random.default_rng(17)
    t16 = O.f2h(rng.uniform(-1, 1, g.n_params).astype(np.float32))
    table = O.h2f(t16)
    x = rng.uniform(0, 1, (B, D)).astype(np.float32)
    dout = np.zeros((B, case.OUTP), np.float32)
    dout[:, :n_out] = O.h2f(O.f2h(rng.uniform(-1, 1, (B, n_out)).astype(np.float32)))
    u_x = rng.uniform(-1, 1, (B, D)).astype(np.float32)
    p = F.case_params(case, table)
    rows = encoded_rows(torch, case, x, table)
    t = grid_truth(case, g, x, t16, rows, p[:case.n_mlp], dout, u_x)
    net = make_net(torch, case)
    assert net.n_params == case.n_mlp + g.n_params
    net.forward(x, p)
    got = bbi(net, u_x, dout)
    again = bbi(net, u_x, dout)
    net.close()
    assert not any(np.isnan(v).any() for v in got.values())
    ratios = S.check(t["ref"], got["ddout"], got["params"][:case.n_mlp], case.NH, "grid in front")
    np.testing.assert_array_equal(_bits(again["params"][:case.n_mlp]), _bits(got["params"][:case.n_mlp]))
    np.testing.assert_array_equal(_bits(again["ddout"]), _bits(got["ddout"]))
    ratios["dx"] = S.check_one("dx", got["dx"], t["dx"], t["tol_dx"], "grid in front")
    assert np.abs(t["dx_a"]).max() > 0 and np.abs(t["dx_b"]).max() > 0
    table_grad = got["params"][case.n_mlp:].astype(np.float64)
    err = np.linalg.norm(table_grad - t["table"])
    ratios["table"] = float(err / t["tol_table"])
    assert err <= t["tol_table"], ("table gradient", err, t["tol_table"])
    # each contributor alone would miss: they add, neither overwrites the other
    assert rel_err(table_grad, t["g_a"]) > 2e-2 and rel_err(table_grad, t["g_b"]) > 2e-2
    print("grid in front", ratios)


def test_refusals(torch_mod):
    """an fp32 network over OneBlob or a Composite refuses the call with "not implemented" and names the encoding;
    Sine is refused as today (the forward that would make the context)"""
    torch = torch_mod
    net_cfg = {"otype": "CutlassMLP", "activation": "Softplus", "output_activation": "None", "n_neurons": 16, "n_hidden_layers": 1}
    comp = {"otype": "Composite", "nested": [dict(GRID, n_dims_to_encode=2), {"otype": "OneBlob", "n_bins": 4}]}
    for n_in, enc, name in ((2, F.ONEBLOB4, "OneBlobEncoding"), (3, comp, "CompositeEncoding")):
        m = Net(torch, n_in, 1, net_cfg, enc)
        x = np.full((256, n_in), 0.25, np.float32)
        m.forward(x, m.initial_params(3))
        msg = bbi(m, np.zeros((256, n_in), np.float32), np.zeros((256, m.width), np.float32), expect_fail=True)
        assert "not implemented" in msg and "backward_backward_input" in msg and name in msg, msg
        m.close()
    sine = Net(torch, 16, 16, dict(net_cfg, activation="Sine"))
    xd = torch.zeros(256, 16, device="cuda")
    pd = torch.zeros(sine.n_params, device="cuda")
    od = torch.empty(256, 16, device="cuda")
    assert not sine.lib.tcnn_module_forward(sine.h, None, 256, _vp(xd), _vp(od), _vp(pd), 1)
    assert "Sine has no backward from its forward value" in sine.lib.tcnn_last_error().decode()
    sine.close()
    # the fp16 network module still has none
    m16 = Net(torch, 3, 1, net_cfg, None, precision=1)
    x = np.full((256, 3), 0.25, np.float32)
    m16.forward(x, O.f2h(m16.initial_params(3)))
    z = torch.zeros(256, 16, dtype=torch.float16, device="cuda")
    u = torch.zeros(256, 3, device="cuda")
    rc = m16.lib.tcnn_module_backward_backward_input(m16.h, None, m16.ctx, 256, _vp(u), _vp(m16.x), _vp(z), None, _vp(z), None, _vp(m16.p))
    assert rc != 0 and "not implemented" in m16.lib.tcnn_last_error().decode()
    m16.close()
