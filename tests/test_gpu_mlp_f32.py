"""GPU tests of fp32-precision network modules through the C-ABI (tcnn_create_network_precision,
tcnn_create_network_with_input_encoding_precision with TCNN_PRECISION_FP32): csrc/mlp_f32.hip behind the fp32
encoding, against the float64 reference and the bounds of tests/mlp_f32_reference.py (derived there from the
operation count; tests/test_mlp_f32_reference.py is their CPU proof).

The rows the first layer reads are the fp32 ENCODING module's own output for the same inputs (the same
EncodingHost, alignment 16; tests/test_gpu_encoding_f32.py holds it to float64), so the network's bounds start
from exact inputs. dL/dinput is checked where the encoding's backward is a copy (Identity) or linear in dL/dy with a
known Jacobian (OneBlob, against the fp32 encoding module's own backward of the reference dL/d(encoding)); the grid
in front has its dL/dparams checked against tests/test_grid_f32_reference.py instead.
"""
import ctypes
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest

import mlp_f32_reference as F
import module_matrix_cases as M
import test_grid_f32_reference as G
from oracle import oracle as O
from test_gpu_composite import GRID2_L4
from test_gpu_encoding_f32 import FP16, FP32, Mod, _vp

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


class Net(Mod):
    """A network module of either precision through the C-ABI (Mod's forward / backward, numpy in and out).
    ctor "precision": the _precision constructors; "plain": the constructors without one (fp16)."""

    def __init__(self, torch, n_in, n_out, net, enc=None, precision=FP32, ctor="precision"):
        from tinycudann import _lib as L
        self.torch, self.L, self.lib = torch, L, L.lib()
        nj, ej = json.dumps(net).encode(), None if enc is None else json.dumps(enc).encode()
        if ctor == "plain":
            assert precision == FP16
            h = self.lib.tcnn_create_network(n_in, n_out, nj) if enc is None else self.lib.tcnn_create_network_with_input_encoding(n_in, n_out, ej, nj)
        elif enc is None:
            h = self.lib.tcnn_create_network_precision(n_in, n_out, nj, precision)
        else:
            h = self.lib.tcnn_create_network_with_input_encoding_precision(n_in, n_out, ej, nj, precision)
        self.h = L.check_ptr(h)
        self.f32 = precision == FP32
        self.dt = torch.float32 if self.f32 else torch.float16
        self.n_in = n_in
        self.n_params = self.lib.tcnn_module_n_params(self.h)
        self.width = self.lib.tcnn_module_n_output_dims(self.h)
        self.ctx = None

    def inference(self, x, params):
        torch = self.torch
        xd = torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()
        p = self._dev(params)
        out = torch.full((x.shape[0], self.width), float("nan"), dtype=self.dt, device="cuda")
        self.L.check(self.lib.tcnn_module_inference(self.h, None, x.shape[0], _vp(xd), _vp(out), _vp(p)))
        torch.cuda.synchronize()
        return self._host(out)


def make_net(torch, case, precision=FP32, ctor="precision"):
    return Net(torch, case.n_in, case.n_out, case.net, case.enc, precision, ctor)


def encoded_rows(torch, case, x, table=None):
    """the rows the network's first layer reads: the fp32 encoding module's output at alignment 16 (a lone grid
    takes none: its rows, then the zero padding the network's grid writes)"""
    enc = case.enc if case.enc is not None else {"otype": "Identity"}
    lone_grid = case.enc is not None and case.enc["otype"] != "OneBlob"
    m = Mod(torch, case.n_in, enc, FP32, 0 if lone_grid else 16)
    rows = m.forward(x, table)
    m.close()
    if lone_grid:
        rows = np.concatenate([rows, np.zeros((x.shape[0], case.IN - rows.shape[1]), np.float32)], axis=1)
    assert rows.shape[1] == case.IN and not np.isnan(rows).any()
    return np.ascontiguousarray(rows)


def setup(torch, case, B):
    x2, dout = F.case_inputs(case, B)
    g = table = None
    if case.enc is not None and case.enc["otype"] != "OneBlob":
        g = O.grid_cfg(case.enc, case.n_in)
        table = np.random.default_rng(7).uniform(-1, 1, g.n_params).astype(np.float32)
    p = F.case_params(case, table)
    x, rows = F.keep_clear(case, p, x2, encoded_rows(torch, case, x2, table), B)
    ref = F.reference(case.W, case.IN, case.NH, case.OUTP, case.act, case.out_act, p[:case.n_mlp], rows, dout)
    return x, rows, dout, p, ref, g


def run(torch, case, x, dout, p):
    net = make_net(torch, case)
    assert net.n_params == p.size and net.width == case.OUTP
    assert net.lib.tcnn_module_param_precision(net.h) == FP32 and net.lib.tcnn_module_output_precision(net.h) == FP32
    assert net.lib.tcnn_module_n_network_params(net.h) == case.n_mlp
    out = net.forward(x, p)
    dx, grad = net.backward(dout)
    net.close()
    assert not np.isnan(out).any() and not np.isnan(grad).any() and not np.isnan(dx).any()
    return out, dx, grad


@pytest.mark.parametrize("B", F.BATCHES)
@pytest.mark.parametrize("case", F.CASES, ids=[c.id for c in F.CASES])
def test_forward_backward_against_float64(torch_mod, case, B):
    """outputs, every matrix's dL/dparams (per element and per matrix) and dL/dinput within the bounds of
    tests/mlp_f32_reference.py; a grid in front: its dL/dparams within test_grid_f32_reference.gradient_bound
    for the reference dL/d(encoding), plus that gradient's own bound e_in carried through the (linear) sums."""
    if case.enc is not None and case.enc["otype"] != "OneBlob":
        assert case.enc == GRID2_L4
    x, rows, dout, p, ref, g = setup(torch_mod, case, B)
    out, dx, grad = run(torch_mod, case, x, dout, p)
    ratios = F.check(ref, out, grad[:case.n_mlp], None, case.NH, case.id)
    denc, e_in = ref["dinput"], ref["e_in"]
    if case.enc is None:  # Identity, scale 1: dL/dinput is dL/d(encoding)'s first columns
        q = np.abs(dx - denc[:, :case.n_in]) / e_in[:, :case.n_in]
        ratios["dinput"] = float(q.max())
        assert q.max() <= 1.0, (case.id, "dinput", q.max())
    elif case.enc["otype"] == "OneBlob":
        # the fp32 encoding module's backward of float32(reference dL/d(encoding)): the same kernel on inputs that
        # differ by e_in + u |denc| per column; both sides sum n_bins products per input (<= 4 IN roundings in all)
        enc = Mod(torch_mod, case.n_in, case.enc, FP32, 16)
        enc.forward(x)
        want, _ = enc.backward(denc.astype(np.float32))
        enc.close()
        nv = case.n_in * case.enc["n_bins"]
        J = M.oneblob_jacobian(types.SimpleNamespace(enc_cfg=case.enc, IN=nv), x)  # |d enc_j / d x_d| [B][nv][D]
        bound = (np.einsum("bjd,bj->bd", J, e_in[:, :nv] + U * np.abs(denc[:, :nv])) + 4 * case.IN * U * np.einsum("bjd,bj->bd", J, np.abs(denc[:, :nv])) + 1e-35)
        # the Jacobian above is the fp16 oracle's: 2^-10 relative slack for its own rounding
        q = np.abs(dx.astype(np.float64) - want) / (bound * (1 + 2.0 ** -10))
        ratios["dinput"] = float(q.max())
        assert q.max() <= 1.0, (case.id, "dinput", q.max())
    else:
        LF = g.n_levels * g.n_features_per_level
        gref, count, absum, esum, S_level = G.grid_gradient(g, x, denc[:, :LF])
        _, _, absum_hi, _, S_hi = G.grid_gradient(g, x, np.abs(denc[:, :LF]) + e_in[:, :LF])
        tol = G.gradient_bound(g, gref, count, absum_hi, esum, S_hi) + (absum_hi - absum)
        gg = grad[case.n_mlp:].astype(np.float64)
        r = np.abs(gg - gref)[count > 0] / tol[count > 0]
        ratios["grid"] = float(r.max())
        assert r.max() <= 1.0, (case.id, "grid dL/dparams", r.max())
        assert np.all(gg[count == 0] == 0)
    print(case.id, B, ratios)


def _exact_net(torch, n_in=32, n_out=16):
    net = {"otype": "CutlassMLP", "activation": "None", "output_activation": "None", "n_neurons": 16, "n_hidden_layers": 0}
    return Net(torch, n_in, n_out, net)


def test_operand_map_is_exact(torch_mod):
    """One 16 x 32 matrix (two k steps of the MFMA loop), small integers, asymmetric (W[n][k] = 3 n - 5 k + 1):
    identity rows pick its columns exactly; rows holding a distinct power of two per k index of one k step sum to
    an integer < 2^18 in which a dropped or doubled k shows; and with integer dL/dy the backward-data product and
    the weight-gradient sums are exact integers too (all below 2^24)."""
    B, IN, N = 256, 32, 16
    n, k = np.meshgrid(np.arange(N), np.arange(IN), indexing="ij")
    W = (3 * n - 5 * k + 1).astype(np.float32)
    assert not np.array_equal(W[:, :16], W[:, :16].T)
    eye = np.zeros((B, IN), np.float32)
    eye[np.arange(B), np.arange(B) % IN] = 1.0
    pw = np.zeros((B, IN), np.float32)
    for b in range(B):
        blk = (b // 16) % 2
        pw[b, 16 * blk:16 * blk + 16] = 2.0 ** np.arange(16)
    W2 = (1 + (n + k + k // 16) % 2).astype(np.float32)  # 1 or 2, a different pattern per k step
    dy = np.random.default_rng(3).integers(-4, 5, (B, N)).astype(np.float32)
    net = _exact_net(torch_mod)
    for Wm, x in ((W, eye), (W2, pw), (W, pw)):
        out = net.forward(x, Wm.ravel())
        np.testing.assert_array_equal(out, (x.astype(np.float64) @ Wm.astype(np.float64).T).astype(np.float32))
        assert np.all(np.abs(x.astype(np.float64) @ Wm.astype(np.float64).T) < 2 ** 24)
        dx, grad = net.backward(dy)
        np.testing.assert_array_equal(dx, (dy.astype(np.float64) @ Wm.astype(np.float64)).astype(np.float32))
        gw = dy.astype(np.float64).T @ x.astype(np.float64)  # a column's terms share one power of two: exact partial sums
        np.testing.assert_array_equal(grad.reshape(N, IN), gw.astype(np.float32))
    net.close()


def test_wide_range_inputs_and_exponential_outputs(torch_mod):
    """Inputs at 2^-20 (below fp16's smallest subnormal 2^-24 after one product, flushed by an fp16 engine), a
    first matrix at 2^18 and output pre-activations up to 30 under Exponential (exp(30) ~ 1e13, far above fp16's
    65504): output, gradients and dL/dinput within the same bounds."""
    B, W = 256, 16
    rng = np.random.default_rng(5)
    x = (2.0 ** -20 * rng.uniform(0.5, 1.0, (B, 16))).astype(np.float32)
    W0 = (2.0 ** 18 * rng.uniform(0.5, 1.0, (W, 16))).astype(np.float32)
    Wo = rng.uniform(-0.2, 1.0, (16, W)).astype(np.float32)
    h = x.astype(np.float64) @ W0.astype(np.float64).T
    Wo = (Wo * np.float32(30.0 / (h @ Wo.astype(np.float64).T).max())).astype(np.float32)
    z = h @ Wo.astype(np.float64).T
    assert 29.0 < z.max() <= 30.01
    p = np.concatenate([W0.ravel(), Wo.ravel()])
    dout = rng.uniform(-1, 1, (B, 16)).astype(np.float32)
    net_cfg = {"otype": "FullyFusedMLP", "activation": "None", "output_activation": "Exponential", "n_neurons": W, "n_hidden_layers": 1}
    ref = F.reference(W, 16, 1, 16, "None", "Exponential", p, x, dout)
    net = Net(torch_mod, 16, 16, net_cfg)
    out = net.forward(x, p)
    dx, grad = net.backward(dout)
    net.close()
    assert out.max() > 1e12 and np.isfinite(out).all()
    r = F.check(ref, out, grad, dx, 1, "wide-range")
    print("wide range", r)


def test_two_runs_give_equal_bits(torch_mod):
    case = next(c for c in F.CASES if c.name == "w64h3o17" and c.act == "Tanh")
    x, rows, dout, p, ref, g = setup(torch_mod, case, 768)
    a, b = run(torch_mod, case, x, dout, p), run(torch_mod, case, x, dout, p)
    for u, v in zip(a, b):
        np.testing.assert_array_equal(u.view(np.uint32), v.view(np.uint32))


@pytest.mark.parametrize("name", ["w16h1", "oneblob-w32h2"])
def test_fp16_precision_constructors_are_the_existing_modules(torch_mod, name):
    case = next(c for c in F.CASES if c.name == name and c.act == "ReLU")
    x, dout = F.case_inputs(case, 256)
    x = x[:256]
    res = []
    for ctor in ("precision", "plain"):
        net = make_net(torch_mod, case, FP16, ctor)
        assert net.lib.tcnn_module_param_precision(net.h) == FP16
        p16 = O.f2h(net.initial_params(3))
        out = net.forward(x, p16)
        dx, grad = net.backward(O.f2h(dout))
        res.append((p16, out, dx.view(np.uint32), grad, net.lib.tcnn_module_engine(net.h), net.lib.tcnn_module_hyperparams(net.h)))
        net.close()
    for u, v in zip(*res):
        if isinstance(u, bytes):
            assert u == v
        else:
            np.testing.assert_array_equal(u, v)


@pytest.mark.parametrize("name", ["w48h2", "grid-w32h2", "h0"])
def test_initialize_params_matches_fp16(torch_mod, name):
    """the same fp32 values, the same count, hyperparams and name as the fp16 module of the same config"""
    case = next(c for c in F.CASES if c.name == name and c.act == "ReLU")
    a, b = make_net(torch_mod, case, FP32), make_net(torch_mod, case, FP16)
    assert a.n_params == b.n_params and a.width == b.width
    np.testing.assert_array_equal(a.initial_params(11).view(np.uint32), b.initial_params(11).view(np.uint32))
    assert json.loads(a.lib.tcnn_module_hyperparams(a.h)) == json.loads(b.lib.tcnn_module_hyperparams(b.h))
    assert a.lib.tcnn_module_name(a.h) == b.lib.tcnn_module_name(b.h)
    assert abs(a.lib.tcnn_default_loss_scale(FP32) - 1.0) == 0
    a.close()
    b.close()


def test_refusals(torch_mod):
    from tinycudann import _lib as L
    lib = L.lib()
    net = {"otype": "CutlassMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": 16, "n_hidden_layers": 1}
    assert not lib.tcnn_create_network_precision(3, 1, json.dumps(net).encode(), 7)
    assert "create_network: precision must be Fp16 or Fp32" in lib.tcnn_last_error().decode()
    assert not lib.tcnn_create_network_with_input_encoding_precision(2, 1, json.dumps(F.ONEBLOB4).encode(), json.dumps(net).encode(), -1)
    assert "precision must be Fp16 or Fp32" in lib.tcnn_last_error().decode()
    ff48 = dict(net, otype="FullyFusedMLP", n_neurons=48)
    assert not lib.tcnn_create_network_precision(3, 1, json.dumps(ff48).encode(), FP32)
    assert "FullyFusedMLP only supports 16, 32, 64, and 128 neurons, but got 48" in lib.tcnn_last_error().decode()
    # Sine: inference runs, a forward that keeps a context is refused
    sine = dict(net, activation="Sine")
    m = Net(torch_mod, 16, 16, sine)
    x = np.random.default_rng(1).uniform(-1, 1, (256, 16)).astype(np.float32)
    p = m.initial_params(5)
    out = m.inference(x, p).astype(np.float64)
    W0, Wo = p[:256].reshape(16, 16).astype(np.float64), p[256:].reshape(16, 16).astype(np.float64)
    np.testing.assert_allclose(out, np.sin(x @ W0.T) @ Wo.T, rtol=0, atol=1e-5)
    xd, pd = torch_mod.from_numpy(x).cuda(), torch_mod.from_numpy(p).cuda()
    od = torch_mod.empty((256, 16), dtype=torch_mod.float32, device="cuda")
    assert not lib.tcnn_module_forward(m.h, None, 256, _vp(xd), _vp(od), _vp(pd), 0)
    assert "Sine has no backward from its forward value" in lib.tcnn_last_error().decode()
    # as on the fp16 module: no grid, no max_level; no second order
    assert lib.tcnn_module_set_max_level(m.h, ctypes.c_float(0.5)) != 0
    assert "module has no grid encoding" in lib.tcnn_last_error().decode()
    m.close()


def test_empty_batch_is_a_no_op(torch_mod):
    case = F.CASES[0]
    net = make_net(torch_mod, case)
    g = torch_mod.full((net.n_params,), 7.0, dtype=torch_mod.float32, device="cuda")
    ctx = net.L.check_ptr(net.lib.tcnn_module_forward(net.h, None, 0, None, None, None, 1))
    net.L.check(net.lib.tcnn_module_backward(net.h, None, ctx, 0, None, None, _vp(g), None, None, None))
    torch_mod.cuda.synchronize()
    assert float(g.abs().max()) == 0.0
    net.lib.tcnn_context_destroy(ctx)
    net.close()


def _gradients(torch, name="oneblob-w32h2"):
    case = next(c for c in F.CASES if c.name == name and c.act == "ReLU")
    x, dout = F.case_inputs(case, 256)
    p = F.case_params(case)
    out, dx, grad = run(torch, case, x[:256], dout, p)
    return np.concatenate([out.ravel(), dx.ravel(), grad.ravel()])


def test_no_forward_keep_gives_the_same_bits(torch_mod, tmp_path):
    """TCNN_NO_FORWARD_KEEP=1 (read when a module is built) in a fresh child process: the backward recomputes the
    forward and returns the same bits"""
    want = _gradients(torch_mod)
    path = str(tmp_path / "g.npy")
    code = "import numpy as np, torch, test_gpu_mlp_f32 as T; np.save(%r, T._gradients(torch))" % path
    env = dict(os.environ, TCNN_NO_FORWARD_KEEP="1", PYTHONPATH=os.pathsep.join(p for p in sys.path if p))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    np.testing.assert_array_equal(np.load(path).view(np.uint32), want.view(np.uint32))
