"""The torch front end (tinycudann/modules.py, csrc/torch_ext.cpp) in the autograd graphs its callers build,
against the float64 MLP reference (tests/mlp_reference.py) and the oracle's grid functions.

Every other GPU test of the binding makes one model(x) and one backward, on the default stream, with a
contiguous fp32 x and the module object alive throughout. NeuralBTF, SDF and NeRF code calls one module several
times per step at different batch sizes, mixes first- and second-order terms in one loss, accumulates gradients,
freezes parameters, passes column slices and runs on side streams. The engine state those patterns stress -- one
workspace, one fp32 gradient buffer and one scaled-dL/dy buffer per module, a pool of kept encodings that recycles
a buffer when a context dies, kept encodings trusted by pointer identity, the stream taken from the input tensor,
the module's lifetime against the graph's -- is what this module runs, on the C++ autograd node and on the
Python node (modules._EXT = None).

Networks (module_matrix_cases.graph_case, the matrix's scaled seed-42 parameters): T OneBlob 16 + W32/H2 (tile
kernel), I 5 inputs + W64/H2 ReLU (tile, branchy), G grid + W64/H2 (register kernel without dL/dinput, tile with
it), L 16 inputs + W48/H1 CutlassMLP (layered); the kernel family is asserted. The loss of a call is
(out.float() * c).sum() with the matrix's fp16-exact c; the binding's loss scale is handled as in
test_gpu_module_matrix.py::test_torch_front_end (module_matrix_cases.torch_reference). Checks of one call are the
matrix's: outputs within 4 fp16 ulps, weight gradients per element and per matrix, dL/dinput per element (OneBlob
through the CPU encoder's linear backward; the grid's own gradients at relative L2 1e-3 / 2e-3), padded output
rows exactly zero, relative L2 within mlp_reference.aggregate_bar. params.grad summed over two calls in one graph:
mlp_reference.check_wgrad_sum, proved on the CPU by test_mlp_reference.py::test_oracle_sum_of_two_calls_within_bound.
TCNN_MATRIX_RATIOS=<file> appends every test's worst ratios (profiles/torch_graph_ratios.txt).
"""
import gc
import json
import os
import weakref

import numpy as np
import pytest

import mlp_reference as R
import module_matrix_cases as C
import test_grid_f32_reference as G
from helpers import rel_err
from oracle import oracle as O
from test_gpu_module_matrix import _oneblob_dx_check

pytestmark = pytest.mark.gpu

S = 128.0  # the binding's loss scale for fp16 modules
EIKONAL_GRID = {"otype": "HashGrid", "n_levels": 4, "n_features_per_level": 2, "log2_hashmap_size": 8, "base_resolution": 4,
                "per_level_scale": 2.0, "interpolation": "Smoothstep"}


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


def _sync(torch):
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:  # a HIP error leaves the device unusable: end the session, run nothing more on it
        pytest.exit(f"HIP error: {e}", returncode=3)


def _dump(case_id, B, kind, ratios):
    path = os.environ.get("TCNN_MATRIX_RATIOS")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"case": case_id, "B": B, "side": "gpu", "kind": kind, "ratios": ratios}) + "\n")


def _np64(t):
    return t.detach().double().cpu().numpy()


class Net:
    """one torch module of a graph case with the case's scaled parameters (fp32 masters whose fp16 rounding is
    module_matrix_cases.scale_params16, asserted)"""

    def __init__(self, torch, name, seed=C.SEED):
        import tinycudann as tcnn
        self.torch, self.name = torch, name
        case = self.case = C.graph_case(name)
        if case.enc_cfg is None:
            self.model = tcnn.Network(case.n_in, case.n_out, case.net, seed=seed)
        else:
            self.model = tcnn.NetworkWithInputEncoding(case.n_in, case.n_out, case.enc_cfg, case.net, seed=seed)
        nat = self.model.native_tcnn_module
        # a dispatch change cannot silently move the case to another kernel family
        assert nat.backward_kernel(True) == case.kernel_dx and nat.backward_kernel(False) == case.kernel_nodx
        host = C.host_params32(case, seed)
        np.testing.assert_array_equal(self.model.params.detach().cpu().numpy().view(np.uint32), host.view(np.uint32))
        with torch.no_grad():
            self.model.params[:case.n_mlp].mul_(case.scale)
            self.model.params[case.n_mlp:].mul_(C.GRID_SCALE)
        self.p16 = C.scale_params16(case, host)
        np.testing.assert_array_equal(self.model.params.detach().half().cpu().numpy().view(np.uint16), self.p16)
        assert float(self.model.loss_scale) == S


class Call:
    """one model(x) of a Net: the draw, the device tensors and the loss; holds no reference to the module"""

    def __init__(self, net, B, seed, want_dx=True, filtered=False, form=None, run=True):
        torch = net.torch
        case = self.case = C.graph_case(net.name, B)
        self.x, self.enc, self.dout = C.draw(case, net.p16, filtered, seed)
        if form == "float16":  # fp16-exact inputs, so that the reference sees the values the module does
            self.x = O.h2f(O.f2h(self.x))
            self.enc = C.encode(case, net.p16, self.x)
        self.c = torch.from_numpy(O.h2f(self.dout[:, :case.n_out])).cuda()
        x = torch.from_numpy(self.x).cuda()
        if form == "slice":  # columns 1 .. n_in of a wider tensor
            wide = torch.zeros(B, case.n_in + 3, device="cuda")
            wide[:, 1:1 + case.n_in] = x
            x = wide[:, 1:1 + case.n_in]
        elif form == "transposed":
            x = x.t().contiguous().t()
        elif form == "float64":
            x = x.double()
        elif form == "float16":
            x = x.half()
        assert form not in ("slice", "transposed") or not x.is_contiguous()
        self.x_d = x.requires_grad_(want_dx)
        if run:
            self.forward(net)

    def forward(self, net):
        self.out = net.model(self.x_d)
        assert self.out.shape == (self.case.B, self.case.n_out) and self.out.dtype == net.torch.float16
        return self.out

    def loss(self):
        return (self.out.float() * self.c).sum()


def _check_dx(case, p16, call, ref, dx, per_element):
    """dL/dx of one call against the reference, the matrix's way for the case's encoding"""
    assert dx.shape == call.x.shape and np.isfinite(dx).all() and np.abs(dx).max() > 0.0
    bar = R.aggregate_bar(case.W, case.NH, case.out_act)
    ratios = {}
    if case.enc.startswith("identity"):  # dL/dinput is dL/d(encoding); padding columns have no input behind them
        r, m = ref["dinput"][:, :case.n_in], ref["mag_in"][:, :case.n_in]
        if per_element:
            ratios["dinput"] = R.check_dinput(dx, r, m)
        if not (per_element and case.branchy):
            ratios["agg_in"] = rel_err(dx, r)
            assert ratios["agg_in"] <= bar, ("dinput rel L2", ratios["agg_in"], bar)
    elif case.enc.startswith("oneblob"):
        if per_element:
            ratios["dinput"] = _oneblob_dx_check(case, call.x, ref, dx, True)
        if not (per_element and case.branchy):
            ratios["agg_in"] = _oneblob_dx_check(case, call.x, ref, dx, False)
            assert ratios["agg_in"] <= bar, ("dinput rel L2", ratios["agg_in"], bar)
    else:  # the grid's own backward: the oracle on the loss-scaled fp16 dL/d(encoding), divided by the scale
        g = O.grid_cfg(C.GRID, 2)
        ratios["dx_rel"] = rel_err(dx, O.grid_bwd_input(g, call.x, p16[case.n_mlp:], _denc_soa(ref)).astype(np.float64) / S)
        assert ratios["dx_rel"] <= 2e-3, ("grid dL/dx rel L2", ratios["dx_rel"])
    return ratios


def _denc_soa(ref):
    return np.ascontiguousarray(O.f2h((ref["dinput"] * S).astype(np.float32)).T)


def _check_call(net, call, dx=None, per_element=None, tag=""):
    """output and dL/dx (x.grad unless given) of one call; returns (reference, ratios)"""
    case = call.case
    per_element = (not case.branchy) if per_element is None else per_element
    ref = C.torch_reference(case, net.p16, call.enc, call.dout, S)
    R.check_output(_np64(call.out.float()), ref["out"][:, :case.n_out])
    if dx is None and call.x_d.grad is not None:
        assert call.x_d.grad.shape == call.x_d.shape and call.x_d.grad.dtype == call.x_d.dtype
        dx = _np64(call.x_d.grad)
    ratios = {}
    if dx is not None:
        ratios = {k + tag: v for k, v in _check_dx(case, net.p16, call, ref, dx, per_element).items()}
    return ref, ratios


def _check_params(net, calls, refs, grad, per_element=None):
    """params.grad accumulated over calls (one or more) against the sum of their references"""
    case = calls[0].case
    per_element = (not case.branchy) if per_element is None else per_element
    assert grad.shape == (net.model.params.numel(),) and np.isfinite(grad).all()
    bar = R.aggregate_bar(case.W, case.NH, case.out_act)
    mlp = grad[:case.n_mlp]
    if len(refs) == 1:
        ratios = R.check_wgrad(mlp, refs[0], fp16_out=True) if per_element else {}
        if not (per_element and case.branchy):
            ratios["agg_w"] = R.check_aggregate(mlp, refs[0], bar)[0]
    else:
        ratios = R.check_wgrad_sum(mlp, refs, bar, per_element)
    # padded outputs had zero dL/dy: their rows of the output matrix's gradient are exactly zero
    rows = mlp[case.n_mlp - case.OUTP * (case.W if case.NH else case.IN):].reshape(case.OUTP, -1)
    assert np.all(rows[case.n_out:] == 0.0) and np.abs(rows[:case.n_out]).max() > 0.0
    if case.enc == "grid":
        g = O.grid_cfg(C.GRID, 2)
        want = sum(O.grid_bwd(g, c.x, _denc_soa(r)).astype(np.float64) for c, r in zip(calls, refs)) / S
        ratios["grid_rel"] = rel_err(grad[case.n_mlp:], want)
        assert ratios["grid_rel"] <= 1e-3, ("grid gradient rel L2", ratios["grid_rel"])
    return ratios


def _check_step(net, call, per_element=None):
    """the single-call checks after a backward: output, x.grad (if requested), params.grad"""
    ref, ratios = _check_call(net, call, per_element=per_element)
    ratios.update(_check_params(net, [call], [ref], _np64(net.model.params.grad), per_element))
    return ratios


# ---- B.1 ----
TWICE = [(n, d, False) for n, d in C.GRAPH_TWICE] + [("T", True, True)]


@pytest.mark.parametrize("name,want_dx,create_graph", TWICE,
                         ids=[f"{n}-{'dx' if d else 'nodx'}" + ("-create_graph" if cg else "") for n, d, cg in TWICE])
def test_one_module_twice_in_one_graph(torch_mod, node, name, want_dx, create_graph):
    """o1 = model(x1) at B = 256, o2 = model(x2) at B = 300 (padded to 512), one loss, one backward: both forward
    contexts are alive at once, the second forward grows the workspace and takes a second kept-encoding buffer, and
    the first call's backward runs after the larger call used the module's buffers. Outputs and x.grad per call;
    params.grad, the fp32 sum of two fp16 gradients, per element against ref1 + ref2. create_graph=False takes the
    nodes' one-call fast path, create_graph=True the differentiable backward."""
    torch = torch_mod
    net = Net(torch, name)
    calls = [Call(net, B, seed, want_dx) for seed, B in enumerate(C.GRAPH_TWICE_B)]
    loss = calls[0].loss() + calls[1].loss()
    if create_graph:
        grads = torch.autograd.grad(loss, [net.model.params] + [c.x_d for c in calls], create_graph=True)
        assert all(g.requires_grad for g in grads)
        pgrad, dxs = grads[0], [_np64(g) for g in grads[1:]]
    else:
        loss.backward()
        pgrad, dxs = net.model.params.grad, [None, None]
    _sync(torch)
    assert pgrad.dtype == torch.float32
    ratios, refs = {}, []
    for k, (call, dx) in enumerate(zip(calls, dxs)):
        assert want_dx or call.x_d.grad is None
        ref, r = _check_call(net, call, dx=dx, tag=str(k + 1))
        assert want_dx == any(key.startswith(("dinput", "agg_in", "dx_rel")) for key in r)
        refs.append(ref)
        ratios.update(r)
    ratios.update(_check_params(net, calls, refs, _np64(pgrad)))
    _dump(C.graph_id(name, want_dx) + ("-create_graph" if create_graph else ""), "+".join(map(str, C.GRAPH_TWICE_B)),
          f"graph-twice-{node}", ratios)


# ---- B.2 ----
@pytest.mark.parametrize("name", ["T", "G"])
def test_batch_size_changes_between_steps(torch_mod, node, name):
    """steps at B = 512, 256, 768, 256 on one module (T with dL/dx, G without: the register kernel and its kept
    encoding), gradients cleared and the graph freed in between, a fresh draw each: a step after a larger one
    must see nothing of it (workspace tails, the recycled kept-encoding buffer, the fp32 gradient buffer)."""
    torch = torch_mod
    net = Net(torch, name)
    for step, B in enumerate((512, 256, 768, 256)):
        net.model.params.grad = None
        call = Call(net, B, seed=step, want_dx=name == "T")
        call.loss().backward()
        _sync(torch)
        _dump(C.graph_id(name, name == "T"), B, f"graph-steps{step}-{node}", _check_step(net, call))
        del call


# ---- B.3 ----
@pytest.mark.parametrize("name", ["T", "G"])
def test_retain_graph_backward_twice(torch_mod, node, name):
    """backward(retain_graph=True), then backward again on the same graph: the forward context is used twice.
    The first gradient against the reference; after the second every element of params.grad (fp32) and x.grad is
    exactly twice the first."""
    torch = torch_mod
    net = Net(torch, name)
    call = Call(net, 300, seed=0, want_dx=name == "T")
    loss = call.loss()
    loss.backward(retain_graph=True)
    _sync(torch)
    _dump(C.graph_id(name, name == "T"), 300, f"graph-retain-{node}", _check_step(net, call))
    first = net.model.params.grad.clone()
    first_dx = call.x_d.grad.clone() if name == "T" else None
    loss.backward()
    _sync(torch)
    assert first.abs().max() > 0 and torch.equal(net.model.params.grad, 2 * first)
    if name == "T":
        assert first_dx.abs().max() > 0 and torch.equal(call.x_d.grad, 2 * first_dx)


# ---- B.4 ----
def test_two_modules_interleaved(torch_mod, node):
    """forward A, forward B, backward B, backward A on two T models with different seeds: each against its own
    reference, and bit for bit what the same call gives alone on a fresh model."""
    torch = torch_mod
    specs = [(C.SEED, 256, 0), (C.SEED + 1, 300, 1)]  # (parameter seed, B, draw seed)
    nets = [Net(torch, "T", seed) for seed, _, _ in specs]
    calls = [Call(net, B, ds) for net, (_, B, ds) in zip(nets, specs)]
    calls[1].loss().backward()
    calls[0].loss().backward()
    _sync(torch)
    for k, (net, call, (seed, B, ds)) in enumerate(zip(nets, calls, specs)):
        _dump(call.case.id + f"-seed{seed}", B, f"graph-interleaved-{node}", _check_step(net, call))
        alone_net = Net(torch, "T", seed)
        alone = Call(alone_net, B, ds)
        alone.loss().backward()
        _sync(torch)
        assert torch.equal(alone.out, call.out)
        assert torch.equal(alone_net.model.params.grad, net.model.params.grad)
        assert torch.equal(alone.x_d.grad, call.x_d.grad)


# ---- B.5 ----
@pytest.mark.parametrize("config", ["x_only", "params_only", "neither", "no_grad"])
def test_who_needs_a_gradient(torch_mod, node, config):
    """frozen parameters with x.requires_grad; x without grad; neither under grad mode; torch.no_grad()"""
    torch = torch_mod
    net = Net(torch, "T")
    net.model.params.requires_grad_(config == "params_only")
    want_dx = config == "x_only"
    if config == "no_grad":
        with torch.no_grad():
            call = Call(net, 300, 0, want_dx=False)
    else:
        call = Call(net, 300, 0, want_dx=want_dx)
    if config in ("neither", "no_grad"):
        _sync(torch)
        assert call.out.grad_fn is None and not call.out.requires_grad
        _check_call(net, call)
        return
    call.loss().backward()
    _sync(torch)
    ref, ratios = _check_call(net, call)
    if config == "x_only":
        assert net.model.params.grad is None and "dinput" in ratios
    else:
        assert call.x_d.grad is None
        ratios.update(_check_params(net, [call], [ref], _np64(net.model.params.grad)))
    _dump(call.case.id, 300, f"graph-needs_{config}-{node}", ratios)


# ---- B.6 ----
@pytest.mark.parametrize("form", ["slice", "transposed", "float64", "float16"])
@pytest.mark.parametrize("name", ["T", "I"])
def test_input_forms(torch_mod, node, name, form):
    """x as a column slice of a wider tensor, as the transpose of an [n_in, B] tensor, as float64 and as float16
    (fp16-exact values): x.grad has x's shape and dtype (asserted in _check_call) and passes the per-element check
    (I: on ReLU-clear samples), params.grad as well."""
    torch = torch_mod
    net = Net(torch, name)
    call = Call(net, 300, 0, filtered=net.case.branchy, form=form)
    call.loss().backward()
    _sync(torch)
    assert call.x_d.grad is not None
    _dump(call.case.id, 300, f"graph-form_{form}-{node}", _check_step(net, call, per_element=True))


@pytest.mark.parametrize("loss", ["sum", "permuted"])
def test_doutput_forms(torch_mod, node, loss):
    """out.sum() (an expanded, stride-0 gradient of ones) and a loss through out[:, [2, 0, 1]], against the
    reference on the corresponding dL/dy"""
    torch = torch_mod
    net = Net(torch, "T")
    call = Call(net, 300, 0)
    n_out = call.case.n_out
    if loss == "sum":
        call.out.sum().backward()
        call.dout[:, :n_out] = O.f2h(np.ones((300, n_out), np.float32))
    else:
        perm = [2, 0, 1]
        (call.out[:, perm].float() * call.c).sum().backward()
        c16 = call.dout[:, :n_out].copy()
        call.dout[:, perm] = c16  # d loss / d out[:, perm[k]] = c[:, k]
    _sync(torch)
    _dump(call.case.id, 300, f"graph-dout_{loss}-{node}", _check_step(net, call))


# ---- B.7 ----
def test_graph_outlives_the_module(torch_mod, node):
    """A function builds the model, runs model(x) and returns only the output and the parameters: the graph is
    then the only owner of the engine module, and must keep it alive until the backward has run (the Python node
    keeps ctx.native_tcnn_module; the C++ node keeps the same object in its saved data). The weak reference shows
    both halves without touching a destroyed module: alive while the graph is, collected once the graph is gone."""
    torch = torch_mod
    import tinycudann as tcnn

    def build():
        net = Net(torch, "T")
        call = Call(net, 300, 0)
        return call, net.model.params, net.p16, weakref.ref(net.model.native_tcnn_module)

    call, params, p16, native = build()
    gc.collect()
    assert native() is not None, "the autograd graph does not keep the engine module alive"
    tcnn.free_temporary_memory()
    other = Net(torch, "L")  # an unrelated module: freed host memory gets a chance to be reused
    Call(other, 256, 1).loss().backward()
    call.loss().backward()
    _sync(torch)

    class Owner:  # what _check_call / _check_params read of a Net
        pass
    net = Owner()
    net.p16, net.model = p16, Owner()
    net.model.params = params
    ref, ratios = _check_call(net, call)
    ratios.update(_check_params(net, [call], [ref], _np64(params.grad)))
    _dump(call.case.id, 300, f"graph-outlives-{node}", ratios)
    del call.out, call
    gc.collect()
    assert native() is None, "the engine module is still referenced after its graph is gone"


# ---- B.8 ----
@pytest.fixture(scope="module")
def sleep_cycles(torch_mod):
    """cycles for which torch.cuda._sleep lasts at least 20 ms on this device (timed with two events)"""
    torch = torch_mod

    def timed(cycles):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        torch.cuda._sleep(cycles)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    timed(1000)
    cycles = 1_000_000
    for _ in range(4):
        ms = timed(cycles)
        if ms >= 20.0:
            return cycles
        cycles = int(cycles * 30.0 / max(ms, 0.01))
    pytest.fail(f"torch.cuda._sleep could not be calibrated to 20 ms ({cycles} cycles: {ms} ms)")


def _behind_a_sleep(torch, stream, cycles, x_real, requires_grad=True):
    """x full of NaN (written and synchronised on the default stream), and on the side stream a sleep followed by
    the copy of the real values into x: until the sleep ends, work on any other stream reads the NaNs. The caller
    keeps x_real alive until it has synchronised (the copy is still pending when this returns)."""
    x = torch.full_like(x_real, float("nan")).requires_grad_(requires_grad)
    _sync(torch)
    with torch.cuda.stream(stream), torch.no_grad():
        torch.cuda._sleep(cycles)
        x.copy_(x_real)
    return x


@pytest.fixture(scope="module")
def side_stream(torch_mod, sleep_cycles):
    """A side stream the default stream really overtakes. With few hardware queues a stream can share its queue with
    the default stream, and work on the two is then serialised whatever the binding does: the first of torch's pool
    streams behind whose sleep a plain torch copy on the default stream still reads the NaNs. A condition of the
    method, like the sleep's length; the control below is what shows that the module's own forward is caught."""
    torch = torch_mod
    real = torch.zeros(64, device="cuda")
    for _ in range(8):
        s = torch.cuda.Stream()
        x = _behind_a_sleep(torch, s, sleep_cycles, real, requires_grad=False)
        seen = x.clone()  # default stream
        s.synchronize()
        _sync(torch)
        if torch.isnan(seen).all():
            return s
    pytest.fail("no side stream runs concurrently with the default stream")


def test_side_stream_network(torch_mod, node, sleep_cycles, side_stream):
    """forward, loss and backward of T on a side stream, behind a >= 20 ms sleep and the copy that makes x valid:
    a kernel, memset or copy the binding or the engine issues on another stream reads NaNs or a stale buffer."""
    torch = torch_mod
    net = Net(torch, "T")
    call = Call(net, 300, 0, run=False)
    real = call.x_d.detach()
    s = side_stream
    call.x_d = _behind_a_sleep(torch, s, sleep_cycles, real)
    with torch.cuda.stream(s):
        call.forward(net)
        call.loss().backward()
    s.synchronize()
    _sync(torch)
    assert torch.isfinite(call.out).all() and torch.isfinite(call.x_d.grad).all() and torch.isfinite(net.model.params.grad).all()
    _dump(call.case.id, 300, f"graph-stream-{node}", _check_step(net, call))


def _eikonal_encoding(torch, rng):
    import tinycudann as tcnn
    enc = tcnn.Encoding(2, EIKONAL_GRID, dtype=torch.float32)
    assert enc.params.dtype == torch.float32 and enc.loss_scale == 1.0 and enc.n_output_dims == 8
    table16 = O.f2h(rng.uniform(-1, 1, enc.params.numel()).astype(np.float32))
    with torch.no_grad():
        enc.params.copy_(torch.from_numpy(O.h2f(table16)).cuda())
    return enc, table16


def _check_encoding_first_order(y, dx, pgrad, pos, table16, u16):
    """y of an fp32 grid encoding against the float64 grid reference within its forward bound
    (test_grid_f32_reference.py); dL/dx and dL/dparams of loss = (y * u).sum() against the oracle at the tolerances of
    test_gpu_encoding_f32.py::test_torch_encoding_fp32"""
    g = O.grid_cfg(EIKONAL_GRID, 2)
    u_soa = np.ascontiguousarray(u16.T)
    yref, A, E = G.grid_forward(g, pos, O.h2f(table16))
    assert np.all(np.abs(y - yref) <= G.forward_bound(g, A, E))
    dxref = O.grid_bwd_input(g, pos, table16, u_soa)
    np.testing.assert_allclose(dx, dxref, rtol=1e-4, atol=1e-4 * np.abs(dxref).max())
    e = rel_err(pgrad, O.grid_bwd(g, pos, u_soa))
    assert e <= 2e-3, ("grid gradient rel L2", e)
    return {"pgrad_rel": e}


def test_side_stream_encoding(torch_mod, node, sleep_cycles, side_stream):
    """the same on the fp32 grid encoding of the eikonal test: everything finite and against the oracle"""
    torch = torch_mod
    rng = np.random.default_rng(21)
    enc, table16 = _eikonal_encoding(torch, rng)
    pos = rng.uniform(0, 1, (300, 2)).astype(np.float32)
    u16 = O.f2h(rng.uniform(-1, 1, (300, 8)).astype(np.float32))
    u = torch.from_numpy(O.h2f(u16)).cuda()
    real = torch.from_numpy(pos).cuda()
    s = side_stream
    x = _behind_a_sleep(torch, s, sleep_cycles, real)
    with torch.cuda.stream(s):
        y = enc(x)
        (y * u).sum().backward()
    s.synchronize()
    _sync(torch)
    assert torch.isfinite(y).all() and torch.isfinite(x.grad).all() and torch.isfinite(enc.params.grad).all()
    ratios = _check_encoding_first_order(y.detach().cpu().numpy(), x.grad.cpu().numpy(), enc.params.grad.cpu().numpy(), pos, table16, u16)
    _dump("encoding-f32-grid-l4", 300, f"graph-stream-{node}", ratios)


def test_side_stream_control_detects(torch_mod, node, sleep_cycles, side_stream):
    """The control of the two tests above: the same sequence with the forward issued on the default stream, without
    a synchronise, is what a binding that ignored the current stream would do. It reads the NaN positions (a valid
    tensor, only stale): the grid encoding's output is NaN, and the network's output -- OneBlob clamps its kernel's
    CDF, so NaN encodes to finite values -- fails the output check."""
    torch = torch_mod
    rng = np.random.default_rng(21)
    enc, _ = _eikonal_encoding(torch, rng)
    real = torch.from_numpy(rng.uniform(0, 1, (300, 2)).astype(np.float32)).cuda()
    s = side_stream
    x = _behind_a_sleep(torch, s, sleep_cycles, real, requires_grad=False)
    y = enc(x)  # default stream: overtakes the side stream's sleep and copy
    s.synchronize()
    _sync(torch)
    assert torch.isnan(y).any(), "the control did not detect: a forward on another stream saw the real positions"
    net = Net(torch, "T")
    call = Call(net, 300, 0, want_dx=False, run=False)
    real = call.x_d
    call.x_d = _behind_a_sleep(torch, s, sleep_cycles, real, requires_grad=False)
    call.forward(net)
    s.synchronize()
    _sync(torch)
    with pytest.raises(AssertionError):
        _check_call(net, call)


# ---- B.9 ----
def test_eikonal_pattern_fp32_grid(torch_mod, node):
    """The SDF pattern on tcnn.Encoding(2, Smoothstep hash grid, dtype=float32), two point sets (B = 256 and 300)
    in one graph: y = enc(x), g = autograd.grad((y * w).sum(), x, create_graph=True), loss = (y * u).sum() +
    (g * v).sum() per call, one backward of the total. First- and second-order parameter gradients of both calls
    accumulate in enc.params.grad. x.grad is the sum of the first-order dL/dx of the u term and the second-order one of
    the v term. Tolerances: test_gpu_encoding_f32.py::test_torch_encoding_fp32's. u is sized so that the first-order
    parameter gradient is within a factor of 10 of the second-order one (asserted on the reference): the 2e-3 bar on
    their sum cannot pass with either missing."""
    torch = torch_mod
    rng = np.random.default_rng(9)
    enc, table16 = _eikonal_encoding(torch, rng)
    g = O.grid_cfg(EIKONAL_GRID, 2)
    calls, total = [], 0.0
    for B in (256, 300):
        pos = rng.uniform(0, 1, (B, 2)).astype(np.float32)
        w16 = O.f2h((rng.standard_normal((B, 8)) * 0.1).astype(np.float32))
        u16 = O.f2h((rng.standard_normal((B, 8)) * 0.01).astype(np.float32))
        v = (rng.standard_normal((B, 2)) * 1e-3).astype(np.float32)
        x = torch.from_numpy(pos).cuda().requires_grad_(True)
        w = torch.from_numpy(O.h2f(w16)).cuda().requires_grad_(True)
        y = enc(x)
        assert y.dtype == torch.float32 and y.shape == (B, 8)
        gx = torch.autograd.grad((y * w).sum(), x, create_graph=True)[0]
        total = total + (y * torch.from_numpy(O.h2f(u16)).cuda()).sum() + (gx * torch.from_numpy(v).cuda()).sum()
        calls.append((pos, w16, u16, v, x, w, gx))
    total.backward()
    _sync(torch)
    first, second, ratios = 0.0, 0.0, {}
    for k, (pos, w16, u16, v, x, w, gx) in enumerate(calls):
        w_soa, u_soa = np.ascontiguousarray(w16.T), np.ascontiguousarray(u16.T)
        rgrad, rddy, rdx = O.grid_bwd_bwd(g, pos, table16, v, w_soa)
        gxn, gref = gx.detach().cpu().numpy(), O.grid_bwd_input(g, pos, table16, w_soa)
        np.testing.assert_allclose(gxn, gref, rtol=1e-4, atol=1e-4 * np.abs(gxn).max())
        dxref = rdx.astype(np.float64) + O.grid_bwd_input(g, pos, table16, u_soa)
        assert 0.1 <= np.linalg.norm(rdx) / np.linalg.norm(dxref - rdx) <= 10.0
        assert x.grad.dtype == torch.float32 and w.grad.dtype == torch.float32
        np.testing.assert_allclose(_np64(x.grad), dxref, rtol=1e-4, atol=1e-4 * np.abs(dxref).max())
        np.testing.assert_allclose(w.grad.cpu().numpy(), rddy, rtol=2e-3, atol=1e-4 * np.abs(rddy).max())
        ratios[f"g_rel{k + 1}"], ratios[f"xgrad_rel{k + 1}"] = rel_err(gxn, gref), rel_err(_np64(x.grad), dxref)
        ratios[f"wgrad_rel{k + 1}"] = rel_err(w.grad.cpu().numpy(), rddy)
        first, second = first + O.grid_bwd(g, pos, u_soa).astype(np.float64), second + rgrad.astype(np.float64)
    assert 0.1 <= np.linalg.norm(first) / np.linalg.norm(second) <= 10.0
    ratios["pgrad_rel"] = rel_err(_np64(enc.params.grad), first + second)
    assert ratios["pgrad_rel"] <= 2e-3, ("grid gradient rel L2", ratios["pgrad_rel"])
    _dump("encoding-f32-grid-l4", "256+300", f"graph-eikonal-{node}", ratios)
