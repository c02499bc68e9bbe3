"""tinycudann.Loss on the GPU against the numpy restatement of the reference's nine losses
(tests/loss_reference.py, pinned on the CPU by tests/test_loss_reference.py).

  1. fp16 predictions (a [:, :dims] view of a padded [n, 16] tensor): the gradient that reaches the padded leaf
     through (loss * s).backward() equals R.evaluate's, bit for bit, zero outside the view
  2. the value: |S - sum64 v| <= (n dims) 2^-24 sum|v| (the bound of any summation order of the restatement's fp32
     values v), and two calls give the same bits -- also with many partial sums (n = 65536, dims = 3)
  3. fp32 predictions that no fp16 holds: the gradient against the closed-form float64 derivative of
     R.value_f64 with the normaliser held fixed, within 2^-20 |ref| + one fp32 denormal (at most 8 fp32 roundings
     of 2^-24 each are 2^-21; the tolerance doubles that)
  4. autograd graphs, on the C++ node and on the Python node, which agree bit for bit
"""
import functools
import pickle

import numpy as np
import pytest

import loss_reference as R
from helpers import CONFIG_HASH
from oracle import oracle as O

pytestmark = pytest.mark.gpu

STRIDE = 16
NS = (1, 255, 257)  # one element; below and above one workgroup's 2048 elements at dims = 16 (and 8, 9 rows more)
SCALES = (1.0, 128.0, float(np.float32(0.37)))
SIGN_LOSSES = ("L1", "RelativeL1", "Mape", "Smape")
C01 = float(np.float32(0.01))  # the constants as the engine holds them (fp32)


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(params=[False, True], ids=["cpp_node", "python_node"])
def node(request, monkeypatch):
    """both autograd nodes, selected as tests/test_gpu_encoding_f32.py does"""
    from tinycudann import modules
    if request.param:
        monkeypatch.setattr(modules, "_EXT", None)
    elif modules._EXT is None:
        pytest.fail("the C++ autograd node (lib/_tcnn_torch) is not built")
    return "python" if request.param else "cpp"


def _dims_of(otype):
    return (3, 6) if otype == "RelativeL2Luminance" else (1, 3, 6, 16)


CASES = [(o, d) for o in R.LOSSES for d in _dims_of(o)]


@functools.lru_cache(maxsize=None)
def _inputs(n, dims, seed=3):
    """drawn as tests/test_loss_reference.py::_inputs draws, padded columns zero; every seventh element has
    prediction == target (the sign losses' copysign of a zero difference)"""
    rng = np.random.default_rng(seed)
    pred = np.zeros((n, STRIDE), np.float32)
    pred[:, :dims] = rng.uniform(0.2, 2.0, size=(n, dims))
    pred16 = O.f2h(pred)
    tgt = rng.uniform(0.05, 1.0, size=(n, dims)).astype(np.float32)
    pdf = rng.uniform(0.25, 4.0, size=(n, dims)).astype(np.float32)
    planted = np.arange(n * dims).reshape(n, dims) % 7 == 3
    tgt[planted] = O.h2f(pred16)[:, :dims][planted]
    for a in (pred16, tgt, pdf):
        a.setflags(write=False)
    return pred16, tgt, pdf


@functools.lru_cache(maxsize=None)
def _reference(otype, n, dims, with_pdf, scale):
    pred16, tgt, pdf = _inputs(n, dims)
    return R.evaluate(otype, pred16, tgt, scale, pdf if with_pdf else None)


def _value_bound(v):
    """(sum in float64, bound of |S - sum| for an fp32 sum of v in any order)"""
    v64 = v.astype(np.float64)
    return v64.sum(), v.size * 2.0 ** -24 * np.abs(v64).sum()


def _leaf16(torch, pred16):
    return torch.from_numpy(pred16.view(np.float16).copy()).cuda().requires_grad_(True)


def _bits16(t):
    return t.detach().cpu().numpy().view(np.uint16)


def _bits32(t):
    return t.detach().float().cpu().numpy().reshape(-1).view(np.uint32)


# ---------------------------------------------------------------------------------------------
# 1, 2: fp16 predictions
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_pdf", [False, True], ids=["nopdf", "pdf"])
@pytest.mark.parametrize("otype,dims", CASES)
def test_fp16_gradient_bits_and_value(torch_mod, otype, dims, with_pdf):
    torch = torch_mod
    import tinycudann as tcnn
    loss = tcnn.Loss(otype)
    for n in NS:
        pred16, tgt, pdf = _inputs(n, dims)
        t_d = torch.from_numpy(tgt.copy()).cuda()
        q_d = torch.from_numpy(pdf.copy()).cuda() if with_pdf else None
        values = []
        for s in SCALES:
            what = (otype, dims, with_pdf, n, s)
            leaf = _leaf16(torch, pred16)
            view = leaf[:, :dims]
            assert view.stride(0) == STRIDE  # taken as it is: rows of the padded tensor
            value = loss(view, t_d, q_d)
            assert value.shape == () and value.dtype == torch.float32 and value.is_cuda, what
            (value * s).backward()
            v_ref, g_ref = _reference(otype, n, dims, with_pdf, s)
            got = _bits16(leaf.grad)
            assert got.shape == (n, STRIDE)
            bad = np.flatnonzero(got != g_ref)
            assert bad.size == 0, (what, int(bad.size), int(bad[0]), hex(int(got.flat[bad[0]])), hex(int(g_ref.flat[bad[0]])))
            assert not got[:, dims:].any(), what  # zero outside the view
            values.append(value)
        # the planted elements: a zero difference gives +scale for the sign losses, never a zero gradient
        if otype in SIGN_LOSSES and n * dims > 3:
            planted = np.arange(n * dims).reshape(n, dims) % 7 == 3
            assert np.all(O.h2f(got[:, :dims])[planted] > 0), what
        # 2: the value (independent of the scale: the same bits from the three calls)
        S = [float(v.item()) for v in values]
        assert _bits32(values[0]) == _bits32(values[1]) == _bits32(values[2]), (otype, dims, with_pdf, n, S)
        total, bound = _value_bound(v_ref[:, :dims])
        print(otype, dims, with_pdf, n, "S", S[0], "sum64", total, "|diff|", abs(S[0] - total), "bound", bound)
        assert abs(S[0] - total) <= bound, (otype, dims, with_pdf, n, S[0], total, bound)


def test_value_with_many_partials_is_reproducible(torch_mod):
    """n = 65536, dims = 3: 96 workgroups' partial sums and the final sum"""
    torch = torch_mod
    import tinycudann as tcnn
    n, dims = 65536, 3
    pred16, tgt, pdf = _inputs(n, dims)
    view = _leaf16(torch, pred16)[:, :dims]
    t_d, q_d = torch.from_numpy(tgt.copy()).cuda(), torch.from_numpy(pdf.copy()).cuda()
    for otype in ("RelativeL2", "L1"):
        loss = tcnn.Loss(otype)
        a, b = loss(view, t_d, q_d), loss(view, t_d, q_d)
        assert _bits32(a) == _bits32(b), otype
        total, bound = _value_bound(R.evaluate(otype, pred16, tgt, 1.0, pdf)[0][:, :dims])
        print(otype, "S", a.item(), "sum64", total, "bound", bound)
        assert abs(float(a.item()) - total) <= bound, (otype, a.item(), total, bound)


# ---------------------------------------------------------------------------------------------
# 3: fp32 predictions
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _inputs32(n, dims, seed=11):
    rng = np.random.default_rng(seed)
    pred = rng.uniform(0.2, 2.0, size=(n, dims)).astype(np.float32)
    tgt = rng.uniform(0.05, 1.0, size=(n, dims)).astype(np.float32)
    pdf = rng.uniform(0.25, 4.0, size=(n, dims)).astype(np.float32)
    return pred, tgt, pdf


def _lum64(p, dims):
    r, g, b = p[:, 0], p[:, 1], p[:, 2]
    if dims >= 6:
        r, g, b = r + p[:, 3], g + p[:, 4], b + p[:, 5]
    c = [float(np.float32(x)) for x in (0.299, 0.587, 0.114)]
    return (c[0] * r + c[1] * g + c[2] * b)[:, None]


def _norm64(otype, p, t, dims):
    if otype == "RelativeL2":
        return p * p + C01
    if otype == "RelativeL2Luminance":
        lum = _lum64(p, dims)
        return np.broadcast_to(lum * lum + C01, p.shape)
    if otype == "RelativeL1":
        return np.abs(p) + C01
    if otype == "Mape":
        return np.abs(t) + C01
    if otype == "Smape":
        return 0.5 * (np.abs(t) + np.abs(p)) + C01
    return None


def _derivative64(otype, p, t, q, nt, norm):
    """d R.value_f64 / dp in float64, the normaliser norm held fixed"""
    d = p - t
    if otype == "L2":
        return 2.0 * d / q / nt
    if otype in ("RelativeL2", "RelativeL2Luminance"):
        return 2.0 * d / norm / q / nt
    if otype == "L1":
        return np.sign(d) / q / nt
    if otype in ("RelativeL1", "Mape", "Smape"):
        return np.sign(d) / norm / q / nt
    if otype == "CrossEntropy":
        return -t / q / nt / p
    return -(t * t / q / nt) / (p * p)


def test_fp32_generator_keeps_95_percent():
    """(CPU arithmetic) the share of elements clear of the sign losses' kink, for the shapes and seed used below"""
    for dims in (1, 3, 6, 16):
        pred, tgt, _ = _inputs32(257, dims)
        assert (np.abs(pred - tgt) > 1e-3).mean() >= 0.95, dims


@pytest.mark.parametrize("with_pdf", [False, True], ids=["nopdf", "pdf"])
@pytest.mark.parametrize("otype,dims", CASES)
def test_fp32_gradient_and_value(torch_mod, otype, dims, with_pdf):
    torch = torch_mod
    import tinycudann as tcnn
    n, s = 257, 128.0
    pred, tgt, pdf = _inputs32(n, dims)
    assert (O.h2f(O.f2h(pred)) != pred).mean() > 0.9  # not fp16 values
    p, t = pred.astype(np.float64), tgt.astype(np.float64)
    q = pdf.astype(np.float64) if with_pdf else np.ones_like(p)
    nt = float(n * dims)
    norm = _norm64(otype, p, t, dims)
    leaf = torch.from_numpy(pred.copy()).cuda().requires_grad_(True)
    value = tcnn.Loss(otype)(leaf, torch.from_numpy(tgt.copy()).cuda(), torch.from_numpy(pdf.copy()).cuda() if with_pdf else None)
    (value * s).backward()
    assert leaf.grad.dtype == torch.float32
    got = leaf.grad.cpu().numpy().astype(np.float64)
    ref = s * _derivative64(otype, p, t, q, nt, norm)
    keep = np.ones(p.shape, bool)
    if otype in SIGN_LOSSES:
        keep = np.abs(p - t) > 1e-3
        assert keep.mean() >= 0.95
    tol = 2.0 ** -20 * np.abs(ref) + 2.0 ** -149
    err = np.abs(got - ref)
    print(otype, dims, with_pdf, "max err / tol", float(np.max((err / tol)[keep])))
    assert np.all(err[keep] <= tol[keep]), (otype, dims, with_pdf, float(np.max((err / tol)[keep])))
    # the value
    ref_v = R.value_f64(otype, p, t, q, nt, norm)
    mag = np.abs(ref_v)
    if otype == "Variance":
        f = t ** 2 / q / nt
        mag = np.abs(f / p) + np.abs(f / q)
    bound = ref_v.size * 2.0 ** -24 * np.abs(ref_v).sum() + 1e-6 * mag.sum()
    print(otype, dims, with_pdf, "S", value.item(), "sum64", ref_v.sum(), "bound", bound)
    assert abs(float(value.item()) - ref_v.sum()) <= bound


# ---------------------------------------------------------------------------------------------
# 4: graphs
# ---------------------------------------------------------------------------------------------
def _model_batch(torch, B=256):
    import tinycudann as tcnn
    model = tcnn.NetworkWithInputEncoding(2, 3, CONFIG_HASH["encoding"], CONFIG_HASH["network"], seed=1337)
    rng = np.random.default_rng(7)
    x = torch.from_numpy(rng.uniform(0, 1, (B, 2)).astype(np.float32)).cuda()
    tgt = rng.uniform(0.05, 1.0, (B, 3)).astype(np.float32)
    return model, x, tgt


def test_prediction_straight_from_a_network(torch_mod, node):
    """the strided [B, 3] slice of the module's [B, 16] output, taken as it is: value and dL/doutput follow from
    the module's actual output by 1 and 2, and the gradient reaches the parameters"""
    torch = torch_mod
    import tinycudann as tcnn
    model, x, tgt = _model_batch(torch)
    out = model(x)
    assert out.dtype == torch.float16 and out.shape == (256, 3) and out.stride(0) == 16
    seen = []
    out.register_hook(seen.append)
    value = tcnn.Loss("RelativeL2")(out, torch.from_numpy(tgt.copy()).cuda())
    value.backward()
    pred16 = np.zeros((256, STRIDE), np.uint16)
    pred16[:, :3] = _bits16(out)
    v_ref, g_ref = R.evaluate("RelativeL2", pred16, tgt, 1.0)
    np.testing.assert_array_equal(_bits16(seen[0]), g_ref[:, :3])
    total, bound = _value_bound(v_ref[:, :3])
    assert abs(float(value.item()) - total) <= bound
    g = model.params.grad
    assert g is not None and torch.isfinite(g).all() and bool((g != 0).any())


def test_two_losses_on_one_prediction(torch_mod, node):
    torch = torch_mod
    import tinycudann as tcnn
    n, dims = 255, 3
    pred16, tgt, pdf = _inputs(n, dims)
    leaf = _leaf16(torch, pred16)
    view = leaf[:, :dims]
    t_d = torch.from_numpy(tgt.copy()).cuda()
    total = tcnn.Loss("L2")(view, t_d) + tcnn.Loss("Smape")(view, t_d, torch.from_numpy(pdf.copy()).cuda())
    total.backward()
    g1 = torch.from_numpy(_reference("L2", n, dims, False, 1.0)[1].view(np.float16))
    g2 = torch.from_numpy(_reference("Smape", n, dims, True, 1.0)[1].view(np.float16))
    want = {_bits16(g1 + g2).tobytes(), _bits16(g2 + g1).tobytes()}  # fp16 addition commutes; either order
    assert _bits16(leaf.grad).tobytes() in want


def test_retain_graph_no_grad_and_target_grad(torch_mod, node):
    torch = torch_mod
    import tinycudann as tcnn
    n, dims = 257, 6
    pred16, tgt, _ = _inputs(n, dims)
    loss = tcnn.Loss("RelativeL2Luminance")
    leaf = _leaf16(torch, pred16)
    target = torch.from_numpy(tgt.copy()).cuda().requires_grad_(True)
    value = loss(leaf[:, :dims], target)
    value.backward(retain_graph=True)
    first = _bits16(leaf.grad).copy()
    np.testing.assert_array_equal(first, _reference("RelativeL2Luminance", n, dims, False, 1.0)[1])
    leaf.grad = None
    value.backward()
    np.testing.assert_array_equal(_bits16(leaf.grad), first)
    assert target.grad is None  # no gradient flows to the target
    with torch.no_grad():
        quiet = loss(leaf[:, :dims], target)
    assert quiet.grad_fn is None and not quiet.requires_grad
    assert _bits32(quiet) == _bits32(value)
    # predictions that need no gradient: a value, no graph
    plain = loss(leaf.detach()[:, :dims], target.detach())
    assert plain.grad_fn is None and _bits32(plain) == _bits32(value)


def test_double_backward_is_refused(torch_mod, node):
    torch = torch_mod
    import tinycudann as tcnn
    n, dims = 255, 3
    pred16, tgt, _ = _inputs(n, dims)
    leaf = _leaf16(torch, pred16)
    value = tcnn.Loss("L2")(leaf[:, :dims], torch.from_numpy(tgt.copy()).cuda())
    (g,) = torch.autograd.grad(value, leaf, create_graph=True)
    np.testing.assert_array_equal(_bits16(g), _reference("L2", n, dims, False, 1.0)[1])  # the first order still holds
    assert g.requires_grad
    with pytest.raises(RuntimeError, match="not implemented"):
        g.float().sum().backward()


def test_pickle_and_refusals(torch_mod, node):
    torch = torch_mod
    import tinycudann as tcnn
    loss = tcnn.Loss({"otype": "smape"})
    twin = pickle.loads(pickle.dumps(loss))
    assert twin.otype == "smape" and {k for k in twin.__dict__ if not k.startswith("_") and k != "training"} == {"otype"}
    pred16, tgt, _ = _inputs(255, 3)
    view = _leaf16(torch, pred16)[:, :3]
    t_d = torch.from_numpy(tgt.copy()).cuda()
    assert _bits32(loss(view, t_d)) == _bits32(twin(view, t_d)) == _bits32(tcnn.Loss("SMAPE")(view, t_d))
    with pytest.raises(RuntimeError, match="RelativeL2Luminance, L1, RelativeL1, Mape, Smape, CrossEntropy, Variance"):
        tcnn.Loss("Huber")
    with pytest.raises(ValueError, match="dims"):
        tcnn.Loss("L2")(torch.zeros(4, 17, device="cuda", dtype=torch.float16), torch.zeros(4, 17, device="cuda"))
    with pytest.raises(RuntimeError, match="RelativeL2Luminance.*at least 3"):
        tcnn.Loss("RelativeL2Luminance")(view[:, :2], t_d[:, :2])
    with pytest.raises(ValueError, match="shape"):
        loss(view, t_d[:, :2])
    with pytest.raises(ValueError, match="fp16 or fp32"):
        loss(view.double(), t_d)


def _graph_bits(torch):
    """values and gradients of a few graphs, as bytes"""
    import tinycudann as tcnn
    out = {}
    for otype, dims, with_pdf in (("RelativeL2", 3, False), ("RelativeL2Luminance", 6, True), ("Smape", 16, True), ("CrossEntropy", 1, False)):
        n = 257
        pred16, tgt, pdf = _inputs(n, dims)
        t_d = torch.from_numpy(tgt.copy()).cuda()
        q_d = torch.from_numpy(pdf.copy()).cuda() if with_pdf else None
        leaf = _leaf16(torch, pred16)
        v = tcnn.Loss(otype)(leaf[:, :dims], t_d, q_d)
        (v * 0.37).backward()
        out[otype, "fp16"] = (_bits32(v).tobytes(), _bits16(leaf.grad).tobytes())
        leaf32 = torch.from_numpy(_inputs32(n, dims)[0].copy()).cuda().requires_grad_(True)
        v = tcnn.Loss(otype)(leaf32, t_d, q_d)
        (g,) = torch.autograd.grad(v, leaf32, create_graph=True)
        out[otype, "fp32"] = (_bits32(v).tobytes(), _bits32(g).tobytes())
    model, x, tgt = _model_batch(torch)
    v = tcnn.Loss("L1")(model(x), torch.from_numpy(tgt.copy()).cuda())
    v.backward()
    out["model"] = (_bits32(v).tobytes(), _bits16(model.params.grad.half()).tobytes())
    return out


def test_the_two_nodes_agree_bit_for_bit(torch_mod, monkeypatch):
    from tinycudann import modules
    if modules._EXT is None:
        pytest.fail("the C++ autograd node (lib/_tcnn_torch) is not built")
    cpp = _graph_bits(torch_mod)
    monkeypatch.setattr(modules, "_EXT", None)
    py = _graph_bits(torch_mod)
    assert cpp.keys() == py.keys()
    for k in cpp:
        assert cpp[k] == py[k], k
