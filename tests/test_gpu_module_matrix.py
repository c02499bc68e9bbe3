"""Module::forward + Module::backward with an external dL/dy on every MLP engine against the float64
reference (tests/mlp_reference.py): the path tinycudann.NetworkWithInputEncoding / Network train through.

It runs the kernel variants the Trainer tests never reach: the register-resident kernel's external-dL/dy
instantiations (with the kept SoA encoding, and recomputing), the tile kernel's output-activation
transfer of a caller's gradient, the layer-wise engine's copy + in-place transfer, and the fall-through
from the register kernel to the tile kernel when dL/dinput is requested. Cases, inputs and the CPU proof
of every bound: tests/module_matrix_cases.py, tests/test_mlp_reference.py.

Every case: create the module through the C-ABI, assert the kernel family it will run
(tcnn_module_backward_kernel, tcnn_module_inference_engine), assert that tcnn_module_initialize_params
gives the parameters the CPU proof used, forward, backward, then
  * outputs within 4 fp16 ulps of the output scale;
  * weight gradients per element and per matrix (8 fp16 ulps of the float64 abs-backprop magnitude + the
    fp16 rounding of the returned gradient), the failing matrix named;
  * dL/dinput per element in the same form -- for OneBlob through the CPU encoder's linear backward, for
    the grid only the existing relative-L2 bars (grid gradient 1e-3, dL/dx 2e-3: the grid's own backward
    is checked per element elsewhere);
  * the rows of the output matrix's gradient that belong to padded outputs are exactly zero;
  * relative L2 of the whole gradient and of dL/dinput (1e-3, 2e-3 for W128 / 5 layers / exponential-type
    outputs; the plain bars, also for the fp16 gradient) on unfiltered samples: the same run for smooth
    activations and None; branchy activations (ReLU, LeakyReLU) get the per-element checks on samples
    clear of the branches and this one on a second, unfiltered batch.
TCNN_MATRIX_RATIOS=<file> appends every case's worst ratios (profiles/module_matrix_ratios.txt).
"""
import ctypes
import json
import os

import numpy as np
import pytest

import mlp_reference as R
import module_matrix_cases as C
from helpers import rel_err
from oracle import oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available()
    from tinycudann import _lib as L
    return torch, L, L.lib(), torch.cuda.get_device_properties(0).multi_processor_count


def _vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _dump(case, kind, ratios):
    path = os.environ.get("TCNN_MATRIX_RATIOS")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"case": case.id, "B": case.B, "side": "gpu", "kind": kind, "ratios": ratios}) + "\n")


class Mod:
    """one C-ABI module of a case with the case's scaled fp16 parameters on the device"""

    def __init__(self, gpu, case):
        self.torch, self.L, self.lib, _ = gpu
        torch, L, lib = self.torch, self.L, self.lib
        self.case = case
        net = json.dumps(case.net).encode()
        if case.enc_cfg is None:
            self.m = L.check_ptr(lib.tcnn_create_network(case.n_in, case.n_out, net))
        else:
            self.m = L.check_ptr(lib.tcnn_create_network_with_input_encoding(case.n_in, case.n_out, json.dumps(case.enc_cfg).encode(), net))
        self.n = lib.tcnn_module_n_params(self.m)
        assert lib.tcnn_module_n_output_dims(self.m) == case.OUTP
        # a dispatch change cannot silently move the case to another kernel family
        assert lib.tcnn_module_backward_kernel(self.m, 0).decode() == case.kernel_nodx
        assert lib.tcnn_module_backward_kernel(self.m, 1).decode() == case.kernel_dx
        assert lib.tcnn_module_engine(self.m).decode() == ("layered" if case.kernel_dx == "layered" else "fused")
        assert lib.tcnn_module_inference_engine(self.m).decode() == ("layered" if case.kernel_dx == "layered" else "fused")
        # the parameters are the ones the CPU proof ran on
        p32 = torch.zeros(self.n, dtype=torch.float32, device="cuda")
        L.check(lib.tcnn_module_initialize_params(self.m, C.SEED, _vp(p32), 1.0))
        host = C.host_params32(case)
        np.testing.assert_array_equal(p32.cpu().numpy().view(np.uint32), host.view(np.uint32))
        self.p16 = C.scale_params16(case, host)
        self.p16_d = torch.from_numpy(self.p16.view(np.float16)).cuda()

    def close(self):
        self.lib.tcnn_module_destroy(self.m)

    def forward(self, x, prep):
        torch = self.torch
        x_d = torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()
        out = torch.empty(x.shape[0], self.case.OUTP, dtype=torch.float16, device="cuda")
        ctx = self.L.check_ptr(self.lib.tcnn_module_forward(self.m, None, x.shape[0], _vp(x_d), _vp(out), _vp(self.p16_d), int(prep)))
        return ctx, x_d, out

    def run(self, x, dout16, want_dx, other_x=None):
        """forward, backward. other_x: the backward gets the context of a forward on other_x, whose kept
        encoding it must not reuse (it recomputes). Returns (out, fp16 gradient as float64, dx or None)."""
        torch, L, lib, case = self.torch, self.L, self.lib, self.case
        B = x.shape[0]
        ctx, x_d, out = self.forward(x, want_dx)
        if other_x is not None:
            lib.tcnn_context_destroy(ctx)
            ctx, _keep_alive, _ = self.forward(other_x, want_dx)
        d_d = torch.from_numpy(dout16.view(np.float16)).cuda()
        grad = torch.full((self.n,), float("nan"), dtype=torch.float16, device="cuda")
        dx = torch.full((B, case.n_in), float("nan"), dtype=torch.float32, device="cuda") if want_dx else None
        try:
            L.check(lib.tcnn_module_backward(self.m, None, ctx, B, _vp(dx), _vp(d_d), _vp(grad), _vp(x_d), _vp(out), _vp(self.p16_d)))
            torch.cuda.synchronize()
        except Exception as e:  # a HIP error leaves the device unusable: end the session, run nothing more on it
            if any(k in str(e).lower() for k in ("illegal memory", "hip error", " failed: ")):
                pytest.exit(f"HIP error in {case.id}: {e}", returncode=3)
            raise
        lib.tcnn_context_destroy(ctx)
        return (out.float().cpu().numpy().astype(np.float64), grad.float().cpu().numpy().astype(np.float64),
                dx.cpu().numpy().astype(np.float64) if want_dx else None)


def _oneblob_dx_check(case, x, ref, dx, per_element):
    """dL/dx through OneBlob: the CPU encoder's backward (linear in dL/d(encoding)) of the reference's fp16
    dL/d(encoding); its per-element bound is the encoding bound carried through |d enc / d x|, plus the
    fp32 summation error of the IN-term sums on either side (2 IN 2^-24 of the terms' magnitude)."""
    nb = case.enc_cfg["n_bins"]
    dref = O.oneblob_bwd(x, nb, O.f2h(ref["dinput"].astype(np.float32))).astype(np.float64)
    if not per_element:
        return rel_err(dx, dref)
    J = C.oneblob_jacobian(case, x)
    b_enc = R.ULPS * 2.0 ** -10 * ref["mag_in"] + 2.0 ** -11 * np.abs(ref["dinput"]) + 2.0 ** -25
    bound = np.einsum("bj,bjd->bd", b_enc, J) + 2 * case.IN * 2.0 ** -24 * np.einsum("bj,bjd->bd", np.abs(ref["dinput"]), J) + 2.0 ** -25
    q = np.abs(dx - dref) / bound
    k = int(np.argmax(q))
    assert q.flat[k] <= 1.0, ("dinput (OneBlob)", float(q.flat[k]), k, dx.flat[k], dref.flat[k])
    return float(q.flat[k])


def _verify(case, p16, x, enc, dout, got, per_element, kind):
    """the assertions of one run (module docstring); returns and records the ratios"""
    out, grad, dx = got
    assert np.isfinite(grad).all() and (dx is None or np.isfinite(dx).all())  # every element written
    ref = C.reference(case, p16, enc, dout)
    denc, ref_in = None, ref
    if dx is not None and case.enc.startswith("identity"):  # Identity, scale 1: dL/dinput is dL/d(encoding) itself;
        denc = dx  # padding columns have no input behind them
        ref_in = dict(ref, dinput=ref["dinput"][:, :case.n_in], mag_in=ref["mag_in"][:, :case.n_in])
    ratios = C.check_against_reference(case, ref_in, out, grad[:case.n_mlp], denc, per_element, fp16_out=True)
    # padded outputs had zero dL/dy: their rows of the output matrix's gradient are exactly zero
    rows = grad[case.n_mlp - case.OUTP * (case.W if case.NH else case.IN):case.n_mlp].reshape(case.OUTP, -1)
    assert np.all(rows[case.n_out:] == 0.0)
    assert np.abs(rows[:case.n_out]).max() > 0.0
    bar = R.aggregate_bar(case.W, case.NH, case.out_act)
    if dx is not None and case.enc.startswith("oneblob"):
        if per_element:
            ratios["dinput"] = _oneblob_dx_check(case, x, ref, dx, True)
        if not (per_element and case.branchy):
            ratios["agg_in"] = _oneblob_dx_check(case, x, ref, dx, False)
            assert ratios["agg_in"] <= bar, ("dinput rel L2", ratios["agg_in"], bar)
    if case.enc in C.GRID_ENCS:  # the grid's own backward, unchanged by the case: the existing relative-L2 bars
        g = O.grid_cfg(C.GRID, case.n_in)
        denc_soa = np.ascontiguousarray(O.f2h(ref["dinput"].astype(np.float32)).T)
        e = rel_err(grad[case.n_mlp:], O.grid_bwd(g, x, denc_soa))
        assert e <= 1e-3, ("grid gradient rel L2", e)
        ratios["grid_rel"] = e
        if dx is not None:
            e = rel_err(dx, O.grid_bwd_input(g, x, p16[case.n_mlp:], denc_soa))
            assert e <= 2e-3, ("grid dL/dx rel L2", e)
            ratios["dx_rel"] = e
    _dump(case, kind, ratios)
    return ratios


def _run_case(gpu, case, want_dx, kinds=("per_element", "aggregate"), tag=""):
    """per element on (filtered, for a branchy case) samples; a branchy case also aggregate on unfiltered ones"""
    mod = Mod(gpu, case)
    try:
        if "per_element" in kinds:
            x, enc, dout = C.draw(case, mod.p16, filtered=case.branchy)
            _verify(case, mod.p16, x, enc, dout, mod.run(x, dout, want_dx), True, "per_element" + tag)
        if case.branchy and "aggregate" in kinds:
            x, enc, dout = C.draw(case, mod.p16, filtered=False)
            _verify(case, mod.p16, x, enc, dout, mod.run(x, dout, want_dx), False, "aggregate" + tag)
    finally:
        mod.close()


def _ids(cs):
    return [c.id for c in cs]


REGISTER = [c for c in C.CASES if c.group == "register"]
TILE = [c for c in C.CASES if c.group == "tile"]
LAYERED = [c for c in C.CASES if c.group == "layered"]


@pytest.mark.parametrize("case", REGISTER, ids=_ids(REGISTER))
def test_register_kernel_external_dout(gpu, case):
    """k_fused_train_grid<.., EXT, ENC>: the backward without dL/dinput reads the SoA encoding its forward
    kept; with the context of a forward on another input it recomputes the encoding (EXT alone). Both
    against float64."""
    mod = Mod(gpu, case)
    try:
        x, enc, dout = C.draw(case, mod.p16, filtered=case.branchy)
        other, _, _ = C.draw(case, mod.p16, filtered=False, seed=1)
        kept = mod.run(x, dout, False)
        _verify(case, mod.p16, x, enc, dout, kept, True, "per_element-kept")
        recomputed = mod.run(x, dout, False, other_x=other)
        _verify(case, mod.p16, x, enc, dout, recomputed, True, "per_element-recomputed")
        if case.branchy:
            x, enc, dout = C.draw(case, mod.p16, filtered=False)
            _verify(case, mod.p16, x, enc, dout, mod.run(x, dout, False), False, "aggregate-kept")
    finally:
        mod.close()


@pytest.mark.parametrize("case", REGISTER, ids=_ids(REGISTER))
def test_register_shapes_with_dinput_run_the_tile_kernel(gpu, case):
    """the same networks with dL/dinput requested leave the register kernel (Mod asserts "tile"); their
    parameter gradients are checked against float64, not against the register kernel's"""
    _run_case(gpu, case, True, tag="-dx")


@pytest.mark.parametrize("case", TILE, ids=_ids(TILE))
def test_tile_engine(gpu, case):
    _run_case(gpu, case, True)


@pytest.mark.parametrize("case", LAYERED, ids=_ids(LAYERED))
def test_layered_engine(gpu, case):
    _run_case(gpu, case, True)


@pytest.mark.parametrize("idx", range(8))
def test_uneven_persistent_loops(gpu, idx):
    """B = 256 (n_cu + 1): 32- or 64-sample tiles over n_cu or 2 n_cu workgroups, 32 FUSED_WAVES-sample
    iterations over (8 / FUSED_WAVES) n_cu blocks -- in each some workgroups take one tile more than the
    rest -- and launch_wgrad's ragged last chunk. Hidden None: per element; ReLU: aggregate."""
    case = C.uneven_cases(gpu[3])[idx]
    want_dx = case.kernel_nodx != "register"  # the register kernel runs only without dL/dinput
    _run_case(gpu, case, want_dx, kinds=("aggregate",) if case.branchy else ("per_element",), tag="-uneven")


TORCH = C.torch_cases()


@pytest.mark.parametrize("case", TORCH, ids=[c.id + f"-B{c.B}" for c in TORCH])
def test_torch_front_end(gpu, case):
    """tcnn.Network / tcnn.NetworkWithInputEncoding: loss (out.float() * c).sum(), params.grad and x.grad
    against the float64 reference of the B real rows. Module.forward pads B = 300 to 512 rows and slices the
    output to n_output_dims columns; the padded rows and columns must contribute nothing. The binding
    multiplies dL/dy by its loss scale (128, exact in fp16 for |c| <= 1) and divides the gradients by it:
    the reference runs on 128 c and is divided by 128 (module_matrix_cases.torch_reference)."""
    torch = gpu[0]
    import tinycudann as tcnn
    if case.enc_cfg is None:
        model = tcnn.Network(case.n_in, case.n_out, case.net, seed=C.SEED)
    else:
        model = tcnn.NetworkWithInputEncoding(case.n_in, case.n_out, case.enc_cfg, case.net, seed=C.SEED)
    nat = model.native_tcnn_module
    assert nat.backward_kernel(True) == case.kernel_dx
    host = C.host_params32(case)
    np.testing.assert_array_equal(model.params.detach().cpu().numpy().view(np.uint32), host.view(np.uint32))
    with torch.no_grad():
        model.params.mul_(case.scale)
    p16 = C.scale_params16(case, host)
    np.testing.assert_array_equal(model.params.detach().half().cpu().numpy().view(np.uint16), p16)
    s = float(model.loss_scale)
    assert s == 128.0
    for filtered in ((True, False) if case.branchy else (False,)):
        x, enc, dout = C.draw(case, p16, filtered=filtered)
        c16 = dout[:, :case.n_out]
        x_d = torch.from_numpy(x).cuda().requires_grad_(True)
        model.params.grad = None
        out = model(x_d)
        assert out.shape == (case.B, case.n_out) and out.dtype == torch.float16
        (out.float() * torch.from_numpy(O.h2f(c16)).cuda()).sum().backward()
        torch.cuda.synchronize()
        ref = C.torch_reference(case, p16, enc, dout, s)
        got_out = np.zeros((case.B, case.OUTP))
        got_out[:, :case.n_out] = out.detach().float().cpu().numpy()
        grad = model.params.grad.cpu().numpy().astype(np.float64)
        dx = x_d.grad.cpu().numpy().astype(np.float64)
        assert np.isfinite(grad).all() and np.isfinite(dx).all()
        per_element = filtered or not case.branchy
        if case.enc_cfg is None:
            ref_in = dict(ref, dinput=ref["dinput"][:, :case.n_in], mag_in=ref["mag_in"][:, :case.n_in])
            ratios = C.check_against_reference(case, ref_in, got_out, grad[:case.n_mlp], dx, per_element, fp16_out=True)
        else:
            ratios = C.check_against_reference(case, ref, got_out, grad[:case.n_mlp], None, per_element, fp16_out=True)
            if per_element:
                ratios["dinput"] = _oneblob_dx_check(case, x, ref, dx, True)
            if not (per_element and case.branchy):
                ratios["agg_in"] = _oneblob_dx_check(case, x, ref, dx, False)
                assert ratios["agg_in"] <= R.aggregate_bar(case.W, case.NH, case.out_act)
        _dump(case, ("per_element" if per_element else "aggregate") + f"-torch-B{case.B}", ratios)
