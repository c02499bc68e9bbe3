"""torch.nn front-end mirroring reference bindings/torch/tinycudann/modules.py:91-329 on top of the
C-ABI runtime module (include/tcnn_mi355x.h, which replaces reference src/cpp_api.cu +
bindings/torch/tinycudann/bindings.cpp).

Provenance: the autograd plumbing below (null-tensor conventions, `_module_function`,
`_module_function_backward`, `Module.forward`'s batch padding and the pickling hooks) follows the
reference's modules.py:81-204 (tiny-cuda-nn, Copyright (c) 2020-2022 NVIDIA CORPORATION, BSD-3-Clause)
closely on purpose: it is the plugin API whose exact behaviour -- loss-scale multiply/divide order,
null-tensor conventions, output slicing -- callers such as NeuralBTF depend on."""
import ctypes
import gc
import json
import os
import sys
import warnings

import torch

from tinycudann import _lib as L

if not torch.cuda.is_available():
    raise EnvironmentError("Unknown compute capability. Ensure PyTorch with ROCm support and an MI355X are available.")

PRECISION_FP32 = 0
PRECISION_FP16 = 1
LAYOUT_SOA = 15  # TCNN_LAYOUT_SOA_INPUT | _OUTPUT | _DL_DOUTPUT | _DL_DINPUT


class _C:
    """Stand-in for the reference's compiled `tinycudann._C` module-level functions
    (bindings.cpp:285-336), so scripts written against it (e.g. scripts/test_grid_bwdbwd.py,
    which imports `_C` from tinycudann.modules) run unchanged. Everything goes to the C-ABI."""

    class Precision:
        Fp32 = PRECISION_FP32
        Fp16 = PRECISION_FP16

    @staticmethod
    def preferred_precision():
        return L.lib().tcnn_preferred_precision()

    @staticmethod
    def batch_size_granularity():
        return L.lib().tcnn_batch_size_granularity()

    @staticmethod
    def default_loss_scale(precision):
        return L.lib().tcnn_default_loss_scale(precision)

    @staticmethod
    def free_temporary_memory():
        L.lib().tcnn_free_temporary_memory()

    @staticmethod
    def has_networks():
        return bool(L.lib().tcnn_has_networks())


def _torch_precision(p):
    return torch.half if p == PRECISION_FP16 else torch.float


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream(t=None):
    """the current stream of t's device (default: the current device) as a raw handle -- the binding's
    hot path makes a few of these calls per step, and torch.cuda.current_stream() builds a Stream object
    each time (the torch step is host-bound at 2^16 points, tools/torch_host_breakdown.py)"""
    if _raw_stream is not None:
        return _raw_stream(t.device.index if t is not None else torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return t.data_ptr() if t is not None else None  # ctypes converts the int for a c_void_p argument


_GRANULARITY = None

# The C++ autograd node (csrc/torch_ext.cpp, built in-tree next to the engine library): one pybind call per
# forward and a C++ backward. The Python autograd.Function below is the same node and stays the fallback
# (TCNN_TORCH_PY=1 selects it: A/B switch).
_EXT = None
if not os.environ.get("TCNN_TORCH_PY"):
    try:
        _libdir = os.path.dirname(L.LIB_PATH)
        if _libdir not in sys.path:
            sys.path.append(_libdir)
        import _tcnn_torch as _EXT  # noqa: E402
    except ImportError:
        _EXT = None


def _granularity():
    global _GRANULARITY
    if _GRANULARITY is None:
        _GRANULARITY = int(L.lib().tcnn_batch_size_granularity())
    return _GRANULARITY


def free_temporary_memory():
    gc.collect()
    L.lib().tcnn_free_temporary_memory()


class _NativeModule:
    """Python twin of bindings.cpp's Module class (bindings.cpp:75-171). A module's sizes and
    precisions are fixed at creation; they are read once here, so a training step makes no ctypes
    round trips for them (the torch step is host-bound: tools/torch_step_profile.py)."""

    def __init__(self, handle):
        self.h = L.check_ptr(handle)
        lib = L.lib()
        self._n_in = lib.tcnn_module_n_input_dims(self.h)
        self._n_out = lib.tcnn_module_n_output_dims(self.h)
        self._n_params = lib.tcnn_module_n_params(self.h)
        self._param_dtype = _torch_precision(lib.tcnn_module_param_precision(self.h))
        self._out_dtype = _torch_precision(lib.tcnn_module_output_precision(self.h))

    # bindings.cpp:306-313: sizes are methods on the native module, as in the reference
    def n_input_dims(self):
        return self._n_in

    def n_output_dims(self):
        return self._n_out

    def n_params(self):
        return self._n_params

    def __del__(self):
        try:
            L.lib().tcnn_module_destroy(self.h)
        except Exception:
            pass

    def param_precision(self):
        return L.lib().tcnn_module_param_precision(self.h)

    def output_precision(self):
        return L.lib().tcnn_module_output_precision(self.h)

    def hyperparams(self):
        return json.loads(L.lib().tcnn_module_hyperparams(self.h).decode())

    def name(self):
        return L.lib().tcnn_module_name(self.h).decode()

    def engine(self):
        """the engine training / backward runs on ("fused", "layered"; "encoding" for encodings)"""
        return L.lib().tcnn_module_engine(self.h).decode()

    def inference_engine(self):
        return L.lib().tcnn_module_inference_engine(self.h).decode()

    def backward_kernel(self, with_dinput):
        """the kernel family a backward runs, with or without dL/dinput: "register", "tile", "layered", "chain" (a
        fused fp32 network module; "encoding" for encodings)"""
        return L.lib().tcnn_module_backward_kernel(self.h, int(bool(with_dinput))).decode()

    def initial_params(self, seed):
        p = torch.zeros(self.n_params(), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        L.check(L.lib().tcnn_module_initialize_params(self.h, seed, _ptr(p), 1.0))
        return p

    def fwd(self, input, params):
        assert input.dtype == torch.float32 and input.is_contiguous() and input.shape[1] == self._n_in
        assert params.dtype == self._param_dtype and params.numel() == self._n_params
        B = input.shape[0]
        out = torch.empty(B, self._n_out, dtype=self._out_dtype, device=input.device)
        if not (input.requires_grad or params.requires_grad):
            L.check(L.lib().tcnn_module_inference(self.h, _stream(input), B, _ptr(input), _ptr(out), _ptr(params)))
            return None, out
        ctx = L.check_ptr(L.lib().tcnn_module_forward(self.h, _stream(input), B, _ptr(input), _ptr(out), _ptr(params),
                                                       int(input.requires_grad)))
        return _NativeContext(ctx), out

    def bwd_scaled(self, ctx, input, params, output, doutput, loss_scale, need_input, need_params):
        """the binding's first-order backward (modules.py:128-138 of the reference: doutput * loss_scale,
        Module::backward, dL/dinput and dL/dparams divided by loss_scale) as ONE engine call
        (tcnn_module_backward_scaled), with the same roundings as the three torch operations"""
        B = input.shape[0]
        dL_dinput = torch.empty_like(input) if need_input else None
        dL_dparams = torch.empty(self._n_params, dtype=self._param_dtype, device=input.device) if need_params else None
        if doutput.dtype != self._out_dtype:
            doutput = doutput.to(self._out_dtype)
        if not doutput.is_contiguous():
            doutput = doutput.contiguous()
        L.check(L.lib().tcnn_module_backward_scaled(self.h, _stream(input), ctx.h, B, _ptr(dL_dinput), _ptr(doutput),
                                                    _ptr(dL_dparams), _ptr(input), _ptr(output), _ptr(params),
                                                    float(loss_scale), 0))
        return dL_dinput, dL_dparams

    def bwd(self, ctx, input, params, output, dL_doutput):
        B = input.shape[0]
        dL_dinput = torch.empty_like(input) if input.requires_grad else None
        dL_dparams = torch.empty(self.n_params(), dtype=_torch_precision(self.param_precision()), device=input.device) if params.requires_grad else None
        dL_doutput = dL_doutput.to(_torch_precision(self.output_precision())).contiguous()
        L.check(L.lib().tcnn_module_backward(self.h, _stream(input), ctx.h, B, _ptr(dL_dinput), _ptr(dL_doutput),
                                             _ptr(dL_dparams), _ptr(input), _ptr(output), _ptr(params)))
        return dL_dinput, dL_dparams

    def fwd_soa(self, input, params, n_out):
        """the forward on batch-contiguous matrices (tcnn_module_forward_layout, every layout bit set): input
        [n_input_dims, B] -> output [n_out, B], n_out the unpadded n_output_dims"""
        assert input.dtype == torch.float32 and input.is_contiguous() and input.shape[0] == self._n_in
        assert params.dtype == self._param_dtype and params.numel() == self._n_params
        B = input.shape[1]
        out = torch.empty(n_out, B, dtype=self._out_dtype, device=input.device)
        if not (input.requires_grad or params.requires_grad):
            L.check(L.lib().tcnn_module_inference_layout(self.h, _stream(input), B, _ptr(input), _ptr(out), _ptr(params), LAYOUT_SOA))
            return None, out
        ctx = L.check_ptr(L.lib().tcnn_module_forward_layout(self.h, _stream(input), B, _ptr(input), _ptr(out), _ptr(params),
                                                              int(input.requires_grad), LAYOUT_SOA))
        return _NativeContext(ctx), out

    def bwd_soa(self, ctx, input, params, output, dL_doutput, need_input, need_params):
        """dL_doutput [n_out, B] -> dL_dinput [n_input_dims, B], dL_dparams"""
        B = input.shape[1]
        dL_dinput = torch.empty_like(input) if need_input else None
        dL_dparams = torch.empty(self._n_params, dtype=self._param_dtype, device=input.device) if need_params else None
        dL_doutput = dL_doutput.to(self._out_dtype).contiguous()
        L.check(L.lib().tcnn_module_backward_layout(self.h, _stream(input), ctx.h, B, _ptr(dL_dinput), _ptr(dL_doutput),
                                                    _ptr(dL_dparams), _ptr(input), _ptr(output), _ptr(params), LAYOUT_SOA))
        return dL_dinput, dL_dparams

    def jacobian(self, input, params, n_out, soa):
        """tcnn_module_inference_jacobian: input [B, D] -> (output [B, padded n_out], J [B, n_out, D]); soa: input
        [D, B] -> (output [n_out, B], J [n_out, D, B])"""
        assert input.dtype == torch.float32 and input.is_contiguous() and input.shape[0 if soa else 1] == self._n_in
        assert params.dtype == self._param_dtype and params.numel() == self._n_params
        B, D, dev = input.shape[1 if soa else 0], self._n_in, input.device
        out = torch.empty((n_out, B) if soa else (B, self._n_out), dtype=self._out_dtype, device=dev)
        jac = torch.empty((n_out, D, B) if soa else (B, n_out, D), dtype=torch.float32, device=dev)
        L.check(L.lib().tcnn_module_inference_jacobian(self.h, _stream(input), B, _ptr(input), _ptr(out), _ptr(jac), _ptr(params),
                                                       3 if soa else 0))
        return out, jac

    def jvp(self, input, directions, params, n_out, soa):
        """tcnn_module_inference_jvp: input [B, D], directions [B, K, D] or None (the unit vectors, K = D) ->
        (output [B, padded n_out], Jv [B, n_out, K]); soa: input [D, B], directions [K, D, B] -> (output [n_out, B],
        Jv [n_out, K, B])"""
        assert input.dtype == torch.float32 and input.is_contiguous() and input.shape[0 if soa else 1] == self._n_in
        assert params.dtype == self._param_dtype and params.numel() == self._n_params
        B, D, dev = input.shape[1 if soa else 0], self._n_in, input.device
        K = D if directions is None else directions.shape[0 if soa else 1]
        if directions is not None:
            assert directions.dtype == torch.float32 and directions.is_contiguous()
            assert tuple(directions.shape) == ((K, D, B) if soa else (B, K, D))
        out = torch.empty((n_out, B) if soa else (B, self._n_out), dtype=self._out_dtype, device=dev)
        jv = torch.empty((n_out, K, B) if soa else (B, n_out, K), dtype=torch.float32, device=dev)
        L.check(L.lib().tcnn_module_inference_jvp(self.h, _stream(input), B, _ptr(input), _ptr(directions), 0 if directions is None else K,
                                                  _ptr(out), _ptr(jv), _ptr(params), 3 if soa else 0))
        return out, jv

    def jvp_second(self, input, directions, params, n_out, soa):
        """tcnn_module_inference_jvp_second: jvp() and second [B, n_out] (soa: [n_out, B]) =
        sum_k v_k^T (d^2 output / d input^2) v_k in the same launch"""
        assert input.dtype == torch.float32 and input.is_contiguous() and input.shape[0 if soa else 1] == self._n_in
        assert params.dtype == self._param_dtype and params.numel() == self._n_params
        B, D, dev = input.shape[1 if soa else 0], self._n_in, input.device
        K = D if directions is None else directions.shape[0 if soa else 1]
        if directions is not None:
            assert directions.dtype == torch.float32 and directions.is_contiguous()
            assert tuple(directions.shape) == ((K, D, B) if soa else (B, K, D))
        out = torch.empty((n_out, B) if soa else (B, self._n_out), dtype=self._out_dtype, device=dev)
        jv = torch.empty((n_out, K, B) if soa else (B, n_out, K), dtype=torch.float32, device=dev)
        second = torch.empty((n_out, B) if soa else (B, n_out), dtype=torch.float32, device=dev)
        L.check(L.lib().tcnn_module_inference_jvp_second(self.h, _stream(input), B, _ptr(input), _ptr(directions),
                                                         0 if directions is None else K, _ptr(out), _ptr(jv), _ptr(second), _ptr(params),
                                                         3 if soa else 0))
        return out, jv, second

    def hessian(self, input, directions, params, n_out, soa):
        """tcnn_module_inference_hessian: jvp() and hessian [B, n_out, K, K] (soa: [n_out, K, K, B]) =
        v_k^T (d^2 output / d input^2) v_k' in the same launch"""
        assert input.dtype == torch.float32 and input.is_contiguous() and input.shape[0 if soa else 1] == self._n_in
        assert params.dtype == self._param_dtype and params.numel() == self._n_params
        B, D, dev = input.shape[1 if soa else 0], self._n_in, input.device
        K = D if directions is None else directions.shape[0 if soa else 1]
        if directions is not None:
            assert directions.dtype == torch.float32 and directions.is_contiguous()
            assert tuple(directions.shape) == ((K, D, B) if soa else (B, K, D))
        out = torch.empty((n_out, B) if soa else (B, self._n_out), dtype=self._out_dtype, device=dev)
        jv = torch.empty((n_out, K, B) if soa else (B, n_out, K), dtype=torch.float32, device=dev)
        hess = torch.empty((n_out, K, K, B) if soa else (B, n_out, K, K), dtype=torch.float32, device=dev)
        L.check(L.lib().tcnn_module_inference_hessian(self.h, _stream(input), B, _ptr(input), _ptr(directions),
                                                      0 if directions is None else K, _ptr(out), _ptr(jv), _ptr(hess), _ptr(params),
                                                      3 if soa else 0))
        return out, jv, hess

    def fwd_jvp(self, input, directions, params, n_out):
        """tcnn_module_forward_jvp: jvp() on AoS matrices, keeping a context for bwd_jvp"""
        B, D = input.shape[0], self._n_in
        K = D if directions is None else directions.shape[1]
        out = torch.empty(B, self._n_out, dtype=self._out_dtype, device=input.device)
        jv = torch.empty(B, n_out, K, dtype=torch.float32, device=input.device)
        ctx = L.check_ptr(L.lib().tcnn_module_forward_jvp(self.h, _stream(input), B, _ptr(input), _ptr(directions),
                                                           0 if directions is None else K, _ptr(out), _ptr(jv), _ptr(params)))
        return _NativeContext(ctx), out, jv

    def bwd_jvp(self, ctx, input, directions, params, dL_doutput, dL_djvp):
        """tcnn_module_backward_jvp: dL_doutput [B, padded n_out] and dL_djvp [B, n_out, K] (either None: zero) ->
        dL_dparams"""
        dL_dparams = torch.empty(self._n_params, dtype=self._param_dtype, device=input.device)
        L.check(L.lib().tcnn_module_backward_jvp(self.h, _stream(input), ctx.h, input.shape[0], _ptr(dL_doutput), _ptr(dL_djvp),
                                                 _ptr(dL_dparams), _ptr(input), _ptr(directions), _ptr(params)))
        return dL_dparams

    def fwd_jvp_second(self, input, directions, params, n_out):
        """tcnn_module_forward_jvp_second: jvp_second() on AoS matrices, keeping a context for bwd_jvp_second"""
        B, D = input.shape[0], self._n_in
        K = D if directions is None else directions.shape[1]
        out = torch.empty(B, self._n_out, dtype=self._out_dtype, device=input.device)
        jv = torch.empty(B, n_out, K, dtype=torch.float32, device=input.device)
        second = torch.empty(B, n_out, dtype=torch.float32, device=input.device)
        ctx = L.check_ptr(L.lib().tcnn_module_forward_jvp_second(self.h, _stream(input), B, _ptr(input), _ptr(directions),
                                                                  0 if directions is None else K, _ptr(out), _ptr(jv), _ptr(second),
                                                                  _ptr(params)))
        return _NativeContext(ctx), out, jv, second

    def bwd_jvp_second(self, ctx, input, directions, params, dL_doutput, dL_djvp, dL_dsecond):
        """tcnn_module_backward_jvp_second: dL_doutput [B, padded n_out], dL_djvp [B, n_out, K] and dL_dsecond [B, n_out]
        (any None: zero) -> dL_dparams"""
        dL_dparams = torch.empty(self._n_params, dtype=self._param_dtype, device=input.device)
        L.check(L.lib().tcnn_module_backward_jvp_second(self.h, _stream(input), ctx.h, input.shape[0], _ptr(dL_doutput), _ptr(dL_djvp),
                                                        _ptr(dL_dsecond), _ptr(dL_dparams), _ptr(input), _ptr(directions), _ptr(params)))
        return dL_dparams

    def bwd_bwd_input(self, ctx, input, params, dL_ddLdinput, dL_doutput):
        """bindings.cpp:185-239: second-order gradients from dL/d(dL/dinput)."""
        B = input.shape[0]
        dev = input.device
        dL_ddLdoutput = (torch.zeros(B, self.n_output_dims(), dtype=_torch_precision(self.output_precision()), device=dev)
                         if dL_doutput.requires_grad else None)
        dL_dparams = (torch.zeros(self.n_params(), dtype=_torch_precision(self.param_precision()), device=dev)
                      if params.requires_grad else None)
        dL_dinput = torch.zeros(B, self.n_input_dims(), dtype=torch.float32, device=dev) if input.requires_grad else None
        if dL_doutput.requires_grad or params.requires_grad:
            dL_ddLdinput = dL_ddLdinput.to(torch.float32).contiguous()
            dout = dL_doutput.detach().to(_torch_precision(self.output_precision())).contiguous()
            L.check(L.lib().tcnn_module_backward_backward_input(
                self.h, _stream(input), ctx.h, B, _ptr(dL_ddLdinput), _ptr(input),
                _ptr(dout) if (params.requires_grad or input.requires_grad) else None,
                _ptr(dL_dparams), _ptr(dL_ddLdoutput), _ptr(dL_dinput), _ptr(params)))
        return dL_ddLdoutput, dL_dparams, dL_dinput


class _NativeContext:
    def __init__(self, h):
        self.h = h

    def __del__(self):
        try:
            L.lib().tcnn_context_destroy(self.h)
        except Exception:
            pass


def null_tensor_like(tensor):
    return torch.empty([], dtype=tensor.dtype, device=tensor.device)


def null_tensor_to_none(tensor):
    if len(tensor.shape) == 0:
        return None
    return tensor


class _module_function(torch.autograd.Function):
    @staticmethod
    def forward(ctx, native_tcnn_module, input, params, loss_scale):
        ctx.set_materialize_grads(False)
        native_ctx, output = native_tcnn_module.fwd(input, params)
        ctx.save_for_backward(input, params, output)
        ctx.native_tcnn_module = native_tcnn_module
        ctx.native_ctx = native_ctx
        ctx.loss_scale = loss_scale
        return output

    @staticmethod
    def backward(ctx, doutput):
        if doutput is None:
            return None, None, None, None
        if not doutput.is_cuda:
            warnings.warn("doutput must be a CUDA tensor, but isn't. This indicates suboptimal performance.")
            doutput = doutput.cuda()
        input, params, output = ctx.saved_tensors
        if not torch.is_grad_enabled():
            # a first-order backward (no create_graph): nothing will differentiate the gradients, so the
            # differentiable wrapper below and its torch scaling ops are skipped -- one engine call, same values
            if doutput.dtype != output.dtype:
                doutput = doutput.to(output.dtype)  # the binding's doutput * loss_scale has the output's dtype
            input_grad, params_grad = ctx.native_tcnn_module.bwd_scaled(
                ctx.native_ctx, input, params, output, doutput, ctx.loss_scale, ctx.needs_input_grad[1], ctx.needs_input_grad[2])
            return None, input_grad, params_grad, None
        input_grad, params_grad = _module_function_backward.apply(ctx, doutput, input, params, output)
        return None, null_tensor_to_none(input_grad), null_tensor_to_none(params_grad), None


class _module_function_backward(torch.autograd.Function):
    """modules.py:128-170 of the reference: the backward as a differentiable function, so that
    d(dL/dinput)/d(doutput, params, input) flows through Module.bwd_bwd_input."""

    @staticmethod
    def forward(ctx, ctx_fwd, doutput, input, params, output):
        ctx.ctx_fwd = ctx_fwd
        ctx.save_for_backward(input, params, doutput)
        with torch.no_grad():
            scaled_grad = doutput * ctx_fwd.loss_scale
            input_grad, params_grad = ctx_fwd.native_tcnn_module.bwd(ctx_fwd.native_ctx, input, params, output, scaled_grad)
            input_grad = null_tensor_like(input) if input_grad is None else (input_grad / ctx_fwd.loss_scale)
            params_grad = null_tensor_like(params) if params_grad is None else (params_grad / ctx_fwd.loss_scale)
        return input_grad, params_grad

    @staticmethod
    def backward(ctx, dinput_grad, dparams_grad):
        input, params, doutput = ctx.saved_tensors
        if dinput_grad is None:
            return None, None, None, None, None
        with torch.enable_grad():
            doutput = doutput * ctx.ctx_fwd.loss_scale
        with torch.no_grad():
            doutput_grad, params_grad, input_grad = ctx.ctx_fwd.native_tcnn_module.bwd_bwd_input(
                ctx.ctx_fwd.native_ctx, input, params, dinput_grad, doutput)
            params_grad = None if params_grad is None else (params_grad / ctx.ctx_fwd.loss_scale)
            input_grad = None if input_grad is None else (input_grad / ctx.ctx_fwd.loss_scale)
        return None, doutput_grad, input_grad, params_grad, None


class _module_function_soa(torch.autograd.Function):
    """_module_function on batch-contiguous matrices (Module.forward(x, layout="soa")): first order only, a double
    backward raises (once_differentiable)."""

    @staticmethod
    def forward(ctx, native_tcnn_module, input, params, loss_scale, n_out):
        ctx.set_materialize_grads(False)
        native_ctx, output = native_tcnn_module.fwd_soa(input, params, n_out)
        ctx.save_for_backward(input, params, output)
        ctx.native_tcnn_module = native_tcnn_module
        ctx.native_ctx = native_ctx
        ctx.loss_scale = loss_scale
        return output

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, doutput):
        if doutput is None:
            return None, None, None, None, None
        input, params, output = ctx.saved_tensors
        input_grad, params_grad = ctx.native_tcnn_module.bwd_soa(
            ctx.native_ctx, input, params, output, doutput.to(output.dtype) * ctx.loss_scale, ctx.needs_input_grad[1], ctx.needs_input_grad[2])
        input_grad = None if input_grad is None else input_grad / ctx.loss_scale
        params_grad = None if params_grad is None else params_grad / ctx.loss_scale
        return None, input_grad, params_grad, None, None


class _jvp_function(torch.autograd.Function):
    """value_and_jvp / value_and_jacobian with differentiable=True: the output and the product carry a graph to the
    parameters (tcnn_module_forward_jvp / tcnn_module_backward_jvp). First order, parameters only."""

    @staticmethod
    def forward(ctx, native_tcnn_module, input, directions, params, n_out):
        ctx.set_materialize_grads(False)
        native_ctx, output, jv = native_tcnn_module.fwd_jvp(input, directions, params, n_out)
        ctx.save_for_backward(input, params)
        ctx.directions = directions
        ctx.native_tcnn_module = native_tcnn_module
        ctx.native_ctx = native_ctx
        return output, jv

    @staticmethod
    def backward(ctx, doutput, djv):
        if torch.is_grad_enabled():
            raise ValueError("value_and_jvp(differentiable=True) is differentiable once: a double backward through it "
                             "(create_graph=True) is not implemented")
        if doutput is None and djv is None:
            return None, None, None, None, None
        input, params = ctx.saved_tensors
        doutput = None if doutput is None else doutput.to(torch.float32).contiguous()
        djv = None if djv is None else djv.to(torch.float32).contiguous()
        params_grad = ctx.native_tcnn_module.bwd_jvp(ctx.native_ctx, input, ctx.directions, params, doutput, djv)
        return None, None, None, params_grad, None


class _jvp_second_function(torch.autograd.Function):
    """value_jvp_and_second / value_jacobian_and_laplacian with differentiable=True: the output, the product and the
    second-order sum carry a graph to the parameters (tcnn_module_forward_jvp_second /
    tcnn_module_backward_jvp_second). First order, parameters only."""

    @staticmethod
    def forward(ctx, native_tcnn_module, input, directions, params, n_out):
        ctx.set_materialize_grads(False)
        native_ctx, output, jv, second = native_tcnn_module.fwd_jvp_second(input, directions, params, n_out)
        ctx.save_for_backward(input, params)
        ctx.directions = directions
        ctx.native_tcnn_module = native_tcnn_module
        ctx.native_ctx = native_ctx
        return output, jv, second

    @staticmethod
    def backward(ctx, doutput, djv, dsecond):
        if torch.is_grad_enabled():
            raise ValueError("value_jvp_and_second(differentiable=True) is differentiable once: a double backward through it "
                             "(create_graph=True) is not implemented")
        if doutput is None and djv is None and dsecond is None:
            return None, None, None, None, None
        input, params = ctx.saved_tensors
        doutput, djv, dsecond = (None if t is None else t.to(torch.float32).contiguous() for t in (doutput, djv, dsecond))
        params_grad = ctx.native_tcnn_module.bwd_jvp_second(ctx.native_ctx, input, ctx.directions, params, doutput, djv, dsecond)
        return None, None, None, params_grad, None


class Module(torch.nn.Module):
    def __init__(self, seed=1337):
        super().__init__()
        self.native_tcnn_module = self._native_tcnn_module()
        self.dtype = _torch_precision(self.native_tcnn_module.param_precision())
        self.seed = seed
        initial_params = self.native_tcnn_module.initial_params(seed)
        self.params = torch.nn.Parameter(initial_params, requires_grad=True)
        self.register_parameter(name="params", param=self.params)
        self.loss_scale = L.lib().tcnn_default_loss_scale(self.native_tcnn_module.param_precision())

    def forward(self, x, layout="aos"):
        """layout="aos" (the default, the reference's call): x [B, n_input_dims] -> [B, n_output_dims].
        layout="soa": batch-contiguous matrices, x [n_input_dims, B] -> [n_output_dims, B], and in the backward a
        [n_output_dims, B] dL/doutput -> a [n_input_dims, B] dL/dinput, with no padded output columns anywhere. Served
        by fp32 FullyFusedMLP network modules (dtype=torch.float32); first order only (a double backward raises)."""
        if layout == "soa":
            return self._forward_soa(x)
        if layout != "aos":
            raise ValueError(f"layout must be 'aos' or 'soa', got {layout!r}")
        if not x.is_cuda:
            warnings.warn("input must be a CUDA tensor, but isn't. This indicates suboptimal performance.")
            x = x.cuda()
        batch_size = x.shape[0]
        g = _granularity()
        padded = (batch_size + g - 1) // g * g
        x_padded = x if batch_size == padded else torch.nn.functional.pad(x, [0, 0, 0, padded - batch_size])
        if x_padded.dtype != torch.float:
            x_padded = x_padded.to(torch.float)
        if not x_padded.is_contiguous():
            x_padded = x_padded.contiguous()
        params = self.params
        pdtype = self.native_tcnn_module._param_dtype
        if params.dtype != pdtype:
            params = params.to(pdtype)
        if not params.is_contiguous():
            params = params.contiguous()
        if _EXT is not None:
            output = _EXT.module_apply(self.native_tcnn_module.h, self.native_tcnn_module, x_padded, params, float(self.loss_scale))
        else:
            output = _module_function.apply(self.native_tcnn_module, x_padded, params, self.loss_scale)
        if batch_size == padded and output.shape[1] == self.n_output_dims:
            return output
        return output[:batch_size, :self.n_output_dims]

    def _forward_soa(self, x):
        if not x.is_cuda:
            warnings.warn("input must be a CUDA tensor, but isn't. This indicates suboptimal performance.")
            x = x.cuda()
        batch_size = x.shape[1]
        g = _granularity()
        padded = (batch_size + g - 1) // g * g
        if batch_size != padded:
            x = torch.nn.functional.pad(x, [0, padded - batch_size])
        x = x.to(torch.float).contiguous()
        params = self.params.to(self.native_tcnn_module._param_dtype).contiguous()
        output = _module_function_soa.apply(self.native_tcnn_module, x, params, self.loss_scale, self.n_output_dims)
        return output if batch_size == padded else output[:, :batch_size]

    def value_and_jacobian(self, x, layout="aos", differentiable=False):
        """f(x) and its input Jacobian at inference, in one forward-mode launch that keeps nothing:
        layout="aos": x [B, n_input_dims] -> (y [B, n_output_dims], J [B, n_output_dims, n_input_dims]);
        layout="soa": x [n_input_dims, B] -> (y [n_output_dims, B], J [n_output_dims, n_input_dims, B]),
        with J[b, o, d] = dy_o / dx_d and y the bits forward(x) returns. Inference only: no autograd graph is recorded,
        the results do not require grad and gradients do not flow through this call to x or to the parameters (use
        forward and autograd.grad for that). Served by fp32 FullyFusedMLP modules (dtype=torch.float32): a Network, or
        a NetworkWithInputEncoding behind a lone Identity encoding or behind a lone grid encoding (the latter through
        tcnn_module_inference_jvp with the unit directions); every activation but Sine.
        differentiable=True: as value_and_jvp."""
        if differentiable:
            return self._value_and_jvp_differentiable(x, None, layout)
        return self._value_and_jvp(x, None, layout, unit_call=self._grid_in_front())

    def _value_and_jvp_differentiable(self, x, v, layout, second=False):
        """v [B, K, D] or None (the unit vectors): (y, Jv [B, n_output_dims, K]) with a graph to the parameters; second:
        and q [B, n_output_dims]"""
        if layout != "aos":
            raise ValueError(f"differentiable=True serves layout='aos' only (batch-contiguous matrices are not implemented), got {layout!r}")
        if x.requires_grad or (v is not None and v.requires_grad):
            raise ValueError("differentiable=True produces the gradient of the parameters only: dL/dx and dL/dv are not implemented, "
                             "so x and v must not require grad (detach them, or use forward and autograd.grad)")
        if not x.is_cuda:
            warnings.warn("input must be a CUDA tensor, but isn't. This indicates suboptimal performance.")
            x = x.cuda()
        batch_size = x.shape[0]
        if v is not None and v.shape[0] != batch_size:
            raise ValueError(f"v has another batch size than x: {tuple(v.shape)}")
        padded = (batch_size + 255) // 256 * 256  # the reverse pass runs whole 256-row granules

        def prepare(t):
            if batch_size != padded:
                t = torch.nn.functional.pad(t, [0, 0] * (t.dim() - 1) + [0, padded - batch_size])
            return t.to(torch.float).contiguous()

        params = self.params.to(self.native_tcnn_module._param_dtype).contiguous()
        if second:
            y, jv, q = _jvp_second_function.apply(self.native_tcnn_module, prepare(x), None if v is None else prepare(v.to(x.device)),
                                                  params, self.n_output_dims)
            return y[:batch_size, :self.n_output_dims], jv[:batch_size], q[:batch_size]
        y, jv = _jvp_function.apply(self.native_tcnn_module, prepare(x), None if v is None else prepare(v.to(x.device)), params,
                                    self.n_output_dims)
        return y[:batch_size, :self.n_output_dims], jv[:batch_size]

    def value_and_jvp(self, x, v, layout="aos", differentiable=False):
        """f(x) and directional input derivatives (Jacobian-vector products) at inference, in one forward-mode launch
        that keeps nothing (tcnn_module_inference_jvp):
        layout="aos": x [B, n_input_dims], v [B, n_input_dims] -> (y [B, n_output_dims], Jv [B, n_output_dims]), or
                      v [B, K, n_input_dims] -> Jv [B, n_output_dims, K];
        layout="soa": x [n_input_dims, B], v [n_input_dims, B] -> (y [n_output_dims, B], Jv [n_output_dims, B]), or
                      v [K, n_input_dims, B] -> Jv [n_output_dims, K, B],
        with Jv[b, o, k] = sum_d dy_o / dx_d v[b, k, d] and y the bits forward(x) returns. Inference only, as
        value_and_jacobian. Served by the modules value_and_jacobian serves.
        differentiable=True (opt-in; the default is the call above, bit for bit): y and Jv carry the same bits and an
        autograd graph to the parameters, so a loss on the value and on the derivative trains the module in one keeping
        forward and one reverse pass (tcnn_module_forward_jvp / tcnn_module_backward_jvp). layout="aos" only, at most 3
        directions (1 at width 128; the Jacobian counts as n_input_dims), gradients for the parameters only: x or v
        requiring grad, layout="soa" and a double backward each raise a ValueError."""
        if v.dim() not in (2, 3):
            raise ValueError(f"v must be [B, D] or [B, K, D] ([D, B] or [K, D, B] for layout='soa'), got {tuple(v.shape)}")
        if differentiable:
            y, jv = self._value_and_jvp_differentiable(x, v if v.dim() == 3 else v.unsqueeze(1), layout)
            return y, (jv if v.dim() == 3 else jv.squeeze(2))
        y, jv = self._value_and_jvp(x, v if v.dim() == 3 else v.unsqueeze(0 if layout == "soa" else 1), layout, unit_call=False)
        return y, (jv if v.dim() == 3 else jv.squeeze(1 if layout == "soa" else 2))

    def _grid_in_front(self):
        """a grid encoding stands alone in front of the network"""
        return self.native_tcnn_module.hyperparams().get("encoding", {}).get("otype") == "Grid"

    def _value_and_jvp(self, x, v, layout, unit_call):
        """v None: the Jacobian, from tcnn_module_inference_jvp with null directions when unit_call, else from
        tcnn_module_inference_jacobian"""
        if layout not in ("aos", "soa"):
            raise ValueError(f"layout must be 'aos' or 'soa', got {layout!r}")
        soa = layout == "soa"
        with torch.no_grad():
            if not x.is_cuda:
                warnings.warn("input must be a CUDA tensor, but isn't. This indicates suboptimal performance.")
                x = x.cuda()
            batch_size = x.shape[1 if soa else 0]
            g = _granularity()
            padded = (batch_size + g - 1) // g * g

            def prepare(t):
                if batch_size != padded:
                    t = torch.nn.functional.pad(t, [0, padded - batch_size] if soa else [0, 0] * (t.dim() - 1) + [0, padded - batch_size])
                return t.to(torch.float).contiguous()

            x = prepare(x)
            params = self.params.detach().to(self.native_tcnn_module._param_dtype).contiguous()
            if v is None and not unit_call:
                y, jac = self.native_tcnn_module.jacobian(x, params, self.n_output_dims, soa)
            else:
                if v is not None and v.shape[2 if soa else 0] != batch_size:
                    raise ValueError(f"v has another batch size than x: {tuple(v.shape)}")
                y, jac = self.native_tcnn_module.jvp(x, None if v is None else prepare(v.to(x.device)), params, self.n_output_dims, soa)
            if soa:
                return (y, jac) if batch_size == padded else (y[:, :batch_size], jac[:, :, :batch_size])
            return y[:batch_size, :self.n_output_dims], jac[:batch_size]

    def value_jvp_and_second(self, x, v=None, layout="aos", differentiable=False):
        """value_and_jvp and the summed second directional derivatives, in one forward-mode launch that keeps nothing
        (tcnn_module_inference_jvp_second, the "forward Laplacian"):
        layout="aos": x [B, n_input_dims], v [B, K, n_input_dims] -> (y [B, n_output_dims], Jv [B, n_output_dims, K],
                      q [B, n_output_dims]);
        layout="soa": x [n_input_dims, B], v [K, n_input_dims, B] -> (y [n_output_dims, B], Jv [n_output_dims, K, B],
                      q [n_output_dims, B]),
        with q[b, o] = sum_k v[b, k]^T (d^2 y_o / dx^2) v[b, k]; y and Jv are value_and_jvp's bits. A v of [B, D] ([D, B])
        is one direction, K = 1: q is the curvature along it and Jv drops the K axis. v=None: the unit vectors, Jv the
        Jacobian and q the Laplacian. Inference only, as value_and_jacobian; served by the modules it serves.
        differentiable=True (opt-in; the default is the call above, bit for bit): y, Jv and q carry the same bits and an
        autograd graph to the parameters, so a loss on the Laplacian (a Poisson residual, a curvature term) trains the
        module in one keeping forward and one reverse pass (tcnn_module_forward_jvp_second /
        tcnn_module_backward_jvp_second). layout="aos" only, at most 3 directions (the Laplacian counts as
        n_input_dims), widths 16, 32 and 64, gradients for the parameters only: x or v requiring grad, layout="soa" and
        a double backward each raise a ValueError."""
        if layout not in ("aos", "soa"):
            raise ValueError(f"layout must be 'aos' or 'soa', got {layout!r}")
        if v is not None and v.dim() not in (2, 3):
            raise ValueError(f"v must be [B, D] or [B, K, D] ([D, B] or [K, D, B] for layout='soa'), got {tuple(v.shape)}")
        soa = layout == "soa"
        one = v is not None and v.dim() == 2
        if one:
            v = v.unsqueeze(0 if soa else 1)
        if differentiable:
            y, jv, q = self._value_and_jvp_differentiable(x, v, layout, second=True)
            return y, (jv.squeeze(2) if one else jv), q
        with torch.no_grad():
            if not x.is_cuda:
                warnings.warn("input must be a CUDA tensor, but isn't. This indicates suboptimal performance.")
                x = x.cuda()
            batch_size = x.shape[1 if soa else 0]
            if v is not None and v.shape[2 if soa else 0] != batch_size:
                raise ValueError(f"v has another batch size than x: {tuple(v.shape)}")
            g = _granularity()
            padded = (batch_size + g - 1) // g * g

            def prepare(t):
                if batch_size != padded:
                    t = torch.nn.functional.pad(t, [0, padded - batch_size] if soa else [0, 0] * (t.dim() - 1) + [0, padded - batch_size])
                return t.to(torch.float).contiguous()

            params = self.params.detach().to(self.native_tcnn_module._param_dtype).contiguous()
            y, jv, q = self.native_tcnn_module.jvp_second(prepare(x), None if v is None else prepare(v.to(x.device)), params,
                                                          self.n_output_dims, soa)
            if soa:
                y, jv, q = y[:, :batch_size], jv[:, :, :batch_size], q[:, :batch_size]
            else:
                y, jv, q = y[:batch_size, :self.n_output_dims], jv[:batch_size], q[:batch_size]
            return y, (jv.squeeze(1 if soa else 2) if one else jv), q

    def value_jacobian_and_laplacian(self, x, layout="aos", differentiable=False):
        """value_jvp_and_second with the unit vectors: (y, J [B, n_output_dims, n_input_dims], the Laplacian
        sum_d d^2 y_o / dx_d^2 [B, n_output_dims]); layout="soa": J [n_output_dims, n_input_dims, B], [n_output_dims, B].
        differentiable=True: as value_jvp_and_second."""
        return self.value_jvp_and_second(x, None, layout, differentiable)

    def value_jvp_and_hessian(self, x, v=None, layout="aos"):
        """value_and_jvp and every second directional derivative, in one forward-mode launch that keeps nothing
        (tcnn_module_inference_hessian):
        layout="aos": x [B, n_input_dims], v [B, K, n_input_dims] -> (y [B, n_output_dims], Jv [B, n_output_dims, K],
                      H [B, n_output_dims, K, K]);
        layout="soa": x [n_input_dims, B], v [K, n_input_dims, B] -> (y [n_output_dims, B], Jv [n_output_dims, K, B],
                      H [n_output_dims, K, K, B]),
        with H[b, o, k, l] = v[b, k]^T (d^2 y_o / dx^2) v[b, l], symmetric to the bit; y and Jv are value_and_jvp's bits
        and H[b, o, k, k] is value_jvp_and_second's q for v[:, k] alone. K <= 3. v=None: the unit vectors, Jv the
        Jacobian and H the input Hessian d^2 y_o / dx_d dx_e (n_input_dims <= 3). Inference only, as
        value_and_jacobian: no graph is recorded. Served by the modules value_jvp_and_second serves."""
        if layout not in ("aos", "soa"):
            raise ValueError(f"layout must be 'aos' or 'soa', got {layout!r}")
        if v is not None and v.dim() != 3:
            raise ValueError(f"v must be [B, K, D] ([K, D, B] for layout='soa'), got {tuple(v.shape)}")
        soa = layout == "soa"
        with torch.no_grad():
            if not x.is_cuda:
                warnings.warn("input must be a CUDA tensor, but isn't. This indicates suboptimal performance.")
                x = x.cuda()
            batch_size = x.shape[1 if soa else 0]
            if v is not None and v.shape[2 if soa else 0] != batch_size:
                raise ValueError(f"v has another batch size than x: {tuple(v.shape)}")
            g = _granularity()
            padded = (batch_size + g - 1) // g * g

            def prepare(t):
                if batch_size != padded:
                    t = torch.nn.functional.pad(t, [0, padded - batch_size] if soa else [0, 0] * (t.dim() - 1) + [0, padded - batch_size])
                return t.to(torch.float).contiguous()

            params = self.params.detach().to(self.native_tcnn_module._param_dtype).contiguous()
            y, jv, h = self.native_tcnn_module.hessian(prepare(x), None if v is None else prepare(v.to(x.device)), params,
                                                       self.n_output_dims, soa)
            if soa:
                return y[:, :batch_size], jv[:, :, :batch_size], h[..., :batch_size]
            return y[:batch_size, :self.n_output_dims], jv[:batch_size], h[:batch_size]

    def value_jacobian_and_hessian(self, x, layout="aos"):
        """value_jvp_and_hessian with the unit vectors: (y, J [B, n_output_dims, n_input_dims], the input Hessian
        [B, n_output_dims, n_input_dims, n_input_dims]); layout="soa": J [n_output_dims, n_input_dims, B],
        [n_output_dims, n_input_dims, n_input_dims, B]."""
        return self.value_jvp_and_hessian(x, None, layout)

    def __getstate__(self):
        """modules.py:194-199: pickle everything except the native module (a C-ABI handle)."""
        state = self.__dict__.copy()
        del state["native_tcnn_module"]
        return state

    def __setstate__(self, state):
        """modules.py:201-204: rebuild the native module from the stored configuration."""
        self.__dict__.update(state)
        self.native_tcnn_module = self._native_tcnn_module()

    def extra_repr(self):
        return (f"n_input_dims={self.n_input_dims}, n_output_dims={self.n_output_dims}, seed={self.seed}, "
                f"dtype={self.dtype}, hyperparams={self.native_tcnn_module.hyperparams()}")


def _network_precision(dtype, who):
    """dtype=None / torch.float16: the fp16 module; torch.float32: the fp32 module (parameters, output and
    gradients fp32, f32 matrix-core kernels)"""
    if dtype is None or dtype == torch.float16:
        return PRECISION_FP16
    if dtype == torch.float32:
        return PRECISION_FP32
    raise ValueError(f"{who} only supports fp32 or fp16 precision, but got {dtype}")


class NetworkWithInputEncoding(Module):
    def __init__(self, n_input_dims, n_output_dims, encoding_config, network_config, seed=1337, dtype=None):
        if not _C.has_networks():
            raise RuntimeError("Cannot create `NetworkWithInputEncoding` because tiny-cuda-nn was not compiled with neural network support.")
        self.n_input_dims = n_input_dims
        self.n_output_dims = n_output_dims
        self.encoding_config = encoding_config
        self.network_config = network_config
        self.precision = _network_precision(dtype, "NetworkWithInputEncoding")
        super().__init__(seed=seed)

    def _native_tcnn_module(self):
        enc, net = json.dumps(self.encoding_config).encode(), json.dumps(self.network_config).encode()
        if getattr(self, "precision", PRECISION_FP16) == PRECISION_FP16:  # (a pickle from before `precision`: fp16)
            return _NativeModule(L.lib().tcnn_create_network_with_input_encoding(self.n_input_dims, self.n_output_dims, enc, net))
        return _NativeModule(L.lib().tcnn_create_network_with_input_encoding_precision(
            self.n_input_dims, self.n_output_dims, enc, net, self.precision))


class Network(Module):
    def __init__(self, n_input_dims, n_output_dims, network_config, seed=1337, dtype=None):
        if not _C.has_networks():
            raise RuntimeError("Cannot create `Network` because tiny-cuda-nn was not compiled with neural network support.")
        self.n_input_dims = n_input_dims
        self.n_output_dims = n_output_dims
        self.network_config = network_config
        self.precision = _network_precision(dtype, "Network")
        super().__init__(seed=seed)

    def _native_tcnn_module(self):
        net = json.dumps(self.network_config).encode()
        if getattr(self, "precision", PRECISION_FP16) == PRECISION_FP16:
            return _NativeModule(L.lib().tcnn_create_network(self.n_input_dims, self.n_output_dims, net))
        return _NativeModule(L.lib().tcnn_create_network_precision(self.n_input_dims, self.n_output_dims, net, self.precision))


class Encoding(Module):
    def __init__(self, n_input_dims, encoding_config, seed=1337, dtype=None):
        self.n_input_dims = n_input_dims
        self.encoding_config = encoding_config
        if dtype is None:
            self.precision = _C.preferred_precision()
        elif dtype == torch.float16:
            self.precision = PRECISION_FP16
        elif dtype == torch.float32:
            self.precision = PRECISION_FP32
        else:
            raise ValueError(f"Encoding only supports fp32 or fp16 precision, but got {dtype}")
        super().__init__(seed=seed)
        self.n_output_dims = self.native_tcnn_module.n_output_dims()

    def _native_tcnn_module(self):
        return _NativeModule(L.lib().tcnn_create_encoding(self.n_input_dims, json.dumps(self.encoding_config).encode(),
                                                           self.precision))
