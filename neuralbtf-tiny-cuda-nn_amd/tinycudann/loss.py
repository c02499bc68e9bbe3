"""tinycudann.Loss: the engine's nine losses (csrc/loss_device.h; reference src/loss.cu:57-65) as a torch
module over the C-ABI's tcnn_loss_forward / tcnn_loss_backward (csrc/loss_torch.hip).

    loss = tinycudann.Loss("RelativeL2")
    value = loss(model(x), target)          # 0-dim fp32 tensor on the GPU, the reference's total
    value.backward()                        # the reference's gradient, normalisers held fixed

The value is summed on the device in a fixed order (bit-reproducible) and nothing is read back. The gradient
takes the incoming grad_output as the reference's loss_scale, read from device memory by the kernel. The
autograd node is the C++ one of csrc/torch_ext.cpp when it is built; the Python node below is the same node
over ctypes and the fallback (selected as tinycudann.Module's is: extension missing, or TCNN_TORCH_PY=1).
"""
import torch

from tinycudann import _lib as L

MAX_DIMS = 16
_FLOAT_DTYPES = (torch.float16, torch.float32)


def _modules():
    from tinycudann import modules  # raises without a GPU, as the reference does at import time
    return modules


def _loss_grad(loss_type, grad_output, pred, target, pdf):
    M = _modules()
    if grad_output.dtype != torch.float32 or grad_output.device != pred.device:
        grad_output = grad_output.to(device=pred.device, dtype=torch.float32)
    grad = torch.empty(pred.shape, dtype=pred.dtype, device=pred.device)
    L.check(L.lib().tcnn_loss_backward(loss_type, M._stream(pred), pred.shape[0], pred.shape[1], M._ptr(pred),
                                       int(pred.dtype == torch.float32), pred.stride(0), M._ptr(target), M._ptr(pdf),
                                       M._ptr(grad_output), M._ptr(grad)))
    return grad


class _loss_function(torch.autograd.Function):
    @staticmethod
    def forward(ctx, loss_type, pred, target, pdf):
        M = _modules()
        ctx.set_materialize_grads(False)
        n, dims = pred.shape
        lib = L.lib()
        n_ws = lib.tcnn_loss_workspace_floats(n, dims)
        value = torch.empty((), dtype=torch.float32, device=pred.device)
        workspace = torch.empty(n_ws, dtype=torch.float32, device=pred.device)
        L.check(lib.tcnn_loss_forward(loss_type, M._stream(pred), n, dims, M._ptr(pred), int(pred.dtype == torch.float32),
                                      pred.stride(0), M._ptr(target), M._ptr(pdf), M._ptr(workspace), n_ws, M._ptr(value)))
        ctx.loss_type = loss_type
        ctx.save_for_backward(pred, target, pdf)
        return value

    @staticmethod
    def backward(ctx, grad_output):
        if grad_output is None or not ctx.needs_input_grad[1]:
            return None, None, None, None
        pred, target, pdf = ctx.saved_tensors
        if torch.is_grad_enabled():  # create_graph=True: the gradient as a node whose own backward refuses
            return None, _loss_function_backward.apply(ctx.loss_type, grad_output, pred, target, pdf), None, None
        return None, _loss_grad(ctx.loss_type, grad_output, pred, target, pdf), None, None


class _loss_function_backward(torch.autograd.Function):
    @staticmethod
    def forward(ctx, loss_type, grad_output, pred, target, pdf):
        return _loss_grad(loss_type, grad_output, pred, target, pdf)

    @staticmethod
    def backward(ctx, grad):
        raise RuntimeError("tinycudann.Loss: the double backward of a loss is not implemented")


class Loss(torch.nn.Module):
    """One of L2, RelativeL2, RelativeL2Luminance, L1, RelativeL1, Mape, Smape, CrossEntropy, Variance
    (case-insensitive), given as a string or a {"otype": ...} dict. Holds only its otype."""

    def __init__(self, otype_or_config="RelativeL2"):
        super().__init__()
        otype = otype_or_config.get("otype", "RelativeL2") if isinstance(otype_or_config, dict) else otype_or_config
        if not isinstance(otype, str):
            raise TypeError(f"tinycudann.Loss: the otype must be a string, got {type(otype).__name__}")
        self.otype = otype
        self._type()  # an unknown otype fails here, with the engine's message

    def _type(self):
        t = L.lib().tcnn_loss_type(self.otype.encode())
        if t < 0:
            raise L.TcnnError(L.lib().tcnn_last_error().decode())
        return t

    def __getstate__(self):
        state = self.__dict__.copy()
        state.pop("_loss_type", None)
        return state

    def extra_repr(self):
        return f"otype={self.otype}"

    def forward(self, prediction, target, data_pdf=None):
        loss_type = self.__dict__.get("_loss_type")
        if loss_type is None:
            loss_type = self.__dict__["_loss_type"] = self._type()
        if prediction.dim() != 2 or not prediction.is_cuda:
            raise ValueError("tinycudann.Loss: the prediction must be a GPU tensor [n, dims]")
        if prediction.dtype not in _FLOAT_DTYPES:
            raise ValueError(f"tinycudann.Loss: the prediction must be fp16 or fp32, got {prediction.dtype}")
        n, dims = prediction.shape
        if n < 1 or not 1 <= dims <= MAX_DIMS:
            raise ValueError(f"tinycudann.Loss: the prediction must be [n >= 1, 1 <= dims <= {MAX_DIMS}], got {list(prediction.shape)}")
        if (dims > 1 and prediction.stride(1) != 1) or (n > 1 and prediction.stride(0) < dims):
            prediction = prediction.contiguous()  # rows of any stride are read as they are; columns must be adjacent
        target = self._operand("target", target, prediction)
        if data_pdf is not None:
            data_pdf = self._operand("data_pdf", data_pdf, prediction)
        M = _modules()
        if M._EXT is not None:
            return M._EXT.loss_apply(loss_type, prediction, target, data_pdf)
        return _loss_function.apply(loss_type, prediction, target, data_pdf)

    @staticmethod
    def _operand(name, t, prediction):
        if t.shape != prediction.shape:
            raise ValueError(f"tinycudann.Loss: {name} must have the prediction's shape {list(prediction.shape)}, got {list(t.shape)}")
        if t.device != prediction.device:
            raise ValueError(f"tinycudann.Loss: {name} must be on the prediction's device")
        if not t.dtype.is_floating_point:
            raise ValueError(f"tinycudann.Loss: {name} must be a floating-point tensor, got {t.dtype}")
        if t.dtype != torch.float32:
            t = t.to(torch.float32)
        return t if t.is_contiguous() else t.contiguous()
