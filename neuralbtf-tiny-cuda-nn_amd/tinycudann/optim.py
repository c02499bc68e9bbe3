"""tinycudann.optim: the engine's Adam (csrc/adam_device.h; reference optimizers/adam.h:47-119, 235-283) as a
torch.optim.Optimizer over the C-ABI's tcnn_adam_step_buffers (k_adam_torch, csrc/optimizers.hip).

    opt = tinycudann.optim.Adam(tinycudann.optim.param_groups(model, learning_rate=1e-2, l2_reg=1e-6))
    loss(model(x), target).backward(); opt.step(); opt.zero_grad()

What differs from torch.optim.Adam is what the reference's Adam does: every parameter carries its own step
count; a non-matrix parameter (a hash-grid entry) whose gradient is zero is skipped -- not moved, not counted;
l2_reg applies to matrix (network) parameters only, non_matrix_learning_rate_factor to the others; relative and
absolute decay, clipping and AdaBound's bounds are options. step() is one kernel launch per parameter tensor
on the current stream, with no host synchronisation and no readback.
"""
import ctypes

import torch

from tinycudann import _lib as L

# the reference's names and defaults (adam.h:235-283), in tcnn_adam_options order
_HYPER = (("learning_rate", 1e-3), ("beta1", 0.9), ("beta2", 0.999), ("epsilon", 1e-8), ("l2_reg", 1e-8), ("relative_decay", 0.0),
          ("absolute_decay", 0.0), ("clipping_magnitude", 0.0), ("non_matrix_learning_rate_factor", 1.0), ("adabound", False),
          ("optimize_matrix_params", True), ("optimize_non_matrix_params", True))
_TABLE_GRANULE = 1024  # bias-correction factors are computed this many steps ahead


def _modules():
    from tinycudann import modules  # raises without a GPU, as the reference does at import time
    return modules


def param_groups(model, **options):
    """Parameter groups of a torch.nn.Module for Adam: one group per tinycudann module's `params`, whose n_matrix
    is the module's network parameter count (0 for an Encoding, all for a Network, the network's part of a
    NetworkWithInputEncoding), and one group of every other parameter (all matrix parameters). options go into
    every group."""
    M = _modules()
    groups, seen = [], set()
    for m in model.modules():
        if isinstance(m, M.Module):
            p = m.params
            if id(p) in seen:
                continue
            seen.add(id(p))
            n_matrix = int(L.lib().tcnn_module_n_network_params(m.native_tcnn_module.h))
            groups.append(dict(options, params=[p], n_matrix=n_matrix))
    rest = [p for p in model.parameters() if id(p) not in seen]
    if rest:
        groups.append(dict(options, params=rest, n_matrix=None))
    return groups


class Adam(torch.optim.Optimizer):
    """The reference's Adam. Group options: learning_rate (alias lr), beta1, beta2, epsilon, l2_reg,
    relative_decay, absolute_decay, clipping_magnitude, non_matrix_learning_rate_factor, adabound,
    optimize_matrix_params, optimize_non_matrix_params, and n_matrix: how many leading elements of each of the
    group's parameter tensors are matrix parameters (None, or more than a tensor holds: all of them). Parameters are fp32, contiguous GPU
    tensors; gradients fp32 or fp16. State per tensor: exp_avg, exp_avg_sq (fp32), param_steps (the per-element
    step counts, uint32 bits in an int32 tensor) and step (the steps this tensor has taken)."""

    def __init__(self, params, n_matrix=None, lr=None, **options):
        unknown = set(options) - {k for k, _ in _HYPER}
        if unknown:
            raise TypeError(f"tinycudann.optim.Adam: unknown options {sorted(unknown)}")
        if lr is not None:
            if "learning_rate" in options and float(options["learning_rate"]) != float(lr):
                raise ValueError("tinycudann.optim.Adam: lr and learning_rate are the same option and differ")
            options["learning_rate"] = lr
        defaults = dict(_HYPER, n_matrix=n_matrix)
        defaults.update(options)
        self._tables = {}  # (device, beta1, beta2) -> bias-correction factors of steps 1 .. len
        super().__init__(params, defaults)

    def add_param_group(self, group):
        group = dict(group)
        if "lr" in group:  # the alias, so that code written for torch.optim.Adam builds the same group
            lr = group.pop("lr")
            if "learning_rate" in group and float(group["learning_rate"]) != float(lr):
                raise ValueError("tinycudann.optim.Adam: lr and learning_rate are the same option and differ")
            group["learning_rate"] = lr
        super().add_param_group(group)
        group = self.param_groups[-1]
        group["lr"] = group["learning_rate"]
        for p in group["params"]:
            _check_param(p)
        if group["n_matrix"] is not None and group["n_matrix"] < 0:
            raise ValueError(f"tinycudann.optim.Adam: n_matrix must be None or a count, got {group['n_matrix']}")

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        # torch casts every state tensor of a floating-point parameter to the parameter's dtype; the per-element step
        # counts are integers (fp32 holds them exactly only up to 2^24): they are taken from the saved state as they are
        saved_ids = [i for g in state_dict["param_groups"] for i in g["params"]]
        params = [p for g in self.param_groups for p in g["params"]]
        for i, p in zip(saved_ids, params):
            saved = state_dict["state"].get(i)
            if saved is not None and "param_steps" in saved:
                self.state[p]["param_steps"] = saved["param_steps"].to(device=p.device, dtype=torch.int32, copy=True)

    @staticmethod
    def _learning_rate(group):
        """lr and learning_rate name one option: whichever was written since the last step holds (an LR scheduler
        writes lr), and both leave with that value"""
        seen = group.get("_lr_applied", group["learning_rate"])
        value = group["lr"] if group["lr"] != seen else group["learning_rate"]
        group["lr"] = group["learning_rate"] = group["_lr_applied"] = value
        return float(value)

    def _table(self, device, beta1, beta2, upto):
        """device tensor of sqrt(1 - beta2^t) / (1 - beta1^t), t = 1 .. len >= upto, computed on the host by the C
        library (as the trainer's Adam does; a device powf differs in the last bit for some t) a granule ahead, so
        the host-to-device copy happens once in 1024 steps"""
        key = (device, beta1, beta2)
        table = self._tables.get(key)
        if table is None or table.numel() < upto:
            n = (upto + _TABLE_GRANULE - 1) // _TABLE_GRANULE * _TABLE_GRANULE
            host = torch.empty(n, dtype=torch.float32)
            L.check(L.lib().tcnn_adam_bias_factors(beta1, beta2, 1, n, host.data_ptr()))
            table = self._tables[key] = host.to(device)
        return table

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        M = _modules()
        ext = M._EXT
        lib = L.lib()
        for group in self.param_groups:
            lr = self._learning_rate(group)
            hyper = (lr,) + tuple(float(group[k]) for k, _ in _HYPER[1:])
            options = None
            for p in group["params"]:
                grad = p.grad
                if grad is None:
                    continue
                _check_param(p)
                grad = _checked_grad(p, grad)
                state = self.state[p]
                if not state:
                    state["step"] = 0
                    state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    state["param_steps"] = torch.zeros(p.shape, dtype=torch.int32, device=p.device)
                step = state["step"] = int(state["step"]) + 1
                n = p.numel()
                n_matrix = n if group["n_matrix"] is None else int(group["n_matrix"])
                table = self._table(p.device, hyper[1], hyper[2], step)
                m1, m2, steps = state["exp_avg"], state["exp_avg_sq"], state["param_steps"]
                if ext is not None:
                    ext.adam_step(p, grad, m1, m2, steps, table, n_matrix, step, hyper)
                    continue
                if options is None:
                    options = L.AdamOptions(*hyper[:9], *(int(v) for v in hyper[9:]))
                L.check(lib.tcnn_adam_step_buffers(M._stream(p), ctypes.byref(options), n, n_matrix, step, p.data_ptr(), grad.data_ptr(),
                                                   int(grad.dtype == torch.float16), m1.data_ptr(), m2.data_ptr(), steps.data_ptr(),
                                                   table.data_ptr(), table.numel()))
        return loss


def _check_param(p):
    if not p.is_cuda:
        raise ValueError("tinycudann.optim.Adam: parameters must be GPU tensors")
    if p.dtype != torch.float32:
        raise ValueError(f"tinycudann.optim.Adam: parameters must be fp32, got {p.dtype}")
    if not p.is_contiguous():
        raise ValueError("tinycudann.optim.Adam: parameters must be contiguous")


def _checked_grad(p, grad):
    if grad.is_sparse:
        raise ValueError("tinycudann.optim.Adam: sparse gradients are not supported")
    if grad.dtype not in (torch.float32, torch.float16):
        raise ValueError(f"tinycudann.optim.Adam: gradients must be fp32 or fp16, got {grad.dtype}")
    if grad.device != p.device or grad.shape != p.shape:
        raise ValueError("tinycudann.optim.Adam: a gradient must have its parameter's device and shape")
    return grad if grad.is_contiguous() else grad.contiguous()
