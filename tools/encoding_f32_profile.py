"""Kernel-trace workload of the lone config_hash grid encoding module at B = 2^18 in one precision:
forward, backward to the parameters, dL/dinput, `--iters` times each after a warm-up. Run it under
`rocprofv3 --kernel-trace --stats -- python tools/encoding_f32_profile.py --precision fp32` (and fp16)
and read the per-kernel averages from the stats file (profiles/encoding_f32.txt).
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "neuralbtf-tiny-cuda-nn_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", choices=["fp16", "fp32"], required=True)
    ap.add_argument("--batch", type=int, default=1 << 18)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    import torch
    from tinycudann import _lib as L
    lib = L.lib()
    cfg = json.load(open(os.path.join(REPO, "tests", "golden", "config_hash.json")))["encoding"]
    prec = 0 if a.precision == "fp32" else 1
    dt = torch.float32 if prec == 0 else torch.float16
    m = L.check_ptr(lib.tcnn_create_encoding(2, json.dumps(cfg).encode(), prec))
    n, W = lib.tcnn_module_n_params(m), lib.tcnn_module_n_output_dims(m)
    g = torch.Generator(device="cuda").manual_seed(1)
    B = a.batch
    p = (torch.rand(n, device="cuda", generator=g) * 2 - 1).to(dt)
    x = torch.rand(B, 2, device="cuda", generator=g)
    dy = torch.randn(B, W, device="cuda", generator=g).to(dt)
    out = torch.empty(B, W, dtype=dt, device="cuda")
    grad = torch.empty(n, dtype=dt, device="cuda")
    dx = torch.empty(B, 2, device="cuda")
    vp = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    ctx = L.check_ptr(lib.tcnn_module_forward(m, None, B, vp(x), vp(out), vp(p), 1))
    for it in range(3 + a.iters):
        L.check(lib.tcnn_module_inference(m, None, B, vp(x), vp(out), vp(p)))
        L.check(lib.tcnn_module_backward(m, None, ctx, B, None, vp(dy), vp(grad), vp(x), vp(out), vp(p)))
        L.check(lib.tcnn_module_backward(m, None, ctx, B, vp(dx), vp(dy), None, vp(x), vp(out), vp(p)))
        torch.cuda.synchronize()
    assert torch.isfinite(out.float()).all() and torch.isfinite(grad.float()).all() and torch.isfinite(dx).all()
    lib.tcnn_context_destroy(ctx)
    lib.tcnn_module_destroy(m)
    print("profile workload ok", a.precision, "B", B, "params", n)


if __name__ == "__main__":
    main()
