"""Timing of the one-launch value-and-Jacobian call of an fp32 FullyFusedMLP network module (csrc/mlp_f32_jacobian.hip)
against today's route to the same numbers, arms of ONE module in one process through the C-ABI:

  J  tcnn_module_inference_jacobian: y and dy/dx in one forward-mode launch, nothing kept
  I  tcnn_module_inference alone (the value only: the floor)
  R  the route without the call: tcnn_module_forward (keeps its context), then one tcnn_module_backward per output with
     a one-hot dL/dy and dL_dparams null

on Network(3, n_out, FullyFusedMLP, NH 2, ReLU), n_out in {1, 3}, W in {32, 64, 128}, B = 2^16, all AoS. The arms
alternate window by window; medians of the windows (wall clock, synchronised at a window's two ends only) and the
windows themselves. An arm wins a row only if the two arms' window ranges do not overlap. --once runs each arm a few
times and exits: the run to put under a kernel trace.

  python tools/mlp_f32_jacobian_ab.py [--out profiles/mlp_f32_jacobian_ab.json] [--windows 5] [--steps 5000] [--once]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "neuralbtf-tiny-cuda-nn_amd")]

D, NH, OUTP = 3, 2, 16


def vp(t):
    return ctypes.c_void_p(t.data_ptr())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5000)
    ap.add_argument("--log2b", type=int, default=16)
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    import torch
    from tinycudann import _lib as L

    lib, B = L.lib(), 1 << args.log2b
    x = torch.rand(B, D, device="cuda") * 2 - 1
    res = {"batch": B, "windows": args.windows, "steps_per_window": args.steps, "n_in": D, "n_hidden_layers": NH, "rows": []}
    for W in (32, 64, 128):
        for n_out in (1, 3):
            net = {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": W, "n_hidden_layers": NH}
            m = L.check_ptr(lib.tcnn_create_network_precision(D, n_out, json.dumps(net).encode(), 0))
            p = torch.zeros(lib.tcnn_module_n_params(m), device="cuda")
            L.check(lib.tcnn_module_initialize_params(m, 1337, vp(p), 1.0))
            y, y2, jac = torch.empty(B, OUTP, device="cuda"), torch.empty(B, OUTP, device="cuda"), torch.empty(B, n_out, D, device="cuda")
            onehot = [torch.zeros(B, OUTP, device="cuda") for _ in range(n_out)]
            for o, t in enumerate(onehot):
                t[:, o] = 1.0
            dx = [torch.empty(B, D, device="cuda") for _ in range(n_out)]

            def call():
                L.check(lib.tcnn_module_inference_jacobian(m, None, B, vp(x), vp(y), vp(jac), vp(p), 0))

            def inference():
                L.check(lib.tcnn_module_inference(m, None, B, vp(x), vp(y2), vp(p)))

            def route():
                ctx = L.check_ptr(lib.tcnn_module_forward(m, None, B, vp(x), vp(y2), vp(p), 1))
                for o in range(n_out):
                    L.check(lib.tcnn_module_backward(m, None, ctx, B, vp(dx[o]), vp(onehot[o]), None, vp(x), vp(y2), vp(p)))
                lib.tcnn_context_destroy(ctx)

            arms = {"jacobian": call, "inference": inference, "forward_backward": route}
            for step in arms.values():
                for _ in range(3 if args.once else 30):
                    step()
            torch.cuda.synchronize()
            agree = float((jac - torch.stack(dx, 1)).abs().max())
            if args.once:
                lib.tcnn_module_destroy(m)
                continue
            us = {arm: [] for arm in arms}
            for _ in range(args.windows):
                for arm, step in arms.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(args.steps):
                        step()
                    torch.cuda.synchronize()
                    us[arm].append((time.perf_counter() - t0) * 1e6 / args.steps)
            j, r = us["jacobian"], us["forward_backward"]
            row = {"n_neurons": W, "n_out": n_out, "y_bits_equal_inference": bool(torch.equal(y, y2)), "max_abs_J_minus_route": agree}
            for arm, v in us.items():
                row[arm + "_us"] = {"median": statistics.median(v), "min": min(v), "max": max(v), "windows": v}
            row["jacobian_over_route"] = statistics.median(j) / statistics.median(r)
            row["verdict"] = "jacobian wins" if max(j) < min(r) else "jacobian loses" if max(r) < min(j) else "tie"
            res["rows"].append(row)
            lib.tcnn_module_destroy(m)
    print(json.dumps(res, indent=1))
    if args.out:
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
