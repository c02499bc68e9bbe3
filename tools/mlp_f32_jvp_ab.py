"""Timing of the one-launch value-and-JVP call of an fp32 FullyFusedMLP network module behind a hash grid
(csrc/mlp_f32_jvp.hip) against today's route to the same numbers, arms of ONE module in one process through the C-ABI:

  J   tcnn_module_inference_jvp with null directions: y and the Jacobian dy/dx in one forward-mode launch
  V   tcnn_module_inference_jvp with one direction per sample (K = 1): y and d/dt f(x + t v)
  R   the route without the call, the arm to compare against: tcnn_module_forward (keeps its context), then one
      tcnn_module_backward per output with a one-hot dL/dy, dL/dinput asked for and dL_dparams null
  I   tcnn_module_inference alone (the value only: the floor)

on NetworkWithInputEncoding(3, n_out, HashGrid L 16 F 2 log2_hashmap_size 19, FullyFusedMLP NH 2, ReLU), n_out in {1, 3},
W in {32, 64, 128}, B = 2^16, all AoS. The arms alternate window by window; medians of the windows (wall clock,
synchronised at a window's two ends only) and the windows themselves. An arm wins a row only if the two arms' window
ranges do not overlap. --once runs each arm a few times and exits: the run to put under a kernel trace.

  python tools/mlp_f32_jvp_ab.py [--out profiles/mlp_f32_jvp_ab.json] [--windows 5] [--steps 2000] [--once]
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
GRID = {"otype": "HashGrid", "n_levels": 16, "n_features_per_level": 2, "log2_hashmap_size": 19, "base_resolution": 16,
        "per_level_scale": 1.5}


def vp(t):
    return ctypes.c_void_p(t.data_ptr())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--log2b", type=int, default=16)
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    import torch
    from tinycudann import _lib as L

    lib, B = L.lib(), 1 << args.log2b
    x = torch.rand(B, D, device="cuda")
    v = torch.rand(B, 1, D, device="cuda") * 2 - 1
    res = {"batch": B, "windows": args.windows, "steps_per_window": args.steps, "n_in": D, "n_hidden_layers": NH, "encoding": GRID, "rows": []}
    for W in (32, 64, 128):
        for n_out in (1, 3):
            net = {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": W, "n_hidden_layers": NH}
            m = L.check_ptr(lib.tcnn_create_network_with_input_encoding_precision(D, n_out, json.dumps(GRID).encode(), json.dumps(net).encode(), 0))
            p = torch.zeros(lib.tcnn_module_n_params(m), device="cuda")
            L.check(lib.tcnn_module_initialize_params(m, 1337, vp(p), 1.0))
            p[lib.tcnn_module_n_network_params(m):].uniform_(-1, 1)  # a table with slopes to compare
            y, y1, y2 = (torch.empty(B, OUTP, device="cuda") for _ in range(3))
            jac, jv = torch.empty(B, n_out, D, device="cuda"), torch.empty(B, n_out, 1, device="cuda")
            onehot = [torch.zeros(B, OUTP, device="cuda") for _ in range(n_out)]
            for o, t in enumerate(onehot):
                t[:, o] = 1.0
            dx = [torch.empty(B, D, device="cuda") for _ in range(n_out)]

            def jacobian():
                L.check(lib.tcnn_module_inference_jvp(m, None, B, vp(x), None, 0, vp(y), vp(jac), vp(p), 0))

            def direction():
                L.check(lib.tcnn_module_inference_jvp(m, None, B, vp(x), vp(v), 1, vp(y1), vp(jv), vp(p), 0))

            def inference():
                L.check(lib.tcnn_module_inference(m, None, B, vp(x), vp(y2), vp(p)))

            def route():
                ctx = L.check_ptr(lib.tcnn_module_forward(m, None, B, vp(x), vp(y2), vp(p), 1))
                for o in range(n_out):
                    L.check(lib.tcnn_module_backward(m, None, ctx, B, vp(dx[o]), vp(onehot[o]), None, vp(x), vp(y2), vp(p)))
                lib.tcnn_context_destroy(ctx)

            arms = {"jvp_unit": jacobian, "jvp_k1": direction, "forward_backward": route, "inference": inference}
            for step in arms.values():
                for _ in range(3 if args.once else 30):
                    step()
            torch.cuda.synchronize()
            route_j = torch.stack(dx, 1)
            agree = float((jac - route_j).abs().max())
            agree_v = float((jv[:, :, 0] - torch.einsum("bod,bd->bo", route_j, v[:, 0])).abs().max())
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
            r = us["forward_backward"]
            row = {"n_neurons": W, "n_out": n_out, "y_bits_equal_inference": bool(torch.equal(y, y2) and torch.equal(y1, y2)),
                   "max_abs_J_minus_route": agree, "max_abs_Jv_minus_route": agree_v, "max_abs_J": float(route_j.abs().max())}
            for arm, t in us.items():
                row[arm + "_us"] = {"median": statistics.median(t), "min": min(t), "max": max(t), "windows": t}
            for arm in ("jvp_unit", "jvp_k1"):
                j = us[arm]
                row[arm + "_over_route"] = statistics.median(j) / statistics.median(r)
                row[arm + "_verdict"] = "call wins" if max(j) < min(r) else "call loses" if max(r) < min(j) else "tie"
            res["rows"].append(row)
            lib.tcnn_module_destroy(m)
    print(json.dumps(res, indent=1))
    if args.out:
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
