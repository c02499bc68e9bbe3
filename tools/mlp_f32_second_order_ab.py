"""A/B of the eikonal step on the fp32 network module against what a caller stacks today:

  gx = autograd.grad(y.sum(), x, create_graph=True);  loss = (y w).sum() + ((gx.norm(dim=-1) - 1)^2).mean();  loss.backward()

  A  tinycudann.NetworkWithInputEncoding(3, 1, HashGrid, {Softplus, W 64, 2 hidden layers}, dtype=torch.float32):
     first and second order in engine kernels (csrc/mlp_f32.hip, NetworkF32Host::backward_backward_input)
  B  tinycudann.Encoding(3, HashGrid, dtype=torch.float32) + torch.nn.Linear(bias=False) / Softplus(beta=10) in fp32:
     the same fp32 encoding module, the layers and their double backward in torch

at B = 2^16, gradients to every parameter and to x, both arms in one process, alternated window by window; medians of
the windows (wall clock, synchronised at a window's two ends only).

  python tools/mlp_f32_second_order_ab.py [--out profiles/mlp_f32_second_order_ab.json] [--windows 5] [--steps 200] [--arm A|B]
  --arm: run one arm only, a few steps, for a kernel-trace run of its own (rocprofv3 --kernel-trace --stats --)
  --kernel-stats A=FILE.csv B=FILE.csv: fold the traces' per-kernel times into the JSON under "kernels"
"""
import argparse
import csv
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "neuralbtf-tiny-cuda-nn_amd")]

N_IN, W, NH, N_OUT = 3, 64, 2, 1
GRID = {"otype": "HashGrid", "n_levels": 16, "n_features_per_level": 2, "log2_hashmap_size": 15, "base_resolution": 16,
        "per_level_scale": 1.5, "interpolation": "Smoothstep"}
ARM_STEPS = 20  # steps of a single-arm (trace) run


def make_arm(torch, tcnn, name, x, w):
    if name == "A":
        net = {"otype": "FullyFusedMLP", "activation": "Softplus", "output_activation": "None", "n_neurons": W, "n_hidden_layers": NH}
        model = tcnn.NetworkWithInputEncoding(N_IN, N_OUT, GRID, net, dtype=torch.float32)
    else:
        enc = tcnn.Encoding(N_IN, GRID, dtype=torch.float32)
        L, A = torch.nn.Linear, torch.nn.Softplus
        model = torch.nn.Sequential(enc, L(enc.n_output_dims, W, bias=False), A(beta=10), L(W, W, bias=False), A(beta=10),
                                    L(W, N_OUT, bias=False)).cuda()

    def step():
        for p in model.parameters():
            p.grad = None
        x.grad = None
        y = model(x)
        gx = torch.autograd.grad(y.sum(), x, create_graph=True)[0]
        ((y * w).sum() + ((gx.norm(dim=-1) - 1) ** 2).mean()).backward()
    return step


def kernel_times(path, steps):
    out = {}
    for row in csv.DictReader(open(path)):
        name = row.get("Name") or row.get("KernelName")
        if name:
            out[name] = {"calls_per_step": int(row["Calls"]) / steps, "average_us": float(row["AverageNs"]) / 1e3,
                         "us_per_step": float(row["TotalDurationNs"]) / 1e3 / steps}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--log2b", type=int, default=16)
    ap.add_argument("--arm", default=None, choices=["A", "B"])
    ap.add_argument("--kernel-stats", nargs="*", default=[])
    args = ap.parse_args()
    if args.kernel_stats:
        res = json.load(open(args.out))
        res["kernels"] = {a.split("=", 1)[0]: kernel_times(a.split("=", 1)[1], ARM_STEPS) for a in args.kernel_stats}
        for arm, k in res["kernels"].items():
            res["kernel_us_per_step_" + arm] = sum(v["us_per_step"] for v in k.values())
            res["launches_per_step_" + arm] = sum(v["calls_per_step"] for v in k.values())
        json.dump(res, open(args.out, "w"), indent=1)
        return
    import torch
    import tinycudann as tcnn

    B = 1 << args.log2b
    torch.manual_seed(0)
    x = torch.rand(B, N_IN, device="cuda", requires_grad=True)
    w = torch.rand(B, N_OUT, device="cuda")
    if args.arm:
        step = make_arm(torch, tcnn, args.arm, x, w)
        for _ in range(ARM_STEPS):
            step()
        torch.cuda.synchronize()
        return
    arms = {name: make_arm(torch, tcnn, name, x, w) for name in "AB"}
    for step in arms.values():
        for _ in range(30):
            step()
    torch.cuda.synchronize()
    us = {name: [] for name in arms}
    for _ in range(args.windows):
        for name, step in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                step()
            torch.cuda.synchronize()
            us[name].append((time.perf_counter() - t0) * 1e6 / args.steps)
    res = {"batch": B, "windows": args.windows, "steps_per_window": args.steps, "encoding": GRID,
           "network": {"n_in": N_IN, "n_neurons": W, "n_hidden_layers": NH, "n_out": N_OUT, "activation": "Softplus"},
           "A_tcnn_fp32_module_us": {"median": statistics.median(us["A"]), "windows": us["A"]},
           "B_encoding_plus_torch_layers_us": {"median": statistics.median(us["B"]), "windows": us["B"]}}
    res["A_over_B"] = res["A_tcnn_fp32_module_us"]["median"] / res["B_encoding_plus_torch_layers_us"]["median"]
    print(json.dumps(res, indent=1))
    if args.out:
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
