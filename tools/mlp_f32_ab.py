"""A/B of the fp32 network module against what a caller stacks today: forward + backward of

  A  tinycudann.Network(32, 16, {W 64, 2 hidden layers, ReLU}, dtype=torch.float32)  (csrc/mlp_f32.hip)
  B  torch.nn.Sequential(Linear(32, 64, bias=False), ReLU, Linear(64, 64, bias=False), ReLU, Linear(64, 16, bias=False))
     in fp32

at B = 2^16 through the torch front end (loss = output.sum(), gradients to the parameters and to the input), both
arms in one process, alternated window by window; medians of the windows (wall clock, synchronised at a window's
two ends only). Beside the times, the kernels' own floor: FLOPs over the f32 matrix-core peak and the fp32
activation bytes over the HBM bandwidth (MI355X: 157.3 TF, 8 TB/s).

  python tools/mlp_f32_ab.py [--out profiles/mlp_f32_ab.json] [--windows 5] [--steps 200] [--arm A|B]
  --arm: run one arm only, a few steps, for a kernel-trace run of its own (rocprofv3 --kernel-trace --stats --)
  --kernel-stats FILE.csv ...: fold a trace's per-kernel times into the JSON under "kernels"
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

N_IN, W, NH, N_OUT = 32, 64, 2, 16
PEAK_F32_MFMA, PEAK_HBM = 157.3e12, 8.0e12


def floor(B):
    """what forward + backward must do: 2 B N K flops per product, three products per layer (forward, backward
    data, weight gradient); every activation row written once and read by the next layer, by the backward's
    transfer and by the weight gradient, every delta written once and read twice"""
    layers = [(W, N_IN), (W, W), (N_OUT, W)]
    flops = sum(3 * 2 * B * n * k for n, k in layers)
    widths = [N_IN, W, W, N_OUT]
    fwd_bytes = 4 * B * (sum(widths[1:]) + sum(widths[:-1]))            # each layer: read its input, write its output
    bwd_bytes = 4 * B * sum(2 * n + 2 * k + k for n, k in layers)       # dy, y (transfer) read twice, x read, dx written
    return {"flops": flops, "bytes": fwd_bytes + bwd_bytes, "mfma_floor_us": flops / PEAK_F32_MFMA * 1e6,
            "hbm_floor_us": (fwd_bytes + bwd_bytes) / PEAK_HBM * 1e6}


def make_arm(torch, tcnn, name, x):
    if name == "A":
        net = {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": W, "n_hidden_layers": NH}
        model = tcnn.Network(N_IN, N_OUT, net, dtype=torch.float32)
    else:
        L = torch.nn.Linear
        model = torch.nn.Sequential(L(N_IN, W, bias=False), torch.nn.ReLU(), L(W, W, bias=False), torch.nn.ReLU(),
                                    L(W, N_OUT, bias=False)).cuda()

    def step():
        for p in model.parameters():
            p.grad = None
        x.grad = None
        model(x).sum().backward()
    return step


def kernel_times(paths):
    out = {}
    for p in paths:
        for row in csv.DictReader(open(p)):
            name = row.get("Name") or row.get("KernelName")
            if name:
                out[name] = {"calls": int(row["Calls"]), "average_us": float(row["AverageNs"]) / 1e3, "total_us": float(row["TotalDurationNs"]) / 1e3}
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
        res["kernels"] = kernel_times(args.kernel_stats)
        json.dump(res, open(args.out, "w"), indent=1)
        return
    import torch
    import tinycudann as tcnn

    B = 1 << args.log2b
    x = torch.rand(B, N_IN, device="cuda", requires_grad=True)
    if args.arm:
        step = make_arm(torch, tcnn, args.arm, x)
        for _ in range(20):
            step()
        torch.cuda.synchronize()
        return
    arms = {name: make_arm(torch, tcnn, name, x) for name in "AB"}
    for step in arms.values():
        for _ in range(50):
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
    res = {"batch": B, "windows": args.windows, "steps_per_window": args.steps,
           "network": {"n_in": N_IN, "n_neurons": W, "n_hidden_layers": NH, "n_out": N_OUT, "activation": "ReLU"},
           "A_tcnn_fp32_us": {"median": statistics.median(us["A"]), "windows": us["A"]},
           "B_torch_sequential_fp32_us": {"median": statistics.median(us["B"]), "windows": us["B"]},
           "floor": floor(B)}
    res["A_over_B"] = res["A_tcnn_fp32_us"]["median"] / res["B_torch_sequential_fp32_us"]["median"]
    print(json.dumps(res, indent=1))
    if args.out:
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
