"""A/B of the fused fp32 MLP kernels (csrc/mlp_f32_fused.hip) against the layer kernels (csrc/mlp_f32.hip): two arms
in one process through the torch front end,

  F  tinycudann.Network(32, 16, {"otype": "FullyFusedMLP", W, 2 hidden layers, ReLU}, dtype=torch.float32)
  C  the same with "otype": "CutlassMLP" (one launch per layer: the path every fp32 module ran before)

at B = 2^16 and W = 64 and 128, for three calls a user makes:

  inference      model(x) under no_grad
  train          forward + backward with gradients to the parameters and to the input
  input_grad     forward + backward with the gradient to the input only (normals of an SDF)

The arms alternate window by window; medians of the windows (wall clock, synchronised at a window's two ends only).
An arm wins a row only if the two arms' window ranges do not overlap; anything else is a tie. Beside the times, the
HBM traffic of the network's launches in floats per batch row, counted from the shapes (encoding and weight-gradient
launches, equal in both arms, are left out).

  python tools/mlp_f32_fused_ab.py [--out profiles/mlp_f32_fused_ab.json] [--windows 5] [--steps 200]
  --arm F|C --mode MODE --width W: run one arm and one call only, a few steps, for a kernel-trace run of its own
      (rocprofv3 --kernel-trace --stats --)
  --kernel-stats KEY=FILE.csv ...: fold traces' per-kernel times into the JSON under "kernels"[KEY]
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

N_IN, NH, N_OUT = 32, 2, 16
WIDTHS = (64, 128)
MODES = ("inference", "train", "input_grad")
OTYPE = {"F": "FullyFusedMLP", "C": "CutlassMLP"}


def traffic(W):
    """floats per batch row that the network's launches move through HBM (weights stay in L2)"""
    IN, OUTP = N_IN, N_OUT
    widths = [IN] + [W] * NH + [OUTP]
    layered_fwd = sum(a + b for a, b in zip(widths[:-1], widths[1:]))  # each layer reads its input, writes its output
    # backward data, per layer: dL/dy and the forward value beside it read, dL/dx written (an output activation of
    # None, as timed here, reads no output value: OUTP floats less in both columns)
    layered_bwd = sum(2 * n + k for k, n in zip(widths[:-1], widths[1:]))
    hidden = NH * W
    return {"inference": {"layered": layered_fwd, "fused": IN + OUTP},
            "forward_keep": {"layered": layered_fwd, "fused": IN + hidden + OUTP},
            "chain_input_only": {"layered": layered_bwd, "fused": 2 * OUTP + hidden + IN},
            "chain_with_params": {"layered": layered_bwd, "fused": 2 * OUTP + 2 * hidden + IN}}


def make_step(torch, tcnn, arm, mode, W, x):
    net = {"otype": OTYPE[arm], "activation": "ReLU", "output_activation": "None", "n_neurons": W, "n_hidden_layers": NH}
    model = tcnn.Network(N_IN, N_OUT, net, dtype=torch.float32)
    want = {"F": ("fused", "chain"), "C": ("layered", "layered")}[arm]
    nat = model.native_tcnn_module
    assert (nat.engine(), nat.backward_kernel(True)) == want and nat.inference_engine() == want[0], (arm, nat.engine())
    if mode == "inference":
        xi = x.detach()
        # as in the reference's binding, parameters that require a gradient make even a no_grad call keep a context
        model.params.requires_grad_(False)

        def step():
            with torch.no_grad():
                model(xi)
        return step
    model.params.requires_grad_(mode == "train")

    def step():
        model.params.grad = None
        x.grad = None
        model(x).sum().backward()
    return step


def kernel_times(path):
    out = {}
    for row in csv.DictReader(open(path)):
        name = row.get("Name") or row.get("KernelName")
        if name:
            out[name] = {"calls": int(row["Calls"]), "average_us": float(row["AverageNs"]) / 1e3, "total_us": float(row["TotalDurationNs"]) / 1e3}
    return out


def verdict(f, c):
    if max(f) < min(c):
        return "fused wins"
    if max(c) < min(f):
        return "fused loses"
    return "tie"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--log2b", type=int, default=16)
    ap.add_argument("--arm", default=None, choices=list(OTYPE))
    ap.add_argument("--mode", default="train", choices=MODES)
    ap.add_argument("--width", type=int, default=64, choices=WIDTHS)
    ap.add_argument("--kernel-stats", nargs="*", default=[])
    args = ap.parse_args()
    if args.kernel_stats:
        res = json.load(open(args.out))
        for item in args.kernel_stats:
            key, path = item.split("=", 1)
            res.setdefault("kernels", {})[key] = kernel_times(path)
        json.dump(res, open(args.out, "w"), indent=1)
        return
    import torch
    import tinycudann as tcnn

    B = 1 << args.log2b
    x = torch.rand(B, N_IN, device="cuda", requires_grad=True)
    if args.arm:
        step = make_step(torch, tcnn, args.arm, args.mode, args.width, x)
        for _ in range(20):
            step()
        torch.cuda.synchronize()
        return
    res = {"batch": B, "windows": args.windows, "steps_per_window": args.steps,
           "network": {"n_in": N_IN, "n_hidden_layers": NH, "n_out": N_OUT, "activation": "ReLU"}, "rows": {}}
    for W in WIDTHS:
        res["rows"][f"W{W}"] = {"floats_per_row": traffic(W)}
        for mode in MODES:
            arms = {arm: make_step(torch, tcnn, arm, mode, W, x) for arm in OTYPE}
            for step in arms.values():
                for _ in range(50):
                    step()
            torch.cuda.synchronize()
            us = {arm: [] for arm in arms}
            for _ in range(args.windows):
                for arm, step in arms.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(args.steps):
                        step()
                    torch.cuda.synchronize()
                    us[arm].append((time.perf_counter() - t0) * 1e6 / args.steps)
            res["rows"][f"W{W}"][mode] = {
                "fused_us": {"median": statistics.median(us["F"]), "windows": us["F"]},
                "layered_us": {"median": statistics.median(us["C"]), "windows": us["C"]},
                "fused_over_layered": statistics.median(us["F"]) / statistics.median(us["C"]),
                "verdict": verdict(us["F"], us["C"])}
    print(json.dumps(res, indent=1))
    if args.out:
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
