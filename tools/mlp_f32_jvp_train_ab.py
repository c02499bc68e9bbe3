"""A/B of the eikonal step on an fp32 network module, the configuration of profiles/mlp_f32_second_order_ab.json
(HashGrid 3-D, 16 levels, F 2, 2^15 entries, Smoothstep; Softplus, W 64, two hidden layers, one output, B 2^16):

  A  y, J = module.value_and_jacobian(x, differentiable=True);  loss = (y w).sum() + ((J.norm(dim=-1) - 1)^2).mean()
     one keeping forward-mode launch and its reverse pass (csrc/mlp_f32_jvp_train.hip)
  B  gx = autograd.grad(y.sum(), x, create_graph=True);  the same loss on gx: the double-backward route
     (backward, backward_backward_input)

Both arms run in one process on one module, alternated window by window; medians of the windows and their ranges (wall
clock, synchronised at a window's two ends only). Arm A produces dL/dparams only, arm B also dL/dx.

  python tools/mlp_f32_jvp_train_ab.py [--out profiles/mlp_f32_jvp_train_ab.json] [--windows 5] [--steps 200]
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "neuralbtf-tiny-cuda-nn_amd"), os.path.join(REPO, "tools")]

from mlp_f32_second_order_ab import GRID, N_IN, N_OUT, NH, W  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--log2b", type=int, default=16)
    args = ap.parse_args()
    import torch
    import tinycudann as tcnn

    B = 1 << args.log2b
    torch.manual_seed(0)
    x = torch.rand(B, N_IN, device="cuda")
    xg = x.clone().requires_grad_(True)
    w = torch.rand(B, N_OUT, device="cuda")
    net = {"otype": "FullyFusedMLP", "activation": "Softplus", "output_activation": "None", "n_neurons": W, "n_hidden_layers": NH}
    model = tcnn.NetworkWithInputEncoding(N_IN, N_OUT, GRID, net, dtype=torch.float32)

    def step_a():
        model.params.grad = None
        y, J = model.value_and_jacobian(x, differentiable=True)
        ((y * w).sum() + ((J.norm(dim=-1) - 1) ** 2).mean()).backward()

    def step_b():
        model.params.grad = None
        y = model(xg)
        gx = torch.autograd.grad(y.sum(), xg, create_graph=True)[0]
        ((y * w).sum() + ((gx.norm(dim=-1) - 1) ** 2).mean()).backward()

    arms = {"A": step_a, "B": step_b}
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
    summary = lambda v: {"median": statistics.median(v), "min": min(v), "max": max(v), "windows": v}
    res = {"batch": B, "windows": args.windows, "steps_per_window": args.steps, "encoding": GRID,
           "network": {"n_in": N_IN, "n_neurons": W, "n_hidden_layers": NH, "n_out": N_OUT, "activation": "Softplus"},
           "A_differentiable_jvp_us": summary(us["A"]), "B_double_backward_us": summary(us["B"])}
    res["A_over_B"] = res["A_differentiable_jvp_us"]["median"] / res["B_double_backward_us"]["median"]
    print(json.dumps(res, indent=1))
    if args.out:
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
