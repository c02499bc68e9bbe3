"""Timing of a training step through the forward Laplacian of an fp32 FullyFusedMLP network module
(csrc/mlp_f32_jvp2_train.hip, Module.value_jacobian_and_laplacian(differentiable=True)): a Poisson-residual step
((lap y - f)^2).mean() + y.mean() and its backward to the parameters, through the torch front end in one process.

  alone  Network(3, 1): the new step against the only route there was: the same network restated as plain fp32 torch
         layers over the same parameters, the Laplacian by nested autograd.grad(create_graph=True), then backward().
         The torch arm clones x and rebuilds the ones padding every step, and its softplus(beta=10) is torch's, linear
         above its threshold (z > 2), so there its function is not exactly the module's: neither matters at the gap seen;
  grid   NetworkWithInputEncoding(3, 1, HashGrid L 16 F 2 T 2^19 Smoothstep): the new step alone. The fused module has
         no second order behind a grid and plain torch has no such encoding, so there is no baseline route.

NH 2, Softplus, B = 2^16, W in {32, 64}. The arms alternate window by window; medians of the windows (wall clock,
synchronised at a window's two ends only) and the windows themselves. An arm wins a row only if the two arms' window
ranges do not overlap.

  python tools/mlp_f32_jvp2_train_ab.py [--out profiles/mlp_f32_jvp2_train_ab.json] [--windows 5] [--steps 50]
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "neuralbtf-tiny-cuda-nn_amd")]

D, NH, IN = 3, 2, 16
GRID = {"otype": "HashGrid", "n_levels": 16, "n_features_per_level": 2, "log2_hashmap_size": 19, "base_resolution": 16,
        "per_level_scale": 1.5, "interpolation": "Smoothstep"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--log2b", type=int, default=16)
    args = ap.parse_args()
    import torch
    import tinycudann as tcnn

    B = 1 << args.log2b
    x, f = torch.rand(B, D, device="cuda"), torch.rand(B, 1, device="cuda")
    res = {"batch": B, "windows": args.windows, "steps_per_window": args.steps, "n_in": D, "n_hidden_layers": NH, "encoding": GRID, "rows": []}

    def loss_of(y, lap):
        return ((lap - f) ** 2).mean() + y.mean()

    for W in (32, 64):
        net = {"otype": "FullyFusedMLP", "activation": "Softplus", "output_activation": "None", "n_neurons": W, "n_hidden_layers": NH}
        for front in ("alone", "grid"):
            m = tcnn.Network(D, 1, net, dtype=torch.float32) if front == "alone" else tcnn.NetworkWithInputEncoding(D, 1, GRID, net, dtype=torch.float32)

            def step():
                m.params.grad = None
                y, _, lap = m.value_jacobian_and_laplacian(x, differentiable=True)
                loss_of(y, lap).backward()
                return m.params.grad

            row, arms = {"n_neurons": W, "front": front}, {"step": step}
            if front == "alone":
                p = m.params.detach().clone().requires_grad_(True)
                sizes = [W * IN] + [W * W] * (NH - 1) + [16 * W]

                def torch_step():
                    p.grad = None
                    xg = x.clone().requires_grad_(True)
                    h, off = torch.cat([xg, torch.ones(B, IN - D, device="cuda")], 1), 0
                    for j, n in enumerate(sizes):
                        h = h @ p[off:off + n].reshape(-1, h.shape[1]).T
                        h, off = (torch.nn.functional.softplus(h, beta=10.0) if j < NH else h), off + n
                    y = h[:, :1]
                    g = torch.autograd.grad(y.sum(), xg, create_graph=True)[0]
                    lap = sum(torch.autograd.grad(g[:, d].sum(), xg, create_graph=True)[0][:, d] for d in range(D))
                    loss_of(y, lap[:, None]).backward()
                    return p.grad

                arms["torch_layers"] = torch_step
                a, b = step().clone(), torch_step()
                row["max_abs_grad"] = float(b.abs().max())
                row["max_abs_step_minus_torch"] = float((a - b).abs().max())
            else:
                row["baseline"] = "none: no route to a Laplacian loss behind a grid exists without this call"
            for s in arms.values():
                for _ in range(5):
                    s()
            us = {arm: [] for arm in arms}
            for _ in range(args.windows):
                for arm, s in arms.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(args.steps):
                        s()
                    torch.cuda.synchronize()
                    us[arm].append((time.perf_counter() - t0) * 1e6 / args.steps)
            for arm, t in us.items():
                row[arm + "_us"] = {"median": statistics.median(t), "min": min(t), "max": max(t), "windows": t}
            if "torch_layers" in us:
                c, r = us["step"], us["torch_layers"]
                row["step_over_torch"] = statistics.median(c) / statistics.median(r)
                row["verdict"] = "step wins" if max(c) < min(r) else "step loses" if max(r) < min(c) else "tie"
            res["rows"].append(row)
    print(json.dumps(res, indent=1))
    if args.out:
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
