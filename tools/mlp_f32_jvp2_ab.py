"""Timing of the forward Laplacian of an fp32 FullyFusedMLP network module (csrc/mlp_f32_jvp2.hip,
Module.value_jacobian_and_laplacian: y, dy/dx and sum_d d^2 y / dx_d^2 in one forward-mode launch) against the
double-backward route to the same Laplacian, through the torch front end in one process:

  alone  Network(3, 1): the new call against forward, autograd.grad(create_graph=True) and one grad per input
         dimension on the same module (tcnn_module_backward_backward_input);
  grid   NetworkWithInputEncoding(3, 1, HashGrid L 16 F 2 T 2^19 Smoothstep): the new call against an Encoding module
         and a Network module composed in torch through the same route, since the fused module has no second order there.

NH 2, Softplus, B = 2^16, W in {32, 64}; W 128 is refused by the new call and is recorded as such. The arms alternate
window by window; medians of the windows (wall clock, synchronised at a window's two ends only) and the windows
themselves. An arm wins a row only if the two arms' window ranges do not overlap.

  python tools/mlp_f32_jvp2_ab.py [--out profiles/mlp_f32_jvp2_ab.json] [--windows 5] [--steps 100]
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "neuralbtf-tiny-cuda-nn_amd")]

D, NH = 3, 2
GRID = {"otype": "HashGrid", "n_levels": 16, "n_features_per_level": 2, "log2_hashmap_size": 19, "base_resolution": 16,
        "per_level_scale": 1.5, "interpolation": "Smoothstep"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--log2b", type=int, default=16)
    args = ap.parse_args()
    import torch
    import tinycudann as tcnn

    B = 1 << args.log2b
    x = torch.rand(B, D, device="cuda")
    res = {"batch": B, "windows": args.windows, "steps_per_window": args.steps, "n_in": D, "n_hidden_layers": NH, "encoding": GRID, "rows": []}

    def laplacian_by_autograd(f):
        xg = x.clone().requires_grad_(True)
        g = torch.autograd.grad(f(xg).sum(), xg, create_graph=True)[0]
        return sum(torch.autograd.grad(g[:, d].sum(), xg, retain_graph=True)[0][:, d] for d in range(D))

    for W in (32, 64, 128):
        net = {"otype": "FullyFusedMLP", "activation": "Softplus", "output_activation": "None", "n_neurons": W, "n_hidden_layers": NH}
        for front in ("alone", "grid"):
            if front == "alone":
                m = tcnn.Network(D, 1, net, dtype=torch.float32)
                route = lambda: laplacian_by_autograd(m)  # noqa: E731
            else:
                m = tcnn.NetworkWithInputEncoding(D, 1, GRID, net, dtype=torch.float32)
                enc = tcnn.Encoding(D, GRID, dtype=torch.float32)
                tail = tcnn.Network(enc.n_output_dims, 1, net, dtype=torch.float32)
                n_mlp = tail.params.numel()
                with torch.no_grad():  # the same function in both arms: one table, one set of matrices
                    m.params[n_mlp:].uniform_(-1, 1)
                    enc.params.copy_(m.params[n_mlp:])
                    tail.params.copy_(m.params[:n_mlp])
                route = lambda: laplacian_by_autograd(lambda t: tail(enc(t)))  # noqa: E731
            call = lambda: m.value_jacobian_and_laplacian(x)[2]  # noqa: E731
            row = {"n_neurons": W, "front": front}
            try:
                lap = call()
            except tcnn.TcnnError as e:  # the refusal is the row's result
                row["refused"] = str(e)
                res["rows"].append(row)
                continue
            ref = route()
            row["max_abs_laplacian"] = float(ref.abs().max())
            row["max_abs_call_minus_route"] = float((lap[:, 0] - ref).abs().max())
            arms = {"call": call, "double_backward": route}
            for step in arms.values():
                for _ in range(10):
                    step()
            us = {arm: [] for arm in arms}
            for _ in range(args.windows):
                for arm, step in arms.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(args.steps):
                        step()
                    torch.cuda.synchronize()
                    us[arm].append((time.perf_counter() - t0) * 1e6 / args.steps)
            for arm, t in us.items():
                row[arm + "_us"] = {"median": statistics.median(t), "min": min(t), "max": max(t), "windows": t}
            c, r = us["call"], us["double_backward"]
            row["call_over_route"] = statistics.median(c) / statistics.median(r)
            row["verdict"] = "call wins" if max(c) < min(r) else "call loses" if max(r) < min(c) else "tie"
            res["rows"].append(row)
    print(json.dumps(res, indent=1))
    if args.out:
        json.dump(res, open(args.out, "w"), indent=1)
        with open(os.path.splitext(args.out)[0].replace("_ab", "_ab_ratios") + ".txt", "w") as f:
            for r in res["rows"]:
                f.write(f"W {r['n_neurons']} {r['front']}: " + (f"refused ({r['refused']})" if "refused" in r else
                        f"call {r['call_us']['median']:.1f} us, double backward {r['double_backward_us']['median']:.1f} us, "
                        f"ratio {r['call_over_route']:.4f}, {r['verdict']}") + "\n")


if __name__ == "__main__":
    main()
