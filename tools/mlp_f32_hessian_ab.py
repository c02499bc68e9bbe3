"""Timing of the input Hessian of an fp32 FullyFusedMLP network module (csrc/mlp_f32_hessian.hip,
Module.value_jacobian_and_hessian: y, dy/dx and d^2 y / dx_d dx_e in one forward-mode launch) against the two routes
there were before it, through the torch front end in one process:

  polarisation     six one-direction value_jvp_and_second launches (e_0, e_1, e_2, e_0 + e_1, e_0 + e_2, e_1 + e_2) and
                   H_de = (q(e_d + e_e) - q(e_d) - q(e_e)) / 2;
  double_backward  forward, autograd.grad(create_graph=True) and one grad per input dimension
                   (tcnn_module_backward_backward_input); behind the grid an Encoding module and a Network module
                   composed in torch, since the fused module has no second order there
                   (tools/mlp_f32_jvp2_ab.py's route, keeping every row of H).

NH 2, Softplus, 3 inputs, 1 output, B = 2^16, W in {32, 64}, alone and behind HashGrid L 16 F 2 T 2^19 Smoothstep. The arms
alternate window by window; medians of the windows (wall clock, synchronised at a window's two ends only) and the
windows themselves. The call wins or loses against an arm only if the two window ranges do not overlap.

  python tools/mlp_f32_hessian_ab.py [--out profiles/mlp_f32_hessian_ab.json] [--windows 5] [--steps 100]
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
PAIRS = [(0, 1), (0, 2), (1, 2)]


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
    eye = torch.eye(D, device="cuda")
    dirs = [eye[d].expand(B, D).contiguous() for d in range(D)] + [(eye[d] + eye[e]).expand(B, D).contiguous() for d, e in PAIRS]
    res = {"batch": B, "windows": args.windows, "steps_per_window": args.steps, "n_in": D, "n_hidden_layers": NH, "encoding": GRID, "rows": []}

    def hessian_by_autograd(f):
        xg = x.clone().requires_grad_(True)
        g = torch.autograd.grad(f(xg).sum(), xg, create_graph=True)[0]
        return torch.stack([torch.autograd.grad(g[:, d].sum(), xg, retain_graph=True)[0] for d in range(D)], 1)

    for W in (32, 64):
        net = {"otype": "FullyFusedMLP", "activation": "Softplus", "output_activation": "None", "n_neurons": W, "n_hidden_layers": NH}
        for front in ("alone", "grid"):
            if front == "alone":
                m = tcnn.Network(D, 1, net, dtype=torch.float32)
                route = lambda: hessian_by_autograd(m)  # noqa: E731
            else:
                m = tcnn.NetworkWithInputEncoding(D, 1, GRID, net, dtype=torch.float32)
                enc = tcnn.Encoding(D, GRID, dtype=torch.float32)
                tail = tcnn.Network(enc.n_output_dims, 1, net, dtype=torch.float32)
                n_mlp = tail.params.numel()
                with torch.no_grad():  # the same function in every arm: one table, one set of matrices
                    m.params[n_mlp:].uniform_(-1, 1)
                    enc.params.copy_(m.params[n_mlp:])
                    tail.params.copy_(m.params[:n_mlp])
                route = lambda: hessian_by_autograd(lambda t: tail(enc(t)))  # noqa: E731

            def polarisation():
                q = [m.value_jvp_and_second(x, v)[2][:, 0] for v in dirs]
                H = torch.empty(B, D, D, device="cuda")
                for d in range(D):
                    H[:, d, d] = q[d]
                for i, (d, e) in enumerate(PAIRS):
                    H[:, d, e] = H[:, e, d] = 0.5 * (q[D + i] - q[d] - q[e])
                return H

            call = lambda: m.value_jacobian_and_hessian(x)[2][:, 0]  # noqa: E731
            row = {"n_neurons": W, "front": front}
            H, ref = call(), route()
            row["max_abs_hessian"] = float(ref.abs().max())
            row["max_abs_call_minus_double_backward"] = float((H - ref).abs().max())
            row["max_abs_call_minus_polarisation"] = float((H - polarisation()).abs().max())
            arms = {"call": call, "polarisation": polarisation, "double_backward": route}
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
            c = us["call"]
            for arm, t in us.items():
                row[arm + "_us"] = {"median": statistics.median(t), "min": min(t), "max": max(t), "windows": t}
                if arm != "call":
                    row["call_over_" + arm] = statistics.median(c) / statistics.median(t)
                    row["verdict_" + arm] = "call wins" if max(c) < min(t) else "call loses" if max(t) < min(c) else "tie"
            res["rows"].append(row)
    print(json.dumps(res, indent=1))
    if args.out:
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
