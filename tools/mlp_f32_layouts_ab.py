"""A/B of batch-contiguous (SoA) against AoS matrices on a fused fp32 network module (csrc/mlp_f32_fused.hip), two arms
of ONE module in one process through the C-ABI:

  A  tcnn_module_*_layout with mask 0 (the AoS entries: [B][32] in, [B][16] padded out)
  S  the same calls with every layout bit set ([32][B] in, [1][B] out, [1][B] dL/doutput, [32][B] dL/dinput)

on Network(32, 1, FullyFusedMLP, W 64, 2 hidden layers, ReLU) at B = 2^16, for inference and for forward + backward
with dL/dinput only (the SDF-normal call). The arms alternate window by window; medians of the windows (wall clock,
synchronised at a window's two ends only) and the windows themselves. A layout wins a row only if the two arms' window
ranges do not overlap. Beside the times, the floats per batch row the network's launches move, counted from the code.

  python tools/mlp_f32_layouts_ab.py [--out profiles/mlp_f32_layouts_ab.json] [--windows 5] [--steps 200]
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

N_IN, N_OUT, OUTP, W, NH = 32, 1, 16, 64, 2
FLOATS_PER_ROW = {  # counted from csrc/mlp_f32_fused.hip, not measured; weights stay in L2
    # AoS: the Identity launch (x read, e written), then the network's (e read, padded y written). SoA: the first
    # layer reads x as it lies, no Identity launch, and one output float
    "inference": {"aos": 2 * N_IN + (N_IN + OUTP), "soa": N_IN + N_OUT},
    # forward keeping [e | h_1 h_2 | y] AoS and writing the caller's output; chain (output activation None: y is not
    # read back): dL/dy and the hidden values read, D_0 written; AoS then runs Identity's backward (D_0 read, dL/dinput
    # written), SoA's D_0 is dL/dinput
    "input_grad": {"aos": 2 * N_IN + (N_IN + NH * W + 2 * OUTP) + (OUTP + NH * W + N_IN) + 2 * N_IN,
                   "soa": (N_IN + N_IN + NH * W + OUTP + N_OUT) + (N_OUT + NH * W + N_IN)},
}


def vp(t):
    return ctypes.c_void_p(t.data_ptr())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--log2b", type=int, default=16)
    args = ap.parse_args()
    import torch
    from tinycudann import _lib as L

    lib, B = L.lib(), 1 << args.log2b
    net = {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": W, "n_hidden_layers": NH}
    m = L.check_ptr(lib.tcnn_create_network_precision(N_IN, N_OUT, json.dumps(net).encode(), 0))
    assert lib.tcnn_module_engine(m) == b"fused"
    p = torch.zeros(lib.tcnn_module_n_params(m), device="cuda")
    L.check(lib.tcnn_module_initialize_params(m, 1337, vp(p), 1.0))
    x = torch.rand(B, N_IN, device="cuda")
    bufs = {0: (x, torch.empty(B, OUTP, device="cuda"), torch.zeros(B, OUTP, device="cuda"), torch.empty(B, N_IN, device="cuda")),
            15: (x.T.contiguous(), torch.empty(N_OUT, B, device="cuda"), torch.ones(N_OUT, B, device="cuda"), torch.empty(N_IN, B, device="cuda"))}
    bufs[0][2][:, :N_OUT] = 1.0

    def make_step(mask, mode):
        xi, out, dout, dx = bufs[mask]
        if mode == "inference":
            return lambda: L.check(lib.tcnn_module_inference_layout(m, None, B, vp(xi), vp(out), vp(p), mask))

        def step():
            ctx = L.check_ptr(lib.tcnn_module_forward_layout(m, None, B, vp(xi), vp(out), vp(p), 1, mask))
            L.check(lib.tcnn_module_backward_layout(m, None, ctx, B, vp(dx), vp(dout), None, vp(xi), vp(out), vp(p), mask))
            lib.tcnn_context_destroy(ctx)
        return step

    res = {"batch": B, "windows": args.windows, "steps_per_window": args.steps,
           "network": {"n_in": N_IN, "n_hidden_layers": NH, "n_neurons": W, "n_out": N_OUT, "activation": "ReLU"}, "rows": {}}
    for mode in ("inference", "input_grad"):
        arms = {"aos": make_step(0, mode), "soa": make_step(15, mode)}
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
        a, s = us["aos"], us["soa"]
        res["rows"][mode] = {"floats_per_row_counted": FLOATS_PER_ROW[mode],
                             "aos_us": {"median": statistics.median(a), "windows": a},
                             "soa_us": {"median": statistics.median(s), "windows": s},
                             "soa_over_aos": statistics.median(s) / statistics.median(a),
                             "verdict": "soa wins" if max(s) < min(a) else "soa loses" if max(a) < min(s) else "tie"}
    same = torch.equal(bufs[15][1].T, bufs[0][1][:, :N_OUT]) and torch.equal(bufs[15][3].T, bufs[0][3])
    res["soa_bits_equal_aos"] = bool(same)
    lib.tcnn_module_destroy(m)
    print(json.dumps(res, indent=1))
    if args.out:
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
