"""A/B of the torch training step with and without the engine's loss and optimizer objects, at B = 2^16 on
config_hash's and config_btf's models, three variants alternated window by window in one process:

  A  today's loop: the RelativeL2 torch expression + torch.optim.Adam(fused=True)
  B  tinycudann.Loss("RelativeL2") + torch.optim.Adam(fused=True)
  C  tinycudann.Loss("RelativeL2") + tinycudann.optim.Adam

Per variant: the median over the windows of the step time (wall clock over a window, synchronised at its two ends
only) and the host time by phase (timers around the five calls of a step, no synchronisation inside). A's own window
spread is the noise band against which C is judged.

  python tools/torch_objects_ab.py [--out profiles/torch_objects_ab.json] [--windows 5] [--steps 500]
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "neuralbtf-tiny-cuda-nn_amd")]

PHASES = ("forward", "loss", "zero_grad", "backward", "optimizer")


def make_variant(torch, tcnn, name, cfg, n_in, x, tgt):
    model = tcnn.NetworkWithInputEncoding(n_in, 3, cfg["encoding"], cfg["network"]).cuda()
    engine_loss = tcnn.Loss("RelativeL2")
    if name == "C":
        opt = tcnn.optim.Adam(tcnn.optim.param_groups(model, learning_rate=0.01))
    else:
        opt = torch.optim.Adam(model.parameters(), lr=0.01, fused=True)
    tgt16 = tgt.to(torch.float16)
    phases = dict.fromkeys(PHASES, 0.0)

    def step():
        t0 = time.perf_counter()
        out = model(x)
        t1 = time.perf_counter()
        if name == "A":
            loss = ((out - tgt16) ** 2 / (out.detach() ** 2 + 0.01)).mean()
        else:
            loss = engine_loss(out, tgt)
        t2 = time.perf_counter()
        opt.zero_grad()
        t3 = time.perf_counter()
        loss.backward()
        t4 = time.perf_counter()
        opt.step()
        t5 = time.perf_counter()
        for k, d in zip(PHASES, (t1 - t0, t2 - t1, t3 - t2, t4 - t3, t5 - t4)):
            phases[k] += d
    return step, phases


def run_model(torch, tcnn, cfg, n_in, B, windows, steps):
    x = torch.rand(B, n_in, device="cuda")
    tgt = torch.stack([0.5 + 0.4 * torch.sin(6 * x[:, 0]), x[:, 1], x[:, 0] * x[:, 1]], dim=1).contiguous()
    variants = {name: make_variant(torch, tcnn, name, cfg, n_in, x, tgt) for name in "ABC"}
    for step, _ in variants.values():
        for _ in range(50):
            step()
    torch.cuda.synchronize()
    step_us = {name: [] for name in variants}
    host_us = {name: {k: [] for k in PHASES} for name in variants}
    for _ in range(windows):
        for name, (step, phases) in variants.items():
            for k in PHASES:
                phases[k] = 0.0
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                step()
            torch.cuda.synchronize()
            step_us[name].append((time.perf_counter() - t0) * 1e6 / steps)
            for k in PHASES:
                host_us[name][k].append(phases[k] * 1e6 / steps)
    res = {}
    for name in variants:
        res[name] = {"step_us_median": statistics.median(step_us[name]), "step_us_windows": step_us[name],
                     "host_us_by_phase_median": {k: statistics.median(v) for k, v in host_us[name].items()}}
    a = res["A"]["step_us_windows"]
    res["noise_band_us"] = [min(a), max(a)]
    res["C_over_A"] = res["C"]["step_us_median"] / res["A"]["step_us_median"]
    res["C_not_slower_than_A_beyond_band"] = res["C"]["step_us_median"] <= max(a)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--log2b", type=int, default=16)
    args = ap.parse_args()
    import torch
    import tinycudann as tcnn

    B = 1 << args.log2b
    res = {"batch": B, "windows": args.windows, "steps_per_window": args.steps}
    for cfg_name, n_in in (("config_hash", 2), ("config_btf", 8)):
        cfg = json.load(open(os.path.join(REPO, "tests", "golden", cfg_name + ".json")))
        res[cfg_name] = run_model(torch, tcnn, cfg, n_in, B, args.windows, args.steps)
    print(json.dumps(res, indent=1))
    if args.out:
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
