"""Headline benchmark: training steps/s at batch 2^18 on data/config_hash.json (HashGrid L16 F2
log2T15 s1.5 + FullyFusedMLP 64x2, RelativeL2, Adam) -- BASELINE.json `metric`.

One step = Trainer::training_step over one 2^18-point batch resident in HBM: fused grid-encode +
MLP fwd + loss + MLP bwd + weight gradients, grid backward, reductions, Adam (and, with N>1 ranks,
the RCCL all-reduce of the gradient sums, overlapped with the grid backward). Synthetic data:
uniform positions, analytic RGB targets. Multi-GPU is data parallel:
  --scaling strong (default; BASELINE configs[4] / SURVEY C5): the global 2^18 batch is sharded
      2^18/N points per rank; `value` = global 2^18-sample steps per second;
  --scaling weak: every rank trains on its own 2^18 batch; `value` = 2^18-sample steps completed by
      all ranks per second.

  python bench.py [--gpus N --steps K --warmup W] [--dump-outputs DIR] [--full]
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
      --master-port P bench.py --gpus N --steps K --warmup W

A plain run sets up, warms up, times the K steps and prints the result line. --full adds what takes
runs of its own: the profiled pass behind `phase_ms` / `roofline` and the CPU baseline
(`cpu_baseline`); --no-profile / --no-cpu-baseline drop either again. --dump-outputs DIR writes what
the last timed step left with the caller (DIR/<name>.npy, see dump_outputs); the inputs are seeded,
so two builds run with the same arguments can be compared array for array.
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(REPO, "neuralbtf-tiny-cuda-nn_amd")
for _p in (REPO, PKG):
    if _p not in sys.path:
        sys.path.insert(0, _p)

# MI355X peaks (/opt/skills/guides/MI355X_MICROARCH.md): dense fp16 MFMA, HBM3E
PEAK_FP16_TFLOPS = 2500.0
PEAK_HBM_GBS = 8000.0
# Algorithmic work per training sample (config_hash: W64 H2 in32 out_p16 D2 L16 F2)
MLP_TRAIN_FLOP_PER_SAMPLE = 43008
GRID_BWD_BYTES_PER_SAMPLE = 584
PHASES = ["fused_grid_mlp_fwd_loss_bwd", "grid_bwd_with_network_adam_tail", "adam_grid_slab_sums", "loss_sum"]
ADAM_BYTES_PER_PARAM = 36  # Adam's fp32 master/m/v/step + fp16 grad/weight traffic
# Per-kernel phase times come from hipEvents the trainer records on its stream (tcnn_trainer_profile_*)
# during a profiled pass of PHASE_STEPS steps run right after the timed region, events on every
# PHASE_EVERY-th step: each event record idles the GPU ~6 us (~5 records per sampled step), so events
# inside the timed region would bias `value` (r04: every 25th timed step, i.e. ONE sampled step in the
# driver's 20-step run -- VERDICT r04 weak item 8)
PHASE_STEPS = 100
PHASE_EVERY = 2


def rgb_field_torch(pos):
    import torch
    x, y = pos[:, 0].double(), pos[:, 1].double()
    r = 0.5 + 0.5 * torch.sin(9.0 * x) * torch.cos(7.0 * y)
    g = 0.5 + 0.4 * torch.sin(23.0 * x * y + 1.0)
    b = 0.5 + 0.3 * torch.cos(31.0 * x) * torch.sin(17.0 * y) + 0.1 * (torch.floor(x * 40) % 2)
    return torch.stack([r, g, b], dim=1).float().contiguous()


def _cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_baseline(cfg):
    """CPU restatement (oracle/, fp32 OpenMP) timed on the host: the `port` baseline (the reference
    has no CPU path). Bounded sample (~30 s): every core this process's affinity mask
    allows at C3 (B=2^18, the bench workload -- `value`, `cores` = that count), the box's CPU share
    (OMP_NUM_THREADS, 16 on the GPU box) at C3 and C1 (B=2^16), and one thread at C1. Each timed after
    one warm-up step."""
    import numpy as np
    from oracle import oracle as O
    threads = int(os.environ.get("OMP_NUM_THREADS", "0") or 0) or min(16, os.cpu_count() or 1)
    try:
        all_cores = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        all_cores = os.cpu_count() or threads

    def timed(B, n_threads, budget_s, max_steps):
        om = O.OracleModel(cfg, 2, 3, seed=1337)
        r = O.pcg32(1337)
        pos = O.generate_uniform(r, 2 * B).reshape(B, 2)
        tgt = np.stack([0.5 + 0.5 * np.sin(9 * pos[:, 0]), pos[:, 1], pos[:, 0] * pos[:, 1]], axis=1).astype(np.float32)
        om.train_step(pos, tgt, n_threads=n_threads)  # warm-up
        n, t0 = 0, time.perf_counter()
        while True:
            om.train_step(pos, tgt, n_threads=n_threads)
            n += 1
            el = time.perf_counter() - t0
            if el >= budget_s or n >= max_steps:
                return n / el, n, el

    ca, na, ea = timed(1 << 18, all_cores, 6.0, 100)
    c3, n3, e3 = timed(1 << 18, threads, 8.0, 50)
    c1, n1, e1 = timed(1 << 16, threads, 4.0, 100)
    s1, ns1, es1 = timed(1 << 16, 1, 6.0, 20)
    # `value`: the faster of all affinity-visible cores and the box's CPU share (on the GPU box the
    # affinity mask shows the whole host, 256 cores, but the job's CPU share is 16: the 256-thread run
    # is oversubscribed and slower -- both are reported)
    best_all = ca >= c3
    return {
        "value": ca if best_all else c3,
        "unit": "training steps/s (2^18-sample batches)",
        "cores": all_cores if best_all else threads,
        "kind": "port",
        "cpu": _cpu_model(),
        "sample": f"oracle training steps of config_hash.json on the GPU box's host ({_cpu_model()}): "
                  f"C3 B=2^18 on {all_cores} affinity-visible cores: {na} steps in {ea:.1f} s ({ca:.3f}/s); "
                  f"on the {threads}-thread CPU share: {n3} steps in {e3:.1f} s ({c3:.3f}/s)",
        "variants": {
            f"C3_2^18_{all_cores}threads_all_affinity_cores_steps_per_s": ca,
            f"C3_2^18_{threads}threads_steps_per_s": c3,
            f"C1_2^16_{threads}threads_steps_per_s": c1,
            "C1_2^16_1thread_steps_per_s": s1,
            "C1_samples": f"{n1} steps in {e1:.1f} s ({threads} threads), {ns1} steps in {es1:.1f} s (1 thread)",
        },
    }


DEFAULT_WORKLOAD = "HashGrid L16 F2 log2T15 s1.5 base16 + FullyFusedMLP W64 H2 ReLU, RelativeL2, Adam, B=2^18"


def workload_tag(cfg, B):
    """the workload's name, derived from the loaded config and the per-rank batch (it also keys the
    committed PMC traffic files, so a variant's line never carries another config's bytes)"""
    e, n = cfg.get("encoding", {}), cfg.get("network", {})
    eo = e.get("otype", "OneBlob")
    if eo.lower() in ("hashgrid", "grid", "densegrid", "tiledgrid"):
        L = e.get("n_levels", 16)
        enc = (f"{eo} L{L} F{e.get('n_features_per_level', 2)} log2T{e.get('log2_hashmap_size', 19)} "
               f"s{e.get('per_level_scale', 2.0):g} base{e.get('base_resolution', 16)}")
    elif eo.lower() == "oneblob":
        enc = f"OneBlob bins{e.get('n_bins', 16)}"
    else:
        enc = eo
    lb = B.bit_length() - 1
    bs = f"2^{lb}" if B == 1 << lb else str(B)
    return (f"{enc} + {n.get('otype', 'MLP')} W{n.get('n_neurons', 128)} H{n.get('n_hidden_layers', 5)} "
            f"{n.get('activation', 'ReLU')}, {cfg.get('loss', {}).get('otype', 'RelativeL2')}, "
            f"{cfg.get('optimizer', {}).get('otype', 'Adam')}, B={bs}")


GRID_BWD_SLOTS = 32768  # int32 accumulators of one LDS item (grid_bwd_lds.h: 128 KiB)


def grid_binned_params(cfg, D=2):
    """Grid parameters of the levels the engine's binned backward takes (runtime.cpp: from the first
    level whose one feature exceeds an LDS item on; their Adam runs inside k_grid_acc). Level sizes
    as GridEncodingTemplated (grid.h:668-730) in float32."""
    import numpy as np
    e = cfg.get("encoding", {})
    if e.get("otype", "").lower() not in ("hashgrid", "grid", "densegrid", "tiledgrid"):
        return 0
    L, F = e.get("n_levels", 16), e.get("n_features_per_level", 2)
    log2T, base = e.get("log2_hashmap_size", 19), e.get("base_resolution", 16)
    gtype = e.get("type", "Hash" if e["otype"].lower() in ("hashgrid", "grid") else ("Tiled" if e["otype"].lower() == "tiledgrid" else "Dense"))
    ls = np.log2(np.float32(e.get("per_level_scale", 2.0)))
    sizes = []
    for l in range(L):
        scale = np.float32(np.exp2(np.float32(l) * ls)) * np.float32(base) - np.float32(1.0)
        res = int(np.ceil(scale)) + 1
        n = min(res ** D, 0xffffffff // 2)
        n = (n + 7) // 8 * 8
        if gtype.lower() == "hash":
            n = min(n, 1 << log2T)
        elif gtype.lower() == "tiled":
            n = min(n, base ** D)
        sizes.append(n)
    first = next((l for l in range(L) if sizes[l] > GRID_BWD_SLOTS), L)
    return sum(sizes[first:]) * F


def pmc_traffic(kernel, tag):
    """HBM bytes per launch of `kernel` from the newest committed PMC summary measured on the SAME
    workload (profiles/*_pmc_traffic*.json whose "workload" equals `tag`; files without the key
    predate it and were measured on the default workload), tools/pmc_traffic.py: FETCH_SIZE x2 +
    WRITE_SIZE; None when no such file exists."""
    import glob
    files = sorted(glob.glob(os.path.join(REPO, "profiles", "*_pmc_traffic*.json")))
    for f in reversed(files):
        try:
            d = json.load(open(f))
            if d.get("workload", DEFAULT_WORKLOAD) != tag:
                continue
            k = d["kernels"].get(kernel)
            return k["hbm_bytes"] if k else None
        except (OSError, ValueError, KeyError):
            continue
    return None


DUMP_MAX_ELEMS = 4 << 20  # per array: 16 MiB of float32, three arrays at the most -> under 64 MB in all


def dump_outputs(out_dir, arrays):
    """Write what the last timed step left with the caller as out_dir/<name>.npy (float32; the loss
    float64): `params` = the fp16 parameters the step updated, `params_fp32` = their fp32 masters
    (single GPU: with a sharded optimizer a rank holds only its shard), `loss` = the step's loss. An
    array above DUMP_MAX_ELEMS is cut to a fixed sample (sorted indices of a generator seeded with
    1337, a function of the array's length alone)."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    shapes = {}
    for name, a in arrays.items():
        a = np.ascontiguousarray(a)
        if a.size > DUMP_MAX_ELEMS:
            idx = np.sort(np.random.default_rng(1337).choice(a.size, DUMP_MAX_ELEMS, replace=False))
            a = a.reshape(-1)[idx]
        np.save(os.path.join(out_dir, name + ".npy"), a)
        shapes[name] = list(a.shape)
    return shapes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch-log2", type=int, default=18)
    ap.add_argument("--config", default=os.path.join(REPO, "tests", "golden", "config_hash.json"))
    ap.add_argument("--log2-hashmap-size", type=int, default=None, help="override encoding.log2_hashmap_size")
    ap.add_argument("--per-level-scale", type=float, default=None, help="override encoding.per_level_scale")
    ap.add_argument("--full", action="store_true",
                    help="also run the profiled pass (phase_ms, roofline) and the CPU baseline (cpu_baseline)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed (parameters, loss) as DIR/<name>.npy")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-profile", action="store_true", help="with --full: skip the profiled pass")
    ap.add_argument("--dist-backend", default="nccl", help="nccl (= RCCL on ROCm) or gloo (rehearsal)")
    ap.add_argument("--scaling", choices=["strong", "weak"], default="strong",
                    help="strong: shard the global batch over ranks (configs[4]); weak: a full batch per rank")
    ap.add_argument("--allreduce-dtype", choices=["fp32", "fp16"], default="fp32")
    ap.add_argument("--no-overlap", action="store_true", help="all-reduce after the whole backward")
    ap.add_argument("--optimizer", choices=["sharded", "replicated"], default="sharded",
                    help="N > 1: sharded (default) = each rank's Adam on 1/N of the parameters after summing that shard's "
                         "gradients, then the fp16 parameters gathered; replicated = all-reduce of the gradient sums, Adam "
                         "everywhere (exchange torch/engine only)")
    ap.add_argument("--exchange", choices=["peer", "engine", "torch"], default="peer",
                    help="N > 1: peer (default) = the engine sums the shards straight from the other ranks' memory over "
                         "xGMI (csrc/dp_peer.hip; falls back to engine if a rank cannot map its peers); engine = RCCL "
                         "issued by the training step itself (tcnn_trainer_set_dp); torch = torch.distributed collectives "
                         "driven from Python")
    ap.add_argument("--graph", action="store_true", help="replay the single-GPU training step as a hipGraph")
    ap.add_argument("--all-ranks-on-device0", action="store_true",
                    help="rehearse N>1 on a 1-GPU box (gloo); never used for measurements")
    ap.add_argument("--print-workload", action="store_true", help="print the workload tag and exit (no GPU)")
    args = ap.parse_args()

    if args.print_workload:
        cfg = json.load(open(args.config))
        if args.log2_hashmap_size is not None:
            cfg["encoding"]["log2_hashmap_size"] = args.log2_hashmap_size
        if args.per_level_scale is not None:
            cfg["encoding"]["per_level_scale"] = args.per_level_scale
        world = int(os.environ.get("WORLD_SIZE", "1"))
        B = (1 << args.batch_log2) // (world if args.scaling == "strong" else 1)
        print(workload_tag(cfg, B))
        return

    if args.graph:
        # the HIP runtime's graph packet capture costs ~5 us between consecutive replays; without it
        # replay is within ~1 us of the eager step (profiles/r06_graph_env.txt). Read at HIP init.
        os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")
    import torch
    import torch.distributed as dist

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    dev = 0 if args.all_ranks_on_device0 else local_rank
    torch.cuda.set_device(dev)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if args.dist_backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", dev))
        else:
            dist.init_process_group(args.dist_backend)

    from tinycudann import Trainer
    import ctypes
    from tinycudann import _lib as L

    cfg = json.load(open(args.config))
    if args.log2_hashmap_size is not None:
        cfg["encoding"]["log2_hashmap_size"] = args.log2_hashmap_size
    if args.per_level_scale is not None:
        cfg["encoding"]["per_level_scale"] = args.per_level_scale
    B_global = 1 << args.batch_log2
    B = B_global // world if args.scaling == "strong" else B_global  # this rank's points per step
    assert B % 256 == 0, "per-rank batch must be a multiple of 256"
    tag = workload_tag(cfg, B)
    trainer = Trainer(2, 3, cfg, seed=1337)
    g = torch.Generator(device="cuda")
    g.manual_seed(1337 + 7919 * rank)
    NB = 4
    batches = []
    for _ in range(NB):
        pos = torch.rand(B, 2, device="cuda", generator=g).contiguous()
        batches.append((pos, rgb_field_torch(pos)))

    from tinycudann.parallel import DataParallelTrainer
    sharded = world > 1 and args.optimizer == "sharded" and args.allreduce_dtype == "fp32"
    exchange = args.exchange if args.allreduce_dtype == "fp32" else "torch"
    if exchange == "peer":
        sharded = world > 1  # the peer exchange is the sharded schedule
    # a peer wait that cannot complete ends the run after 60 s instead of the library's 300 s default
    # (a benchmark step is microseconds; nothing rank-0-only runs between its steps)
    dp = DataParallelTrainer(trainer, overlap=not args.no_overlap, allreduce_dtype=args.allreduce_dtype,
                             shard_optimizer=sharded, exchange=exchange, peer_fallback=True, peer_timeout_s=60.0)
    exchange = dp.exchange  # what actually runs (peer falls back to engine collectively)
    if args.graph:
        trainer.set_graph(True)

    def step(i):
        pos, tgt = batches[i % NB]
        dp.training_step(pos, tgt)

    for i in range(args.warmup):
        step(i)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.steps):
        step(i)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    if world > 1:
        dist.barrier()
    elapsed = t1 - t0
    if world > 1:
        e = torch.tensor([elapsed], dtype=torch.float64, device="cuda" if args.dist_backend == "nccl" else "cpu")
        dist.all_reduce(e, op=dist.ReduceOp.MAX)
        elapsed = float(e.item())

    dumped = None
    if args.dump_outputs is not None and rank == 0:
        # device copies now: the profiled pass of --full trains on
        dumped = {"params": trainer.params().float()}
        if world == 1:
            dumped["params_fp32"] = trainer.params_fp32().clone()
        dumped_loss = trainer.loss()

    phase_ms = None
    if args.full and not args.no_profile:
        # the profiled pass: the same step on the same batches, events on every PHASE_EVERY-th step
        L.check(L.lib().tcnn_trainer_profile_begin_sampled(trainer.h, PHASE_EVERY))
        for i in range(PHASE_STEPS):
            step(i)
        torch.cuda.synchronize()
        ms = (ctypes.c_double * len(PHASES))()
        nst = ctypes.c_uint32(0)
        L.check(L.lib().tcnn_trainer_profile_end(trainer.h, ms, len(PHASES), ctypes.byref(nst)))
        phase_ms = {PHASES[k]: ms[k] for k in range(len(PHASES))}
        phase_ms["sampled_steps"] = nst.value
        phase_ms["source"] = (f"hipEvents on the trainer's stream, every {PHASE_EVERY}th step of a {PHASE_STEPS}-step "
                              "pass right after the timed region (events inside it would bias value)")
        if world > 1:
            dist.barrier()

    loss = trainer.loss()
    dp.close()  # collective teardown on every rank (the peer exchange gathers its sharded state)
    if rank != 0:
        if world > 1:
            dist.destroy_process_group()
        return

    units = args.steps if args.scaling == "strong" else world * args.steps  # global 2^18-sample steps
    value = units / elapsed
    res = {
        "metric": "training steps/sec at batch=2^18, config_hash.json (HashGrid+64-wide MLP)",
        "value": value,
        "unit": "training steps/s (2^18-sample batches, whole job)",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": 1000.0 * elapsed / args.steps,
        "higher_is_better": True,
        "scaling": args.scaling,
        "vs_baseline": None,
        "dtype": "fp16 storage / fp32 MFMA accumulate",
        "data": "synthetic (uniform positions, analytic RGB targets), random-init weights (Trainer seed 1337)",
        "config": {
            "workload": tag,
            "config_file": os.path.relpath(args.config, REPO) + ("" if args.log2_hashmap_size is None and
                                                                args.per_level_scale is None else " (overridden)"),
            "global_batch": B * world, "per_gpu_batch": B,
            "parallelism": "dp1" if world == 1 else (f"dp{world} batch-sharded ({B_global}/{world} points per rank)" if args.scaling == "strong"
                            else f"dp{world} ({B} points per rank)") +
                           ((", fp32 reduce-scatter + Adam on 1/N of the parameters + fp16 all-gather (sharded optimizer)" if sharded else
                             f", {args.allreduce_dtype} all-reduce" + ("" if args.no_overlap else " overlapped with the grid backward")) +
                            (", peer-memory exchange over xGMI issued by the engine's step (no collective library)" if exchange == "peer" else
                             ", RCCL issued by the engine's step" if exchange == "engine" else ", torch.distributed from Python")
                            if world > 1 else ""),
        },
        "step_graph": bool(args.graph),
        "samples_per_s": value * B_global,
        "final_loss": loss,
    }
    if phase_ms and (phase_ms[PHASES[0]] > 0 or phase_ms[PHASES[1]] > 0):
        res["phase_ms"] = phase_ms
        t_fused = phase_ms[PHASES[0]]
        t_gbwd = phase_ms[PHASES[1]]
        if t_fused >= t_gbwd:
            achieved = MLP_TRAIN_FLOP_PER_SAMPLE * B / (t_fused * 1e-3) / 1e12
            res["roofline"] = {"kernel": "k_fused_train_grid", "bound": "mfma", "achieved": achieved,
                               "peak": PEAK_FP16_TFLOPS, "unit": "TFLOP/s", "frac": achieved / PEAK_FP16_TFLOPS,
                               "traffic": pmc_traffic("k_fused_train_grid", tag)}
        else:
            # the grid backward launch also carries the network-gradient reduction + Adam on the
            # network parameters (16 extra workgroups); their bytes are < 1 % of the grid's
            nb = grid_binned_params(cfg)
            if nb == 0:
                achieved = GRID_BWD_BYTES_PER_SAMPLE * B / (t_gbwd * 1e-3) / 1e9
                res["roofline"] = {"kernel": "k_grid_bwd_lds", "bound": "hbm", "achieved": achieved,
                                   "peak": PEAK_HBM_GBS, "unit": "GB/s", "frac": achieved / PEAK_HBM_GBS,
                                   "traffic": pmc_traffic("k_grid_bwd_lds", tag)}
            else:
                # binned levels (e.g. log2T 19): the phase is k_grid_bwd_lds + k_grid_bin + k_grid_acc,
                # and k_grid_acc applies Adam to the binned parameters: algorithmic bytes = the grid
                # backward's per sample + Adam's per binned parameter; traffic = the three kernels'
                achieved = (GRID_BWD_BYTES_PER_SAMPLE * B + ADAM_BYTES_PER_PARAM * nb) / (t_gbwd * 1e-3) / 1e9
                parts = [pmc_traffic(k, tag) for k in ("k_grid_bwd_lds", "k_grid_bin", "k_grid_acc")]
                res["roofline"] = {"kernel": "grid backward phase: k_grid_bwd_lds + k_grid_bin + k_grid_acc (incl. Adam of "
                                             f"{nb} binned parameters)", "bound": "hbm", "achieved": achieved,
                                   "peak": PEAK_HBM_GBS, "unit": "GB/s", "frac": achieved / PEAK_HBM_GBS,
                                   "traffic": sum(parts) if all(p is not None for p in parts) else None}
    if dumped is not None:
        import numpy as np
        arrays = {k: v.cpu().numpy() for k, v in dumped.items()}
        arrays["loss"] = np.array([dumped_loss], dtype=np.float64)
        res["dumped_outputs"] = dump_outputs(args.dump_outputs, arrays)
    if args.full and world == 1 and not args.no_cpu_baseline:
        res["cpu_baseline"] = cpu_baseline(cfg)
    print(json.dumps(res))
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
