# Bit-identity check between two builds of the engine (TCNN_LIB_PATH selects the library): a few
# training steps of config_hash at several batch sizes and position mixes; prints one digest per case
# (params fp32 + fp16 after 4 steps) and the 4 losses. Run once per build and compare the lines.
import hashlib
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "neuralbtf-tiny-cuda-nn_amd"))

import torch  # noqa: E402

from tinycudann import Trainer  # noqa: E402

cfg = json.load(open(os.path.join(REPO, "tests", "golden", "config_hash.json")))
g = torch.Generator(device="cuda").manual_seed(7)
for B, frac_out in ((1 << 15, 0.0), (1 << 18, 0.0), ((1 << 16) + 256, 0.0), (1 << 16, 0.002)):
    t = Trainer(2, 3, cfg, seed=1337)
    assert t.engine == "fused", t.engine
    h = hashlib.sha256()
    losses = []
    for step in range(4):
        pos = torch.rand(B, 2, device="cuda", generator=g)
        if frac_out:
            m = torch.rand(B, device="cuda", generator=g) < frac_out
            pos[m, 0] = 1.25
        tgt = torch.stack([0.5 + 0.5 * torch.sin(9 * pos[:, 0]), pos[:, 1], pos[:, 0] * pos[:, 1]], 1).contiguous()
        t.training_step(pos, tgt, run_optimizer=True)
        losses.append(t.loss())
    torch.cuda.synchronize()
    h.update(t.params_fp32().cpu().numpy().tobytes())
    h.update(t.params().cpu().numpy().tobytes())
    print("case", B, frac_out, h.hexdigest()[:16], "losses", " ".join("%.9g" % v for v in losses), flush=True)
    del t

# Encoding-Module backward (tcnn_module_backward, as _module_grad in tests/test_gpu_grid_large.py): one
# digest of dL/dparams per grid-backward path, at B = 256 (one chunk, replicas on the coarse levels) and
# B = 16640 (two chunks, a partial last batch), 0.2 % of the positions outside [0, 1].
import ctypes  # noqa: E402

import numpy as np  # noqa: E402

from tinycudann import _lib as L  # noqa: E402

FP32, FP16 = 0, 1
ENC = cfg["encoding"]
HASH = {"otype": "HashGrid", "type": "Hash", "interpolation": "Linear"}
MODULE_CASES = [
    # name, D, encoding, precision, environment, per-point max_level
    ("d3_f4_hash", 3, dict(HASH, n_levels=6, n_features_per_level=4, log2_hashmap_size=14, base_resolution=8, per_level_scale=1.5), FP16, {}, False),
    ("d2_f8", 2, dict(HASH, n_levels=6, n_features_per_level=8, log2_hashmap_size=15, base_resolution=16, per_level_scale=2.0), FP16, {}, False),
    ("d3_tiled", 3, dict(HASH, type="Tiled", n_levels=6, n_features_per_level=2, base_resolution=24, per_level_scale=1.5), FP16, {}, False),
    ("log2t19", 2, dict(ENC, log2_hashmap_size=19, per_level_scale=2.0), FP16, {}, False),
    ("config_hash_feature_plan", 2, ENC, FP16, {"TCNN_GRID_BWD_PLAN": "feature"}, False),
    ("nearest", 2, dict(ENC, interpolation="Nearest"), FP16, {}, False),
    ("smoothstep", 2, dict(ENC, interpolation="Smoothstep"), FP16, {}, False),
    ("stochastic", 2, dict(ENC, stochastic_interpolation=True), FP16, {}, False),
    ("max_level_per_point", 2, ENC, FP16, {}, True),
    ("fp32_f2", 2, ENC, FP32, {}, False),
    ("fp32_f4", 2, dict(HASH, n_levels=8, n_features_per_level=4, log2_hashmap_size=16, base_resolution=16, per_level_scale=2.0), FP32, {}, False),
]


def _vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def module_grad_digest(D, enc, precision, env, per_point, B):
    lib = L.lib()
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)  # the plan switch is read when the module is built
    m = L.check_ptr(lib.tcnn_create_encoding(D, json.dumps(enc).encode(), precision))
    for k, v in old.items():  # the caller's own setting comes back
        if v is None:
            del os.environ[k]
        else:
            os.environ[k] = v
    try:
        dt = torch.float32 if precision == FP32 else torch.float16
        rng = np.random.default_rng(1000 + B)
        pos = rng.random((B, D), dtype=np.float32)
        out_idx = rng.choice(B, max(1, B // 500), replace=False)
        pos[out_idx] += rng.choice(np.array([-0.7, 1.5], np.float32), (out_idx.size, 1))
        W, n = lib.tcnn_module_n_output_dims(m), lib.tcnn_module_n_params(m)
        p32 = torch.zeros(n, dtype=torch.float32, device="cuda")
        L.check(lib.tcnn_module_initialize_params(m, 1337, _vp(p32), 1.0))
        p = p32.to(dt)
        pos_d = torch.from_numpy(pos).cuda()
        if per_point:
            ml = torch.from_numpy(rng.random(B, dtype=np.float32)).cuda()
            L.check(lib.tcnn_module_set_max_level_gpu(m, _vp(ml)))
        out = torch.empty(B, W, dtype=dt, device="cuda")
        ctx = L.check_ptr(lib.tcnn_module_forward(m, None, B, _vp(pos_d), _vp(out), _vp(p), 0))
        dy = torch.from_numpy(rng.standard_normal((B, W)).astype(np.float32)).cuda().to(dt)
        grad = torch.empty(n, dtype=dt, device="cuda")
        L.check(lib.tcnn_module_backward(m, None, ctx, B, None, _vp(dy), _vp(grad), _vp(pos_d), _vp(out), _vp(p)))
        torch.cuda.synchronize()
        lib.tcnn_context_destroy(ctx)
        g = grad.cpu().numpy()
        return hashlib.sha256(g.tobytes()).hexdigest()[:16], float(np.abs(g.astype(np.float64)).sum())
    finally:
        lib.tcnn_module_destroy(m)


for name, D, enc, precision, env, per_point in MODULE_CASES:
    for B in (256, 16640):
        print("module", name, B, "%s sum|g|=%.9g" % module_grad_digest(D, enc, precision, env, per_point, B), flush=True)
