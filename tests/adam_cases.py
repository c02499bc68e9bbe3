"""Optimizer blocks of the Adam option tests, shared by tests/test_adam_reference.py (the oracle's Adam
against a float64 restatement, CPU) and tests/test_gpu_adam_options.py (the engine's five Adam paths against
the oracle, bit for bit): the cases, the crafted optimizer state and the models the GPU tests train.

A case is (optimizer block, loss scale). Keys a block leaves out take Adam's defaults (learning_rate 1e-3,
beta1 0.9, beta2 0.999, epsilon 1e-8, l2_reg 1e-8, no decay, no clipping, factor 1, both classes trained).
"""
import copy

import numpy as np

from helpers import CONFIG_HASH, CONFIG_ONEBLOB

CASES = {
    "default": ({}, 128.0),
    # both decays, a learning rate at which rel_decay * lr and abs_decay * lr move every master
    "decay": ({"learning_rate": 1e-2, "relative_decay": 0.05, "absolute_decay": 2e-3}, 128.0),
    # the clip at the learning rate: a first Adam step moves a parameter by lr against its gradient's sign, so of
    # the grid entries (|w| <= 1e-4 at init) those that move away from zero are clipped, about half
    "clip": ({"clipping_magnitude": 1e-3}, 128.0),
    # (the learning rate lifts the l2 term's share of a step, ~1e-4 of it, above the masters' fp32 spacing)
    "l2_nonmat": ({"learning_rate": 1e-2, "l2_reg": 1e-3, "non_matrix_learning_rate_factor": 0.25}, 128.0),
    "adabound_upper": ({"adabound": True}, 128.0),
    "adabound_lower": ({"adabound": True, "learning_rate": 1e-8}, 128.0),
    "freeze_matrix": ({"optimize_matrix_params": False}, 128.0),
    "freeze_nonmatrix": ({"optimize_non_matrix_params": False}, 128.0),
    "betas_eps": ({"beta1": 0.5, "beta2": 0.9, "epsilon": 1e-3}, 128.0),
    "loss_scale_100": ({}, 100.0),  # not a power of two: the division branch
    "loss_scale_1": ({}, 1.0),
    # decay, clip, factor, betas and the division together. The clip sits at the non-matrix step lr * factor (half
    # the moving grid entries, as in "clip") and inside the range of the network's initial weights (|w| < 0.2,
    # moved by lr = 0.1), so it binds on a part of either class in every model
    # (the absolute decay pulls a grid entry back by 2e-4 * lr * factor ~ 1e-5, a tenth of its initial range)
    "combined": ({"learning_rate": 0.1, "relative_decay": 0.05, "absolute_decay": 2e-4, "clipping_magnitude": 0.05,
                  "non_matrix_learning_rate_factor": 0.5, "l2_reg": 1e-3, "beta1": 0.8, "beta2": 0.95}, 100.0),
}
CASE_NAMES = list(CASES)

# what a case is named for: the block with these keys removed is the same update without the feature
NAMED_KEYS = {
    "decay": ("relative_decay", "absolute_decay"),
    "l2_nonmat": ("l2_reg", "non_matrix_learning_rate_factor"),
    "betas_eps": ("beta1", "beta2", "epsilon"),
}


def optimizer_block(case):
    return dict({"otype": "Adam"}, **CASES[case][0])


def loss_scale(case):
    return CASES[case][1]


def with_optimizer(cfg, case):
    """cfg with its optimizer block replaced by the case's"""
    c = copy.deepcopy(cfg)
    c["optimizer"] = optimizer_block(case)
    return c


# ---------------------------------------------------------------------------------------------
# the crafted optimizer state
# ---------------------------------------------------------------------------------------------
CRAFT_N = 4099        # a few thousand parameters, not a multiple of 4 (nor of the 64-periodic specials)
CRAFT_N_MATRIX = 2050  # class boundary: 2050 % 4 == 2
CRAFT_GLOBAL_STEP = 50  # optimizer steps taken before the first tested one; every per-parameter count differs from it

F16_MAX, F16_SUBNORMAL_MIN, F16_NEG_SUBNORMAL_MAX, F16_NEG_ZERO = 0x7BFF, 0x0001, 0x83FF, 0x8000


def crafted_state(n=CRAFT_N, seed=20):
    """{"w32", "g16" (fp16 bits), "m1", "m2", "steps"} of n parameters: magnitudes spread over the decades a
    training run sees (gradients 1e-5 .. 30 before the loss scale is divided out, masters 1e-4 .. 1 of both signs,
    nonzero previous moments, per-parameter step counts 0 .. 40), with the special values planted every 64
    parameters so that any class boundary leaves every one of them in both classes:
      i % 64 == 0: gradient +0      1: gradient -0         2: +65504 (largest finite fp16)   3: -65504
               4: smallest fp16 subnormal   5: the negative subnormal of largest magnitude
               6: master +0         7: master -0           8: a fresh parameter (zero moments, step count 0)
               9: step count 0 with moments left over     10: gradient 0 on a master that only decays
    Gradients of +-0 are "zero in one class and nonzero in the other": a matrix parameter is updated through them
    (its gradient becomes l2_reg * w), a non-matrix parameter is skipped. No inf, no NaN."""
    rng = np.random.default_rng(seed)
    sign = lambda: rng.choice(np.float64([-1.0, 1.0]), n)
    g16 = (sign() * 10.0 ** rng.uniform(-5.0, 1.5, n)).astype(np.float16).view(np.uint16)
    w32 = (sign() * 10.0 ** rng.uniform(-4.0, 0.0, n)).astype(np.float32)
    m1 = (sign() * 10.0 ** rng.uniform(-7.0, -1.0, n)).astype(np.float32)
    m2 = (10.0 ** rng.uniform(-13.0, -2.0, n)).astype(np.float32)
    steps = rng.choice(np.uint32([1, 2, 3, 5, 9, 40]), n).astype(np.uint32)
    k = np.arange(n) % 64
    g16[k == 0] = 0
    g16[k == 1] = F16_NEG_ZERO
    g16[k == 2] = F16_MAX
    g16[k == 3] = F16_MAX | 0x8000
    g16[k == 4] = F16_SUBNORMAL_MIN
    g16[k == 5] = F16_NEG_SUBNORMAL_MAX
    w32[k == 6] = 0.0
    w32[k == 7] = -0.0
    m1[k == 8] = 0.0
    m2[k == 8] = 0.0
    steps[(k == 8) | (k == 9)] = 0
    g16[k == 10] = 0
    return {"w32": w32, "g16": g16, "m1": m1, "m2": m2, "steps": steps}


def tiled_state(n):
    """the crafted state repeated to n parameters"""
    return {k: np.resize(v, n).copy() for k, v in crafted_state().items()}


# ---------------------------------------------------------------------------------------------
# the models of the GPU tests
# ---------------------------------------------------------------------------------------------
def _cfg(base, encoding=None, network=None):
    c = copy.deepcopy(base)
    if encoding is not None:
        c["encoding"] = encoding
    c["network"].update(network or {})
    return c


# (a) the standalone kernel: a matrix-only model and the smallest grid model (both classes)
CFG_SMALL_ONEBLOB = _cfg(CONFIG_ONEBLOB, {"otype": "OneBlob", "n_bins": 16}, {"n_neurons": 32, "n_hidden_layers": 2})
CFG_SMALL_GRID = _cfg(CONFIG_HASH, dict(CONFIG_HASH["encoding"], log2_hashmap_size=8), {"n_neurons": 32, "n_hidden_layers": 2})
# (d) the smallest table of config_hash's grid with levels on both sides of the LDS budget (2^15 entries a level)
CFG_BINNED = _cfg(CONFIG_HASH, dict(CONFIG_HASH["encoding"], log2_hashmap_size=16))
# (e) the engines whose step ends in the standalone kernel
CFG_TILE = _cfg(CONFIG_HASH, None, {"n_neurons": 128, "n_hidden_layers": 2})
CFG_LAYERED = _cfg(CONFIG_ONEBLOB, None, {"otype": "CutlassMLP", "n_neurons": 64, "n_hidden_layers": 2})

SEQUENTIAL_CASES = ("combined", "adabound_upper", "freeze_matrix")
# (AdaBound too: its bounds reach the binned pass through arguments of its own)
BINNED_CASES = ("combined", "freeze_nonmatrix", "adabound_upper")
RANGE_CASES = ("combined", "freeze_nonmatrix")

# name -> (config, batch size, cases): the training steps whose gradients reach Adam on the GPU
TRAINED = {
    "fused": (CONFIG_HASH, 1024, tuple(CASE_NAMES)),
    "binned": (CFG_BINNED, 256, BINNED_CASES),
    "tile": (CFG_TILE, 1024, SEQUENTIAL_CASES),
    "layered": (CFG_LAYERED, 1024, SEQUENTIAL_CASES),
}
