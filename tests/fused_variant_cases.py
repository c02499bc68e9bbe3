"""The register-resident fused training kernel (k_fused_train_grid / k_fused_train_grid_loss, csrc/mlp_fused.h) and
the fused forward (k_fused_fwd_grid) on 3-D grids and on every grid option they accept: cases, inputs and the CPU
side, shared by tests/test_fused_variants_reference.py (the oracle alone: the inputs are sound and each assertion
of the GPU file can fail) and tests/test_gpu_fused_variants.py (the HIP kernels against the oracle).

Cases. ENC is a 16-level F = 2 grid small enough for a 20 ms oracle step that still mixes dense and hashed levels
at D = 2 (levels 11-15 hashed) and D = 3 (levels 6-15). GRID_CASES: D in {2, 3} x the grid options at W64/H2 ReLU,
RelativeL2; SHAPE_CASES: the four fused shapes x hidden None / ReLU at D = 3, and one L2 case; NONE_CASES: hidden
None on every (D, hash) the others leave out, so that each (D, hash, activation) instantiation at W64/H2 runs.

Inputs. Parameters are the trainer's own seed-1337 initial fp32 parameters (the oracle's, bit-identical:
test_gpu_parity.py::test_trainer_init_matches_oracle) with the recipe of test_gpu_losses.scaled_params: the grid
table x 1e4 (uniform +-1, so a wrong hash or corner moves the loss and not only the gradients) and the 16 x W
output matrix replaced by its absolute values (outputs positive and O(1); with a signed output matrix only 6 % of
the samples are clear of an fp16 rounding boundary of the output). Positions are float32 uniform [0, 1)^D,
targets uniform [0.1, 1]. Per-element checks run on the first B samples of a 2 B pool (hidden None: 16 B,
pool_factor) that pass helpers.relu_margin_ok(check_output=True); aggregate checks on the first B of the pool,
unfiltered.
"""
import copy
import functools
import itertools

import numpy as np

from helpers import CONFIG_HASH, rel_err, relu_margin_ok
from oracle import oracle as O
from test_gpu_losses import scaled_params

SEED = 1337
B = 256  # the smallest batch training_step accepts (BATCH_GRANULARITY, the reference's): two workgroups of four 32-sample slices
B_INFER = 288  # a multiple of 32 (NetworkHost::inference) and not of k_fused_fwd_grid's 128-sample workgroup
N_OUT = 3
ENC = {"otype": "HashGrid", "n_levels": 16, "n_features_per_level": 2, "log2_hashmap_size": 12, "base_resolution": 4,
       "per_level_scale": 1.3}
GRID_OPTIONS = {
    "default": {},  # Hash, CoherentPrime, Linear
    "prime": {"hash": "Prime"},
    "reversedprime": {"hash": "ReversedPrime"},
    "tiled": {"type": "Tiled"},
    "dense": {"type": "Dense", "per_level_scale": 1.15},  # at 1.3 and D = 3: 31.8 M parameters
    "smoothstep": {"interpolation": "Smoothstep"},
    "nearest": {"interpolation": "Nearest"},
}
HASHES = ("CoherentPrime", "Prime", "ReversedPrime")
INTERPS = ("Linear", "Smoothstep", "Nearest")
FUSED_SHAPES = [(64, 2), (64, 1), (32, 2), (32, 1)]  # TCNN_FUSED_SHAPES, IN = 32


class Case:
    def __init__(self, name, D, enc=None, W=64, NH=2, act="ReLU", loss="RelativeL2"):
        self.id, self.D, self.W, self.NH, self.act, self.loss = name, D, W, NH, act, loss
        self.enc = dict(ENC, **(enc or {}))
        self.cfg = {
            "loss": {"otype": loss},
            "optimizer": copy.deepcopy(CONFIG_HASH["optimizer"]),
            "encoding": self.enc,
            "network": {"otype": "FullyFusedMLP", "activation": act, "output_activation": "None", "n_neurons": W, "n_hidden_layers": NH},
        }
        self.n_mlp = O.mlp_n_params(W, 32, NH, 16)

    def with_enc(self, **kw):
        """the same case with encoding keys replaced (the negative controls: another hash on the same table)"""
        return Case(self.id + "+" + ",".join(f"{k}={v}" for k, v in kw.items()), self.D, dict(self.enc, **kw), self.W, self.NH,
                    self.act, self.loss)

    def __repr__(self):
        return self.id


GRID_CASES = [Case(f"d{D}-{name}", D, opt) for D in (2, 3) for name, opt in GRID_OPTIONS.items()]
SHAPE_CASES = [Case(f"d3-w{W}h{NH}-{act}", 3, None, W, NH, act) for W, NH in FUSED_SHAPES for act in ("None", "ReLU")]
L2_CASE = Case("d3-w64h2-ReLU-L2", 3, loss="L2")
# the kernels are instantiated per (D, hash, hidden activation): hidden None on the hashes and dimensions the cases
# above leave out (D = 3 CoherentPrime is SHAPE_CASES' d3-w64h2-None)
NONE_CASES = [Case(f"d{D}-{h.lower()}-None", D, {"hash": h}, act="None") for D in (2, 3) for h in HASHES
              if (D, h) != (3, "CoherentPrime")]
ALL_CASES = GRID_CASES + SHAPE_CASES + [L2_CASE] + NONE_CASES
INFERENCE_CASES = GRID_CASES + NONE_CASES + [c for c in SHAPE_CASES if c.id == "d3-w64h2-None"]
BY_ID = {c.id: c for c in ALL_CASES}
assert len(BY_ID) == len(ALL_CASES)
# (b) batches with in-range, edge and out-of-range slices; (d) three optimizer steps; (f) the other losses
MIXED_RANGE_CASES = ["d3-default", "d3-dense", "d3-tiled", "d2-prime"]
ADAM_CASES = ["d3-default", "d3-tiled"]
SWEEP_CASE = "d3-default"
LOSS_SHAPE = "d3-w32h1-ReLU"


def grid(case):
    return O.grid_cfg(case.enc, case.D)


def oracle_model(case, w32=None):
    """the CPU model of a case; w32: its fp32 parameters (the fp16 copies rounded from them, as
    Trainer.set_params_full_precision does), default: the seed-1337 initialisation"""
    om = O.OracleModel(case.cfg, case.D, N_OUT, seed=SEED)
    assert om.n_mlp_params == case.n_mlp
    if w32 is not None:
        assert len(w32) == om.n_params, (case.id, len(w32), om.n_params)
        om.w32[:] = w32
        om.w16[:] = O.f2h(w32)
    return om


def test_params(case, w32_init):
    """the test parameters from the trainer's (or the oracle's) initial ones: test_gpu_losses.scaled_params"""
    return scaled_params(case.cfg, w32_init, case.n_mlp)


test_params.__test__ = False  # a helper, not a test


@functools.lru_cache(maxsize=None)
def cpu_params(case_id):
    """the test parameters from the oracle's initialisation (read-only)"""
    case = BY_ID[case_id]
    om = oracle_model(case)  # (its arrays are views of memory the model owns: keep it alive while they are read)
    w = test_params(case, om.w32)
    w.setflags(write=False)
    return w


def pool(case, n, seed=0):
    """n candidate samples: positions float32 uniform [0, 1)^D, targets uniform [0.1, 1]"""
    rng = np.random.default_rng(100 * case.D + seed)
    pos = rng.uniform(0.0, 1.0, (n, case.D)).astype(np.float32)
    pos = np.minimum(pos, np.float32(1.0 - 2.0 ** -24))  # float64 -> float32 may round up to 1.0
    tgt = rng.uniform(0.1, 1.0, (n, N_OUT)).astype(np.float32)
    return pos, tgt


def encode_rows(case, w16, pos):
    """the encoded rows [n][32] as float32 (fp16 values) the network sees"""
    return O.h2f(O.grid_fwd(grid(case), pos, np.asarray(w16, np.uint16)[case.n_mlp:])).T


def safe_mask(case, w16, pos):
    """helpers.relu_margin_ok per sample: clear of every hidden ReLU boundary (hidden None: no branch) and of the
    output's fp16 rounding boundaries"""
    w16 = np.asarray(w16, np.uint16)
    return relu_margin_ok(case.W, 32, case.NH, w16[:case.n_mlp], encode_rows(case, w16, pos), check_output=True, act=case.act)


def pool_factor(case):
    """The safe samples come from a pool of pool_factor x B candidates. ReLU: 2 (62-82 % of the candidates are safe,
    test_fused_variants_reference.py prints the share). Hidden None: 16, the module matrix's cap. The linear
    network's hidden values have both signs, so its outputs cancel (|y| ~ 0.3 against sum |w a| ~ 10, predictions
    in -1.2 .. 1.3) and the 2^-18 sum |w a| margin around an fp16 rounding boundary of y leaves 11-21 %."""
    return 2 if case.act == "ReLU" else 16


def batches(case, w32, n=B):
    """((positions, targets) of the first n pool samples, (positions, targets) of the first n safe samples of the
    pool_factor x n pool, the number of safe samples in the pool); asserts the pool yields n"""
    pos, tgt = pool(case, pool_factor(case) * n)
    ok = safe_mask(case, O.f2h(w32), pos)
    assert ok.sum() >= n, (case.id, int(ok.sum()), n)
    idx = np.flatnonzero(ok)[:n]
    return (pos[:n].copy(), tgt[:n].copy()), (np.ascontiguousarray(pos[idx]), np.ascontiguousarray(tgt[idx])), int(ok.sum())


def mixed_range_batch(case, n=B):
    """(b): slice 0 in range; slice 1 with one coordinate at exactly 1.0 and one at exactly 0.0 (in range: the
    branch-free index still applies); slice 2 with three positions in [-0.5, 0) u (1, 1.5] (the whole wave takes the
    general index); the other slices in range"""
    pos, tgt = pool(case, n, seed=7)
    pos[32 + 5, case.D - 1] = 1.0
    pos[32 + 20, 0] = 0.0
    pos[64 + 3, 0] = -0.25
    pos[64 + 17, case.D - 1] = 1.375
    pos[64 + 31] = np.linspace(1.5, -0.5, case.D, dtype=np.float32)  # every coordinate outside, both sides
    inside = np.all((pos >= 0) & (pos <= 1), axis=1)
    assert inside[:64].all() and inside[96:].all() and (~inside[64:96]).sum() == 3
    return pos, tgt


def oracle_step(case, w32, pos, tgt, n_threads=4):
    """one oracle training step without the optimizer: (loss, fp32 gradients [network | grid])"""
    om = oracle_model(case, w32)
    loss = om.train_step(pos, tgt, run_optimizer=False, n_threads=n_threads)
    return loss, np.array(om.grad32)


def oracle_outputs(case, w32, pos, n_threads=4):
    return O.h2f(oracle_model(case, w32).inference(pos, n_threads=n_threads))[:, :N_OUT]


def step_difference(case_a, case_b, w32, pos_a, pos_b, tgt):
    """what the GPU assertions would see if the kernel computed case_b on pos_b where case_a on pos_a was meant (same
    parameters): (relative loss difference, rel_err of the network gradients, rel_err of the grid gradients, share
    of outputs further apart than 40 fp16 ulps of the output scale)"""
    la, ga = oracle_step(case_a, w32, pos_a, tgt)
    lb, gb = oracle_step(case_b, w32, pos_b, tgt)
    ya, yb = oracle_outputs(case_a, w32, pos_a), oracle_outputs(case_b, w32, pos_b)
    ulp = float(np.spacing(np.float16(np.abs(ya).max())))
    nm = case_a.n_mlp
    return (abs(la - lb) / abs(la), rel_err(gb[:nm], ga[:nm]), rel_err(gb[nm:], ga[nm:]),
            float((np.abs(ya.astype(np.float64) - yb) > 40 * ulp).mean()))


def position_permutations(D):
    return [p for p in itertools.permutations(range(D)) if p != tuple(range(D))]


RATIOS_HEADER = """\
# Fused training kernel variants (tests/test_gpu_fused_variants.py) on the MI355X against the CPU oracle, per case:
# step: loss_rel = |loss - oracle| / |oracle|, mlp_rel / grid_rel = relative L2 error of the network / grid gradients
#       (bar 1e-3 each), pe_mlp / pe_grid = worst |got - oracle| / bound of the two per-element checks (bar 1)
# infer: the largest output error in fp16 ulps of the output scale (bar 4)
"""
