"""The oracle's Adam (orc_adam_step, oracle/tcnn_oracle.c) against a float64 restatement of the reference's
per-parameter update (optimizers/adam.h:72-119, weight_decay in common_device.h:870-873), for every optimizer
block of tests/adam_cases.py -- the oracle is the yardstick tests/test_gpu_adam_options.py holds the engine to
bit for bit, so its option branches get a reference of their own first.

The restatement (adam_float64) takes the oracle's fp32 state before a step as exact numbers and evaluates, in
float64 and with the fp32 values of the hyperparameters:

    g   = g16 / loss_scale;   skipped when the class is frozen, or a non-matrix parameter has g == 0
    g  += l2_reg * w                                  (matrix parameters only)
    m1' = beta1 m1 + (1 - beta1) g,   m2' = beta2 m2 + (1 - beta2) g^2
    lr  = learning_rate [* non_matrix_learning_rate_factor] * sqrt(1 - beta2^t) / (1 - beta1^t),  t = ++steps[i]
    eff = clamp(lr / (sqrt(m2') + epsilon), lower, upper)
          lower = 0.1 - 0.1 / ((1 - beta2) T + 1), upper = 0.1 + 0.1 / ((1 - beta2) T)  with AdaBound, T the
          optimizer's global step; [0, FLT_MAX] without
    w'  = (1 - relative_decay lr) w - copysign(absolute_decay lr, w) - eff m1',  clamped to +-clipping_magnitude

The bound (per element, derived, not fitted). u = 2^-24 is the relative error of one fp32 rounding; rnd(x) =
u |x| + 2^-150 (the second term: results in the subnormal range). Every fp32 operation of the oracle's sequence
adds one rnd of its result to the propagated error of its operands; E(x) is the resulting bound of |oracle x -
exact x|:

    E(g)   = rnd(g16 / loss_scale) [+ rnd(g) for the fma of l2_reg]
    E(g^2) = 2 |g| E(g) + E(g)^2 + rnd(g^2)
    E(m1') = (1 - beta1) E(g) + 2 u |(1 - beta1) g| + rnd(m1')      (1 - beta1 is itself rounded: 2 u, not u)
    E(m2') = (1 - beta2) E(g^2) + 2 u |(1 - beta2) g^2| + rnd(m2')
    R(1 - b^t) = u (1 + 2 b^t / (1 - b^t))        powf within one ulp (2 u b^t), then the subtraction; relative
    R(lr)  = u [factor] + R(1 - beta2^t) / 2 + u [sqrtf] + R(1 - beta1^t) + u [division] + u [product]
    E(sqrt m2') = min(E(m2') / sqrt(m2'), sqrt(E(m2'))) + u sqrt(m2'),   E(d) = E(sqrt m2') + rnd(d), d = sqrt(m2') + epsilon
    E(eff) = max(eff0 ((R(lr) + E(d) / d) / (1 - E(d) / d) + u), E(lower), E(upper))   clamping is 1-Lipschitz
             with a = (1 - beta2) T (two roundings), b = a + 1, E(b) = 2 u a + u b, q = 0.1 / b:
             E(lower) = q (E(b) / b + u) + u lower (the cancellation in 0.1 - q keeps q's absolute error);
             E(upper) = 3 u (0.1 / a) + u upper
    E(w'unclipped) = |w| (|relative_decay lr| (R(lr) + u) + rnd(1 - relative_decay lr))
                     + |absolute_decay lr| (R(lr) + u) + rnd(decayed)
                     + |eff| E(m1') + |m1'| E(eff) + E(eff) E(m1') + rnd(w')

First-order terms are multiplied by 1.01 for the products of errors left out. With the default block the bound
is dominated by R(lr) at small t (beta2^t / (1 - beta2^t) ~ 1000 / t: the cancellation in 1 - beta2^t), about
1e-4 of the size of the update; a wrong sign, order or operand is an error of the size of a whole term. What
is discrete must agree exactly: which parameters are skipped (bit-unchanged in every array), the step counts,
the fp16 copy (the rounded master) and the clipped masters (+-clipping_magnitude exactly, wherever the
unclipped float64 value is outside the clip by more than its bound).
"""
import numpy as np
import pytest

import adam_cases as AC
from helpers import assert_adam_bits, bits, fresh_adam_state, make_batch, oracle_adam_step, oracle_grad16
from oracle import oracle as O

U = 2.0 ** -24
FLT_MAX = float(np.finfo(np.float32).max)
DEFAULTS = {"learning_rate": 1e-3, "beta1": 0.9, "beta2": 0.999, "epsilon": 1e-8, "l2_reg": 1e-8, "relative_decay": 0.0,
            "absolute_decay": 0.0, "clipping_magnitude": 0.0, "non_matrix_learning_rate_factor": 1.0, "adabound": False,
            "optimize_matrix_params": True, "optimize_non_matrix_params": True}


def rnd(x):
    return U * np.abs(x) + 2.0 ** -150


def hyper(opt):
    """the block's values as the fp32 numbers the optimizer holds"""
    h = dict(DEFAULTS)
    h.update({k: v for k, v in opt.items() if k in DEFAULTS})
    return {k: (bool(v) if isinstance(DEFAULTS[k], bool) else float(np.float32(v))) for k, v in h.items()}


def adabound_bounds(h, T):
    """(lower, upper, E(lower), E(upper)) of the effective learning rate at global step T"""
    if not h["adabound"]:
        return 0.0, FLT_MAX, 0.0, 0.0
    c = float(np.float32(0.1))
    a = (1.0 - h["beta2"]) * T  # two roundings: 1 - beta2 and the product
    b = a + 1.0
    Eb = 2 * U * a + U * b
    lo_q = c / b
    lower = c - lo_q
    E_lower = 1.01 * (lo_q * (Eb / b + U) + U * abs(lower)) + 2.0 ** -150
    up_q = c / a
    upper = c + up_q
    E_upper = 1.01 * (up_q * 3 * U + U * upper)
    return lower, upper, E_lower, E_upper


def adam_float64(opt, n_matrix, loss_scale, T, w32, g16, m1, m2, steps):
    """One step (global step T after its increment) from the fp32 state (w32, m1, m2, steps) and fp16 gradient
    bits g16, in float64. Returns {"updated", "w" (clipped), "w_unclipped", "m1", "m2", "steps", "E_w", "E_m1",
    "E_m2"}; rows of skipped parameters hold their inputs and zero bounds."""
    h = hyper(opt)
    n = w32.size
    w = w32.astype(np.float64)
    wsign = np.where(np.signbit(w32), -1.0, 1.0)  # copysign reads the sign bit: -0 counts as negative
    matrix = np.arange(n) < n_matrix
    g0 = O.h2f(g16).astype(np.float64) / float(np.float32(loss_scale))
    updated = np.where(matrix, h["optimize_matrix_params"], h["optimize_non_matrix_params"] & (g0 != 0.0))
    E_g = rnd(g0)
    g = np.where(matrix, h["l2_reg"] * w + g0, g0)
    E_g = E_g + np.where(matrix, rnd(g), 0.0)
    gsq = g * g
    E_gsq = 2 * np.abs(g) * E_g + E_g ** 2 + rnd(gsq)
    c1, c2 = 1.0 - h["beta1"], 1.0 - h["beta2"]
    m1n = h["beta1"] * m1.astype(np.float64) + c1 * g
    E_m1 = c1 * E_g + 2 * U * np.abs(c1 * g) + rnd(m1n)
    m2n = h["beta2"] * m2.astype(np.float64) + c2 * gsq
    E_m2 = c2 * E_gsq + 2 * U * np.abs(c2 * gsq) + rnd(m2n)
    t = steps.astype(np.float64) + 1.0
    p1, p2 = h["beta1"] ** t, h["beta2"] ** t
    R_q1, R_q2 = U * (1 + 2 * p1 / (1 - p1)), U * (1 + 2 * p2 / (1 - p2))
    lr = h["learning_rate"] * np.where(matrix, 1.0, h["non_matrix_learning_rate_factor"]) * np.sqrt(1 - p2) / (1 - p1)
    R_lr = 1.01 * (U + 0.5 * R_q2 + U + R_q1 + U + U)
    s = np.sqrt(m2n)
    E_s = np.minimum(E_m2 / np.maximum(s, 1e-300), np.sqrt(E_m2)) + U * s
    d = s + h["epsilon"]
    E_d = E_s + rnd(d)
    assert np.all(E_d < 0.25 * d)
    eff0 = lr / d
    E_eff0 = 1.01 * eff0 * ((R_lr + E_d / d) / (1 - E_d / d) + U)
    lower, upper, E_lower, E_upper = adabound_bounds(h, float(T))
    eff = np.clip(eff0, lower, upper)
    E_eff = np.maximum(E_eff0, max(E_lower, E_upper)) if h["adabound"] else E_eff0
    rd, ad = h["relative_decay"] * lr, h["absolute_decay"] * lr
    om = 1.0 - rd
    E_om = np.abs(rd) * (R_lr + U) + rnd(om) * (rd != 0.0)
    decayed = om * w - wsign * ad
    E_dec = np.abs(w) * E_om + np.abs(ad) * (R_lr + U) + rnd(decayed)
    nw = decayed - eff * m1n
    E_w = 1.01 * (E_dec + np.abs(eff) * E_m1 + np.abs(m1n) * E_eff + E_eff * E_m1) + rnd(nw)
    c = h["clipping_magnitude"]
    out = {"updated": updated, "w_unclipped": np.where(updated, nw, w),
           "w": np.where(updated, np.clip(nw, -c, c) if c != 0.0 else nw, w),
           "m1": np.where(updated, m1n, m1), "m2": np.where(updated, m2n, m2), "steps": np.where(updated, t, steps).astype(np.uint32),
           "E_w": np.where(updated, E_w, 0.0), "E_m1": np.where(updated, E_m1, 0.0), "E_m2": np.where(updated, E_m2, 0.0)}
    return out


def oracle_state():
    s = AC.crafted_state()
    g16 = s.pop("g16")
    s["w16"] = O.f2h(s["w32"])
    return s, g16


def step_gradients(g16, k):
    """the crafted gradients of step k: rotated by 5 k parameters (a multiple of neither 4 nor 16), so every
    special gradient meets other masters, moments and step counts on the later steps"""
    return np.roll(g16, 5 * k)


# ---------------------------------------------------------------------------------------------
# what the oracle's output says about the branches taken (from the oracle's arrays alone)
# ---------------------------------------------------------------------------------------------
def branch_stats(opt, n_matrix, T, before, after):
    """updated mask and the fractions of updated parameters on which the clip / AdaBound's upper / lower bound
    binds in a step of the oracle (global step T) from state `before` to `after`"""
    h = hyper(opt)
    upd = after["steps"] != before["steps"]
    n_upd = max(int(upd.sum()), 1)
    st = {"updated": upd, "n_updated": int(upd.sum())}
    c = np.float32(h["clipping_magnitude"])
    st["clip"] = float(np.sum(upd & (np.abs(after["w32"]) == c))) / n_upd if c != 0 else 0.0
    if h["adabound"]:
        matrix = np.arange(upd.size) < n_matrix
        t = after["steps"].astype(np.float64)
        lr = (h["learning_rate"] * np.where(matrix, 1.0, h["non_matrix_learning_rate_factor"])
              * np.sqrt(1 - h["beta2"] ** np.maximum(t, 1)) / (1 - h["beta1"] ** np.maximum(t, 1)))
        eff0 = lr / (np.sqrt(after["m2"].astype(np.float64)) + h["epsilon"])
        lower, upper, _, _ = adabound_bounds(h, float(T))
        st["upper"] = float(np.sum(upd & (eff0 > upper * (1 + 1e-5)))) / n_upd
        st["lower"] = float(np.sum(upd & (eff0 < lower * (1 - 1e-5)))) / n_upd
    return st


def run_oracle(case, n_matrix, T, state, g16, opt=None):
    after = {k: v.copy() for k, v in state.items()}
    oracle_adam_step(AC.optimizer_block(case) if opt is None else opt, n_matrix, AC.loss_scale(case), T, after, g16)
    return after


def assert_case_hits_its_branch(case, n_matrix, T, before, g16, what):
    """The conditions that keep a case from passing vacuously, on one oracle step from `before` with gradients
    g16 (taken at the case's loss scale)."""
    opt = AC.optimizer_block(case)
    after = run_oracle(case, n_matrix, T, before, g16)
    st = branch_stats(opt, n_matrix, T, before, after)
    upd = st["updated"]
    n = upd.size
    matrix = np.arange(n) < n_matrix
    frozen = {"freeze_matrix": matrix, "freeze_nonmatrix": ~matrix}.get(case)
    trainable = ~frozen if frozen is not None else np.ones(n, bool)
    if not trainable.any():  # a frozen matrix class in a model without a non-matrix one: nothing may move
        assert_adam_bits(after, before, (what, case, "nothing to train"))
        return st
    assert upd[trainable & matrix].all() and upd[trainable].any(), (what, case, st["n_updated"])
    if case in ("clip", "combined"):
        assert 0.10 <= st["clip"] <= 0.90, (what, case, st["clip"])
    if case == "adabound_upper":
        assert st["upper"] >= 0.10, (what, case, st["upper"])
    if case == "adabound_lower":
        assert st["lower"] >= 0.10, (what, case, st["lower"])
    if case in AC.NAMED_KEYS:
        neutral = {k: v for k, v in opt.items() if k not in AC.NAMED_KEYS[case]}
        for other, name in ((run_oracle(case, n_matrix, T, before, g16, opt=neutral), "without its keys"),
                            (run_oracle("default", n_matrix, T, before, g16), "default")):
            assert np.array_equal(other["steps"], after["steps"])
            differ = float(np.sum(upd & (bits(other["w32"]) != bits(after["w32"])))) / st["n_updated"]
            assert differ >= 0.90, (what, case, name, differ)
    if frozen is not None:
        assert_adam_bits(after, before, (what, case, "frozen class"), where=frozen)
        assert not upd[frozen].any()
    if case in ("loss_scale_100", "combined"):
        # the division is not a multiplication by the rounded reciprocal: the two differ on a good part of the
        # gradients, so an engine that multiplied would be caught
        gf = O.h2f(g16)
        ls = np.float32(AC.loss_scale(case))
        nz = gf != 0
        assert np.mean((gf / ls)[nz] != (gf * (np.float32(1) / ls))[nz]) >= 0.10, (what, case)
    return st


# ---------------------------------------------------------------------------------------------
# tests
# ---------------------------------------------------------------------------------------------
def test_crafted_state_has_the_edges():
    s = AC.crafted_state()
    n, nm = AC.CRAFT_N, AC.CRAFT_N_MATRIX
    assert s["w32"].size == n and 2000 <= n <= 9999 and nm % 4 != 0 and 0 < nm < n
    gf = O.h2f(s["g16"])
    assert np.isfinite(gf).all()
    for cls in (slice(0, nm), slice(nm, n)):
        g16, w, m1, m2, st = (s[k][cls] for k in ("g16", "w32", "m1", "m2", "steps"))
        for v in (0x0000, AC.F16_NEG_ZERO, AC.F16_MAX, AC.F16_MAX | 0x8000, AC.F16_SUBNORMAL_MIN, AC.F16_NEG_SUBNORMAL_MAX):
            assert (g16 == v).sum() >= 16, hex(v)
        assert (w > 0).any() and (w < 0).any()
        assert ((w == 0) & ~np.signbit(w)).sum() >= 8 and ((w == 0) & np.signbit(w)).sum() >= 8
        assert (m1 != 0).mean() > 0.9 and (m2 > 0).mean() > 0.9
        assert ((st == 0) & (m2 == 0)).any() and ((st == 0) & (m2 != 0)).any()
        assert (st != AC.CRAFT_GLOBAL_STEP).all() and len(np.unique(st)) >= 5


def test_reference_bound_is_tight_enough_to_see_a_wrong_term():
    """The bound stays far below the size of each term of the update (on the combined case: the decay terms, the
    Adam term), so an update with one of them wrong in sign or order is outside it."""
    s, g16 = oracle_state()
    opt = AC.optimizer_block("combined")
    r = adam_float64(opt, AC.CRAFT_N_MATRIX, AC.loss_scale("combined"), AC.CRAFT_GLOBAL_STEP + 1, s["w32"], g16, s["m1"], s["m2"], s["steps"])
    u = r["updated"]
    move = np.abs(r["w_unclipped"] - s["w32"].astype(np.float64))
    assert np.median(r["E_w"][u] / np.maximum(move[u], 1e-300)) < 1e-3
    assert np.mean(r["E_w"][u] < 1e-2 * move[u]) > 0.95


@pytest.mark.parametrize("case", AC.CASE_NAMES)
def test_oracle_adam_matches_float64(case):
    """orc_adam_step against adam_float64 over 3 consecutive steps of the crafted state, each step from the
    oracle's own state before it: masters and both moments within the derived bound of the module docstring per
    element (E_w, E_m1, E_m2); skipped parameters bit-unchanged in every array; step counts, fp16 copies and
    clipped masters exact."""
    opt, ls, nm = AC.optimizer_block(case), AC.loss_scale(case), AC.CRAFT_N_MATRIX
    state, g16_0 = oracle_state()
    clip = float(np.float32(opt.get("clipping_magnitude", 0.0)))
    for k in range(3):
        T = AC.CRAFT_GLOBAL_STEP + 1 + k
        g16 = step_gradients(g16_0, k)
        before = {n: v.copy() for n, v in state.items()}
        oracle_adam_step(opt, nm, ls, T, state, g16)
        r = adam_float64(opt, nm, ls, T, before["w32"], g16, before["m1"], before["m2"], before["steps"])
        upd = r["updated"]
        assert_adam_bits(state, before, (case, k, "skipped"), where=~upd)
        assert np.array_equal(state["steps"], r["steps"]), (case, k)
        assert np.array_equal(state["w16"], O.f2h(state["w32"])), (case, k)
        assert np.isfinite(state["w32"]).all() and np.isfinite(state["m1"]).all() and np.isfinite(state["m2"]).all()
        for name, bound in (("w", "E_w"), ("m1", "E_m1"), ("m2", "E_m2")):
            got = state["w32" if name == "w" else name].astype(np.float64)
            ratio = np.abs(got - r[name]) / np.maximum(r[bound], 1e-300)
            ratio[~upd] = 0.0
            i = int(np.argmax(ratio))
            assert ratio[i] <= 1.0, (case, k, name, i, float(ratio[i]), float(got[i]), float(r[name][i]), float(r[bound][i]))
        if clip != 0.0:
            sure = upd & (np.abs(r["w_unclipped"]) - clip > r["E_w"])
            assert 0.10 <= sure.sum() / upd.sum() <= 0.90, (case, k)
            assert np.array_equal(state["w32"][sure], (np.sign(r["w_unclipped"][sure]) * clip).astype(np.float32)), (case, k)
            at_clip = upd & (np.abs(state["w32"]) == np.float32(clip))
            assert np.all(np.abs(r["w_unclipped"][at_clip]) >= clip - r["E_w"][at_clip]), (case, k)
            assert np.all(np.abs(state["w32"][upd]) <= np.float32(clip)), (case, k)


@pytest.mark.parametrize("case", AC.CASE_NAMES)
@pytest.mark.parametrize("model", ["crafted", "tiled_matrix_only", "tiled_small_grid"])
def test_case_hits_its_branch_on_crafted_state(case, model):
    """Each case exercises what it is named for on the crafted state -- as the CPU test steps it and as the GPU
    test of the standalone kernel tiles it over its two models (their parameter counts, with and without a
    non-matrix class)."""
    if model == "crafted":
        s, g16 = oracle_state()
        nm = AC.CRAFT_N_MATRIX
    else:
        cfg = AC.CFG_SMALL_ONEBLOB if model == "tiled_matrix_only" else AC.CFG_SMALL_GRID
        om = O.OracleModel(cfg, 2, 3, seed=1337)
        s = AC.tiled_state(om.n_params)
        g16 = s.pop("g16")
        s["w16"] = O.f2h(s["w32"])
        nm = om.n_mlp_params
    T0 = AC.CRAFT_GLOBAL_STEP
    for k in range(3):
        g = step_gradients(g16, k)
        assert_case_hits_its_branch(case, nm, T0 + 1 + k, s, g, (model, k))
        oracle_adam_step(AC.optimizer_block(case), nm, AC.loss_scale(case), T0 + 1 + k, s, g)


@pytest.fixture(scope="module")
def trained_gradients():
    """name -> (n_matrix, initial state, {loss scale: fp16 gradient bits of the first training step}) for the
    models the GPU tests train, on the GPU tests' first batch"""
    out = {}
    for name, (cfg, B, cases) in AC.TRAINED.items():
        om = O.OracleModel(cfg, 2, 3, seed=1337)
        pos, tgt = make_batch(B)
        w16 = om.w16.copy()
        grads = {ls: oracle_grad16(cfg, w16, pos, tgt, ls) for ls in sorted({AC.loss_scale(c) for c in cases})}
        if 128.0 in grads:  # the composition of oracle_grad16 is the oracle's own training step
            om.train_step(pos, tgt, run_optimizer=False, n_threads=4)
            assert np.array_equal(grads[128.0], om.grad16), name
        out[name] = (om.n_mlp_params, fresh_adam_state(om.w32), grads)
    return out


@pytest.mark.parametrize("name,case", [(n, c) for n, (_, _, cases) in AC.TRAINED.items() for c in cases])
def test_case_hits_its_branch_on_trained_gradients(trained_gradients, name, case):
    """The same conditions on the first step of every model the GPU tests train (config_hash on the fused
    engine, the 2^16-entry table of the binned pass, the tile and the layer-wise model), from the oracle's
    gradients of the GPU tests' first batch: the GPU cases are known to take their branches before they run."""
    nm, state, grads = trained_gradients[name]
    st = assert_case_hits_its_branch(case, nm, 1, state, grads[AC.loss_scale(case)], name)
    if name == "binned":
        # few enough points that most 4-parameter groups of the table see no gradient (the group-wide skip of
        # the binned pass), and some do
        g = grads[AC.loss_scale(case)][nm:]
        live = (O.h2f(g).reshape(-1, 4) != 0).any(axis=1)
        assert 0.001 < live.mean() < 0.5, live.mean()
