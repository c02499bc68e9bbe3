"""Self-checks of the numpy restatement of the stacked optimizers (tests/optimizer_reference.py), on the CPU."""
import numpy as np

import optimizer_reference as R


def _problem(n=37, seed=5):
    rng = np.random.default_rng(seed)
    w32 = rng.standard_normal(n).astype(np.float32) * 0.3
    grads = [R.f2h((rng.standard_normal(n) * 4.0).astype(np.float32)) for _ in range(9)]
    return w32, grads


def test_exponential_decay_factor_sequence():
    """start 2, interval 3, end 8, base 0.5: the factor halves at nested counts 2, 5 and 8, then stops (11 > end)"""
    s = R.ExponentialDecay(1e-2, decay_base=0.5, decay_interval=3, decay_start=2, decay_end=8)
    got = []
    for step in range(12):
        lr = s.before_step(step)
        got.append(float(s.factor))
        assert lr == np.float32(np.float32(1e-2) * s.factor)
    assert got == [1.0, 1.0, 0.5, 0.5, 0.5, 0.25, 0.25, 0.25, 0.125, 0.125, 0.125, 0.125]
    # set_learning_rate stores value / factor, so the reported rate is the value
    assert s.set_learning_rate(4e-3) == np.float32(np.float32(np.float32(4e-3) / np.float32(0.125)) * np.float32(0.125))
    # the factor resets at step 0
    assert s.before_step(0) == s.base_lr and float(s.factor) == 1.0


def test_ema_of_constant_weights_is_the_constant():
    """the debiased average of a constant is the constant from step 1 on (within the fp32 bound), half and full precision"""
    w32 = np.array([0.75, -1.5, 3.0e-3, 0.0, 12.0], np.float32)  # exact in fp16
    for full in (False, True):
        st = R.Stack({"otype": "Ema", "decay": 0.9, "full_precision": full, "nested": {"otype": "SGD", "learning_rate": 0.0, "l2_reg": 0.0}})
        S = R.fresh_state(w32, st)
        for step in range(1, 8):
            st.step(S, np.zeros(w32.size, np.uint16))
            assert np.array_equal(S["w32"], w32)
            ref = R.h2f(S["w16"])
            got = R.h2f(S["weights_ema"])
            assert np.all(np.abs(got - ref) <= R.fp32_bound(np.abs(ref) * 2, R.N_OPS["ema"]) * step + R.fp16_ulp(ref) * (0 if full else 1)), (full, step)
    old, new = R.ema_debias(0.9, 1)
    assert old == 0.0 and abs(float(new) - 10.0) < 1e-5


def test_batched_multiplier_one_is_the_nested_optimizer():
    w32, grads = _problem()
    nested = {"otype": "SGD", "learning_rate": 0.05, "l2_reg": 1e-4}
    a, b = R.Stack({"otype": "Batched", "batch_size_multiplier": 1, "nested": nested}), R.Stack(nested)
    Sa, Sb = R.fresh_state(w32, a), R.fresh_state(w32, b)
    for k, g in enumerate(grads):
        a.step(Sa, g)
        b.step(Sb, g)
        assert np.array_equal(Sa["averaged_gradients_half"], g)  # g / 1 is exact
        assert np.array_equal(Sa["w32"].view(np.uint32), Sb["w32"].view(np.uint32)), k
        assert a.count() == b.count() == k + 1


def test_batched_steps_every_multiplier_calls():
    w32, grads = _problem()
    st = R.Stack({"otype": "Batched", "batch_size_multiplier": 3, "nested": {"otype": "SGD", "learning_rate": 0.05}})
    S = R.fresh_state(w32, st)
    moved = []
    for g in grads[:7]:
        before = S["w32"].copy()
        checks = st.step(S, g)
        moved.append(not np.array_equal(before, S["w32"]))
        assert ("w32" in checks) == moved[-1]
    assert moved == [False, False, True, False, False, True, False]
    assert st.count() == 7 and st.count(1) == 2  # Batched's own counter; the nested optimizer's


def test_lookahead_alpha_one_keeps_the_nested_trajectory():
    """alpha 1: the blend is look * 0 + w * 1 = w, so the fp32 weights follow the nested optimizer alone"""
    w32, grads = _problem()
    nested = {"otype": "SGD", "learning_rate": 0.05, "l2_reg": 1e-4}
    a, b = R.Stack({"otype": "Lookahead", "alpha": 1.0, "n_steps": 3, "nested": nested}), R.Stack(nested)
    Sa, Sb = R.fresh_state(w32, a), R.fresh_state(w32, b)
    for k, g in enumerate(grads):
        a.step(Sa, g)
        b.step(Sb, g)
        assert np.array_equal(Sa["w32"].view(np.uint32), Sb["w32"].view(np.uint32)), k
    # the slow weights were refreshed at nested counts 0, 3 and 6 only
    assert a.custom_weights() == "weights_lookahead" and b.custom_weights() is None


def test_lookahead_blends_at_step_zero_and_every_n_steps():
    w32, grads = _problem()
    st = R.Stack({"otype": "Lookahead", "alpha": 0.5, "n_steps": 3, "nested": {"otype": "SGD", "learning_rate": 0.05}})
    S = R.fresh_state(w32, st)
    blends = []
    for g in grads[:7]:
        checks = st.step(S, g)
        blends.append("weights_lookahead" in checks and checks["weights_lookahead"][0] == "f16")
    assert blends == [True, False, False, True, False, False, True]


def test_stack_hyperparams_and_learning_rate_rules():
    cfg = {"otype": "Ema", "decay": 0.95, "nested": {"otype": "ExponentialDecay", "decay_start": 2, "decay_interval": 3, "decay_end": 8,
                                                     "decay_base": 0.5, "nested": {"otype": "SGD", "learning_rate": 1e-2}}}
    st = R.Stack(cfg)
    h = st.hyperparams()
    assert h["otype"] == "EMA" and h["full_precision"] is False
    assert h["nested"]["otype"] == "ExponentialDecay" and h["nested"]["nested"] == {"otype": "SGD", "learning_rate": 1e-2, "l2_reg": 1e-8}
    S = R.fresh_state(np.ones(4, np.float32), st)
    rates = []
    for _ in range(4):
        st.step(S, np.zeros(4, np.uint16))
        rates.append(st.learning_rate())
    assert rates == [float(np.float32(1e-2))] * 2 + [float(np.float32(np.float32(1e-2) * np.float32(0.5)))] * 2
    st.set_learning_rate(1e-3)
    assert st.learning_rate() == float(np.float32(np.float32(np.float32(1e-3) / np.float32(0.5)) * np.float32(0.5)))


def test_absolute_mode_values_dominate():
    """A >= |value| for every update, with equality when no term cancels"""
    w32, grads = _problem()
    for val, A in (R.sgd_update(w32, grads[0], 128.0, 0.05, 1e-4), R.ema_update(w32, grads[1], 0.9, 0.5, 2.0),
                   R.lookahead_blend(grads[2], w32, 0.25), R.batched_pool(w32, grads[3], 3, False)):
        assert np.all(A >= np.abs(val) * (1 - 1e-15))
    val, A = R.batched_pool(w32, grads[3], 3, True)
    assert np.array_equal(np.abs(val), A)
