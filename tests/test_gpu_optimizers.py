"""SGD and the Ema / ExponentialDecay / Lookahead / Batched optimizers on the three training engines.

After every training_step the engine's state (parameters and fp16 gradients through helpers.trainer_arrays, the
optimizer's state through Trainer.optimizer_state(stacked=True)) is compared with tests/optimizer_reference.py
applied to the engine's OWN previous state and its own fp16 gradients, one step at a time (no drift):

  * fp32 values (w32, tmp, the pool): |got - ref64| <= (n_ops + 2) 2^-24 A + 2^-149, A the absolute-mode value,
    n_ops the reference expression's rounded operations (SGD 5, EMA 6, Lookahead 4, pool 2);
  * fp16 values with an fp32 witness (w16 of w32, weights_ema of tmp, the half pool of the pool): bit-equal to
    f16_rn(witness);
  * half-precision EMA and the Lookahead slow weights (no witness): the fp32 bound plus one fp16 ulp of |ref|;
  * Adam under ExponentialDecay / Ema / Batched: bit-equal to oracle.adam_step with the scheduled learning rate.
  * Adam after a Lookahead blend (the blended w32 is not observable between the two): Adam is configured with
    l2_reg = relative_decay = absolute_decay = 0, so it is w' = rn(w + c) with c independent of w and the blend's
    bound passes through unchanged, plus 3 x 2^-24 |w'| (the driver's fp32 rounding of the blend, and the two
    roundings of w'); m1, m2 and the step counts stay bit-exact. A frozen Adam (optimize_*_params false) shows
    the blend alone, with the 4-operation bound and its bit-exact witnesses.

Models (batches of 256 or 512 points, at most 12 steps):
  A   fused register engine: config_hash.json with log2_hashmap_size 10. Its 16 levels stay: the register engine
      takes a 32-wide encoding only, at 4 levels (8 features, padded to 16) the model trains on the tile engine.
      37504 parameters = 18.3 workgroup spans of the optimizer kernels (2048 parameters): not a multiple.
  A4  the same with n_levels 4: a grid encoding on the tile engine.
  B   tile engine: OneBlob n_bins 4 on 2 inputs, FullyFusedMLP 16 wide, one hidden layer: 512 parameters, fewer
      than one span (a short grid whose last workgroup is mostly idle).
  C   layer-wise engine: A's encoding with CutlassMLP, 48 wide.
Every parameter count of a trainable model is a multiple of 16 (MLP matrices, grid levels aligned to 8 entries),
so the kernels' one-at-a-time tail is not reachable through a Trainer; tests/cpp/optimizer_api_consumer.cpp runs
the kernels on counts that are no multiple of 8."""
import copy
import json

import numpy as np
import pytest

import optimizer_reference as R
from helpers import CONFIG_HASH, bits, make_batch, oracle_adam_step, trainer_arrays

pytestmark = pytest.mark.gpu

LOSS_SCALE = 128.0


def _model(name):
    c = copy.deepcopy(CONFIG_HASH)
    c["encoding"]["log2_hashmap_size"] = 10
    if name == "A4":
        c["encoding"]["n_levels"] = 4
    elif name == "B":
        c["encoding"] = {"otype": "OneBlob", "n_bins": 4}
        c["network"] = {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": 16, "n_hidden_layers": 1}
    elif name == "C":
        c["network"] = {"otype": "CutlassMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": 48, "n_hidden_layers": 2}
    return c


ENGINE = {"A": "fused", "A4": "fused", "B": "fused", "C": "layered"}
N_PARAMS = {"A": 37504, "B": 512}
ADAM = {"otype": "Adam", "learning_rate": 1e-2, "beta1": 0.9, "beta2": 0.99, "epsilon": 1e-15, "l2_reg": 1e-6}
ADAM_PLAIN_W = dict(ADAM, l2_reg=0.0)  # under Lookahead: w' = rn(w + c)
NGP = {"otype": "Ema", "decay": 0.95, "nested": {"otype": "ExponentialDecay", "decay_start": 2, "decay_interval": 3, "decay_end": 8,
                                                 "decay_base": 0.5, "nested": ADAM}}


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


_batches = {}


def batch(torch, B, step):
    if (B, step) not in _batches:
        pos, tgt = make_batch(B, step=step)
        _batches[(B, step)] = (torch.from_numpy(pos).cuda(), torch.from_numpy(tgt).cuda())
    return _batches[(B, step)]


def make_trainer(model, opt, seed=1337):
    from tinycudann import Trainer
    cfg = _model(model)
    cfg["optimizer"] = opt
    t = Trainer(2, 3, cfg, seed=seed)
    assert t.engine == ENGINE[model], (model, t.engine)
    if model in N_PARAMS:
        assert t.n_params == N_PARAMS[model], t.n_params
    return t


def engine_state(t, stack):
    """every array the restatement tracks, from the engine (fp16 as uint16 bits)"""
    a = trainer_arrays(t)
    S = {"w32": a["w32"], "w16": a["w16"], "g16": a["g16"], "g32": a["g32"]}
    st = t.optimizer_state(stacked=True)
    names = {"first_moments": "m1", "second_moments": "m2", "param_steps": "steps"}
    has_adam = stack is None or stack.levels[-1]["kind"] == "adam"
    for k, v in st.items():
        if k in names and not has_adam:
            continue
        h = v.cpu().numpy()
        if h.dtype == np.float16:
            h = h.view(np.uint16)
        if h.dtype == np.int32:
            h = h.view(np.uint32)
        S[names.get(k, k)] = h
    return S


def make_stack(t, opt):
    def adam_fn(block, global_step, S, g16):
        oracle_adam_step(block, t.n_network_params, LOSS_SCALE, global_step, S, g16)
    return R.Stack(opt, adam_fn)


def tracked(S):
    return {k: v for k, v in S.items() if k not in ("g16", "g32")}


def assert_same_bits(got, ref, what):
    assert sorted(got) == sorted(ref), (what, sorted(got), sorted(ref))
    for k in ref:
        bad = np.flatnonzero(bits(got[k]) != bits(ref[k]))
        assert bad.size == 0, (what, k, int(bad.size), int(bad[0]))


def run_steps(torch, t, stack, n_steps, B, first_batch=0, after_step=None, do_step=None):
    """n_steps training steps, each compared with the restatement applied to the engine's previous state;
    returns the engine's last state"""
    prev = engine_state(t, stack)
    for s in range(n_steps):
        x, y = batch(torch, B, first_batch + s)
        (do_step or t.training_step)(x, y)
        got = engine_state(t, stack)
        S = {k: v.copy() for k, v in tracked(prev).items()}
        checks = stack.step(S, got["g16"], LOSS_SCALE, observed=got)
        what = ("step", s)
        R.assert_checks(got, checks, what)
        for k in tracked(prev):  # whatever the step does not write stays as it was
            if k not in checks:
                assert np.array_equal(bits(got[k]), bits(prev[k])), (what, k, "changed")
        assert np.float32(t.learning_rate()) == np.float32(stack.learning_rate()), (what, t.learning_rate(), stack.learning_rate())
        assert t.optimizer_step_count == stack.count(), (what, t.optimizer_step_count, stack.count())
        assert np.isfinite(t.loss())
        if after_step:
            after_step(s, prev, got, checks)
        prev = got
    return prev


def assert_fresh(t, stack):
    S = engine_state(t, stack)
    assert_same_bits(tracked(S), R.fresh_state(S["w32"], stack), "initial state")
    cw = stack.custom_weights()
    pi = t.params_inference().cpu().numpy().view(np.uint16)
    assert np.array_equal(pi, S[cw or "w16"])
    return S


# ---- 1: SGD ----
@pytest.mark.parametrize("model", ["A", "A4", "B", "C"])
def test_sgd(torch_mod, model):
    opt = {"otype": "sgd", "learning_rate": 0.05, "l2_reg": 1e-4}  # otypes compare case-insensitively
    t = make_trainer(model, opt)
    stack = make_stack(t, opt)
    first = assert_fresh(t, stack)
    assert t.params_inference().data_ptr() == t.params().data_ptr()  # no custom weights
    last = run_steps(torch_mod, t, stack, 6, 256)
    moved = np.mean(last["w32"] != first["w32"])
    assert moved > 0.9, moved  # every parameter, the grid's zero-gradient ones included (l2_reg)


# ---- 2: the instant-ngp stack ----
@pytest.mark.parametrize("full_precision", [False, True])
@pytest.mark.parametrize("model", ["A", "B", "C"])
def test_ema_exponential_decay_adam(torch_mod, model, full_precision):
    """12 steps: the factor halves at nested counts 2, 5 and 8 and then stops. inference() reads weights_ema:
    a plain-Adam trainer given (float)weights_ema through set_params_full_precision holds exactly those fp16
    parameters (fp16 -> fp32 -> fp16 is exact), so the two inferences must agree bit for bit (bound 0)."""
    from tinycudann import Trainer
    torch = torch_mod
    opt = copy.deepcopy(NGP)
    opt["full_precision"] = full_precision
    t = make_trainer(model, opt)
    stack = make_stack(t, opt)
    assert_fresh(t, stack)
    rates = []
    last = run_steps(torch, t, stack, 12, 512, after_step=lambda s, p, g, c: rates.append(t.learning_rate()))
    lr = np.float32(1e-2)
    f = [1, 1, .5, .5, .5, .25, .25, .25, .125, .125, .125, .125]
    assert rates == [float(np.float32(lr * np.float32(k))) for k in f], rates
    assert ("tmp" in last) == full_precision
    ema = t.params_inference().cpu().numpy().view(np.uint16)
    assert np.array_equal(ema, last["weights_ema"]) and not np.array_equal(ema, last["w16"])
    plain_cfg = _model(model)
    plain = Trainer(2, 3, plain_cfg, seed=7)
    plain.set_params_full_precision(R.h2f(ema).astype(np.float32))
    assert np.array_equal(trainer_arrays(plain)["w16"], ema)
    x, _ = batch(torch, 512, 40)
    assert torch.equal(t.inference(x), plain.inference(x))
    # a second inference after another step: the training weight image is not handed to it
    xb, yb = batch(torch, 512, 12)
    t.training_step(xb, yb)
    plain.set_params_full_precision(R.h2f(t.params_inference().cpu().numpy().view(np.uint16)).astype(np.float32))
    assert torch.equal(t.inference(x), plain.inference(x))


# ---- 3: the wrapper keeps Adam's schedule ----
def test_exponential_decay_keeps_the_fast_path(torch_mod):
    """ExponentialDecay{Adam} whose decay starts beyond the run: parameters, Adam state, both gradient buffers
    and every loss bit-identical to plain Adam's over 8 steps, on the same engine and with Adam's own schedule
    (tcnn_trainer_optimizer_schedule: "inline", against "staged" for a stack that acts between the gradients and
    the update)."""
    torch = torch_mod
    a = make_trainer("A", ADAM)
    b = make_trainer("A", {"otype": "ExponentialDecay", "decay_start": 1000, "nested": ADAM})
    assert (a.optimizer_schedule, b.optimizer_schedule) == ("adam", "inline") and a.engine == b.engine
    assert make_trainer("A", NGP).optimizer_schedule == "inline"
    for staged in ({"otype": "SGD"}, {"otype": "Lookahead", "nested": ADAM}, {"otype": "Ema", "nested": {"otype": "Batched", "nested": ADAM}}):
        assert make_trainer("B", staged).optimizer_schedule == "staged"
    for s in range(8):
        x, y = batch(torch, 512, s)
        a.training_step(x, y)
        b.training_step(x, y)
        assert a.loss() == b.loss()
    sa, sb = engine_state(a, None), engine_state(b, None)
    assert_same_bits(sb, sa, "ExponentialDecay{Adam} vs Adam")
    assert b.learning_rate() == a.learning_rate() and b.optimizer_step_count == 8


# ---- 4: Lookahead ----
@pytest.mark.parametrize("model", ["A", "B"])
def test_lookahead_adam(torch_mod, model):
    """n_steps 3, alpha 0.5, 7 steps: blends at nested counts 0, 3 and 6. The step after a blend must train on
    the blended weights (the fused engine's cached weight image is invalidated): its loss equals the loss of a
    fresh plain trainer loaded with the parameters the blend step left."""
    from tinycudann import Trainer
    torch = torch_mod
    opt = {"otype": "Lookahead", "n_steps": 3, "alpha": 0.5, "nested": ADAM_PLAIN_W}
    t = make_trainer(model, opt)
    stack = make_stack(t, opt)
    assert_fresh(t, stack)
    blends = []

    def after(s, prev, got, checks):
        blends.append(checks.get("weights_lookahead", ("",))[0] == "f16")
        assert np.array_equal(t.params_inference().cpu().numpy().view(np.uint16), got["weights_lookahead"])
        if blends[-1]:
            fresh = Trainer(2, 3, _model(model), seed=3)
            fresh.set_params_full_precision(got["w32"])
            assert np.array_equal(trainer_arrays(fresh)["w16"], got["w16"])
            x, y = batch(torch, 256, s + 1)
            fresh.training_step(x, y, run_optimizer=False)
            after.expect = fresh.loss()
        elif after.expect is not None:
            assert t.loss() == after.expect, (s, t.loss(), after.expect)
            after.expect = None

    after.expect = None
    run_steps(torch, t, stack, 7, 256, after_step=after)
    assert blends == [True, False, False, True, False, False, True]


def test_lookahead_blend_alone(torch_mod):
    """A frozen Adam below Lookahead: the step is the blend alone, so w32 is checked with the 4-operation bound
    and weights_lookahead = w16 = f16_rn(w32) bit for bit (step 0 blends the fp16 copy with the fp32 masters)."""
    opt = {"otype": "Lookahead", "n_steps": 2, "alpha": 0.25,
           "nested": dict(ADAM_PLAIN_W, optimize_matrix_params=False, optimize_non_matrix_params=False)}
    t = make_trainer("B", opt)
    stack = make_stack(t, opt)
    w = np.linspace(-1.0, 1.0, t.n_params).astype(np.float32) * np.float32(1.0 + 2.0 ** -12)  # fp32 masters off the fp16 grid
    t.set_params_full_precision(w)
    first = assert_fresh(t, stack)

    def after(s, prev, got, checks):
        assert np.array_equal(got["weights_lookahead"], got["w16"]) and np.array_equal(got["w16"], R.f2h(got["w32"]))
        assert checks["w32"][3] == R.N_OPS["lookahead"] and checks["w32"][0] == "f32"

    last = run_steps(torch_mod, t, stack, 1, 256, after_step=after)
    assert not np.array_equal(last["w32"], first["w32"])  # look = f16(w) != w: the blend moved the masters


# ---- 5: Batched ----
@pytest.mark.parametrize("opt", [
    {"otype": "Batched", "batch_size_multiplier": 3, "nested": {"otype": "SGD", "learning_rate": 0.05}},
    {"otype": "Ema", "decay": 0.9, "nested": {"otype": "Batched", "batch_size_multiplier": 3, "nested": ADAM}},
], ids=["Batched{SGD}", "Ema{Batched{Adam}}"])
def test_batched(torch_mod, opt):
    t = make_trainer("B", opt)
    stack = make_stack(t, opt)
    assert_fresh(t, stack)
    moved = []
    run_steps(torch_mod, t, stack, 7, 256, after_step=lambda s, p, g, c: moved.append(not np.array_equal(p["w32"], g["w32"])))
    assert moved == [False, False, True, False, False, True, False]
    # Optimizer::step() of the outermost level is Batched's own counter (Ema reports its nested level's)
    assert t.optimizer_step_count == 7 and stack.count(len(stack.levels) - 1) == 2


# ---- 6: snapshots ----
def _serialize_json(t, optimizer):
    import ctypes
    from tinycudann import _lib as L
    n = ctypes.c_uint64(0)
    L.check(L.lib().tcnn_trainer_serialize_json(t.h, int(optimizer), None, 0, ctypes.byref(n)))
    buf = ctypes.create_string_buffer(n.value)
    L.check(L.lib().tcnn_trainer_serialize_json(t.h, int(optimizer), buf, n.value, ctypes.byref(n)))
    return json.loads(buf.value.decode())


def _bin(j, dtype):
    return np.array(j["bytes"], np.uint8).view(dtype)


@pytest.mark.parametrize("full_precision", [False, True])
def test_snapshot_round_trip(torch_mod, full_precision):
    """Key layout of the reference's nested serialize(), params_binary = the EMA weights, and a round trip.
    Trainer::deserialize sets BOTH parameter sets from params_binary (trainer.h:295-304) and, with full precision,
    restarts tmp from the fp16 average (ema.h:200-203), so the loaded trainer does not continue the saved
    trainer's trajectory; what must hold is that the loaded state is exactly what those rules give, that two
    trainers loading the same bytes continue bit-identically, and that each of their 3 next steps matches the
    restatement applied to the loaded state."""
    torch = torch_mod
    opt = copy.deepcopy(NGP)
    opt["full_precision"] = full_precision
    t = make_trainer("B", opt)
    stack = make_stack(t, opt)
    last = run_steps(torch, t, stack, 4, 256)
    snap = _serialize_json(t, True)
    assert sorted(snap) == ["n_params", "optimizer", "params_binary", "params_type"]
    o = snap["optimizer"]
    assert sorted(o) == ["nested", "weights_ema_binary"]
    assert sorted(o["nested"]) == ["learning_rate", "learning_rate_factor", "nested"]
    assert sorted(o["nested"]["nested"]) == ["base_learning_rate", "current_step", "first_moments_binary", "param_steps_binary",
                                              "second_moments_binary"]
    assert o["nested"]["learning_rate"] == float(np.float32(1e-2)) and o["nested"]["learning_rate_factor"] == 0.5
    assert o["nested"]["nested"]["current_step"] == 4
    assert o["nested"]["nested"]["base_learning_rate"] == float(np.float32(np.float32(1e-2) * np.float32(0.5)))
    assert np.array_equal(_bin(o["weights_ema_binary"], np.uint16), last["weights_ema"])
    assert np.array_equal(_bin(snap["params_binary"], np.uint16), last["weights_ema"])
    assert np.array_equal(_bin(_serialize_json(t, False)["params_binary"], np.uint16), last["weights_ema"])
    assert "optimizer" not in _serialize_json(t, False)

    blob = t.serialize(optimizer=True)
    loaded = [make_trainer("B", opt, seed=s) for s in (11, 12)]
    stacks = []
    for u in loaded:
        u.deserialize(blob)
        S = engine_state(u, stack)
        ema = last["weights_ema"]
        expect = {"w16": ema, "w32": R.h2f(ema).astype(np.float32), "weights_ema": ema, "m1": last["m1"], "m2": last["m2"],
                  "steps": last["steps"]}
        if full_precision:
            expect["tmp"] = R.h2f(ema).astype(np.float32)
        assert_same_bits(tracked(S), expect, "loaded state")
        assert u.optimizer_step_count == 4 and u.learning_rate() == t.learning_rate()
        st = make_stack(u, opt)  # the restatement's host state as the snapshot holds it
        st.levels[2]["step"] = 4
        st.levels[1]["sched"].factor = np.float32(0.5)
        st._set_lr(2, st.levels[1]["sched"].learning_rate())
        stacks.append(st)
        assert u.serialize(optimizer=True) == blob  # a fixed point of the round trip
    ends = [run_steps(torch, u, st, 3, 256, first_batch=4) for u, st in zip(loaded, stacks)]
    assert_same_bits(tracked(ends[0]), tracked(ends[1]), "two loaded trainers")
    assert loaded[0].learning_rate() == float(np.float32(np.float32(1e-2) * np.float32(0.25)))  # the factor halved again at count 5


def test_plain_adam_snapshot_keeps_its_layout(torch_mod):
    """beside a stacked trainer's nested layout, plain Adam's snapshot keeps its five keys and its parameters"""
    x, y = batch(torch_mod, 256, 0)
    s = make_trainer("B", {"otype": "Lookahead", "nested": {"otype": "Batched", "nested": {"otype": "SGD"}}})
    s.training_step(x, y)
    o = _serialize_json(s, True)["optimizer"]
    assert sorted(o) == ["nested", "weights_lookahead_binary"]
    assert sorted(o["nested"]) == ["averaged_gradients_binary", "averaged_gradients_half_binary", "current_step", "nested"]
    assert sorted(o["nested"]["nested"]) == ["current_step", "learning_rate"]
    assert o["nested"]["current_step"] == 1 and o["nested"]["nested"]["current_step"] == 0
    u = make_trainer("B", {"otype": "Lookahead", "nested": {"otype": "Batched", "nested": {"otype": "SGD"}}}, seed=5)
    u.deserialize(s.serialize(optimizer=True))
    assert u.serialize(optimizer=True) == s.serialize(optimizer=True) and u.optimizer_step_count == 1
    t = make_trainer("B", ADAM)
    t.training_step(x, y)
    snap = _serialize_json(t, True)
    assert sorted(snap["optimizer"]) == ["base_learning_rate", "current_step", "first_moments_binary", "param_steps_binary",
                                         "second_moments_binary"]
    assert np.array_equal(_bin(snap["params_binary"], np.uint16), trainer_arrays(t)["w16"])
    assert t.optimizer_buffers() == {} and t.params_inference().data_ptr() == t.params().data_ptr()


# ---- 7: hyper-parameters ----
def _approx_tree(got, ref, path="optimizer"):
    assert sorted(got) == sorted(ref), (path, sorted(got), sorted(ref))
    for k, v in ref.items():
        if isinstance(v, dict):
            _approx_tree(got[k], v, path + "." + k)
        elif isinstance(v, float):
            assert got[k] == pytest.approx(v, rel=1e-6), (path, k, got[k], v)
        else:
            assert got[k] == v, (path, k, got[k], v)


def test_update_hyperparams(torch_mod):
    torch = torch_mod
    opt = copy.deepcopy(NGP)
    t = make_trainer("B", opt)
    stack = make_stack(t, opt)
    h = t.hyperparams()["optimizer"]
    ref = stack.hyperparams()
    ref["nested"]["nested"] = h["nested"]["nested"]  # Adam's own echo (its existing tests cover it)
    _approx_tree(h, ref)
    assert h["otype"] == "EMA" and h["nested"]["nested"]["otype"] == "Adam"
    assert h["nested"]["nested"]["learning_rate"] == pytest.approx(1e-2, rel=1e-6)
    # each level takes its own keys and passes "nested" down
    t.update_hyperparams({"optimizer": {"decay": 0.5, "nested": {"decay_base": 0.25, "nested": {"learning_rate": 3e-3, "beta1": 0.8}}}})
    h = t.hyperparams()["optimizer"]
    assert h["decay"] == 0.5 and h["nested"]["decay_base"] == 0.25
    assert h["nested"]["nested"]["learning_rate"] == pytest.approx(3e-3, rel=1e-6) and h["nested"]["nested"]["beta1"] == pytest.approx(0.8)
    # the reference's rule: ExponentialDecay keeps its own base rate and hands base x factor to the nested
    # optimizer before every step (exponential_decay.h:69), so a rate written past it lasts until that step
    assert t.learning_rate() == float(np.float32(1e-2))
    stack.levels[0]["p"]["decay"] = 0.5
    stack.levels[1]["sched"].decay_base = np.float32(0.25)
    stack.levels[2]["p"]["beta1"] = 0.8
    run_steps(torch, t, stack, 3, 256)
    assert t.hyperparams()["optimizer"]["nested"]["nested"]["learning_rate"] == pytest.approx(2.5e-3, rel=1e-6)
    # set_learning_rate through the wrapper stores value / factor
    t.set_learning_rate(4e-3)
    stack.set_learning_rate(4e-3)
    assert np.float32(t.learning_rate()) == np.float32(stack.learning_rate())
    run_steps(torch, t, stack, 2, 256, first_batch=3)
    with pytest.raises(Exception, match="full_precision"):
        t.update_hyperparams({"optimizer": {"full_precision": True}})
    with pytest.raises(Exception, match="n_steps"):
        make_trainer("B", {"otype": "Lookahead", "n_steps": 0, "nested": ADAM})


# ---- 8: refusals and fallbacks ----
@pytest.mark.parametrize("otype, message", [
    ("Average", "Optimizer 'Average' is not implemented by the MI355X engine"),
    ("Novograd", "Optimizer 'Novograd' is not implemented by the MI355X engine"),
    ("Composite", "Optimizer 'Composite' is not implemented by the MI355X engine"),
    ("Shampoo", "Cannot create `ShampooOptimizer` because tiny-cuda-nn was not compiled with cuBLAS and cuSolver."),
    ("Nope", "Invalid optimizer type: Nope"),
])
def test_refused_otypes(torch_mod, otype, message):
    from tinycudann import _lib as L
    supported = "Adam, SGD, ExponentialDecay, Ema, Lookahead, Batched"
    for opt in ({"otype": otype}, {"otype": "Ema", "nested": {"otype": otype}}):
        with pytest.raises(L.TcnnError) as e:
            make_trainer("B", opt)
        assert message in str(e.value) and supported in str(e.value), str(e.value)
    t = make_trainer("B", {"otype": "SGD"})  # the library still works
    x, y = batch(torch_mod, 256, 0)
    t.training_step(x, y)
    assert np.isfinite(t.loss())


def test_graph_replay_steps_eagerly(torch_mod):
    torch = torch_mod
    a, b = make_trainer("A", NGP), make_trainer("A", NGP)
    b.set_graph(True)
    x, y = batch(torch, 512, 0)
    for _ in range(5):  # one batch buffer: a plain-Adam trainer would capture and replay
        a.training_step(x, y)
        b.training_step(x, y)
    assert b.graph_stats() == (0, 0)
    stack = make_stack(a, NGP)
    assert_same_bits(tracked(engine_state(b, stack)), tracked(engine_state(a, stack)), "graph on vs off")


def test_data_parallel_is_refused(torch_mod):
    import ctypes
    from tinycudann import _lib as L

    class Comm:  # a one-rank RCCL communicator, straight from the C-ABI (no process group)
        def __init__(self):
            uid = (ctypes.c_uint8 * 128)()
            L.check(L.lib().tcnn_dp_unique_id(uid))
            self.h = L.check_ptr(L.lib().tcnn_dp_comm_create(uid, 1, 0))

        def __del__(self):
            L.lib().tcnn_dp_comm_destroy(self.h)

    comm = Comm()
    t = make_trainer("A", NGP)
    with pytest.raises(L.TcnnError, match="needs a plain Adam optimizer"):
        t.set_dp(comm)
    with pytest.raises(L.TcnnError, match="optimizer_step_range.*plain Adam"):
        t.optimizer_step_range(0, 16)
    blob = (__import__("ctypes").c_uint8 * L.lib().tcnn_dp_peer_blob_bytes())()
    assert L.lib().tcnn_trainer_dp_peer_export(t.h, 1, 0, blob) != 0
    assert "plain Adam" in L.lib().tcnn_last_error().decode()
    x, y = batch(torch_mod, 512, 0)
    t.training_step(x, y)  # still trains
    plain = make_trainer("A", ADAM)
    plain.set_dp(comm)  # plain Adam still attaches
    plain.set_dp(None)


def test_training_halves_step_the_tree(torch_mod):
    """forward / backward / optimizer_step and training_step(run_optimizer=False) + optimizer_step run the same tree"""
    torch = torch_mod
    a, b, c = (make_trainer("B", NGP) for _ in range(3))
    for s in range(3):
        x, y = batch(torch, 256, s)
        a.training_step(x, y)
        b.training_step(x, y, run_optimizer=False)
        b.optimizer_step()
    stack = make_stack(a, NGP)
    assert_same_bits(tracked(engine_state(b, stack)), tracked(engine_state(a, stack)), "training_step(False) + optimizer_step")

    def halves(x, y):
        ctx = c.forward(x, y)
        c.backward(ctx, x)
        c.optimizer_step()

    run_steps(torch, c, make_stack(c, NGP), 3, 256, do_step=halves)
