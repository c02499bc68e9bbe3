"""CPU pins of tests/mlp_reference.py, the float64 restatement the Module matrix
(tests/test_gpu_module_matrix.py) compares the HIP engines with:

  * exact mode (no fp16 rounding) against central finite differences of sum(y * dout), for every hidden x
    output activation pair: the analytic backward-from-the-forward-value is the derivative of the forward;
  * every case of the GPU matrix through the fp32 CPU oracle (O.mlp_fwd / O.mlp_bwd, activation =
    hidden | output << 8), checked against the float64 reference with the assertions the GPU gets: the
    proof that the chosen inputs leave headroom, that every branchy case finds its B samples among 16 B
    candidates, and that the oracle -- a second restatement, fp32 sums in another order -- stays inside
    every bound. The oracle's worst ratios are the yardstick the GPU's are written next to
    (profiles/module_matrix_ratios.txt; TCNN_MATRIX_RATIOS=<file> makes this module append its own).
"""
import json
import os

import numpy as np
import pytest

import mlp_reference as R
import module_matrix_cases as C
from helpers import rel_err

PAIRS = [(a, o) for a in R.ACTIVATIONS for o in R.ACTIVATIONS]


@pytest.mark.parametrize("act,out_act", PAIRS, ids=[f"{a}-{o}" for a, o in PAIRS])
def test_exact_mode_matches_finite_differences(act, out_act):
    """W16, IN16, NH2, B = 8, every parameter and every input element, central differences with h = 1e-6 of
    L = sum(y * dout) in float64.

    Bound. The central difference (L(t + h) - L(t - h)) / 2h differs from dL/dt by
      * truncation h^2 |L'''| / 6. Each differentiation of an activation brings a factor of at most K_ACT = 10
        (Squareplus / Softplus are functions of 10 z), so |L'''| <= K_ACT^3 times the first-derivative scale:
        h^2 K_ACT^3 gmax = 1e-9 gmax, gmax = max |analytic gradient|;
      * cancellation: L is a sum of terms of total magnitude S = sum |y * dout|, each evaluation carries a
        relative error of a few 2^-53 per operation along a path of ~64 operations (two 16-term dot
        products per layer, three layers, the activations): 64 * 2^-53 * S per evaluation, two evaluations,
        divided by 2h: 64 * 2^-53 * S / h = 7e-9 S.
    The branchy activations are piecewise linear: the bound holds as long as no pre-activation changes
    sign inside +-h, which the test asserts (|z| > 1e-4 >> h * sum |dz/dt|)."""
    W, IN, NH, OUTP, B, h = 16, 16, 2, 16, 8, 1e-6
    def clear_of_branches(mats, x):
        a = x
        for k in range(NH + 1):
            z = a @ mats[k].T
            if (act if k < NH else out_act).lower() in C.BRANCHY and np.abs(z).min() <= 1e-4:
                return False
            a = R.act_forward(act, z)
        return True

    for attempt in range(64):  # the first draw with no pre-activation within reach of the step
        rng = np.random.default_rng(1000 * attempt + R.ACTIVATIONS.index(act) * 16 + R.ACTIVATIONS.index(out_act))
        mats = [rng.uniform(-0.25, 0.25, s) for s in ((W, IN), (W, W), (OUTP, W))]
        x, dout = rng.uniform(-1, 1, (B, IN)), rng.uniform(-1, 1, (B, OUTP))
        if clear_of_branches(mats, x):
            break
    assert clear_of_branches(mats, x)

    def run(ms, xs, backward=False):
        return R.mlp_reference(W, IN, NH, OUTP, act, out_act, None, None, None, exact=True, mats=ms, x=xs, dout=dout, backward=backward)

    ref = run(mats, x, backward=True)
    loss = lambda r: float((r["out"] * dout).sum())  # noqa: E731
    S = float(np.abs(ref["out"] * dout).sum())
    analytic = [ref["wgrad"][k] for k in range(NH + 1)] + [ref["dinput"]]
    gmax = max(float(np.abs(g).max()) for g in analytic)
    tol = h * h * R.K_ACT ** 3 * gmax + 64 * 2.0 ** -53 * S / h
    worst = 0.0
    for t, target in enumerate(mats + [x]):
        fd = np.empty_like(target)
        for idx in np.ndindex(*target.shape):
            keep = target[idx]
            vals = []
            for sgn in (1.0, -1.0):
                target[idx] = keep + sgn * h
                vals.append(loss(run(mats, x)))
            target[idx] = keep
            fd[idx] = (vals[0] - vals[1]) / (2 * h)
        err = float(np.abs(fd - analytic[t]).max())
        worst = max(worst, err)
        assert err <= tol, (t, err, tol, gmax, S)
    assert gmax > 1e-3  # a vanishing gradient would make the comparison vacuous


def test_sine_is_refused():
    with pytest.raises(ValueError):
        R.mlp_reference(16, 16, 1, 16, "Sine", "None", np.zeros(512, np.uint16), np.zeros((8, 16), np.uint16), np.zeros((8, 16), np.uint16))
    with pytest.raises(ValueError):
        R.act_factor("Sine", np.zeros(1))


def test_rounding_mode_is_single_rne():
    """f64_to_f16 rounds once: a value just above an fp16 tie, which a float32 stop would round to the tie
    and then to even, goes up"""
    tie = 1.0 + 2.0 ** -11  # halfway between the fp16 values 1 and 1 + 2^-10
    assert R.f64_to_f16(np.array([tie + 2.0 ** -40]))[0] == 1.0 + 2.0 ** -10
    assert R.f64_to_f16(np.array([tie]))[0] == 1.0
    assert R.f64_to_f16(np.array([tie - 2.0 ** -40]))[0] == 1.0


@pytest.mark.parametrize("case", C.ALL_CPU_CASES, ids=[c.id for c in C.ALL_CPU_CASES])
def test_scales_keep_outputs_in_range(case):
    """SCALES against the rule it was chosen by (module_matrix_cases.choose_scale): on the 256- or 300-sample
    first draw the last hidden pre-activation's standard deviation is <= 1 and every output pre-activation is
    inside +-4, so Exponential, Sigmoid and Tanh outputs stay out of saturation. The uneven cases reuse a
    constant chosen at B = 256 on B = 256 (n_cu + 1) samples, and one case's unfiltered batch is a second
    draw (AGG_SEEDS): the maximum of n roughly normal values grows like sqrt(2 ln n), over the 16 output
    columns sqrt(ln(16 * 65792) / ln(16 * 256)) = 1.29, so those stay inside +-4 * 1.29 = +-5.2 (all have
    output activation None; exp(5.2) = 181 would still be far inside the fp16 range)."""
    sd, mx = C.preactivation_stats(case, C.scale_params16(case, C.host_params32(case)))
    first_draw = case.B <= 300 and case.id not in C.AGG_SEEDS
    assert first_draw or case.out_act == "None"
    assert mx <= (4.0 if first_draw else 5.2), (mx, sd)
    assert case.NH == 0 or sd <= 1.0, (mx, sd)
    assert mx >= 1.0  # no vanishing output either


def _context_reuse_cfgs():
    from helpers import CONFIG_HASH
    grid = CONFIG_HASH["encoding"]
    relu = lambda w, nh: {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None",  # noqa: E731
                          "n_neurons": w, "n_hidden_layers": nh}
    return {"config_hash": CONFIG_HASH, "configs3_hashgrid_w128_h4": {"encoding": grid, "network": relu(128, 4)},
            "oneblob64_w64_h2": {"encoding": {"otype": "OneBlob", "n_bins": 64}, "network": relu(64, 2)}}


@pytest.mark.parametrize("name", ["config_hash", "configs3_hashgrid_w128_h4", "oneblob64_w64_h2"])
def test_oracle_within_context_reuse_bounds(name):
    """the inputs of test_gpu_tile_engine.py::test_module_forward_context_reused_by_backward (seed-42
    initialisation unscaled: a +-1e-4 grid table, gradients down in the fp16 subnormals) through the fp32
    oracle, its gradient rounded to fp16 as the Module's is: B ReLU-clear samples exist among 16 B, and the
    per-element, per-matrix bound of check_wgrad (which carries the fp16 rounding per element) holds."""
    from oracle import oracle as O
    cfg = _context_reuse_cfgs()[name]
    net = cfg["network"]
    W, NH = net["n_neurons"], net["n_hidden_layers"]
    IN, nm, g = C.encoded_dims(cfg)
    p16 = O.f2h(C.init_params32(W, IN, NH, 16, cfg["encoding"] if g is not None else None))
    _, enc, dout = C.context_reuse_inputs(cfg, p16)
    ref = R.mlp_reference(W, IN, NH, 16, "ReLU", "None", p16[:nm], enc, dout)
    out16, hidden = O.mlp_fwd(W, IN, NH, 16, p16[:nm], enc, input_soa=False, n_threads=8)
    wg, _ = O.mlp_bwd(W, IN, NH, 16, p16[:nm], enc, hidden, dout, input_soa=False, n_threads=8)
    R.check_output(O.h2f(out16)[:, :3], ref["out"][:, :3])
    R.check_wgrad(O.h2f(O.f2h(wg)), ref, fp16_out=True)


def _dump(case, kind, ratios):
    path = os.environ.get("TCNN_MATRIX_RATIOS")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"case": case.id, "B": case.B, "side": "oracle", "kind": kind, "ratios": ratios}) + "\n")


def _dump_graph(case, name, want_dx, ratios):
    path = os.environ.get("TCNN_MATRIX_RATIOS")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"case": C.graph_id(name, want_dx), "B": "+".join(map(str, C.GRAPH_TWICE_B)), "side": "oracle",
                                "kind": "graph-twice", "ratios": ratios}) + "\n")


@pytest.mark.parametrize("case", C.ALL_CPU_CASES, ids=[c.id for c in C.ALL_CPU_CASES])
def test_oracle_within_every_bound(case):
    """the fp32 oracle against the float64 reference, the GPU's assertions; branchy cases: per element on
    the filtered batch (draw asserts that B of 16 B candidates survive), aggregate on the unfiltered one"""
    p16 = C.scale_params16(case, C.host_params32(case))
    per_element = not (case.uneven and case.branchy)  # the uneven ReLU runs are aggregate-only
    if per_element:
        _, enc, dout = C.draw(case, p16, filtered=case.branchy)
        ref = C.reference(case, p16, enc, dout)
        out, wg, denc = C.oracle_run(case, p16, enc, dout, n_threads=8)
        assert np.abs(ref["out"][:, :case.n_out]).max() > 2.0 ** -6  # no vacuous output check
        _dump(case, "per_element", C.check_against_reference(case, ref, out, wg, denc, True, fp16_out=False))
    if case.branchy:
        _, enc, dout = C.draw(case, p16, filtered=False)
        ref = C.reference(case, p16, enc, dout)
        out, wg, denc = C.oracle_run(case, p16, enc, dout, n_threads=8)
        _dump(case, "aggregate", C.check_against_reference(case, ref, out, wg, denc, False, fp16_out=False))


@pytest.mark.parametrize("name,want_dx", C.GRAPH_TWICE, ids=[f"{n}-{'dx' if d else 'nodx'}" for n, d in C.GRAPH_TWICE])
def test_oracle_sum_of_two_calls_within_bound(name, want_dx):
    """The CPU proof of tests/test_gpu_torch_graphs.py's twice-in-one-graph bound: one module called at B = 256
    (draw seed 0) and B = 300 (seed 1), the fp32 oracle per call on 128 dL/dy, its gradient rounded to fp16 and
    divided by 128 in fp16 as the binding returns it, the two summed in fp32 as torch accumulates them. The sum
    passes mlp_reference.check_wgrad_sum against the float64 references (per element and aggregate; the ReLU
    network on unfiltered draws aggregate only), and each call passes the single-call checks."""
    from oracle import oracle as O
    s, total, refs, ratios = 128.0, None, [], {}
    for seed, B in enumerate(C.GRAPH_TWICE_B):
        case = C.graph_case(name, B)
        p16 = C.scale_params16(case, C.host_params32(case))
        _, enc, dout = C.draw(case, p16, filtered=False, seed=seed)
        ref = C.torch_reference(case, p16, enc, dout, s)
        dout_s = dout.copy()
        dout_s[:, :case.n_out] = O.f2h(O.h2f(dout[:, :case.n_out]) * np.float32(s))
        out, wg, denc = C.oracle_run(case, p16, enc, dout_s, n_threads=8)
        g16 = O.h2f(O.f2h(O.h2f(O.f2h(wg.astype(np.float32))) / np.float32(s)))  # fp16(fp16(g) / s)
        total = g16 if total is None else total + g16  # float32 + float32
        R.check_output(out[:, :case.n_out], ref["out"][:, :case.n_out])
        if case.branchy:
            ratios[f"agg_in{seed + 1}"] = rel_err(denc / s, ref["dinput"])
            assert ratios[f"agg_in{seed + 1}"] <= R.aggregate_bar(case.W, case.NH, case.out_act)
        else:
            ratios[f"dinput{seed + 1}"] = R.check_dinput(denc / s, ref["dinput"], ref["mag_in"])
        refs.append(ref)
    assert total.dtype == np.float32
    ratios.update(R.check_wgrad_sum(total, refs, R.aggregate_bar(case.W, case.NH, case.out_act), per_element=not case.branchy))
    _dump_graph(case, name, want_dx, ratios)
