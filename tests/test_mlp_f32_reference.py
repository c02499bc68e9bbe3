"""CPU proof of the fp32 network bounds (tests/mlp_f32_reference.py): they are neither unreachable nor vacuous.

A numpy float32 evaluation of every case of the GPU table (fp32 products and sums, the weight gradient in the
kernels' 256-row slabs, numpy's float32 exp / tanh / log) passes every bound; the worst ratio it reaches over all
cases and both batch sizes is 0.21 (an output of the single matrix h0-None-None, B = 256; dL/dinput 0.13 on the
same case; weight gradients 0.021, W1 of w48h2-LeakyReLU-None): a rigorous worst-case bound is approached most
closely where it is shortest, one chain of 64 terms, and stays far from the deep cases, whose errors would all have
to line up through every |M|. The same evaluation fails with one gradient element moved by 2^-12 of its magnitude, and with
one hidden activation rounded to fp16, on every case up to NH W = 144 (see PROBES)."""
import numpy as np
import pytest

import mlp_f32_reference as F
import mlp_reference as R
import test_grid_f32_reference as G
from oracle import oracle as O

WORST = {}


def cpu_rows(case, x):
    """the encoded rows on the CPU (inputs of the network; the GPU test takes the fp32 encoding module's own)"""
    if case.enc is None:
        return F.identity_rows(case, x), None
    if case.enc["otype"] == "OneBlob":
        rows = np.ones((x.shape[0], case.IN), np.float32)  # OneBlob pads with ones
        v = O.h2f(O.oneblob_fwd(x, case.enc["n_bins"])).astype(np.float32)
        rows[:, :v.shape[1]] = v
        return rows, None
    g = O.grid_cfg(case.enc, case.n_in)
    table = np.random.default_rng(7).uniform(-1, 1, g.n_params).astype(np.float32)
    rows = np.zeros((x.shape[0], case.IN), np.float32)
    rows[:, :g.n_levels * g.n_features_per_level] = G.grid_forward(g, x, table)[0].astype(np.float32)
    return rows, table


def setup(case, B):
    x, dout = F.case_inputs(case, B)
    rows, table = cpu_rows(case, x)
    assert rows.shape[1] == case.IN
    p = F.case_params(case, table)
    _, rows = F.keep_clear(case, p, x, rows, B)
    net = p[:case.n_mlp]
    ref = F.reference(case.W, case.IN, case.NH, case.OUTP, case.act, case.out_act, net, rows, dout)
    return net, rows, dout, ref


@pytest.mark.parametrize("B", F.BATCHES)
@pytest.mark.parametrize("case", F.CASES, ids=[c.id for c in F.CASES])
def test_float32_evaluation_is_within_the_bounds(case, B):
    net, rows, dout, ref = setup(case, B)
    out, _, wg, din = F.eval_f32(case.W, case.IN, case.NH, case.OUTP, case.act, case.out_act, net, rows, dout)
    ratios = F.check(ref, out, wg, din, case.NH, case.id)
    WORST[(case.id, B)] = max(ratios.values())
    print(case.id, B, ratios)
    # the forward magnitudes dominate the values they bound where the activation fixes 0 (|act(z)| <= L |z|)
    if case.act.lower() in ("none", "relu", "leakyrelu", "tanh") and case.NH:
        assert np.all(np.abs(ref["hidden"][0]) <= ref["mag_fwd"][1] * (1 + 1e-12))


# The probes run where a 2^-12 defect stands above a rigorous worst-case bound: errors propagate through |M|, which
# grows by about sqrt(K) per layer relative to the values themselves, so on the deepest and widest cases (NH W > 144:
# w64h3o17, w128h2) the bound passes 2^-12 of the magnitude and such a probe cannot show. Those cases are held by
# the same formulas; the 16 / 32 / 48 / 144-wide cases and the single matrix show that the formulas bite.
PROBES = [c for c in F.CASES if c.out_act == "None" and c.NH * c.W <= 144]


@pytest.mark.parametrize("case", PROBES, ids=[c.id for c in PROBES])
def test_a_moved_gradient_element_fails(case):
    """one element of the output matrix's gradient moved by 2^-12 of its magnitude (mag_w: sum |delta| |a|). The
    output matrix, because its bound carries the forward error only: the first matrix's also carries every
    layer's transfer error (L_phi up to 10 per smooth layer) and reaches 2^-12 of the magnitude on the three-layer
    Softplus / Squareplus / Tanh cases."""
    net, rows, dout, ref = setup(case, 256)
    out, _, wg, din = F.eval_f32(case.W, case.IN, case.NH, case.OUTP, case.act, case.out_act, net, rows, dout)
    wg = wg.copy()
    off = wg.size - ref["mag_w"][-1].size
    j = int(np.argmax(ref["mag_w"][-1]))
    wg[off + j] += np.float32(2.0 ** -12 * ref["mag_w"][-1].flat[j])
    with pytest.raises(AssertionError):
        F.check(ref, out, wg, din, case.NH, case.id)


HIDDEN_PROBES = [c for c in PROBES if c.NH > 0]


@pytest.mark.parametrize("case", HIDDEN_PROBES, ids=[c.id for c in HIDDEN_PROBES])
def test_a_hidden_activation_rounded_to_fp16_fails(case):
    """the last hidden activation stored as fp16 (what the fp16 engine does, and what an fp32 engine must not):
    every case fails. One single ELEMENT rounded (the one with the largest rounding error) is caught on the
    one-tile case, W 16 -- a K-term bound grows with K while one element's 2^-12 does not, so at W >= 48 one
    element in 256 rows hides inside it."""
    net, rows, dout, ref = setup(case, 256)

    def to_fp16(hidden):
        h = hidden[-1]
        r = h.astype(np.float16).astype(np.float32)
        if case.W == 16:
            j = int(np.argmax(np.abs(r - h)))
            h.flat[j] = r.flat[j]
        else:
            h[...] = r

    out, _, wg, din = F.eval_f32(case.W, case.IN, case.NH, case.OUTP, case.act, case.out_act, net, rows, dout, perturb_hidden=to_fp16)
    with pytest.raises(AssertionError):
        F.check(ref, out, wg, din, case.NH, case.id)


def test_case_table_matches_the_issue():
    ids = {c.name for c in F.CASES}
    assert ids == {"w16h1", "w48h2", "w64h3o17", "w128h2", "w144h1", "h0", "oneblob-w32h2", "grid-w32h2"}
    for a in R.ACTIVATIONS:
        for n in ("w48h2", "w64h3o17"):
            assert any(c.name == n and c.act == a for c in F.CASES)
            assert a == "None" or any(c.name == n and c.out_act == a for c in F.CASES)
