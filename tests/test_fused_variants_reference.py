"""The CPU side of tests/test_gpu_fused_variants.py, on the oracle alone: the inputs of every case are sound, and each
kind of mistake the fused gather could make (another hash, another interpolation, permuted axes, another grid type)
moves the oracle's step by more than 10 x the tolerances the GPU file asserts -- 1e-3 relative on the loss and on
the gradient vectors, 4 fp16 ulps of the output scale on the outputs -- so those assertions can fail.
Cases and inputs: tests/fused_variant_cases.py."""
import itertools

import numpy as np
import pytest

import fused_variant_cases as C
from helpers import rel_err
from oracle import oracle as O

GRAD_BAR = 1e-2  # 10 x the GPU file's rel_err bar
OUT_SHARE = 0.5  # more than half of the outputs further apart than 40 ulps (10 x assert_within_fp16_ulps' 4)
IDS = [c.id for c in C.ALL_CASES]


def _assert_visible(d, what):
    loss_rel, mlp_rel, grid_rel, out_share = d
    print(f"{what}: loss {loss_rel:.3g} network gradient {mlp_rel:.3g} grid gradient {grid_rel:.3g} outputs beyond 40 ulps {out_share:.3g}")
    assert mlp_rel > GRAD_BAR, (what, mlp_rel)
    assert grid_rel > GRAD_BAR, (what, grid_rel)
    assert out_share > OUT_SHARE, (what, out_share)


@pytest.mark.parametrize("case_id", IDS)
def test_inputs_are_sound(case_id):
    case = C.BY_ID[case_id]
    w = C.cpu_params(case_id)
    w16 = O.f2h(w)
    assert np.abs(w[case.n_mlp:]).max() > 0.9  # the table is O(1)
    (pos_all, _), (pos, tgt), n_safe = C.batches(case, w)  # asserts the pool yields B safe samples
    n_pool = C.pool_factor(case) * C.B
    print(f"{case_id}: {n_safe} of {n_pool} candidates safe ({n_safe / n_pool:.0%})")
    assert pos.shape == (C.B, case.D) and pos_all.shape == (C.B, case.D) and pos.dtype == np.float32
    assert pos.min() >= 0 and pos.max() < 1 and tgt.min() >= 0.1 and tgt.max() <= 1
    enc = O.grid_fwd(C.grid(case), pos, w16[case.n_mlp:])
    out16, hidden = O.mlp_fwd(case.W, 32, case.NH, 16, w16[:case.n_mlp], enc, activation=O.act_code(case.act))
    pred = O.h2f(out16)[:, :C.N_OUT]
    print(f"{case_id}: predictions {pred.min():.3g} .. {pred.max():.3g}")
    assert np.abs(pred).max() > 0.5  # O(1): the loss sees the table
    if case.act == "ReLU":
        # |output matrix| behind a ReLU: positive by construction (a linear network's predictions have both signs)
        assert pred.min() > 0, float(pred.min())
        for k in range(case.NH):  # a wrong ReLU mask is visible: neither nearly all nor nearly none of the units pass
            active = float((O.h2f(hidden[k]) > 0).mean())
            assert 0.05 <= active <= 0.95, (k, active)
    # the sample's loss gradient is not negligible anywhere it is checked per element
    assert np.abs(pred - tgt).max() > 0.1


def test_case_matrix_is_the_one_the_kernels_are_instantiated_for():
    grids = {(c.D, c.enc.get("hash", "CoherentPrime"), c.enc.get("type", "Hash"), c.enc.get("interpolation", "Linear")) for c in C.GRID_CASES}
    for D in (2, 3):
        for h in C.HASHES:
            assert (D, h, "Hash", "Linear") in grids
        for t in ("Tiled", "Dense"):
            assert (D, "CoherentPrime", t, "Linear") in grids
        for i in C.INTERPS:
            assert (D, "CoherentPrime", "Hash", i) in grids
    assert all((c.W, c.NH, c.act, c.loss) == (64, 2, "ReLU", "RelativeL2") for c in C.GRID_CASES)
    assert {(c.W, c.NH, c.act) for c in C.SHAPE_CASES} == {(W, NH, a) for W, NH in C.FUSED_SHAPES for a in ("None", "ReLU")}
    assert all(c.D == 3 and c.enc == C.ENC for c in C.SHAPE_CASES + [C.L2_CASE])
    # every (D, hash, hidden activation) the launchers instantiate at W64/H2: in a training step and in inference
    for cases in (C.ALL_CASES, C.INFERENCE_CASES):
        seen = {(c.D, c.enc.get("hash", "CoherentPrime"), c.act) for c in cases if (c.W, c.NH) == (64, 2)}
        assert seen == {(D, h, a) for D in (2, 3) for h in C.HASHES for a in ("None", "ReLU")}, seen
    assert C.B == 256  # training_step's granularity: more than one workgroup, no smaller batch exists
    assert C.B_INFER % 32 == 0 and C.B_INFER % 128 != 0
    for D in (2, 3):  # the table mixes dense and hashed levels
        g = C.grid(C.BY_ID[f"d{D}-default"])
        dense = [g.offsets[l + 1] - g.offsets[l] < 1 << 12 for l in range(16)]
        assert any(dense) and not all(dense), (D, dense)


@pytest.mark.parametrize("D", [2, 3])
def test_wrong_hash_is_visible(D):
    case = C.BY_ID[f"d{D}-default"]
    w = C.cpu_params(case.id)
    (pos, tgt), _, _ = C.batches(case, w)
    for a, b in itertools.combinations(C.HASHES, 2):
        ca, cb = case.with_enc(hash=a), case.with_enc(hash=b)
        assert C.grid(ca).n_params == C.grid(cb).n_params  # the same table
        _assert_visible(C.step_difference(ca, cb, w, pos, pos, tgt), (D, a, b))
        _assert_visible(C.step_difference(cb, ca, w, pos, pos, tgt), (D, b, a))


@pytest.mark.parametrize("D", [2, 3])
def test_wrong_interpolation_is_visible(D):
    case = C.BY_ID[f"d{D}-default"]
    w = C.cpu_params(case.id)
    (pos, tgt), _, _ = C.batches(case, w)
    for a, b in itertools.permutations(C.INTERPS, 2):
        _assert_visible(C.step_difference(case.with_enc(interpolation=a), case.with_enc(interpolation=b), w, pos, pos, tgt), (D, a, b))


@pytest.mark.parametrize("case_id", [c.id for c in C.GRID_CASES])
def test_wrong_axis_order_is_visible(case_id):
    """the bug a D = 3 index loop would have: every permutation of the position columns, on every grid option"""
    case = C.BY_ID[case_id]
    w = C.cpu_params(case_id)
    (pos, tgt), _, _ = C.batches(case, w)
    for p in C.position_permutations(case.D):
        _assert_visible(C.step_difference(case, case, w, pos, np.ascontiguousarray(pos[:, p]), tgt), (case_id, p))


@pytest.mark.parametrize("D", [2, 3])
def test_wrong_grid_type_is_caught_by_construction(D):
    """Hash, Tiled and Dense tables have different sizes: a wrong hash_grid flag reads another table layout"""
    n = {t: C.grid(C.BY_ID[f"d{D}-default"].with_enc(type=t)).n_params for t in ("Hash", "Tiled")}
    n["Dense"] = C.grid(C.BY_ID[f"d{D}-dense"]).n_params
    n["Dense at the hash scale"] = C.grid(C.BY_ID[f"d{D}-default"].with_enc(type="Dense")).n_params
    print(D, n)
    assert len(set(n.values())) == 4, n
    assert n["Hash"] == C.grid(C.BY_ID[f"d{D}-default"]).n_params and n["Tiled"] == C.grid(C.BY_ID[f"d{D}-tiled"]).n_params
    if D == 3:
        assert n["Dense"] < 250000 < 30000000 < n["Dense at the hash scale"]  # why the Dense case has its own scale


@pytest.mark.parametrize("D", [2, 3])
def test_loss_sees_the_hash_only_with_an_order_one_table(D):
    """why the tests scale the table: at the seed-1337 initialisation (table +-1e-4) Prime instead of CoherentPrime
    moves the loss by less than the 1e-3 the GPU file allows; at the test parameters by much more"""
    case = C.BY_ID[f"d{D}-default"]
    wrong = case.with_enc(hash="Prime")
    w = C.cpu_params(case.id)
    (pos, tgt), _, _ = C.batches(case, w)
    om = C.oracle_model(case)
    w_init = np.array(om.w32)
    d_init = C.step_difference(case, wrong, w_init, pos, pos, tgt)
    d_test = C.step_difference(case, wrong, w, pos, pos, tgt)
    print(f"D={D}: relative loss difference {d_init[0]:.3g} at the initialisation, {d_test[0]:.3g} at the test parameters")
    assert d_init[0] < 1e-3 < 1e-2 < d_test[0], (d_init, d_test)
    assert d_init[1] > GRAD_BAR  # only the gradients see it there


def test_mixed_range_batches_are_what_they_claim():
    for cid in C.MIXED_RANGE_CASES:
        case = C.BY_ID[cid]
        pos, tgt = C.mixed_range_batch(case)
        assert pos.shape == (C.B, case.D)
        assert (pos[32:64] == 1.0).sum() == 1 and (pos[32:64] == 0.0).sum() == 1
        out = ~np.all((pos >= 0) & (pos <= 1), axis=1)
        assert out.sum() == 3 and out[64:96].sum() == 3
        assert pos[out].min() >= -0.5 and pos[out].max() <= 1.5
        # the out-of-range positions matter to the step: without them the gradients differ by more than the bar
        w = C.cpu_params(cid)
        inside = pos.copy()
        inside[out] = np.clip(inside[out], 0.0, 1.0)
        _, ga = C.oracle_step(case, w, pos, tgt)
        _, gb = C.oracle_step(case, w, inside, tgt)
        assert rel_err(gb[case.n_mlp:], ga[case.n_mlp:]) > GRAD_BAR, cid
