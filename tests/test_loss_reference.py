"""CPU tests of tests/loss_reference.py, the numpy restatement of the reference's nine losses that the
GPU loss tests compare against (no GPU and no HIP library needed):

  * its RelativeL2 and L2 rows equal the C oracle's (oracle.relative_l2 / oracle.l2) bit for bit,
    gradients and values -- the one place where an independent implementation has an opinion
  * for every loss the gradient is the derivative of the value with respect to the prediction, the
    normaliser (p*p + 0.01, |p| + 0.01, the luminance, the Smape denominator) held fixed as the
    reference's gradients hold it: a central finite difference in float64
  * the details the formulas are easy to get wrong on: copysign at a zero difference, the sign of
    CrossEntropy / Variance, Variance's second division by the pdf, the luminance's columns
"""
import numpy as np
import pytest

import loss_reference as R
from oracle import oracle as O

N, STRIDE = 4096, 16


def _inputs(dims, seed=3):
    rng = np.random.default_rng(seed)
    pred = np.zeros((N, STRIDE), np.float32)
    pred[:, :max(dims, 6)] = rng.uniform(0.2, 2.0, size=(N, max(dims, 6)))  # the luminance reads 6 columns
    pred16 = O.f2h(pred)
    tgt = rng.uniform(0.05, 1.0, size=(N, dims)).astype(np.float32)
    pdf = rng.uniform(0.25, 4.0, size=(N, dims)).astype(np.float32)
    return pred16, tgt, pdf


@pytest.mark.parametrize("otype,fn", [("RelativeL2", O.relative_l2), ("L2", O.l2)])
def test_rows_equal_the_oracle_bit_for_bit(otype, fn):
    pred16, tgt, _ = _inputs(3)
    _, g_ref, v_ref = fn(pred16, tgt, loss_scale=128.0, want_values=True)
    v, g = R.evaluate(otype, pred16, tgt, 128.0)
    np.testing.assert_array_equal(g[:, :3], g_ref[:, :3])
    np.testing.assert_array_equal(v[:, :3].view(np.uint32), v_ref[:, :3].view(np.uint32))
    assert not g[:, 3:].any() and not v[:, 3:].any()


@pytest.mark.parametrize("with_pdf", [False, True])
@pytest.mark.parametrize("dims", [3, 6])
@pytest.mark.parametrize("otype", R.LOSSES)
def test_gradient_is_the_finite_difference_of_the_value(otype, dims, with_pdf):
    pred16, tgt, pdf = _inputs(dims)
    ls = 128.0
    v, g16 = R.evaluate(otype, pred16, tgt, ls, pdf if with_pdf else None)
    pred = O.h2f(pred16)
    p = pred[:, :dims].astype(np.float64)
    lum = R.luminance(pred, dims)[:, None]
    norm = R.normaliser(otype, pred[:, :dims], tgt, lum)
    norm = None if norm is None else np.asarray(norm, np.float64)
    q = pdf.astype(np.float64) if with_pdf else np.ones_like(p)
    nt = float(N * dims)
    h = 1e-4
    keep = np.abs(p - tgt) > 10 * h  # |d| is not differentiable at 0
    fd = (R.value_f64(otype, p + h, tgt, q, nt, norm) - R.value_f64(otype, p - h, tgt, q, nt, norm)) / (2 * h)
    got = O.h2f(g16)[:, :dims].astype(np.float64) / ls
    # the gradient is an fp32 result rounded to fp16 (2^-11 relative; 2^-25 absolute below the normal range, scaled);
    # the difference quotient's truncation error is h^2 f''' / 6 <= 1e-7 relative for p >= 0.2
    tol = 2.0 ** -10 * np.abs(fd) + 2.0 ** -24 / ls
    assert keep.mean() > 0.95
    assert np.all(np.abs(got - fd)[keep] <= tol[keep]), float(np.max((np.abs(got - fd) / tol)[keep]))
    # the value itself against float64: at most 7 fp32 operations, each within 2^-24 relative (log within 2^-23),
    # of the terms' magnitude -- Variance's value is a difference of two terms that can cancel
    ref = R.value_f64(otype, p, tgt, q, nt, norm)
    mag = np.abs(ref)
    if otype == "Variance":
        f = tgt.astype(np.float64) ** 2 / q / nt
        mag = np.abs(f / p) + np.abs(f / q)
    assert np.all(np.abs(v[:, :dims] - ref) <= 1e-6 * mag)


def test_sign_losses_at_zero_difference_give_plus_scale():
    pred16 = O.f2h(np.full((4, STRIDE), 0.5, np.float32))
    tgt = np.full((4, 3), 0.5, np.float32)
    for otype in ("L1", "RelativeL1", "Mape", "Smape"):
        v, g = R.evaluate(otype, pred16, tgt, 128.0)
        assert not v.any()
        assert np.all(O.h2f(g)[:, :3] > 0), otype  # copysignf(scale, +0) = +scale, not 0


def test_cross_entropy_and_variance_signs_and_pdf():
    pred16 = O.f2h(np.full((2, STRIDE), 2.0, np.float32))
    tgt = np.full((2, 1), 0.5, np.float32)
    v, g = R.evaluate("CrossEntropy", pred16, tgt, 1.0)
    assert np.all(v[:, 0] < 0) and np.all(O.h2f(g)[:, 0] < 0)  # p > 1: -t log p < 0
    np.testing.assert_allclose(v[:, 0], -0.5 * np.log(2.0) / 2, rtol=1e-6)
    # Variance: factor / p - factor / pdf with factor = t*t / pdf / n  (two divisions by the pdf)
    pdf = np.full((2, 1), 4.0, np.float32)
    v, g = R.evaluate("Variance", pred16, tgt, 1.0, pdf)
    f = 0.25 / 4.0 / 2
    np.testing.assert_allclose(v[:, 0], f / 2.0 - f / 4.0, rtol=1e-6)
    np.testing.assert_allclose(O.h2f(g)[:, 0], -f / 4.0, rtol=2.0 ** -10)
    v1, _ = R.evaluate("Variance", O.f2h(np.full((2, STRIDE), 0.25, np.float32)), tgt, 1.0, np.full((2, 1), 0.125, np.float32))
    assert np.all(v1[:, 0] < 0)  # p > pdf


def test_luminance_columns():
    pred = np.zeros((1, STRIDE), np.float32)
    pred[0, :6] = [1.0, 2.0, 4.0, 8.0, 16.0, 32.0]
    assert R.luminance(pred, 3)[0] == pytest.approx(0.299 * 1 + 0.587 * 2 + 0.114 * 4, rel=1e-6)
    assert R.luminance(pred, 4)[0] == R.luminance(pred, 3)[0]
    assert R.luminance(pred, 6)[0] == pytest.approx(0.299 * 9 + 0.587 * 18 + 0.114 * 36, rel=1e-6)
    # every output of the sample, a fourth included, is normalised by the one luminance
    pred16 = O.f2h(pred)
    tgt = np.zeros((1, 4), np.float32)
    v, _ = R.evaluate("RelativeL2Luminance", pred16, tgt, 1.0)
    lum = float(R.luminance(pred, 4)[0])
    np.testing.assert_allclose(v[0, :4], np.array([1.0, 4.0, 16.0, 64.0]) / (lum * lum + 0.01) / 4, rtol=1e-6)


def test_any_letter_case_and_unknown_otype():
    assert R.canonical("crossentropy") == "CrossEntropy" and R.canonical("SMAPE") == "Smape"
    with pytest.raises(KeyError):
        R.canonical("Huber")
