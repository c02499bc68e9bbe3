"""A numpy restatement of the reference's nine losses (src/loss.cu:57-65), element by element as its
kernels compute them (include/tiny-cuda-nn/losses/*.h, the lines between `const float prediction`
and `gradients[i] =`): fp32 operations in the reference's order, the fp16 gradient rounded once from
the fp32 result (oracle.f2h), padded columns zero.

Three expressions of the form a*b + c are contracted by the reference's compiler; the engine writes
them as explicit FMAs (csrc/loss_device.h) and this file emulates fmaf(a, b, c) as
float32(float64(a) * float64(b) + float64(c)): the product of two fp32 values is exact in fp64, so the
only difference from a true FMA is the double rounding of the sum (fp64, then fp32), which changes the
result in about 2^-29 of the cases.

  L2                   l2.h:66-74                       d*d / pdf / n ;        2 d / pdf
  RelativeL2           relative_l2.h:66-75              d*d / (p*p + 0.01) / pdf / n ; 2 d / (p*p + 0.01) / pdf
  RelativeL2Luminance  relative_l2_luminance.h:66-86    as RelativeL2 with the sample's luminance for p
  L1                   l1.h:66-74                       |d| / pdf / n ;        copysign(1 / pdf, d)
  RelativeL1           relative_l1.h:66-76              scale = 1 / (|p| + 0.01) / pdf ; |d| scale / n ; copysign(scale, d)
  Mape                 mape.h:66-77                     scale = 1 / (|t| + 0.01) / pdf
  Smape                smape.h:66-77                    scale = 1 / (0.5 (|t| + |p|) + 0.01) / pdf
  CrossEntropy         cross_entropy.h:66-76            factor = -t / pdf / n ; factor log p ; factor / p
  Variance             variance_is.h:66-76              factor = t*t / pdf / n ; factor / p - factor / pdf ; -factor / (p*p)
(d = p - t, n = n_total = batch * dims; gradients are loss_scale * gradient / n, except CrossEntropy
and Variance whose factor already holds 1 / n.)
"""
import numpy as np

from oracle import oracle as O

LOSSES = ("L2", "RelativeL2", "RelativeL2Luminance", "L1", "RelativeL1", "Mape", "Smape", "CrossEntropy", "Variance")
# the losses whose arithmetic holds an FMA (emulated here, see above); the other six are plain fp32
FMA_LOSSES = ("RelativeL2", "RelativeL2Luminance", "Smape")

f32 = np.float32


def canonical(otype):
    """the reference's spelling of a loss otype given in any letter case"""
    return {n.lower(): n for n in LOSSES}[otype.lower()]


def fmaf(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(f32)


def luminance(pred, dims):
    """relative_l2_luminance.h:68-77 on fp32 predictions [n, stride] (stride >= 6, padded columns included):
    the association of the three-term sum is the engine's choice, fmaf(0.114, b, fmaf(0.587, g, 0.299 r))"""
    pred = np.asarray(pred, f32)
    r, g, b = pred[:, 0], pred[:, 1], pred[:, 2]
    if dims >= 6:
        r, g, b = r + pred[:, 3], g + pred[:, 4], b + pred[:, 5]
    return fmaf(f32(0.114), b, fmaf(f32(0.587), g, f32(0.299) * r))


def normaliser(otype, p, t, lum):
    """the quantity the reference's gradient treats as a constant (fp32): p*p + 0.01, |p| + 0.01, ...; None if none"""
    otype = canonical(otype)
    c = f32(0.01)
    if otype == "RelativeL2":
        return fmaf(p, p, c)
    if otype == "RelativeL2Luminance":
        return fmaf(lum, lum, c)
    if otype == "RelativeL1":
        return np.abs(p) + c
    if otype == "Mape":
        return np.abs(t) + c
    if otype == "Smape":
        return fmaf(f32(0.5), np.abs(t) + np.abs(p), c)
    return None


def evaluate(otype, pred16, target, loss_scale=128.0, pdf=None):
    """pred16: uint16 fp16 bits [n, stride]; target, pdf: float32 [n, dims]. Returns (values float32 [n, stride],
    gradients uint16 [n, stride]); columns >= dims are zero."""
    otype = canonical(otype)
    pred16 = np.ascontiguousarray(pred16, np.uint16)
    n, stride = pred16.shape
    t = np.ascontiguousarray(target, f32)
    dims = t.shape[1]
    assert t.shape[0] == n and dims <= stride
    pred = O.h2f(pred16)
    p = pred[:, :dims]
    # a division by an absent pdf (1) is exact, so one code path serves both
    q = np.ones((n, dims), f32) if pdf is None else np.ascontiguousarray(pdf, f32)
    nt = f32(n * dims)
    ls = f32(loss_scale)
    d = p - t
    with np.errstate(all="ignore"):
        if otype in ("L2", "RelativeL2", "RelativeL2Luminance"):
            lum = luminance(pred, dims)[:, None] if otype == "RelativeL2Luminance" else None
            pse = f32(1.0) if otype == "L2" else normaliser(otype, p, t, lum)
            v = d * d / pse / q / nt
            g = ls * (f32(2.0) * d / pse / q) / nt
        elif otype == "L1":
            v = np.abs(d) / q / nt
            g = ls * np.copysign(f32(1.0) / q, d) / nt
        elif otype in ("RelativeL1", "Mape", "Smape"):
            scale = f32(1.0) / normaliser(otype, p, t, None) / q
            v = np.abs(d) * scale / nt
            g = ls * np.copysign(scale, d) / nt  # d == 0: +scale
        elif otype == "CrossEntropy":
            factor = -t / q / nt
            v = factor * np.log(p)
            g = ls * (factor / p)
        else:
            factor = t * t / q / nt
            v = factor / p - factor / q
            g = ls * (-factor / (p * p))
    assert v.dtype == f32 and g.dtype == f32
    values = np.zeros((n, stride), f32)
    grads = np.zeros((n, stride), np.uint16)
    values[:, :dims] = v
    grads[:, :dims] = O.f2h(np.ascontiguousarray(g))
    return values, grads


def value_f64(otype, p, t, pdf, n_total, norm):
    """The loss value of one element in float64 as a function of the prediction p, with the normaliser held at norm
    (what the reference's gradient differentiates)."""
    otype = canonical(otype)
    p, t, pdf = (np.asarray(x, np.float64) for x in (p, t, pdf))
    d = p - t
    if otype == "L2":
        return d * d / pdf / n_total
    if otype in ("RelativeL2", "RelativeL2Luminance"):
        return d * d / norm / pdf / n_total
    if otype == "L1":
        return np.abs(d) / pdf / n_total
    if otype in ("RelativeL1", "Mape", "Smape"):
        return np.abs(d) / norm / pdf / n_total
    if otype == "CrossEntropy":
        return -t / pdf / n_total * np.log(p)
    f = t * t / pdf / n_total
    return f / p - f / pdf


def ulp_diff16(a, b):
    """distance in fp16 ulps between two arrays of fp16 bits (finite values)"""
    def key(x):
        x = np.asarray(x, np.uint16).astype(np.int32)
        return np.where(x & 0x8000, -(x & 0x7FFF), x & 0x7FFF)
    return np.abs(key(a) - key(b))


def ulp_diff32(a, b):
    """distance in fp32 ulps between two float32 arrays (finite values)"""
    def key(x):
        x = np.ascontiguousarray(x, f32).view(np.uint32).astype(np.int64)
        return np.where(x & 0x80000000, -(x & 0x7FFFFFFF), x & 0x7FFFFFFF)
    return np.abs(key(a) - key(b))
