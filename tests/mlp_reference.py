"""A float64 restatement of the fully connected network, every activation: forward, backward from an
external dL/dy, and the abs-backprop magnitudes that size the per-element bounds. Plain numpy.

Semantics are the reference's: include/tiny-cuda-nn/common_device.h:102-297 for the activations and
for their backward from the STORED FORWARD VALUE (warp_activation_backward), fully_fused_mlp.cu for the
places where a value is stored as fp16. Sums are float64; values are rounded to fp16 (one rounding,
nearest even) exactly where the reference stores fp16:

  * every hidden activation and the output (after its activation);
  * the output-activation transfer g * (T)factor(y): the factor as fp16, the fp16 product;
  * each layer's delta: the fp16 matrix product, then the same transfer with the hidden activation;
  * dL/dinput.

exact=True rounds nowhere: the exact float64 network, whose analytic gradients finite differences check
(tests/test_mlp_reference.py). Sine is refused, as the engine refuses it for training: it has no
backward from its forward value (common_device.h:261-265).

Parameter layout (the engine's): [W x IN | (NH - 1) W x W | OUTP x W] row-major fp16, the one OUTP x IN
matrix when NH == 0. Rows are AoS: x [B][IN], dL/dy [B][OUTP].

The bounds of the Module matrix (tests/test_gpu_module_matrix.py, tests/test_mlp_reference.py) are
restated here once, in check_output / check_wgrad / check_dinput / aggregate_bar; they are helpers.py's.
"""
import numpy as np

from helpers import assert_within_fp16_ulps, assert_wgrad_per_element, rel_err, wgrad_per_element_bound

ACTIVATIONS = ["None", "ReLU", "LeakyReLU", "Exponential", "Sigmoid", "Squareplus", "Softplus", "Tanh"]
K_ACT = 10.0  # common_device.h:100


def f64_to_f16(r):
    """float64 -> the float16 value (as float64) with ONE round-to-nearest-even: float32 with
    round-to-odd first, which makes the float32 -> float16 step exact (a direct cast may round twice)."""
    r = np.asarray(r, np.float64)
    f = r.astype(np.float32)
    inexact = f.astype(np.float64) != r
    even = (f.view(np.uint32) & 1) == 0
    toward = np.where(r > f.astype(np.float64), np.float32(np.inf), np.float32(-np.inf))
    f = np.where(inexact & even, np.nextafter(f, toward), f)
    with np.errstate(over="ignore"):
        return f.astype(np.float16).astype(np.float64)


def _key(name):
    k = name.lower()
    if k == "sine":
        raise ValueError("Sine has no backward from its forward value: refused for training")
    names = [a.lower() for a in ACTIVATIONS]
    if k not in names:
        raise ValueError("unknown activation " + name)
    return k


def act_forward(name, z):
    """warp_activation (common_device.h:102-160) in float64"""
    k = _key(name)
    if k == "none":
        return z
    if k == "relu":
        return np.maximum(z, 0.0)
    if k == "leakyrelu":
        return z * np.where(z > 0.0, 1.0, 0.01)
    if k == "exponential":
        return np.exp(z)
    if k == "sigmoid":
        return 1.0 / (1.0 + np.exp(-z))
    if k == "squareplus":
        t = z * K_ACT
        return 0.5 * (t + np.sqrt(t * t + 4.0)) / K_ACT
    if k == "softplus":
        return np.logaddexp(z * K_ACT, 0.0) / K_ACT
    return np.tanh(z)


def act_factor(name, y, rnd=lambda v: v):
    """d act / d z written in the forward value y (warp_activation_backward, common_device.h:240-297);
    rnd rounds where the reference's expression is fp16 (Sigmoid's 1 - y)."""
    k = _key(name)
    if k == "none":
        return np.ones_like(y)
    if k == "relu":
        return (y > 0.0).astype(np.float64)
    if k == "leakyrelu":
        return np.where(y > 0.0, 1.0, 0.01)
    if k == "exponential":
        return y
    if k == "sigmoid":
        return y * rnd(1.0 - y)
    if k == "squareplus":
        t = y * K_ACT
        return t * t / (t * t + 1.0)
    if k == "softplus":
        return 1.0 - np.exp(-y * K_ACT)
    return 1.0 - y * y


def split_params(W, IN, NH, OUTP, params16):
    """the fp16 parameter bits as float64 matrices [M_0 .. M_NH] ([M_out] alone for NH == 0)"""
    p = np.asarray(params16, np.uint16).view(np.float16).astype(np.float64)
    shapes = [(OUTP, IN)] if NH == 0 else [(W, IN)] + [(W, W)] * (NH - 1) + [(OUTP, W)]
    assert p.size == sum(r * c for r, c in shapes), (p.size, shapes)
    mats, off = [], 0
    for r, c in shapes:
        mats.append(p[off:off + r * c].reshape(r, c))
        off += r * c
    return mats


def _h(a):
    return np.asarray(a, np.uint16).view(np.float16).astype(np.float64)


def mlp_reference(W, IN, NH, OUTP, act, out_act, params16, x16, dout16, exact=False, mats=None, x=None, dout=None,
                  backward=True):
    """Forward + backward. params16 / x16 / dout16: fp16 bits (uint16); exact mode may pass float64 mats /
    x / dout instead. Returns a dict:
      out [B][OUTP], hidden [a_1 .. a_NH], wgrad [dM_0 .. dM_NH] (float64, per matrix), dinput [B][IN],
      mag_w [per matrix] = sum_i |delta_i| |a_i| and mag_in [B][IN]: the abs-backprop magnitudes, the
      deltas propagated through |M| with |transfer factor| (the definition of oracle.mlp_wgrad_magnitude).
    The smooth activations compute that factor from a rounded fp16 forward value (Sigmoid's y (1 - y), Tanh's
    1 - y^2, Squareplus); the fp32 oracle stays below 0.06 of the bound on every such case of the matrix
    (tests/test_mlp_reference.py), so the magnitudes carry no extra term for it."""
    rnd = (lambda v: v) if exact else f64_to_f16
    mats = split_params(W, IN, NH, OUTP, params16) if mats is None else mats
    a = _h(x16) if x is None else np.asarray(x, np.float64)
    g = _h(dout16) if dout is None else np.asarray(dout, np.float64)
    acts = [a]
    for k in range(NH):
        a = rnd(act_forward(act, a @ mats[k].T))
        acts.append(a)
    y = rnd(act_forward(out_act, a @ mats[NH].T))
    if not backward:
        return {"out": y, "hidden": acts[1:]}

    def transfer(name, gv, fwd, mag=False):
        """g * (T)factor(fwd): fp16 g, fp16 factor, fp16 product (None / ReLU pass g or 0)"""
        k = _key(name)
        gv = rnd(gv)
        if k == "none":
            return gv
        if k == "relu":
            return gv * (fwd > 0.0)
        f = rnd(act_factor(name, fwd, rnd))
        if mag:  # the magnitude chain: unrounded
            return gv * np.abs(f)
        return rnd(gv * f)

    g_abs = np.abs(transfer(out_act, np.abs(g), y, mag=True))
    g = transfer(out_act, g, y)
    wgrad, mag_w = [None] * (NH + 1), [None] * (NH + 1)
    d, d_abs = g, g_abs
    for k in range(NH, -1, -1):
        wgrad[k] = d.T @ acts[k]
        mag_w[k] = np.abs(d_abs).T @ np.abs(acts[k])
        back, back_abs = d @ mats[k], np.abs(d_abs) @ np.abs(mats[k])
        if k > 0:
            d = transfer(act, back, acts[k])
            d_abs = np.abs(transfer(act, back_abs, acts[k], mag=True))
    return {"out": y, "hidden": acts[1:], "wgrad": wgrad, "dinput": rnd(back), "mag_w": mag_w, "mag_in": back_abs,
            "dout_transferred": g}


# ---- the bounds, restated once (helpers.py derives them) ----
ULPS = 8


def check_output(got, ref):
    """network outputs: 4 fp16 ulps at the output scale (helpers.assert_within_fp16_ulps)"""
    assert_within_fp16_ulps(got, ref, n_ulp=4)


def matrix_names(NH):
    return ["Wout"] if NH == 0 else ["W0"] + [f"W{k}" for k in range(1, NH)] + ["Wout"]


def check_wgrad(got_flat, ref, fp16_out=True):
    """weight gradients per element and per matrix: helpers.assert_wgrad_per_element with the float64
    magnitude, 8 ulps (+ the fp16 rounding of the gradient the Module returns). Returns
    {matrix name: worst ratio}; a matrix over the bound fails with its name."""
    got_flat = np.asarray(got_flat, np.float64)
    ratios, off = {}, 0
    for name, r, m in zip(matrix_names(len(ref["wgrad"]) - 1), ref["wgrad"], ref["mag_w"]):
        n = r.size
        try:
            ratios[name] = assert_wgrad_per_element(got_flat[off:off + n], r.ravel(), m.ravel(), ulps=ULPS, fp16_out=fp16_out)
        except AssertionError as e:
            raise AssertionError((name,) + tuple(e.args)) from None
        off += n
    assert off == got_flat.size, (off, got_flat.size)
    return ratios


def check_wgrad_sum(got_flat, refs, bar, per_element=True):
    """The weight gradient torch accumulates when one module is called several times in one graph: the
    fp32 sum of the calls' fp16 gradients, against the sum of the calls' float64 references. Per element and
    per matrix the bound is the sum of the calls' own bounds (check_wgrad's, fp16 gradient) plus the rounding
    of each fp32 addition, 2^-24 of the |reference| sums; relative L2 of the whole sum within bar (that alone with per_element=False:
    unfiltered samples of a branchy network). Returns {matrix name: worst ratio, "agg_w": relative L2}."""
    got_flat = np.asarray(got_flat, np.float64)
    ratios, off = {}, 0
    for k, name in enumerate(matrix_names(len(refs[0]["wgrad"]) - 1) if per_element else []):
        rs = [r["wgrad"][k].ravel() for r in refs]
        bound = sum(wgrad_per_element_bound(r, ref["mag_w"][k].ravel(), ulps=ULPS, fp16_out=True) for r, ref in zip(rs, refs))
        bound = bound + (len(refs) - 1) * 2.0 ** -24 * sum(np.abs(r) for r in rs)
        n = rs[0].size
        q = np.abs(got_flat[off:off + n] - sum(rs)) / bound
        j = int(np.argmax(q))
        assert q[j] <= 1.0, (name, float(q[j]), j, got_flat[off + j], float(sum(rs)[j]))
        ratios[name] = float(q[j])
        off += n
    assert off == got_flat.size or not per_element, (off, got_flat.size)
    flat = sum(np.concatenate([w.ravel() for w in r["wgrad"]]) for r in refs)
    ratios["agg_w"] = rel_err(got_flat, flat)
    assert ratios["agg_w"] <= bar, ("wgrad rel L2", ratios["agg_w"], bar)
    return ratios


def check_dinput(got, ref_dinput, mag_in):
    """dL/dinput (or dL/d(encoding)) per element: 8 * 2^-10 mag_in + 2^-11 |ref| + 2^-25 (the same form,
    the abs-backprop input magnitude; the reference value is an fp16). Returns the worst ratio."""
    got, r, m = (np.asarray(v, np.float64) for v in (got, ref_dinput, mag_in))
    bound = ULPS * 2.0 ** -10 * m + 2.0 ** -11 * np.abs(r) + 2.0 ** -25
    q = np.abs(got - r) / bound
    k = int(np.argmax(q))
    assert q.flat[k] <= 1.0, ("dinput", float(q.flat[k]), k, got.flat[k], r.flat[k], m.flat[k])
    return float(q.flat[k])


def aggregate_bar(W, NH, out_act):
    """relative L2 bar of the existing engine tests (test_gpu_tile_engine.py, test_gpu_layered.py): 1e-3;
    2e-3 for W >= 128, >= 5 hidden layers and exponential-type output activations"""
    return 2e-3 if (W >= 128 or NH >= 5 or out_act.lower() in ("exponential", "softplus", "squareplus")) else 1e-3


def check_aggregate(got_flat, ref, bar, dinput=None):
    """relative L2 of the whole weight gradient (and of dL/dinput) within bar: the plain bar, also for the
    fp16 gradient a Module returns, as in the existing Module tests (its rounding is ~2e-4 of the norm for
    gradients in the normal fp16 range, which the matrix's scaled parameters give)."""
    flat = np.concatenate([w.ravel() for w in ref["wgrad"]])
    e = rel_err(got_flat, flat)
    assert e <= bar, ("wgrad rel L2", e, bar)
    if dinput is not None:
        ed = rel_err(dinput, ref["dinput"])
        assert ed <= bar, ("dinput rel L2", ed, bar)
        return e, ed
    return e, None
