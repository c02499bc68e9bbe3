"""Shared test helpers: seeded synthetic batches (reference sample's pcg32{1337} strided RNG for
positions, an analytic RGB field for targets) and device<->host plumbing for trainer buffers."""
import ctypes
import json
import os

import numpy as np

from oracle import oracle as O

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CONFIG_HASH = json.load(open(os.path.join(GOLD, "config_hash.json")))
CONFIG_ONEBLOB = json.load(open(os.path.join(GOLD, "config_oneblob.json")))


def rgb_field(pos):
    """Smooth synthetic RGB image on [0,1)^2 (stands in for albert.jpg's bilinear texture fetch)."""
    x, y = pos[:, 0].astype(np.float64), pos[:, 1].astype(np.float64)
    r = 0.5 + 0.5 * np.sin(9.0 * x) * np.cos(7.0 * y)
    g = 0.5 + 0.4 * np.sin(23.0 * x * y + 1.0)
    b = 0.5 + 0.3 * np.cos(31.0 * x) * np.sin(17.0 * y) + 0.1 * ((x * 40).astype(np.int64) % 2)
    return np.stack([r, g, b], axis=1).astype(np.float32)


def make_batch(B, seed=1337, step=0, n_dims=2):
    """positions [B,n_dims] from pcg32{seed} in generate_random_uniform order (random.h:39-70),
    advanced by `step` batches; targets from rgb_field (of the first two coordinates)."""
    r = O.pcg32(seed)
    if step:
        O.lib().orc_pcg32_advance(ctypes.byref(r), n_dims * B * step)
    pos = O.generate_uniform(r, n_dims * B).reshape(B, n_dims)
    return pos, rgb_field(pos)


_hip = None


def hip():
    global _hip
    if _hip is None:
        import torch  # noqa: F401  (loads the HIP runtime torch uses; same SONAME as ours)
        _hip = ctypes.CDLL("libamdhip64.so.7")
        _hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        _hip.hipDeviceSynchronize.argtypes = []
    return _hip


def d2h(ptr, n, dtype):
    """copy n elements of dtype from a device pointer to a numpy array"""
    out = np.empty(n, dtype=dtype)
    hip().hipDeviceSynchronize()
    rc = hip().hipMemcpy(out.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(ptr), out.nbytes, 2)  # D2H
    assert rc == 0
    return out


def trainer_arrays(t):
    from tinycudann import _lib as L
    lib = L.lib()
    n = t.n_params
    return {
        "w32": d2h(lib.tcnn_trainer_params_fp32(t.h), n, np.float32),
        "w16": d2h(lib.tcnn_trainer_params(t.h), n, np.uint16),
        "g16": d2h(lib.tcnn_trainer_param_gradients(t.h), n, np.uint16),
        "g32": d2h(lib.tcnn_trainer_gradients_fp32(t.h), n, np.float32),
    }


ADAM_ARRAYS = ("w32", "w16", "m1", "m2", "steps")


def fresh_adam_state(w32):
    """the optimizer state of a new trainer with masters w32 (fp16 copies rounded from them, zero moments)"""
    w32 = np.array(w32, np.float32)
    n = w32.size
    return {"w32": w32, "w16": O.f2h(w32), "m1": np.zeros(n, np.float32), "m2": np.zeros(n, np.float32),
            "steps": np.zeros(n, np.uint32)}


def oracle_adam_step(opt, n_matrix, loss_scale, global_step, state, g16):
    """One step of the oracle's Adam (optimizer block opt, global_step = the optimizer's step count after its
    increment) on state (ADAM_ARRAYS, updated in place) with the fp16 gradient bits g16."""
    O.adam_step(O.adam_cfg(opt), n_matrix, float(loss_scale), int(global_step), state["w32"], state["w16"],
                np.ascontiguousarray(g16, np.uint16), state["m1"], state["m2"], state["steps"])


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def adam_arrays(t):
    """the trainer's Adam arrays on the host: ADAM_ARRAYS and the fp16 gradients g16"""
    a = trainer_arrays(t)
    m1, m2, st = (x.cpu().numpy() for x in t.optimizer_state())
    return {"w32": a["w32"], "w16": a["w16"], "g16": a["g16"], "m1": m1, "m2": m2, "steps": st.view(np.uint32)}


def assert_adam_bits(got, ref, what, names=ADAM_ARRAYS, where=None):
    """got[k] and ref[k] bit-identical for every k of names (on the elements where, if given)"""
    for k in names:
        g, r = bits(got[k]), bits(ref[k])
        if where is not None:
            g, r = g[where], r[where]
        bad = np.flatnonzero(g != r)
        # (what, array, mismatches, first mismatching index, got bits, expected bits)
        assert bad.size == 0, (what, k, int(bad.size), int(bad[0]), hex(int(g[bad[0]])), hex(int(r[bad[0]])))


def oracle_grad16(cfg, w16, pos, tgt, loss_scale=128.0, n_threads=4):
    """fp16 parameter gradients (bits) of one oracle training step of cfg (a 32-column grid encoding or OneBlob,
    ReLU MLP, RelativeL2) at fp16 parameters w16, with the loss scaled by loss_scale: what OracleModel.train_step
    leaves in grad16 at its fixed loss scale of 128."""
    enc_cfg, net = cfg["encoding"], cfg["network"]
    W, NH = net["n_neurons"], net["n_hidden_layers"]
    w16 = np.asarray(w16, np.uint16)
    if enc_cfg["otype"].lower() == "oneblob":
        D, nb = pos.shape[1], enc_cfg["n_bins"]
        IN = (D * nb + 15) // 16 * 16
        nm = O.mlp_n_params(W, IN, NH, 16)
        enc = O.oneblob_fwd(pos, nb, IN - D * nb)
        out16, hidden = O.mlp_fwd(W, IN, NH, 16, w16[:nm], enc, input_soa=False, n_threads=n_threads)
        _, dout, _ = O.relative_l2(out16, tgt, loss_scale=loss_scale)
        wg, _ = O.mlp_bwd(W, IN, NH, 16, w16[:nm], enc, hidden, dout, input_soa=False, want_dinput=False, n_threads=n_threads)
        return O.f2h(wg)
    g = O.grid_cfg(enc_cfg, pos.shape[1])
    IN = g.n_levels * g.n_features_per_level
    assert IN % 16 == 0
    nm = O.mlp_n_params(W, IN, NH, 16)
    enc = O.grid_fwd(g, pos, w16[nm:])
    out16, hidden = O.mlp_fwd(W, IN, NH, 16, w16[:nm], enc, n_threads=n_threads)
    _, dout, _ = O.relative_l2(out16, tgt, loss_scale=loss_scale)
    wg, denc = O.mlp_bwd(W, IN, NH, 16, w16[:nm], enc, hidden, dout, n_threads=n_threads)
    return O.f2h(np.concatenate([wg, O.grid_bwd(g, pos, denc)]))


def rel_err(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def assert_within_fp16_ulps(got, ref, n_ulp=4):
    """max |got - ref| <= n_ulp fp16 ulps at the output scale (max |ref|): the network-output bar
    (fp32 MFMA accumulation vs the oracle's CPU summation order). A fixed absolute tolerance above
    the output scale would accept unwritten (zero) rows -- the seed-1337 init gives outputs ~1e-5."""
    scale = float(np.abs(ref).max())
    assert scale > 0
    ulp = float(np.spacing(np.float16(scale)))
    err = float(np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64)).max())
    assert err <= n_ulp * ulp, (err, ulp, scale)
    return err / ulp


def wgrad_per_element_bound(ref, mag, ulps=8, fp16_out=False, floor_rel=1e-6):
    """the per-element bound of assert_wgrad_per_element (derived there), as an array"""
    ref, mag = np.asarray(ref, np.float64), np.asarray(mag, np.float64)
    bound = ulps * 2.0 ** -10 * mag + floor_rel * np.abs(ref).max()
    if fp16_out:
        bound += 2.0 ** -11 * np.abs(ref) + 2.0 ** -25  # fp16 rounding (subnormals: half the smallest step)
    return bound


def assert_wgrad_per_element(got, ref, mag, ulps=8, fp16_out=False, floor_rel=1e-6):
    """Per-element bound of an MLP weight gradient dW = sum_i delta_i a_i. Between the HIP kernels
    (fp32 MFMA) and the oracle (fp32 CPU order) a term's fp16 activation or delta can round to the
    neighbouring fp16 value, so each term may differ by a few fp16 ulps (2^-10 relative):
    |got - ref| <= ulps * 2^-10 * mag + floor_rel * max|ref| (+ 2^-11 |ref| when got was rounded to
    fp16), mag = sum_i |delta_i a_i| (oracle.mlp_wgrad_magnitude). The fp32 summation error of either
    side (K * 2^-24 relative) is far below this."""
    got, ref, mag = (np.asarray(v, np.float64) for v in (got, ref, mag))
    r = np.abs(got - ref) / wgrad_per_element_bound(ref, mag, ulps, fp16_out, floor_rel)
    k = int(np.argmax(r))
    assert r[k] <= 1.0, (float(r[k]), k, got[k], ref[k], mag[k])
    return float(r[k])


def relu_margin_ok(W, IN, NH, params16, x_rows, tau=2.0 ** -11, check_output=False, scale=1.0, act="ReLU", out_rows=0):
    """Per sample: True when no hidden pre-activation of the ReLU MLP lies within tau * sum_k |w_k a_k|
    of zero. At such a boundary fp32-MFMA and CPU summation orders may legitimately take different
    ReLU branches (a discrete difference no rounding bound covers); per-element gradient checks run on
    batches of samples clear of it, the aggregate checks on every sample. tau = 2^-11 covers one fp16
    ulp of difference in any single input term (|w_k| ulp(a_k) <= 2^-11 |w_k a_k|) plus the fp32
    summation-order noise. check_output (loss-driven steps): also False when the output's fp16 rounding
    is within 2^-18 sum |w a| of a rounding boundary. x_rows: float [B][IN] (the fp16 encoded input values).
    scale: the parameters are fp16(scale * params16) (a test's per-case constant). act: the hidden
    activation; only ReLU and LeakyReLU (act = "LeakyReLU": the same boundary, the leaky forward) have a
    branch, any other name checks no hidden layer. out_rows > 0: the network's output activation is
    branchy too -- also False when one of the out_rows output pre-activations is within the margin of
    zero. NH = 0 has no hidden layer: only out_rows can exclude a sample."""
    p = O.h2f(np.asarray(params16, np.uint16)).astype(np.float64)
    if scale != 1.0:
        p = O.h2f(O.f2h((p * scale).astype(np.float32))).astype(np.float64)
    leaky = act.lower() == "leakyrelu"
    branchy = act.lower() in ("relu", "leakyrelu")
    assert branchy or act.lower() == "none" or not check_output, "check_output needs a None, ReLU or LeakyReLU network: " + act
    assert branchy or act.lower() == "none" or out_rows == 0 or NH == 0, \
        "the hidden activation must be None, ReLU or LeakyReLU when out_rows > 0: " + act
    mats, off, k = [], 0, IN
    for _ in range(NH):
        mats.append(p[off:off + W * k].reshape(W, k))
        off += W * k
        k = W
    a = np.asarray(x_rows, np.float64)
    ok = np.ones(a.shape[0], bool)
    if not branchy:
        for Wm in mats:  # hidden None: linear layers, no branch (any other name: only reached with out_rows == 0)
            a = (a @ Wm.T).astype(np.float16).astype(np.float64)
        mats = []
    for Wm in mats:
        z = a @ Wm.T
        mag = np.abs(a) @ np.abs(Wm).T
        ok &= np.all(np.abs(z) >= tau * mag, axis=1)
        a = np.where(z > 0.0, z, 0.01 * z if leaky else 0.0).astype(np.float16).astype(np.float64)  # the fp16 post-activation
    if out_rows:
        Wo = p[off:off + out_rows * k].reshape(out_rows, k)
        ok &= np.all(np.abs(a @ Wo.T) >= tau * (np.abs(a) @ np.abs(Wo).T), axis=1)
    if not check_output:
        return ok
    # the output's fp16 rounding: both sides must round to the same value, else the loss gradient
    # 2 (p - t) / (p^2 + 0.01) of a sample with a small error p - t changes by a large factor
    Wo = p[off:off + 16 * k].reshape(16, k)
    y, ymag = a @ Wo.T, np.abs(a) @ np.abs(Wo).T
    eps = 2.0 ** -18 * ymag
    ok &= np.all((y - eps).astype(np.float16) == (y + eps).astype(np.float16), axis=1)
    return ok


def relu_safe_grid_batch(cfg, params16, B, seed=1337, step=0, n_dims=2):
    """A B-point batch (make_batch order, n_dims position columns) of samples clear of the ReLU boundaries
    (relu_margin_ok) for the grid-encoded network of cfg at params16."""
    W, NH = cfg["network"]["n_neurons"], cfg["network"]["n_hidden_layers"]
    g = O.grid_cfg(cfg["encoding"], n_dims)
    IN = g.n_levels * g.n_features_per_level
    nm = O.mlp_n_params(W, IN, NH, 16)
    p16 = np.asarray(params16, np.uint16)
    pos, tgt = make_batch(4 * B, seed=seed, step=step, n_dims=n_dims)
    enc = O.h2f(O.grid_fwd(g, pos, p16[nm:])).T  # [B][IN]
    ok = relu_margin_ok(W, IN, NH, p16[:nm], enc, check_output=True)
    assert ok.sum() >= B, ok.sum()
    idx = np.nonzero(ok)[0][:B]
    return np.ascontiguousarray(pos[idx]), np.ascontiguousarray(tgt[idx])


def trainer_grad_bounds(cfg, params16, pos, tgt, n_threads=4):
    """The oracle's intermediates of one training step on (pos, tgt) with parameters params16 (grid
    encoding + FullyFusedMLP, RelativeL2): returns (mlp magnitude, grid bound) for per-element checks of
    the trainer's fp32 gradient sums. Grid bound = the grid backward's own bound for the oracle's
    dL/d(encoding) (oracle.grid_grad_tolerance) + 8 fp16 ulps of every update's abs-backprop magnitude
    (the GPU's dL/d(encoding) comes from its own MLP backward: an fp16 delta upstream that rounds to
    its neighbouring value moves it by up to an ulp of that magnitude, cancellation included)."""
    enc_cfg, net = cfg["encoding"], cfg["network"]
    W, NH = net["n_neurons"], net["n_hidden_layers"]
    act = O.act_code(net.get("activation", "ReLU"))  # the hidden activation (ReLU or None: the fused kernel's two)
    g = O.grid_cfg(enc_cfg, pos.shape[1])
    IN = g.n_levels * g.n_features_per_level
    nm = O.mlp_n_params(W, IN, NH, 16)
    p16 = np.asarray(params16, np.uint16)
    enc = O.grid_fwd(g, pos, p16[nm:])
    out16, hidden = O.mlp_fwd(W, IN, NH, 16, p16[:nm], enc, activation=act, n_threads=n_threads)
    _, dout, _ = O.relative_l2(out16, tgt)
    mag, denc_abs = O.mlp_wgrad_magnitude(W, IN, NH, 16, p16[:nm], enc, hidden, dout, activation=act, n_threads=n_threads,
                                          want_dinput=True)
    _, denc = O.mlp_bwd(W, IN, NH, 16, p16[:nm], enc, hidden, dout, activation=act, n_threads=n_threads)
    ref_grid = O.grid_bwd(g, pos, denc)
    absum, _ = O.grid_bwd_stats(g, pos, denc_abs)
    grid_bound = O.grid_grad_tolerance(g, pos, denc, ref_grid) + 8 * 2.0 ** -10 * absum.astype(np.float64)
    return mag, grid_bound


def assert_trainer_grads_per_element(g32, ref32, n_mlp, mag, grid_bound):
    """returns the worst error / bound ratios (network part, grid part)"""
    r_mlp = assert_wgrad_per_element(g32[:n_mlp], ref32[:n_mlp], mag)
    got, ref = np.asarray(g32[n_mlp:], np.float64), np.asarray(ref32[n_mlp:], np.float64)
    r = np.abs(got - ref) / (grid_bound + 1e-30)
    k = int(np.argmax(r))
    assert r[k] <= 1.0, (float(r[k]), k, got[k], ref[k], grid_bound[k])
    return r_mlp, float(r[k])
