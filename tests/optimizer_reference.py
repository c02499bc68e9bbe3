"""numpy restatement of the elementwise optimizers beside Adam and of their stacking, written from the
reference's headers: optimizers/sgd.h:44-69, exponential_decay.h:60-80, ema.h:45-136, lookahead.h:45-96,
batched.h:46-89.

Host-side factors (the ExponentialDecay factor, base x factor, the EMA debias pair) are computed in float32 /
double exactly as the reference's host code computes them. Per-element updates are computed in float64 from
the exact values of their fp32 / fp16 inputs. Beside each value comes its absolute-mode value A: the same
expression with every term replaced by its magnitude, the scale of the fp32 rounding bound

    |got - ref64| <= (n_ops + 2) * 2^-24 * A + 2^-149            (fp32_bound)

n_ops = the rounded fp32 operations of the reference's expression (N_OPS); the + 2 admits any contraction or
association of the same operations.

fp16 arrays are uint16 bit patterns throughout (h2f / f2h convert)."""
import numpy as np

N_OPS = {"sgd": 5, "ema": 6, "lookahead": 4, "pool": 2}
DEFAULTS = {
    "sgd": {"learning_rate": 1e-3, "l2_reg": 1e-8},
    "ema": {"decay": 0.99, "full_precision": False},
    "lookahead": {"alpha": 0.5, "n_steps": 16},
    "batched": {"batch_size_multiplier": 16},
    "exponentialdecay": {"decay_base": 0.1, "decay_interval": 10000, "decay_start": 10000, "decay_end": 10000000},
}
REPORTED_OTYPE = {"sgd": "SGD", "ema": "EMA", "lookahead": "Lookahead", "batched": "Batched",
                  "exponentialdecay": "ExponentialDecay", "adam": "Adam"}


def h2f(bits):
    """fp16 bit patterns -> float64 (exact)"""
    return np.ascontiguousarray(bits, np.uint16).view(np.float16).astype(np.float64)


def f2h(x):
    """fp32 values -> fp16 bit patterns, round to nearest even from the fp32 value"""
    return np.ascontiguousarray(x, np.float32).astype(np.float16).view(np.uint16)


def f64(x):
    return np.asarray(x, np.float64)


def fp32_bound(A, n_ops):
    return (n_ops + 2) * 2.0 ** -24 * f64(A) + 2.0 ** -149


def fp16_ulp(x):
    """one fp16 ulp at |x| (the subnormal step 2^-24 at the least)"""
    a = np.maximum(np.abs(f64(x)), 2.0 ** -14)
    return 2.0 ** (np.floor(np.log2(a)) - 10)


# ---- per-element updates: (value64, absolute-mode value) ----
def sgd_update(w32, g16, loss_scale, lr, l2_reg):
    """sgd.h:56-68: g = g16 / loss_scale + l2_reg * w; w - lr * g"""
    w, g = f64(w32), h2f(g16)
    ls, lr, l2 = float(np.float32(loss_scale)), float(np.float32(lr)), float(np.float32(l2_reg))
    grad = g / ls + l2 * w
    agrad = np.abs(g / ls) + np.abs(l2 * w)
    return w - lr * grad, np.abs(w) + abs(lr) * agrad


def ema_update(prev, w16, decay, debias_old, debias_new):
    """ema.h:57 / 74: ((prev * decay) * debias_old + w * (1 - decay)) * debias_new; prev: tmp (fp32) or the
    fp16 weights_ema widened"""
    p, w = f64(prev), h2f(w16)
    d, o, n = float(np.float32(decay)), float(np.float32(debias_old)), float(np.float32(debias_new))
    a, b = p * d * o, w * (1.0 - d)
    return (a + b) * n, (np.abs(a) + np.abs(b)) * abs(n)


def ema_debias(decay, step):
    """ema.h:107-108 on the host: std::pow(float, uint32_t) is pow(double, double), narrowed to float;
    1 - (float) and 1.0f / (...) are float arithmetic. step = the nested optimizer's count after its step."""
    d = float(np.float32(decay))
    old = np.float32(1) - np.float32(d ** float(step - 1))
    new = np.float32(1.0) / (np.float32(1) - np.float32(d ** float(step)))
    return np.float32(old), np.float32(new)


def lookahead_blend(look16, w32, alpha):
    """lookahead.h:55: look * (1 - alpha) + w * alpha"""
    l, w, a = h2f(look16), f64(w32), float(np.float32(alpha))
    x, y = l * (1.0 - a), w * a
    return x + y, np.abs(x) + np.abs(y)


def batched_pool(pool, g16, multiplier, first):
    """batched.h:56-60: (first ? 0 : pool) + g16 / multiplier"""
    p = np.zeros_like(f64(pool)) if first else f64(pool)
    q = h2f(g16) / float(multiplier)
    return p + q, np.abs(p) + np.abs(q)


class ExponentialDecay:
    """exponential_decay.h:48-80: the factor is a running float product; step = the nested count before the step"""

    def __init__(self, base_lr, decay_base=0.1, decay_interval=10000, decay_start=10000, decay_end=10000000):
        self.base_lr = np.float32(base_lr)
        self.factor = np.float32(1.0)
        self.decay_base = np.float32(decay_base)
        self.interval, self.start, self.end = int(decay_interval), int(decay_start), int(decay_end)

    def before_step(self, step):
        """the nested learning rate of the step that starts at nested count `step`"""
        if step == 0:
            self.factor = np.float32(1.0)
        if step >= self.start and (step - self.start) % self.interval == 0 and step <= self.end:
            self.factor = np.float32(self.factor * self.decay_base)
        return self.learning_rate()

    def learning_rate(self):
        return np.float32(self.base_lr * self.factor)

    def set_learning_rate(self, v):
        self.base_lr = np.float32(np.float32(v) / self.factor)
        return self.learning_rate()


# ---- the stack driver ----
def _kind(cfg):
    return str(cfg.get("otype", "Adam")).lower()


class Stack:
    """An "optimizer" block as a chain of levels, outermost first, with the host-side state of each
    (counters, decay factor). step() advances a state dict one optimizer step and returns, per array it
    changed, what a correct engine may hold:

        ("bits", expected)                  equal bit for bit
        ("f32", ref64, A, n_ops)            fp32 value within fp32_bound(A, n_ops) of ref64
        ("f16", ref64, A, n_ops)            fp16 value with no fp32 witness: fp32_bound plus one fp16 ulp of |ref|
        ("f16_of", name)                    fp16 value = f16_rn of the fp32 array `name`, bit for bit

    State arrays: w32 (float32), w16 (uint16), and per level weights_ema / weights_lookahead /
    averaged_gradients_half (uint16), tmp / averaged_gradients (float32); an Adam level also m1, m2 (float32)
    and steps (uint32), advanced by adam_fn(opt_block, global_step, state, g16) in place (bit-exact, e.g.
    helpers.oracle_adam_step). The driver's own trajectory rounds every fp32 value from its float64 value."""

    def __init__(self, cfg, adam_fn=None):
        self.levels = []
        c = cfg
        while True:
            k = _kind(c)
            assert k in REPORTED_OTYPE, k
            p = dict(DEFAULTS.get(k, {}))
            p.update({key: v for key, v in c.items() if key not in ("otype", "nested")})
            self.levels.append({"kind": k, "p": p, "step": 0})
            if k in ("adam", "sgd"):
                break
            c = c.get("nested", {})
        self.adam_fn = adam_fn
        self.observed = None
        for i in reversed(range(len(self.levels))):  # innermost first: a level's base rate is its nested level's
            lv = self.levels[i]
            if lv["kind"] == "exponentialdecay":
                lv["sched"] = ExponentialDecay(self._lr(i + 1), **lv["p"])

    # Optimizer::learning_rate / step of level i
    def _lr(self, i):
        lv = self.levels[i]
        if lv["kind"] == "adam":
            return np.float32(lv["p"].get("learning_rate", 1e-3))
        if lv["kind"] == "sgd":
            return np.float32(lv["p"]["learning_rate"])
        if lv["kind"] == "exponentialdecay":
            return lv["sched"].learning_rate()
        return self._lr(i + 1)

    def _set_lr(self, i, v):
        lv = self.levels[i]
        if lv["kind"] in ("adam", "sgd"):
            lv["p"]["learning_rate"] = float(np.float32(v))
        elif lv["kind"] == "exponentialdecay":
            self._set_lr(i + 1, lv["sched"].set_learning_rate(v))
        else:
            self._set_lr(i + 1, v)

    def count(self, i=0):
        lv = self.levels[i]
        return lv["step"] if lv["kind"] in ("adam", "sgd", "batched") else self.count(i + 1)

    def learning_rate(self):
        return float(self._lr(0))

    def set_learning_rate(self, v):
        self._set_lr(0, v)

    def custom_weights(self, i=0):
        """name of the inference-parameter array, or None (the training parameters)"""
        k = self.levels[i]["kind"]
        if k in ("adam", "sgd"):
            return None
        if k == "ema":
            return "weights_ema"
        if k == "lookahead":
            return "weights_lookahead"
        return self.custom_weights(i + 1)

    def hyperparams(self, i=0):
        lv = self.levels[i]
        h = {"otype": REPORTED_OTYPE[lv["kind"]]}
        if lv["kind"] != "adam":
            h.update(lv["p"])
        if lv["kind"] not in ("adam", "sgd"):
            h["nested"] = self.hyperparams(i + 1)
        return h

    def step(self, state, g16, loss_scale=128.0, observed=None):
        """one Optimizer::step of the outermost level on state (updated in place) with fp16 gradients g16.
        observed: the engine's state after the same step. Where a value that is only bounded (the Batched
        pool) feeds a later stage of the same step, the driver continues from the engine's own value -- it is
        checked against its bound like any other -- so that the later stage is compared like for like."""
        checks = {}
        self.observed = observed
        self._step(0, state, np.ascontiguousarray(g16, np.uint16), float(loss_scale), checks)
        return checks

    def _step(self, i, S, g16, ls, checks):
        lv = self.levels[i]
        k, p = lv["kind"], lv["p"]
        if k == "adam":
            lv["step"] += 1
            before = {n: S[n].copy() for n in ("w32", "w16", "m1", "m2", "steps")}
            self.adam_fn(dict(p, otype="Adam"), lv["step"], S, g16)
            prior = checks.get("w32")
            for n in ("w32", "w16", "m1", "m2", "steps"):
                checks[n] = ("bits", S[n].copy())
            if prior is not None and prior[0] == "f32" and np.array_equal(S["w32"].view(np.uint32), before["w32"].view(np.uint32)):
                checks["w32"] = prior  # a frozen Adam: the blend's own value and bound stand
                checks["w16"] = ("f16_of", "w32")
            elif prior is not None and prior[0] == "f32":
                # the input w32 was itself only bounded (a Lookahead blend before this step): with l2_reg =
                # relative_decay = absolute_decay = 0 Adam is w' = rn(w + c) with c independent of w, so the
                # input error passes through unchanged, plus the rounding of the driver's fp32 input (1) and
                # of the two results (2)
                assert not any(float(p.get(q, 0.0 if q != "l2_reg" else 1e-8)) for q in ("l2_reg", "relative_decay", "absolute_decay"))
                _, ref_in, A_in, n_in = prior
                ref = f64(S["w32"]) + (ref_in - f64(before["w32"]))
                checks["w32"] = ("f32", ref, A_in + np.abs(ref) * 3.0 / (n_in + 2), n_in)
                checks["w16"] = ("f16_of", "w32")
            return
        if k == "sgd":
            lv["step"] += 1
            ref, A = sgd_update(S["w32"], g16, ls, p["learning_rate"], p["l2_reg"])
            prior = checks.get("w32")
            n_ops = N_OPS["sgd"]
            if prior is not None and prior[0] == "f32":  # a blend before: its bound passes through (|dw'/dw| <= 1)
                A, n_ops = A + prior[2] * (prior[3] + 2) / (n_ops + 2) + np.abs(ref) / (n_ops + 2), n_ops
            S["w32"] = ref.astype(np.float32)
            S["w16"] = f2h(S["w32"])
            checks["w32"] = ("f32", ref, A, n_ops)
            checks["w16"] = ("f16_of", "w32")
            return
        if k == "exponentialdecay":
            self._set_lr(i + 1, lv["sched"].before_step(self.count(i)))
            self._step(i + 1, S, g16, ls, checks)
            return
        if k == "ema":
            self._step(i + 1, S, g16, ls, checks)
            old, new = ema_debias(p["decay"], self.count(i + 1))
            src = self.custom_weights(i + 1) or "w16"
            if p["full_precision"]:
                ref, A = ema_update(S["tmp"], S[src], p["decay"], old, new)
                S["tmp"] = ref.astype(np.float32)
                S["weights_ema"] = f2h(S["tmp"])
                checks["tmp"] = ("f32", ref, A, N_OPS["ema"])
                checks["weights_ema"] = ("f16_of", "tmp")
            else:
                ref, A = ema_update(h2f(S["weights_ema"]), S[src], p["decay"], old, new)
                S["weights_ema"] = f2h(ref.astype(np.float32))
                checks["weights_ema"] = ("f16", ref, A, N_OPS["ema"])
            return
        if k == "lookahead":
            step = self.count(i + 1)
            if step == 0:
                S["weights_lookahead"] = S["w16"].copy()
            if step % int(p["n_steps"]) == 0:
                ref, A = lookahead_blend(S["weights_lookahead"], S["w32"], p["alpha"])
                S["w32"] = ref.astype(np.float32)
                S["w16"] = f2h(S["w32"])
                S["weights_lookahead"] = S["w16"].copy()
                checks["w32"] = ("f32", ref, A, N_OPS["lookahead"])
                checks["w16"] = ("f16_of", "w32")
                checks["weights_lookahead"] = ("f16", ref, A, N_OPS["lookahead"])
            elif step == 0:
                checks["weights_lookahead"] = ("bits", S["weights_lookahead"].copy())
            self._step(i + 1, S, g16, ls, checks)
            return
        if k == "batched":
            m = int(p["batch_size_multiplier"])
            ref, A = batched_pool(S["averaged_gradients"], g16, m, lv["step"] % m == 0)
            S["averaged_gradients"] = ref.astype(np.float32)
            checks["averaged_gradients"] = ("f32", ref, A, N_OPS["pool"])
            if self.observed is not None:
                S["averaged_gradients"] = np.array(self.observed["averaged_gradients"], np.float32)
            lv["step"] += 1
            if lv["step"] % m == 0:
                S["averaged_gradients_half"] = f2h(S["averaged_gradients"])
                checks["averaged_gradients_half"] = ("f16_of", "averaged_gradients")
                self._step(i + 1, S, S["averaged_gradients_half"], ls, checks)
            return
        raise AssertionError(k)


def fresh_state(w32, stack):
    """the state of a new trainer with fp32 parameters w32 under `stack` (Trainer::initialize_params: the
    custom weights receive the fp16 parameters, every other buffer is zero)"""
    w32 = np.array(w32, np.float32)
    n = w32.size
    S = {"w32": w32, "w16": f2h(w32)}
    for lv in stack.levels:
        k = lv["kind"]
        if k == "adam":
            S.update(m1=np.zeros(n, np.float32), m2=np.zeros(n, np.float32), steps=np.zeros(n, np.uint32))
        elif k == "ema":
            S["weights_ema"] = np.zeros(n, np.uint16)
            if lv["p"]["full_precision"]:
                S["tmp"] = np.zeros(n, np.float32)
        elif k == "lookahead":
            S["weights_lookahead"] = np.zeros(n, np.uint16)
        elif k == "batched":
            S["averaged_gradients"] = np.zeros(n, np.float32)
            S["averaged_gradients_half"] = np.zeros(n, np.uint16)
    cw = stack.custom_weights()
    if cw:
        S[cw] = S["w16"].copy()
    return S


def assert_checks(got, checks, what=""):
    """got: {name: array} of the engine's state after the step; checks: Stack.step's result"""
    for name, c in checks.items():
        g = np.ascontiguousarray(got[name])
        if c[0] == "bits":
            gb, eb = g.view(_uint(g)), np.ascontiguousarray(c[1]).view(_uint(c[1]))
            bad = np.flatnonzero(gb != eb)
            assert bad.size == 0, (what, name, "bits", int(bad.size), int(bad[0]), hex(int(gb[bad[0]])), hex(int(eb[bad[0]])))
        elif c[0] == "f16_of":
            eb, gb = f2h(got[c[1]]), g.view(np.uint16)
            bad = np.flatnonzero(gb != eb)
            assert bad.size == 0, (what, name, "f16_rn(" + c[1] + ")", int(bad.size), int(bad[0]), hex(int(gb[bad[0]])), hex(int(eb[bad[0]])))
        else:
            _, ref, A, n_ops = c
            bound = fp32_bound(A, n_ops)
            val = f64(g) if c[0] == "f32" else h2f(g)
            if c[0] == "f16":
                bound = bound + np.maximum(fp16_ulp(ref), 2.0 ** -24)
            assert np.all(np.isfinite(val)), (what, name)
            r = np.abs(val - ref) / bound
            j = int(np.argmax(r))
            assert r[j] <= 1.0, (what, name, c[0], float(r[j]), j, float(val[j]), float(ref[j]), float(bound[j]))


def _uint(a):
    return {2: np.uint16, 4: np.uint32}[np.asarray(a).dtype.itemsize]
