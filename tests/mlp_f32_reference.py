"""The fp32 network engine (csrc/mlp_f32.hip) against float64: the exact reference, its forward magnitudes,
and per-element bounds derived from the operation count. Plain numpy; shared by tests/test_mlp_f32_reference.py
(CPU: the bounds are neither vacuous nor unreachable) and tests/test_gpu_mlp_f32.py (the kernels).

Truth: mlp_reference(..., exact=True, mats=, x=, dout=) of tests/mlp_reference.py (float64, nothing rounded),
which returns wgrad, dinput, mag_w, mag_in. Beside it, the forward magnitudes m_0 = |x|,
m_{k+1} = L_act |M_k| m_k (L_act the activation's Lipschitz factor; y itself for Exponential).

Bounds. u = 2^-24. No figure below comes from what the kernels produce.

  (1) a k-ordered fp32 FMA chain of K terms errs by at most K u sum |a b|; the f32 MFMA is bit for bit such a
      chain (in a permuted order, which the bound does not depend on). Its inputs are the COMPUTED values of the
      layer below, so with e the error bound of an operand: |computed z - z| <= |M| e + K u |M| (|a| + e).
  (2) an activation maps an error e_z to L e_z, L its Lipschitz factor on the interval (1 for None, ReLU,
      LeakyReLU, Tanh, Softplus, Squareplus; 1/4 for Sigmoid; y exp(e_z) for Exponential), plus the accuracy of
      the device library's fp32 function: 2 c u max(|y|, 1), c the worst error profiles/act_f32_ulps.json records
      for the function in that unit over a dense grid (tools/act_f32_ulps.hip, measured on the functions
      themselves, not through the module), doubled for points off the grid. None and ReLU add nothing; LeakyReLU
      is one multiplication: u |y|.
  (3) the backward takes act' from the STORED forward value: the factor phi(y) is computed from the computed y,
      e_phi = L_phi e_y + 2 c_phi u max(|phi|, 1) (L_phi = sup |d phi / d y|: Exponential 1, Sigmoid 1, Tanh 2,
      Squareplus 6.5 = max 20 t / (t^2 + 1)^2, Softplus 10), and the transferred delta d = g phi errs by
      e_g |phi| + (|g| + e_g) e_phi + u (|g| + e_g)(|phi| + e_phi) (the product's rounding). ReLU / LeakyReLU
      factors are exact for samples clear of the branch (clear_of_branches below filters the batch).
  (4) the data backward is chain (1) over N terms: e_back = e_d |M| + N u (|d| + e_d) |M|.
  (5) the weight gradient sums the batch in slabs of SLAB_ROWS rows, each a chain (1) of SLAB_ROWS terms, and
      adds the n_slabs slab values in a fixed order, one 2^-24 per addition:
      e_w = e_d^T (|a| + e_a) + |d|^T e_a + (SLAB_ROWS + n_slabs) u (|d| + e_d)^T (|a| + e_a).
  (6) + 1e-35 absolute: a subnormal product the matrix core may flush (256 terms of 2^-126).
"""
import json
import os

import numpy as np

import mlp_reference as R

U = 2.0 ** -24
SLAB_ROWS = 256  # f32_wgrad_slab_rows(B) for B <= 2^16 (csrc/mlp_f32.hip)
FLOOR = 1e-35
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ULPS = json.load(open(os.path.join(REPO, "profiles", "act_f32_ulps.json")))["activations"]
_NAMES = {a.lower(): a for a in R.ACTIVATIONS}
L_PHI = {"exponential": 1.0, "sigmoid": 1.0, "tanh": 2.0, "squareplus": 6.5, "softplus": 10.0}
BRANCHY = ("relu", "leakyrelu")


def _act_terms(name):
    """(c_forward, c_factor, pre-activation range) of a smooth activation, None for the exact ones"""
    k = name.lower()
    if k in ("none", "relu", "leakyrelu"):
        return None
    e = ULPS[_NAMES[k]]
    return e["forward"], e["factor"], e["range"]


def lipschitz(name, y, ez):
    k = name.lower()
    if k == "sigmoid":
        return np.full_like(y, 0.25)
    if k == "exponential":
        return y * np.exp(ez)
    return np.ones_like(y)


def shapes(W, IN, NH, OUTP):
    return [(OUTP, IN)] if NH == 0 else [(W, IN)] + [(W, W)] * (NH - 1) + [(OUTP, W)]


def split(W, IN, NH, OUTP, params):
    """flat parameters -> matrices (the dtype is kept)"""
    mats, off = [], 0
    for r, c in shapes(W, IN, NH, OUTP):
        mats.append(params[off:off + r * c].reshape(r, c))
        off += r * c
    assert off == params.size
    return mats


def reference(W, IN, NH, OUTP, act, out_act, params, x, dout, e_x=None):
    """float64 truth and bounds for fp32 parameters params [n], rows x [B][IN] (the encoded rows the first layer
    reads; e_x bounds their own error), dL/dy dout [B][OUTP]. Returns mlp_reference's dict plus
      mag_fwd [m_0 .. m_{NH+1}], z [pre-activations per layer],
      e_out [B][OUTP], e_hidden [per hidden layer], e_w [per matrix], e_in [B][IN]: the bounds."""
    mats = [m.astype(np.float64) for m in split(W, IN, NH, OUTP, np.asarray(params))]
    x, dout = np.asarray(x, np.float64), np.asarray(dout, np.float64)
    B = x.shape[0]
    ref = R.mlp_reference(W, IN, NH, OUTP, act, out_act, None, None, None, exact=True, mats=mats, x=x, dout=dout)
    names = [act] * NH + [out_act]
    acts = [x] + ref["hidden"] + [ref["out"]]
    e = np.zeros_like(x) if e_x is None else np.asarray(e_x, np.float64)
    errs, mags, zs = [e], [np.abs(x)], []
    for k in range(NH + 1):
        Mk, a, y = mats[k], acts[k], acts[k + 1]
        A = np.abs(Mk).T
        z = a @ Mk.T
        ez = e @ A + Mk.shape[1] * U * ((np.abs(a) + e) @ A) + FLOOR
        Lf = lipschitz(names[k], y, ez)
        e = Lf * ez
        t = _act_terms(names[k])
        if t is not None:
            assert z.min() >= t[2][0] and z.max() <= t[2][1], (names[k], z.min(), z.max(), "outside the measured range")
            e = e + 2 * t[0] * U * np.maximum(np.abs(y) + Lf * ez, 1.0)
        elif names[k].lower() == "leakyrelu":
            e = e + U * np.abs(y)
        mags.append(y if names[k].lower() == "exponential" else (0.25 if names[k].lower() == "sigmoid" else 1.0) * (mags[-1] @ A))
        errs.append(e)
        zs.append(z)
    ref.update(mag_fwd=mags, z=zs, e_out=errs[-1], e_hidden=errs[1:-1])

    n_slabs = (B + SLAB_ROWS - 1) // SLAB_ROWS
    g, eg = dout, np.zeros_like(dout)
    e_w = [None] * (NH + 1)
    for k in range(NH, -1, -1):
        y, ey, name = acts[k + 1], errs[k + 1], names[k]
        kk = name.lower()
        if kk == "none":
            d, ed = g, eg
        elif kk in BRANCHY:
            phi = R.act_factor(name, y)
            d, ed = g * phi, eg * phi + (U * np.abs(g * phi) if kk == "leakyrelu" else 0.0)
        else:
            phi = np.abs(R.act_factor(name, y))
            ephi = L_PHI[kk] * ey + 2 * _act_terms(name)[1] * U * np.maximum(phi, 1.0)
            d = g * R.act_factor(name, y)
            ed = eg * phi + (np.abs(g) + eg) * ephi + U * (np.abs(g) + eg) * (phi + ephi)
        a, ea = acts[k], errs[k]
        da, aa = np.abs(d) + ed, np.abs(a) + ea
        e_w[k] = ed.T @ aa + np.abs(d).T @ ea + (SLAB_ROWS + n_slabs) * U * (da.T @ aa) + FLOOR
        A = np.abs(mats[k])
        g, eg = d @ mats[k], ed @ A + mats[k].shape[0] * U * (da @ A) + FLOOR
    ref.update(e_w=e_w, e_in=eg)
    assert np.allclose(g, ref["dinput"], rtol=1e-12, atol=1e-300)
    return ref


def clear_of_branches(W, IN, NH, OUTP, act, out_act, params, x, tau=2.0 ** -14):
    """rows of x none of whose ReLU / LeakyReLU pre-activations is within tau of its terms' magnitude of zero
    (a chain of K <= 256 fp32 terms errs by 2^-16 of that magnitude at most, layer on layer: tau = 2^-14 leaves the
    computed sign the true one)"""
    mats = [m.astype(np.float64) for m in split(W, IN, NH, OUTP, np.asarray(params))]
    a = np.asarray(x, np.float64)
    ok = np.ones(a.shape[0], bool)
    for k, name in enumerate([act] * NH + [out_act]):
        z = a @ mats[k].T
        if name.lower() in BRANCHY:
            ok &= (np.abs(z) > tau * (np.abs(a) @ np.abs(mats[k]).T)).all(axis=1)
        a = R.act_forward(name, z)
    return ok


def check(ref, out, wgrad_flat, dinput, NH, label=""):
    """every element of the output, of every matrix's gradient and of dL/dinput within its bound; returns the
    worst ratio per quantity ({"out", matrix names.., "dinput"}); a miss names the quantity"""
    ratios = {}

    def one(name, got, want, bound):
        q = np.abs(np.asarray(got, np.float64) - want) / bound
        q = np.where(np.isnan(q), np.inf, q)
        j = int(np.argmax(q))
        ratios[name] = float(q.flat[j])
        assert q.flat[j] <= 1.0, (label, name, float(q.flat[j]), j, float(np.asarray(got).flat[j]), float(want.flat[j]))

    if out is not None:
        one("out", out, ref["out"], ref["e_out"])
    if wgrad_flat is not None:
        off = 0
        for name, w, ew in zip(R.matrix_names(NH), ref["wgrad"], ref["e_w"]):
            one(name, np.asarray(wgrad_flat)[off:off + w.size].reshape(w.shape), w, ew)
            # per matrix: the Frobenius norm of the error within that of the bound
            err = np.linalg.norm(np.asarray(wgrad_flat, np.float64)[off:off + w.size] - w.ravel())
            assert err <= np.linalg.norm(ew), (label, name, "matrix norm", err, np.linalg.norm(ew))
            off += w.size
        assert off == np.asarray(wgrad_flat).size
    if dinput is not None:
        one("dinput", dinput, ref["dinput"], ref["e_in"])
    return ratios


# ---- a numpy float32 evaluation: the arithmetic of the kernels (fp32 everywhere, fp32 sums, slabs) ----
def _act32(name, z):
    k, t = name.lower(), np.float32(R.K_ACT)
    if k == "none":
        return z
    if k == "relu":
        return np.maximum(z, np.float32(0))
    if k == "leakyrelu":
        return z * np.where(z > 0, np.float32(1), np.float32(0.01))
    if k == "exponential":
        return np.exp(z)
    if k == "sigmoid":
        return np.float32(1) / (np.float32(1) + np.exp(-z))
    if k == "squareplus":
        y = z * t
        return np.float32(0.5) * (y + np.sqrt(y * y + np.float32(4))) / t
    if k == "softplus":
        return np.log(np.exp(z * t) + np.float32(1)) / t
    return np.tanh(z)


def _factor32(name, y):
    k, t = name.lower(), np.float32(R.K_ACT)
    if k == "none":
        return np.ones_like(y)
    if k == "relu":
        return (y > 0).astype(np.float32)
    if k == "leakyrelu":
        return np.where(y > 0, np.float32(1), np.float32(0.01))
    if k == "exponential":
        return y
    if k == "sigmoid":
        return y * (np.float32(1) - y)
    if k == "squareplus":
        s = y * t
        return s * s / (s * s + np.float32(1))
    if k == "softplus":
        return np.float32(1) - np.exp(-y * t)
    return np.float32(1) - y * y


def eval_f32(W, IN, NH, OUTP, act, out_act, params, x, dout, perturb_hidden=None):
    """(out, hidden, flat wgrad, dinput) in float32 arithmetic. perturb_hidden(list of hidden arrays): edits the
    stored hidden activations before anything reads them (the CPU test's fp16-rounding probe)."""
    f = np.float32
    mats = split(W, IN, NH, OUTP, np.asarray(params, f))
    names = [act] * NH + [out_act]
    acts = [np.asarray(x, f)]
    for k in range(NH + 1):
        acts.append(_act32(names[k], (acts[k] @ mats[k].T).astype(f)).astype(f))
        if perturb_hidden is not None and k + 1 == NH and NH > 0:
            perturb_hidden(acts[1:])
    g = np.asarray(dout, f)
    wg = [None] * (NH + 1)
    B = g.shape[0]
    for k in range(NH, -1, -1):
        d = (g * _factor32(names[k], acts[k + 1])).astype(f) if names[k].lower() != "none" else g
        slabs = [d[b:b + SLAB_ROWS].T @ acts[k][b:b + SLAB_ROWS] for b in range(0, B, SLAB_ROWS)]
        s = slabs[0].astype(f)
        for t in slabs[1:]:
            s = (s + t).astype(f)
        wg[k] = s
        g = (d @ mats[k]).astype(f)
    return acts[-1], acts[1:-1], np.concatenate([w.ravel() for w in wg]), g


# ---- the cases (tests/test_gpu_mlp_f32.py's table): the smallest shapes that reach every path ----
class Case:
    def __init__(self, name, W, NH, n_in=16, n_out=3, act="ReLU", out_act="None", enc=None, otype="CutlassMLP", scale=1.5):
        self.name, self.W, self.NH, self.n_in, self.n_out, self.act, self.out_act, self.enc = name, W, NH, n_in, n_out, act, out_act, enc
        self.OUTP = (n_out + 15) // 16 * 16
        if enc is None:
            self.IN = (n_in + 15) // 16 * 16
        elif enc["otype"] == "OneBlob":
            self.IN = (n_in * enc["n_bins"] + 15) // 16 * 16
        else:
            self.IN = (enc["n_levels"] * enc["n_features_per_level"] + 15) // 16 * 16
        self.net = {"otype": otype, "activation": act, "output_activation": out_act, "n_neurons": W, "n_hidden_layers": NH}
        self.scale = scale
        self.n_mlp = sum(r * c for r, c in shapes(W, self.IN, NH, self.OUTP))
        self.id = f"{name}-{act}-{out_act}"

    def __repr__(self):
        return self.id


GRID2_L4 = {"otype": "HashGrid", "n_levels": 4, "n_features_per_level": 2, "log2_hashmap_size": 12, "base_resolution": 8,
            "per_level_scale": 1.5}  # test_gpu_composite.GRID2_L4 (the GPU test asserts the two are equal)
ONEBLOB4 = {"otype": "OneBlob", "n_bins": 4}


def _cases():
    c = []
    for act in ("ReLU", "None"):
        c.append(Case("w16h1", 16, 1, n_in=3, n_out=1, act=act, otype="FullyFusedMLP"))
        c.append(Case("w128h2", 128, 2, act=act, otype="FullyFusedMLP"))
        c.append(Case("w144h1", 144, 1, act=act))
        c.append(Case("h0", 64, 0, act=act, out_act=act))
        c.append(Case("oneblob-w32h2", 32, 2, n_in=2, act=act, enc=ONEBLOB4, otype="FullyFusedMLP"))
        c.append(Case("grid-w32h2", 32, 2, n_in=2, act=act, enc=GRID2_L4, otype="FullyFusedMLP"))
    for act in R.ACTIVATIONS:  # every activation, hidden and output, on W 48 (no multiple of 32) and W 64 (output padded to 32)
        s = 0.6 if act in ("Exponential",) else 1.5  # exp on exp, layer on layer: kept inside the measured range
        c.append(Case("w48h2", 48, 2, act=act, scale=s))
        c.append(Case("w64h3o17", 64, 3, n_out=17, act=act, scale=s, otype="FullyFusedMLP"))
        if act != "None":
            c.append(Case("w48h2", 48, 2, act="ReLU", out_act=act))
            c.append(Case("w64h3o17", 64, 3, n_out=17, act="None", out_act=act, scale=1.0, otype="FullyFusedMLP"))
    return c


CASES = _cases()
BATCHES = (256, 768)  # 768: three workgroup rows of 256 and three weight-gradient slabs


def case_params(case, grid_table=None):
    """fp32 parameters [network | grid table]: tcnn_module_initialize_params(seed 42) as
    module_matrix_cases.init_params32 restates it, the network part times the case's constant (float32
    multiply; NOT fp16-representable), a grid table uniform(-1, 1)"""
    import module_matrix_cases as M
    p = M.init_params32(case.W, case.IN, case.NH, case.OUTP)
    p = (p * np.float32(case.scale)).astype(np.float32)
    if case.enc is not None and case.enc["otype"] != "OneBlob":
        assert grid_table is not None
        p = np.concatenate([p, np.asarray(grid_table, np.float32)])
    return p


def case_inputs(case, B, seed=0):
    """2 B candidate rows (the caller keeps B clear of the branches), as module_matrix_cases.draw draws them:
    Identity inputs uniform [-1, 1], encoded positions uniform [0, 1); dL/dy uniform [-1, 1] on the n_out
    columns asked for and zero on the padding"""
    rng = np.random.default_rng(1000 + seed)
    if case.enc is None:
        x = rng.uniform(-1.0, 1.0, (2 * B, case.n_in)).astype(np.float32)
    else:
        x = rng.uniform(0.0, 1.0, (2 * B, case.n_in)).astype(np.float32)
    dout = np.zeros((B, case.OUTP), np.float32)
    dout[:, :case.n_out] = rng.uniform(-1.0, 1.0, (B, case.n_out)).astype(np.float32)
    return x, dout


def identity_rows(case, x):
    """the Identity encoding's rows: the inputs, then ones"""
    e = np.ones((x.shape[0], case.IN), np.float32)
    e[:, :case.n_in] = x
    return e


def keep_clear(case, params, x, enc_rows, B):
    ok = clear_of_branches(case.W, case.IN, case.NH, case.OUTP, case.act, case.out_act, params[:case.n_mlp], enc_rows)
    idx = np.flatnonzero(ok)[:B]
    assert idx.size == B, (case.id, int(ok.sum()), B)
    return np.ascontiguousarray(x[idx]), np.ascontiguousarray(enc_rows[idx])
