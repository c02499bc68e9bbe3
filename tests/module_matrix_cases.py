"""The Module forward/backward matrix: cases, inputs and the CPU side of every check, shared by
tests/test_mlp_reference.py (oracle against the float64 reference: the CPU proof of every bound and cap)
and tests/test_gpu_module_matrix.py (the HIP engines against the same reference, same assertions).

Inputs. Parameters are tcnn_module_initialize_params(seed 42)'s (here: the oracle's restatement of
that generator, bit-identical), the network part scaled by the case's constant SCALES[...] and a grid
table by GRID_SCALE, then rounded to fp16. The constant was chosen on the CPU (choose_scale
below is the rule) so that the last hidden pre-activation has a standard deviation near 1 and the output
pre-activations stay inside +-4: Exponential, Sigmoid and Tanh stay out of saturation and inside the fp16
range, and no output is ~1e-5 as with the plain initialisation (which would make the output check
vacuous). Identity inputs are fp16-exact uniform [-1, 1]; OneBlob / grid positions are uniform [0, 1)
(the encoded rows, fp16 by construction, are what the network sees); dL/dy is fp16-exact uniform [-1, 1]
on the n_output_dims columns the caller asked for and ZERO on the padded columns: the reference's
cpp_api.cu:96-108 hands the whole padded dL/doutput matrix to the network's backward, so the padded
columns are part of the contract, not ignored (the torch binding's slice feeds them zeros).

Branchy activations (ReLU, LeakyReLU; hidden or output) get their per-element check on B samples clear of
the branch (helpers.relu_margin_ok, tau = 2^-11) out of at most 16 B candidates; the aggregate check runs
on the first B candidates, unfiltered.
"""
import ctypes

import numpy as np

import mlp_reference as R
from helpers import relu_margin_ok
from oracle import oracle as O

SEED = 42
GRID = {"otype": "HashGrid", "n_levels": 16, "n_features_per_level": 2, "log2_hashmap_size": 8, "base_resolution": 16,
        "per_level_scale": 1.5}
GRID_SCALE = 1.0e4  # the +-1e-4 initial table becomes uniform [-1, 1]
OUT_ACTS = ["Sigmoid", "Exponential", "Tanh", "Softplus", "LeakyReLU", "Squareplus", "ReLU"]
BRANCHY = ("relu", "leakyrelu")
FUSED_SHAPES = [(64, 2), (64, 1), (32, 2), (32, 1)]  # TCNN_FUSED_SHAPES, IN = 32
GRID_ENCS = {"grid": 2, "grid3": 3}  # the GRID encoding on two / three input dimensions


class Case:
    def __init__(self, group, enc, W, NH, act="ReLU", out_act="None", otype="FullyFusedMLP", n_out=3, B=256, nodx="tile", dx="tile",
                 uneven=False):
        self.group, self.enc, self.W, self.NH, self.act, self.out_act, self.otype = group, enc, W, NH, act, out_act, otype
        self.n_out, self.B, self.kernel_nodx, self.kernel_dx, self.uneven = n_out, B, nodx, dx, uneven
        self.OUTP = (n_out + 15) // 16 * 16
        if enc == "identity":  # tcnn_create_network: Identity over 16 inputs
            self.n_in, self.IN, self.enc_cfg = 16, 16, None
        elif enc == "identity5":  # 5 inputs, 11 padding columns of ones
            self.n_in, self.IN, self.enc_cfg = 5, 16, None
        elif enc in GRID_ENCS:
            self.n_in, self.IN, self.enc_cfg = GRID_ENCS[enc], 32, GRID
        else:  # "oneblob16" / "oneblob64" on two dimensions
            nb = int(enc[len("oneblob"):])
            self.n_in, self.IN, self.enc_cfg = 2, 2 * nb, {"otype": "OneBlob", "n_bins": nb}
        self.net = {"otype": otype, "activation": act, "output_activation": out_act, "n_neurons": W, "n_hidden_layers": NH}
        self.id = f"{group}-{enc}-{otype[0]}-w{W}h{NH}-{act}-{out_act}-o{n_out}" + ("-uneven" if uneven else "")
        self.scale_key = f"{enc}-w{W}h{NH}-{act}-o{self.OUTP}"
        self.branchy = act.lower() in BRANCHY or out_act.lower() in BRANCHY
        self.n_mlp = O.mlp_n_params(W, self.IN, NH, self.OUTP)
        self.act_code = O.act_code(act) | (O.act_code(out_act) << 8)

    @property
    def scale(self):
        return SCALES[self.scale_key]

    def __repr__(self):
        return self.id


def _cases():
    c = []
    for W, NH in FUSED_SHAPES:  # register kernel without dL/dinput, tile kernel with it
        for act in ("None", "ReLU"):
            c.append(Case("register", "grid", W, NH, act, nodx="register", dx="tile"))
    for W, NH in ((64, 2), (32, 1)):  # the D = 3 instantiations of the register kernel
        for act in ("None", "ReLU"):
            c.append(Case("register", "grid3", W, NH, act, nodx="register", dx="tile"))
    for W, NHs in ((16, (1, 3)), (32, (2, 5)), (64, (3,)), (128, (1, 4))):
        for NH in NHs:
            for enc in ("identity", "oneblob16" if W <= 32 else "oneblob64"):
                for act in ("None", "ReLU"):
                    c.append(Case("tile", enc, W, NH, act))
    for act in ("None", "ReLU"):
        c.append(Case("tile", "oneblob64", 128, 5, act))  # hidden matrices streamed from L2
    for oa in OUT_ACTS:
        c.append(Case("tile", "identity", 32, 2, "None", oa))
        c.append(Case("tile", "oneblob64", 128, 1, "ReLU", oa))
    L = dict(nodx="layered", dx="layered")
    for W in (16, 48, 144, 256):
        for NH in (0, 1, 3):
            c.append(Case("layered", "identity", W, NH, "ReLU" if NH == 3 else "None", otype="CutlassMLP", **L))
    for act in R.ACTIVATIONS[1:]:  # None at W48/H1 is in the loop above
        c.append(Case("layered", "identity", 48, 1, act, otype="CutlassMLP", **L))
    for act, oa in (("Softplus", "Sigmoid"), ("Tanh", "Exponential"), ("Sigmoid", "Squareplus")):  # smooth x saturating
        c.append(Case("layered", "oneblob16", 48, 1, act, oa, otype="CutlassMLP", **L))
    c.append(Case("layered", "oneblob16", 64, 2, "Tanh", **L))  # FullyFusedMLP, non-ReLU hidden: the layered engine
    c.append(Case("layered", "identity", 64, 2, "LeakyReLU", "None", **L))
    for n_out in (1, 16, 17, 40):  # padded outputs 16, 16, 32, 48
        c.append(Case("layered", "identity", 48, 1, "None", otype="CutlassMLP", n_out=n_out, **L))
    return c


def uneven_cases(n_cu):
    """B = 256 (n_cu + 1): every persistent plan gives some workgroups one tile more than the rest, and
    launch_wgrad a ragged last chunk. hidden None: per element; ReLU: aggregate."""
    B = 256 * (n_cu + 1)
    c = []
    for act in ("None", "ReLU"):
        c.append(Case("uneven", "grid", 64, 2, act, B=B, nodx="register", dx="tile", uneven=True))
        c.append(Case("uneven", "identity", 64, 3, act, B=B, uneven=True))
        c.append(Case("uneven", "identity", 128, 4, act, B=B, uneven=True))
        c.append(Case("uneven", "identity", 144, 1, act, otype="CutlassMLP", B=B, nodx="layered", dx="layered", uneven=True))
    return c


def torch_cases():
    """the torch front end: tcnn.Network(5, 3) and tcnn.NetworkWithInputEncoding(2, 3, OneBlob 16), at a batch
    Module.forward pads (300 -> 512) and one it does not"""
    c = []
    for B in (300, 256):
        c.append(Case("torch", "identity5", 64, 2, "ReLU", B=B))
        c.append(Case("torch", "oneblob16", 32, 2, "None", B=B))
    return c


def graph_case(name, B=256):
    """the networks of tests/test_gpu_torch_graphs.py (multi-call autograd graphs on the torch front end), at
    batch size B: T OneBlob 16 + W32/H2 (tile kernel), I 5 inputs + W64/H2 ReLU (tile, branchy), G grid + W64/H2
    (register kernel without dL/dinput, tile with it), L 16 inputs + W48/H1 CutlassMLP (layered)"""
    if name == "T":
        return Case("graph", "oneblob16", 32, 2, "None", B=B)
    if name == "I":
        return Case("graph", "identity5", 64, 2, "ReLU", B=B)
    if name == "G":
        return Case("graph", "grid", 64, 2, "None", B=B, nodx="register", dx="tile")
    assert name == "L", name
    return Case("graph", "identity", 48, 1, "None", otype="CutlassMLP", B=B, nodx="layered", dx="layered")


def graph_id(name, want_dx):
    return graph_case(name).id + ("-dx" if want_dx else "-nodx")


# B.1 of test_gpu_torch_graphs.py: (network, dL/dx requested); two calls each, B = 256 (seed 0) and 300 (seed 1)
GRAPH_TWICE = [("T", True), ("G", True), ("G", False), ("L", True), ("I", True)]
GRAPH_TWICE_B = (256, 300)

CASES = _cases()
N_CU_CPU = 256  # the MI355X's compute units: the batch the CPU proof runs the uneven cases at
ALL_CPU_CASES = CASES + uneven_cases(N_CU_CPU) + torch_cases()

# per-case parameter constants (key: Case.scale_key), chosen by choose_scale below and recorded here;
# test_mlp_reference.py::test_scales_keep_outputs_in_range holds every entry to the rule
SCALES = {
    "grid-w64h2-None-o16": 1.3,
    "grid-w64h2-ReLU-o16": 1.6,
    "grid-w64h1-None-o16": 1.6,
    "grid-w64h1-ReLU-o16": 1.7,
    "grid-w32h2-None-o16": 1.2,
    "grid-w32h2-ReLU-o16": 1.5,
    "grid-w32h1-None-o16": 1.4,
    "grid-w32h1-ReLU-o16": 1.6,
    "grid3-w64h2-None-o16": 1.4,
    "grid3-w64h2-ReLU-o16": 1.6,
    "grid3-w32h1-None-o16": 1.6,
    "grid3-w32h1-ReLU-o16": 1.8,
    "identity-w16h1-None-o16": 1.2,
    "identity-w16h1-ReLU-o16": 1.6,
    "oneblob16-w16h1-None-o16": 2.1,
    "oneblob16-w16h1-ReLU-o16": 2.7,
    "identity-w16h3-None-o16": 1.2,
    "identity-w16h3-ReLU-o16": 1.4,
    "oneblob16-w16h3-None-o16": 1.3,
    "oneblob16-w16h3-ReLU-o16": 2.0,
    "identity-w32h2-None-o16": 1.1,
    "identity-w32h2-ReLU-o16": 1.5,
    "oneblob16-w32h2-None-o16": 1.6,
    "oneblob16-w32h2-ReLU-o16": 2.0,
    "identity-w32h5-None-o16": 1.1,
    "identity-w32h5-ReLU-o16": 1.5,
    "oneblob16-w32h5-None-o16": 1.3,
    "oneblob16-w32h5-ReLU-o16": 1.6,
    "identity-w64h3-None-o16": 1.2,
    "identity-w64h3-ReLU-o16": 1.6,
    "oneblob64-w64h3-None-o16": 1.4,
    "oneblob64-w64h3-ReLU-o16": 1.9,
    "identity-w128h1-None-o16": 1.5,
    "identity-w128h1-ReLU-o16": 2.0,
    "oneblob64-w128h1-None-o16": 2.3,
    "oneblob64-w128h1-ReLU-o16": 2.7,
    "identity-w128h4-None-o16": 1.2,
    "identity-w128h4-ReLU-o16": 1.6,
    "oneblob64-w128h4-None-o16": 1.3,
    "oneblob64-w128h4-ReLU-o16": 1.7,
    "oneblob64-w128h5-None-o16": 1.2,
    "oneblob64-w128h5-ReLU-o16": 1.8,
    "identity-w16h0-None-o16": 1.7,
    "identity-w48h0-None-o16": 1.7,
    "identity-w48h1-None-o16": 1.3,
    "identity-w48h3-ReLU-o16": 1.5,
    "identity-w144h0-None-o16": 1.7,
    "identity-w144h1-None-o16": 1.7,
    "identity-w144h3-ReLU-o16": 1.7,
    "identity-w256h0-None-o16": 1.7,
    "identity-w256h1-None-o16": 2.0,
    "identity-w256h3-ReLU-o16": 1.8,
    "identity-w48h1-ReLU-o16": 1.4,
    "identity-w48h1-LeakyReLU-o16": 1.5,
    "identity-w48h1-Exponential-o16": 0.82,
    "identity-w48h1-Sigmoid-o16": 1.9,
    "identity-w48h1-Squareplus-o16": 1.4,
    "identity-w48h1-Softplus-o16": 1.4,
    "identity-w48h1-Tanh-o16": 1.7,
    "oneblob16-w48h1-Softplus-o16": 2.6,
    "oneblob16-w48h1-Tanh-o16": 2.4,
    "oneblob16-w48h1-Sigmoid-o16": 1.8,
    "oneblob16-w64h2-Tanh-o16": 2.0,
    "identity-w64h2-LeakyReLU-o16": 1.5,
    "identity-w48h1-None-o32": 1.4,
    "identity-w48h1-None-o48": 1.5,
    "identity-w144h1-ReLU-o16": 1.8,
    "identity5-w64h2-ReLU-o16": 1.4,
}


# Unfiltered batches whose first draw (seed 0) holds a ReLU tie that fp32 and float64 sums resolve differently
# -- the fp32 CPU oracle itself then misses the aggregate bar against float64 (test_mlp_reference.py: 9.7e-3
# against 2e-3 for this case, a last-hidden-layer pre-activation 8.5e-7 of its terms' magnitude away from
# zero) -- draw with the next seed instead. The bar stays. The same network at B = 256 (n_cu + 1) (uneven W128/H4
# ReLU) shows the mechanism at a smaller size: 1.39e-3 on the MI355X and 1.30e-3 for the fp32 oracle against the
# same 2e-3 bar, the least headroom of the matrix (every other aggregate figure is ~2e-4, the fp16 rounding).
AGG_SEEDS = {"tile-identity-F-w128h4-ReLU-None-o3": 1}


# ---- parameters and inputs ----
def host_params32(case, seed=SEED):
    """tcnn_module_initialize_params(seed) restated with the oracle's generators: pcg32{seed}, Xavier
    uniform per matrix in layout order, then the grid table uniform +-1e-4 (float32 [network | grid])"""
    return init_params32(case.W, case.IN, case.NH, case.OUTP, GRID if case.enc in GRID_ENCS else None, seed,
                         n_dims=GRID_ENCS.get(case.enc, 2))


def init_params32(W, IN, NH, OUTP, grid=None, seed=SEED, n_dims=2):
    """host_params32 for any network; grid: the grid encoding's config (on n_dims input dimensions) or None"""
    rng = O.pcg32(seed)
    shapes = [(OUTP, IN)] if NH == 0 else [(W, IN)] + [(W, W)] * (NH - 1) + [(OUTP, W)]
    parts = []
    for r, cc in shapes:
        m = np.empty(r * cc, np.float32)
        O.lib().orc_xavier_uniform(ctypes.byref(rng), r, cc, m.ctypes.data_as(ctypes.c_void_p), 1.0)
        parts.append(m)
    if grid is not None:
        parts.append(O.generate_uniform(rng, O.grid_cfg(grid, n_dims).n_params, -1e-4, 1e-4))
    return np.concatenate(parts)


def scale_params16(case, p32, scale=None):
    """fp16 bits of the scaled parameters (float32 multiply, then one rounding: what the GPU test does
    with torch on the device's float32 copy)"""
    p = np.array(p32, np.float32)
    p[:case.n_mlp] *= np.float32(case.scale if scale is None else scale)
    p[case.n_mlp:] *= np.float32(GRID_SCALE)
    return O.f2h(p)


def encode(case, params16, x):
    """the encoded rows [B][IN] (fp16 bits) the network sees, with the oracle's encoders"""
    if case.enc.startswith("identity"):
        return O.identity_fwd(x, n_pad=case.IN - case.n_in)
    if case.enc in GRID_ENCS:
        return np.ascontiguousarray(O.grid_fwd(O.grid_cfg(GRID, case.n_in), x, params16[case.n_mlp:]).T)
    return O.oneblob_fwd(x, case.enc_cfg["n_bins"])


def draw(case, params16, filtered, seed=0):
    """(x float32 [B][n_in], encoded fp16 bits [B][IN], dout fp16 bits [B][OUTP]). filtered: B samples clear
    of every branch out of 16 B candidates (asserts the cap is met); else the first B candidates."""
    B, n = case.B, case.B * (16 if filtered else 1)
    rng = np.random.default_rng(1000 + seed + (0 if filtered else AGG_SEEDS.get(case.id, 0)))
    if case.enc.startswith("identity"):
        x = O.h2f(O.f2h(rng.uniform(-1.0, 1.0, (n, case.n_in)).astype(np.float32)))
    else:
        x = rng.uniform(0.0, 1.0, (n, case.n_in)).astype(np.float32)
    dout = np.zeros((B, case.OUTP), np.uint16)
    dout[:, :case.n_out] = O.f2h(rng.uniform(-1.0, 1.0, (B, case.n_out)).astype(np.float32))
    enc = encode(case, params16, x)
    if filtered:
        ok = relu_margin_ok(case.W, case.IN, case.NH, params16[:case.n_mlp], O.h2f(enc), act=case.act,
                            out_rows=case.OUTP if case.out_act.lower() in BRANCHY else 0)
        idx = np.flatnonzero(ok)[:B]
        assert idx.size == B, (case.id, int(ok.sum()), B)
        x, enc = np.ascontiguousarray(x[idx]), np.ascontiguousarray(enc[idx])
    return x, enc, dout


def encoded_dims(cfg):
    """(IN, n_mlp, grid cfg or None) of a two-input config {"encoding": grid or OneBlob, "network": ..}, 16 padded outputs"""
    enc, net = cfg["encoding"], cfg["network"]
    g = None if enc["otype"] == "OneBlob" else O.grid_cfg(enc, 2)
    IN = 2 * enc["n_bins"] if g is None else g.n_levels * g.n_features_per_level
    return IN, O.mlp_n_params(net["n_neurons"], IN, net["n_hidden_layers"], 16), g


def relu_clear_positions(cfg, params16, B, seed):
    """(positions [B][2], encoded fp16 bits [B][IN]) of a two-input ReLU config: the first B of
    helpers.make_batch(16 B, seed)'s positions clear of every hidden ReLU boundary (helpers.relu_margin_ok,
    tau = 2^-11) at params16; asserts that B survive."""
    from helpers import make_batch
    net = cfg["network"]
    assert net["activation"] == "ReLU" and net["output_activation"] == "None"
    IN, nm, g = encoded_dims(cfg)
    pos = make_batch(16 * B, seed=seed)[0]
    if g is None:
        enc = O.oneblob_fwd(pos, cfg["encoding"]["n_bins"])
    else:
        enc = np.ascontiguousarray(O.grid_fwd(g, pos, params16[nm:]).T)
    ok = relu_margin_ok(net["n_neurons"], IN, net["n_hidden_layers"], params16[:nm], O.h2f(enc))
    idx = np.flatnonzero(ok)[:B]
    assert idx.size == B, (int(ok.sum()), B)
    return np.ascontiguousarray(pos[idx]), np.ascontiguousarray(enc[idx])


def context_reuse_inputs(cfg, params16, B=1024):
    """The first batch and dL/dy of test_gpu_tile_engine.py::test_module_forward_context_reused_by_backward:
    (positions, encoded fp16 bits, dL/dy fp16 bits [B][16]); ReLU-clear positions, since its gradient is
    checked per element."""
    pos, enc = relu_clear_positions(cfg, params16, B, seed=11)
    dout = np.zeros((B, 16), np.float32)
    dout[:, :3] = np.random.default_rng(0).standard_normal((B, 3)) * 0.05
    return pos, enc, O.f2h(dout)


def reference(case, params16, enc16, dout16):
    return R.mlp_reference(case.W, case.IN, case.NH, case.OUTP, case.act, case.out_act, params16[:case.n_mlp], enc16, dout16)


def torch_reference(case, params16, enc16, dout16, loss_scale):
    """reference() as the torch binding computes it: the binding multiplies dL/dy by its loss scale (128, exact
    in fp16 for |dL/dy| <= 1) and divides the gradients by it, so the reference runs on loss_scale * dL/dy and
    its gradients and magnitudes are divided by loss_scale (powers of two commute with every rounding above
    the subnormals; the bounds' 2^-25 covers those)."""
    s = float(loss_scale)
    dout_s = np.array(dout16, np.uint16)
    dout_s[:, :case.n_out] = O.f2h(O.h2f(dout_s[:, :case.n_out]) * np.float32(s))
    ref = reference(case, params16, enc16, dout_s)
    for k in ("wgrad", "mag_w"):
        ref[k] = [m / s for m in ref[k]]
    ref["dinput"], ref["mag_in"] = ref["dinput"] / s, ref["mag_in"] / s
    return ref


def oracle_run(case, params16, enc16, dout16, n_threads=4):
    """the fp32 CPU oracle on the same rows: (out, flat weight gradient, dL/d(encoding)) as float64"""
    p = params16[:case.n_mlp]
    W, IN, NH, OUTP, a = case.W, case.IN, case.NH, case.OUTP, case.act_code
    out16, hidden = O.mlp_fwd(W, IN, NH, OUTP, p, enc16, input_soa=False, activation=a, n_threads=n_threads)
    g16 = O.act_bwd_output(a, out16, dout16.copy())
    wg, din = O.mlp_bwd(W, IN, NH, OUTP, p, enc16, hidden, g16, input_soa=False, activation=a, n_threads=n_threads)
    return O.h2f(out16).astype(np.float64), wg.astype(np.float64), O.h2f(din).astype(np.float64)


def check_against_reference(case, ref, out, wgrad_flat, denc, per_element, fp16_out):
    """The assertions both the oracle (CPU) and the HIP engines (GPU) get; fp16_out (the gradient a Module
    returns is fp16) adds that rounding to the per-element bound only, the aggregate bars are the same. Returns the ratios:
    {matrix: worst per-element ratio, "dinput": ..} for a per-element run, {"agg_w", "agg_in"} otherwise."""
    R.check_output(out[:, :case.n_out], ref["out"][:, :case.n_out])
    if per_element:
        ratios = R.check_wgrad(wgrad_flat, ref, fp16_out=fp16_out)
        if denc is not None:
            ratios["dinput"] = R.check_dinput(denc, ref["dinput"], ref["mag_in"])
        if not case.branchy:  # every sample is in the batch: the aggregate bar applies to the same run (a dropped
            # tile at a large batch, or swapped columns of a deep linear network, hide inside the per-element bound)
            ratios["agg_w"], ratios["agg_in"] = R.check_aggregate(wgrad_flat, ref, R.aggregate_bar(case.W, case.NH, case.out_act), denc)
        return ratios
    ew, ei = R.check_aggregate(wgrad_flat, ref, R.aggregate_bar(case.W, case.NH, case.out_act), denc)
    return {"agg_w": ew, "agg_in": ei}


def oneblob_jacobian(case, x):
    """|d enc_j / d x_d| [B][IN][D] of the OneBlob encoder, from its linear backward on one-hot rows"""
    nb = case.enc_cfg["n_bins"]
    J = np.empty((x.shape[0], case.IN, 2))
    for j in range(case.IN):
        e = np.zeros((x.shape[0], case.IN), np.float32)
        e[:, j] = 1.0
        J[:, j, :] = O.oneblob_bwd(x, nb, O.f2h(e))
    return np.abs(J)


def preactivation_stats(case, p16):
    """(standard deviation of the last hidden layer's pre-activations, max |output pre-activation|) on the
    case's unfiltered inputs, float64 sums over the fp16 hidden values"""
    _, enc, _ = draw(case, p16, filtered=False)
    mats = R.split_params(case.W, case.IN, case.NH, case.OUTP, p16[:case.n_mlp])
    a, sd = O.h2f(enc).astype(np.float64), 0.0
    for k in range(case.NH):
        z = a @ mats[k].T
        sd = z.std()
        a = R.f64_to_f16(R.act_forward(case.act, z))
    return sd, np.abs(a @ mats[case.NH].T).max()


def choose_scale(case, seed=SEED):
    """The rule behind SCALES: the largest constant (two significant digits) for which the last hidden
    pre-activation's standard deviation is <= 1 and every output pre-activation is inside +-4, on the
    case's unfiltered inputs (test_mlp_reference.py::test_scales_keep_outputs_in_range pins the table to it)."""
    p32 = host_params32(case, seed)
    lo, hi = 0.05, 64.0
    for _ in range(40):
        mid = (lo * hi) ** 0.5
        sd, mx = preactivation_stats(case, scale_params16(case, p32, mid))
        if sd <= 1.0 and mx <= 4.0 and np.isfinite(mx):
            lo = mid
        else:
            hi = mid
    e = 10.0 ** (np.floor(np.log10(lo)) - 1)
    return float(f"{np.floor(lo / e) * e:.2g}")


RATIOS_HEADER = """\
# Module matrix (tests/test_gpu_module_matrix.py): worst ratio |got - float64 reference| / bound per matrix and for
# dL/dinput (per_element runs), relative L2 (aggregate runs: agg_w weight gradients, agg_in dL/dinput; grid_rel /
# dx_rel: the grid's own gradients). Each entry: MI355X / fp32 CPU oracle on the same inputs
# (tests/test_mlp_reference.py). Both test modules append JSON lines under TCNN_MATRIX_RATIOS=<file>;
# PYTHONPATH=. python tests/module_matrix_cases.py <gpu lines> <oracle lines> <this file> merges them.
"""


GRAPH_RATIOS_HEADER = """\
# Torch front end, multi-call autograd graphs (tests/test_gpu_torch_graphs.py): worst ratio |got - float64 reference|
# / bound per matrix and for dL/dinput, relative L2 for agg_* / *_rel (agg_w: the summed weight gradient, grid_rel /
# dx_rel: the grid's own gradients; g_rel / xgrad_rel / wgrad_rel / pgrad_rel: the eikonal pattern's). Kinds are
# graph-<test>-<node>. Each entry: MI355X / fp32 CPU oracle on the same inputs (tests/test_mlp_reference.py, the
# twice-in-one-graph cases only). Both test modules append JSON lines under TCNN_MATRIX_RATIOS=<file>;
# PYTHONPATH=. python tests/module_matrix_cases.py <gpu lines> <oracle lines> <this file> graph merges them.
"""


def merge_ratios(gpu_path, oracle_path, out_path, header=None):
    """profiles/module_matrix_ratios.txt (profiles/torch_graph_ratios.txt with header=GRAPH_RATIOS_HEADER) from
    the JSON lines the two test modules wrote: one line per GPU run, each figure next to the oracle's for the
    same case, batch size and kind (per_element / aggregate; graph-<test>, the GPU's kind without its last part)"""
    import json
    header = RATIOS_HEADER if header is None else header

    def lines(path):
        return [json.loads(ln) for ln in open(path) if ln.strip()]

    fmt = lambda v: "-" if v is None else f"{v:.3g}"  # noqa: E731
    oracle = {(e["case"], e["B"], e["kind"]): e["ratios"] for e in lines(oracle_path)}
    worst, out = [], [header]
    for e in lines(gpu_path):
        kind = e["kind"].split("-")[0]
        ref = oracle.get((e["case"], e["B"], e["kind"].rsplit("-", 1)[0]), oracle.get((e["case"], e["B"], kind), {}))
        cells = []
        for k, v in e["ratios"].items():
            cells.append(f"{k}={fmt(v)}/{fmt(ref.get(k))}")
            if kind in ("per_element", "graph") and v is not None and not (k.startswith("agg_") or k.endswith("_rel")):
                worst.append((v, f"{e['case']} [{e['kind']}] {k} {fmt(v)} (oracle {fmt(ref.get(k))})"))
        out.append(f"{e['case']} [{e['kind']}] " + " ".join(cells) + "\n")
    worst.sort(key=lambda t: -t[0])
    out.append("# largest per-element GPU ratios: " + "; ".join(t[1] for t in worst[:5]) + "\n")
    with open(out_path, "w") as f:
        f.writelines(out)


if __name__ == "__main__":
    import sys
    merge_ratios(*sys.argv[1:4], header=GRAPH_RATIOS_HEADER if sys.argv[4:5] == ["graph"] else None)
