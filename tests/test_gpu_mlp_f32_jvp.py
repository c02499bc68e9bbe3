"""GPU tests of tcnn_module_inference_jvp (csrc/mlp_f32_jvp.hip): the value and directional input derivatives of an fp32
FullyFusedMLP network module behind a lone grid, in one forward-mode launch, against float64.

Truth. de/dx [B][IN][D] in float64 comes from the corner walk of test_grid_f32_reference.level_corners (its entries and
its fraction, the single-rounded fmaf) by differentiating the weights: per level and dimension d,
scale pd_d sum over the 2^(D-1) edges along d of (prod_{e != d} a_e) (v_right - v_left), pd = 6 f (1 - f) from the exact
fraction f for Smoothstep and 1 for Linear. Row o of J is mlp_f32_reference's dL/d(encoded row) for a one-hot dL/dy at
the rows the module's own encoding writes (y must be tcnn_module_inference's bits), contracted with de/dx, and
Jv[o][k] = sum_d J[o][d] v[k][d].

Bound, from operation counts, per element, u = 2^-24, T[col][k] = sum_d |de_col/dx_d| |v_k[d]|:
  sum_col e_in[col] T[col][k]
      e_in is the reference's bound of dL/d(encoded row), derived for the same contractions in reverse order. Forward
      mode has K = W terms per hidden product where the reverse has N = W or OUTP, and its first layer sums IN terms
      where the reverse's last product sums W: IN <= W in every case here, so its count is not larger.
  + sum_col |dinput[col]| sum_d err[col][d] |v_k[d]|
      err is the fp32 error of de/dx (level_tangent_f32): with A = scale pd sum_edges (prod a) |v_right - v_left|, it is
      c u A with c = (D - 1) subtractions 1 - f, (D - 1) products from the scale on, 1 subtraction v_right - v_left,
      1 product with it, one FMA rounding per edge (2^(D-1)) against a partial sum that A bounds, and 1 for the second
      order: c = 2 (D - 1) + 2^(D-1) + 3. Smoothstep adds 3 u A for the three roundings of pd and, as
      test_grid_f32_reference.forward_bound argues for the value, (3 + 1) u E for the absolute error 3 u s_e of each
      polynomial value s_e inside the other dimensions' factors, E = scale pd sum_edges S |v_right - v_left| with
      S = sum_{e != d} s_e prod_{e' != d, e} a_e'.
  + D u sum_col |dinput[col]| T[col][k], with directions only: the D roundings of sum_d (de/dx_d) v[d], each against a
      partial sum that T bounds. The unit directions select one term and round nothing.

Inputs are kept clear of the ReLU branches (mlp_f32_reference.keep_clear) and at least 2^-10 of a cell away from every
cell boundary on every level, where the derivative jumps; the filter may reject a quarter of the candidates at most
(expected about 2 2^-10 L D, under 10 % here). Batches 128 and 384 are one and three pairs of the kernel's 64-row
workgroups.
"""
import functools

import numpy as np
import pytest

import mlp_f32_reference as F
import test_gpu_mlp_f32 as T
import test_gpu_mlp_f32_jacobian as JT
import test_grid_f32_reference as G
from oracle import oracle as O
from test_gpu_encoding_f32 import FP16, FP32, Mod, _vp

pytestmark = pytest.mark.gpu

GUARD, SENTINEL, U = JT.GUARD, JT.SENTINEL, 2.0 ** -24
DENSE2_F4 = {"otype": "DenseGrid", "n_levels": 8, "n_features_per_level": 4, "base_resolution": 4, "per_level_scale": 1.5,
             "interpolation": "Smoothstep"}
TILED3_F8 = {"otype": "TiledGrid", "n_levels": 8, "n_features_per_level": 8, "base_resolution": 4, "per_level_scale": 1.5,
             "hash": "CoherentPrime"}
HASH3_L16 = {"otype": "HashGrid", "n_levels": 16, "n_features_per_level": 2, "log2_hashmap_size": 12, "base_resolution": 8,
             "per_level_scale": 1.5}


def gc(name, W, NH, D, n_out, act, out_act, enc):
    return F.Case(name, W, NH, n_in=D, n_out=n_out, act=act, out_act=out_act, enc=enc, otype="FullyFusedMLP")


CASES = [gc("hash3-l4f2-w16h1", 16, 1, 3, 1, "ReLU", "None", F.GRID2_L4),  # dense and hashed levels, 8 padding columns
         gc("dense2-l8f4-smooth-w32h2", 32, 2, 2, 3, "Tanh", "None", DENSE2_F4),
         gc("tiled3-l8f8-w64h2o17", 64, 2, 3, 17, "Tanh", "Sigmoid", TILED3_F8),  # lanes share a level, two output tiles
         gc("hash3-l16f2-w128h2", 128, 2, 3, 1, "Tanh", "None", HASH3_L16)]
IDS = [c.id for c in CASES]


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


def fractions(g, l, x):
    p = (x.astype(np.float64) * np.float64(np.float32(g.scales[l])) + 0.5).astype(np.float32)  # one rounding == fmaf
    return (p - np.floor(p)).astype(np.float64)


def encoding_jacobian(g, x, table, IN):
    """(de/dx, its fp32 error bound), float64 [B][IN][D], zero on the padding columns"""
    B, D, L, Fe = x.shape[0], g.n_pos_dims, g.n_levels, g.n_features_per_level
    t = np.asarray(table, np.float64).reshape(-1, Fe)
    dE, err = np.zeros((B, IN, D)), np.zeros((B, IN, D))
    if g.interpolation == 0:
        return dE, err
    smooth = g.interpolation == 2
    c_units = 2 * (D - 1) + (1 << (D - 1)) + 3
    for l in range(L):
        idx, _, _ = G.level_corners(g, l, x)
        v, f, scale = t[idx], fractions(g, l, x), np.float64(np.float32(g.scales[l]))
        s = f * f * (3.0 - 2.0 * f) if smooth else f
        for d in range(D):
            pd = 6.0 * f[:, d] * (1.0 - f[:, d]) if smooth else np.ones(B)
            val, A, E = np.zeros((B, Fe)), np.zeros((B, Fe)), np.zeros((B, Fe))
            for c in (c for c in range(1 << D) if not c & (1 << d)):
                a = {e: (s[:, e] if c & (1 << e) else 1.0 - s[:, e]) for e in range(D) if e != d}
                w = np.prod(list(a.values()), axis=0) if a else np.ones(B)
                S = sum(s[:, e] * np.prod([a[k] for k in a if k != e], axis=0) for e in a) if smooth else 0.0
                diff = v[:, c | (1 << d)] - v[:, c]
                val += (w * scale * pd)[:, None] * diff
                A += (w * scale * pd)[:, None] * np.abs(diff)
                E += (S * scale * pd)[:, None] * np.abs(diff)
            dE[:, l * Fe:(l + 1) * Fe, d] = val
            err[:, l * Fe:(l + 1) * Fe, d] = U * ((c_units + (3 if smooth else 0)) * A + 4 * E)
    return dE, err


def clear_of_boundaries(g, x):
    ok = np.ones(x.shape[0], bool)
    for l in range(g.n_levels):
        f = fractions(g, l, x)
        ok &= np.all((f >= 2.0 ** -10) & (f <= 1 - 2.0 ** -10), axis=1)
    return ok


def truth(case, g, p, table, x, rows, v=None):
    """(Jv [B][n_out][K], its bound) in float64; v None: the unit directions, Jv = J"""
    B, D = x.shape
    dE, err = encoding_jacobian(g, x, table, case.IN)
    va = np.broadcast_to(np.eye(D), (B, D, D)) if v is None else np.abs(v.astype(np.float64))
    vv = np.broadcast_to(np.eye(D), (B, D, D)) if v is None else v.astype(np.float64)
    Tm = np.einsum("bcd,bkd->bck", np.abs(dE), va)
    Jv, Eb = np.empty((B, case.n_out, vv.shape[1])), np.empty((B, case.n_out, vv.shape[1]))
    for o in range(case.n_out):
        dout = np.zeros((B, case.OUTP), np.float32)
        dout[:, o] = 1.0
        ref = F.reference(case.W, case.IN, case.NH, case.OUTP, case.act, case.out_act, p[:case.n_mlp], rows, dout)
        di = ref["dinput"]
        Jv[:, o] = np.einsum("bc,bcd,bkd->bk", di, dE, vv)
        Eb[:, o] = (np.einsum("bc,bck->bk", ref["e_in"], Tm) + np.einsum("bc,bcd,bkd->bk", np.abs(di), err, va) +
                    (0.0 if v is None else D * U * np.einsum("bc,bck->bk", np.abs(di), Tm)) + F.FLOOR)
    return Jv, Eb


@functools.lru_cache(maxsize=None)
def setup(i, B):
    """inputs clear of the cell boundaries and of the ReLU branches, parameters and encoded rows of case i, once"""
    import torch
    case = CASES[i]
    g = O.grid_cfg(case.enc, case.n_in)
    table = np.random.default_rng(7).uniform(-1, 1, g.n_params).astype(np.float32)
    p = F.case_params(case, table)
    x4 = F.case_inputs(case, 2 * B)[0]
    ok = clear_of_boundaries(g, x4)
    assert ok.mean() >= 0.75, (case.id, "the boundary filter rejects", 1 - ok.mean())
    x2 = np.ascontiguousarray(x4[ok])
    x, rows = F.keep_clear(case, p, x2, T.encoded_rows(torch, case, x2, table), B)
    return g, table, p, x, rows


@functools.lru_cache(maxsize=None)
def unit_truth(i, B):
    g, table, p, x, rows = setup(i, B)
    return truth(CASES[i], g, p, table, x, rows)


def directions(x, K, seed=3):
    return np.random.default_rng(seed).uniform(-1, 1, (x.shape[0], K, x.shape[1])).astype(np.float32)


def call(torch, net, case, x, p, v=None, mask=0, fn="tcnn_module_inference_jvp"):
    """one call under a layout mask; (y [B][OUTP], or [B][n_out] under the output bit, Jv [B][n_out][K]), each result
    buffer exactly its size plus a guard that must come back untouched"""
    B, D, n = x.shape[0], case.n_in, case.n_out
    K = D if v is None else v.shape[1]
    xd = torch.from_numpy(np.ascontiguousarray(x.T if mask & 1 else x)).cuda()
    vd = None if v is None else torch.from_numpy(np.ascontiguousarray(v.transpose(1, 2, 0) if mask & 1 else v)).cuda()
    pd = torch.from_numpy(p).cuda()
    ny = n * B if mask & 2 else B * case.OUTP
    y = torch.full((ny + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    J = torch.full((B * n * K + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    if fn == "tcnn_module_inference_jvp":
        net.L.check(net.lib.tcnn_module_inference_jvp(net.h, None, B, _vp(xd), _vp(vd), 0 if v is None else K, _vp(y), _vp(J), _vp(pd), mask))
    else:
        net.L.check(net.lib.tcnn_module_inference_jacobian(net.h, None, B, _vp(xd), _vp(y), _vp(J), _vp(pd), mask))
    torch.cuda.synchronize()
    y, J = y.cpu().numpy(), J.cpu().numpy()
    assert np.all(y[ny:] == SENTINEL) and np.all(J[B * n * K:] == SENTINEL), "written past the unpadded size"
    assert not np.any(J[:B * n * K] == SENTINEL), "an element of the product was not written"
    if mask & 2:
        return y[:ny].reshape(n, B).T.copy(), J[:B * n * K].reshape(n, K, B).transpose(2, 0, 1).copy()
    return y[:ny].reshape(B, case.OUTP), J[:B * n * K].reshape(B, n, K)


def worst(label, got, want, bound):
    q = np.abs(got.astype(np.float64) - want) / bound
    q = np.where(np.isnan(q), np.inf, q)
    print(f"jvp-ratio {label} worst |Jv - truth| / bound = {q.max():.4f}")
    assert np.abs(want).max() > 0 and q.max() <= 1.0, (label, float(q.max()), np.unravel_index(int(np.argmax(q)), q.shape))


@pytest.mark.parametrize("B", [128, 384])
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_against_float64(torch_mod, i, B):
    case = CASES[i]
    _, _, p, x, _ = setup(i, B)
    Jt, Et = unit_truth(i, B)
    net = T.make_net(torch_mod, case)
    assert net.lib.tcnn_module_engine(net.h) == b"fused" and net.n_params == p.size
    y, J = call(torch_mod, net, case, x, p)
    want = JT.inference(net, x, p)
    net.close()
    worst(f"{case.id} B={B} unit", J, Jt, Et)
    np.testing.assert_array_equal(y.view(np.uint32), want.view(np.uint32))


def test_nearest_is_zero(torch_mod):
    case = gc("nearest", 32, 2, 3, 3, "Tanh", "None", dict(F.GRID2_L4, interpolation="Nearest"))
    g = O.grid_cfg(case.enc, 3)
    p = F.case_params(case, np.random.default_rng(7).uniform(-1, 1, g.n_params).astype(np.float32))
    x = F.case_inputs(case, 64)[0]
    net = T.make_net(torch_mod, case)
    y, J = call(torch_mod, net, case, x, p)
    want = JT.inference(net, x, p)
    net.close()
    assert np.all(J == 0) and np.abs(y).max() > 0
    np.testing.assert_array_equal(y.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("K", [1, 4])  # 4: two passes at three tangents per pass
@pytest.mark.parametrize("i", [0, 2], ids=[IDS[0], IDS[2]])
def test_directions(torch_mod, i, K):
    case = CASES[i]
    g, table, p, x, rows = setup(i, 128)
    v = directions(x, K)
    net = T.make_net(torch_mod, case)
    y, Jv = call(torch_mod, net, case, x, p, v)
    want = JT.inference(net, x, p)
    net.close()
    worst(f"{case.id} K={K}", Jv, *truth(case, g, p, table, x, rows, v))
    np.testing.assert_array_equal(y.view(np.uint32), want.view(np.uint32))


def test_soa_is_aos_transposed(torch_mod):
    case = CASES[0]
    _, _, p, x, _ = setup(0, 128)
    v = directions(x, 2)
    net = T.make_net(torch_mod, case)
    y0, J0 = call(torch_mod, net, case, x, p, v)
    for mask in (1, 2, 3):
        y, J = call(torch_mod, net, case, x, p, v, mask)
        np.testing.assert_array_equal(y.view(np.uint32), y0[:, :y.shape[1]].view(np.uint32), err_msg=f"y, mask {mask}")
        np.testing.assert_array_equal(J.view(np.uint32), J0.view(np.uint32), err_msg=f"Jv, mask {mask}")
    net.close()


def test_identity_front_matches_jacobian_call(torch_mod):
    i = JT.IDS.index("identity-w32h2-Tanh-Tanh")
    case = JT.CASES[i][0]
    x, p, _ = JT.setup(i, 128)
    net = JT.make(torch_mod, i)
    y, J = call(torch_mod, net, case, x, p)
    y0, J0 = call(torch_mod, net, case, x, p, fn="tcnn_module_inference_jacobian")
    net.close()
    np.testing.assert_array_equal(y.view(np.uint32), y0.view(np.uint32))
    np.testing.assert_array_equal(J.view(np.uint32), J0.view(np.uint32))


def test_torch_front_end(torch_mod):
    torch = torch_mod
    import tinycudann as tcnn
    case, B = CASES[1], 200
    m = tcnn.NetworkWithInputEncoding(2, 3, case.enc, case.net, dtype=torch.float32)
    g = O.grid_cfg(case.enc, 2)
    x4 = np.random.default_rng(5).uniform(0, 1, (2 * B, 2)).astype(np.float32)
    xh = np.ascontiguousarray(x4[clear_of_boundaries(g, x4)][:B])
    assert xh.shape[0] == B
    x, v = torch.from_numpy(xh).cuda(), torch.from_numpy(directions(xh, 2)).cuda()
    y, J = m.value_and_jacobian(x)
    y2, Jv = m.value_and_jvp(x, v)
    _, Jv1 = m.value_and_jvp(x, v[:, 0])
    assert y.shape == (B, 3) and J.shape == (B, 3, 2) and Jv.shape == (B, 3, 2) and Jv1.shape == (B, 3)
    assert not any(t.requires_grad for t in (y, J, y2, Jv, Jv1))
    with torch.no_grad():
        assert torch.equal(y, m(x)) and torch.equal(y2, y) and torch.equal(Jv1, Jv[:, :, 0])
    p = m.params.detach().cpu().numpy()
    rows = T.encoded_rows(torch, case, xh, p[case.n_mlp:])
    Jt, Et = truth(case, g, p, p[case.n_mlp:], xh, rows)
    Vt, Ev = truth(case, g, p, p[case.n_mlp:], xh, rows, v.cpu().numpy())
    worst("torch value_and_jacobian", J.cpu().numpy(), Jt, Et)
    worst("torch value_and_jvp", Jv.cpu().numpy(), Vt, Ev)
    xg = x.clone().requires_grad_(True)
    yg = m(xg)
    for o in range(3):
        a = torch.autograd.grad(yg[:, o].sum(), xg, retain_graph=True)[0].cpu().numpy().astype(np.float64)
        assert np.all(np.abs(J[:, o].cpu().numpy() - a) <= 2 * Et[:, o])
        av = np.einsum("bd,bkd->bk", a, v.cpu().numpy().astype(np.float64))
        assert np.all(np.abs(Jv[:, o].cpu().numpy() - av) <= 2 * Ev[:, o])


GRID_FRONT = " behind GridEncoding"
REFUSED = {  # what: (D, encoding, network changes or None for the encoding alone, precision, the front and the reason the message names)
    "fp16": (3, F.GRID2_L4, {}, FP16, "", ""),
    "cutlass": (3, F.GRID2_L4, {"otype": "CutlassMLP"}, FP32, "", ""),
    "encoding": (3, F.GRID2_L4, None, FP32, "", ""),
    "composite": (3, {"otype": "Composite", "nested": [dict(F.GRID2_L4, n_dims_to_encode=2), {"otype": "Identity"}]}, {}, FP32,
                  " behind CompositeEncoding", ""),
    "oneblob": (3, F.ONEBLOB4, {}, FP32, " behind OneBlobEncoding", ""),
    "sine": (3, F.GRID2_L4, {"activation": "Sine"}, FP32, None, None),
    "d4": (4, F.GRID2_L4, {}, FP32, GRID_FRONT, r": a grid of 4 input dimensions \(2 or 3 are served\)"),
    "f1": (3, dict(F.GRID2_L4, n_features_per_level=1), {}, FP32, GRID_FRONT, r": a grid of 1 features per level \(2, 4 or 8 are served\)"),
    "wide": (3, dict(HASH3_L16, n_features_per_level=8), {}, FP32, GRID_FRONT, r": an encoded width of 128 \(at most 64 is served\)"),
    "max_level": (3, F.GRID2_L4, {}, FP32, GRID_FRONT, ": a grid with max_level or stochastic interpolation in effect"),
}


@pytest.mark.parametrize("what", list(REFUSED))
def test_refusals(torch_mod, what):
    torch = torch_mod
    D, enc, change, precision, front, why = REFUSED[what]
    if change is None:  # an encoding alone
        m = Mod(torch, D, enc, FP32)
    else:
        m = T.Net(torch, D, 3, dict(gc("refuse", 64, 2, D, 3, "ReLU", "None", None).net, **change), enc, precision)
    if what == "max_level":
        m.L.check(m.lib.tcnn_module_set_max_level(m.h, 0.5))
    p = m.initial_params(3)
    p = p if m.f32 else p.astype(np.float16).view(np.uint16)
    x = np.random.default_rng(2).uniform(0, 1, (256, D)).astype(np.float32)
    xd, pd = torch.from_numpy(x).cuda(), m._dev(p)
    y = torch.zeros(256 * 128, dtype=torch.float32, device="cuda")
    J = torch.zeros(256 * 3 * D, dtype=torch.float32, device="cuda")
    name = m.lib.tcnn_module_name(m.h).decode()
    message = (rf"{name}: Sine has no backward from its forward value" if what == "sine" else
               rf"^{name}{front}: inference_jvp is not implemented by the MI355X engine yet \(fp32 FullyFusedMLP network modules alone, "
               rf"behind a lone Identity encoding or behind a lone grid encoding only\){why}$")
    with pytest.raises(m.L.TcnnError, match=message):
        m.L.check(m.lib.tcnn_module_inference_jvp(m.h, None, 256, _vp(xd), None, 0, _vp(y), _vp(J), _vp(pd), 0))
    out = m.forward(x, p) if change is None else m.inference(x, p)
    assert np.isfinite(out.astype(np.float32) if m.f32 else out.view(np.float16).astype(np.float32)).all()
    m.close()
