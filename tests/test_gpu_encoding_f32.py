"""GPU tests of fp32-precision encoding modules (tcnn_create_encoding(..., TCNN_PRECISION_FP32),
tinycudann.Encoding(dtype=torch.float32), create_encoding<float>): csrc/grid_f32.hip and the float
instantiations of the typed kernels in grid.hip, composite.hip and encodings.hip, against the float64
restatement of tests/test_grid_f32_reference.py, the oracle and the fp16 modules. Every bound is derived
in a docstring (here or beside the reference) from the kernel's operation count; none comes from what
the kernels produce.
"""
import ctypes
import json
import os
import pickle
import subprocess

import numpy as np
import pytest

import test_composite_reference as R
import test_grid_f32_reference as G
from helpers import CONFIG_HASH, GOLD, rel_err
from oracle import oracle as O
from test_gpu_composite import GRID2_L4, GRID3_L4, REFUSALS

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIG_BTF = json.load(open(os.path.join(GOLD, "config_btf.json")))
FP32, FP16 = 0, 1
B = 257  # a partial wave and a partial 256-thread workgroup
CASE_IDS = [c[0] for c in G.GRID_CASES]


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


def _vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


class Mod:
    """An encoding module of either precision through the C-ABI, numpy in and out (the Mod of
    tests/test_gpu_composite.py with a precision): parameters, rows, dL/dy and dL/dparams are float32
    arrays for an Fp32 module, uint16 fp16 bits for an Fp16 one."""

    def __init__(self, torch, n_in, enc, precision=FP32, alignment=0):
        from tinycudann import _lib as L
        self.torch, self.L, self.lib = torch, L, L.lib()
        self.h = L.check_ptr(self.lib.tcnn_create_encoding_aligned(n_in, json.dumps(enc).encode(), precision, alignment))
        self.f32 = precision == FP32
        self.dt = torch.float32 if self.f32 else torch.float16
        self.n_in = n_in
        self.n_params = self.lib.tcnn_module_n_params(self.h)
        self.width = self.lib.tcnn_module_n_output_dims(self.h)
        self.ctx = None

    def _dev(self, a):
        a = np.ascontiguousarray(a)
        return self.torch.from_numpy(a if self.f32 else a.view(np.float16)).cuda()

    def _host(self, t):
        a = t.cpu().numpy()
        return a if self.f32 else a.view(np.uint16)

    def initial_params(self, seed=1337):
        p32 = self.torch.zeros(max(self.n_params, 1), dtype=self.torch.float32, device="cuda")
        self.L.check(self.lib.tcnn_module_initialize_params(self.h, seed, _vp(p32), 1.0))
        return p32[:self.n_params].cpu().numpy()

    def forward(self, x, params=None):
        torch = self.torch
        self.close_ctx()
        n = x.shape[0]
        self.x = torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()
        self.p = None if params is None else self._dev(params)
        # pre-filled with NaN: every column of every row must be written
        self.out = torch.full((n, self.width), float("nan"), dtype=self.dt, device="cuda")
        self.ctx = self.L.check_ptr(self.lib.tcnn_module_forward(self.h, None, n, _vp(self.x), _vp(self.out), _vp(self.p), 1))
        torch.cuda.synchronize()
        return self._host(self.out)

    def backward(self, dy, want_dx=True, want_params=True, loss_scale=None):
        torch = self.torch
        n = self.x.shape[0]
        d = self._dev(dy)
        dx = torch.full((n, self.n_in), float("nan"), dtype=torch.float32, device="cuda") if want_dx else None
        g = torch.full((self.n_params,), float("nan"), dtype=self.dt, device="cuda") if want_params and self.n_params else None
        if loss_scale is None:
            rc = self.lib.tcnn_module_backward(self.h, None, self.ctx, n, _vp(dx), _vp(d), _vp(g), _vp(self.x), _vp(self.out), _vp(self.p))
        else:
            rc = self.lib.tcnn_module_backward_scaled(self.h, None, self.ctx, n, _vp(dx), _vp(d), _vp(g), _vp(self.x), _vp(self.out),
                                                      _vp(self.p), ctypes.c_float(loss_scale), 0)
        self.L.check(rc)
        torch.cuda.synchronize()
        return (dx.cpu().numpy() if dx is not None else None), (self._host(g) if g is not None else None)

    def backward_backward(self, gx, dy, want_grad=True):
        """second order: (dL/dgrid, dL/d(dL/dy) [B, width], dL/dx) from dL/d(dL/dx) and dL/dy"""
        torch = self.torch
        n = self.x.shape[0]
        g_d = torch.from_numpy(np.ascontiguousarray(gx, np.float32)).cuda()
        d = self._dev(dy)
        grad = torch.full((self.n_params,), float("nan"), dtype=self.dt, device="cuda") if want_grad else None
        ddy = torch.full((n, self.width), 7.0, dtype=self.dt, device="cuda")  # padding columns must come back 0
        dx = torch.full((n, self.n_in), float("nan"), dtype=torch.float32, device="cuda")
        self.L.check(self.lib.tcnn_module_backward_backward_input(self.h, None, self.ctx, n, _vp(g_d), _vp(self.x), _vp(d), _vp(grad),
                                                                   _vp(ddy), _vp(dx), _vp(self.p)))
        torch.cuda.synchronize()
        return (self._host(grad) if grad is not None else None), self._host(ddy), dx.cpu().numpy()

    def close_ctx(self):
        if self.ctx:
            self.lib.tcnn_context_destroy(self.ctx)
            self.ctx = None

    def close(self):
        self.close_ctx()
        self.lib.tcnn_module_destroy(self.h)


# ---------------------------------------------------------------------------------------------
# 1: grid forward
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,D,enc", G.GRID_CASES, ids=CASE_IDS)
def test_grid_forward(torch_mod, name, D, enc):
    """|got - ref| <= forward_bound (tests/test_grid_f32_reference.py: (2D + 2^D + 1) * 2^-24 * A, plus the
    Smoothstep polynomial's counted roundings) against the float64 restatement, on a uniform(-1, 1) float32
    table that is not fp16-representable; every column of every row written."""
    g = O.grid_cfg(enc, D)
    m = Mod(torch_mod, D, enc)
    assert m.n_params == g.n_params and m.width == g.n_levels * g.n_features_per_level
    pos, table, _ = G.make_inputs(g, B, 10)
    assert np.any(O.h2f(O.f2h(table)) != table)
    got = m.forward(pos, table).astype(np.float64)
    assert not np.isnan(got).any()
    ref, A, E = G.grid_forward(g, pos, table)
    r = np.abs(got - ref) / G.forward_bound(g, A, E)
    print(name, "fp32 forward: max error / bound", r.max())
    assert r.max() <= 1.0, (name, r.max(), np.unravel_index(r.argmax(), r.shape))
    m.close()


def test_grid_forward_nearest_is_bit_exact(torch_mod):
    """Nearest copies one entry: got == table[idx], bit for bit."""
    enc = dict(G.GRID2_L8, interpolation="Nearest")
    g = O.grid_cfg(enc, 2)
    m = Mod(torch_mod, 2, enc)
    pos, table, _ = G.make_inputs(g, B, 11)
    got = m.forward(pos, table)
    F = g.n_features_per_level
    t = table.reshape(-1, F)
    for l in range(g.n_levels):
        idx, _, _ = G.level_corners(g, l, pos)
        np.testing.assert_array_equal(got[:, l * F:(l + 1) * F].view(np.uint32), t[idx[:, 0]].view(np.uint32))
    m.close()


def test_grid_forward_padded_row(torch_mod):
    """A lone OneBlob / Identity takes an alignment; a lone grid's padding comes from a composite: the
    composite of one grid at alignment 16 has zero padding and the lone grid's values, bit for bit."""
    enc = dict(G.GRID3_F4, n_levels=3)
    g = O.grid_cfg(enc, 3)
    pos, table, _ = G.make_inputs(g, B, 12)
    lone = Mod(torch_mod, 3, enc)
    comp = Mod(torch_mod, 3, {"otype": "Composite", "nested": [enc]}, alignment=16)
    assert lone.width == 12 and comp.width == 16
    a, b = lone.forward(pos, table), comp.forward(pos, table)
    np.testing.assert_array_equal(b[:, :12].view(np.uint32), a.view(np.uint32))
    np.testing.assert_array_equal(b[:, 12:], 0.0)
    lone.close()
    comp.close()


# ---------------------------------------------------------------------------------------------
# 2: gradient to the parameters
# ---------------------------------------------------------------------------------------------
def check_param_gradient(torch_mod, D, enc, n, seed):
    g = O.grid_cfg(enc, D)
    m = Mod(torch_mod, D, enc)
    pos, table, dy = G.make_inputs(g, n, seed)
    m.forward(pos, table)
    _, grad = m.backward(dy, want_dx=False)
    assert not np.isnan(grad).any()
    ref, count, absum, esum, S_level = G.grid_gradient(g, pos, dy)
    tol = G.gradient_bound(g, ref, count, absum, esum, S_level)
    r = np.abs(grad - ref)[count > 0] / tol[count > 0]
    print("fp32 dL/dparams: max error / bound", r.max(), "B", n)
    assert r.max() <= 1.0, (r.max(), int(r.argmax()))
    assert np.all(grad[count == 0] == 0)
    # bit-reproducible: the int32 sums are order-independent
    _, again = m.backward(dy, want_dx=False)
    np.testing.assert_array_equal(again.view(np.uint32), grad.view(np.uint32))
    # dL/dy scaled by 2^-30: the same bound, which scales with it (a path that narrowed dL/dy to fp16 would
    # flush these values to zero)
    s = np.float32(2.0 ** -30)
    _, small = m.backward(dy * s, want_dx=False)
    rs = np.abs(small.astype(np.float64) - ref * 2.0 ** -30)[count > 0] / (tol[count > 0] * 2.0 ** -30)
    print("fp32 dL/dparams, dL/dy * 2^-30: max error / bound", rs.max())
    assert rs.max() <= 1.0, rs.max()
    assert np.abs(small).max() > 0
    m.close()


@pytest.mark.parametrize("name,D,enc", G.GRID_CASES, ids=CASE_IDS)
def test_grid_param_gradient(torch_mod, name, D, enc):
    """Per element against the float64 restatement within gradient_bound (tests/test_grid_f32_reference.py:
    oracle.grid_grad_tolerance restated for fp32), twice with identical bytes, and with dL/dy * 2^-30."""
    check_param_gradient(torch_mod, D, enc, B, 20)


# levels too large for the LDS as one item: entry ranges of a dense level (level 1: 72^2 entries x 8 features
# = 41472 slots > 32768, the generic index) and of a hashed level (2^14 entries x 4 features: two hash ranges)
SPLIT_CASES = [
    ("dense_range_split", 2, {"otype": "DenseGrid", "n_levels": 2, "n_features_per_level": 8, "base_resolution": 48, "per_level_scale": 1.5}),
    ("hash_range_split", 3, {"otype": "HashGrid", "n_levels": 2, "n_features_per_level": 4, "log2_hashmap_size": 14, "base_resolution": 16,
                             "per_level_scale": 2.0}),
]


@pytest.mark.parametrize("name,D,enc", SPLIT_CASES, ids=[c[0] for c in SPLIT_CASES])
def test_grid_param_gradient_split_levels(torch_mod, name, D, enc):
    """the levels the fp16 path would split by features or bin run as entry ranges here: same bound"""
    g = O.grid_cfg(enc, D)
    F = g.n_features_per_level
    assert max(G.level_size(g, l) * F for l in range(g.n_levels)) > 32768
    check_param_gradient(torch_mod, D, enc, B, 22)


def test_grid_param_gradient_two_chunks(torch_mod):
    """B = 16387: more than one point chunk (B / 8192), so the slab reduction runs"""
    check_param_gradient(torch_mod, 2, G.GRID2_L8, 16387, 21)


# ---------------------------------------------------------------------------------------------
# 3: dL/dinput and second order
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,D,enc", G.GRID_CASES, ids=CASE_IDS)
def test_grid_input_gradient_and_second_order(torch_mod, name, D, enc):
    """These quantities are fp32 arithmetic in both precisions, so on an fp16-representable table and
    dL/dy (widened to fp32) the fp32 module is held to the oracle with the fp16 tests' tolerances: dL/dx
    rtol = atol = 1e-5 (tests/test_gpu_grid_input.py); second order as tests/test_gpu_grid_second_order.py --
    dL/d(dL/dy) rtol 2e-3, atol 1e-4 max; dL/dx rtol 1e-4, atol 1e-4 max; dL/dgrid relative L2 <= 2e-3. With
    dL/dy (and dL/d(dL/dx)) scaled by 2^-30 every output scales by the power of two it is linear in, within
    the same rtol (an fp16 dL/dy would have flushed to zero)."""
    g = O.grid_cfg(enc, D)
    m = Mod(torch_mod, D, enc)
    LF = g.n_levels * g.n_features_per_level
    pos, table, dy = G.make_inputs(g, B, 30)
    t16, dy16 = O.f2h(table), O.f2h(dy)
    table, dy = O.h2f(t16), O.h2f(dy16)
    dy_soa = np.ascontiguousarray(dy16.T)
    m.forward(pos, table)
    dx, _ = m.backward(dy, want_params=False)
    ref_dx = O.grid_bwd_input(g, pos, t16, dy_soa)
    np.testing.assert_allclose(dx, ref_dx, rtol=1e-5, atol=1e-5)
    s = np.float32(2.0 ** -30)
    dxs, _ = m.backward(dy * s, want_params=False)
    np.testing.assert_allclose(dxs.astype(np.float64) * 2.0 ** 30, ref_dx, rtol=1e-5, atol=1e-5)
    assert np.abs(dxs).max() > 0
    # second order
    rng = np.random.default_rng(31)
    gx = (rng.standard_normal((B, D)) * 1e-3).astype(np.float32)
    rgrad, rddy, rdx = O.grid_bwd_bwd(g, pos, t16, gx, dy_soa)
    grad, ddy, dx2 = m.backward_backward(gx, dy)
    assert np.all(ddy[:, LF:] == 0)
    np.testing.assert_allclose(ddy[:, :LF], rddy, rtol=2e-3, atol=1e-4 * np.abs(rddy).max())
    np.testing.assert_allclose(dx2, rdx, rtol=1e-4, atol=1e-4 * np.abs(rdx).max())
    assert rel_err(grad, rgrad) <= 2e-3
    grad_s, ddy_s, dx2_s = m.backward_backward(gx * s, dy * s)
    np.testing.assert_allclose(ddy_s[:, :LF].astype(np.float64) * 2.0 ** 30, rddy, rtol=2e-3, atol=1e-4 * np.abs(rddy).max())
    np.testing.assert_allclose(dx2_s.astype(np.float64) * 2.0 ** 60, rdx, rtol=1e-4, atol=1e-4 * np.abs(rdx).max())
    assert rel_err(grad_s.astype(np.float64) * 2.0 ** 60, rgrad) <= 2e-3
    m.close()


# ---------------------------------------------------------------------------------------------
# 4: parameter-free parts, fp32 against fp16
# ---------------------------------------------------------------------------------------------
PARAM_FREE = [
    ("oneblob4", 3, {"otype": "OneBlob", "n_bins": 4}),
    ("oneblob16", 3, {"otype": "OneBlob", "n_bins": 16}),
    # a power-of-two scale: the fp16 module rounds dL/dy * scale to fp16 (the reference's (T) cast), which is
    # then exact, so the two precisions' dL/dinput agree bit for bit
    ("identity", 5, {"otype": "Identity", "scale": 2.0, "offset": -0.25}),
    ("triangle1", 3, {"otype": "TriangleWave", "n_frequencies": 1}),
    ("triangle12", 3, {"otype": "TriangleWave", "n_frequencies": 12}),
] + [("sh%d" % d, 3, {"otype": "SphericalHarmonics", "degree": d}) for d in range(1, 9)] + [
    ("nrc", 10, {"otype": "NRC"}),
    # the widest row the composite kernels take (256 columns): one wave's fp32 staging tile is 64 rows of 257
    # dwords, past the default dynamic-LDS limit, so the launch raises the kernel's limit first
    ("wide256", 16, {"otype": "Composite", "nested": [{"otype": "OneBlob", "n_bins": 16, "n_dims_to_encode": 8},
                                                      {"otype": "TriangleWave", "n_frequencies": 16, "n_dims_to_encode": 8}]}),
]


@pytest.mark.parametrize("name,n_in,enc", PARAM_FREE, ids=[c[0] for c in PARAM_FREE])
@pytest.mark.parametrize("alignment", [0, 16])
def test_parameter_free_parts_match_fp16(torch_mod, name, n_in, enc, alignment):
    """The fp32 module stores the fp32 value each part computes just before the fp16 module rounds it:
    fp16_rn(out32) == out16 bit for bit, padding columns included; with an fp16-representable dL/dy the two
    modules' dL/dinput are the same fp32 arithmetic on the same numbers: bit-equal. SphericalHarmonics fp32
    values also pass test_sh_forward's bound without its fp16-ulp term: 64 * 2^-24 * M against the float64
    statement (at most 64 fp32 roundings, each relative to a partial result that M bounds)."""
    rng = np.random.default_rng(40)
    x = rng.uniform(0, 1, (B, n_in)).astype(np.float32)
    m32, m16 = Mod(torch_mod, n_in, enc, FP32, alignment), Mod(torch_mod, n_in, enc, FP16, alignment)
    assert m32.width == m16.width and m32.n_params == 0
    o32, o16 = m32.forward(x), m16.forward(x)
    assert not np.isnan(o32).any()
    np.testing.assert_array_equal(O.f2h(o32), o16)
    dy16 = O.f2h(rng.standard_normal(o32.shape).astype(np.float32))
    dx32, _ = m32.backward(O.h2f(dy16))
    dx16, _ = m16.backward(dy16)
    assert not np.isnan(dx32).any()
    np.testing.assert_array_equal(dx32.view(np.uint32), dx16.view(np.uint32))
    if enc["otype"] == "SphericalHarmonics":
        deg = enc["degree"]
        dirs = 2.0 * x.astype(np.float64) - 1.0
        pad = m32.width - deg * deg
        ref, M = R.sh_reference(dirs, deg), R.sh_reference(dirs, deg, absolute=True)
        r = np.abs(o32[:, pad:].astype(np.float64) - ref) / (64 * 2.0 ** -24 * M)
        assert r.max() <= 1.0, r.max()
        np.testing.assert_array_equal(o32[:, :pad], 1.0)
    m32.close()
    m16.close()


# ---------------------------------------------------------------------------------------------
# 5: composites with grids
# ---------------------------------------------------------------------------------------------
COMPOSITES = [
    ("btf", 8, CONFIG_BTF["encoding"]),
    ("two_grids_oneblob", 7, {"otype": "Composite", "nested": [dict(GRID2_L4, n_dims_to_encode=2), dict(GRID3_L4, n_dims_to_encode=3),
                                                                {"otype": "OneBlob", "n_bins": 4}]}),
    # an input column that no part reads
    ("unread_column", 4, {"otype": "Composite", "nested": [dict(GRID2_L4, n_dims_to_encode=2),
                                                            {"otype": "Identity", "n_dims_to_encode": 1, "dims_to_encode_begin": 3}]}),
]


@pytest.mark.parametrize("name,n_in,enc", COMPOSITES, ids=[c[0] for c in COMPOSITES])
def test_composite_with_grids(torch_mod, name, n_in, enc):
    """Widths and columns equal the fp16 module's (R.composite_layout); each grid's value columns equal the
    lone fp32 grid module's output bit for bit and its padding is 0; parameter-free columns round to the fp16
    module's; each grid's parameter gradient passes gradient_bound; unread input columns get dL/dx = 0."""
    parts, total = R.composite_layout(n_in, enc, 16)
    m = Mod(torch_mod, n_in, enc, FP32, 16)
    m16 = Mod(torch_mod, n_in, enc, FP16, 16)
    assert m.width == total == m16.width and m.n_params == m16.n_params
    nested = enc["nested"]
    rng = np.random.default_rng(50)
    table = rng.uniform(-1, 1, m.n_params).astype(np.float32)
    x = rng.uniform(0, 1, (B, n_in)).astype(np.float32)
    out = m.forward(x, table)
    assert not np.isnan(out).any()
    out16 = m16.forward(x, O.f2h(table))
    dy = rng.standard_normal(out.shape).astype(np.float32)
    dx, grad = m.backward(dy)
    assert not np.isnan(dx).any() and not np.isnan(grad).any()
    off, read = 0, np.zeros(n_in, bool)
    for p, n in zip(parts, nested):
        cols, pads = R.value_columns(p), R.pad_columns(p)
        read[p["in_col"]:p["in_col"] + p["n_in"]] = True
        if p["kind"] in R.GRIDS:
            g = O.grid_cfg(n, p["n_in"])
            pos = np.ascontiguousarray(x[:, p["in_col"]:p["in_col"] + p["n_in"]])
            tab = table[off:off + g.n_params]
            lone = Mod(torch_mod, p["n_in"], {k: v for k, v in n.items() if k not in ("n_dims_to_encode", "dims_to_encode_begin")})
            np.testing.assert_array_equal(out[:, cols].view(np.uint32), lone.forward(pos, tab).view(np.uint32))
            lone.close()
            np.testing.assert_array_equal(out[:, pads], 0.0)
            d = np.ascontiguousarray(dy[:, cols])
            ref, count, absum, esum, S_level = G.grid_gradient(g, pos, d)
            tol = G.gradient_bound(g, ref, count, absum, esum, S_level)
            r = np.abs(grad[off:off + g.n_params] - ref)[count > 0] / tol[count > 0]
            assert r.max() <= 1.0, (name, p["kind"], off, r.max())
            off += g.n_params
        else:
            np.testing.assert_array_equal(O.f2h(out[:, cols]), out16[:, cols])
            np.testing.assert_array_equal(out[:, pads], 1.0)
    assert off == m.n_params
    np.testing.assert_array_equal(dx[:, ~read], 0.0)
    m.close()
    m16.close()


# ---------------------------------------------------------------------------------------------
# 6: module surface
# ---------------------------------------------------------------------------------------------
def test_module_surface(torch_mod):
    torch = torch_mod
    enc = G.GRID2_L8
    a, h = Mod(torch, 2, enc, FP32), Mod(torch, 2, enc, FP16)
    lib = a.lib
    assert lib.tcnn_module_param_precision(a.h) == FP32 and lib.tcnn_module_output_precision(a.h) == FP32
    assert lib.tcnn_module_param_precision(h.h) == FP16 and lib.tcnn_module_output_precision(h.h) == FP16
    assert lib.tcnn_default_loss_scale(FP32) == 1.0
    np.testing.assert_array_equal(a.initial_params(), h.initial_params())
    assert lib.tcnn_module_name(a.h) == lib.tcnn_module_name(h.h)
    assert lib.tcnn_module_hyperparams(a.h) == lib.tcnn_module_hyperparams(h.h)
    assert a.n_params == h.n_params and a.width == h.width
    # B = 0: forward / backward succeed, dL/dparams is zero-filled as fp32 (4 bytes per element)
    x0 = torch.zeros(0, 2, device="cuda")
    o0 = torch.zeros(0, a.width, device="cuda")
    p = torch.zeros(a.n_params, device="cuda")
    ctx = a.L.check_ptr(lib.tcnn_module_forward(a.h, None, 0, _vp(x0), _vp(o0), _vp(p), 1))
    for scaled in (False, True):
        gr = torch.full((a.n_params + 1,), float("nan"), device="cuda")
        if scaled:
            a.L.check(lib.tcnn_module_backward_scaled(a.h, None, ctx, 0, None, _vp(o0), _vp(gr), _vp(x0), _vp(o0), _vp(p),
                                                      ctypes.c_float(128.0), 0))
        else:
            a.L.check(lib.tcnn_module_backward(a.h, None, ctx, 0, None, _vp(o0), _vp(gr), _vp(x0), _vp(o0), _vp(p)))
        torch.cuda.synchronize()
        grn = gr.cpu().numpy()
        assert np.all(grn[:-1] == 0) and np.isnan(grn[-1])  # all n_params floats, and nothing past them
    lib.tcnn_context_destroy(ctx)
    a.close()
    h.close()


def test_backward_scaled_loss_scales_agree(torch_mod):
    """tcnn_module_backward_scaled with loss_scale 1 and 128 must agree within one fp32 rounding per element
    (2^-23 relative); by derivation they are bit-equal, which is what is asserted. The scale 128 multiplies
    dL/dy exactly; the backward's pre-pass sum of |dL/dy|, its product with 1.01 and the limit derived from it
    all scale exactly by 128 (the exponent clamp is far away), so the fixed-point exponent e drops by exactly
    7 and dy * 128 * 2^(e - 7) == dy * 2^e: the int32 sums are identical, the decoded slabs are 128 times
    larger exactly, their fixed-order fp32 sum scales exactly, and the final division by 128 is exact. dL/dx
    is fp32 arithmetic that commutes with a power-of-two factor in the same way. loss_scale 1 is the plain
    backward, bit for bit."""
    m = Mod(torch_mod, 2, G.GRID2_L8)
    g = O.grid_cfg(G.GRID2_L8, 2)
    pos, table, dy = G.make_inputs(g, B, 60)
    m.forward(pos, table)
    dx1, g1 = m.backward(dy, loss_scale=1.0)
    dx128, g128 = m.backward(dy, loss_scale=128.0)
    dxp, plain = m.backward(dy)
    np.testing.assert_array_equal(g1.view(np.uint32), plain.view(np.uint32))
    np.testing.assert_array_equal(dx1.view(np.uint32), dxp.view(np.uint32))
    assert np.all(np.abs(g128.astype(np.float64) - g1) <= 2.0 ** -23 * np.abs(g1))
    np.testing.assert_array_equal(g128.view(np.uint32), g1.view(np.uint32))
    np.testing.assert_array_equal(dx128.view(np.uint32), dx1.view(np.uint32))
    assert np.abs(g1).max() > 0
    m.close()


# ---------------------------------------------------------------------------------------------
# grid options on an fp32 module (in the style of tests/test_gpu_grid_options.py)
# ---------------------------------------------------------------------------------------------
def masked_levels(g, ml):
    """[B, L] bool: level l of point i is masked -- (float)l >= max_level_i * n_features / F + 1e-3 in fp32
    (grid.h:69-91; the backward's `>` differs only on exact equality, which these values do not hit)"""
    L, F = g.n_levels, g.n_features_per_level
    thr = (np.asarray(ml, np.float32) * np.float32(L * F)) / np.float32(F) + np.float32(1e-3)
    lv = np.arange(L, dtype=np.float32)[None, :]
    assert not np.any(np.abs(lv - thr[:, None]) < 1e-4)
    return lv >= thr[:, None]


@pytest.mark.parametrize("per_point", [False, True], ids=["scalar", "per_point"])
def test_max_level_masking_fp32(torch_mod, per_point):
    """max_level on an fp32 grid module: masked levels output exactly 0, the others pass forward_bound;
    dL/dparams is the float64 gradient of the masked dL/dy within gradient_bound -- with S_level taken from the
    unmasked dL/dy, because the kernel's scale pre-pass sums every point's |dL/dy|, masked or not, so that is
    what its fixed-point step follows; dL/dx against the oracle on an fp16-representable table and dL/dy
    (rtol = atol = 1e-5, as test_max_level_masking)."""
    torch = torch_mod
    enc = G.GRID2_L8
    g = O.grid_cfg(enc, 2)
    m = Mod(torch, 2, enc)
    L, F = g.n_levels, g.n_features_per_level
    pos, table, dy = G.make_inputs(g, B, 70)
    t16, dy16 = O.f2h(table), O.f2h(dy)
    table, dy = O.h2f(t16), O.h2f(dy16)
    rng = np.random.default_rng(71)
    if per_point:
        ml = rng.uniform(0, 1, B).astype(np.float32)
        ml_d = torch.from_numpy(ml).cuda()
        m.L.check(m.lib.tcnn_module_set_max_level_gpu(m.h, _vp(ml_d)))
        O.grid_set_max_level(g, 0.0, ml)
    else:
        ml = np.full(B, 0.45, np.float32)
        m.L.check(m.lib.tcnn_module_set_max_level(m.h, 0.45))
        O.grid_set_max_level(g, 0.45)
    mask = np.repeat(masked_levels(g, ml), F, axis=1)  # [B, L * F]
    assert mask.any() and not mask.all()
    np.testing.assert_array_equal(O.grid_fwd(g, pos, t16).T == 0, mask)  # the oracle masks the same outputs
    out = m.forward(pos, table)
    assert not np.isnan(out).any()
    np.testing.assert_array_equal(out[mask], 0.0)
    g_plain = O.grid_cfg(enc, 2)
    ref, A, E = G.grid_forward(g_plain, pos, table)
    assert np.all(np.abs(out.astype(np.float64) - ref)[~mask] <= G.forward_bound(g_plain, A, E)[~mask])
    dx, grad = m.backward(dy)
    gref, count, absum, esum, _ = G.grid_gradient(g_plain, pos, np.where(mask, 0.0, dy))
    S_level = G.grid_gradient(g_plain, pos, dy)[4]
    tol = G.gradient_bound(g_plain, gref, count, absum, esum, S_level)
    r = np.abs(grad - gref)[count > 0] / tol[count > 0]
    assert r.max() <= 1.0, r.max()
    dy_soa = np.ascontiguousarray(dy16.T)
    np.testing.assert_allclose(dx, O.grid_bwd_input(g, pos, t16, dy_soa), rtol=1e-5, atol=1e-5)
    top = int(g.offsets[L - 1]) * F
    if not per_point:
        assert np.all(grad[top:] == 0) and np.any(grad[:top] != 0)  # masked levels get no gradient
    m.close()


def test_stochastic_interpolation_backward_fp32(torch_mod):
    """stochastic_interpolation on an fp32 grid module: the forward is unaffected (bit-equal to the plain fp32
    module's), the backward sends each (point, level) gradient with weight 1 to the corner picked by
    pcg32{1337}.advance(i + l * B) -- against the oracle's stochastic backward on an fp16-representable dL/dy,
    relative L2 <= 1e-3 as test_stochastic_interpolation_backward, and far from the interpolating gradient."""
    enc = dict(G.GRID2_L8, stochastic_interpolation=True)
    g = O.grid_cfg(enc, 2)
    m, plain = Mod(torch_mod, 2, enc), Mod(torch_mod, 2, G.GRID2_L8)
    n = 1024
    pos, table, dy = G.make_inputs(g, n, 72)
    dy16 = O.f2h(dy)
    dy = O.h2f(dy16)
    np.testing.assert_array_equal(m.forward(pos, table).view(np.uint32), plain.forward(pos, table).view(np.uint32))
    _, grad = m.backward(dy, want_dx=False)
    dy_soa = np.ascontiguousarray(dy16.T)
    assert rel_err(grad, O.grid_bwd(g, pos, dy_soa)) <= 1e-3
    assert rel_err(grad, O.grid_bwd(O.grid_cfg(G.GRID2_L8, 2), pos, dy_soa)) > 0.1  # really stochastic
    _, again = m.backward(dy, want_dx=False)
    np.testing.assert_array_equal(again.view(np.uint32), grad.view(np.uint32))
    m.close()
    plain.close()


@pytest.mark.parametrize("n_in,enc,message", REFUSALS, ids=[str(i) for i in range(len(REFUSALS))])
def test_refusals_at_fp32(torch_mod, n_in, enc, message):
    from tinycudann import _lib as L
    lib = L.lib()
    assert not lib.tcnn_create_encoding(n_in, json.dumps(enc).encode(), FP32)
    assert message in lib.tcnn_last_error().decode(), lib.tcnn_last_error().decode()


def test_double_backward_of_composites_refused_at_fp32(torch_mod):
    m = Mod(torch_mod, 7, COMPOSITES[1][2], FP32, 16)
    m.forward(np.full((4, 7), 0.25, np.float32), np.zeros(m.n_params, np.float32))
    z = torch_mod.zeros(4, m.width, device="cuda")
    rc = m.lib.tcnn_module_backward_backward_input(m.h, None, m.ctx, 4, _vp(z), _vp(m.x), _vp(m.out), None, _vp(m.out), _vp(z), _vp(m.p))
    assert rc != 0 and "not implemented" in m.lib.tcnn_last_error().decode()
    m.close()


# ---------------------------------------------------------------------------------------------
# 7: torch
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("python_node", [False, True], ids=["cpp_node", "python_node"])
def test_torch_encoding_fp32(torch_mod, python_node, monkeypatch):
    """tcnn.Encoding(dtype=torch.float32) through the C++ autograd node and the Python fallback: dtypes,
    first and double backward (the pattern and tolerances of tests/test_gpu_grid_second_order.py, on
    fp16-representable parameters and weights so the oracle's fp16 inputs are exact), a pickle round trip,
    and composition with a torch.nn.Linear without casts."""
    torch = torch_mod
    import tinycudann as tcnn
    from tinycudann import modules
    if python_node:
        monkeypatch.setattr(modules, "_EXT", None)
    elif modules._EXT is None:
        pytest.fail("the C++ autograd node (lib/_tcnn_torch) is not built")
    enc_cfg = dict(CONFIG_HASH["encoding"], interpolation="Smoothstep")
    enc = tcnn.Encoding(2, enc_cfg, dtype=torch.float32)
    assert enc.params.dtype == torch.float32 and enc.loss_scale == 1.0 and enc.dtype == torch.float32
    rng = np.random.default_rng(5)
    table16 = O.f2h(rng.uniform(-1, 1, enc.params.numel()).astype(np.float32))
    with torch.no_grad():
        enc.params.copy_(torch.from_numpy(O.h2f(table16)).cuda())
    n = 512
    pos = rng.uniform(0, 1, (n, 2)).astype(np.float32)
    x = torch.from_numpy(pos).cuda().requires_grad_(True)
    y = enc(x)
    assert y.dtype == torch.float32 and y.shape == (n, enc.n_output_dims)
    # first order, and a Linear on top without casts
    lin = torch.nn.Linear(enc.n_output_dims, 3).cuda()
    lin(y).sum().backward()
    assert enc.params.grad.dtype == torch.float32 and enc.params.grad.abs().max() > 0
    assert x.grad is not None and x.grad.dtype == torch.float32 and torch.isfinite(x.grad).all()
    enc.params.grad = None
    x.grad = None
    # pickle round trip: the same output bit for bit
    enc2 = pickle.loads(pickle.dumps(enc))
    assert enc2.params.dtype == torch.float32
    assert torch.equal(enc2(x.detach()), enc(x.detach()))
    sd = enc.state_dict()
    enc3 = tcnn.Encoding(2, enc_cfg, dtype=torch.float32)
    enc3.load_state_dict(sd)
    assert torch.equal(enc3(x.detach()), enc(x.detach()))
    # double backward
    w16 = O.f2h((rng.standard_normal((n, enc.n_output_dims)) * 0.1).astype(np.float32))
    w = torch.from_numpy(O.h2f(w16)).cuda().requires_grad_(True)
    v = torch.from_numpy((rng.standard_normal((n, 2)) * 1e-3).astype(np.float32)).cuda()
    y = enc(x)
    gx = torch.autograd.grad((y * w).sum(), x, create_graph=True)[0]
    (gx * v).sum().backward()
    torch.cuda.synchronize()
    g = O.grid_cfg(enc_cfg, 2)
    dy_soa = np.ascontiguousarray(w16.T)  # loss scale 1: dL/dy = w
    rgrad, rddy, rdx = O.grid_bwd_bwd(g, pos, table16, v.cpu().numpy(), dy_soa)
    gxn = gx.detach().cpu().numpy()
    np.testing.assert_allclose(gxn, O.grid_bwd_input(g, pos, table16, dy_soa), rtol=1e-4, atol=1e-4 * np.abs(gxn).max())
    np.testing.assert_allclose(x.grad.cpu().numpy(), rdx, rtol=1e-4, atol=1e-4 * np.abs(rdx).max())
    assert w.grad.dtype == torch.float32
    np.testing.assert_allclose(w.grad.cpu().numpy(), rddy, rtol=2e-3, atol=1e-4 * np.abs(rddy).max())
    assert rel_err(enc.params.grad.cpu().numpy(), rgrad) <= 2e-3


# ---------------------------------------------------------------------------------------------
# 8: C++
# ---------------------------------------------------------------------------------------------
def test_cpp_encoding_f32_consumer():
    """tests/cpp/encoding_f32_consumer.cpp (built by the Makefile): create_encoding<float> and
    tcnn::cpp::create_encoding(..., Precision::Fp32) report Fp32 and give the same finite inference output."""
    exe = os.path.join(REPO, "neuralbtf-tiny-cuda-nn_amd", "bin", "encoding_f32_consumer")
    assert os.path.exists(exe), "build it with make -C neuralbtf-tiny-cuda-nn_amd"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "encoding f32 api ok" in r.stdout, r.stdout
