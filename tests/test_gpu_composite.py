"""GPU tests of the Composite, SphericalHarmonics and TriangleWave encodings (csrc/composite.hip and
the host plumbing around it) against the CPU references of tests/test_composite_reference.py and the
oracle's pieces (grid, MLP, OneBlob, Identity, loss, Adam). The bounds are derived in each test's
docstring; none of them comes from what the kernels produce.
"""
import ctypes
import json
import os
import pickle

import numpy as np
import pytest

import test_composite_reference as R
from helpers import (CONFIG_HASH, GOLD, assert_within_fp16_ulps, assert_wgrad_per_element, make_batch, rel_err, relu_margin_ok,
                     trainer_arrays)
from oracle import oracle as O

pytestmark = pytest.mark.gpu

CONFIG_BTF = json.load(open(os.path.join(GOLD, "config_btf.json")))


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


def _vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


class Mod:
    """A C-ABI module (encoding, or network with input encoding) with numpy in and out."""

    def __init__(self, torch, n_in, enc, alignment=0, net=None, n_out=0):
        from tinycudann import _lib as L
        self.torch, self.L, self.lib = torch, L, L.lib()
        e = json.dumps(enc).encode()
        if net is not None:
            h = self.lib.tcnn_create_network_with_input_encoding(n_in, n_out, e, json.dumps(net).encode())
        else:
            h = self.lib.tcnn_create_encoding_aligned(n_in, e, 1, alignment)
        self.h = L.check_ptr(h)
        self.n_in = n_in
        self.n_params = self.lib.tcnn_module_n_params(self.h)
        self.width = self.lib.tcnn_module_n_output_dims(self.h)
        self.ctx = None

    def initial_params(self, seed=1337):
        p32 = self.torch.zeros(max(self.n_params, 1), dtype=self.torch.float32, device="cuda")
        self.L.check(self.lib.tcnn_module_initialize_params(self.h, seed, _vp(p32), 1.0))
        return p32[:self.n_params].cpu().numpy()

    def forward(self, x, params16=None):
        torch = self.torch
        self.close_ctx()
        B = x.shape[0]
        self.x = torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()
        self.p = None if params16 is None else torch.from_numpy(np.ascontiguousarray(params16).view(np.float16)).cuda()
        # pre-filled with NaN: every column of every row must be written (there is no memset)
        self.out = torch.full((B, self.width), float("nan"), dtype=torch.float16, device="cuda")
        self.ctx = self.L.check_ptr(self.lib.tcnn_module_forward(self.h, None, B, _vp(self.x), _vp(self.out), _vp(self.p), 1))
        torch.cuda.synchronize()
        return self.out.cpu().numpy().view(np.uint16)

    def backward(self, dy16, want_dx=True, want_params=True):
        torch = self.torch
        B = self.x.shape[0]
        dy = torch.from_numpy(np.ascontiguousarray(dy16).view(np.float16)).cuda()
        dx = torch.full((B, self.n_in), float("nan"), dtype=torch.float32, device="cuda") if want_dx else None
        g = torch.full((self.n_params,), float("nan"), dtype=torch.float16, device="cuda") if want_params and self.n_params else None
        self.L.check(self.lib.tcnn_module_backward(self.h, None, self.ctx, B, _vp(dx), _vp(dy), _vp(g), _vp(self.x), _vp(self.out),
                                                   _vp(self.p)))
        torch.cuda.synchronize()
        return (dx.cpu().numpy() if dx is not None else None), (g.float().cpu().numpy() if g is not None else None)

    def close_ctx(self):
        if self.ctx:
            self.lib.tcnn_context_destroy(self.ctx)
            self.ctx = None

    def close(self):
        self.close_ctx()
        self.lib.tcnn_module_destroy(self.h)


def ulp_fp16(v):
    return np.spacing(np.abs(np.asarray(v, np.float64)).astype(np.float16)).astype(np.float64)


@pytest.fixture(scope="module")
def sh_points():
    """257 rows of [0, 1]^3: 200 unit directions mapped by (d + 1) / 2 and 57 uniform points off the sphere"""
    rng = np.random.default_rng(11)
    d = rng.standard_normal((200, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    x = np.concatenate([(d + 1.0) / 2.0, rng.uniform(0, 1, (57, 3))]).astype(np.float32)
    return x, 2.0 * x.astype(np.float64) - 1.0  # the kernel's input and the exact direction it stands for


def sh_input_gradient_reference(dirs, degree, dy):
    """dL/dx = 2 sum_j dL/dy_j dY_j/dd (central differences of the float64 statement), and the bound
    2^-18 sum_j |dL/dy_j| G_j with G_j the same difference of the absolute-mode statement"""
    J = R.sh_reference_jacobian(dirs, degree)
    G = R.sh_reference_jacobian(dirs, degree, absolute=True)
    ref = 2.0 * np.einsum("nj,njc->nc", dy, J)
    bound = 2.0 ** -18 * np.einsum("nj,njc->nc", np.abs(dy), G)
    return ref, bound, J


# ---------------------------------------------------------------------------------------------
# 1, 2: SphericalHarmonics as an Encoding module
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("degree", range(1, 9))
def test_sh_forward(torch_mod, sh_points, degree):
    """|got - ref| <= ulp_fp16(|ref|) + 64 * 2^-24 * M, M the absolute-mode value (the sum of the
    magnitudes of the polynomial's terms). The kernel evaluates the same polynomial in fp32 in its
    own order: an output passes through at most 64 fp32 roundings (38 by the count in sh_device.h,
    plus the rounding of 2x - 1 entering each of up to 7 factors), each at most 2^-24 of a partial
    result that M bounds; rounding that fp32 value to fp16 instead of the exact one moves the stored
    number by at most one fp16 ulp of the reference."""
    x, dirs = sh_points
    m = Mod(torch_mod, 3, {"otype": "SphericalHarmonics", "degree": degree})
    assert m.width == degree * degree and m.n_params == 0
    out = m.forward(x)
    got = O.h2f(out).astype(np.float64)
    assert not np.isnan(got).any()
    ref = R.sh_reference(dirs, degree)
    M = R.sh_reference(dirs, degree, absolute=True)
    r = np.abs(got - ref) / (ulp_fp16(ref) + 64 * 2.0 ** -24 * M)
    print("SH forward degree", degree, "max error / bound", r.max())
    assert r.max() <= 1.0, (degree, r.max(), np.unravel_index(r.argmax(), r.shape))
    m.close()


def test_sh_padding_comes_first(torch_mod, sh_points):
    x, dirs = sh_points
    m = Mod(torch_mod, 3, {"otype": "SphericalHarmonics", "degree": 3}, alignment=16)
    assert m.width == 16
    out = O.h2f(m.forward(x))
    assert not np.isnan(out).any()
    np.testing.assert_array_equal(out[:, :7], np.ones((257, 7), np.float32))
    plain = Mod(torch_mod, 3, {"otype": "SphericalHarmonics", "degree": 3})
    np.testing.assert_array_equal(out[:, 7:], O.h2f(plain.forward(x)))
    m.close()
    plain.close()


@pytest.mark.parametrize("degree", range(1, 9))
def test_sh_input_gradient(torch_mod, sh_points, degree):
    """dL/dx against 2 sum_j dL/dy_j dY_j/dd from central differences (h = 1e-5) of the float64
    statement; bound 2^-18 sum_j |dL/dy_j| G_j, G_j the abs-sum of the terms of dY_j/dd (the same
    difference of the absolute-mode statement): 64 fp32 roundings of 2^-24 each, relative to the
    magnitudes of the terms summed, as in the forward. (The difference quotient's own error is
    h^2 Y''' / 6 ~ 1e-9 relative and 1e-16 / h = 1e-11 of rounding, far below 2^-18.)"""
    x, dirs = sh_points
    rng = np.random.default_rng(100 + degree)
    m = Mod(torch_mod, 3, {"otype": "SphericalHarmonics", "degree": degree})
    m.forward(x)
    dy16 = O.f2h(rng.standard_normal((x.shape[0], degree * degree)).astype(np.float32))
    dx, _ = m.backward(dy16)
    ref, bound, _ = sh_input_gradient_reference(dirs, degree, O.h2f(dy16).astype(np.float64))
    if degree == 1:  # a constant: exactly zero
        np.testing.assert_array_equal(dx, np.zeros_like(dx))
    else:
        r = np.abs(dx - ref) / bound
        print("SH dL/dinput degree", degree, "max error / bound", r.max())
        assert r.max() <= 1.0, (degree, r.max())
    m.close()


# ---------------------------------------------------------------------------------------------
# 3: TriangleWave
# ---------------------------------------------------------------------------------------------
def triangle_points(dims):
    rng = np.random.default_rng(5)
    x = rng.uniform(0, 1, (65, dims)).astype(np.float32)
    x[:4, 0] = [0.0, 0.25, 0.5, 1.0 - 2.0 ** -24]
    return x


@pytest.mark.parametrize("dims", [1, 3])
@pytest.mark.parametrize("n_frequencies", [1, 12])
def test_triangle_wave(torch_mod, n_frequencies, dims):
    """Forward bit-equal to the float32 statement (every step is one correctly rounded IEEE operation,
    the products by powers of two are exact); dL/dinput = sum_k dL/dy_k (+-2^(k+1)) within
    2^-20 sum_k |dL/dy_k| 2^(k+1): the products are exact and an fp32 sum of at most 12 terms rounds at
    most 11 times by 2^-24 of a partial sum."""
    x = triangle_points(dims)
    m = Mod(torch_mod, dims, {"otype": "TriangleWave", "n_frequencies": n_frequencies})
    assert m.width == dims * n_frequencies
    out = m.forward(x)
    y, dydx = R.triangle_wave_reference(x, n_frequencies)
    np.testing.assert_array_equal(out, O.f2h(y))
    rng = np.random.default_rng(6)
    dy16 = O.f2h(rng.standard_normal(out.shape).astype(np.float32))
    dx, _ = m.backward(dy16)
    t = O.h2f(dy16).astype(np.float64) * dydx.astype(np.float64)
    ref = t.reshape(65, dims, n_frequencies).sum(axis=2)
    bound = 2.0 ** -20 * np.abs(t).reshape(65, dims, n_frequencies).sum(axis=2)
    assert np.all(np.abs(dx - ref) <= bound), np.abs(dx - ref).max()
    m.close()


# ---------------------------------------------------------------------------------------------
# 4: composite layout (NRC), refusals
# ---------------------------------------------------------------------------------------------
NRC_PERMUTED = {"otype": "Composite", "nested": [
    {"n_dims_to_encode": 3, "dims_to_encode_begin": 7, "otype": "TriangleWave", "n_frequencies": 12},
    {"n_dims_to_encode": 5, "dims_to_encode_begin": 2, "otype": "OneBlob", "n_bins": 4},
    {"n_dims_to_encode": 2, "dims_to_encode_begin": 0, "otype": "Identity"}]}


@pytest.mark.parametrize("enc", [{"otype": "NRC"}, NRC_PERMUTED], ids=["nrc", "permuted"])
def test_composite_layout_nrc(torch_mod, enc):
    parts, total = R.composite_layout(10, enc, 16)
    assert total == 64
    m = Mod(torch_mod, 10, enc, alignment=16)
    assert m.width == 64 and m.n_params == 0
    rng = np.random.default_rng(8)
    for B in (1, 63, 64, 65, 257):
        x = rng.uniform(0, 1, (B, 10)).astype(np.float32)
        out = m.forward(x)
        assert not np.isnan(O.h2f(out)).any()
        tri, blob, ident = parts
        xs = lambda p: np.ascontiguousarray(x[:, p["in_col"]:p["in_col"] + p["n_in"]])
        np.testing.assert_array_equal(out[:, R.value_columns(tri)], O.f2h(R.triangle_wave_reference(xs(tri), 12)[0]))
        np.testing.assert_array_equal(out[:, R.value_columns(blob)], O.oneblob_fwd(xs(blob), 4))
        np.testing.assert_array_equal(out[:, R.value_columns(ident)], O.identity_fwd(xs(ident)))
        assert R.pad_columns(ident) == slice(58, 64)
        np.testing.assert_array_equal(O.h2f(out[:, 58:]), np.ones((B, 6), np.float32))
    # dL/dinput of the three parts in one launch: TriangleWave and Identity as stated, OneBlob as the oracle
    dy16 = O.f2h(rng.standard_normal(out.shape).astype(np.float32))
    dx, _ = m.backward(dy16)
    dyf = O.h2f(dy16)
    np.testing.assert_array_equal(dx[:, ident["in_col"]:ident["in_col"] + 2], dyf[:, R.value_columns(ident)])
    ref_blob = O.oneblob_bwd(xs(blob), 4, np.ascontiguousarray(dy16[:, R.value_columns(blob)]))
    np.testing.assert_array_equal(dx[:, blob["in_col"]:blob["in_col"] + 5], ref_blob)
    t = dyf[:, R.value_columns(tri)].astype(np.float64) * R.triangle_wave_reference(xs(tri), 12)[1]
    got = dx[:, tri["in_col"]:tri["in_col"] + 3]
    assert np.all(np.abs(got - t.reshape(B, 3, 12).sum(axis=2)) <= 2.0 ** -20 * np.abs(t).reshape(B, 3, 12).sum(axis=2))
    m.close()


def test_unread_input_columns_get_zero_gradient(torch_mod):
    enc = {"otype": "Composite", "nested": [{"n_dims_to_encode": 1, "dims_to_encode_begin": 1, "otype": "Identity", "scale": 2.0},
                                            {"n_dims_to_encode": 1, "dims_to_encode_begin": 3, "otype": "TriangleWave", "n_frequencies": 2}]}
    m = Mod(torch_mod, 5, enc)
    assert m.width == 3
    x = np.random.default_rng(2).uniform(0, 1, (70, 5)).astype(np.float32)
    m.forward(x)
    dx, _ = m.backward(O.f2h(np.ones((70, 3), np.float32)))
    np.testing.assert_array_equal(dx[:, [0, 2, 4]], np.zeros((70, 3), np.float32))
    np.testing.assert_array_equal(dx[:, 1], np.full(70, 2.0, np.float32))
    assert np.all(np.abs(dx[:, 3]) >= 2.0)
    m.close()


SH3 = {"n_dims_to_encode": 3, "otype": "SphericalHarmonics"}
REFUSALS = [
    (6, {"otype": "Composite", "nested": [dict(SH3), dict(SH3, dims_to_encode_begin=2)]}, "overlap"),
    (6, {"otype": "Composite", "reduction": "Sum", "nested": [dict(SH3), dict(SH3)]}, "not implemented"),
    (6, {"otype": "Composite", "nested": [dict(SH3), {"otype": "Composite", "nested": [dict(SH3)]}]}, "nested Composite"),
    (6, {"otype": "Composite", "nested": [dict(SH3), {"otype": "Frequency"}]}, "'Frequency' is not implemented"),
    (2, {"otype": "SphericalHarmonics"}, "Can only encode 3D directions"),
    (3, {"otype": "SphericalHarmonics", "degree": 9}, "only implemented up to degree 8"),
    (5, {"otype": "Composite", "nested": [dict(SH3), dict(SH3)]}, "must not encode more dims"),
    (5, {"otype": "Composite", "nested": [dict(SH3), dict(SH3, dims_to_encode_begin=3)]}, "beyond the composite"),
    (3, {"otype": "Frequency"}, "'Frequency' is not implemented by the MI355X engine yet"),
]


@pytest.mark.parametrize("n_in,enc,message", REFUSALS, ids=[str(i) for i in range(len(REFUSALS))])
def test_refusals(torch_mod, n_in, enc, message):
    from tinycudann import _lib as L
    lib = L.lib()
    assert not lib.tcnn_create_encoding(n_in, json.dumps(enc).encode(), 1)
    assert message in lib.tcnn_last_error().decode(), lib.tcnn_last_error().decode()
    m = Mod(torch_mod, 3, {"otype": "SphericalHarmonics", "degree": 2})  # the library still works
    assert O.h2f(m.forward(np.full((3, 3), 0.5, np.float32)))[0, 0] == np.float32(np.float16(0.28209479))
    m.close()


def test_module_names_hyperparams_and_unsupported_calls(torch_mod):
    from tinycudann import _lib as L
    lib = L.lib()
    cases = [(3, {"otype": "SphericalHarmonics"}, "SphericalHarmonicsEncoding", {"otype": "SphericalHarmonics", "degree": 4}),
             (2, {"otype": "TriangleWave", "n_frequencies": 3}, "TriangleWaveEncoding", {"otype": "TriangleWave", "n_frequencies": 3}),
             (10, {"otype": "NRC"}, "CompositeEncoding",
              {"otype": "Composite", "nested": [{"otype": "TriangleWave", "n_frequencies": 12}, {"otype": "OneBlob", "n_bins": 4},
                                                {"otype": "Identity", "scale": 1.0, "offset": 0.0}]})]
    for n_in, enc, name, hyper in cases:
        m = Mod(torch_mod, n_in, enc)
        assert lib.tcnn_module_name(m.h).decode() == name
        assert json.loads(lib.tcnn_module_hyperparams(m.h).decode()) == hyper
        assert lib.tcnn_module_set_max_level(m.h, 1.0) != 0
        assert "not implemented" in lib.tcnn_last_error().decode()
        x = np.full((4, n_in), 0.25, np.float32)
        m.forward(x)
        z = torch_mod.zeros(4, max(m.width, n_in), device="cuda")
        assert lib.tcnn_module_backward_backward_input(m.h, None, m.ctx, 4, _vp(z), _vp(m.x), _vp(m.out), None, _vp(m.out), _vp(z), None) != 0
        assert "not implemented" in lib.tcnn_last_error().decode()
        m.close()


# ---------------------------------------------------------------------------------------------
# 5, 9: composites with grids as a module
# ---------------------------------------------------------------------------------------------
GRID3_F4 = {"otype": "HashGrid", "n_levels": 4, "n_features_per_level": 4, "log2_hashmap_size": 10, "base_resolution": 4,
            "per_level_scale": 1.5}
GRID2_L8 = {"otype": "HashGrid", "n_levels": 8, "n_features_per_level": 2, "log2_hashmap_size": 12, "base_resolution": 8,
            "per_level_scale": 1.5}
GRID2_L4 = dict(GRID2_L8, n_levels=4)
GRID3_L4 = {"otype": "HashGrid", "n_levels": 4, "n_features_per_level": 2, "log2_hashmap_size": 11, "base_resolution": 4,
            "per_level_scale": 2.0}


def check_grid_parts(torch_mod, n_in, nested, alignment, B=256):
    """Forward slices bit-equal to the oracle grid; dL/dparams per element within the grid backward's
    own bound (oracle.grid_grad_tolerance) plus the fp16 rounding of the module's fp16 gradient output
    (2^-11 relative, 2^-25 in the subnormals); dL/dinput of the grid columns as tests/test_gpu_grid_input.py
    (rtol = atol = 1e-5); parameter-free parts as their references."""
    enc = {"otype": "Composite", "nested": nested}
    parts, total = R.composite_layout(n_in, enc, alignment)
    m = Mod(torch_mod, n_in, enc, alignment=alignment)
    assert m.width == total
    grids = [(p, O.grid_cfg(n, p["n_in"])) for p, n in zip(parts, nested) if p["kind"] in R.GRIDS]
    assert m.n_params == sum(g.n_params for _, g in grids)
    rng = np.random.default_rng(3)
    table = O.f2h(rng.uniform(-1, 1, m.n_params).astype(np.float32))
    x = rng.uniform(0, 1, (B, n_in)).astype(np.float32)
    out = m.forward(x, table)
    assert not np.isnan(O.h2f(out)).any()
    dy16 = O.f2h(rng.standard_normal(out.shape).astype(np.float32))
    dx, grad = m.backward(dy16)
    assert not np.isnan(dx).any() and not np.isnan(grad).any()
    off = 0
    for p, g in grids:  # the tables lie in nested order
        pos = np.ascontiguousarray(x[:, p["in_col"]:p["in_col"] + p["n_in"]])
        tab = table[off:off + g.n_params]
        np.testing.assert_array_equal(out[:, R.value_columns(p)], O.grid_fwd(g, pos, tab).T)
        np.testing.assert_array_equal(out[:, R.pad_columns(p)], 0)
        dy_soa = np.ascontiguousarray(dy16[:, R.value_columns(p)].T)
        ref = O.grid_bwd(g, pos, dy_soa).astype(np.float64)
        tol = O.grid_grad_tolerance(g, pos, dy_soa, ref) + 2.0 ** -11 * np.abs(ref) + 2.0 ** -25
        r = np.abs(grad[off:off + g.n_params] - ref) / tol
        assert r.max() <= 1.0, (p["kind"], off, r.max(), int(r.argmax()))
        np.testing.assert_allclose(dx[:, p["in_col"]:p["in_col"] + p["n_in"]], O.grid_bwd_input(g, pos, tab, dy_soa), rtol=1e-5, atol=1e-5)
        off += g.n_params
    for p, n in zip(parts, nested):
        xs = np.ascontiguousarray(x[:, p["in_col"]:p["in_col"] + p["n_in"]])
        if p["kind"] == "sphericalharmonics":
            deg = n.get("degree", 4)
            dirs = 2.0 * xs.astype(np.float64) - 1.0
            got = O.h2f(out[:, R.value_columns(p)]).astype(np.float64)
            ref, M = R.sh_reference(dirs, deg), R.sh_reference(dirs, deg, absolute=True)
            assert np.all(np.abs(got - ref) <= ulp_fp16(ref) + 64 * 2.0 ** -24 * M)
            np.testing.assert_array_equal(O.h2f(out[:, R.pad_columns(p)]), 1.0)
            gref, bound, _ = sh_input_gradient_reference(dirs, deg, O.h2f(dy16[:, R.value_columns(p)]).astype(np.float64))
            assert np.all(np.abs(dx[:, p["in_col"]:p["in_col"] + 3] - gref) <= bound)
        elif p["kind"] == "oneblob":
            np.testing.assert_array_equal(out[:, R.value_columns(p)], O.oneblob_fwd(xs, n["n_bins"]))
            np.testing.assert_array_equal(O.h2f(out[:, R.pad_columns(p)]), 1.0)
    m.close()
    return parts


def test_composite_sh_then_wide_feature_grid(torch_mod):
    parts = check_grid_parts(torch_mod, 6, [dict(SH3, degree=2), dict(GRID3_F4)], 16)
    assert [(p["out_col"], p["width"]) for p in parts] == [(0, 4), (4, 28)]


def test_composite_grid_then_sh(torch_mod):
    parts = check_grid_parts(torch_mod, 5, [dict(GRID2_L8, n_dims_to_encode=2), dict(SH3, degree=3)], 16)
    assert [(p["out_col"], p["width"]) for p in parts] == [(0, 16), (16, 16)]


def test_composite_two_grids_and_oneblob(torch_mod):
    nested = [dict(GRID2_L4, n_dims_to_encode=2), dict(GRID3_L4, n_dims_to_encode=3), {"otype": "OneBlob", "n_bins": 4}]
    parts = check_grid_parts(torch_mod, 7, nested, 16)
    assert [(p["out_col"], p["width"]) for p in parts] == [(0, 8), (8, 8), (16, 16)]


# ---------------------------------------------------------------------------------------------
# 6, 7: network gradients per element
# ---------------------------------------------------------------------------------------------
def btf_encoding(n_levels):
    enc = json.loads(json.dumps(CONFIG_BTF["encoding"]))
    enc["nested"][0]["n_levels"] = n_levels
    return enc


@pytest.mark.parametrize("n_levels,engine", [(16, "fused"), (8, "layered")])
def test_network_gradients_per_element(torch_mod, n_levels, engine):
    """config_btf (16 grid levels: encoded width 64, the tile engine) and the same model with 8 levels
    (width 48, which the tile kernel does not take: the layer-wise engine), C-ABI forward / backward with
    an external dL/dout, on the first 256 of 512 candidates clear of the ReLU boundaries
    (helpers.relu_margin_ok). The oracle MLP runs on the rows the engine's own Encoding module produced
    (checked by the tests above). Output within 4 fp16 ulps; dW per element (helpers.assert_wgrad_per_element,
    plus the fp16 rounding of the module's fp16 gradient output); grid gradient within
    helpers.trainer_grad_bounds' bound (grid tolerance + 8 fp16 ulps of the abs-backprop sum) on the
    grid's slice of dL/d(encoding); dL/dinput of the SH columns: the oracle's dL/d(encoding) through the
    SH gradient reference, within its 2^-18 bound plus 8 * 2^-10 of the abs-backprop magnitude
    sum_j |dL/d(encoding)_j|_abs 2 |dY_j/dd|."""
    enc, net = btf_encoding(n_levels), CONFIG_BTF["network"]
    parts, IN = R.composite_layout(8, enc, 16)
    W, NH = 64, 2
    net_m = Mod(torch_mod, 8, enc, net=net, n_out=3)
    enc_m = Mod(torch_mod, 8, enc, alignment=16)
    assert net_m.lib.tcnn_module_engine(net_m.h).decode() == engine
    assert enc_m.width == IN == 32 * n_levels // 16 + 32
    nm = O.mlp_n_params(W, IN, NH, 16)
    assert net_m.n_params == nm + enc_m.n_params
    p16 = O.f2h(net_m.initial_params(1337))
    cand = O.generate_uniform(O.pcg32(77), 512 * 8).reshape(512, 8)
    rows = enc_m.forward(cand, p16[nm:])
    ok = relu_margin_ok(W, IN, NH, p16[:nm], O.h2f(rows), check_output=False)
    assert ok.sum() >= 256, ok.sum()
    idx = np.nonzero(ok)[0][:256]
    x, rows = np.ascontiguousarray(cand[idx]), np.ascontiguousarray(rows[idx])
    rng = np.random.default_rng(12)
    dout = np.zeros((256, 16), np.float32)
    dout[:, :3] = rng.standard_normal((256, 3))
    dout16 = O.f2h(dout)

    out = net_m.forward(x, p16)
    dx, grad = net_m.backward(dout16)

    ref_out, hidden = O.mlp_fwd(W, IN, NH, 16, p16[:nm], rows, input_soa=False)
    assert_within_fp16_ulps(O.h2f(out), O.h2f(ref_out))
    wref, denc = O.mlp_bwd(W, IN, NH, 16, p16[:nm], rows, hidden, dout16, input_soa=False)
    mag, denc_abs = O.mlp_wgrad_magnitude(W, IN, NH, 16, p16[:nm], rows, hidden, dout16, input_soa=False, want_dinput=True)
    assert_wgrad_per_element(grad[:nm], wref, mag, fp16_out=True)

    gp = parts[0]
    g = O.grid_cfg(enc["nested"][0], 2)
    pos = np.ascontiguousarray(x[:, :2])
    denc_soa = np.ascontiguousarray(denc[:, R.value_columns(gp)].T)
    abs_soa = np.ascontiguousarray(denc_abs[:, R.value_columns(gp)].T)
    gref = O.grid_bwd(g, pos, denc_soa).astype(np.float64)
    absum, _ = O.grid_bwd_stats(g, pos, abs_soa)
    bound = O.grid_grad_tolerance(g, pos, denc_soa, gref) + 8 * 2.0 ** -10 * absum.astype(np.float64)
    bound += 2.0 ** -11 * np.abs(gref) + 2.0 ** -25  # the module's gradient output is fp16
    r = np.abs(grad[nm:] - gref) / (bound + 1e-30)
    assert r.max() <= 1.0, ("grid", r.max(), int(r.argmax()))

    for p in parts[1:]:
        dirs = 2.0 * x[:, p["in_col"]:p["in_col"] + 3].astype(np.float64) - 1.0
        ref, b18, J = sh_input_gradient_reference(dirs, 4, O.h2f(denc[:, R.value_columns(p)]).astype(np.float64))
        babs = 8 * 2.0 ** -10 * np.einsum("nj,njc->nc", O.h2f(denc_abs[:, R.value_columns(p)]).astype(np.float64), 2.0 * np.abs(J))
        r = np.abs(dx[:, p["in_col"]:p["in_col"] + 3] - ref) / (b18 + babs + 1e-30)
        assert r.max() <= 1.0, ("sh dinput", p["in_col"], r.max())
    net_m.close()
    enc_m.close()


# ---------------------------------------------------------------------------------------------
# 8: trainer
# ---------------------------------------------------------------------------------------------
def btf_batch(B, seed=31):
    x = O.generate_uniform(O.pcg32(seed), B * 8).reshape(B, 8)
    d = 2.0 * x[:, 2:5] - 1.0
    t = np.stack([0.5 + 0.4 * np.sin(7 * x[:, 0]) * d[:, 2], 0.5 + 0.4 * x[:, 1] * d[:, 0], 0.3 + 0.5 * x[:, 5] * x[:, 6]], axis=1)
    return np.ascontiguousarray(x), np.ascontiguousarray(t.astype(np.float32))


def test_trainer_config_btf(torch_mod):
    """Initial parameters bit-equal to xavier MLP then uniform +-1e-4 grid from the continuing pcg32
    stream; one loss-driven step on 512 samples: loss within 1e-3 relative, gradient relative L2
    <= 2e-3 for the MLP and for the grid (the bounds of tests/test_gpu_layered.py for W64 / W128);
    then 8 optimizer steps: the loss falls and the parameters equal oracle.adam_step applied to the
    engine's own fp16 gradients bit for bit."""
    torch = torch_mod
    from tinycudann import Trainer
    t = Trainer(8, 3, CONFIG_BTF, seed=1337)
    assert t.engine == "fused"
    W, IN, NH = 64, 64, 2
    nm = O.mlp_n_params(W, IN, NH, 16)
    g = O.grid_cfg(CONFIG_BTF["encoding"]["nested"][0], 2)
    assert t.n_params == nm + g.n_params
    rng = O.pcg32(int(O.seed_seq([1337], 2)[0]))
    w32 = np.empty(t.n_params, np.float32)
    off = 0
    for rows, cols in ((W, IN), (W, W), (16, W)):
        O.lib().orc_xavier_uniform(ctypes.byref(rng), rows, cols, w32[off:].ctypes.data_as(ctypes.c_void_p), 1.0)
        off += rows * cols
    w32[nm:] = O.generate_uniform(rng, g.n_params, -1e-4, 1e-4)
    a = trainer_arrays(t)
    np.testing.assert_array_equal(a["w32"].view(np.uint32), w32.view(np.uint32))
    np.testing.assert_array_equal(a["w16"], O.f2h(w32))

    B = 512
    x, tgt = btf_batch(B)
    xd, td = torch.from_numpy(x).cuda(), torch.from_numpy(tgt).cuda()
    t.training_step(xd, td, run_optimizer=False)
    loss = t.loss()
    a = trainer_arrays(t)
    enc_m = Mod(torch, 8, CONFIG_BTF["encoding"], alignment=16)
    rows = enc_m.forward(x, a["w16"][nm:])
    enc_m.close()
    out16, hidden = O.mlp_fwd(W, IN, NH, 16, a["w16"][:nm], rows, input_soa=False)
    loss_ref, dout, _ = O.relative_l2(out16, tgt)
    assert abs(loss - loss_ref) <= 1e-3 * abs(loss_ref), (loss, loss_ref)
    wref, denc = O.mlp_bwd(W, IN, NH, 16, a["w16"][:nm], rows, hidden, dout, input_soa=False)
    gref = O.grid_bwd(g, np.ascontiguousarray(x[:, :2]), np.ascontiguousarray(denc[:, :32].T))
    e_mlp, e_grid = rel_err(a["g32"][:nm], wref), rel_err(a["g32"][nm:], gref)
    print("trainer gradient relative L2: mlp", e_mlp, "grid", e_grid)
    assert e_mlp <= 2e-3, e_mlp
    assert e_grid <= 2e-3, e_grid

    adam = O.adam_cfg(CONFIG_BTF["optimizer"])
    w32, w16 = a["w32"].copy(), a["w16"].copy()
    m1 = np.zeros(t.n_params, np.float32); m2 = np.zeros_like(m1); steps = np.zeros(t.n_params, np.uint32)
    losses = []
    for s in range(8):
        t.training_step(xd, td, run_optimizer=True)
        losses.append(t.loss())
        a = trainer_arrays(t)
        O.adam_step(adam, nm, 128.0, s + 1, w32, w16, a["g16"], m1, m2, steps)
        np.testing.assert_array_equal(a["w32"].view(np.uint32), w32.view(np.uint32))
        np.testing.assert_array_equal(a["w16"], w16)
    assert losses[-1] < losses[0], losses


# ---------------------------------------------------------------------------------------------
# 10: front-ends
# ---------------------------------------------------------------------------------------------
def test_torch_modules_and_pickle(torch_mod, sh_points):
    torch = torch_mod
    import tinycudann as tcnn
    torch.manual_seed(0)
    model = tcnn.NetworkWithInputEncoding(8, 3, CONFIG_BTF["encoding"], CONFIG_BTF["network"])
    x = torch.rand(256, 8, device="cuda", requires_grad=True)
    y = model(x)
    assert y.shape == (256, 3)
    y.float().square().sum().backward()
    assert torch.isfinite(x.grad).all() and x.grad[:, 2:].abs().sum() > 0
    assert torch.isfinite(model.params.grad).all() and model.params.grad.abs().sum() > 0
    clone = pickle.loads(pickle.dumps(model))
    with torch.no_grad():
        assert torch.equal(clone(x.detach()), model(x.detach()))

    # tinycudann.Encoding of an SH composite with requires_grad inputs: the bound of test_sh_input_gradient
    pts, dirs = sh_points
    enc = tcnn.Encoding(3, {"otype": "Composite", "nested": [{"otype": "SphericalHarmonics", "degree": 4}]})
    xs = torch.from_numpy(pts).cuda().requires_grad_(True)
    out = enc(xs)
    dy16 = O.f2h(np.random.default_rng(4).standard_normal((257, 16)).astype(np.float32))
    out.backward(torch.from_numpy(dy16.view(np.float16)).cuda().to(out.dtype))
    ref, bound, _ = sh_input_gradient_reference(dirs, 4, O.h2f(dy16).astype(np.float64))
    # the autograd function scales dL/dy by the loss scale 128 in fp16 and divides dL/dx by it in
    # fp32: powers of two, exact unless a scaled fp16 value overflows (|dy| < 6 here)
    assert np.all(np.abs(xs.grad.cpu().numpy() - ref) <= bound)


def test_trainer_snapshots(torch_mod):
    """json and msgpack snapshots of a composite trainer restore identical outputs"""
    torch = torch_mod
    from tinycudann import Trainer
    from tinycudann import _lib as L
    lib = L.lib()
    t = Trainer(8, 3, CONFIG_BTF, seed=5)
    x, tgt = btf_batch(256, seed=3)
    xd, td = torch.from_numpy(x).cuda(), torch.from_numpy(tgt).cuda()
    for _ in range(3):
        t.training_step(xd, td)
    before = t.inference(xd).cpu().numpy()
    assert np.abs(before).max() > 0
    n = ctypes.c_uint64(0)
    L.check(lib.tcnn_trainer_serialize_json(t.h, 1, None, 0, ctypes.byref(n)))
    buf = ctypes.create_string_buffer(n.value)
    L.check(lib.tcnn_trainer_serialize_json(t.h, 1, buf, n.value, ctypes.byref(n)))
    text = buf.raw[:n.value]
    assert json.loads(text.decode().rstrip("\0")) is not None
    for snap in (text, t.serialize(optimizer=True)):
        t2 = Trainer(8, 3, CONFIG_BTF, seed=99)
        assert not np.array_equal(t2.inference(xd).cpu().numpy(), before)
        t2.deserialize(snap)
        np.testing.assert_array_equal(t2.inference(xd).cpu().numpy(), before)


# ---------------------------------------------------------------------------------------------
# 11: every encoding is a part list -- a lone encoding against its one-part Composite
# ---------------------------------------------------------------------------------------------
GRID2_L5 = {"otype": "HashGrid", "n_levels": 5, "n_features_per_level": 2, "log2_hashmap_size": 12, "base_resolution": 8,
            "per_level_scale": 1.5}
DENSE3_F4 = {"otype": "DenseGrid", "n_levels": 3, "n_features_per_level": 4, "base_resolution": 4, "per_level_scale": 2.0}
LONE = [(2, {"otype": "OneBlob", "n_bins": 64}, 0, 128),
        (3, {"otype": "OneBlob", "n_bins": 16}, 32, 64),
        (3, {"otype": "Identity", "scale": 1.5, "offset": -0.25}, 16, 16),
        (2, GRID2_L5, 0, 10),
        (3, DENSE3_F4, 0, 12)]


@pytest.mark.parametrize("n_in,enc,alignment,width", LONE, ids=["oneblob64", "oneblob16_padded", "identity_padded", "hashgrid", "densegrid"])
def test_lone_encoding_equals_one_part_composite(torch_mod, n_in, enc, alignment, width):
    """X alone runs its own kernel (encodings.hip, grid.hip), {"otype": "Composite", "nested": [X]} the
    composite kernels: forward, dL/dinput and dL/dparams are bit-equal at B = 1000 (not a multiple of 64
    or 256: the kernels' tails run). OneBlob and Identity evaluate the same fp32 operation sequence in
    both; the grid kernels are the same, and the grid backward sums in integers in LDS."""
    lone = Mod(torch_mod, n_in, enc, alignment=alignment)
    comp = Mod(torch_mod, n_in, {"otype": "Composite", "nested": [enc]}, alignment=alignment)
    assert lone.width == comp.width == width and lone.n_params == comp.n_params
    rng = np.random.default_rng(17)
    B = 1000
    x = rng.uniform(0, 1, (B, n_in)).astype(np.float32)
    table = O.f2h(rng.uniform(-1, 1, lone.n_params).astype(np.float32)) if lone.n_params else None
    dy16 = O.f2h(rng.standard_normal((B, width)).astype(np.float32))
    got = []
    for m in (lone, comp):
        out = m.forward(x, table)
        dx, grad = m.backward(dy16)
        assert not np.isnan(O.h2f(out)).any() and not np.isnan(dx).any()
        got.append((out, dx, grad))
        m.close()
    np.testing.assert_array_equal(got[0][0], got[1][0])
    np.testing.assert_array_equal(got[0][1].view(np.uint32), got[1][1].view(np.uint32))
    if lone.n_params:
        assert not np.isnan(got[0][2]).any() and np.abs(got[0][2]).max() > 0
        np.testing.assert_array_equal(got[0][2].view(np.uint32), got[1][2].view(np.uint32))


def test_lone_encodings_keep_no_table_limits(torch_mod):
    """The composite kernels' table limits (64 input dims, 256 columns) do not bind a lone Identity or
    OneBlob: 80 input dims, and 7 dims x 64 bins = 448 columns. Forward bit-equal to the oracle (Identity:
    fp16(fma(x, scale, offset))), dL/dinput against the oracle (Identity: the reference's statement) to the
    tolerance of test_gpu_layered.py's test_oneblob_encoding_bit_exact (rtol = atol = 1e-5)."""
    rng = np.random.default_rng(23)
    B = 300
    x = rng.uniform(0, 1, (B, 80)).astype(np.float32)
    m = Mod(torch_mod, 80, {"otype": "Identity", "scale": 0.75, "offset": 0.125})
    assert m.width == 80
    np.testing.assert_array_equal(m.forward(x), O.identity_fwd(x, 0.75, 0.125))
    dy16 = O.f2h(rng.standard_normal((B, 80)).astype(np.float32))
    dx, _ = m.backward(dy16)
    # identity.h:84: dL/dx = (T)((float)dL/dy * scale), the fp32 product (exact: 11 x 2 significant bits) rounded to fp16
    np.testing.assert_allclose(dx, O.h2f(O.f2h(0.75 * O.h2f(dy16))), rtol=1e-5, atol=1e-5)
    m.close()

    x = rng.uniform(0, 1, (B, 7)).astype(np.float32)
    m = Mod(torch_mod, 7, {"otype": "OneBlob", "n_bins": 64})
    assert m.width == 448
    np.testing.assert_array_equal(m.forward(x), O.oneblob_fwd(x, 64))
    dy16 = O.f2h(rng.standard_normal((B, 448)).astype(np.float32))
    dx, _ = m.backward(dy16)
    np.testing.assert_allclose(dx, O.oneblob_bwd(x, 64, dy16), rtol=1e-5, atol=1e-5)
    m.close()


def test_padded_lone_grid_through_network(torch_mod):
    """A lone grid of 10 features under a W64/H2 network: the network's alignment 16 pads it with 6 zero
    columns and the model trains on the tile engine. One loss-driven step at B = 512 against
    oracle.OracleModel: the bounds of test_gpu_layered.py's test_layered_step_gradients_and_loss for
    W64 grid configs (loss 1e-3 relative, gradient relative L2 <= 1e-3 for the network and for the grid)."""
    from tinycudann import Trainer
    cfg = dict(CONFIG_HASH, encoding=GRID2_L5,
               network={"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": 64, "n_hidden_layers": 2})
    t = Trainer(2, 3, cfg, seed=1337)
    assert t.engine == "fused"
    om = O.OracleModel(cfg, 2, 3, seed=1337)
    nm = O.mlp_n_params(64, 16, 2, 16)
    assert t.n_params == om.n_params == nm + O.grid_cfg(GRID2_L5, 2).n_params and om.n_mlp_params == nm
    np.testing.assert_array_equal(trainer_arrays(t)["w16"], om.w16)
    pos, tgt = make_batch(512)
    t.training_step(torch_mod.from_numpy(pos).cuda(), torch_mod.from_numpy(tgt).cuda(), run_optimizer=False)
    loss, loss_ref = t.loss(), om.train_step(pos, tgt, run_optimizer=False, n_threads=4)
    assert abs(loss - loss_ref) <= 1e-3 * abs(loss_ref), (loss, loss_ref)
    g32 = trainer_arrays(t)["g32"]
    e_mlp, e_grid = rel_err(g32[:nm], om.grad32[:nm]), rel_err(g32[nm:], om.grad32[nm:])
    print("padded lone grid gradient relative L2: mlp", e_mlp, "grid", e_grid)
    assert e_mlp <= 1e-3, e_mlp
    assert e_grid <= 1e-3, e_grid


def test_encoding_module_names_and_hyperparams(torch_mod):
    """name() and hyperparams() of the six spellings (no kernel runs), and the alignment a lone grid refuses"""
    from tinycudann import _lib as L
    lib = L.lib()
    grid_hyper = {"otype": "Grid", "type": "Hash", "n_levels": 5, "n_features_per_level": 2, "base_resolution": 8, "per_level_scale": 1.5,
                  "interpolation": "Linear", "hash": "CoherentPrime", "log2_hashmap_size": 12}
    blob = {"otype": "OneBlob", "n_bins": 4}
    cases = [(2, GRID2_L5, "GridEncoding", grid_hyper),
             (2, blob, "OneBlobEncoding", blob),
             (3, {"otype": "Identity", "scale": 1.5, "offset": -0.25}, "IdentityEncoding", {"otype": "Identity", "scale": 1.5, "offset": -0.25}),
             (3, {"otype": "SphericalHarmonics", "degree": 3}, "SphericalHarmonicsEncoding", {"otype": "SphericalHarmonics", "degree": 3}),
             (2, {"otype": "TriangleWave", "n_frequencies": 5}, "TriangleWaveEncoding", {"otype": "TriangleWave", "n_frequencies": 5}),
             (2, {"otype": "Composite", "nested": [blob]}, "CompositeEncoding", {"otype": "Composite", "nested": [blob]})]
    for n_in, enc, name, hyper in cases:
        m = Mod(torch_mod, n_in, enc)
        assert lib.tcnn_module_name(m.h).decode() == name
        assert json.loads(lib.tcnn_module_hyperparams(m.h).decode()) == hyper
        m.close()
    assert not lib.tcnn_create_encoding_aligned(2, json.dumps(GRID2_L5).encode(), 1, 16)
    assert lib.tcnn_last_error().decode() == "create_encoding: a grid encoding module takes no alignment"
