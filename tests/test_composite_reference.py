"""CPU references for the Composite, SphericalHarmonics and TriangleWave encodings, and tests of the
references themselves (no GPU). tests/test_gpu_composite.py checks the HIP kernels against these.

  * sh_reference: real spherical harmonics as polynomials in three independent variables, in float64,
    written from the recurrences (not from generated polynomials):
        m = 0:  Y(l, 0)  = K(l, 0) P(l, 0)
        m > 0:  Y(l, m)  = sqrt(2) K(l, m) Re((x + iy)^m) P(l, m)
                Y(l, -m) = sqrt(2) K(l, m) Im((x + iy)^m) P(l, m)
        K(l, m) = sqrt((2l + 1) (l - m)! / (4 pi (l + m)!))
        P(m, m) = (-1)^m (2m - 1)!!,  P(m + 1, m) = (2m + 1) z P(m, m),
        P(l, m) = ((2l - 1) z P(l - 1, m) - (l + m - 1) P(l - 2, m)) / (l - m)
    at output index l^2 + l + m. absolute=True evaluates the same statement with every subtraction
    turned into an addition at (|x|, |y|, |z|): the sum of the magnitudes of the polynomial's terms,
    the scale of a rounding error of any evaluation order.
  * triangle_wave_reference: float32, one IEEE operation per step.
  * composite_layout: columns, widths and padding of a composite's parts.
"""
import json
import math
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _double_factorial(n):
    r = 1
    while n > 1:
        r *= n
        n -= 2
    return r


def sh_reference(d, degree, absolute=False):
    """d float64 [N, 3] (NOT normalised) -> float64 [N, degree^2]"""
    d = np.asarray(d, np.float64)
    x, y, z = (np.abs(d[:, i]) if absolute else d[:, i] for i in range(3))
    sub = (lambda p, q: p + q) if absolute else (lambda p, q: p - q)
    out = np.zeros((d.shape[0], degree * degree))
    a, b = np.ones_like(x), np.zeros_like(x)  # Re, Im of (x + iy)^m
    for m in range(degree):
        if m > 0:
            a, b = sub(a * x, b * y), a * y + b * x
        pmm = float(_double_factorial(2 * m - 1))
        if m % 2 == 1 and not absolute:
            pmm = -pmm
        p1 = p2 = None
        for l in range(m, degree):
            if l == m:
                p = np.full_like(x, pmm)
            elif l == m + 1:
                p = (2 * m + 1) * z * p1
            else:
                p = sub((2 * l - 1) * z * p1, (l + m - 1) * p2) / (l - m)
            K = math.sqrt((2 * l + 1) * math.factorial(l - m) / (4 * math.pi * math.factorial(l + m)))
            if m == 0:
                out[:, l * l + l] = K * p
            else:
                out[:, l * l + l + m] = math.sqrt(2.0) * K * a * p
                out[:, l * l + l - m] = math.sqrt(2.0) * K * b * p
            p2, p1 = p1, p
    return out


def sh_reference_jacobian(d, degree, absolute=False, h=1e-5):
    """central differences of sh_reference: float64 [N, degree^2, 3] = dY_j / d(x, y, z). With
    absolute=True (at |d|): the abs-sum of the terms of each derivative."""
    d = np.abs(np.asarray(d, np.float64)) if absolute else np.asarray(d, np.float64)
    J = np.empty((d.shape[0], degree * degree, 3))
    for c in range(3):
        e = np.zeros(3)
        e[c] = h
        J[:, :, c] = (sh_reference(d + e, degree, absolute) - sh_reference(d - e, degree, absolute)) / (2 * h)
    return J


def triangle_wave_reference(x, n_frequencies):
    """x float32 [B, D] -> (y float32 [B, D * n_frequencies], dy/dx float32 same shape); output
    j = dim * n_frequencies + k: v = x 2^(k-1) + k/4, y = |v - floor(v) - 1/2| 4 - 1, dy/dx = +-2^(k+1),
    negative when (int)floor(2v) is even. float32 throughout, one correctly rounded operation per step."""
    x = np.asarray(x, np.float32)
    B, D = x.shape
    y = np.empty((B, D * n_frequencies), np.float32)
    dydx = np.empty_like(y)
    for k in range(n_frequencies):
        v = np.ldexp(x, k - 1).astype(np.float32) + np.float32(0.25 * k)
        assert v.dtype == np.float32
        r = np.abs(v - np.floor(v) - np.float32(0.5)) * np.float32(4.0) - np.float32(1.0)
        assert r.dtype == np.float32
        even = np.floor(v * np.float32(2.0)).astype(np.int64) % 2 == 0
        y[:, k::n_frequencies] = r
        dydx[:, k::n_frequencies] = np.where(even, -1.0, 1.0) * 2.0 ** (k + 1)
    return y, dydx


GRIDS = ("grid", "hashgrid", "tiledgrid", "densegrid")


def _expand(enc):
    ot = enc.get("otype", "OneBlob").lower()
    if ot in ("nrc", "oneblobfrequency"):
        return {"otype": "Composite", "nested": [
            {"n_dims_to_encode": 3, "otype": "TriangleWave", "n_frequencies": enc.get("n_frequencies", 12)},
            {"n_dims_to_encode": 5, "otype": "OneBlob", "n_bins": enc.get("n_bins", 4)},
            {"otype": "Identity"}]}
    if ot != "composite":
        return {"otype": "Composite", "nested": [dict(enc)]}
    return enc


def composite_layout(n_dims, enc, alignment=1):
    """The parts of a composite (or of one encoding standing alone) over n_dims inputs: a list of dicts
    kind, in_col, n_in, out_col, width, n_values, pad_first, pad_value, align -- and the total width.
    Input ranges: a nested entry with n_dims_to_encode starts where the previous one ended, or at its
    dims_to_encode_begin; the single entry without n_dims_to_encode takes the dims the others leave
    (only when no entry names dims_to_encode_begin); empty entries vanish. Widths: a grid's is a
    multiple of its n_features_per_level, and so must its first column be; entry i is widened until
    entry i + 1 starts aligned, and the composite's own alignment widens the last entry. Padding: grid 0,
    OneBlob / Identity / TriangleWave 1 after the values, SphericalHarmonics 1 before them."""
    enc = _expand(enc)
    nested = enc["nested"]
    total = 0
    for n in nested:
        total += n.get("n_dims_to_encode", 0)
        if "dims_to_encode_begin" in n:
            total = None
            break
    rest = None if total is None else n_dims - total
    parts, off = [], 0
    for n in nested:
        if "n_dims_to_encode" in n:
            if "dims_to_encode_begin" in n:
                off = n["dims_to_encode_begin"]
            k = n["n_dims_to_encode"]
        else:
            assert rest is not None
            k, rest = rest, None
        if k > 0:
            ot = n.get("otype", "OneBlob").lower()
            if ot in GRIDS:
                F = n.get("n_features_per_level", 2)
                vals, align, pad_first, pad_value = n.get("n_levels", 16) * F, F, False, 0.0
            elif ot == "sphericalharmonics":
                vals, align, pad_first, pad_value = n.get("degree", 4) ** 2, 1, True, 1.0
            elif ot == "trianglewave":
                vals, align, pad_first, pad_value = k * n.get("n_frequencies", 12), 1, False, 1.0
            elif ot == "oneblob":
                vals, align, pad_first, pad_value = k * n.get("n_bins", 16), 1, False, 1.0
            else:
                assert ot == "identity", ot
                vals, align, pad_first, pad_value = k, 1, False, 1.0
            parts.append(dict(kind=ot, in_col=off, n_in=k, n_values=vals, align=align, pad_first=pad_first, pad_value=pad_value))
        off += k
    col = 0
    for i, p in enumerate(parts):
        a = parts[i + 1]["align"] if i + 1 < len(parts) else max(alignment, 1)
        p["out_col"] = col
        p["width"] = -(-(col + p["n_values"]) // a) * a - col
        col += p["width"]
    return parts, col


def value_columns(p):
    c0 = p["out_col"] + (p["width"] - p["n_values"] if p["pad_first"] else 0)
    return slice(c0, c0 + p["n_values"])


def pad_columns(p):
    c0 = p["out_col"] if p["pad_first"] else p["out_col"] + p["n_values"]
    return slice(c0, c0 + p["width"] - p["n_values"])


# ---------------------------------------------------------------------------------------------
# the references checked against known values
# ---------------------------------------------------------------------------------------------
def test_sh_spot_values():
    rng = np.random.default_rng(0)
    d = rng.uniform(-1, 1, (64, 3))
    x, y, z = d.T
    Y = sh_reference(d, 4)
    want = {
        1: -0.48860251190291987 * y,
        4: 1.0925484305920792 * x * y,
        6: 0.94617469575755997 * z * z - 0.31539156525251999,
        9: 0.59004358992664352 * y * (-3.0 * x * x + y * y),
        12: 0.37317633259011546 * z * (5.0 * z * z - 3.0),
        14: 1.4453057213202769 * z * (x * x - y * y),
    }
    for j, w in want.items():
        assert np.abs(Y[:, j] - w).max() <= 1e-14, (j, np.abs(Y[:, j] - w).max())


def test_sh_absolute_mode_bounds_the_value():
    rng = np.random.default_rng(1)
    d = rng.uniform(-1, 1, (256, 3))
    for deg in range(1, 9):
        assert np.all(sh_reference(d, deg, absolute=True) >= np.abs(sh_reference(d, deg)) * (1 - 1e-12))


def test_sh_orthonormal_on_the_sphere():
    # Gauss-Legendre in cos(theta) (24 nodes: exact to degree 47) x 48 equal steps in phi (exact for
    # trigonometric degree < 48); products of two degree-7 harmonics have degree 14
    mu, w = np.polynomial.legendre.leggauss(24)
    phi = (np.arange(48) + 0.5) * (2 * np.pi / 48)
    M, P = np.meshgrid(mu, phi, indexing="ij")
    s = np.sqrt(1 - M * M)
    d = np.stack([s * np.cos(P), s * np.sin(P), M], axis=-1).reshape(-1, 3)
    wq = np.repeat(w, 48) * (2 * np.pi / 48)
    Y = sh_reference(d, 8)
    G = (Y * wq[:, None]).T @ Y
    assert np.abs(G - np.eye(64)).max() <= 1e-13, np.abs(G - np.eye(64)).max()


def test_triangle_wave_reference_values():
    x = np.array([[0.0], [0.25], [0.5], [0.75]], np.float32)
    y, dy = triangle_wave_reference(x, 2)
    # k = 0: v = x / 2; k = 1: v = x + 1/4
    np.testing.assert_array_equal(y[:, 0], np.array([1.0, 0.5, 0.0, -0.5], np.float32))
    np.testing.assert_array_equal(y[:, 1], np.array([0.0, -1.0, 0.0, 1.0], np.float32))
    np.testing.assert_array_equal(dy[:, 0], np.array([-2.0, -2.0, -2.0, -2.0], np.float32))
    np.testing.assert_array_equal(dy[:, 1], np.array([-4.0, 4.0, 4.0, -4.0], np.float32))


def _widths(n_dims, enc, alignment):
    parts, total = composite_layout(n_dims, enc, alignment)
    return [p["width"] for p in parts], total, parts


def test_layout_config_btf():
    cfg = json.load(open(os.path.join(GOLD, "config_btf.json")))
    w, total, parts = _widths(8, cfg["encoding"], 16)
    assert w == [32, 16, 16] and total == 64
    assert [(p["in_col"], p["n_in"]) for p in parts] == [(0, 2), (2, 3), (5, 3)]


def test_layout_nrc_10_inputs():
    w, total, parts = _widths(10, {"otype": "NRC"}, 16)
    assert w == [36, 20, 8] and total == 64
    assert parts[2]["n_values"] == 2 and pad_columns(parts[2]) == slice(58, 64)


def test_layout_grid_then_sh():
    enc = {"otype": "Composite", "nested": [{"n_dims_to_encode": 2, "otype": "HashGrid", "n_levels": 8},
                                            {"otype": "SphericalHarmonics", "degree": 3}]}
    w, total, parts = _widths(5, enc, 16)
    assert w == [16, 16] and total == 32
    assert pad_columns(parts[1]) == slice(16, 23) and value_columns(parts[1]) == slice(23, 32)


def test_layout_sh_then_wide_feature_grid():
    enc = {"otype": "Composite", "nested": [{"n_dims_to_encode": 3, "otype": "SphericalHarmonics", "degree": 2},
                                            {"otype": "HashGrid", "n_levels": 4, "n_features_per_level": 4}]}
    w, total, parts = _widths(6, enc, 1)
    assert w == [4, 16] and parts[1]["out_col"] == 4 and total == 20
    # degree 3 (9 values) has to be widened to 12 for the grid's 4-feature alignment: padding first
    enc["nested"][0]["degree"] = 3
    w, total, parts = _widths(6, enc, 1)
    assert w == [12, 16] and pad_columns(parts[0]) == slice(0, 3) and parts[1]["out_col"] == 12


def test_layout_dims_to_encode_begin_counts_only_beside_n_dims():
    enc = {"otype": "Composite", "nested": [{"n_dims_to_encode": 2, "dims_to_encode_begin": 3, "otype": "Identity"},
                                            {"n_dims_to_encode": 1, "otype": "Identity"}]}
    parts, _ = composite_layout(6, enc)
    assert [(p["in_col"], p["n_in"]) for p in parts] == [(3, 2), (5, 1)]
