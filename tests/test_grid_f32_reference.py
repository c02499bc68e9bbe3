"""CPU reference of the fp32-precision grid encoding (csrc/grid_f32.hip) and tests of that reference.

A vectorised float64 numpy restatement of the multiresolution grid for any D: positions as the
single-rounded fmaf (float64(x) * float64(scale) + 0.5 rounded once to float32, as tests/test_fixtures.py
argues), floor and fraction (exact in float32), the corner indices of dense, tiled and hashed levels under
each of the three hashes (reference common_device.h:645-707), and float64 weights, interpolation sums and gradient
sums. tests/test_gpu_encoding_f32.py checks the fp32 kernels against it; here it is checked against the
oracle (the reference's fp16 arithmetic) on fp16-representable tables, where the two may differ only by
the fp16 roundings the oracle models.
"""
import numpy as np
import pytest

from oracle import oracle as O

# the three hashes' per-dimension factors (prime_hash, coherent_prime_hash, reversed_prime_hash,
# common_device.h:645-661; csrc/grid_device.h hash_prime), keyed by the oracle's hash_type
PRIMES = {
    0: (1958374283, 2654435761, 805459861, 3674653429),  # Prime
    1: (1, 2654435761, 805459861, 3674653429),           # CoherentPrime
    2: (2165219737, 1434869437, 2097192037, 3674653429),  # ReversedPrime
}
M32 = np.uint64(0xFFFFFFFF)

GRID2_L8 = {"otype": "HashGrid", "n_levels": 8, "n_features_per_level": 2, "log2_hashmap_size": 12, "base_resolution": 8,
            "per_level_scale": 1.5}
GRID3_F4 = {"otype": "HashGrid", "n_levels": 4, "n_features_per_level": 4, "log2_hashmap_size": 10, "base_resolution": 4,
            "per_level_scale": 1.5}
DENSE3_F1 = {"otype": "DenseGrid", "n_levels": 3, "n_features_per_level": 1, "base_resolution": 4, "per_level_scale": 1.5,
             "interpolation": "Smoothstep"}
TILED4_F8 = {"otype": "TiledGrid", "n_levels": 2, "n_features_per_level": 8, "base_resolution": 3, "per_level_scale": 2.0}
# (name, D, encoding): dense + hashed levels, wide features, Smoothstep on a dense grid, a tiled 4-D grid
GRID_CASES = [("grid2_l8", 2, GRID2_L8), ("grid3_f4", 3, GRID3_F4), ("dense3_f1_smooth", 3, DENSE3_F1), ("tiled4_f8", 4, TILED4_F8)]
# the other two hashes, pinned to the oracle below (CPU only: tests/test_gpu_grid_dispatch.py runs them on the GPU)
HASH_CASES = [(f"{name}_{h.lower()}", D, dict(enc, hash=h)) for name, D, enc in GRID_CASES[:2] for h in ("Prime", "ReversedPrime")]
PIN_CASES = GRID_CASES + HASH_CASES


def level_size(g, l):
    return int(g.offsets[l + 1] - g.offsets[l])


def grid_index(g, l, pg):
    """grid_index (common_device.h:690-707) of integer corner coordinates pg uint64 [B, D] on level l, in
    uint32 arithmetic: the dense stride loop while the stride fits the level, the hash where the level is
    hashed and smaller than the dense extent, then % size."""
    D = g.n_pos_dims
    size, res = level_size(g, l), int(g.res[l])
    stride, index = 1, np.zeros(pg.shape[0], np.uint64)
    for d in range(D):
        if stride > size:
            break
        index = (index + pg[:, d] * np.uint64(stride)) & M32
        stride = (stride * res) & 0xFFFFFFFF
    if g.grid_type == 0 and size < stride:
        index = np.zeros(pg.shape[0], np.uint64)
        for d in range(D):
            index ^= (pg[:, d] * np.uint64(PRIMES[int(g.hash_type)][d])) & M32
    return (index % np.uint64(size)).astype(np.int64)


def level_corners(g, l, pos):
    """Level l for positions pos float32 [B, D]: entry indices int64 [B, 2^D] (offset included), float64
    weights [B, 2^D] in the reference's corner order (bit d of the corner: coordinate d + 1, weight frac_d;
    grid.h:144-163), and S [B, 2^D] = sum_d s_d prod_{e != d} a_e, the sensitivity of the weight to the
    Smoothstep polynomial's value s_d (zero for Linear; see forward_bound)."""
    D = g.n_pos_dims
    B = pos.shape[0]
    scale = np.float64(np.float32(g.scales[l]))
    p = (pos.astype(np.float64) * scale + 0.5).astype(np.float32)  # one rounding == fmaf
    fl = np.floor(p)
    frac = (p - fl).astype(np.float64)  # exact
    pg = fl.astype(np.int64).astype(np.uint64)
    smooth = g.interpolation == 2
    s = frac * frac * (3.0 - 2.0 * frac) if smooth else frac
    NC = 1 << D
    if g.interpolation == 0:  # Nearest: the floor corner with weight 1
        idx = np.repeat((grid_index(g, l, pg) + int(g.offsets[l]))[:, None], NC, axis=1)
        w = np.zeros((B, NC))
        w[:, 0] = 1.0
        return idx, w, np.zeros((B, NC))
    idx = np.empty((B, NC), np.int64)
    w = np.ones((B, NC))
    S = np.zeros((B, NC))
    for c in range(NC):
        local = pg.copy()
        a = np.empty((B, D))
        for d in range(D):
            if c & (1 << d):
                local[:, d] += np.uint64(1)
                a[:, d] = s[:, d]
            else:
                a[:, d] = 1.0 - s[:, d]
        w[:, c] = np.prod(a, axis=1)
        if smooth:
            for d in range(D):
                S[:, c] += s[:, d] * np.prod(np.delete(a, d, axis=1), axis=1)
        idx[:, c] = grid_index(g, l, local) + int(g.offsets[l])
    return idx, w, S


def grid_forward(g, pos, table):
    """table: float [n_params]. Returns float64 (ref, A, E), each [B, L * F]: the interpolated features,
    A = sum_c |w_c| |v_c| and E = sum_c S_c |v_c| (forward_bound)."""
    L, F = g.n_levels, g.n_features_per_level
    B = pos.shape[0]
    t = np.asarray(table, np.float64).reshape(-1, F)
    ref, A, E = (np.zeros((B, L * F)) for _ in range(3))
    for l in range(L):
        idx, w, S = level_corners(g, l, pos)
        v = t[idx]  # [B, NC, F]
        ref[:, l * F:(l + 1) * F] = np.einsum("bc,bcf->bf", w, v)
        A[:, l * F:(l + 1) * F] = np.einsum("bc,bcf->bf", np.abs(w), np.abs(v))
        E[:, l * F:(l + 1) * F] = np.einsum("bc,bcf->bf", S, np.abs(v))
    return ref, A, E


def forward_bound(g, A, E):
    """Bound of |fp32 kernel - ref| per output (k_grid_fwd_f32 / encode_level_f32).

    Linear, c = 2D + 2^D + 1 units of 2^-24 A with A = sum_c |w_c| |v_c|: a weight is a product of D
    factors f_d or 1 - f_d -- the fraction f_d is exact, the D subtractions 1 - f_d round once each, up to D
    multiplications round once each (2D relative roundings of the weight); the chain of 2^D FMAs rounds
    once per corner, each rounding relative to a partial sum that A bounds; one unit for the second-order
    terms. Smoothstep replaces f_d by s_d = f_d^2 (3 - 2 f_d), computed as p * p * fma(-2, p, 3): 3
    roundings, an error of at most 3 * 2^-24 s_d in s_d -- ABSOLUTE for the factor 1 - s_d, so it is
    propagated through the weight instead of being counted relative to it: |dw_c| <= 3 * 2^-24 S_c with
    S_c = sum_d s_d prod_{e != d} a_e (a_e the factors of corner c), plus 2^-24 slack on that term for its
    own second order: the bound gains (3 + 1) * 2^-24 E, E = sum_c S_c |v_c|. Nearest is bit-exact."""
    D = g.n_pos_dims
    b = (2 * D + (1 << D) + 1) * 2.0 ** -24 * A
    if g.interpolation == 2:
        b = b + 4 * 2.0 ** -24 * E
    return b


def grid_gradient(g, pos, dy):
    """dy: float [B, L * F] (AoS). Returns float64 [n_params] arrays: the gradient sum_i w dy, count_p (the
    number of updates an element receives), absum = sum |w dy|, esum = sum S |dy| (Smoothstep term), and
    S_level [L] = sum_i max_f |dy_i,f|."""
    L, F = g.n_levels, g.n_features_per_level
    dy = np.asarray(dy, np.float64)
    grad, count, absum, esum = (np.zeros(g.n_params) for _ in range(4))
    S_level = np.zeros(L)
    for l in range(L):
        idx, w, S = level_corners(g, l, pos)
        d = dy[:, l * F:(l + 1) * F]
        S_level[l] = np.abs(d).max(axis=1).sum()
        nz = w != 0.0 if g.interpolation == 0 else np.ones_like(w, bool)  # Nearest: one update per point
        for f in range(F):
            e = (idx * F + f)[nz]
            np.add.at(grad, e, (w * d[:, f:f + 1])[nz])
            np.add.at(count, e, 1.0)
            np.add.at(absum, e, np.abs(w * d[:, f:f + 1])[nz])
            np.add.at(esum, e, (S * np.abs(d[:, f:f + 1]))[nz])
    return grad, count, absum, esum, S_level


def gradient_bound(g, ref, count, absum, esum, S_level):
    """Per-element bound of |fp32 kernel gradient - ref| (k_grid_bwd_lds_f32), oracle.grid_grad_tolerance
    restated for fp32 weights and fp32 dL/dy:
      count_p * 2^-29.9 * S_level   every update is rounded to the item's int32 fixed point, whose step is at
                                    most 2^-29.9 times the chunk's sum of max_f |dL/dy| <= S_level
      (count_p + 2D + 1) * 2^-24 * sum |w dy|   the fp32 weight (2D roundings, as forward_bound), the rounding
                                    of the product w * dy, and the int32 -> fp32 conversion and fixed-order
                                    fp32 sum of the chunk slabs (at most one rounding per update)
      2^-23 |ref|                   the last rounding of the stored value
    and for Smoothstep the polynomial's 3 roundings propagated absolutely as in forward_bound:
    4 * 2^-24 * sum S |dy|."""
    L, F, D = g.n_levels, g.n_features_per_level, g.n_pos_dims
    tol = np.zeros(g.n_params)
    for l in range(L):
        a, b = int(g.offsets[l]) * F, int(g.offsets[l + 1]) * F
        tol[a:b] = count[a:b] * S_level[l] * 2.0 ** -29.9
    tol += (count + 2 * D + 1) * 2.0 ** -24 * absum + 2.0 ** -23 * np.abs(ref)
    if g.interpolation == 2:
        tol += 4 * 2.0 ** -24 * esum
    return tol


def make_inputs(g, B, seed):
    """positions in [0, 1)^D, a uniform(-1, 1) float32 table (not fp16-representable), standard-normal dL/dy"""
    rng = np.random.default_rng(seed)
    pos = rng.uniform(0, 1, (B, g.n_pos_dims)).astype(np.float32)
    table = rng.uniform(-1, 1, g.n_params).astype(np.float32)
    dy = rng.standard_normal((B, g.n_levels * g.n_features_per_level)).astype(np.float32)
    return pos, table, dy


# ---------------------------------------------------------------------------------------------
# the reference against the oracle
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,D,enc", PIN_CASES, ids=[c[0] for c in PIN_CASES])
def test_reference_forward_matches_oracle(name, D, enc):
    """On an fp16-representable table the oracle (the reference's fp16 arithmetic) and the float64
    restatement touch the same entries and differ only by the oracle's fp16 roundings: each of the 2^D
    weights is rounded to fp16 (2^-11 relative, or 2^-25 absolute in the subnormals) and each of the 2^D
    fp16 FMAs rounds its partial sum (2^-11 of a value A bounds, or 2^-25): (2^D + 1) * 2^-11 * A, widened
    by 1 % for the second order and the fp32 weight error, plus 2^-25 * (sum_c |v_c| + 2^D); for Smoothstep
    the fp32 polynomial's error (forward_bound's E term)."""
    g = O.grid_cfg(enc, D)
    pos, table, _ = make_inputs(g, 257, 1)
    t16 = O.f2h(table)
    t = O.h2f(t16)
    got = O.h2f(O.grid_fwd(g, pos, t16)).T.astype(np.float64)
    ref, A, E = grid_forward(g, pos, t)
    L, F, NC = g.n_levels, g.n_features_per_level, 1 << D
    vsum = np.zeros_like(ref)
    tt = np.abs(t.astype(np.float64)).reshape(-1, F)
    for l in range(L):
        idx, _, _ = level_corners(g, l, pos)
        vsum[:, l * F:(l + 1) * F] = tt[idx].sum(axis=1)
    bound = (NC + 1) * 2.0 ** -11 * A * 1.01 + 2.0 ** -25 * (vsum + NC) + 4 * 2.0 ** -24 * E
    r = np.abs(got - ref) / bound
    print(name, "oracle vs float64 reference: max error / bound", r.max())
    assert r.max() <= 1.0
    assert np.abs(got - ref).max() > 0  # the comparison is not vacuous: fp16 arithmetic does differ


@pytest.mark.parametrize("name,D,enc", PIN_CASES, ids=[c[0] for c in PIN_CASES])
def test_reference_gradient_matches_oracle(name, D, enc):
    """The oracle's backward adds fp32(w16 * dy16) sequentially in fp32: against the float64 sums it is
    off by the fp16 rounding of each weight (2^-11 |w dy|, or 2^-25 |dy| in the subnormals) and by its
    fp32 additions and products ((count + 1) * 2^-24 * sum |w dy|). Same entries, same counts."""
    g = O.grid_cfg(enc, D)
    pos, _, dy = make_inputs(g, 257, 2)
    dy16 = O.f2h(dy)
    dyh = O.h2f(dy16)
    got = O.grid_bwd(g, pos, np.ascontiguousarray(dy16.T)).astype(np.float64)
    ref, count, absum, esum, _ = grid_gradient(g, pos, dyh)
    _, ocount = O.grid_bwd_stats(g, pos, np.ascontiguousarray(dy16.T))
    if g.interpolation != 0:
        np.testing.assert_array_equal(ocount, count)  # the same entries are touched, as often
    dsum = np.zeros(g.n_params)
    F = g.n_features_per_level
    for l in range(g.n_levels):
        idx, w, _ = level_corners(g, l, pos)
        for f in range(F):
            np.add.at(dsum, idx * F + f, np.abs(dyh[:, l * F + f:l * F + f + 1]) * np.ones_like(w))
    bound = 2.0 ** -11 * absum * 1.01 + 2.0 ** -25 * dsum + (count + 1) * 2.0 ** -24 * absum + 4 * 2.0 ** -24 * esum
    r = np.abs(got - ref) / np.maximum(bound, 1e-300)
    assert r[count > 0].max() <= 1.0, (name, r.max())
    assert np.all(got[count == 0] == 0) and np.all(ref[count == 0] == 0)


def test_cases_cover_dense_hashed_and_tiled_levels():
    kinds = set()
    for _, D, enc in GRID_CASES:
        g = O.grid_cfg(enc, D)
        for l in range(g.n_levels):
            full = int(g.res[l]) ** D
            size = level_size(g, l)
            kinds.add("hashed" if g.grid_type == 0 and size < full else ("tiled" if size < full else "dense"))
    assert kinds == {"hashed", "dense", "tiled"}
