"""The grid backward's streaming pre-pass (grid_bwd_lds.h): the fused kernel emits per-slice sums of
max_f |dL/denc| (dy_bound), the grid backward takes its fixed-point scale from them and streams dL/dy
under the accumulation -- and falls back to the exact pre-pass wherever the guard of grid_bwd_scale.h
cannot prove the same exponent. Everything must stay bit-identical to TCNN_GRID_BWD_STREAM=0."""
import ctypes

import numpy as np
import pytest

from helpers import CONFIG_HASH, bits, make_batch, trainer_arrays

pytestmark = pytest.mark.gpu

N_LEVELS = CONFIG_HASH["encoding"]["n_levels"]


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def dbg():
    """the test-only entries of csrc/debug_grid_bwd.h; fallback counting on for this module"""
    from tinycudann import _lib as L
    lib = L.lib()
    vp, u32p = ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32)
    lib.tcnn_debug_grid_bwd_count_fallbacks.argtypes = [ctypes.c_int]
    lib.tcnn_debug_grid_bwd_fallbacks.argtypes = [u32p]
    lib.tcnn_debug_step_dldenc.argtypes = [vp, vp, ctypes.c_size_t, vp, ctypes.c_size_t, ctypes.POINTER(ctypes.c_int)]
    lib.tcnn_debug_grid_backward_items.argtypes = [vp, vp, ctypes.c_uint32, vp, vp, vp, vp, ctypes.c_size_t, u32p, u32p]
    for f in ("tcnn_debug_grid_bwd_count_fallbacks", "tcnn_debug_grid_bwd_fallbacks", "tcnn_debug_step_dldenc",
              "tcnn_debug_grid_backward_items"):
        getattr(lib, f).restype = ctypes.c_int
    L.check(lib.tcnn_debug_grid_bwd_count_fallbacks(1))
    yield lib
    L.check(lib.tcnn_debug_grid_bwd_count_fallbacks(0))


def _fallbacks(lib):
    from tinycudann import _lib as L
    n = ctypes.c_uint32(0)
    L.check(lib.tcnn_debug_grid_bwd_fallbacks(ctypes.byref(n)))
    return n.value


def _trainer(monkeypatch, stream):
    """the switch is read when the engine is built (as TCNN_NO_TILE_ENGINE in test_gpu_layered.py)"""
    from tinycudann import Trainer
    if stream:
        monkeypatch.delenv("TCNN_GRID_BWD_STREAM", raising=False)
    else:
        monkeypatch.setenv("TCNN_GRID_BWD_STREAM", "0")
    t = Trainer(2, 3, CONFIG_HASH, seed=1337)
    monkeypatch.delenv("TCNN_GRID_BWD_STREAM", raising=False)
    assert t.engine == "fused"
    return t


def _batch(B, step, outside):
    pos, tgt = make_batch(B, step=step)
    if outside:  # 0.2 % of the positions outside [0, 1]: the generic per-corner path
        rng = np.random.default_rng(7 + step)
        idx = rng.choice(B, max(1, B // 500), replace=False)
        pos[idx] += rng.choice(np.array([-0.7, 1.5], np.float32), (idx.size, 1))
    return pos, tgt


def _assert_same(a, b, what):
    for k in ("w32", "w16", "g16", "g32"):
        x, y = bits(a[k]), bits(b[k])
        bad = np.flatnonzero(x != y)
        assert bad.size == 0, (what, k, int(bad.size), int(bad[0]), hex(int(x[bad[0]])), hex(int(y[bad[0]])))


@pytest.mark.parametrize("outside", [False, True])
@pytest.mark.parametrize("B", [256, 16384, 65792])
def test_three_steps_bit_identical_to_stream_off(torch_mod, dbg, monkeypatch, B, outside):
    """B = 256: one chunk of 8 slices (most threads read no slice sum); 16384: 2 chunks (slab sums in
    Adam); 65792: 8 chunks of 257 slices (partial last batch, waves with two slices)."""
    torch = torch_mod
    new, old = _trainer(monkeypatch, True), _trainer(monkeypatch, False)
    for s in range(3):
        pos, tgt = _batch(B, s, outside)
        p, g = torch.from_numpy(pos).cuda(), torch.from_numpy(tgt).cuda()
        old.training_step(p, g)
        assert _fallbacks(dbg) == 0  # no slice sums given: nothing to fall back from
        new.training_step(p, g)
        n_fb = _fallbacks(dbg)
        print(f"B {B} outside {outside} step {s}: {n_fb} fallback workgroups")
        assert np.float32(new.loss()).view(np.uint32) == np.float32(old.loss()).view(np.uint32)
        _assert_same(trainer_arrays(new), trainer_arrays(old), (B, outside, s))


def test_nan_target_gives_nan_gradient_through_the_fallback(torch_mod, dbg, monkeypatch):
    torch = torch_mod
    B = 16384
    new, old = _trainer(monkeypatch, True), _trainer(monkeypatch, False)
    pos, tgt = make_batch(B)
    tgt[4321, 1] = np.nan
    p, g = torch.from_numpy(pos).cuda(), torch.from_numpy(tgt).cuda()
    old.training_step(p, g)
    new.training_step(p, g)
    assert _fallbacks(dbg) >= 1  # the non-finite slice sum sends its workgroups to the exact pre-pass
    a, b = trainer_arrays(new), trainer_arrays(old)
    assert np.isnan(b["g32"]).any() and np.isnan(a["g32"]).any()
    _assert_same(a, b, "nan target")


@pytest.mark.parametrize("B", [256, 65792])
def test_emitted_slice_sums(torch_mod, dbg, monkeypatch, B):
    """Each dy_bound entry is the fp32 sum of its slice's 32 per-sample max_f |dL/denc|, added as one
    pair add and a 4-level tree: 5 roundings on every path, all terms >= 0, so it lies within
    (1 + 2^-24)^5 - 1 < 5.0001 * 2^-24 relative of the real sum. Every slice of every level is written."""
    torch = torch_mod
    from tinycudann import _lib as L
    t = _trainer(monkeypatch, True)
    pos, tgt = make_batch(B)
    t.training_step(torch.from_numpy(pos).cuda(), torch.from_numpy(tgt).cuda())
    w = np.empty((N_LEVELS, B), np.uint32)
    bound = np.full((N_LEVELS, B // 32), -1.0, np.float32)
    live = ctypes.c_int(0)
    L.check(dbg.tcnn_debug_step_dldenc(t.h, w.ctypes.data, w.nbytes, bound.ctypes.data, bound.nbytes, ctypes.byref(live)))
    assert live.value == 1
    mb = np.maximum(w & 0x7fff, (w >> 16) & 0x7fff).astype(np.uint16)
    assert (mb < 0x7c00).all()  # finite dL/denc on this batch
    s = mb.view(np.float16).astype(np.float64).reshape(N_LEVELS, B // 32, 32).sum(axis=2)
    assert (s > 0).mean() > 0.99  # (an unwritten entry could not hide behind a zero sum)
    err = np.abs(bound.astype(np.float64) - s)
    tol = 5.0001 * 2.0 ** -24 * s
    k = np.unravel_index(np.argmax(err - tol), err.shape)
    print(f"B {B}: max err / tol = {float((err / np.maximum(tol, 1e-300)).max()):.3f}")
    assert (bound >= 0).all()
    assert (err <= tol).all(), (k, float(bound[k]), float(s[k]))
    # stream off: nothing is emitted
    t0 = _trainer(monkeypatch, False)
    t0.training_step(torch.from_numpy(pos).cuda(), torch.from_numpy(tgt).cuda())
    L.check(dbg.tcnn_debug_step_dldenc(t0.h, w.ctypes.data, w.nbytes, bound.ctypes.data, bound.nbytes, ctypes.byref(live)))
    assert live.value == 0


def _lim(m, P):
    """grid_bwd_scale_lim (D = 2) in float32 arithmetic"""
    f = np.float32
    return (f(2147483647.0) - f(4.0) * f(P)) / (f(m) * f(1.01))


def _search_m(P, j, want):
    """a float32 m whose lim is `want` relative to 2^j: 'below' = the largest float under 2^j, 'above' =
    2^j itself or its successor, 'inside' = mantissa near 1.5"""
    f = np.float32
    p2 = f(2.0 ** j)
    target = {"below": p2, "above": p2, "inside": f(1.5 * 2.0 ** j)}[want]
    m = (f(2147483647.0) - f(4.0) * f(P)) / (target * f(1.01))
    cands = [m]
    lo = hi = m
    for _ in range(64):
        lo, hi = np.nextafter(lo, f(0)), np.nextafter(hi, f(np.inf))
        cands += [lo, hi]
    for c in cands:
        lim = _lim(c, P)
        if want == "below" and lim == np.nextafter(p2, f(0)):
            return c
        if want == "above" and p2 <= lim <= np.nextafter(p2, f(np.inf)):
            return c
        if want == "inside" and abs(float(lim) / float(p2) - 1.5) < 0.01:
            return c
    raise AssertionError(("no m found", P, j, want))


def _split_fp16(m):
    """m (float32, 24-bit significand) as three fp16 values of different exponents whose sum is m in
    any order: 11 + 11 + 2 bits of the significand"""
    mant, ex = np.frexp(np.float64(m))
    q = int(mant * 2 ** 24)  # 24-bit integer, m = q * 2^(ex - 24)
    parts = [(q >> 13) << 13, ((q >> 2) & 0x7ff) << 2, q & 3]
    vals = [np.float64(p) * 2.0 ** (int(ex) - 24) for p in parts]
    h = np.array(vals, np.float64).astype(np.float16)
    assert (h.astype(np.float64) == np.array(vals)).all() and np.float32(sum(vals)) == np.float32(m)
    return h


@pytest.mark.parametrize("want", ["below", "above", "inside"])
def test_guard_band_falls_back_and_stays_bit_identical(torch_mod, dbg, monkeypatch, want):
    """dL/dy crafted so that the chunk's sum (exact in every order: three fp16 values of different
    exponents) puts lim one ulp under / at a power of two -> every workgroup falls back; a sum with lim
    in the middle of the binade -> none does. The slabs equal those of the exact path (no slice sums)."""
    torch = torch_mod
    from tinycudann import _lib as L
    B = 256
    t = _trainer(monkeypatch, True)
    m = _search_m(B, 24, want)
    h = _split_fp16(m)
    pos, _ = make_batch(B)
    dy = np.zeros((N_LEVELS, B, 2), np.float16)
    dy[:, 3, 0], dy[:, 40, 1], dy[:, 200, 0] = h[0], -h[1], h[2]  # (feature 1, a negative value: max_f | . |)
    per_point = np.abs(dy.astype(np.float32)).max(axis=2)
    bound = per_point.reshape(N_LEVELS, B // 32, 32).sum(axis=2, dtype=np.float32)
    assert np.float32(bound[0].sum(dtype=np.float32)) == np.float32(m)
    d_pos = torch.from_numpy(pos).cuda()
    d_dy = torch.from_numpy(dy).cuda()
    d_bound = torch.from_numpy(bound).cuda()
    slabs = []
    counts = []
    for bptr in (None, d_bound.data_ptr()):
        out = np.full(1 << 22, np.nan, np.float32)
        nc, stride = ctypes.c_uint32(0), ctypes.c_uint32(0)
        L.check(dbg.tcnn_debug_grid_backward_items(t.h, None, B, d_pos.data_ptr(), d_dy.data_ptr(), bptr, out.ctypes.data, out.size,
                                                   ctypes.byref(nc), ctypes.byref(stride)))
        assert nc.value == 1
        slabs.append(out[:stride.value].copy())
        counts.append(_fallbacks(dbg))
    print(f"{want}: m = {float(m)!r}, lim = {float(_lim(m, B))!r}, fallbacks {counts}")
    assert counts[0] == 0
    assert np.array_equal(bits(slabs[0]), bits(slabs[1]))
    assert np.isfinite(slabs[0]).all() and np.abs(slabs[0]).max() > 0
    if want == "inside":
        assert counts[1] == 0
    else:
        assert counts[1] >= 1
