"""Wiring of the grid launchers' shape dispatch (csrc/grid_dispatch.h): every D in {2, 3, 4} x
F in {1, 2, 4, 8} x hash in {Prime, CoherentPrime, ReversedPrime} runs the kernel instantiated for exactly
that shape, at fp16 and at fp32, in the forward, the parameter backward (LDS items, and the binned passes
for levels too large for the LDS), dL/dinput and the second-order kernel.

Each case is an encoding module through the C-ABI on a tiny grid -- 3 levels, base resolution 4, scale 2,
2^4 entries per level, Linear, B = 256 uniform positions, table and dL/dy uniform in [-1, 1] rounded to
fp16 -- so all 72 cases together are a few seconds.

Why a wrong instantiation cannot pass. A wrong D or F reads or writes other columns and entries and
misses every tolerance below by orders of magnitude. A wrong hash is the subtle one, and the forward
bound is built for it: an output is a convex combination of at most 16 table values with |value| <= 1;
the fp16 rounding of each weight and of each FMA step adds at most 2^-11 each, so the kernel and the
oracle agree to about 0.02 < 0.05. test_hashes_discriminate asserts on the CPU oracle that between any
two hash types more than half of the outputs of every (D, F) differ by MORE than 0.05 (measured: >= 60 %
at D = 2, whose dense level 0 cannot differ, >= 82 % at D = 3 and 4), so a table of primes that stopped
discriminating fails loudly instead of weakening the GPU checks.

Tolerances are those of the tests that own each quantity:
  fp16  forward vs oracle.grid_fwd: max |diff| <= 0.05 (above); dL/dparams vs oracle.grid_bwd per element
        within oracle.grid_grad_tolerance (plus half an fp16 ulp of the module's fp16 output, as
        tests/test_gpu_grid_large.py applies it); dL/dx rtol = atol = 1e-5 (tests/test_gpu_grid_input.py);
        second order as tests/test_gpu_grid_second_order.py.
  fp32  forward and dL/dparams vs the float64 restatement of tests/test_grid_f32_reference.py within its
        forward_bound / gradient_bound; dL/dx and second order vs the oracle as
        tests/test_gpu_encoding_f32.py does (fp32 arithmetic in both precisions).
"""
import functools
import itertools

import numpy as np
import pytest

import test_grid_f32_reference as G
from helpers import rel_err
from oracle import oracle as O

HASHES = ("Prime", "CoherentPrime", "ReversedPrime")
DIMS, FEATURES = (2, 3, 4), (1, 2, 4, 8)
B = 256
FP32, FP16 = 0, 1


def tiny_enc(F, hash_name):
    return {"otype": "HashGrid", "n_levels": 3, "n_features_per_level": F, "log2_hashmap_size": 4, "base_resolution": 4,
            "per_level_scale": 2.0, "interpolation": "Linear", "hash": hash_name}


@functools.lru_cache(maxsize=None)
def case(D, F):
    """Inputs of one (D, F) -- the same for the three hashes, whose tables have the same size -- and the
    oracle's results per hash; computed once, shared by every test, never modified."""
    rng = np.random.default_rng(1000 * D + F)
    g0 = O.grid_cfg(tiny_enc(F, "CoherentPrime"), D)
    LF = g0.n_levels * F
    pos = rng.uniform(0, 1, (B, D)).astype(np.float32)
    t16 = O.f2h(rng.uniform(-1, 1, g0.n_params).astype(np.float32))
    dy16 = O.f2h(rng.uniform(-1, 1, (B, LF)).astype(np.float32))
    gx = (rng.standard_normal((B, D)) * 1e-3).astype(np.float32)  # keeps the fp16 module's dL/dgrid inside fp16
    dy_soa = np.ascontiguousarray(dy16.T)
    ref = {}
    for h in HASHES:
        g = O.grid_cfg(tiny_enc(F, h), D)
        assert g.n_params == g0.n_params
        grad = O.grid_bwd(g, pos, dy_soa)
        ref[h] = dict(g=g, fwd=O.h2f(O.grid_fwd(g, pos, t16)).T, grad=grad, tol=O.grid_grad_tolerance(g, pos, dy_soa, grad),
                      dx=O.grid_bwd_input(g, pos, t16, dy_soa), bwd_bwd=O.grid_bwd_bwd(g, pos, t16, gx, dy_soa))
    return dict(pos=pos, t16=t16, dy16=dy16, gx=gx, ref=ref)


@pytest.mark.parametrize("D,F", list(itertools.product(DIMS, FEATURES)))
def test_hashes_discriminate(D, F):
    """The negative control of the 0.05 forward bound, on the CPU oracle: between every two hash types
    more than half of the outputs differ by more than 0.05."""
    c = case(D, F)
    for a, b in itertools.combinations(HASHES, 2):
        frac = float(np.mean(np.abs(c["ref"][a]["fwd"] - c["ref"][b]["fwd"]) > 0.05))
        print(f"D={D} F={F} {a} vs {b}: {100 * frac:.0f} % of the outputs differ by more than 0.05")
        assert frac > 0.5, (D, F, a, b, frac)


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.mark.gpu
@pytest.mark.parametrize("D,F", list(itertools.product(DIMS, FEATURES)))
@pytest.mark.parametrize("precision", [FP16, FP32], ids=["fp16", "fp32"])
def test_every_shape_runs_its_own_kernels(torch_mod, precision, D, F):
    from test_gpu_encoding_f32 import Mod
    from test_gpu_grid_large import _check_grid_grad
    c = case(D, F)
    pos, t16, dy16, gx = c["pos"], c["t16"], c["dy16"], c["gx"]
    table, dy = O.h2f(t16), O.h2f(dy16)
    LF = 3 * F
    for h in HASHES:
        r = c["ref"][h]
        g, what = r["g"], f"D={D} F={F} {h} {'fp32' if precision == FP32 else 'fp16'}"
        m = Mod(torch_mod, D, tiny_enc(F, h), precision)
        assert m.n_params == g.n_params and m.width == LF
        rgrad, rddy, rdx2 = r["bwd_bwd"]
        if precision == FP16:
            out = O.h2f(m.forward(pos, t16))
            err = np.abs(out - r["fwd"]).max()
            print(what, "forward: max |gpu - oracle|", err)
            assert err <= 0.05, (what, err)
            dx, grad = m.backward(dy16)
            _check_grid_grad(O.h2f(grad), r["grad"], r["tol"], True, what)
            np.testing.assert_allclose(dx, r["dx"], rtol=1e-5, atol=1e-5, err_msg=what)
            grad2, ddy, dx2 = m.backward_backward(gx, dy16)
            grad2, ddy = O.h2f(grad2), O.h2f(ddy)
            np.testing.assert_allclose(ddy[:, :LF], O.h2f(O.f2h(rddy)), rtol=2e-3, atol=1e-4 * np.abs(rddy).max(), err_msg=what)
        else:
            out = m.forward(pos, table).astype(np.float64)
            ref, A, E = G.grid_forward(g, pos, table)
            ratio = (np.abs(out - ref) / G.forward_bound(g, A, E)).max()
            print(what, "forward: max error / bound", ratio)
            assert ratio <= 1.0, (what, ratio)
            dx, grad = m.backward(dy)
            gref, count, absum, esum, S_level = G.grid_gradient(g, pos, dy)
            tol = G.gradient_bound(g, gref, count, absum, esum, S_level)
            ratio = (np.abs(grad - gref)[count > 0] / tol[count > 0]).max()
            print(what, "dL/dparams: max error / bound", ratio)
            assert ratio <= 1.0, (what, ratio)
            assert np.all(grad[count == 0] == 0), what
            np.testing.assert_allclose(dx, r["dx"], rtol=1e-5, atol=1e-5, err_msg=what)
            grad2, ddy, dx2 = m.backward_backward(gx, dy)
            np.testing.assert_allclose(ddy[:, :LF], rddy, rtol=2e-3, atol=1e-4 * np.abs(rddy).max(), err_msg=what)
        np.testing.assert_allclose(dx2, rdx2, rtol=1e-4, atol=1e-4 * np.abs(rdx2).max(), err_msg=what)
        assert rel_err(grad2, rgrad) <= 2e-3, (what, rel_err(grad2, rgrad))
        m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("D,h", list(zip(DIMS, HASHES)))
def test_binned_backward_every_dim(torch_mod, D, h):
    """The binned passes (k_grid_bin, k_grid_acc) dispatch on the shape too: the configuration
    tests/test_gpu_grid_large.py bins (16 levels, F = 2, 2^19 entries: the fine levels do not fit the LDS)
    at its smallest batch, per element within oracle.grid_grad_tolerance. One hash per D, each hash once
    (a table of 2^24 parameters costs the oracle half a second): the hash rung itself is the one the small
    cases above check for every shape."""
    from test_gpu_grid_large import ENC_T19, _check_grid_grad, _module_case
    got, ref, tol, g = _module_case(torch_mod, dict(ENC_T19, hash=h), D, 256)
    assert (g.offsets[g.n_levels] - g.offsets[g.n_levels - 1]) * g.n_features_per_level > 32768  # the finest level exceeds the LDS slots
    _check_grid_grad(got, ref, tol, True, f"binned D={D} {h}")
