"""Register budgets of the fp32-precision encoding kernels (csrc/grid_f32.hip and the float
instantiations of the typed kernels in grid.hip, composite.hip and encodings.hip), read from the built
library's code-object metadata (CPU: no GPU needed), in the manner of
tests/test_composite_kernel_resources.py. An fp32 grid forward keeps 2^D gathered entries of up to 8
floats in registers (128 for D = 4, F = 8) and the LDS backward runs 1024-thread workgroups (at most 128
registers per thread): a spill to scratch would cost either silently, so every fp32 kernel must have no
spilled register and no private segment.
"""
import os
import re
import subprocess
import sys
import tempfile

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(REPO, "neuralbtf-tiny-cuda-nn_amd", "lib", "libtcnn_mi355x.so")
LLVM = "/opt/rocm/lib/llvm/bin"
sys.path.insert(0, os.path.join(REPO, "tools"))

pytestmark = pytest.mark.skipif(not os.path.exists(LIB) or not os.path.exists(f"{LLVM}/llvm-readelf"),
                                reason="library or ROCm llvm tools missing")

KEYS = (".vgpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".private_segment_fixed_size",
        ".group_segment_fixed_size")

# the kernels of grid_f32.hip by name; the typed kernels by their last template argument, float (demangled)
F32_ONLY = ("k_grid_fwd_f32", "k_grid_bwd_lds_f32")
TYPED = ("k_grid_bwd_input", "k_grid_bwd_bwd", "k_composite_fwd", "k_composite_bwd_input", "k_oneblob_fwd", "k_oneblob_fwd8",
         "k_oneblob_bwd", "k_identity_fwd", "k_identity_bwd", "k_fill_pad")


@pytest.fixture(scope="module")
def kernels():
    import kernel_resources as KR
    out = {}
    with tempfile.TemporaryDirectory() as d:
        for co in KR.code_objects(LIB, d):
            notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], capture_output=True, text=True).stdout
            for rec in notes.split("  - .agpr_count")[1:]:
                rec = ".agpr_count" + rec
                m = re.search(r"\.name:\s+(\S+)", rec)
                if not m:
                    continue
                out[m.group(1)] = {k: int((re.search(re.escape(k) + r":\s+(\d+)", rec) or [None, "0"])[1]) for k in KEYS}
    return out


def base_of(name):
    """the kernel template a mangled name instantiates at float, or None. Itanium mangling: the template
    argument list `I...E` of a typed kernel ends in `f` (float; `DF16_` is _Float16), then `E` closes the
    nested name and `v` is the return type: `k_composite_fwdIfEEv...`, `k_grid_bwd_inputILj2E...E0EfEEv...`"""
    for b in F32_ONLY:
        if b + "I" in name:
            return b
    for b in TYPED:
        if re.search(re.escape(b) + r"I(?:\w*E)?fEEv", name):
            return b
    return None


@pytest.fixture(scope="module")
def f32_kernels(kernels):
    return {k: v for k, v in kernels.items() if base_of(k)}


def test_fp32_kernels_are_in_the_library(f32_kernels):
    found = [base_of(k) for k in f32_kernels]
    for base in F32_ONLY + TYPED:
        assert base in found, (base, sorted(f32_kernels)[:8])
    # the set launch_grid_fwd instantiates: D in {2, 3, 4} x F in {1, 2, 4, 8} x 3 hash types
    assert found.count("k_grid_fwd_f32") == 36
    assert found.count("k_grid_bwd_lds_f32") == 72  # and with / without the grid options
    assert found.count("k_grid_bwd_input") == 36 and found.count("k_grid_bwd_bwd") == 36


def test_fp32_kernels_do_not_spill(f32_kernels):
    bad = {k[:100]: v for k, v in f32_kernels.items() if v[".vgpr_spill_count"] or v[".sgpr_spill_count"]}
    assert not bad, bad


def test_fp32_kernels_have_no_private_segment(f32_kernels):
    bad = {k[:100]: v for k, v in f32_kernels.items() if v[".private_segment_fixed_size"]}
    assert not bad, bad


def test_fp32_backward_fits_a_1024_thread_workgroup(f32_kernels):
    """1024 threads = 16 waves on 4 SIMDs: 4 waves per SIMD, so at most 128 registers per thread"""
    for k, v in f32_kernels.items():
        if base_of(k) == "k_grid_bwd_lds_f32":
            assert v[".vgpr_count"] <= 128, (k[:100], v)
