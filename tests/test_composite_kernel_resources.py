"""Register budgets of the composite encoding kernels (csrc/composite.hip), read from the built
library's code-object metadata (CPU: no GPU needed). SphericalHarmonics of degree 8 has 64 outputs
per sample; a kernel that collected them in an array before storing would spill them to scratch, so
every k_composite_fwd / k_composite_bwd_input code object must have no spilled register and no
private segment at all (the part table, a by-value kernel argument indexed by a runtime part number,
must stay in the kernel-argument segment too).
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


@pytest.fixture(scope="module")
def composite_kernels():
    import kernel_resources as KR
    out = {}
    with tempfile.TemporaryDirectory() as d:
        for co in KR.code_objects(LIB, d):
            notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], capture_output=True, text=True).stdout
            for rec in notes.split("  - .agpr_count")[1:]:
                rec = ".agpr_count" + rec
                m = re.search(r"\.name:\s+(\S+)", rec)
                if not m or "k_composite_" not in m.group(1):
                    continue
                out[m.group(1)] = {k: int((re.search(re.escape(k) + r":\s+(\d+)", rec) or [None, "0"])[1]) for k in KEYS}
    return out


def test_both_composite_kernels_are_in_the_library(composite_kernels):
    names = " ".join(composite_kernels)
    assert "k_composite_fwd" in names and "k_composite_bwd_input" in names, names


def test_composite_kernels_do_not_spill(composite_kernels):
    print(composite_kernels)
    bad = {k: v for k, v in composite_kernels.items() if v[".vgpr_spill_count"] or v[".sgpr_spill_count"]}
    assert not bad, bad


def test_composite_kernels_have_no_private_segment(composite_kernels):
    bad = {k: v for k, v in composite_kernels.items() if v[".private_segment_fixed_size"]}
    assert not bad, bad
