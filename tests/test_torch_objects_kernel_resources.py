"""Register budgets of the torch loss and optimizer kernels (csrc/loss_torch.hip and k_adam_torch in
csrc/optimizers.hip), read from the built library's code-object metadata (CPU: no GPU needed).
k_adam_torch keeps the state of 8 parameters in registers through the shared Adam update; the loss
kernels run the run-time switch over the nine losses. None of them may spill a register or have a
private segment; the only LDS is the value kernels' block reduction (256 floats).
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
FAMILIES = ("k_loss_torch_value", "k_loss_torch_sum", "k_loss_torch_grad", "k_adam_torch")


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
                if not m or not any(f in m.group(1) for f in FAMILIES):
                    continue
                out[m.group(1)] = {k: int((re.search(re.escape(k) + r":\s+(\d+)", rec) or [None, "0"])[1]) for k in KEYS}
    return out


def test_every_instantiation_is_in_the_library(kernels):
    """value and gradient kernels for {fp16, fp32} predictions x {with, without} data_pdf, the final sum, and
    k_adam_torch for fp32 and fp16 gradients"""
    count = {f: sum(f in name for name in kernels) for f in FAMILIES}
    assert count == {"k_loss_torch_value": 4, "k_loss_torch_sum": 1, "k_loss_torch_grad": 4, "k_adam_torch": 2}, sorted(kernels)


def test_kernels_do_not_spill(kernels):
    print(kernels)
    bad = {k: v for k, v in kernels.items() if v[".vgpr_spill_count"] or v[".sgpr_spill_count"]}
    assert not bad, bad


def test_kernels_have_no_private_segment(kernels):
    bad = {k: v for k, v in kernels.items() if v[".private_segment_fixed_size"]}
    assert not bad, bad


def test_lds_is_the_block_reduction_only(kernels):
    for name, v in kernels.items():
        want = 1024 if ("k_loss_torch_value" in name or "k_loss_torch_sum" in name) else 0
        assert v[".group_segment_fixed_size"] == want, (name, v)
