"""Register budgets of the input-Hessian kernels (csrc/mlp_f32_hessian.hip), read from the built library's code-object
metadata (CPU: no GPU needed), in the manner of tests/test_mlp_f32_jvp2_train_kernel_resources.py. A pass holds up to ten
quantities of a W-wide row in registers beside their accumulators (the value, three tangents, six pairs): none of the
kernels may have a spilled register or a private segment.
"""
import pytest

from test_encoding_f32_kernel_resources import kernels, pytestmark  # noqa: F401 (the fixture and the skip)

# kernel template -> instantiations: W x (D, F) and W for the two fronts
NEW = {"k_f32_grid_mlp_hessian": 18, "k_f32_identity_mlp_hessian": 3}


@pytest.fixture(scope="module")
def new_kernels(kernels):  # noqa: F811
    return {k: v for k, v in kernels.items() if any(b + "I" in k for b in NEW)}


def test_kernels_are_there_and_do_not_spill_or_use_scratch(new_kernels):
    for base, count in NEW.items():
        assert sum(base + "I" in k for k in new_kernels) == count, base
    bad = {k[:100]: v for k, v in new_kernels.items()
           if v[".vgpr_spill_count"] or v[".sgpr_spill_count"] or v[".private_segment_fixed_size"]}
    assert not bad, bad
