"""The C++ caller of fp32 network modules (tests/cpp/mlp_f32_consumer.cpp, built by the Makefile):
tcnn::cpp::create_network / create_network_with_input_encoding with Precision::Fp32 report Fp32, and a
W = 16 network's forward and backward agree with a host double loop."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_mlp_f32_consumer():
    exe = os.path.join(REPO, "neuralbtf-tiny-cuda-nn_amd", "bin", "mlp_f32_consumer")
    assert os.path.exists(exe), "build it with make -C neuralbtf-tiny-cuda-nn_amd"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "mlp f32 api ok" in r.stdout, r.stdout
