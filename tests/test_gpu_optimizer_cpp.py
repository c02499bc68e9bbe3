"""The stacked optimizers through the C++ template API: tests/cpp/optimizer_api_consumer.cpp builds
Ema{ExponentialDecay{Adam}} with create_optimizer, trains 4 steps through tcnn::Trainer, reads params_inference(),
checks use_inference_params and the snapshot, and runs the optimizer kernels on parameter counts that are no
multiple of 8 (built by the Makefile against include/tiny-cuda-nn/*.h + libtcnn_mi355x.so)."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(REPO, "neuralbtf-tiny-cuda-nn_amd", "bin", "optimizer_api_consumer")


@pytest.mark.gpu
def test_optimizer_api_consumer_runs():
    assert os.path.exists(BIN), "build it with make -C neuralbtf-tiny-cuda-nn_amd"
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "optimizer_api ok: Ema / ExponentialDecay / Adam through tcnn::Trainer" in r.stdout, r.stdout


def test_headers_declare_the_optimizer_interface():
    inc = os.path.join(REPO, "include", "tiny-cuda-nn")
    opt = open(os.path.join(inc, "optimizer.h")).read()
    for sym in ["create_optimizer(", "float learning_rate() const", "void set_learning_rate(", "custom_weights()", "\"nested\"",
                "ExponentialDecay", "Lookahead", "Batched", "Invalid optimizer type: "]:
        assert sym in opt, sym
    tr = open(os.path.join(inc, "trainer.h")).read()
    assert "tcnn_trainer_params_inference(m_h)" in tr and "tcnn_trainer_forward_inference_params(" in tr
    capi = open(os.path.join(REPO, "include", "tcnn_mi355x.h")).read()
    for sym in ["tcnn_trainer_params_inference(", "tcnn_trainer_optimizer_buffer(", "tcnn_trainer_learning_rate(",
                "tcnn_trainer_set_learning_rate(", "tcnn_trainer_optimizer_schedule(", "tcnn_trainer_forward_inference_params("]:
        assert sym in capi, sym
