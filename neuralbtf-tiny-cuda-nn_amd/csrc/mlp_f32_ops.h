// mlp_f32_ops.h -- what the fp32 network kernels share (mlp_f32.hip, mlp_f32_fused.hip): the f32 MFMA and the
// activation split. Both files apply an activation through these very functions, which is one half of why the fused
// kernels give the layer kernels' bits (the other half is the accumulation order; mlp_f32_fused.hip).
#pragma once

#include "act_f32.h"
#include "kernels.h"

namespace tcnn_amd {

static_assert(AF32_NONE == ACT_NONE && AF32_RELU == ACT_RELU && AF32_LEAKY_RELU == ACT_LEAKY_RELU && AF32_EXPONENTIAL == ACT_EXPONENTIAL &&
                  AF32_SINE == ACT_SINE && AF32_SIGMOID == ACT_SIGMOID && AF32_SQUAREPLUS == ACT_SQUAREPLUS &&
                  AF32_SOFTPLUS == ACT_SOFTPLUS && AF32_TANH == ACT_TANH,
              "act_f32.h restates the activation codes of kernels.h");

namespace {

__device__ __forceinline__ f4 mfma4(float a, float b, f4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// The rare activations stay out of line, as in the fp16 layer-wise engine: the MFMA loops inline None / ReLU only.
__device__ __noinline__ float act_fwd_f32_ool(int a, float x) { return act_fwd_f32(a, x); }
__device__ __noinline__ float act_bwd_f32_ool(int a, float g, float y) { return act_bwd_f32(a, g, y); }

__device__ __forceinline__ float fwd_act(int a, float x) {
	if (a == ACT_NONE) return x;
	if (a == ACT_RELU) return x > 0.0f ? x : 0.0f;
	return act_fwd_f32_ool(a, x);
}
__device__ __forceinline__ float bwd_act(int a, float g, float y) {
	if (a == ACT_NONE) return g;
	if (a == ACT_RELU) return y > 0.0f ? g : 0.0f;
	return act_bwd_f32_ool(a, g, y);
}
__device__ __forceinline__ f4 bwd_act4(int a, f4 g, const float* __restrict__ y) {
	if (a == ACT_NONE) return g;
	const f4 yv = *(const f4*)y;
	f4 o;
#pragma unroll
	for (int e = 0; e < 4; ++e) o[e] = bwd_act(a, g[e], yv[e]);
	return o;
}

}  // namespace
}  // namespace tcnn_amd
