// act_f32.h -- the activations of the fp32 network engine (mlp_f32.hip): the fp16 engine's formulas
// (mlp_fused.h act_fwd_rt / act_bwd_rt, reference common_device.h:102-297) with nothing rounded to fp16.
// The transfer is written in the STORED FORWARD VALUE y, like the reference's warp_activation_backward.
// tools/act_f32_ulps.hip measures these very functions against host double.
#pragma once

#include <hip/hip_runtime.h>

namespace tcnn_amd {

// the runtime activation codes (kernels.h ACT_*), restated so that this header stands alone
enum : int {
	AF32_NONE = 0, AF32_RELU = 1, AF32_LEAKY_RELU = 2, AF32_EXPONENTIAL = 3, AF32_SINE = 4, AF32_SIGMOID = 5,
	AF32_SQUAREPLUS = 6, AF32_SOFTPLUS = 7, AF32_TANH = 8,
};
constexpr float K_ACT_F32 = 10.0f;

__device__ __forceinline__ float act_fwd_f32(int a, float x) {
	switch (a) {
		case AF32_RELU: return x > 0.0f ? x : 0.0f;
		case AF32_LEAKY_RELU: return x * (x > 0.0f ? 1.0f : 0.01f);
		case AF32_EXPONENTIAL: return expf(x);
		case AF32_SINE: return sinf(x);
		case AF32_SIGMOID: return 1.0f / (1.0f + expf(-x));
		case AF32_SQUAREPLUS: {
			const float y = x * K_ACT_F32;
			return 0.5f * (y + sqrtf(y * y + 4.0f)) / K_ACT_F32;
		}
		case AF32_SOFTPLUS: return logf(expf(x * K_ACT_F32) + 1.0f) / K_ACT_F32;
		case AF32_TANH: return tanhf(x);
		default: return x;
	}
}

// d act / d z in the forward value y (Sine has none: the engine refuses it for training)
__device__ __forceinline__ float act_factor_f32(int a, float y) {
	switch (a) {
		case AF32_RELU: return y > 0.0f ? 1.0f : 0.0f;
		case AF32_LEAKY_RELU: return y > 0.0f ? 1.0f : 0.01f;
		case AF32_EXPONENTIAL: return y;
		case AF32_SIGMOID: return y * (1.0f - y);
		case AF32_SQUAREPLUS: {
			const float t = y * K_ACT_F32;
			return t * t / (t * t + 1.0f);
		}
		case AF32_SOFTPLUS: return 1.0f - expf(-y * K_ACT_F32);
		case AF32_TANH: return 1.0f - y * y;
		default: return 1.0f;
	}
}

// d^2 act / d z^2 in the forward value y: the curvature the second-order input gradient needs. Zero for
// None, ReLU and LeakyReLU. Squareplus: K z = t - 1 / t with t = K y.
__device__ __forceinline__ float act_factor2_f32(int a, float y) {
	switch (a) {
		case AF32_EXPONENTIAL: return y;
		case AF32_SIGMOID: return (y * (1.0f - y)) * (1.0f - 2.0f * y);
		case AF32_SQUAREPLUS: {
			const float t = y * K_ACT_F32;
			const float t2 = t * t, d = t2 + 1.0f;
			return (2.0f * K_ACT_F32) * (t2 * t) / ((d * d) * d);
		}
		case AF32_SOFTPLUS: {
			const float e = expf(-y * K_ACT_F32);
			return K_ACT_F32 * ((1.0f - e) * e);
		}
		case AF32_TANH: return (-2.0f * y) * (1.0f - y * y);
		default: return 0.0f;
	}
}

__device__ __forceinline__ float act_bwd_f32(int a, float g, float y) {
	if (a == AF32_NONE) return g;
	if (a == AF32_RELU) return y > 0.0f ? g : 0.0f;
	return g * act_factor_f32(a, y);
}

}  // namespace tcnn_amd
