// optim_device.h -- per-parameter arithmetic of the elementwise optimizers beside Adam (reference
// optimizers/sgd.h:44-69, ema.h:45-76, lookahead.h:45-58, batched.h:46-61), shared by the kernels of
// optimizers.hip. The library is built with -ffp-contract=off, so every expression below is the
// written sequence of rounded fp32 operations, left to right; an fp32 result that is stored as fp16
// is rounded once from the fp32 value (f16_rn).
#pragma once

#include "common.h"

namespace tcnn_amd {

// The fp16 gradient the optimizers read (the reference's __half gradient buffer, trainer.h:327): the
// fp32 gradient sum times the gradient scale, rounded once -- what adam_core computes for itself.
__device__ __forceinline__ _Float16 optim_grad16(float gsum, float grad_scale) { return f16_rn(gsum * grad_scale); }

// SGD (sgd.h:56-68), 5 operations: g = g16 / loss_scale; g = g + l2_reg * w; w = w - lr * g.
// Every parameter alike: no zero-gradient skip, no matrix / non-matrix distinction.
__device__ __forceinline__ float sgd_update(float w, _Float16 g16, float loss_scale, float lr, float l2_reg) {
	float g = (float)g16 / loss_scale;
	g = g + l2_reg * w;
	return w - lr * g;
}

// EMA (ema.h:57, 74), 6 operations: ((prev * decay) * debias_old + w * (1 - decay)) * debias_new.
// prev is tmp (full precision) or the fp16 weights_ema (half precision); 1 - decay is computed here,
// in fp32, as the reference's kernel does.
__device__ __forceinline__ float ema_update(float prev, _Float16 w16, float decay, float debias_old, float debias_new) {
	const float a = prev * decay * debias_old;
	const float b = (float)w16 * (1.0f - decay);
	return (a + b) * debias_new;
}

// Lookahead blend (lookahead.h:55), 4 operations: look * (1 - alpha) + w * alpha.
__device__ __forceinline__ float lookahead_blend(_Float16 look, float w, float alpha) {
	const float a = (float)look * (1.0f - alpha);
	const float b = w * alpha;
	return a + b;
}

// Batched pool (batched.h:56-60), 2 operations: pool + g16 / multiplier; the first step of a window
// starts from 0 (0 + x is exact).
__device__ __forceinline__ float batched_pool(float pool, _Float16 g16, float multiplier, bool first) {
	const float p = first ? 0.0f : pool;
	return p + (float)g16 / multiplier;
}

}  // namespace tcnn_amd
