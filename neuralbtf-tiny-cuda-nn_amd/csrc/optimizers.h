// optimizers.h -- launchers of the elementwise optimizer kernels (optimizers.hip; arithmetic in
// optim_device.h): SGD, the EMA of the weights, the Lookahead blend, the Batched gradient pool.
#pragma once

#include "common.h"

namespace tcnn_amd {

// ---- kernels: streaming passes over n parameters; every buffer a whole allocation of >= n elements ----
uint32_t optimizer_kernel_span();  // parameters per workgroup of these passes
// g16 = fp16(g32 * grad_scale): the fp16 gradients (the rounding Adam applies to its input)
void launch_grad_f16(hipStream_t st, const float* g32, void* g16, float grad_scale, size_t n);
void launch_sgd(hipStream_t st, float* w32, void* w16, const void* g16, float loss_scale, float lr, float l2_reg, size_t n);
// tmp != nullptr: full precision (tmp carries the average, ema16 its rounding); else ema16 carries it
void launch_ema(hipStream_t st, const void* w16, void* ema16, float* tmp, float decay, float debias_old, float debias_new, size_t n);
void launch_lookahead(hipStream_t st, float* w32, void* w16, void* look16, float alpha, size_t n);
void launch_batched_pool(hipStream_t st, const void* g16, float* pool, uint32_t multiplier, bool first, size_t n);
// tinycudann.optim.Adam on one parameter tensor: the reference's update (adam_tail, adam_device.h) of the fp32
// parameters w32 from the gradients as they are (fp32, or fp16 with grad_f16), the moments and the
// per-parameter step counts; a.n parameters, the first a.n_matrix matrix parameters. All pointers 16-byte aligned.
struct AdamArgs;
void launch_adam_torch(hipStream_t st, const AdamArgs& a, float* w32, const void* grad, bool grad_f16, float* m1, float* m2, uint32_t* steps);
void launch_pool_cast(hipStream_t st, const float* pool, void* pool16, size_t n);

}  // namespace tcnn_amd
