// loss_torch.h -- launchers of the torch loss object's kernels (loss_torch.hip): any of the nine
// losses over predictions [n][dims] (fp16, or fp32 with pred_f32) in rows of row_stride elements,
// fp32 targets and optional data_pdf [n][dims] contiguous. 1 <= dims <= LOSS_TORCH_MAX_DIMS,
// n * dims < 2^32. Nothing is allocated and nothing is read back.
#pragma once

#include "common.h"

namespace tcnn_amd {

constexpr uint32_t LOSS_TORCH_MAX_DIMS = 16;

// floats of workspace launch_loss_torch_value needs (its workgroups)
uint32_t loss_torch_n_partials(uint64_t n, uint32_t dims);
// *value = the loss (sum of the per-element values, each divided by n * dims), summed in a fixed order
void launch_loss_torch_value(hipStream_t st, uint32_t type, uint64_t n, uint32_t dims, const void* pred, bool pred_f32, uint64_t row_stride,
                             const float* target, const float* pdf, float* partial, uint32_t n_partial, float* value);
// grad [n][dims] contiguous, in the predictions' type = *scale * dL/dprediction (scale: device pointer)
void launch_loss_torch_grad(hipStream_t st, uint32_t type, uint64_t n, uint32_t dims, const void* pred, bool pred_f32, uint64_t row_stride,
                            const float* target, const float* pdf, const float* scale, void* grad);

}  // namespace tcnn_amd
