// loss_torch.hip -- the nine losses (loss_device.h) as the torch loss object needs them
// (tinycudann.Loss): predictions P = _Float16 or float in rows of any stride, the reduced value
// instead of per-element values, and the loss scale read from device memory (autograd's grad_output).
//
//   k_loss_torch_value  the sum of the per-element values: each workgroup sums LOSS_SPAN consecutive
//                       elements in a fixed order into partial[block] (a single workgroup writes the
//                       value itself), then
//   k_loss_torch_sum    one workgroup adds the partials in a fixed order. No atomics: the value's
//                       bits depend on the inputs only.
//   k_loss_torch_grad   dL/dprediction [n][dims] contiguous in P: *scale * (...) / n_total, fp16
//                       rounded once from the fp32 result, fp32 as it is.
//
// Access: consecutive lanes on consecutive elements e = row * dims + column. At dims = 3 on a
// 16-column fp16 output row (32 bytes) a wave's 64 elements span 22 rows = 6 cache lines of
// predictions and 2 of targets per load; one lane per row would touch 16 + 6 lines per load for a
// third of the elements each. RelativeL2Luminance re-reads its row's 3 (6) colour columns per
// element, from lines the wave's own loads have just brought in. LDS: the block reduction only.
#include "adam_device.h"
#include "loss_device.h"
#include "loss_torch.h"

namespace tcnn_amd {

namespace {

constexpr uint32_t LOSS_THREADS = 256;
constexpr uint32_t LOSS_PER_THREAD = 8;
constexpr uint32_t LOSS_SPAN = LOSS_THREADS * LOSS_PER_THREAD;

struct LossTorchArgs {
	uint32_t type, dims;
	uint64_t n_elements;  // n * dims < 2^32 (an element index fits 32 bits once it is in range)
	uint64_t row_stride;  // of pred, in elements
	float n_total;
	const void* pred;
	const float* target;  // [n][dims]
	const float* pdf;     // [n][dims] or nullptr
};

// value and gradient of element e (G = float for the value pass, whose gradient is dropped)
template <typename P, bool PDF, typename G>
__device__ __forceinline__ void loss_torch_element(const LossTorchArgs& a, uint32_t e, float loss_scale, float& value, G& grad) {
	const uint32_t row = e / a.dims, col = e - row * a.dims;
	const P* prow = (const P*)a.pred + (uint64_t)row * a.row_stride;
	float lum = 0.0f;
	if (a.type == LOSS_RELATIVE_L2_LUMINANCE) {  // relative_l2_luminance.h:68-77; dims >= 3 (launcher)
		float r = (float)prow[0], g = (float)prow[1], b = (float)prow[2];
		if (a.dims >= 6) r += (float)prow[3], g += (float)prow[4], b += (float)prow[5];
		lum = loss_luminance(r, g, b);
	}
	loss_eval<PDF, LOSS_ANY, G>(a.type, (float)prow[col], a.target[e], PDF ? a.pdf[e] : 1.0f, a.n_total, loss_scale, lum, value, grad);
}

template <typename P, bool PDF>
__global__ __launch_bounds__(256) void k_loss_torch_value(const LossTorchArgs a, float* __restrict__ partial, float* __restrict__ value) {
	__shared__ float lds[LOSS_THREADS];
	const uint64_t e0 = (uint64_t)blockIdx.x * LOSS_SPAN + threadIdx.x;
	float s = 0.0f;
#pragma unroll
	for (uint32_t k = 0; k < LOSS_PER_THREAD; ++k) {
		const uint64_t e = e0 + (uint64_t)k * LOSS_THREADS;
		if (e < a.n_elements) {
			float v, g;
			loss_torch_element<P, PDF, float>(a, (uint32_t)e, 1.0f, v, g);
			s += v;
		}
	}
	lds[threadIdx.x] = s;
	__syncthreads();
	for (uint32_t h = LOSS_THREADS / 2; h > 0; h >>= 1) {
		if (threadIdx.x < h) lds[threadIdx.x] += lds[threadIdx.x + h];
		__syncthreads();
	}
	if (threadIdx.x == 0) *(gridDim.x == 1 ? value : partial + blockIdx.x) = lds[0];
}

__global__ __launch_bounds__(256) void k_loss_torch_sum(const float* __restrict__ partial, uint32_t n, float* __restrict__ value) {
	__shared__ float lds[LOSS_THREADS];
	const float s = block_sum_fixed(partial, n, lds);
	if (threadIdx.x == 0) *value = s;
}

template <typename P, bool PDF>
__global__ __launch_bounds__(256) void k_loss_torch_grad(const LossTorchArgs a, const float* __restrict__ scale, P* __restrict__ grad) {
	const uint64_t e = (uint64_t)blockIdx.x * LOSS_THREADS + threadIdx.x;
	if (e >= a.n_elements) return;
	float v;
	P g;
	loss_torch_element<P, PDF, P>(a, (uint32_t)e, *scale, v, g);
	grad[e] = g;
}

LossTorchArgs loss_torch_args(uint32_t type, uint64_t n, uint32_t dims, const void* pred, uint64_t row_stride, const float* target,
                              const float* pdf) {
	TCNN_CHECK(type < LOSS_N_TYPES, "loss: unknown loss type " + std::to_string(type));
	TCNN_CHECK(dims >= 1 && dims <= LOSS_TORCH_MAX_DIMS,
	           "loss: dims must be in [1, " + std::to_string(LOSS_TORCH_MAX_DIMS) + "], got " + std::to_string(dims));
	TCNN_CHECK(type != LOSS_RELATIVE_L2_LUMINANCE || dims >= 3, "loss: RelativeL2Luminance reads the columns r, g, b: dims must be at least 3");
	TCNN_CHECK(n >= 1 && n < (1ull << 32) && n * dims < (1ull << 32), "loss: n * dims must be in [1, 2^32)");
	TCNN_CHECK(n == 1 || row_stride >= dims, "loss: the prediction's row stride must be at least dims");
	TCNN_CHECK(pred && target, "loss: null predictions or targets");
	return LossTorchArgs{type, dims, n * dims, row_stride, (float)(n * dims), pred, target, pdf};
}

}  // namespace

uint32_t loss_torch_n_partials(uint64_t n, uint32_t dims) { return div_round_up(n * dims, LOSS_SPAN); }

void launch_loss_torch_value(hipStream_t st, uint32_t type, uint64_t n, uint32_t dims, const void* pred, bool pred_f32, uint64_t row_stride,
                             const float* target, const float* pdf, float* partial, uint32_t n_partial, float* value) {
	const LossTorchArgs a = loss_torch_args(type, n, dims, pred, row_stride, target, pdf);
	const uint32_t blocks = loss_torch_n_partials(n, dims);
	TCNN_CHECK(value != nullptr, "loss: null result pointer");
	TCNN_CHECK(blocks == 1 || (partial && n_partial >= blocks), "loss: the workspace holds fewer than " + std::to_string(blocks) + " floats");
	const dim3 grid(blocks), block(LOSS_THREADS);
	if (pred_f32) {
		if (pdf) hipLaunchKernelGGL((k_loss_torch_value<float, true>), grid, block, 0, st, a, partial, value);
		else hipLaunchKernelGGL((k_loss_torch_value<float, false>), grid, block, 0, st, a, partial, value);
	} else {
		if (pdf) hipLaunchKernelGGL((k_loss_torch_value<_Float16, true>), grid, block, 0, st, a, partial, value);
		else hipLaunchKernelGGL((k_loss_torch_value<_Float16, false>), grid, block, 0, st, a, partial, value);
	}
	TCNN_HIP_CHECK(hipGetLastError());
	if (blocks > 1) {
		hipLaunchKernelGGL(k_loss_torch_sum, dim3(1), block, 0, st, partial, blocks, value);
		TCNN_HIP_CHECK(hipGetLastError());
	}
}

void launch_loss_torch_grad(hipStream_t st, uint32_t type, uint64_t n, uint32_t dims, const void* pred, bool pred_f32, uint64_t row_stride,
                            const float* target, const float* pdf, const float* scale, void* grad) {
	const LossTorchArgs a = loss_torch_args(type, n, dims, pred, row_stride, target, pdf);
	TCNN_CHECK(scale && grad, "loss: null grad_output or gradient pointer");
	const dim3 grid(div_round_up(a.n_elements, LOSS_THREADS)), block(LOSS_THREADS);
	if (pred_f32) {
		if (pdf) hipLaunchKernelGGL((k_loss_torch_grad<float, true>), grid, block, 0, st, a, scale, (float*)grad);
		else hipLaunchKernelGGL((k_loss_torch_grad<float, false>), grid, block, 0, st, a, scale, (float*)grad);
	} else {
		if (pdf) hipLaunchKernelGGL((k_loss_torch_grad<_Float16, true>), grid, block, 0, st, a, scale, (_Float16*)grad);
		else hipLaunchKernelGGL((k_loss_torch_grad<_Float16, false>), grid, block, 0, st, a, scale, (_Float16*)grad);
	}
	TCNN_HIP_CHECK(hipGetLastError());
}

}  // namespace tcnn_amd
