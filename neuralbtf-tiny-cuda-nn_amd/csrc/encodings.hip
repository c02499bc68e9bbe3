// encodings.hip -- OneBlob and Identity encodings for gfx950 (reference encodings/oneblob.h,
// encodings/identity.h). Output AoS [B][out_stride] (their preferred layout) at the module's precision
// T (_Float16, or float for an fp32 encoding module: the fp32 value each kernel computes, not narrowed),
// padding columns set to 1 (oneblob.h:200-203, identity.h:62-63).
#include "encodings_device.h"
#include "kernels.h"

namespace tcnn_amd {

// OneBlob forward, one thread per (sample, dim): all n_bins outputs of that dimension.
// (oneblob_fwd_dim, encodings_device.h, reproduces the reference's shuffle semantics).
template <typename T>
__global__ __launch_bounds__(256) void k_oneblob_fwd(uint32_t B, uint32_t D, uint32_t n_bins, uint32_t log2_bins,
                                                      const float* __restrict__ x, uint32_t x_stride, T* __restrict__ out,
                                                      uint32_t out_stride, uint32_t n_pad) {
	const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
	if (t >= B * (D + (n_pad ? 1 : 0))) return;
	const uint32_t i = t / (D + (n_pad ? 1 : 0)), d = t % (D + (n_pad ? 1 : 0));
	T* row = out + (size_t)i * out_stride;
	if (d == D) {  // padding columns
		for (uint32_t j = 0; j < n_pad; ++j) row[D * n_bins + j] = (T)1.0f;
		return;
	}
	const float xv = x[(size_t)i * x_stride + d];
	T* o = row + d * n_bins;
	oneblob_fwd_dim<T>(xv, n_bins, log2_bins, [&](uint32_t b, T v) { o[b] = v; });
}

// Same values, 8 bins per thread and one 16-byte store (fp32: two) (n_bins >= 8): consecutive threads
// write consecutive 16 B (32 B) of a row. Bin b = g + j of the S-bin group g reads cdf(b + 1) for j + 1 < S and
// cdf(g) (+1 for the dimension's last bin) for the group's last bin, exactly as above.
template <typename T>
__global__ __launch_bounds__(256) void k_oneblob_fwd8(uint32_t B, uint32_t D, uint32_t n_bins, uint32_t log2_bins,
                                                       const float* __restrict__ x, uint32_t x_stride, T* __restrict__ out,
                                                       uint32_t out_stride) {
	const uint32_t per_row = D * (n_bins / 8);
	const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
	if (t >= B * per_row) return;
	// n_bins / 8 is a power of two (shifts); so is per_row for D = 1, 2, 4 (no 32-bit udiv sequences)
	const uint32_t lg = log2_bins - 3;
	uint32_t i, rem;
	if ((per_row & (per_row - 1)) == 0) {
		const uint32_t lr = lg + (uint32_t)__builtin_ctz(D);
		i = t >> lr;
		rem = t & (per_row - 1);
	} else {
		i = t / per_row;
		rem = t - i * per_row;
	}
	const uint32_t d = rem >> lg, b0 = 8 * (rem & ((1u << lg) - 1));
	const float xv = x[(size_t)i * x_stride + d];
	const float nb = (float)n_bins;
	const uint32_t S = n_bins < 32 ? n_bins : 32;
	const uint32_t g = b0 & ~(S - 1);
	float left = wrapped_cdf(scalbnf((float)b0, -(int)log2_bins), xv, nb);
	T o[8];
#pragma unroll
	for (uint32_t j = 0; j < 8; ++j) {
		const uint32_t b = b0 + j;
		float right;
		if (b - g + 1 < S) right = wrapped_cdf(scalbnf((float)(b + 1), -(int)log2_bins), xv, nb);
		else right = wrapped_cdf(scalbnf((float)g, -(int)log2_bins), xv, nb) + (b == n_bins - 1 ? 1.0f : 0.0f);
		o[j] = enc_value<T>(right - left);
		left = right;
	}
	T* dst = out + (size_t)i * out_stride + d * n_bins + b0;
	if constexpr (sizeof(T) == 2) {
		*(h8*)dst = h8{o[0], o[1], o[2], o[3], o[4], o[5], o[6], o[7]};
	} else {
		*(f4*)dst = f4{o[0], o[1], o[2], o[3]};
		*(f4*)(dst + 4) = f4{o[4], o[5], o[6], o[7]};
	}
}

template <typename T>
__global__ __launch_bounds__(256) void k_fill_pad(uint32_t B, T* __restrict__ out, uint32_t out_stride, uint32_t col0,
                                                  uint32_t n_pad) {
	const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
	if (t >= B * n_pad) return;
	out[(size_t)(t / n_pad) * out_stride + col0 + t % n_pad] = (T)1.0f;
}

// kernel_one_blob_backward (oneblob.h:116-147): dL/dx[d] = sum_k dL/dy[d*n_bins + k] * (D_left - D_right).
template <typename T>
__global__ __launch_bounds__(256) void k_oneblob_bwd(uint32_t B, uint32_t D, uint32_t n_bins, uint32_t log2_bins,
                                                      const float* __restrict__ x, uint32_t x_stride,
                                                      const T* __restrict__ dy, uint32_t dy_stride, float* __restrict__ dx,
                                                      uint32_t dx_stride) {
	const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
	if (t >= B * D) return;
	const uint32_t i = t / D, d = t % D;
	const float xv = x[(size_t)i * x_stride + d];
	dx[(size_t)i * dx_stride + d] = oneblob_bwd_dim(xv, n_bins, log2_bins, dy + (size_t)i * dy_stride + d * n_bins);
}

static uint32_t ilog2(uint32_t v) {
	uint32_t r = 0;
	while ((1u << r) < v) ++r;
	return r;
}

// The launchers are templates on the module's precision T, instantiated for _Float16 and float below
// each. 16-byte stores of 8 bins: rows and the output pointer must keep every 8-bin group aligned
template <typename T>
void launch_oneblob_fwd(hipStream_t st, uint32_t B, uint32_t D, uint32_t n_bins, const float* x, uint32_t x_stride, T* out,
                        uint32_t out_stride, uint32_t n_pad) {
	TCNN_CHECK(n_bins > 0 && (n_bins & (n_bins - 1)) == 0, "Number of bins must be a power of 2");
	if (!B) return;
	constexpr uint32_t CH = 16 / sizeof(T);  // elements per 16 bytes
	const bool vec = sizeof(T) == 2 ? out_stride % 8 == 0 : (out_stride % CH == 0 && ((uintptr_t)out & 15) == 0);
	if (n_bins >= 8 && vec) {
		const uint32_t n = B * D * (n_bins / 8);
		hipLaunchKernelGGL(k_oneblob_fwd8<T>, dim3(div_round_up(n, 256)), dim3(256), 0, st, B, D, n_bins, ilog2(n_bins), x, x_stride, out,
		                   out_stride);
		if (n_pad)
			hipLaunchKernelGGL(k_fill_pad<T>, dim3(div_round_up(B * n_pad, 256)), dim3(256), 0, st, B, out, out_stride, D * n_bins, n_pad);
	} else {
		const uint32_t n = B * (D + (n_pad ? 1 : 0));
		hipLaunchKernelGGL(k_oneblob_fwd<T>, dim3(div_round_up(n, 256)), dim3(256), 0, st, B, D, n_bins, ilog2(n_bins), x, x_stride, out,
		                   out_stride, n_pad);
	}
	TCNN_HIP_CHECK(hipGetLastError());
}
template void launch_oneblob_fwd<_Float16>(hipStream_t, uint32_t, uint32_t, uint32_t, const float*, uint32_t, _Float16*, uint32_t, uint32_t);
template void launch_oneblob_fwd<float>(hipStream_t, uint32_t, uint32_t, uint32_t, const float*, uint32_t, float*, uint32_t, uint32_t);

template <typename T>
void launch_oneblob_bwd(hipStream_t st, uint32_t B, uint32_t D, uint32_t n_bins, const float* x, uint32_t x_stride, const T* dy,
                        uint32_t dy_stride, float* dx, uint32_t dx_stride) {
	if (!B) return;
	hipLaunchKernelGGL(k_oneblob_bwd<T>, dim3(div_round_up(B * D, 256)), dim3(256), 0, st, B, D, n_bins, ilog2(n_bins), x, x_stride, dy,
	                   dy_stride, dx, dx_stride);
	TCNN_HIP_CHECK(hipGetLastError());
}
template void launch_oneblob_bwd<_Float16>(hipStream_t, uint32_t, uint32_t, uint32_t, const float*, uint32_t, const _Float16*, uint32_t,
                                           float*, uint32_t);
template void launch_oneblob_bwd<float>(hipStream_t, uint32_t, uint32_t, uint32_t, const float*, uint32_t, const float*, uint32_t, float*,
                                        uint32_t);

// identity (identity.h:45-66): out = x * scale + offset (nvcc contracts to one FMA), padding 1.
template <typename T>
__global__ __launch_bounds__(256) void k_identity_fwd(uint32_t B, uint32_t D, float scale, float offset, const float* __restrict__ x,
                                                       uint32_t x_stride, T* __restrict__ out, uint32_t out_stride, uint32_t n_pad) {
	const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
	const uint32_t fan = D + n_pad;
	if (t >= B * fan) return;
	const uint32_t i = t / fan, j = t % fan;
	T v = (T)1.0f;
	if (j < D) {
		if constexpr (sizeof(T) == 2) v = identity_fwd_value(x[(size_t)i * x_stride + j], scale, offset);
		else v = identity_fwd_value_f32(x[(size_t)i * x_stride + j], scale, offset);
	}
	out[(size_t)i * out_stride + j] = v;
}

// identity_backward (identity.h:68-85): dL/dx = (T)(dL/dy * scale) -- stored as fp32 here.
template <typename T>
__global__ __launch_bounds__(256) void k_identity_bwd(uint32_t B, uint32_t D, float scale, const T* __restrict__ dy, uint32_t dy_stride,
                                                       float* __restrict__ dx, uint32_t dx_stride) {
	const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
	if (t >= B * D) return;
	const uint32_t i = t / D, j = t % D;
	dx[(size_t)i * dx_stride + j] = identity_bwd_value(dy[(size_t)i * dy_stride + j], scale);
}

template <typename T>
void launch_identity_fwd(hipStream_t st, uint32_t B, uint32_t D, float scale, float offset, const float* x, uint32_t x_stride, T* out,
                         uint32_t out_stride, uint32_t n_pad) {
	if (!B) return;
	hipLaunchKernelGGL(k_identity_fwd<T>, dim3(div_round_up(B * (D + n_pad), 256)), dim3(256), 0, st, B, D, scale, offset, x, x_stride, out,
	                   out_stride, n_pad);
	TCNN_HIP_CHECK(hipGetLastError());
}
template void launch_identity_fwd<_Float16>(hipStream_t, uint32_t, uint32_t, float, float, const float*, uint32_t, _Float16*, uint32_t,
                                            uint32_t);
template void launch_identity_fwd<float>(hipStream_t, uint32_t, uint32_t, float, float, const float*, uint32_t, float*, uint32_t, uint32_t);

template <typename T>
void launch_identity_bwd(hipStream_t st, uint32_t B, uint32_t D, float scale, const T* dy, uint32_t dy_stride, float* dx,
                         uint32_t dx_stride) {
	if (!B) return;
	hipLaunchKernelGGL(k_identity_bwd<T>, dim3(div_round_up(B * D, 256)), dim3(256), 0, st, B, D, scale, dy, dy_stride, dx, dx_stride);
	TCNN_HIP_CHECK(hipGetLastError());
}
template void launch_identity_bwd<_Float16>(hipStream_t, uint32_t, uint32_t, float, const _Float16*, uint32_t, float*, uint32_t);
template void launch_identity_bwd<float>(hipStream_t, uint32_t, uint32_t, float, const float*, uint32_t, float*, uint32_t);

}  // namespace tcnn_amd
