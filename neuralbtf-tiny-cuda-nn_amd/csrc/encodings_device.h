// encodings_device.h -- per-sample device functions of the parameter-free encodings (OneBlob,
// Identity, TriangleWave), shared by their own kernels (encodings.hip) and the composite kernels
// (composite.hip) so that both produce the same bits.
#pragma once

#include "common.h"

namespace tcnn_amd {

// quartic_cdf / quartic (common_device.h:905-920). The reference is compiled by nvcc with FMA
// contraction on; its contraction points are written out as explicit FMAs here (the library is
// compiled with -ffp-contract=off), the same ones the oracle uses.
__device__ __forceinline__ float quartic_cdf(float x, float inv_radius) {
	const float u = x * inv_radius;
	const float u2 = u * u;
	const float u4 = u2 * u2;
	float p = __builtin_fmaf(-(2.0f / 3.0f), u2, 1.0f);
	p = __builtin_fmaf(1.0f / 5.0f, u4, p);
	return fmaxf(0.0f, fminf(1.0f, __builtin_fmaf((15.0f / 16.0f) * u, p, 0.5f)));
}

__device__ __forceinline__ float quartic_cdf_deriv(float x, float inv_radius) {
	const float u = x * inv_radius;
	const float tmp = fmaxf(__builtin_fmaf(-u, u, 1.0f), 0.0f);
	return (15.0f / 16.0f) * tmp * tmp * inv_radius;
}

// Wrapped CDF at a bin's left boundary (one_blob_subwarp_aligned, oneblob.h:48-51). The two wrap
// terms are clamped for all but the bins within one bin width of the domain's ends: quartic_cdf is
// exactly 0 for u <= -T and exactly 1 for u >= T with T = 1.0625 (every fp32 u checked with this op
// sequence by tools/quartic_clamp_check.c; the last unclamped values are at |u| ~ 1.004), so those
// terms are skipped when no lane of the wave needs them, with bit-identical sums (same addition order).
// The forward is VALU-bound (27 polynomial evaluations per 8 bins before); this removes ~2/3 of them.
__device__ __forceinline__ float wrapped_cdf(float boundary, float x, float n_bins) {
	constexpr float T = 1.0625f;
	const float d = boundary - x;
	const float c = quartic_cdf(d, n_bins);
	// the ballot makes the test wave-uniform (a scalar branch, not predication); inside it every lane
	// evaluates the term, which is exact either way
	float lo = 0.0f, hi = 1.0f;
	if (__builtin_amdgcn_ballot_w64(!((d - 1.0f) * n_bins <= -T))) lo = quartic_cdf(d - 1.0f, n_bins);
	if (__builtin_amdgcn_ballot_w64(!((d + 1.0f) * n_bins >= T))) hi = quartic_cdf(d + 1.0f, n_bins);
	return c + lo + hi;
}

// An encoded fp32 value at the module's precision T: rounded once to fp16, or kept (fp32 modules).
template <typename T>
__device__ __forceinline__ T enc_value(float v) {
	if constexpr (sizeof(T) == 2) return f16_rn(v);
	else return v;
}

// All n_bins OneBlob outputs of one input value, handed to put(bin, value at precision T).
// The reference evaluates each bin's left CDF in its own lane and takes the right CDF from lane
// (bin + 1) with __shfl_sync(..., bin + 1, n_bins) (oneblob.h:53-62). On its 32-lane warps a shuffle
// width above 32 acts as width 32, so for n_bins > 32 the source lane wraps inside each 32-bin
// group: bin b reads the left CDF of bin (b & ~31) + ((b + 1) & 31), and only the last bin of the
// dimension adds the wrap-around 1. This reproduces exactly that (S = min(n_bins, 32)).
template <typename T = _Float16, typename Put>
__device__ __forceinline__ void oneblob_fwd_dim(float xv, uint32_t n_bins, uint32_t log2_bins, Put&& put) {
	const float nb = (float)n_bins;
	const uint32_t S = n_bins < 32 ? n_bins : 32;
	for (uint32_t g = 0; g < n_bins; g += S) {
		const float first = wrapped_cdf(scalbnf((float)g, -(int)log2_bins), xv, nb);
		float left = first;
		for (uint32_t j = 0; j < S; ++j) {
			const uint32_t b = g + j;
			float right;
			if (j + 1 < S) right = wrapped_cdf(scalbnf((float)(b + 1), -(int)log2_bins), xv, nb);
			else right = first + (b == n_bins - 1 ? 1.0f : 0.0f);
			put(b, enc_value<T>(right - left));
			left = right;
		}
	}
}

// kernel_one_blob_backward (oneblob.h:116-147): dL/dx = sum_k dL/dy[k] * (D_left - D_right).
template <typename T>
__device__ __forceinline__ float oneblob_bwd_dim(float xv, uint32_t n_bins, uint32_t log2_bins, const T* __restrict__ dy) {
	const float nb = (float)n_bins;
	float left = quartic_cdf_deriv(-xv, nb) + quartic_cdf_deriv(-xv - 1.0f, nb) + quartic_cdf_deriv(-xv + 1.0f, nb);
	float result = 0.0f;
	for (uint32_t k = 0; k < n_bins; ++k) {
		const float rb = scalbnf((float)(k + 1), -(int)log2_bins);
		const float right = quartic_cdf_deriv(rb - xv, nb) + quartic_cdf_deriv(rb - xv - 1.0f, nb) + quartic_cdf_deriv(rb - xv + 1.0f, nb);
		const float deriv = left - right;
		left = right;
		result = __builtin_fmaf((float)dy[k], deriv, result);
	}
	return result;
}

// identity (identity.h:45-66): out = x * scale + offset (nvcc contracts to one FMA)
__device__ __forceinline__ _Float16 identity_fwd_value(float xv, float scale, float offset) {
	return f16_rn(__builtin_fmaf(xv, scale, offset));
}
// identity_backward (identity.h:68-85): dL/dx = (T)(dL/dy * scale) -- stored as fp32
__device__ __forceinline__ float identity_bwd_value(_Float16 dy, float scale) { return (float)f16_rn((float)dy * scale); }
// the same with T = float (fp32 modules): no narrowing on either side
__device__ __forceinline__ float identity_fwd_value_f32(float xv, float scale, float offset) { return __builtin_fmaf(xv, scale, offset); }
__device__ __forceinline__ float identity_bwd_value(float dy, float scale) { return dy * scale; }

// TriangleWave (triangle_wave.h:46-81), frequency k of one input value: v = x 2^(k-1) + k/4,
// y = |v - floor(v) - 1/2| 4 - 1. Every operation is one correctly rounded fp32 operation (the
// products by powers of two are exact); nothing here may be contracted.
__device__ __forceinline__ float triangle_wave_phase(float xv, uint32_t k) { return scalbnf(xv, (int)k - 1) + (float)k * 0.25f; }
__device__ __forceinline__ float triangle_wave_value(float xv, uint32_t k) {
	const float v = triangle_wave_phase(xv, k);
	return fabsf(v - floorf(v) - 0.5f) * 4.0f - 1.0f;
}
// dy/dx = +-2^(k+1), negative where (int)floor(2 v) is even; recomputed in the backward (no dy_dx buffer)
__device__ __forceinline__ float triangle_wave_deriv(float xv, uint32_t k) {
	const float v = triangle_wave_phase(xv, k);
	return scalbnf(((int)floorf(v * 2.0f) % 2 == 0) ? -1.0f : 1.0f, (int)k + 1);
}

}  // namespace tcnn_amd
