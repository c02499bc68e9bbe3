// grid_f32_device.h -- one level of one point of the fp32 grid, shared by the fp32 forward (grid_f32.hip) and the
// kernel that encodes straight into the first layer's MFMA operand (mlp_f32_jvp.hip): the corner walk with its
// weights and gathers, and the FMA chain that turns them into the level's features. Both callers run these very
// functions, which is why the fused encode gives the forward's bits.
#pragma once

#include "grid_device.h"

namespace tcnn_amd {

// F fp32 features of one table entry / one point-level: one dwordx2 (F = 2), dwordx4 (F = 4) or two
// dwordx4 (F = 8) where the address allows
template <uint32_t F>
struct alignas(F * 4 > 16 ? 16 : F * 4) FVec { float v[F]; };

template <uint32_t F>
__device__ __forceinline__ FVec<F> load_fvec(const float* __restrict__ p, bool vec) {
	if (vec) return *(const FVec<F>*)p;
	FVec<F> r;
#pragma unroll
	for (uint32_t f = 0; f < F; ++f) r.v[f] = p[f];
	return r;
}

// The 2^D corners of one level of one point, in the reference's corner order: the weights, fp32 products in the
// reference's order, and NF features from feature f0 of every corner's entry (NF = F, f0 = 0: the whole entry).
// index(local) is the entry of a cell coordinate within the level. Every gather is issued before anything consumes one.
template <uint32_t D, uint32_t F, uint32_t NF, typename Index>
__device__ __forceinline__ void gather_level_f32(const float* __restrict__ table, const LevelInfo& li, const float* p, const uint32_t* pg,
                                                 uint32_t f0, bool vec, Index&& index, float* w, FVec<NF>* v) {
#pragma unroll
	for (uint32_t c = 0; c < (1u << D); ++c) {
		float wc = 1.0f;
		uint32_t local[D];
#pragma unroll
		for (uint32_t d = 0; d < D; ++d) {
			if ((c & (1u << d)) == 0) { wc *= 1.0f - p[d]; local[d] = pg[d]; }
			else { wc *= p[d]; local[d] = pg[d] + 1; }
		}
		w[c] = wc;
		v[c] = load_fvec<NF>(table + (size_t)(li.offset + index(local)) * F + f0, vec);
	}
}

// r[f] = sum over the corners of w[c] v[c][f]: one fp32 FMA per corner and feature, corners in the reference's order
template <uint32_t NC, uint32_t NF>
__device__ __forceinline__ void combine_level_f32(const float* w, const FVec<NF>* v, float* r) {
#pragma unroll
	for (uint32_t f = 0; f < NF; ++f) r[f] = 0.0f;
#pragma unroll
	for (uint32_t c = 0; c < NC; ++c)
#pragma unroll
		for (uint32_t f = 0; f < NF; ++f) r[f] = __builtin_fmaf(w[c], v[c].v[f], r[f]);
}

// The multipliers of a hash chosen at run time: a kernel that takes the hash as an argument serves the three of them,
// and the choice is wave-uniform, made once.
template <uint32_t D>
__device__ __forceinline__ void hash_primes(HashType h, uint32_t* prime) {
#pragma unroll
	for (uint32_t d = 0; d < D; ++d)
		prime[d] = h == HashType::Prime           ? hash_prime<HashType::Prime>(d)
		           : h == HashType::ReversedPrime ? hash_prime<HashType::ReversedPrime>(d)
		                                          : hash_prime<HashType::CoherentPrime>(d);
}

// grid_index (grid_device.h) with the hash's multipliers as values (hash_primes). The same entry.
template <uint32_t D>
__device__ __forceinline__ uint32_t grid_index_primes(bool hash_grid, uint32_t size, uint32_t res, const uint32_t* pg, const uint32_t* prime) {
	uint32_t stride = 1, index = 0;
#pragma unroll
	for (uint32_t d = 0; d < D; ++d) {
		if (stride > size) break;
		index += pg[d] * stride;
		stride *= res;
	}
	if (hash_grid && size < stride) {
		uint32_t h = 0;
#pragma unroll
		for (uint32_t d = 0; d < D; ++d) h ^= pg[d] * prime[d];
		index = h;
	}
	if ((size & (size - 1)) == 0) return index & (size - 1);
	if (index >= size) {
		index -= size;
		if (index >= size) index %= size;
	}
	return index;
}

// pos_fract (grid_device.h) with the derivative of the interpolation weight with respect to the cell fraction, as
// k_grid_bwd_input computes it (grid.hip): 6 v (1 - v) from the fraction v for Smoothstep, else 1
__device__ __forceinline__ void pos_fract_d(float x, float scale, Interp interp, float& pos, float& dpos, uint32_t& grid) {
	float v = __builtin_fmaf(scale, x, 0.5f);
	const float t = floorf(v);
	grid = (uint32_t)(int)t;
	v -= t;
	dpos = 1.0f;
	if (interp == Interp::Smoothstep) {
		dpos = 6.0f * v * (1.0f - v);
		v = v * v * __builtin_fmaf(-2.0f, v, 3.0f);
	}
	pos = v;
}

// d(level's features) / d(x_gd) from the corners the value gathered: scale pd_gd sum over the 2^(D-1) edges along gd of
// (product of the other dimensions' weights) (v_right - v_left), the arithmetic of k_grid_bwd_input (grid.hip): the
// weight product starts from the scale, and each edge is one FMA (w diff) pd + sum.
template <uint32_t D, uint32_t NF>
__device__ __forceinline__ void level_tangent_f32(uint32_t gd, float scale, const float* p, const float* pd, const FVec<NF>* v, float* g) {
#pragma unroll
	for (uint32_t f = 0; f < NF; ++f) g[f] = 0.0f;
#pragma unroll
	for (uint32_t idx = 0; idx < (1u << (D - 1)); ++idx) {
		float w = scale;
		uint32_t cl = 0;
#pragma unroll
		for (uint32_t nd = 0; nd < D - 1; ++nd) {
			const uint32_t dim = nd >= gd ? nd + 1 : nd;
			if ((idx & (1u << nd)) == 0) w *= 1.0f - p[dim];
			else { w *= p[dim]; cl |= 1u << dim; }
		}
		const uint32_t cr = cl | (1u << gd);
#pragma unroll
		for (uint32_t f = 0; f < NF; ++f) g[f] = __builtin_fmaf(w * (v[cr].v[f] - v[cl].v[f]), pd[gd], g[f]);
	}
}

// One level of one point (reference kernel_grid with T = float, grid.h:93-168): fp32 weight products in
// the reference's order and one fp32 FMA per corner and feature, corners in the reference's order.
template <uint32_t D, uint32_t F, HashType H>
__device__ __forceinline__ void encode_level_f32(const float* __restrict__ table, const LevelInfo& li, bool hash_grid, Interp interp,
                                                 const float* x, bool vec, float* r) {
	float p[D];
	uint32_t pg[D];
#pragma unroll
	for (uint32_t d = 0; d < D; ++d) pos_fract(x[d], li.scale, interp, p[d], pg[d]);
	if (interp == Interp::Nearest) {
		const FVec<F> v = load_fvec<F>(table + (size_t)(li.offset + grid_index<D, H>(hash_grid, li.size, li.res, pg)) * F, vec);
#pragma unroll
		for (uint32_t f = 0; f < F; ++f) r[f] = v.v[f];
		return;
	}
	constexpr uint32_t NC = 1u << D;
	FVec<F> v[NC];
	float w[NC];
	gather_level_f32<D, F, F>(table, li, p, pg, 0, vec, [&](const uint32_t* local) { return grid_index<D, H>(hash_grid, li.size, li.res, local); },
	                          w, v);
	combine_level_f32<NC, F>(w, v, r);
}

}  // namespace tcnn_amd
