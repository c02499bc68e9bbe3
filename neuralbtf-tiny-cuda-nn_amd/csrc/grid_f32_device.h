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

// The second derivative of the interpolation weight with respect to the cell fraction, from pos_fract_d's fraction:
// 6 - 12 v for Smoothstep, else 0
__device__ __forceinline__ float pos_fract_dd(float x, float scale, Interp interp) {
	float v = __builtin_fmaf(scale, x, 0.5f);
	v -= floorf(v);
	return interp == Interp::Smoothstep ? __builtin_fmaf(-12.0f, v, 6.0f) : 0.0f;
}

// u[f] = sum_{d, d'} M[d][d'] d^2(level's features) / dx_d dx_d' from the corners the value gathered, M symmetric (its
// upper triangle is read):
//   d = d' (diag; pdd = 0 otherwise): scale^2 pdd_d sum over the 2^(D-1) edges along d of (product of the other
//     weights) (v_right - v_left), which is level_tangent_f32 with pdd in the place of pd, times the scale;
//   d < d' (mixed), counted twice: scale^2 pd_d pd_d' sum over the 2^(D-2) faces of (the remaining weight)
//     (v_11 - v_10 - v_01 + v_00).
// diag and mixed are wave-uniform: the interpolation, and whether the call has directions.
template <uint32_t D, uint32_t NF>
__device__ __forceinline__ void level_second_f32(float scale, const float* p, const float* pd, const float* pdd, const FVec<NF>* v,
                                                 const float (&M)[D][D], bool diag, bool mixed, float* u) {
	static_assert(D == 2 || D == 3, "a face has at most one dimension beside its two");
#pragma unroll
	for (uint32_t f = 0; f < NF; ++f) u[f] = 0.0f;
	if (diag) {
#pragma unroll
		for (uint32_t d = 0; d < D; ++d) {
			float g[NF];
			level_tangent_f32<D, NF>(d, scale, p, pdd, v, g);
			const float m = M[d][d] * scale;
#pragma unroll
			for (uint32_t f = 0; f < NF; ++f) u[f] = __builtin_fmaf(m, g[f], u[f]);
		}
	}
	if (mixed) {
#pragma unroll
		for (uint32_t d = 0; d < D; ++d)
#pragma unroll
			for (uint32_t e = d + 1; e < D; ++e) {
				float g[NF];
#pragma unroll
				for (uint32_t f = 0; f < NF; ++f) g[f] = 0.0f;
#pragma unroll
				for (uint32_t idx = 0; idx < (1u << (D - 2)); ++idx) {
					float w = 1.0f;
					uint32_t c00 = 0;
#pragma unroll
					for (uint32_t m = 0; m < D; ++m) {  // the dimensions beside d and e: one for D = 3, none for D = 2
						if (m == d || m == e) continue;
						if (idx == 0) w *= 1.0f - p[m];
						else { w *= p[m]; c00 |= 1u << m; }
					}
					const uint32_t c10 = c00 | (1u << d), c01 = c00 | (1u << e), c11 = c10 | c01;
#pragma unroll
					for (uint32_t f = 0; f < NF; ++f) g[f] = __builtin_fmaf(w, (v[c11].v[f] - v[c10].v[f]) - (v[c01].v[f] - v[c00].v[f]), g[f]);
				}
				const float m = 2.0f * M[d][e] * ((scale * pd[d]) * (scale * pd[e]));
#pragma unroll
				for (uint32_t f = 0; f < NF; ++f) u[f] = __builtin_fmaf(m, g[f], u[f]);
			}
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
