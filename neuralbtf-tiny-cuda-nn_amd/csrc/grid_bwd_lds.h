// grid_bwd_lds.h -- the LDS-privatised grid backward (reference kernel_grid_backward, grid.h:214-320):
// kernel template and per-D launchers, instantiated once per input dimension in grid_bwd_d{2,3,4}.hip
// (one translation unit per D keeps the parallel build short).
#pragma once

#include "kernels.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "adam_device.h"
#include "grid_bwd_scale.h"
#include "grid_device.h"
#include "grid_dispatch.h"
#include "wt_store.h"

namespace tcnn_amd {

// LDS accumulators are int32 fixed point with a per-(work item, chunk) power-of-two scale.
// gfx950 executes LDS float atomics (ds_add_f32 / ds_pk_add_f16) at ~195 cycles per wave-instruction
// per CU but ds_add_u32 at ~8 (tools/lds_atomic_bench.hip), and integer sums are order-independent,
// so the gradient is bit-reproducible (the reference's fp16 atomics, grid.h:252-255, are not).
// Range: the bilinear weights of one point sum to 1, so no table entry can receive more than
// sum_i |dL/dy_i| over a chunk's points (hash collisions included); the scale 2^e is the largest
// power of two that keeps that bound plus the rounding of every add below 2^31, i.e. one add
// resolves 2^-31 * sum |dL/dy| ~ 2^-16 * mean |dL/dy| for the ~2^15-point chunks of B = 2^18
// (finer than the reference's fp16 running sums, and insensitive to a single outlier dL/dy).
// 32-bit accumulators let a whole 32768-entry hashed level (one feature) or a whole dense level
// (all features) sit in 128 KiB of LDS: every corner update lands and no lane is masked off.
// Levels larger than that take the binned backward (grid_bin.hip).
constexpr uint32_t GRID_BWD_THREADS = 1024;
constexpr uint32_t GRID_BWD_LDS_BYTES = 128 * 1024;
constexpr uint32_t GRID_BWD_SLOTS = GRID_BWD_LDS_BYTES / 4;



__device__ __forceinline__ void lds_add_i32(int* acc, float v) {
	__hip_atomic_fetch_add(acc, __float2int_rn(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// Index kinds of a level, uniform per work item (reference grid_index, common_device.h:690-707):
//   HASH_POW2  hashed level of power-of-two size: index = hash & (size - 1)
//   DENSE      res^D <= size: index = sum g_d res^d, < 2 size, so `% size` is one conditional subtract
//   GENERIC    anything else (tiled grids, non-power-of-two hashed sizes): grid_index()
//   HASH_RANGE a contiguous entry range [begin, begin + len) of such a hashed level (r06: a hashed
//              level too large for the LDS is split into entry ranges holding all F features, so its
//              slab is in parameter order; corners outside the range are skipped)
enum : int { IDX_HASH_POW2 = 0, IDX_DENSE = 1, IDX_GENERIC = 2, IDX_HASH_RANGE = 3 };

template <uint32_t D, HashType H, int KIND>
__device__ __forceinline__ uint32_t level_index(bool hash_grid, uint32_t size, uint32_t res, const uint32_t* g) {
	if constexpr (KIND == IDX_HASH_POW2 || KIND == IDX_HASH_RANGE) {
		uint32_t h = 0;
#pragma unroll
		for (uint32_t d = 0; d < D; ++d) h ^= g[d] * hash_prime<H>(d);
		return h & (size - 1);
	} else if constexpr (KIND == IDX_DENSE) {
		uint32_t idx = 0, stride = 1;
#pragma unroll
		for (uint32_t d = 0; d < D; ++d) {
			idx += g[d] * stride;
			stride *= res;
		}
		// index % size (common_device.h:706): in-range positions give idx < 2 size; positions
		// outside [0, 1] can give any value
		if (idx >= size) {
			idx -= size;
			if (idx >= size) idx %= size;
		}
		return idx;
	} else {
		return grid_index<D, H>(hash_grid, size, res, g);
	}
}

// The kernel's phases below are shared by two precisions of dL/dy and corner weight. A precision trait
// P carries what differs ("Grid backward: phases and precision traits"):
//   load<F>(level, i, dy)   the dL/dy loader: the point's F features of one level as fp32
//   round_weight(w)         the corner weight as the forward multiplied it
//   EXP_MAX                 upper clamp of the fixed-point exponent (grid_bwd_scale_exp)
//   POINTS_IN_FLIGHT        points per thread whose loads are issued together in the generic loops
//   FAST_2D                 the D == 2 paths tuned for the fp16 training step: accum_point_2d_fast, the
//                           register-resident chunk and the streaming pre-pass
//   OPTS_ALL_KINDS          the options instantiation dispatches on the index kind (else: IDX_GENERIC only)
//   SLAB_PAIR_ALIGNED       write_slab may store a packed pair with one 8-byte store
// This one: fp16 dL/dy in either layout of load_dy (grid_device.h), written by the fused kernel or a Module.
struct PrecF16 {
	// the forward multiplies fp16 table entries by fp16 weights (grid.h:150-167), so dL/dparam sees (half)w
	static __device__ __forceinline__ float round_weight(float w) { return (float)f16_rn(w); }
	// never reached: a non-zero sum of |fp16| is >= 2^-24, so lim < 2^55. Kept as the kernel always had it.
	static constexpr int EXP_MAX = GRID_BWD_EXP_MAX_F16;
	static constexpr uint32_t POINTS_IN_FLIGHT = 8;  // 2 or 4 bytes of dL/dy per point and feature pair: 8 loads hide one latency
	static constexpr bool FAST_2D = true;
	static constexpr bool OPTS_ALL_KINDS = true;
	// mode 0 items start at an even float of a slab: the slab buffer is the allocator's (256-byte aligned),
	// partial_stride = n_lds_params = entries * F, li.offset * F and begin * nf are even for nf = F = 2, f0 = 0
	static constexpr bool SLAB_PAIR_ALIGNED = true;
	int layout;
	const _Float16* dLdy;
	uint32_t dy_stride, B;
	template <uint32_t F>
	__device__ __forceinline__ void load(uint32_t level, uint32_t i, float* dy) const {
		load_dy<F>(layout, dLdy, dy_stride, level, B, i, dy);
	}
};

// One corner's add into the accumulators of entry `rel` -- the only place that issues the LDS atomics.
// MODE: 0 = F == 2, both features as one packed int64 (two int32 halves) per entry -> one
// ds_add_u64 per corner; 1 = the feature group [f0, f0 + nf) per entry (nf < F), ds_add_u32;
// 2 = all F features, ds_add_u32.
template <int MODE, uint32_t F>
__device__ __forceinline__ void lds_corner_add(int* acc, uint32_t rel, uint32_t f0, uint32_t nf, float w, const float (&dy)[F]) {
	if constexpr (MODE == 0) {
		const int a = __float2int_rn(w * dy[0]);
		const int b = __float2int_rn(w * dy[1]);
		const unsigned long long pk = (unsigned long long)(((long long)b << 32) + (long long)a);
		__hip_atomic_fetch_add((unsigned long long*)acc + rel, pk, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
	} else {
#pragma unroll
		for (uint32_t f = 0; f < F; ++f) {
			if constexpr (MODE == 1) {
				if (f - f0 < nf) lds_add_i32(&acc[rel * nf + (f - f0)], w * dy[f]);
			} else {
				lds_add_i32(&acc[rel * F + f], w * dy[f]);
			}
		}
	}
}

// One point's corner updates of one work item into the LDS accumulators (reference
// kernel_grid_backward's per-level body, grid.h:246-317): dy = the point's dL/dy already multiplied by
// the item's fixed-point scale.
template <typename P, uint32_t D, uint32_t F, HashType H, int KIND, int MODE, bool OPTS>
__device__ __forceinline__ void accum_point(const float (&x)[D], const float (&dy)[F], uint32_t i, uint32_t level, uint32_t B,
                                            const LevelInfo& li, bool hash_grid, Interp interp, uint32_t begin, uint32_t len,
                                            uint32_t f0, uint32_t nf, int* acc, const GridOpts& o) {
	float p[D];
	uint32_t pg[D];
#pragma unroll
	for (uint32_t d = 0; d < D; ++d) pos_fract(x[d], li.scale, interp, p[d], pg[d]);
	const bool nearest = interp == Interp::Nearest;
	// stochastic interpolation (grid.h:284-298): one corner, chosen per (point, level), weight 1
	const bool single = nearest || (OPTS && o.stochastic);
	uint32_t cbits = 0;
	if (single && !nearest) {
		const float smp = random_val_1337(i + level * B);
#pragma unroll
		for (uint32_t d = 0; d < D; ++d) cbits |= (smp >= p[d] ? 0u : 1u) << d;
	}
#pragma unroll
	for (uint32_t c0 = 0; c0 < (1u << D); ++c0) {
		if (single && c0 > 0) break;
		const uint32_t c = single ? cbits : c0;
		float w = 1.0f;
		uint32_t local[D];
#pragma unroll
		for (uint32_t d = 0; d < D; ++d) {
			if ((c & (1u << d)) == 0) { w *= 1.0f - p[d]; local[d] = pg[d]; }
			else { w *= p[d]; local[d] = pg[d] + 1; }
		}
		const float wh = single ? 1.0f : P::round_weight(w);
		const uint32_t rel = level_index<D, H, KIND>(hash_grid, li.size, li.res, local) - begin;
		if constexpr (KIND == IDX_GENERIC || KIND == IDX_HASH_RANGE) {  // entry slices may not cover the level
			if (rel >= len) continue;
		}
		lds_corner_add<MODE, F>(acc, rel, f0, nf, wh, dy);
	}
}

// One point's corner updates, D == 2, Linear interpolation, a whole level of kind HASH_POW2 or
// DENSE (for DENSE: a position in [0, 1], so every corner index is below 2 size) -- accum_point's
// arithmetic with the per-dimension hash / dense terms computed once per point and no control flow
// per corner. (As generic code the per-corner index and `% size` paths became exec-mask branches
// around every corner, as in the fused kernel's encode, r03.) fp16 weights: PrecF16::FAST_2D only.
template <uint32_t F, HashType H, int KIND, int MODE>
__device__ __forceinline__ void accum_point_2d_fast(const float (&x)[2], const float (&dy)[F], const LevelInfo& li, uint32_t f0,
                                                    uint32_t nf, int* acc, uint32_t begin = 0, uint32_t len = 0) {
	float p[2];
	uint32_t g[2];
	pos_fract(x[0], li.scale, Interp::Linear, p[0], g[0]);
	pos_fract(x[1], li.scale, Interp::Linear, p[1], g[1]);
	uint32_t t[2][2];
	if constexpr (KIND == IDX_HASH_POW2 || KIND == IDX_HASH_RANGE) {
		t[0][0] = g[0] * hash_prime<H>(0);
		t[0][1] = t[0][0] + hash_prime<H>(0);
		t[1][0] = g[1] * hash_prime<H>(1);
		t[1][1] = t[1][0] + hash_prime<H>(1);
	} else {
		t[0][0] = g[0];
		t[0][1] = g[0] + 1u;
		t[1][0] = g[1] * li.res;
		t[1][1] = t[1][0] + li.res;
	}
#pragma unroll
	for (uint32_t c = 0; c < 4; ++c) {
		const uint32_t bx = c & 1u, by = c >> 1;
		const float w = (bx ? p[0] : 1.0f - p[0]) * (by ? p[1] : 1.0f - p[1]);
		const float wh = (float)f16_rn(w);
		uint32_t rel;
		if constexpr (KIND == IDX_HASH_POW2) {
			rel = (t[0][bx] ^ t[1][by]) & (li.size - 1u);
		} else if constexpr (KIND == IDX_HASH_RANGE) {
			rel = ((t[0][bx] ^ t[1][by]) & (li.size - 1u)) - begin;
			if (rel >= len) continue;  // another range's corner (exec-masked, no branch around the point)
		} else {
			const uint32_t d = t[0][bx] + t[1][by];
			rel = __builtin_elementwise_min(d, d - li.size);  // d % size for d < 2 size
		}
		lds_corner_add<MODE, F>(acc, rel, f0, nf, wh, dy);
	}
}

// Register-resident variant (D == 2, F <= 2, no grid options): the chunk's dL/dy bits were loaded
// into dyb (GRID_BWD_PR points per thread, point i0 + threadIdx.x + p * blockDim.x in slot p) for the
// scale pre-pass and are reused here; positions stream in batches of 8 with the next batch in flight.
constexpr uint32_t GRID_BWD_PR = 32, GRID_BWD_PU = 8;
static_assert(GRID_BWD_THREADS * GRID_BWD_PR == GRID_BWD_REG_POINTS, "kernels.h GRID_BWD_REG_POINTS");
template <uint32_t D>
__device__ __forceinline__ void load_pos_batch(const float* __restrict__ pos, uint32_t pstride, uint32_t i0, uint32_t i1, uint32_t k,
                                               float (&dst)[GRID_BWD_PU][D]) {
#pragma unroll
	for (uint32_t u = 0; u < GRID_BWD_PU; ++u) {
		const uint32_t i = i0 + threadIdx.x + (k * GRID_BWD_PU + u) * blockDim.x;
#pragma unroll
		for (uint32_t d = 0; d < D; ++d) dst[u][d] = i < i1 ? pos[(size_t)i * pstride + d] : 0.0f;
	}
}

// The dL/dy bits (layout 0, F == 2) of batch k, beside its positions.
__device__ __forceinline__ void load_dy_batch(const uint32_t* __restrict__ dy_lv, uint32_t i0, uint32_t i1, uint32_t k,
                                              uint32_t (&dst)[GRID_BWD_PU]) {
#pragma unroll
	for (uint32_t u = 0; u < GRID_BWD_PU; ++u) {
		const uint32_t i = i0 + threadIdx.x + (k * GRID_BWD_PU + u) * blockDim.x;
		dst[u] = i < i1 ? dy_lv[i] : 0u;
	}
}

// STREAM: dyb holds only the first batch (slots 0 .. GRID_BWD_PU-1); the dL/dy bits of batch k + 1
// are loaded from dy_lv (the level's [B] half2 row) together with its positions while batch k is
// accumulated -- plain loads, the compiler places the waits. Same per-point arithmetic either way.
template <uint32_t D, uint32_t F, HashType H, int KIND, int MODE, bool STREAM = false>
__device__ __forceinline__ void grid_bwd_points_regs(const uint32_t (&dyb)[STREAM ? GRID_BWD_PU : GRID_BWD_PR],
                                                     const float (&xs0)[GRID_BWD_PU][D], const uint32_t* __restrict__ dy_lv,
                                                     uint32_t B, const float* __restrict__ pos,
                                                     uint32_t pstride, uint32_t level, const LevelInfo& li, bool hash_grid,
                                                     Interp interp, uint32_t begin, uint32_t len, uint32_t f0, uint32_t nf,
                                                     uint32_t i0, uint32_t i1, float scale, int* acc, const GridOpts& o) {
	constexpr uint32_t U = GRID_BWD_PU, NB = GRID_BWD_PR / U;
	constexpr bool FAST_KIND = D == 2 && (KIND == IDX_HASH_POW2 || KIND == IDX_DENSE || KIND == IDX_HASH_RANGE);
	const bool fast = FAST_KIND && interp == Interp::Linear && (begin == 0 || KIND == IDX_HASH_RANGE);  // whole levels or hash ranges
	float xs[2][U][D];
	uint32_t ds[2][STREAM ? U : 1];
#pragma unroll
	for (uint32_t u = 0; u < U; ++u) {
#pragma unroll
		for (uint32_t d = 0; d < D; ++d) xs[0][u][d] = xs0[u][d];
		if constexpr (STREAM) ds[0][u] = dyb[u];
	}
	// the dL/dy bits of point slot p = k U + u
	auto dy_bits = [&](uint32_t k, uint32_t u) -> uint32_t {
		if constexpr (STREAM) return ds[k & 1][u];
		else return dyb[k * U + u];
	};
#pragma unroll
	for (uint32_t k = 0; k < NB; ++k) {
		if (i0 + threadIdx.x + k * U * blockDim.x >= i1) break;
		if (k + 1 < NB) {
			load_pos_batch<D>(pos, pstride, i0, i1, k + 1, xs[(k + 1) & 1]);
			if constexpr (STREAM) load_dy_batch(dy_lv, i0, i1, k + 1, ds[(k + 1) & 1]);
		}
		bool fast_b = fast;
		if constexpr (FAST_KIND && KIND == IDX_DENSE) {  // dense corners below 2 size need positions in [0, 1]
			bool inr = true;
#pragma unroll
			for (uint32_t u = 0; u < U; ++u)
#pragma unroll
				for (uint32_t d = 0; d < D; ++d) inr = inr && xs[k & 1][u][d] >= 0.0f && xs[k & 1][u][d] <= 1.0f;
			fast_b = fast_b && __builtin_amdgcn_ballot_w64(!inr) == 0;
		}
		if (fast_b) {
			if constexpr (FAST_KIND) {
				if (i0 + threadIdx.x + (k * U + U - 1) * blockDim.x < i1) {  // the whole batch is inside the chunk
#pragma unroll
					for (uint32_t u = 0; u < U; ++u) {
						float dy[F];
#pragma unroll
						for (uint32_t f = 0; f < F; ++f) dy[f] = dy_bits_feature(dy_bits(k, u), f) * scale;
						accum_point_2d_fast<F, H, KIND, MODE>(*(const float(*)[2]) & xs[k & 1][u][0], dy, li, f0, nf, acc, begin, len);
					}
				} else {
					// the chunk's last, partial batch (e.g. 4 points per thread at 4096-point chunks: the
					// 2^15-point shard of N = 8): the same branch-free path per point that exists (r04 sent
					// these through the generic per-corner path, 3.5 us of accumulation for 4 points)
#pragma unroll
					for (uint32_t u = 0; u < U; ++u) {
						const uint32_t p = k * U + u;
						if (i0 + threadIdx.x + p * blockDim.x >= i1) break;
						float dy[F];
#pragma unroll
						for (uint32_t f = 0; f < F; ++f) dy[f] = dy_bits_feature(dy_bits(k, u), f) * scale;
						accum_point_2d_fast<F, H, KIND, MODE>(*(const float(*)[2]) & xs[k & 1][u][0], dy, li, f0, nf, acc, begin, len);
					}
				}
			}
			continue;
		}
#pragma unroll
		for (uint32_t u = 0; u < U; ++u) {
			const uint32_t p = k * U + u;
			const uint32_t i = i0 + threadIdx.x + p * blockDim.x;
			if (i >= i1) break;
			float dy[F];
#pragma unroll
			for (uint32_t f = 0; f < F; ++f) dy[f] = dy_bits_feature(dy_bits(k, u), f) * scale;
			accum_point<PrecF16, D, F, H, KIND, MODE, false>(xs[k & 1][u], dy, i, level, B, li, hash_grid, interp, begin, len, f0, nf, acc, o);
		}
	}
}

// The generic point loop of one (item, chunk): P::POINTS_IN_FLIGHT points per thread loaded together, then
// accumulated. Per thread the points are visited in increasing i with stride blockDim.x.
template <typename P, uint32_t D, uint32_t F, HashType H, int KIND, int MODE, bool OPTS>
__device__ __forceinline__ void grid_bwd_points(const P& src, uint32_t B, const float* __restrict__ pos, uint32_t pstride, uint32_t level,
                                                const LevelInfo& li, bool hash_grid, Interp interp, uint32_t begin,
                                                uint32_t len, uint32_t f0, uint32_t nf, uint32_t i0, uint32_t i1, float scale,
                                                int* acc, const GridOpts& o) {
	constexpr uint32_t NF = F;
	constexpr uint32_t U = P::POINTS_IN_FLIGHT;
	constexpr bool FAST_KIND = P::FAST_2D && D == 2 && !OPTS && (KIND == IDX_HASH_POW2 || KIND == IDX_DENSE || KIND == IDX_HASH_RANGE);
	const bool fast = FAST_KIND && interp == Interp::Linear && (begin == 0 || KIND == IDX_HASH_RANGE);  // accum_point_2d_fast
	for (uint32_t base = i0 + threadIdx.x; base < i1; base += U * blockDim.x) {
		float xs[U][D], dy[U][NF];
#pragma unroll
		for (uint32_t u = 0; u < U; ++u) {
			const uint32_t i = base + u * blockDim.x;
			float v[F];
			if (i < i1) {
#pragma unroll
				for (uint32_t d = 0; d < D; ++d) xs[u][d] = pos[(size_t)i * pstride + d];
				src.template load<F>(level, i, v);
			} else {
#pragma unroll
				for (uint32_t d = 0; d < D; ++d) xs[u][d] = 0.0f;
#pragma unroll
				for (uint32_t f = 0; f < F; ++f) v[f] = 0.0f;
			}
			if (OPTS && i < i1 && (float)level > grid_max_level(o, i, F) + 1e-3f) {  // masked (grid.h:242-244)
#pragma unroll
				for (uint32_t f = 0; f < F; ++f) v[f] = 0.0f;
			}
#pragma unroll
			for (uint32_t f = 0; f < F; ++f) dy[u][f] = v[f] * scale;
		}
		if constexpr (FAST_KIND) {
			bool fast_b = fast;
			if constexpr (KIND == IDX_DENSE) {
				bool inr = true;
#pragma unroll
				for (uint32_t u = 0; u < U; ++u)
#pragma unroll
					for (uint32_t d = 0; d < D; ++d) inr = inr && xs[u][d] >= 0.0f && xs[u][d] <= 1.0f;
				fast_b = fast_b && __builtin_amdgcn_ballot_w64(!inr) == 0;
			}
			if (fast_b && base + (U - 1) * blockDim.x < i1) {
#pragma unroll
				for (uint32_t u = 0; u < U; ++u)
					accum_point_2d_fast<F, H, KIND, MODE>(*(const float(*)[2]) & xs[u][0], dy[u], li, f0, nf, acc, begin, len);
				continue;
			}
		}
#pragma unroll
		for (uint32_t u = 0; u < U; ++u) {
			if (base + u * blockDim.x >= i1) break;
			accum_point<P, D, F, H, KIND, MODE, OPTS>(xs[u], dy[u], base + u * blockDim.x, level, B, li, hash_grid, interp, begin, len, f0,
			                                          nf, acc, o);
		}
	}
}

// ---------------------------------------------------------------------------------------------
// The phases of one (item, chunk) workgroup, in the kernels' order. Each takes its state as arguments.
// ---------------------------------------------------------------------------------------------

// Uniform per item: which index arithmetic its corners take (the IDX_ kinds above).
template <uint32_t D>
__device__ __forceinline__ int item_index_kind(const LevelInfo& li, const GridSlice& it, bool hash_grid) {
	uint64_t full = 1;
	for (uint32_t d = 0; d < D; ++d) full = full * li.res > 0xffffffffull ? 0x100000000ull : full * li.res;
	const bool whole = it.begin == 0 && it.end - it.begin == li.size;
	int kind = IDX_GENERIC;
	if (whole && full <= li.size) kind = IDX_DENSE;
	else if (whole && hash_grid && (li.size & (li.size - 1)) == 0) kind = IDX_HASH_POW2;
	else if (!whole && hash_grid && (li.size & (li.size - 1)) == 0 && full > li.size) kind = IDX_HASH_RANGE;
	return kind;
}

// Run-time index kind / accumulation mode -> template argument, as with_grid_shape (grid_dispatch.h):
// fn gets the value as a std::integral_constant. Every fn body is instantiated once per value, so nest
// them only where each combination is wanted. ALL_KINDS = false (P::OPTS_ALL_KINDS): one body, the
// generic index, which is right for every item.
template <bool ALL_KINDS = true, typename Fn>
__device__ __forceinline__ void with_index_kind(int kind, Fn&& fn) {
	if constexpr (ALL_KINDS) {
		if (kind == IDX_HASH_POW2) return fn(std::integral_constant<int, IDX_HASH_POW2>{});
		if (kind == IDX_HASH_RANGE) return fn(std::integral_constant<int, IDX_HASH_RANGE>{});
		if (kind == IDX_DENSE) return fn(std::integral_constant<int, IDX_DENSE>{});
	}
	fn(std::integral_constant<int, IDX_GENERIC>{});
}

// The accumulation modes F allows (lds_corner_add): packed pairs only for F == 2, all-F only for F > 2;
// everything else (feature groups, F == 1) is mode 1.
__device__ __forceinline__ int item_accum_mode(uint32_t F, uint32_t nf) { return nf < F || F == 1 ? 1 : (F == 2 ? 0 : 2); }
template <uint32_t F, typename Fn>
__device__ __forceinline__ void with_accum_mode(int mode, Fn&& fn) {
	if constexpr (F == 2) {
		if (mode == 0) return fn(std::integral_constant<int, 0>{});
	} else if constexpr (F > 2) {
		if (mode == 2) return fn(std::integral_constant<int, 2>{});
	}
	fn(std::integral_constant<int, 1>{});
}

// Replicas: a small level's accumulators fit the LDS several times; wave w adds into replica
// w % R, which divides the same-address atomic serialisation on the coarse dense levels
// (level 0: 256 entries hit by every point) by up to R. Integer sums: merge_replicas is exact and
// order-independent.
struct AccLayout {
	uint32_t slots;  // int32 slots of one replica (F = 2 packed pairs: 2 per entry)
	uint32_t R, nz;  // replicas; slots to zero
	int* acc_w;      // this wave's replica
};
__device__ __forceinline__ AccLayout make_acc_layout(int* acc, uint32_t len, uint32_t nf) {
	AccLayout a;
	a.slots = len * nf;
	a.R = max(1u, min(16u, GRID_BWD_SLOTS / max(a.slots, 1u)));
	a.nz = a.R * a.slots;
	a.acc_w = acc + ((threadIdx.x >> 6) % a.R) * a.slots;
	return a;
}

__device__ __forceinline__ void zero_accumulators(int* acc, const AccLayout& a) {
	for (uint32_t j = 4 * threadIdx.x; j + 4 <= a.nz; j += 4 * blockDim.x) *(int4*)(acc + j) = int4{0, 0, 0, 0};  // ds_write_b128
	for (uint32_t j = a.nz / 4 * 4 + threadIdx.x; j < a.nz; j += blockDim.x) acc[j] = 0;
}

// Sums every replica into replica 0 and ends with a barrier. packed: the int64 pairs of mode 0 (a carry
// out of the low half must reach the high half, as in the adds themselves).
__device__ __forceinline__ void merge_replicas(int* acc, const AccLayout& a, uint32_t len, bool packed) {
	if (a.R <= 1) return;
	if (packed) {
		long long* a64 = (long long*)acc;
		for (uint32_t j = threadIdx.x; j < len; j += blockDim.x) {
			long long t = a64[j];
			for (uint32_t r = 1; r < a.R; ++r) t += a64[(size_t)r * len + j];
			a64[j] = t;
		}
	} else {
		for (uint32_t j = threadIdx.x; j < a.slots; j += blockDim.x) {
			int t = acc[j];
			for (uint32_t r = 1; r < a.R; ++r) t += acc[(size_t)r * a.slots + j];
			acc[j] = t;
		}
	}
	__syncthreads();
}

// The workgroup's sum of the threads' m, the same float in every thread: a 6-step xor butterfly per
// wave, red[wave], a barrier, then the 16 wave sums added in wave order. The order is part of the
// contract: grid_bwd_scale_guard (grid_bwd_scale.h) is proved for exactly these roundings, and the
// streaming and exact pre-pass must agree on them. red[] may be rewritten only after another barrier.
__device__ __forceinline__ float block_sum_waves(float m, float* red) {
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) m += __shfl_xor(m, o);
	if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
	__syncthreads();
	m = red[0];
#pragma unroll
	for (uint32_t w = 1; w < GRID_BWD_THREADS / 64; ++w) m += red[w];
	return m;
}

// A point's term of the scale bound: max over the item's features of |dL/dy|; +inf for a non-finite one
template <uint32_t F>
__device__ __forceinline__ float dy_bound_term(const float (&dy)[F], uint32_t f0, uint32_t nf) {
	float s = 0.0f;
#pragma unroll
	for (uint32_t f = 0; f < F; ++f)
		if (f - f0 < nf) s = __builtin_isfinite(dy[f]) ? fmaxf(s, fabsf(dy[f])) : __builtin_inff();
	return s;
}

// Exact pre-pass, generic: this thread's sum of the bound terms over the chunk, points in increasing i
// with stride blockDim.x whatever P::POINTS_IN_FLIGHT is (so m is the same float for every batching).
template <typename P, uint32_t F>
__device__ __forceinline__ float dy_bound_sum(const P& src, uint32_t level, uint32_t f0, uint32_t nf, uint32_t i0, uint32_t i1) {
	constexpr uint32_t U = P::POINTS_IN_FLIGHT;
	float m = 0.0f;
	for (uint32_t ib = i0 + threadIdx.x; ib < i1; ib += U * blockDim.x) {
		float dy[U][F];
#pragma unroll
		for (uint32_t u = 0; u < U; ++u) {
			const uint32_t i = ib + u * blockDim.x;
			if (i < i1) src.template load<F>(level, i, dy[u]);
			else {
#pragma unroll
				for (uint32_t f = 0; f < F; ++f) dy[u][f] = 0.0f;
			}
		}
#pragma unroll
		for (uint32_t u = 0; u < U; ++u) m += dy_bound_term<F>(dy[u], f0, nf);
	}
	return m;
}

// Slab store policies of write_slab: plain stores, or write-through (wt_store.h: the slab is read by the
// next launch only -- k_adam, or the sequential reductions). The 16-byte write-through stores go through a
// buffer resource over the workgroup's own range (wave-uniform base, small offsets). PAIR8: dst + 2 j is
// 8-byte aligned for every j (P::SLAB_PAIR_ALIGNED), so a packed pair is one store.
template <bool PAIR8>
struct SlabStorePlain {
	__device__ __forceinline__ SlabStorePlain(float*, uint32_t) {}
	__device__ __forceinline__ void quad(float* dst, uint32_t j, f4 v) const { *(f4*)(dst + j) = v; }
	__device__ __forceinline__ void pair(float* p, float2 v) const {
		if constexpr (PAIR8) *(float2*)p = v;
		else { p[0] = v.x; p[1] = v.y; }
	}
	__device__ __forceinline__ void one(float* p, float v) const { *p = v; }
};
struct SlabStoreWriteThrough {
	wt_rsrc rs;
	__device__ __forceinline__ SlabStoreWriteThrough(float* dst, uint32_t bytes) : rs(wt_make_rsrc(dst, bytes)) {}
	__device__ __forceinline__ void quad(float*, uint32_t j, f4 v) const { wt_store16(rs, 4 * j, v); }
	__device__ __forceinline__ void pair(float* p, float2 v) const { wt_store((float2*)p, v); }
	__device__ __forceinline__ void one(float* p, float v) const { wt_store(p, v); }
};

// Decode replica 0 (int32 fixed point times inv = 2^-e) into the item's run of the chunk slab: len * nf
// floats at dst, contiguous because the plan's items tile their levels (check_items_tile_levels,
// runtime.cpp). 16-byte stores where dst is 16-byte aligned. PACKED: the int64 pairs of mode 0, nf == 2.
template <typename Store, bool PACKED>
__device__ __forceinline__ void write_slab(const int* acc, float* dst, uint32_t len, uint32_t nf, float inv) {
	const uint32_t n = len * nf;
	const Store st(dst, n * 4);
	const bool al = (((uintptr_t)dst) & 15) == 0;
	if constexpr (PACKED) {  // two entries per thread
		const long long* a64 = (const long long*)acc;
		auto dec = [inv](long long t) {
			const int lo = (int)(uint32_t)(unsigned long long)t;
			const int hi = (int)((t - (long long)lo) >> 32);
			return make_float2((float)lo * inv, (float)hi * inv);
		};
		for (uint32_t j = 2 * threadIdx.x; j < len; j += 2 * blockDim.x) {
			const float2 a = dec(a64[j]);
			if (al && j + 1 < len) {
				const float2 b = dec(a64[j + 1]);
				st.quad(dst, 2 * j, f4{a.x, a.y, b.x, b.y});
			} else {
				st.pair(dst + 2 * j, a);
				if (j + 1 < len) st.pair(dst + 2 * j + 2, dec(a64[j + 1]));
			}
		}
	} else {
		for (uint32_t j = 4 * threadIdx.x; j < n; j += 4 * blockDim.x) {
			if (al && j + 4 <= n) {
				const int4 v = *(const int4*)(acc + j);
				st.quad(dst, j, f4{(float)v.x * inv, (float)v.y * inv, (float)v.z * inv, (float)v.w * inv});
			} else {
				for (uint32_t k = j; k < n && k < j + 4; ++k) st.one(dst + k, (float)acc[k] * inv);
			}
		}
	}
}

// Debug time stamp k of this workgroup (dbg_times: 8 per workgroup, null in normal runs)
__device__ __forceinline__ void dbg_stamp(unsigned long long* dbg_times, uint32_t k, unsigned long long extra = 0ull) {
	if (dbg_times && threadIdx.x == 0) dbg_times[8 * blockIdx.x + k] = wall_clock64() + extra;
}

// Network-gradient tail (extra workgroups g = 0 .. n_mlp_groups-1, on CUs the grid items leave
// free): workgroup g sums the fused kernel's slabs for its block of network-parameter columns
// (block_column_sums: the same order as launch_column_sums of the sequential path), applies Adam
// to those parameters and writes them into the next step's fused weight image. No cross-workgroup
// dependency. Workgroup 0 also sums the loss partials and publishes the bias-correction factor.
__device__ __forceinline__ void grid_bwd_mlp_tail(const GridBwdEpilogue& ep, uint32_t g, float* lds) {
	const uint32_t N = ep.n_mlp;
	const uint32_t cb = column_block(N, ep.n_mlp_groups);
	const uint32_t c0 = g * cb;
	if (c0 < N) {
		const uint32_t ncol = min(cb, N - c0);
		float* out = lds;
		float* tmp = lds + cb;
		block_column_sums(ep.wpart, ep.n_wparts, N, c0, ncol, tmp, out);
		const uint32_t nW0 = ep.W * ep.IN, nWh = (ep.NH - 1) * ep.W * ep.W;
		for (uint32_t t = threadIdx.x; t < ncol; t += blockDim.x) {
			const uint32_t i = c0 + t;
			const float s = out[t];
			if (ep.fin.out) {
				grad_finalize_store(s, ep.fin.s, ep.fin.out, i, ep.fin.out_f32);
				continue;
			}
			ep.buf.g32[i] = s;
			if (!ep.apply_adam) continue;
			const _Float16 h = adam_update(ep.adam_mlp, ep.buf, i, s);
			uint32_t o;
			if (i < nW0) {
				o = (i / ep.IN) * ep.RSI + i % ep.IN;
			} else if (i < nW0 + nWh) {
				const uint32_t k = i - nW0;
				o = ep.oWh + (k / ep.W) * ep.RSW + k % ep.W;  // rows of all hidden matrices are consecutive
			} else {
				const uint32_t k = i - nW0 - nWh;
				o = ep.oWo + (4 * ((k / ep.W) & 3) + (k / ep.W) / 4) * ep.RSW + k % ep.W;  // out_row (mlp_fused.h)
			}
			ep.wimage[o] = h;
		}
	}
	if (g == 0) {
		__syncthreads();
		const float l = block_sum_fixed(ep.lpart, ep.n_wparts, lds);
		if (threadIdx.x == 0) *ep.d_loss = l;
	}
}

// The work plan by value (kernel arguments, read with scalar loads): the first thing every workgroup
// needs, so it must not cost a dependent global load at the head of the launch (r06). Plans larger
// than the tables keep reading the device copies.
constexpr uint32_t GRID_BWD_ARG_ITEMS = 32, GRID_BWD_ARG_LEVELS = 24;
struct GridBwdTables {
	uint32_t n_items, n_levels;  // entries valid below (0: read the device arrays)
	GridSlice items[GRID_BWD_ARG_ITEMS];
	LevelInfo levels[GRID_BWD_ARG_LEVELS];
};

// One workgroup = one (work item, chunk of points), or one block of the network-gradient tail.
template <uint32_t D, uint32_t F, HashType H, bool OPTS>
__global__ __launch_bounds__(GRID_BWD_THREADS) void k_grid_bwd_lds(
	int layout, uint32_t B, const float* __restrict__ pos, uint32_t pstride, const _Float16* __restrict__ dLdy, uint32_t dy_stride,
	const GridSlice* __restrict__ items, float* __restrict__ partial, uint32_t partial_stride,
	const LevelInfo* __restrict__ levels, uint32_t hash_grid, uint32_t interp_u, uint32_t pts_per_chunk, uint32_t n_items,
	uint32_t n_chunks, const GridBwdEpilogue ep, unsigned long long* dbg_times, const GridOpts o, const GridBwdTables tb,
	const float* __restrict__ dy_bound, uint32_t* fallback_count, uint32_t wt_stores) {
	extern __shared__ __attribute__((aligned(16))) int acc[];
	const unsigned long long t_start = dbg_times ? wall_clock64() : 0ull;
	__shared__ float red[GRID_BWD_THREADS / 64];
	// 1. tail dispatch
	if (blockIdx.x >= n_items * n_chunks) {
		grid_bwd_mlp_tail(ep, blockIdx.x - n_items * n_chunks, (float*)acc);
		if (dbg_times && threadIdx.x == 0) {
			dbg_times[8 * blockIdx.x] = t_start;
			for (int k = 1; k < 5; ++k) dbg_times[8 * blockIdx.x + k] = wall_clock64();
		}
		return;
	}
	// 2. item and level load.
	// chunk-minor numbering: blocks are dealt round-robin over the 8 XCDs, so with 8 chunks every
	// item of chunk c lands on one XCD and the chunk's positions (re-read by all 26 items of
	// config_hash) stay in that XCD's L2
	const uint32_t item = blockIdx.x / n_chunks, chunk = blockIdx.x % n_chunks;
	GridSlice it;
	if (item < tb.n_items) {  // wave-uniform: scalar loads from the kernel arguments
		it.level = tb.items[item].level;
		it.begin = tb.items[item].begin;
		it.end = tb.items[item].end;
		it.f0 = tb.items[item].f0;
		it.nf = tb.items[item].nf;
	} else {
		it = items[item];
	}
	const uint32_t len = it.end - it.begin;
	const uint32_t nf = it.nf, f0 = it.f0;
	const Interp interp = (Interp)interp_u;
	const uint32_t i0 = chunk * pts_per_chunk;
	const uint32_t i1 = min(B, i0 + pts_per_chunk);
	const PrecF16 src{layout, dLdy, dy_stride, B};

	// The pre-pass: sum of |dL/dy| of this item's features over the chunk -> fixed-point scale. No entry
	// can receive more than that sum (the corner weights of a point sum to 1, hash collisions
	// included), so 2^e (sum + rounding) < 2^31 cannot overflow, and one outlier dL/dy costs the
	// other entries almost no resolution (a max-based bound would lose its whole ratio to the mean).
	// A non-finite dL/dy makes the item's gradient NaN (the reference's fp16 sums would carry it).
	// D == 2, F <= 2 without grid options, and a chunk of at most GRID_BWD_PR points per thread (the
	// config_hash step: 32768-point chunks): the chunk's dL/dy bits are loaded once, all of them in
	// flight together, kept in registers for the accumulation, and the pre-pass is one load latency
	// instead of one per 8 points. The loads are issued first -- they need only the item -- so the
	// level table's load and the accumulators' zeroing run in their shadow (r05: at 2^15 points the
	// item load -> level load -> zeroing -> dL/dy load chain was ~5 us of a 13 us item)
	constexpr bool REGS_OK = PrecF16::FAST_2D && D == 2 && F <= 2 && !OPTS;
	const uint32_t n_pts = i1 > i0 ? i1 - i0 : 0u;
	const bool use_regs = REGS_OK && n_pts <= GRID_BWD_THREADS * GRID_BWD_PR;
	LevelInfo li;
	if (it.level < tb.n_levels) {
		li.scale = tb.levels[it.level].scale;
		li.res = tb.levels[it.level].res;
		li.offset = tb.levels[it.level].offset;
		li.size = tb.levels[it.level].size;
	} else {
		li = levels[it.level];
	}
	// 3. layout
	const AccLayout lay = make_acc_layout(acc, len, nf);
	const int mode = item_accum_mode(F, nf);
	int e = 0;           // the fixed-point exponent: floor(log2(lim)), grid_bwd_scale.h
	bool finite = true;  // the chunk's sum of |dL/dy| is finite

	// 4. the streaming attempt (dy_bound: the fused kernel's per-slice sums of max_f |dL/dy|, [level][B / 32]):
	// the scale comes from the chunk's <= 1024 slice sums -- one 4-byte load per thread instead of 32
	// -- and dL/dy streams in batches under the accumulation, like the positions. The slice sums add
	// up in another order than the exact pre-pass, so the exponent is taken from them only where
	// grid_bwd_scale_guard proves it equal; otherwise the workgroup (uniformly) runs the exact path
	// below from its start (it zeroes the accumulators again; no update has been issued yet).
	// The two paths are disjoint blocks so that neither's registers live across the other. This phase
	// stays a block of the kernel body: as a function of its own the same code compiled to a slower
	// schedule of the 8-point batches (0.7 us at 2^18, profiles/grid_bwd_phases_ab.txt).
	constexpr bool STREAM_OK = REGS_OK && F == 2;
	const float P = (float)(i1 > i0 ? i1 - i0 : 1u);
	bool stream = false;  // workgroup-uniform
	if constexpr (STREAM_OK) {
		const uint32_t n_sl = n_pts / 32u;
		if (dy_bound && layout == 0 && nf == F && use_regs && n_pts > 0 && ((i0 | i1) & 31u) == 0 && n_sl <= GRID_BWD_THREADS) {
			float mh = threadIdx.x < n_sl ? dy_bound[(size_t)it.level * (B / 32u) + i0 / 32u + threadIdx.x] : 0.0f;
			const uint32_t* dy_lv = (const uint32_t*)dLdy + (size_t)it.level * B;
			uint32_t ds0[GRID_BWD_PU];  // the first batch's dL/dy bits and positions, in flight across the reduction
			float xs0[GRID_BWD_PU][D];
			load_dy_batch(dy_lv, i0, i1, 0, ds0);
			load_pos_batch<D>(pos, pstride, i0, i1, 0, xs0);
			zero_accumulators(acc, lay);
			dbg_stamp(dbg_times, 6);  // zeroing issued
			mh = block_sum_waves(mh, red);  // the exact reduction's butterfly and wave order over the slice sums
			stream = grid_bwd_scale_guard(mh, P, D);
			if (stream) {
				e = grid_bwd_scale_exp(mh, P, D, PrecF16::EXP_MAX);
				const float scale = ldexpf(1.0f, e);
				if (dbg_times && threadIdx.x == 0) dbg_times[8 * blockIdx.x + 5] = dbg_times[8 * blockIdx.x + 1] = wall_clock64();
				// nf == F == 2: packed pairs (MODE 0)
				with_index_kind(item_index_kind<D>(li, it, hash_grid != 0), [&](auto k) __attribute__((always_inline)) {
					grid_bwd_points_regs<D, F, H, decltype(k)::value, 0, true>(ds0, xs0, dy_lv, B, pos, pstride, it.level, li, hash_grid != 0, interp,
					                                                           it.begin, len, f0, nf, i0, i1, scale, lay.acc_w, o);
				});
			} else {  // inside the guard band, or a non-finite sum
				if (fallback_count && threadIdx.x == 0) atomicAdd(fallback_count, 1u);
				__syncthreads();  // red[] is rewritten by the exact reduction
			}
		}
	}
	if (!stream) {
		// 5. the exact pre-pass (it zeroes the accumulators again after a refused attempt; no update has been issued yet)
		float m = 0.0f;
		uint32_t dyb[GRID_BWD_PR];
		float xs0[GRID_BWD_PU][D];  // the accumulation's first position batch, in flight across the scale reduction
		// Register-resident chunk: all of its dL/dy bits in flight together, the accumulation's first
		// position batch behind them; the sum below runs over the same points in the same order. These two
		// loops stay in the kernel body, on the kernel's own arguments: as functions over the trait object
		// the pre-pass of a 2^15-point chunk took 8.8 us instead of 7.3 (profiles/grid_bwd_phases_ab.txt).
		if constexpr (REGS_OK) {
			if (use_regs) {
#pragma unroll
				for (uint32_t p = 0; p < GRID_BWD_PR; ++p) {
					const uint32_t i = i0 + threadIdx.x + p * blockDim.x;
					dyb[p] = i < i1 ? load_dy_bits<F>(layout, dLdy, dy_stride, it.level, B, i) : 0u;
				}
				load_pos_batch<D>(pos, pstride, i0, i1, 0, xs0);
			}
		}
		zero_accumulators(acc, lay);
		dbg_stamp(dbg_times, 6);  // zeroing issued
		if constexpr (REGS_OK) {
			if (use_regs) {
#pragma unroll
				for (uint32_t p = 0; p < GRID_BWD_PR; ++p) {
					float s = 0.0f;
#pragma unroll
					for (uint32_t f = 0; f < F; ++f) {
						const float v = dy_bits_feature(dyb[p], f);
						if (f - f0 < nf) s = __builtin_isfinite(v) ? fmaxf(s, fabsf(v)) : __builtin_inff();
					}
					m += s;
				}
			}
		}
		if (!use_regs) m += dy_bound_sum<PrecF16, F>(src, it.level, f0, nf, i0, i1);
		dbg_stamp(dbg_times, 5, m != m ? 1 : 0);  // dL/dy loads done
		m = block_sum_waves(m, red);
		finite = __builtin_isfinite(m);
		e = grid_bwd_scale_exp(m, P, D, PrecF16::EXP_MAX);
		const float scale = ldexpf(1.0f, e);
		dbg_stamp(dbg_times, 1);  // zeroing + pre-pass done
		// 6. accumulate
		const int kind = item_index_kind<D>(li, it, hash_grid != 0);
		if constexpr (REGS_OK) {
			if (use_regs)
				with_index_kind<PrecF16::OPTS_ALL_KINDS || !OPTS>(kind, [&](auto k) __attribute__((always_inline)) {
					with_accum_mode<F>(mode, [&](auto md) __attribute__((always_inline)) {
						grid_bwd_points_regs<D, F, H, decltype(k)::value, decltype(md)::value>(dyb, xs0, nullptr, B, pos, pstride, it.level, li, hash_grid != 0,
						                                                                        interp, it.begin, len, f0, nf, i0, i1, scale, lay.acc_w, o);
					});
				});
		}
		if (!use_regs)
			with_index_kind<PrecF16::OPTS_ALL_KINDS || !OPTS>(kind, [&](auto k) __attribute__((always_inline)) {
				with_accum_mode<F>(mode, [&](auto md) __attribute__((always_inline)) {
					grid_bwd_points<PrecF16, D, F, H, decltype(k)::value, decltype(md)::value, OPTS>(src, B, pos, pstride, it.level, li, hash_grid != 0, interp,
					                                                                                 it.begin, len, f0, nf, i0, i1, scale, lay.acc_w, o);
				});
			});
	}
	__syncthreads();
	dbg_stamp(dbg_times, 2);  // accumulation done
	// 7. merge
	merge_replicas(acc, lay, len, mode == 0);
	dbg_stamp(dbg_times, 3);  // replica merge done
	// 8. write the chunk slab (GridSlabMap layout)
	const float inv = finite ? ldexpf(1.0f, -e) : __builtin_nanf("");
	float* dst = partial + (size_t)chunk * partial_stride + (size_t)li.offset * F + (size_t)f0 * li.size + (size_t)it.begin * nf;
	const bool wt = (wt_stores & WT_GRID_SLAB) != 0;
	using Plain = SlabStorePlain<PrecF16::SLAB_PAIR_ALIGNED>;
	if (mode == 0) {
		if (wt) write_slab<SlabStoreWriteThrough, true>(acc, dst, len, nf, inv);
		else write_slab<Plain, true>(acc, dst, len, nf, inv);
	} else {
		if (wt) write_slab<SlabStoreWriteThrough, false>(acc, dst, len, nf, inv);
		else write_slab<Plain, false>(acc, dst, len, nf, inv);
	}
	if (dbg_times && threadIdx.x == 0) {
		dbg_times[8 * blockIdx.x] = t_start;
		dbg_times[8 * blockIdx.x + 4] = wall_clock64();
	}
}

// One launch of k_grid_bwd_lds: its grid and its arguments, in the kernel's parameter order
// (launch_grid_bwd in grid.hip fills it; grid_bwd_d<D> picks the instantiation).
struct GridBwdLaunch {
	uint32_t n_workgroups;  // n_items * n_chunks + the epilogue's tail workgroups
	int layout;
	uint32_t B;
	const float* pos;
	uint32_t pos_stride;
	const _Float16* dLdy;
	uint32_t dy_stride;
	const GridSlice* items;
	float* partial;
	uint32_t partial_stride;
	const LevelInfo* levels;
	uint32_t hash_grid, interp, pts_per_chunk;
	uint32_t n_items, n_chunks;
	GridBwdEpilogue ep;
	unsigned long long* dbg_times;
	GridOpts opts;
	GridBwdTables tb;
	const float* dy_bound;     // the fused kernel's slice sums of max_f |dL/dy| (null: every workgroup takes the exact pre-pass)
	uint32_t* fallback_count;  // debug: workgroups that had dy_bound but took the exact pre-pass (null: not counted)
	uint32_t wt_stores;        // WT_GRID_SLAB (wt_store.h): the chunk slabs are written through L2
};

template <uint32_t D, uint32_t F, HashType H>
static void grid_bwd_t(hipStream_t st, const GridBwdLaunch& gl) {
	// the options (max_level, stochastic) are a separate instantiation: the default kernel stays lean
	static uint64_t done0 = 0, done1 = 0;
	set_dyn_lds((const void*)k_grid_bwd_lds<D, F, H, false>, (int)GRID_BWD_LDS_BYTES, done0);
	set_dyn_lds((const void*)k_grid_bwd_lds<D, F, H, true>, (int)GRID_BWD_LDS_BYTES, done1);
	const auto kernel = gl.opts.active ? k_grid_bwd_lds<D, F, H, true> : k_grid_bwd_lds<D, F, H, false>;
	hipLaunchKernelGGL(kernel, dim3(gl.n_workgroups), dim3(GRID_BWD_THREADS), GRID_BWD_LDS_BYTES, st, gl.layout, gl.B, gl.pos, gl.pos_stride,
	                   gl.dLdy, gl.dy_stride, gl.items, gl.partial, gl.partial_stride, gl.levels, gl.hash_grid, gl.interp, gl.pts_per_chunk,
	                   gl.n_items, gl.n_chunks, gl.ep, gl.dbg_times, gl.opts, gl.tb, gl.dy_bound, gl.fallback_count, gl.wt_stores);
}

// every (F, hash) instantiation of one D: instantiated in grid_bwd_d{2,3,4}.hip only
template <uint32_t D>
void grid_bwd_d(hipStream_t st, uint32_t F, HashType h, const GridBwdLaunch& gl) {
	with_grid_features(F, [&](auto f) {
		with_grid_hash(h, [&](auto hh) { grid_bwd_t<D, decltype(f)::value, decltype(hh)::value>(st, gl); });
	});
}

}  // namespace tcnn_amd
