// grid_f32.hip -- the multiresolution grid of an fp32-precision encoding module for gfx950
// (reference grid.h with T = float: create_encoding<float>, Encoding(dtype=float32)):
//   k_grid_fwd_f32      fp32 table -> AoS fp32 rows [B][out_stride]
//   k_grid_bwd_lds_f32  fp32 dL/dy (AoS) -> per-chunk fp32 gradient slabs, LDS-privatised int32 sums
// Nothing here is narrowed to fp16: table entries, corner weights, dL/dy and the output stay fp32.
// The index arithmetic is grid_device.h's (pos_fract, grid_index, the reference's corner order), so
// the entries touched are those of the fp16 kernels. dL/dinput and the second-order kernels are the
// typed k_grid_bwd_input / k_grid_bwd_bwd of grid.hip.
#include "kernels.h"

#include <algorithm>

#include "grid_bwd_lds.h"
#include "grid_device.h"
#include "grid_dispatch.h"

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
#pragma unroll
	for (uint32_t c = 0; c < NC; ++c) {  // every gather issued before the FMA chain consumes one
		float wc = 1.0f;
		uint32_t local[D];
#pragma unroll
		for (uint32_t d = 0; d < D; ++d) {
			if ((c & (1u << d)) == 0) { wc *= 1.0f - p[d]; local[d] = pg[d]; }
			else { wc *= p[d]; local[d] = pg[d] + 1; }
		}
		w[c] = wc;
		v[c] = load_fvec<F>(table + (size_t)(li.offset + grid_index<D, H>(hash_grid, li.size, li.res, local)) * F, vec);
	}
#pragma unroll
	for (uint32_t f = 0; f < F; ++f) r[f] = 0.0f;
#pragma unroll
	for (uint32_t c = 0; c < NC; ++c)
#pragma unroll
		for (uint32_t f = 0; f < F; ++f) r[f] = __builtin_fmaf(w[c], v[c].v[f], r[f]);
}

// AoS forward: one thread per point and group of G consecutive levels, G * F >= 4 features, so a thread
// writes 16 contiguous bytes of its row (32 for F = 8) in dwordx4 stores and consecutive threads write
// consecutive groups of a row. vec bit 0: the table allows FVec loads; bit 1: rows allow 16-byte stores.
// Only the value columns [0, L * F) are written (padding is the caller's: memset or k_composite_fwd).
template <uint32_t D, uint32_t F, HashType H>
__global__ __launch_bounds__(256) void k_grid_fwd_f32(uint32_t B, const float* __restrict__ pos, uint32_t pstride,
                                                      const float* __restrict__ table, float* __restrict__ out, uint32_t out_stride,
                                                      const LevelInfo* __restrict__ levels, uint32_t hash_grid, uint32_t interp_u,
                                                      const GridOpts o, uint32_t L, uint32_t vec) {
	constexpr uint32_t G = F >= 4 ? 1 : 4 / F;
	const uint32_t NG = (L + G - 1) / G;
	const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
	const uint32_t i = t / NG, g = t - i * NG;
	if (i >= B) return;
	const Interp interp = (Interp)interp_u;
	float x[D];
#pragma unroll
	for (uint32_t d = 0; d < D; ++d) x[d] = pos[(size_t)i * pstride + d];
	const float ml = o.active ? grid_max_level(o, i, F) + 1e-3f : 3.0e38f;
	float r[G * F];
#pragma unroll
	for (uint32_t k = 0; k < G; ++k) {
		const uint32_t level = g * G + k;
#pragma unroll
		for (uint32_t f = 0; f < F; ++f) r[k * F + f] = 0.0f;
		if (level < L && !((float)level >= ml))  // masked level: output 0 (grid.h:75-91)
			encode_level_f32<D, F, H>(table, levels[level], hash_grid != 0, interp, x, (vec & 1u) != 0, r + k * F);
	}
	float* row = out + (size_t)i * out_stride + g * G * F;
	if ((vec & 2u) && g * G + G <= L) {
#pragma unroll
		for (uint32_t q = 0; q < G * F / 4; ++q) *(f4*)(row + 4 * q) = f4{r[4 * q], r[4 * q + 1], r[4 * q + 2], r[4 * q + 3]};
	} else {
#pragma unroll
		for (uint32_t k = 0; k < G; ++k)
			if (g * G + k < L)
#pragma unroll
				for (uint32_t f = 0; f < F; ++f) row[k * F + f] = r[k * F + f];
	}
}

void launch_grid_fwd_f32(hipStream_t st, const GridCall& gc, uint32_t B, const float* pos, uint32_t pos_stride, const float* table32,
                         float* out32, uint32_t out_stride) {
	if (B == 0) return;
	TCNN_CHECK(gc.L * gc.F <= out_stride, "GridEncoding: fp32 rows narrower than the grid's features");
	with_grid_shape(gc.D, gc.F, gc.hash, [&](auto d, auto f, auto h) {
		constexpr uint32_t D = decltype(d)::value, F = decltype(f)::value;
		constexpr HashType H = decltype(h)::value;
		// FVec loads: entry e sits at table + e F, so the base decides; 16-byte row stores: base and stride
		constexpr uint32_t tb = F * 4u < 16u ? F * 4u : 16u;
		const uint32_t vec = (((uintptr_t)table32 % tb) == 0 ? 1u : 0u) | ((((uintptr_t)out32 % 16) == 0 && out_stride % 4 == 0) ? 2u : 0u);
		constexpr uint32_t G = F >= 4 ? 1 : 4 / F;  // levels per thread (k_grid_fwd_f32)
		const uint64_t n = (uint64_t)B * ((gc.L + G - 1) / G);
		TCNN_CHECK(n < (1ull << 32), "GridEncoding: batch too large for one fp32 forward launch");
		hipLaunchKernelGGL((k_grid_fwd_f32<D, F, H>), dim3(div_round_up(n, 256)), dim3(256), 0, st, B, pos, pos_stride, table32, out32,
		                   out_stride, gc.levels, gc.hash_grid ? 1u : 0u, (uint32_t)gc.interp, gc.opts, gc.L, vec);
	});
	TCNN_HIP_CHECK(hipGetLastError());
}

// =============================================================================================
// backward to the parameters: fp32 dL/dy (AoS rows) -> fp32 gradient slabs
// =============================================================================================
// The LDS-privatised plan of grid_bwd_lds.h with an fp32 AoS dL/dy loader and fp32 corner weights: one
// work item = (level, entry range) with all F features, accumulated for one chunk of points in int32
// fixed point (ds_add_u32 / ds_add_u64: ~25x the rate of LDS float atomics, and order-independent, so
// the gradient is bit-reproducible). An update is fp32(w * dy * 2^e) rounded to the nearest integer;
// 2^e is the item's scale from the chunk's sum of |dL/dy| as in k_grid_bwd_lds. Items always hold all F
// features (GridEncodingHost::plan_f32), so the slabs are in parameter order.

// The fp32 precision trait of the phases in grid_bwd_lds.h (the fields: see PrecF16 there).
struct PrecF32 {
	// the fp32 forward multiplies fp32 entries by the unrounded fp32 weight (encode_level_f32)
	static __device__ __forceinline__ float round_weight(float w) { return w; }
	static constexpr int EXP_MAX = 126;  // fp32 dL/dy may be tiny: scales up to 2^126 keep its bits
	// positions and dL/dy of the points in flight stay live across their loads, U (D + F) registers with F
	// up to 8 fp32 features; 4 is what the fp32 modules were merged with (8 was not measured here)
	static constexpr uint32_t POINTS_IN_FLIGHT = 4;
	// the D == 2 fast paths round weights to fp16 and read packed fp16 dL/dy; no fp32 form was written
	static constexpr bool FAST_2D = false;
	// the options instantiation (max_level, stochastic interpolation) takes the generic index for every
	// item: one accumulation body instead of four (which ran it out of scalar registers)
	static constexpr bool OPTS_ALL_KINDS = false;
	// with one chunk the slab is the caller's gradient buffer, of which only 4-byte alignment is known
	static constexpr bool SLAB_PAIR_ALIGNED = false;
	const float* dLdy;  // AoS rows [B][dy_stride], level l at columns [l F, l F + F)
	uint32_t dy_stride;
	bool vec;  // every row's level slice is FVec-aligned
	template <uint32_t F>
	__device__ __forceinline__ void load(uint32_t level, uint32_t i, float* dy) const {
		const FVec<F> v = load_fvec<F>(dLdy + (size_t)i * dy_stride + level * F, vec);
#pragma unroll
		for (uint32_t f = 0; f < F; ++f) dy[f] = v.v[f];
	}
};

// k_grid_bwd_lds's phases with the fp32 trait: no network tail, no by-value tables, no streaming or
// register-resident pre-pass (PrecF32::FAST_2D), plain slab stores (write-through, wt_store.h, is the
// training step's policy; this kernel never had it).
template <uint32_t D, uint32_t F, HashType H, bool OPTS>
__global__ __launch_bounds__(GRID_BWD_THREADS) void k_grid_bwd_lds_f32(
	uint32_t B, const float* __restrict__ pos, uint32_t pstride, const float* __restrict__ dLdy, uint32_t dy_stride, uint32_t vec,
	const GridSlice* __restrict__ items, float* __restrict__ partial, uint32_t partial_stride, const LevelInfo* __restrict__ levels,
	uint32_t hash_grid, uint32_t interp_u, uint32_t pts_per_chunk, uint32_t n_chunks, const GridOpts o) {
	extern __shared__ __attribute__((aligned(16))) int acc[];
	__shared__ float red[GRID_BWD_THREADS / 64];
	// 2. item and level load (chunk-minor, as k_grid_bwd_lds). Items hold all F features.
	const uint32_t item = blockIdx.x / n_chunks, chunk = blockIdx.x % n_chunks;
	const GridSlice it = items[item];
	const LevelInfo li = levels[it.level];
	const uint32_t len = it.end - it.begin;
	constexpr uint32_t nf = F, f0 = 0;
	constexpr int MODE = F == 2 ? 0 : 2;
	const Interp interp = (Interp)interp_u;
	const uint32_t i0 = chunk * pts_per_chunk;
	const uint32_t i1 = min(B, i0 + pts_per_chunk);
	const PrecF32 src{dLdy, dy_stride, vec != 0};
	// 3. layout
	const AccLayout lay = make_acc_layout(acc, len, nf);
	zero_accumulators(acc, lay);
	// 5. the exact pre-pass: sum over the chunk's points of max_f |dL/dy| -> the fixed-point scale (no entry
	// can receive more: a point's corner weights sum to 1). A non-finite dL/dy makes the item's gradient NaN.
	const float m = block_sum_waves(dy_bound_sum<PrecF32, F>(src, it.level, f0, nf, i0, i1), red);
	const bool finite = __builtin_isfinite(m);
	const int e = grid_bwd_scale_exp(m, (float)(i1 > i0 ? i1 - i0 : 1u), D, PrecF32::EXP_MAX);
	const float scale = ldexpf(1.0f, e);
	// 6. accumulate
	with_index_kind<PrecF32::OPTS_ALL_KINDS || !OPTS>(item_index_kind<D>(li, it, hash_grid != 0), [&](auto k) __attribute__((always_inline)) {
		grid_bwd_points<PrecF32, D, F, H, decltype(k)::value, MODE, OPTS>(src, B, pos, pstride, it.level, li, hash_grid != 0, interp, it.begin, len, f0,
		                                                                  nf, i0, i1, scale, lay.acc_w, o);
	});
	__syncthreads();
	// 7. merge
	merge_replicas(acc, lay, len, MODE == 0);
	// 8. write the chunk slab, parameter order: this item's entries [begin, end) x F are one contiguous range
	const float inv = finite ? ldexpf(1.0f, -e) : __builtin_nanf("");
	float* dst = partial + (size_t)chunk * partial_stride + ((size_t)li.offset + it.begin) * F;
	write_slab<SlabStorePlain<PrecF32::SLAB_PAIR_ALIGNED>, MODE == 0>(acc, dst, len, nf, inv);
}

template <uint32_t D, uint32_t F, HashType H>
static void grid_bwd_f32_t(hipStream_t st, const GridCall& gc, uint32_t B, const float* pos, uint32_t ps, const float* dy, uint32_t dys,
                           const GridSlice* sl, uint32_t n_slices, uint32_t n_chunks, float* part, uint32_t pstr) {
	static uint64_t done0 = 0, done1 = 0;
	set_dyn_lds((const void*)k_grid_bwd_lds_f32<D, F, H, false>, (int)GRID_BWD_LDS_BYTES, done0);
	set_dyn_lds((const void*)k_grid_bwd_lds_f32<D, F, H, true>, (int)GRID_BWD_LDS_BYTES, done1);
	constexpr uint32_t tb = F * 4u < 16u ? F * 4u : 16u;
	const uint32_t vec = ((uintptr_t)dy % tb == 0 && (dys * 4u) % tb == 0) ? 1u : 0u;  // every row's level slice is FVec-aligned
	const auto kernel = gc.opts.active ? k_grid_bwd_lds_f32<D, F, H, true> : k_grid_bwd_lds_f32<D, F, H, false>;
	hipLaunchKernelGGL(kernel, dim3(n_slices * n_chunks), dim3(GRID_BWD_THREADS), GRID_BWD_LDS_BYTES, st, B, pos, ps, dy, dys, vec, sl, part,
	                   pstr, gc.levels, gc.hash_grid ? 1u : 0u, (uint32_t)gc.interp, div_round_up(B, n_chunks), n_chunks, gc.opts);
}

void launch_grid_bwd_f32(hipStream_t st, const GridCall& gc, uint32_t B, const float* pos, uint32_t pos_stride, const float* dLdy32,
                         uint32_t dy_stride, const GridSlice* slices, uint32_t n_slices, uint32_t n_chunks, float* partial,
                         uint32_t partial_stride) {
	if (n_slices == 0 || B == 0) return;  // callers zero the gradient of empty batches
	with_grid_shape(gc.D, gc.F, gc.hash, [&](auto d, auto f, auto h) {
		grid_bwd_f32_t<decltype(d)::value, decltype(f)::value, decltype(h)::value>(st, gc, B, pos, pos_stride, dLdy32, dy_stride, slices,
		                                                                           n_slices, n_chunks, partial, partial_stride);
	});
	TCNN_HIP_CHECK(hipGetLastError());
}

}  // namespace tcnn_amd
