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

template <uint32_t F>
__device__ __forceinline__ void load_dy_f32(const float* __restrict__ dLdy, uint32_t dy_stride, uint32_t level, uint32_t i, bool vec,
                                            float* dy) {
	const FVec<F> v = load_fvec<F>(dLdy + (size_t)i * dy_stride + level * F, vec);
#pragma unroll
	for (uint32_t f = 0; f < F; ++f) dy[f] = v.v[f];
}

// One point's corner updates of one item (accum_point of grid_bwd_lds.h with fp32 weights). dy: the
// point's dL/dy times the item's scale. PACK (F == 2): both features as one int64 add per corner.
template <uint32_t D, uint32_t F, HashType H, int KIND, bool PACK, bool OPTS>
__device__ __forceinline__ void accum_point_f32(const float (&x)[D], const float (&dy)[F], uint32_t i, uint32_t level, uint32_t B,
                                                const LevelInfo& li, bool hash_grid, Interp interp, uint32_t begin, uint32_t len, int* acc,
                                                const GridOpts& o) {
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
		if (single) w = 1.0f;
		const uint32_t rel = level_index<D, H, KIND>(hash_grid, li.size, li.res, local) - begin;
		if constexpr (KIND == IDX_GENERIC || KIND == IDX_HASH_RANGE) {  // entry ranges do not cover the level
			if (rel >= len) continue;
		}
		if constexpr (PACK) {
			const int a = __float2int_rn(w * dy[0]);
			const int b = __float2int_rn(w * dy[1]);
			const unsigned long long pk = (unsigned long long)(((long long)b << 32) + (long long)a);
			__hip_atomic_fetch_add((unsigned long long*)acc + rel, pk, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
		} else {
#pragma unroll
			for (uint32_t f = 0; f < F; ++f) lds_add_i32(&acc[rel * F + f], w * dy[f]);
		}
	}
}

template <uint32_t D, uint32_t F, HashType H, int KIND, bool OPTS>
__device__ __forceinline__ void grid_bwd_points_f32(uint32_t B, const float* __restrict__ pos, uint32_t pstride,
                                                    const float* __restrict__ dLdy, uint32_t dy_stride, bool vec, uint32_t level,
                                                    const LevelInfo& li, bool hash_grid, Interp interp, uint32_t begin, uint32_t len,
                                                    uint32_t i0, uint32_t i1, float scale, int* acc, const GridOpts& o) {
	constexpr uint32_t U = 4;  // points in flight per thread
	for (uint32_t base = i0 + threadIdx.x; base < i1; base += U * blockDim.x) {
		float xs[U][D], dy[U][F];
#pragma unroll
		for (uint32_t u = 0; u < U; ++u) {
			const uint32_t i = base + u * blockDim.x;
			if (i < i1) {
#pragma unroll
				for (uint32_t d = 0; d < D; ++d) xs[u][d] = pos[(size_t)i * pstride + d];
				load_dy_f32<F>(dLdy, dy_stride, level, i, vec, dy[u]);
			} else {
#pragma unroll
				for (uint32_t d = 0; d < D; ++d) xs[u][d] = 0.0f;
#pragma unroll
				for (uint32_t f = 0; f < F; ++f) dy[u][f] = 0.0f;
			}
			const bool masked = OPTS && i < i1 && (float)level > grid_max_level(o, i, F) + 1e-3f;  // grid.h:242-244
#pragma unroll
			for (uint32_t f = 0; f < F; ++f) dy[u][f] = masked ? 0.0f : dy[u][f] * scale;
		}
#pragma unroll
		for (uint32_t u = 0; u < U; ++u) {
			if (base + u * blockDim.x >= i1) break;
			accum_point_f32<D, F, H, KIND, F == 2, OPTS>(xs[u], dy[u], base + u * blockDim.x, level, B, li, hash_grid, interp, begin, len,
			                                             acc, o);
		}
	}
}

template <uint32_t D, uint32_t F, HashType H, bool OPTS>
__global__ __launch_bounds__(GRID_BWD_THREADS) void k_grid_bwd_lds_f32(
	uint32_t B, const float* __restrict__ pos, uint32_t pstride, const float* __restrict__ dLdy, uint32_t dy_stride, uint32_t vec,
	const GridSlice* __restrict__ items, float* __restrict__ partial, uint32_t partial_stride, const LevelInfo* __restrict__ levels,
	uint32_t hash_grid, uint32_t interp_u, uint32_t pts_per_chunk, uint32_t n_chunks, const GridOpts o) {
	extern __shared__ __attribute__((aligned(16))) int acc[];
	__shared__ float red[GRID_BWD_THREADS / 64];
	const uint32_t item = blockIdx.x / n_chunks, chunk = blockIdx.x % n_chunks;  // chunk-minor, as k_grid_bwd_lds
	const GridSlice it = items[item];
	const LevelInfo li = levels[it.level];
	const uint32_t len = it.end - it.begin;
	const Interp interp = (Interp)interp_u;
	const uint32_t i0 = chunk * pts_per_chunk;
	const uint32_t i1 = min(B, i0 + pts_per_chunk);
	const bool dyvec = vec != 0;

	// replicas of a small item's accumulators (wave w adds into replica w % R), as k_grid_bwd_lds
	const uint32_t slots = len * F;
	const uint32_t R = max(1u, min(16u, GRID_BWD_SLOTS / max(slots, 1u)));
	const uint32_t nz = R * slots;
	for (uint32_t j = 4 * threadIdx.x; j + 4 <= nz; j += 4 * blockDim.x) *(int4*)(acc + j) = int4{0, 0, 0, 0};
	for (uint32_t j = nz / 4 * 4 + threadIdx.x; j < nz; j += blockDim.x) acc[j] = 0;
	int* acc_w = acc + ((threadIdx.x >> 6) % R) * slots;

	// pre-pass: sum over the chunk's points of max_f |dL/dy| -> the fixed-point scale (no entry can
	// receive more: a point's corner weights sum to 1). A non-finite dL/dy makes the item's gradient NaN.
	float m = 0.0f;
	for (uint32_t ib = i0 + threadIdx.x; ib < i1; ib += 4 * blockDim.x) {
		float dy[4][F];
#pragma unroll
		for (uint32_t u = 0; u < 4; ++u) {
			const uint32_t i = ib + u * blockDim.x;
			if (i < i1) load_dy_f32<F>(dLdy, dy_stride, it.level, i, dyvec, dy[u]);
			else {
#pragma unroll
				for (uint32_t f = 0; f < F; ++f) dy[u][f] = 0.0f;
			}
		}
#pragma unroll
		for (uint32_t u = 0; u < 4; ++u) {
			float s = 0.0f;
#pragma unroll
			for (uint32_t f = 0; f < F; ++f) s = __builtin_isfinite(dy[u][f]) ? fmaxf(s, fabsf(dy[u][f])) : __builtin_inff();
			m += s;
		}
	}
#pragma unroll
	for (int sh = 32; sh > 0; sh >>= 1) m += __shfl_xor(m, sh);
	if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
	__syncthreads();
	m = red[0];
#pragma unroll
	for (uint32_t w = 1; w < GRID_BWD_THREADS / 64; ++w) m += red[w];
	const float P = (float)(i1 > i0 ? i1 - i0 : 1u);
	const bool finite = __builtin_isfinite(m);
	int e = 0;
	if (m > 0.0f && finite) {
		const float lim = (2147483647.0f - (float)(1u << D) * P) / (m * 1.01f);
		e = ilogbf(lim);
		e = max(-126, min(e, 126));  // fp32 dL/dy may be tiny: scales up to 2^126 keep its bits
	}
	const float scale = ldexpf(1.0f, e);

	uint64_t full = 1;
	for (uint32_t d = 0; d < D; ++d) full = full * li.res > 0xffffffffull ? 0x100000000ull : full * li.res;
	const bool whole = it.begin == 0 && len == li.size;
	const bool pow2 = (li.size & (li.size - 1)) == 0;
	// the options instantiation (max_level, stochastic interpolation) takes the generic index for every
	// item: one accumulation body instead of four (which ran it out of scalar registers)
	if (OPTS)
		grid_bwd_points_f32<D, F, H, IDX_GENERIC, OPTS>(B, pos, pstride, dLdy, dy_stride, dyvec, it.level, li, hash_grid != 0, interp, it.begin, len, i0, i1, scale, acc_w, o);
	else if (whole && full <= li.size)
		grid_bwd_points_f32<D, F, H, IDX_DENSE, OPTS>(B, pos, pstride, dLdy, dy_stride, dyvec, it.level, li, hash_grid != 0, interp, it.begin, len, i0, i1, scale, acc_w, o);
	else if (whole && hash_grid && pow2)
		grid_bwd_points_f32<D, F, H, IDX_HASH_POW2, OPTS>(B, pos, pstride, dLdy, dy_stride, dyvec, it.level, li, hash_grid != 0, interp, it.begin, len, i0, i1, scale, acc_w, o);
	else if (!whole && hash_grid && pow2 && full > li.size)
		grid_bwd_points_f32<D, F, H, IDX_HASH_RANGE, OPTS>(B, pos, pstride, dLdy, dy_stride, dyvec, it.level, li, hash_grid != 0, interp, it.begin, len, i0, i1, scale, acc_w, o);
	else
		grid_bwd_points_f32<D, F, H, IDX_GENERIC, OPTS>(B, pos, pstride, dLdy, dy_stride, dyvec, it.level, li, hash_grid != 0, interp, it.begin, len, i0, i1, scale, acc_w, o);
	__syncthreads();
	if (R > 1) {  // merge the replicas into replica 0 (exact: integer sums)
		if constexpr (F == 2) {
			long long* a64 = (long long*)acc;
			for (uint32_t j = threadIdx.x; j < len; j += blockDim.x) {
				long long t = a64[j];
				for (uint32_t r = 1; r < R; ++r) t += a64[(size_t)r * len + j];
				a64[j] = t;
			}
		} else {
			for (uint32_t j = threadIdx.x; j < slots; j += blockDim.x) {
				int t = acc[j];
				for (uint32_t r = 1; r < R; ++r) t += acc[(size_t)r * slots + j];
				acc[j] = t;
			}
		}
		__syncthreads();
	}
	// the chunk slab, parameter order: this item's entries [begin, end) x F are one contiguous range
	const float inv = finite ? ldexpf(1.0f, -e) : __builtin_nanf("");
	float* dst = partial + (size_t)chunk * partial_stride + ((size_t)li.offset + it.begin) * F;
	const bool al = (((uintptr_t)dst) & 15) == 0;
	if constexpr (F == 2) {  // decode the packed int32 pairs, two entries per thread (16-byte stores)
		const long long* a64 = (const long long*)acc;
		auto dec = [&](long long t) {
			const int lo = (int)(uint32_t)(unsigned long long)t;
			const int hi = (int)((t - (long long)lo) >> 32);
			return make_float2((float)lo * inv, (float)hi * inv);
		};
		for (uint32_t j = 2 * threadIdx.x; j < len; j += 2 * blockDim.x) {
			const float2 a = dec(a64[j]);
			if (al && j + 1 < len) {
				const float2 b = dec(a64[j + 1]);
				*(f4*)(dst + 2 * j) = f4{a.x, a.y, b.x, b.y};
			} else {
				dst[2 * j] = a.x;
				dst[2 * j + 1] = a.y;
				if (j + 1 < len) {
					const float2 b = dec(a64[j + 1]);
					dst[2 * j + 2] = b.x;
					dst[2 * j + 3] = b.y;
				}
			}
		}
	} else {
		for (uint32_t j = 4 * threadIdx.x; j < slots; j += 4 * blockDim.x) {
			if (al && j + 4 <= slots) {
				const int4 v = *(const int4*)(acc + j);
				*(f4*)(dst + j) = f4{(float)v.x * inv, (float)v.y * inv, (float)v.z * inv, (float)v.w * inv};
			} else {
				for (uint32_t k = j; k < slots && k < j + 4; ++k) dst[k] = (float)acc[k] * inv;
			}
		}
	}
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
