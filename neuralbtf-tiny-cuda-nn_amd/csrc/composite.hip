// composite.hip -- the parameter-free parts of a composite encoding for gfx950 (reference
// encodings/composite.h with Concatenation, spherical_harmonics.h, triangle_wave.h, oneblob.h,
// identity.h): SphericalHarmonics, TriangleWave, OneBlob, Identity and every padding column of the
// encoded AoS row [B][width] in ONE forward launch, and their dL/dinput in one backward launch. Rows and
// dL/dy are fp16, or fp32 for an fp32 encoding module (the kernels' element type T: the fp32 value each
// part computes is stored as it is instead of being rounded to fp16).
// Nested grids write their own value columns (launch_grid_fwd on the column slice). A standalone
// SphericalHarmonics or TriangleWave encoding is a composite with one part.
#include "encodings_device.h"
#include "kernels.h"
#include "sh_device.h"

namespace tcnn_amd {

// LDS row stride in elements of T (fp16, or fp32 for an fp32 module) for rows of `width` columns: the row
// rounded up to whole 16-byte chunks plus one dword, i.e. 4n + 1 dwords with n = chunks per row
// (fp16: round_up(width, 8) + 2 elements, n = width / 8; fp32: round_up(width, 4) + 1, n = width / 4).
// Bank arithmetic (64 banks of 4 B; writes and ds_read_b32 bank = dword % 32, lanes conflict within a
// 32-lane half):
//   * column writes: lane s stores column c of its own row, dword s (4n + 1) + c / 2 (fp16) or
//     s (4n + 1) + c (fp32) -- an odd dword stride, so the 32 lanes of a half hit 32 different banks
//     (conflict-free; two fp16 of one dword belong to the same lane);
//   * row reads: lane t reads dword j (0..3) of chunk k of row p, dword p (4n + 1) + 4k + j with
//     consecutive lanes on consecutive chunks. A half covers 32 / n rows x n chunks: banks
//     (p + 4k + j) % 32. n = 8 (fp16 width 64, fp32 width 32): 4 rows x {0, 4, .., 28} + p, all
//     different (conflict-free); n = 4 and n = 16 (fp16 width 32 / 128, fp32 width 16 / 64): 2-way;
//     fp32 rows of 128 columns and more (n >= 32: one row per half, 4k % 32 takes 8 values): 4-way --
//     an fp32 row is an fp16 row of twice the width to the LDS.
template <typename T>
__host__ __device__ inline uint32_t composite_lds_stride(uint32_t width) {
	constexpr uint32_t CH = 16 / sizeof(T);  // elements per 16-byte chunk
	return (width + CH - 1) / CH * CH + 4 / sizeof(T);
}

template <typename Out>
__device__ __forceinline__ void sh_forward_deg(uint32_t degree, float x, float y, float z, Out&& out) {
	switch (degree) {  // wave-uniform
		case 1: sh_forward<1>(x, y, z, out); break;
		case 2: sh_forward<2>(x, y, z, out); break;
		case 3: sh_forward<3>(x, y, z, out); break;
		case 4: sh_forward<4>(x, y, z, out); break;
		case 5: sh_forward<5>(x, y, z, out); break;
		case 6: sh_forward<6>(x, y, z, out); break;
		case 7: sh_forward<7>(x, y, z, out); break;
		default: sh_forward<8>(x, y, z, out); break;
	}
}

template <typename Grad>
__device__ __forceinline__ void sh_backward_deg(uint32_t degree, float x, float y, float z, Grad&& g, float& gx, float& gy, float& gz) {
	switch (degree) {
		case 1: sh_backward<1>(x, y, z, g, gx, gy, gz); break;
		case 2: sh_backward<2>(x, y, z, g, gx, gy, gz); break;
		case 3: sh_backward<3>(x, y, z, g, gx, gy, gz); break;
		case 4: sh_backward<4>(x, y, z, g, gx, gy, gz); break;
		case 5: sh_backward<5>(x, y, z, g, gx, gy, gz); break;
		case 6: sh_backward<6>(x, y, z, g, gx, gy, gz); break;
		case 7: sh_backward<7>(x, y, z, g, gx, gy, gz); break;
		default: sh_backward<8>(x, y, z, g, gx, gy, gz); break;
	}
}

// Forward. A workgroup of blockDim.x / 64 waves owns a tile of blockDim.x samples; each wave encodes
// its own 64 samples, lane = sample, one part after the other, so the kind switch and every loop bound
// are wave-uniform and a sample's shared terms (SH monomials, a OneBlob dimension's CDFs) are computed
// once. Results are staged in LDS as [sample][column] (stride: composite_lds_stride), then the whole
// workgroup writes the rows out with 16-byte stores, consecutive lanes on consecutive 16 B of a row;
// a chunk that shares its 16 bytes with a nested grid's values, or a row that is not 16-byte aligned
// (width % 8 != 0, a module output at an odd address), goes out in 2-byte stores of the owned columns.
// Every column that is not a grid value is written exactly once (no memset before).
template <typename T>
__global__ __launch_bounds__(256) void k_composite_fwd(uint32_t B, const float* __restrict__ x, T* __restrict__ out, const CompTable t,
                                                        uint32_t vec_ok) {
	extern __shared__ uint32_t tile32[];
	T* tile = (T*)tile32;
	constexpr uint32_t CH = 16 / sizeof(T);  // elements per 16-byte chunk
	const uint32_t stride = composite_lds_stride<T>(t.width);
	const uint32_t tile0 = blockIdx.x * blockDim.x;
	const uint32_t i = tile0 + threadIdx.x;
	const float* xrow = x + (size_t)(i < B ? i : B - 1) * t.n_in;  // lanes past the batch encode the last sample (not stored)
	T* row = tile + threadIdx.x * stride;
	for (uint32_t pi = 0; pi < t.n_parts; ++pi) {
		const CompPart& p = t.parts[pi];
		const float* xp = xrow + p.in_col;
		const uint32_t n_pad = p.width - p.n_values;
		switch (p.kind) {
			case COMP_SH: {
				// [0, 1]^3 -> [-1, 1]^3, not normalised (spherical_harmonics.h:65-71); padding first
				const float dx = __builtin_fmaf(xp[0], 2.0f, -1.0f), dy = __builtin_fmaf(xp[1], 2.0f, -1.0f),
				            dz = __builtin_fmaf(xp[2], 2.0f, -1.0f);
				T* o = row + p.out_col + n_pad;
				sh_forward_deg(p.p0, dx, dy, dz, [&](uint32_t j, float v) { o[j] = enc_value<T>(v); });
				for (uint32_t j = 0; j < n_pad; ++j) row[p.out_col + j] = (T)1.0f;
				break;
			}
			case COMP_TRIANGLE: {
				T* o = row + p.out_col;
				for (uint32_t d = 0; d < p.n_in; ++d) {
					const float xv = xp[d];
					for (uint32_t k = 0; k < p.p0; ++k) o[d * p.p0 + k] = enc_value<T>(triangle_wave_value(xv, k));
				}
				break;
			}
			case COMP_ONEBLOB: {
				for (uint32_t d = 0; d < p.n_in; ++d) {
					T* o = row + p.out_col + d * p.p0;
					oneblob_fwd_dim<T>(xp[d], p.p0, p.p1, [&](uint32_t b, T v) { o[b] = v; });
				}
				break;
			}
			case COMP_IDENTITY: {
				T* o = row + p.out_col;
				for (uint32_t d = 0; d < p.n_in; ++d) {
					if constexpr (sizeof(T) == 2) o[d] = identity_fwd_value(xp[d], p.f0, p.f1);
					else o[d] = identity_fwd_value_f32(xp[d], p.f0, p.f1);
				}
				break;
			}
			default: break;  // COMP_GRID: the grid's own launch writes its values
		}
		if (p.kind != COMP_SH) {  // padding after the values: 1, a grid's 0
			const T pv = p.kind == COMP_GRID ? (T)0.0f : (T)1.0f;
			for (uint32_t j = p.n_values; j < p.width; ++j) row[p.out_col + j] = pv;
		}
	}
	__syncthreads();
	const uint32_t chunks = (t.width + CH - 1) / CH;
	const uint32_t sdw = stride * sizeof(T) / 4;
	for (uint32_t idx = threadIdx.x; idx < blockDim.x * chunks; idx += blockDim.x) {
		const uint32_t r = idx / chunks, k = idx - r * chunks;
		const uint32_t ir = tile0 + r;
		if (ir >= B) continue;
		const uint32_t c0 = CH * k;
		const uint32_t gmask = (t.grid_cols[c0 / 32] >> (c0 % 32)) & ((1u << CH) - 1u);
		T* orow = out + (size_t)ir * t.width;
		if (vec_ok && gmask == 0) {  // (vec_ok: width % CH == 0, so the chunk is whole)
			const uint32_t* s = tile32 + r * sdw + 4 * k;
			uint4 v;
			v.x = s[0];
			v.y = s[1];
			v.z = s[2];
			v.w = s[3];
			*(uint4*)(orow + c0) = v;
		} else {
			const T* s = tile + r * stride + c0;
			for (uint32_t j = 0; j < CH; ++j)
				if (c0 + j < t.width && !((gmask >> j) & 1u)) orow[c0 + j] = s[j];
		}
	}
}

// dL/dinput of the parameter-free parts: blockIdx.y = slot (CompTable::slot_*), one thread per sample
// of that slot, so a workgroup runs one kind. Plain stores: input columns are read by at most one part.
template <typename T>
__global__ __launch_bounds__(256) void k_composite_bwd_input(uint32_t B, const float* __restrict__ x, const T* __restrict__ dy,
                                                              uint32_t dy_stride, float* __restrict__ dx, const CompTable t) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= B) return;
	const uint32_t slot = blockIdx.y;
	const uint32_t pi = t.slot_part[slot], col = t.slot_col[slot];
	float* dxrow = dx + (size_t)i * t.n_in;
	if (pi == COMP_SLOT_ZERO) {
		dxrow[col] = 0.0f;
		return;
	}
	const CompPart& p = t.parts[pi];
	const float* xp = x + (size_t)i * t.n_in + p.in_col;
	const T* g = dy + (size_t)i * dy_stride + p.out_col;
	const uint32_t d = col - p.in_col;
	switch (p.kind) {
		case COMP_SH: {
			const float vx = __builtin_fmaf(xp[0], 2.0f, -1.0f), vy = __builtin_fmaf(xp[1], 2.0f, -1.0f),
			            vz = __builtin_fmaf(xp[2], 2.0f, -1.0f);
			const T* gv = g + (p.width - p.n_values);  // padding first
			float gx, gy, gz;
			sh_backward_deg(p.p0, vx, vy, vz, [&](uint32_t j) { return (float)gv[j]; }, gx, gy, gz);
			// times 2: the map from [0, 1]^3 to [-1, 1]^3 (spherical_harmonics.h:96-99)
			dxrow[p.in_col + 0] = 2.0f * gx;
			dxrow[p.in_col + 1] = 2.0f * gy;
			dxrow[p.in_col + 2] = 2.0f * gz;
			break;
		}
		case COMP_TRIANGLE: {
			const float xv = xp[d];
			float r = 0.0f;
			for (uint32_t k = 0; k < p.p0; ++k) r += (float)g[d * p.p0 + k] * triangle_wave_deriv(xv, k);
			dxrow[col] = r;
			break;
		}
		case COMP_ONEBLOB: dxrow[col] = oneblob_bwd_dim(xp[d], p.p0, p.p1, g + d * p.p0); break;
		case COMP_IDENTITY: dxrow[col] = identity_bwd_value(g[d], p.f0); break;
		default: break;
	}
}

static void check_table(const CompTable& t) {
	TCNN_CHECK(t.n_parts <= COMP_MAX_PARTS && t.width <= COMP_MAX_WIDTH && t.n_in <= COMP_MAX_INPUTS && t.n_slots <= COMP_MAX_INPUTS,
	           "composite encoding: part table out of range");
	for (uint32_t i = 0; i < t.n_parts; ++i) {
		const CompPart& p = t.parts[i];
		TCNN_CHECK(p.in_col + p.n_in <= t.n_in && p.out_col + p.width <= t.width && p.n_values <= p.width,
		           "composite encoding: part outside its row");
		TCNN_CHECK(p.kind != COMP_SH || (p.n_in == 3 && p.p0 >= 1 && p.p0 <= 8 && p.n_values == p.p0 * p.p0),
		           "composite encoding: bad SphericalHarmonics part");
		TCNN_CHECK(p.kind != COMP_TRIANGLE || p.n_values == p.n_in * p.p0, "composite encoding: bad TriangleWave part");
		TCNN_CHECK(p.kind != COMP_ONEBLOB || (p.n_values == p.n_in * p.p0 && p.p0 == (1u << p.p1)), "composite encoding: bad OneBlob part");
		TCNN_CHECK(p.kind != COMP_IDENTITY || p.n_values == p.n_in, "composite encoding: bad Identity part");
	}
	for (uint32_t s = 0; s < t.n_slots; ++s) {
		TCNN_CHECK(t.slot_col[s] < t.n_in, "composite encoding: slot outside the input");
		if (t.slot_part[s] == COMP_SLOT_ZERO) continue;
		TCNN_CHECK(t.slot_part[s] < t.n_parts, "composite encoding: slot of no part");
		const CompPart& p = t.parts[t.slot_part[s]];
		TCNN_CHECK(t.slot_col[s] >= p.in_col && t.slot_col[s] < p.in_col + p.n_in, "composite encoding: slot outside its part");
	}
}

// T: the module's precision (_Float16 / float), both instantiated below
template <typename T>
void launch_composite_fwd(hipStream_t st, uint32_t B, const float* x, T* out, const CompTable& t) {
	if (!B || !t.fwd_work) return;
	check_table(t);
	// as many waves per workgroup (4, 2, 1) as keep the staging tile within 32 KiB (one wave of the widest
	// rows is past it: 64 rows of 256 columns)
	constexpr uint32_t CH = 16 / sizeof(T);
	const uint32_t row_bytes = composite_lds_stride<T>(t.width) * sizeof(T);
	uint32_t threads = 256;
	while (threads > 64 && threads * row_bytes > 32768) threads /= 2;
	const uint32_t lds = threads * row_bytes;
	if (lds > 48 * 1024) {
		static uint64_t done = 0;
		set_dyn_lds((const void*)k_composite_fwd<T>, 64 * (COMP_MAX_WIDTH + CH) * (int)sizeof(T), done);
	}
	const uint32_t vec_ok = (t.width % CH == 0 && ((uintptr_t)out & 15) == 0) ? 1u : 0u;
	hipLaunchKernelGGL(k_composite_fwd<T>, dim3(div_round_up(B, threads)), dim3(threads), lds, st, B, x, out, t, vec_ok);
	TCNN_HIP_CHECK(hipGetLastError());
}
template void launch_composite_fwd<_Float16>(hipStream_t, uint32_t, const float*, _Float16*, const CompTable&);
template void launch_composite_fwd<float>(hipStream_t, uint32_t, const float*, float*, const CompTable&);

template <typename T>
void launch_composite_bwd_input(hipStream_t st, uint32_t B, const float* x, const T* dy, uint32_t dy_stride, float* dx, const CompTable& t) {
	if (!B || !t.n_slots) return;
	check_table(t);
	hipLaunchKernelGGL(k_composite_bwd_input<T>, dim3(div_round_up(B, 256), t.n_slots), dim3(256), 0, st, B, x, dy, dy_stride, dx, t);
	TCNN_HIP_CHECK(hipGetLastError());
}
template void launch_composite_bwd_input<_Float16>(hipStream_t, uint32_t, const float*, const _Float16*, uint32_t, float*, const CompTable&);
template void launch_composite_bwd_input<float>(hipStream_t, uint32_t, const float*, const float*, uint32_t, float*, const CompTable&);

}  // namespace tcnn_amd
