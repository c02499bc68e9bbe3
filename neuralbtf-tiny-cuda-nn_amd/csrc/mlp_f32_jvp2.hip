// mlp_f32_jvp2.hip -- the forward Laplacian of an fp32 FullyFusedMLP network module behind a lone grid (or a lone
// Identity): the value f(x), K directional derivatives J(x) v_k and q = sum_k v_k^T H(x) v_k per output, in one
// forward-mode launch that keeps nothing (NetworkF32Host::jvp_second, tcnn_module_inference_jvp_second). Null
// directions mean the D unit vectors: the Jacobian and the Laplacian.
//
// The scheme. A second directional derivative obeys, per layer z = W h, s_k = W t_k, r_k = W u_k:
//   h' = a(z), t_k' = a'(z) s_k, u_k' = a'(z) r_k + a''(z) s_k^2.
// Only the sum over k of u_k is wanted and the recurrence is linear in it, so U = sum_k u_k is summed at the front and
// carried as ONE quantity: U' = a' (W U) + a'' sum_k s_k^2. A pass carries 2 + T2 quantities -- the value, T2
// tangents, U -- where one Taylor coefficient per direction would carry 1 + 2 T2. With T2 = 3 these are the five
// rows of a 16-row tile that the Jacobian kernel's register chain (mlp_f32_chain.h) runs with four.
//
// Work split: mlp_f32_jvp.hip's. 64 batch rows per 256-thread workgroup, one 16-row tile per wave, lane (r, q) supplies
// operand columns 16 s + 4 q + j; no LDS, no shuffle, no barrier. U is one more row through the same MFMAs
// (jac_from_regs), so the value and the tangents see jac_chain's operations in jac_chain's order and carry
// tcnn_module_inference's and tcnn_module_inference_jvp's bits. The gate is jac_activate2: the tangents'
// pre-activations are squared and summed before they are scaled.
//
// Fronts. Behind an Identity U_0 = 0, the first layer's r is not computed and U_1 = a'' sum_k s_k^2. Behind a grid
// U_0[col] = sum_{d, d'} M[d][d'] d^2 e_col / dx_d dx_d' with M = sum_{k in pass} v_k v_k^T formed once per row and pass
// in registers, the second derivatives from the corners the value gathered (jvp2_encode_step, level_second_f32).
//
// Passes. K > T2 runs ceil(K / T2) passes inside the launch. U is linear in the sum over directions, so the passes' q
// add: pass 0 stores q, a later pass loads, adds and stores, the same lane for the same element in a fixed order, which
// keeps the result bit-reproducible. T2 is 3 at W 16, 32 and 64, where the resource report shows no scratch in any
// instantiation (DESIGN.md has the table). W 128 is refused: with T2 = 1 its three rows and their accumulators take
// all 512 registers and 96 to 352 bytes of scratch per lane besides.
//
// Instantiations: W, D and F only, as in mlp_f32_jvp.hip: 18 grid kernels and 3 for the Identity front.
#include "mlp_f32_jvp_device.h"

namespace tcnn_amd {

namespace {

constexpr int JVP2_TANGENTS = 3;  // T2, for every width served

// jac_chain (mlp_f32_jvp.hip) with U as row NQ - 1: from the first layer's pre-activations to memory. Tangent i is
// number d0 + i - 1 of the call's D; the pass with d0 == 0 stores y and q, a later pass adds its U to q.
// Q is [B][NOUT], or [NOUT][B] when ys.
template <int WT, int NQ>
__device__ __forceinline__ void jvp2_chain(f4 (&h)[NQ][WT], const float* __restrict__ wl, uint32_t NH, uint32_t r, uint32_t q, uint32_t row,
                                           uint32_t B, uint32_t OUTP, uint32_t NOUT, uint32_t D, uint32_t d0, bool ys, float* __restrict__ Y,
                                           float* __restrict__ J, float* __restrict__ Q, int act, int oact) {
	constexpr uint32_t W = 16 * WT;
	const uint32_t nt = (NOUT + 15) / 16;
	jac_activate2<WT, NQ>(h, act);
	for (uint32_t l = 1; l < NH; ++l, wl += (size_t)W * W) {
		f4 n[NQ][WT];
#pragma unroll
		for (int i = 0; i < NQ; ++i)
#pragma unroll
			for (int c = 0; c < WT; ++c) n[i][c] = f4{0.0f, 0.0f, 0.0f, 0.0f};
		jac_from_regs<WT, NQ, WT>(wl + (size_t)r * W + 4 * q, WT, h, n);
#pragma unroll
		for (int i = 0; i < NQ; ++i)
#pragma unroll
			for (int c = 0; c < WT; ++c) h[i][c] = n[i][c];
		jac_activate2<WT, NQ>(h, act);
	}
	// output layer: one column tile at a time, as in jac_chain
	for (uint32_t c0 = 0; c0 < nt; ++c0) {
		f4 o[NQ][1];
#pragma unroll
		for (int i = 0; i < NQ; ++i) o[i][0] = f4{0.0f, 0.0f, 0.0f, 0.0f};
		jac_from_regs<WT, NQ, 1>(wl + (size_t)(16 * c0 + r) * W + 4 * q, 1, h, o);
		const uint32_t n0 = 16 * c0 + 4 * q;
		jac_activate2<1, NQ>(o, oact);
		if (d0 == 0) {
			if (ys) {
#pragma unroll
				for (int e = 0; e < 4; ++e)
					if (n0 + e < NOUT) Y[(size_t)(n0 + e) * B + row] = o[0][0][e];
			} else {
				*(f4*)(Y + (size_t)row * OUTP + n0) = o[0][0];
			}
		}
		const size_t so = ys ? (size_t)D * B : D, sd = ys ? B : 1;
		float* je = J + (ys ? ((size_t)n0 * D + d0) * B + row : ((size_t)row * NOUT + n0) * D + d0);
		float* qe = Q + (ys ? (size_t)n0 * B + row : (size_t)row * NOUT + n0);
		const size_t sq = ys ? B : 1;
#pragma unroll
		for (int e = 0; e < 4; ++e, je += so, qe += sq) {
			if (n0 + e < NOUT) {
				float* ji = je;
#pragma unroll
				for (int i = 1; i < NQ - 1; ++i, ji += sd)
					if (d0 + (i - 1) < D) *ji = o[i][0][e];
				// this lane wrote the element in pass 0 and is the only one that touches it
				*qe = d0 ? *qe + o[NQ - 1][0][e] : o[NQ - 1][0][e];
			}
		}
	}
}

// Grid B / 64. W = 16 WT, D input dimensions and F features per level of the grid in front.
template <int WT, uint32_t D, uint32_t F>
__global__ __launch_bounds__(256) void k_f32_grid_mlp_jvp2(const Jvp2Args b) {
	const JvpArgs& a = b.j;
	constexpr uint32_t W = 16 * WT;
	constexpr int T2 = JVP2_TANGENTS, NQ = 2 + T2;  // 0 the value, 1 .. T2 tangents k0 .. k0 + T2 - 1, NQ - 1 is U
	const uint32_t lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;
	const uint32_t row = (blockIdx.x * 4 + (threadIdx.x >> 6)) * JAC_ROWS_PER_WAVE + r;
	if (row >= a.B) return;
	float x[D];
#pragma unroll
	for (uint32_t d = 0; d < D; ++d) x[d] = a.x_soa ? a.X[(size_t)d * a.B + row] : a.X[(size_t)row * D + d];
	uint32_t prime[D];
	hash_primes<D>((HashType)a.hash, prime);
	const uint32_t ks = a.IN / 16;
	for (uint32_t k0 = 0; k0 < a.K; k0 += T2) {
		float dir[T2][D];
#pragma unroll
		for (int i = 0; i < T2; ++i)
#pragma unroll
			for (uint32_t d = 0; d < D; ++d) {
				const uint32_t k = k0 + i;
				dir[i][d] = a.V && k < a.K ? (a.x_soa ? a.V[((size_t)k * D + d) * a.B + row] : a.V[((size_t)row * a.K + k) * D + d]) : 0.0f;
			}
		// M = sum over the pass's directions of v v^T, its upper triangle; the unit vectors of the pass give a 0 / 1 diagonal
		float M[D][D];
#pragma unroll
		for (uint32_t d = 0; d < D; ++d)
#pragma unroll
			for (uint32_t e = 0; e < D; ++e) {
				float m = d == e && d >= k0 && d < k0 + T2 ? 1.0f : 0.0f;
				if (a.V) {
					m = dir[0][d] * dir[0][e];
#pragma unroll
					for (int i = 1; i < T2; ++i) m = __builtin_fmaf(dir[i][d], dir[i][e], m);
				}
				M[d][e] = m;
			}
		// the pass's whole operand, before an accumulator is live
		f4 e[NQ][JVP_MAX_KSTEPS];
#pragma unroll
		for (uint32_t s = 0; s < JVP_MAX_KSTEPS; ++s) {
			if (s < ks) {
				f4 es[NQ];
				jvp2_encode_step<D, F, NQ>(a, s, q, k0, x, dir, M, prime, es);
#pragma unroll
				for (int i = 0; i < NQ; ++i) e[i][s] = es[i];
			}
		}
		// first layer: every quantity against each weight f4 loaded once
		f4 h[NQ][WT];
#pragma unroll
		for (int i = 0; i < NQ; ++i)
#pragma unroll
			for (int c = 0; c < WT; ++c) h[i][c] = f4{0.0f, 0.0f, 0.0f, 0.0f};
		const float* wp = a.P + (size_t)r * a.IN + 4 * q;
#pragma unroll
		for (uint32_t s = 0; s < JVP_MAX_KSTEPS; ++s) {
			if (s < ks) {
#pragma unroll
				for (int c = 0; c < WT; ++c) {
					const f4 w = *(const f4*)(wp + (size_t)c * 16 * a.IN + 16 * s);
#pragma unroll
					for (int j = 0; j < 4; ++j)
#pragma unroll
						for (int i = 0; i < NQ; ++i) h[i][c] = mfma4(w[j], e[i][s][j], h[i][c]);
				}
			}
		}
		jvp2_chain<WT, NQ>(h, a.P + (size_t)W * a.IN, a.NH, r, q, row, a.B, a.OUTP, a.NOUT, a.K, k0, a.y_soa != 0, a.Y, a.J, b.Q, a.act, a.oact);
	}
}

// The same call behind an Identity row (or a network alone): the encoding is linear, so U enters the first gate as zero
template <int WT>
__global__ __launch_bounds__(256) void k_f32_identity_mlp_jvp2(const Jvp2Args b) {
	const JvpArgs& a = b.j;
	constexpr uint32_t W = 16 * WT;
	constexpr int T2 = JVP2_TANGENTS, NQ = 2 + T2;
	const uint32_t lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;
	const uint32_t row = (blockIdx.x * 4 + (threadIdx.x >> 6)) * JAC_ROWS_PER_WAVE + r;
	if (row >= a.B) return;
	for (uint32_t k0 = 0; k0 < a.K; k0 += T2) {
		f4 t[NQ - 1][WT], h[NQ][WT];
		jac_identity_layer<WT, NQ - 1>(t, a.P, a.X, a.x_soa != 0, a.V, a.B, a.D, a.K, a.IN, a.scale, a.offset, r, q, row, k0);
#pragma unroll
		for (int c = 0; c < WT; ++c) {
#pragma unroll
			for (int i = 0; i < NQ - 1; ++i) h[i][c] = t[i][c];
			h[NQ - 1][c] = f4{0.0f, 0.0f, 0.0f, 0.0f};
		}
		jvp2_chain<WT, NQ>(h, a.P + (size_t)W * a.IN, a.NH, r, q, row, a.B, a.OUTP, a.NOUT, a.K, k0, a.y_soa != 0, a.Y, a.J, b.Q, a.act, a.oact);
	}
}

template <int WT>
void jvp2_width(hipStream_t st, const Jvp2Args& a, bool grid, uint32_t D, uint32_t F) {
	const dim3 blocks(a.j.B / JAC_ROWS_PER_BLOCK), block(256);
	if (!grid) {
		hipLaunchKernelGGL((k_f32_identity_mlp_jvp2<WT>), blocks, block, 0, st, a);
		return;
	}
	switch (D * 16 + F) {
		case 2 * 16 + 2: hipLaunchKernelGGL((k_f32_grid_mlp_jvp2<WT, 2, 2>), blocks, block, 0, st, a); break;
		case 2 * 16 + 4: hipLaunchKernelGGL((k_f32_grid_mlp_jvp2<WT, 2, 4>), blocks, block, 0, st, a); break;
		case 2 * 16 + 8: hipLaunchKernelGGL((k_f32_grid_mlp_jvp2<WT, 2, 8>), blocks, block, 0, st, a); break;
		case 3 * 16 + 2: hipLaunchKernelGGL((k_f32_grid_mlp_jvp2<WT, 3, 2>), blocks, block, 0, st, a); break;
		case 3 * 16 + 4: hipLaunchKernelGGL((k_f32_grid_mlp_jvp2<WT, 3, 4>), blocks, block, 0, st, a); break;
		default: hipLaunchKernelGGL((k_f32_grid_mlp_jvp2<WT, 3, 8>), blocks, block, 0, st, a); break;
	}
}

}  // namespace

bool f32_mlp_jvp2_width_ok(uint32_t W) { return W == 16 || W == 32 || W == 64; }

void launch_f32_mlp_jvp2(hipStream_t st, uint32_t B, uint32_t D, uint32_t IN, uint32_t W, uint32_t NH, uint32_t OUTP, uint32_t n_out,
                         const float* params, const float* x, const float* directions, uint32_t n_directions, bool x_soa, float* y, float* jvp,
                         float* second, bool y_soa, int act, int out_act, const GridCall* grid, const float* table, float scale, float offset) {
	const char* what = "fp32 forward Laplacian";
	TCNN_CHECK(f32_mlp_jvp2_width_ok(W), std::string(what) + ": the width must be 16, 32 or 64");
	TCNN_CHECK(NH >= 1, std::string(what) + ": at least one hidden layer");
	TCNN_CHECK(IN && OUTP && IN % 16 == 0 && OUTP % 16 == 0, std::string(what) + ": widths must be multiples of 16");
	TCNN_CHECK(B % 128 == 0, std::string(what) + ": batch must be a multiple of 128");
	TCNN_CHECK(n_out && n_out <= OUTP && OUTP - n_out < 16, std::string(what) + ": the padded output width must be the next multiple of 16");
	TCNN_CHECK(act != ACT_SINE && out_act != ACT_SINE, std::string(what) + ": Sine has no backward from its forward value");
	TCNN_CHECK(directions ? n_directions >= 1 : n_directions == D, std::string(what) + ": at least one direction, or the input width for the unit vectors");
	Jvp2Args b{};
	JvpArgs& a = b.j;
	if (grid) {
		TCNN_CHECK(grid->D == D && f32_mlp_jvp_grid_ok(D, grid->F, IN) && grid->L && grid->L * grid->F <= IN && !grid->opts.active,
		           std::string(what) + ": a grid of 2 or 3 input dimensions, 2, 4 or 8 features per level and at most 64 columns, without options");
		a.table = table;
		a.levels = grid->levels;
		a.L = grid->L;
		a.hash_grid = grid->hash_grid ? 1u : 0u;
		a.interp = (uint32_t)grid->interp;
		const uint32_t tb = grid->F * 4u < 16u ? grid->F * 4u : 16u;  // FVec loads, as in launch_f32_mlp_jvp
		a.vec = (uintptr_t)table % tb == 0 ? 1u : 0u;
		a.hash = (uint32_t)grid->hash;
	} else {
		TCNN_CHECK(D && D <= IN, std::string(what) + ": the input width must lie in [1, encoded width]");
	}
	if (!B) return;
	TCNN_CHECK(params && x && y && jvp && second && (!grid || table),
	           std::string(what) + ": the parameters, the inputs, the output, the product or the second-order sum are missing");
	a.B = B, a.D = D, a.IN = IN, a.NH = NH, a.OUTP = OUTP, a.NOUT = n_out, a.K = n_directions;
	a.P = params, a.X = x, a.V = directions, a.Y = y, a.J = jvp;
	b.Q = second;
	a.x_soa = x_soa ? 1u : 0u, a.y_soa = y_soa ? 1u : 0u;
	a.act = act, a.oact = out_act;
	a.scale = scale, a.offset = offset;
	const uint32_t F = grid ? grid->F : 0;
	switch (W) {
		case 16: jvp2_width<1>(st, b, grid != nullptr, D, F); break;
		case 32: jvp2_width<2>(st, b, grid != nullptr, D, F); break;
		default: jvp2_width<4>(st, b, grid != nullptr, D, F); break;
	}
	TCNN_HIP_CHECK(hipGetLastError());
}

}  // namespace tcnn_amd
