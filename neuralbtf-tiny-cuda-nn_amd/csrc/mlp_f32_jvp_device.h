// mlp_f32_jvp_device.h -- the two fronts of the forward-mode kernels behind a grid or an Identity (mlp_f32_jvp.hip, and
// its keeping twin in mlp_f32_jvp_train.hip): the kernel argument, the grid encoded straight into the MFMA operand
// layout with its tangents, and the first layer behind an Identity row. The forward that keeps a context runs these
// very functions, which is why it gives tcnn_module_inference_jvp's bits.
#pragma once

#include "grid_f32_device.h"
#include "mlp_f32_chain.h"

namespace tcnn_amd {

namespace {

struct JvpArgs {
	uint32_t B, D, IN, NH, OUTP, NOUT, K;  // K: tangents of the call (the directions, or D for the unit vectors)
	const float* P;  // [W0 [W][IN] | W1 .. W_{NH-1} [W][W] | Wout [OUTP][W]]
	const float* X;  // [B][D], or [D][B] when x_soa
	const float* V;  // directions [B][K][D], or [K D][B] when x_soa; null: the D unit vectors
	float* Y;        // [B][OUTP], or [NOUT][B] when y_soa
	float* J;        // [B][NOUT][K], or [NOUT K][B] when y_soa
	uint32_t x_soa, y_soa;
	int act, oact;
	// the grid in front
	const float* table;
	const LevelInfo* levels;
	uint32_t L, hash, hash_grid, interp, vec;  // hash: HashType; vec: the table allows FVec loads
	// the Identity in front
	float scale, offset;
};

constexpr int jvp_tangents(int WT) { return WT == 8 ? 1 : 3; }
constexpr uint32_t JVP_MAX_KSTEPS = 4;  // encoded width <= 64

// The two ends of k_f32_mlp_jacobian (mlp_f32_jacobian.hip) as functions, its operations in its order; that kernel keeps
// them in its body, where the register allocation its width table was measured with holds.
//
// The first layer behind an Identity row (x scale + offset on the D inputs, ones up to IN), lane (r, q)'s batch row
// `row`; X is [B][D], or [D][B] when xs. The value is the K-loop of k_f32_mlp_fwd: k-steps ascending and j = 0..3 into
// one accumulator per element. The tangents need no MFMA. V null: tangent i is input d0 + i - 1 of D, whose
// pre-activation tangent at neuron n is scale W0[n][d], one load per element and zero past D. Else tangent i is
// direction d0 + i - 1 of K, V [B][K][D] or [K D][B] when xs: scale sum_d W0[n][d] v[d], summed in ascending d, one
// FMA per term after the first.
template <int WT, int NQ>
__device__ __forceinline__ void jac_identity_layer(f4 (&h)[NQ][WT], const float* __restrict__ P, const float* __restrict__ X, bool xs,
                                                   const float* __restrict__ V, uint32_t B, uint32_t D, uint32_t K, uint32_t IN, float scale,
                                                   float offset, uint32_t r, uint32_t q, uint32_t row, uint32_t d0) {
#pragma unroll
	for (int c = 0; c < WT; ++c) h[0][c] = f4{0.0f, 0.0f, 0.0f, 0.0f};
	const float* wp = P + (size_t)r * IN + 4 * q;
	for (uint32_t s = 0; s < IN; s += 16) {
		f4 a;
#pragma unroll
		for (int j = 0; j < 4; ++j) {
			const uint32_t k = s + 4 * q + j;
			a[j] = 1.0f;
			if (k < D) a[j] = __builtin_fmaf(xs ? X[(size_t)k * B + row] : X[(size_t)row * D + k], scale, offset);
		}
#pragma unroll
		for (int c = 0; c < WT; ++c) {
			const f4 w = *(const f4*)(wp + (size_t)c * 16 * IN + s);
#pragma unroll
			for (int j = 0; j < 4; ++j) h[0][c] = mfma4(w[j], a[j], h[0][c]);
		}
	}
	const float* wn = P + (size_t)(4 * q) * IN;  // lane (r, q) holds neuron 16 c + 4 q + e as h[.][c][e]
	if (!V) {
#pragma unroll
		for (int i = 1; i < NQ; ++i) {
			const bool in = d0 + (i - 1) < D;
#pragma unroll
			for (int c = 0; c < WT; ++c)
#pragma unroll
				for (int e = 0; e < 4; ++e) h[i][c][e] = in ? scale * wn[(size_t)(16 * c + e) * IN + d0 + (i - 1)] : 0.0f;
		}
		return;
	}
	for (uint32_t d = 0; d < D; ++d) {
#pragma unroll
		for (int i = 1; i < NQ; ++i) {
			const uint32_t k = d0 + (i - 1);
			const float v = k < K ? (xs ? V[((size_t)k * D + d) * B + row] : V[((size_t)row * K + k) * D + d]) : 0.0f;
#pragma unroll
			for (int c = 0; c < WT; ++c)
#pragma unroll
				for (int e = 0; e < 4; ++e) {
					const float w = wn[(size_t)(16 * c + e) * IN + d];
					h[i][c][e] = d ? __builtin_fmaf(w, v, h[i][c][e]) : w * v;
				}
		}
	}
#pragma unroll
	for (int i = 1; i < NQ; ++i)
#pragma unroll
		for (int c = 0; c < WT; ++c)
#pragma unroll
			for (int e = 0; e < 4; ++e) h[i][c][e] *= scale;
}

// Lane quarter q's four columns of k-step s of one batch row: e[0] the value, e[i] the operand of tangent
// k0 + i - 1 (zero past K). x the row's position, dir[i - 1] its direction unless the directions are the unit vectors,
// prime the hash's multipliers.
template <uint32_t D, uint32_t F, int NQ>
__device__ __forceinline__ void jvp_encode_step(const JvpArgs& a, uint32_t s, uint32_t q, uint32_t k0, const float (&x)[D],
                                                const float (&dir)[NQ - 1][D], const uint32_t (&prime)[D], f4 (&e)[NQ]) {
	constexpr uint32_t NF = F == 2 ? 2 : 4, NLV = 4 / NF, NC = 1u << D;  // features per level slot, level slots, corners
	const Interp interp = (Interp)a.interp;
	const bool vec = a.vec != 0, hash_grid = a.hash_grid != 0;
	// A slot past the last level is padding. It walks the last level like the others and drops the result, which keeps
	// the walk free of lane-dependent branches: the compiler issues every gather of the k-step before the first use.
	LevelInfo li[NLV];
	bool on[NLV];
	uint32_t f0[NLV];
	float p[NLV][D], pd[NLV][D], w[NLV][NC];
	FVec<NF> v[NLV][NC];
#pragma unroll
	for (uint32_t u = 0; u < NLV; ++u) {
		const uint32_t col = 16 * s + 4 * q + u * NF, level = col / F;
		f0[u] = col % F;
		on[u] = level < a.L;
		li[u] = a.levels[on[u] ? level : a.L - 1];
		uint32_t pg[D];
#pragma unroll
		for (uint32_t d = 0; d < D; ++d) pos_fract_d(x[d], li[u].scale, interp, p[u][d], pd[u][d], pg[d]);
		const LevelInfo& l = li[u];
		auto index = [&](const uint32_t* local) { return grid_index_primes<D>(hash_grid, l.size, l.res, local, prime); };
		if (interp == Interp::Nearest) v[u][0] = load_fvec<NF>(a.table + (size_t)(l.offset + index(pg)) * F + f0[u], vec);
		else gather_level_f32<D, F, NF>(a.table, l, p[u], pg, f0[u], vec, index, w[u], v[u]);
	}
#pragma unroll
	for (uint32_t u = 0; u < NLV; ++u) {
		if (interp == Interp::Nearest) {  // the entry itself, and a derivative of exactly zero
#pragma unroll
			for (uint32_t f = 0; f < NF; ++f) {
				e[0][u * NF + f] = on[u] ? v[u][0].v[f] : 0.0f;
#pragma unroll
				for (int i = 1; i < NQ; ++i) e[i][u * NF + f] = 0.0f;
			}
			continue;
		}
		float val[NF], g[D][NF];
		combine_level_f32<NC, NF>(w[u], v[u], val);
#pragma unroll
		for (uint32_t gd = 0; gd < D; ++gd) level_tangent_f32<D, NF>(gd, li[u].scale, p[u], pd[u], v[u], g[gd]);
#pragma unroll
		for (uint32_t f = 0; f < NF; ++f) {
			e[0][u * NF + f] = on[u] ? val[f] : 0.0f;
#pragma unroll
			for (int i = 1; i < NQ; ++i) {
				float t = 0.0f;
				if (!a.V) {  // unit direction k0 + i - 1: selected, so that no register array is indexed at run time
#pragma unroll
					for (uint32_t d = 0; d < D; ++d)
						if (k0 + (i - 1) == d) t = g[d][f];
				} else {
					t = g[0][f] * dir[i - 1][0];
#pragma unroll
					for (uint32_t d = 1; d < D; ++d) t = __builtin_fmaf(g[d][f], dir[i - 1][d], t);
				}
				e[i][u * NF + f] = on[u] ? t : 0.0f;
			}
		}
	}
}

// The forward Laplacian's argument (mlp_f32_jvp2.hip): the call above and where sum_k v_k^T H v_k goes
struct Jvp2Args {
	JvpArgs j;
	float* Q;  // [B][NOUT], or [NOUT][B] when y_soa
};

// jvp_encode_step with the second-order operand: e[0] the value and e[1 .. NQ - 2] the tangents, the operations of
// jvp_encode_step in its order, and e[NQ - 1] the column's sum_{d, d'} M[d][d'] d^2 e / dx_d dx_d' with
// M = sum_{k in pass} v_k v_k^T (level_second_f32), from the same corners: no second gather. The term is skipped where
// it is exactly zero -- Nearest, and Linear with the unit directions -- and is zero on the padding columns.
template <uint32_t D, uint32_t F, int NQ>
__device__ __forceinline__ void jvp2_encode_step(const JvpArgs& a, uint32_t s, uint32_t q, uint32_t k0, const float (&x)[D],
                                                 const float (&dir)[NQ - 2][D], const float (&M)[D][D], const uint32_t (&prime)[D],
                                                 f4 (&e)[NQ]) {
	constexpr uint32_t NF = F == 2 ? 2 : 4, NLV = 4 / NF, NC = 1u << D;
	const Interp interp = (Interp)a.interp;
	const bool vec = a.vec != 0, hash_grid = a.hash_grid != 0;
	const bool diag = interp == Interp::Smoothstep, mixed = interp != Interp::Nearest && a.V != nullptr;
	LevelInfo li[NLV];
	bool on[NLV];
	uint32_t f0[NLV];
	float p[NLV][D], pd[NLV][D], pdd[NLV][D], w[NLV][NC];
	FVec<NF> v[NLV][NC];
#pragma unroll
	for (uint32_t u = 0; u < NLV; ++u) {
		const uint32_t col = 16 * s + 4 * q + u * NF, level = col / F;
		f0[u] = col % F;
		on[u] = level < a.L;
		li[u] = a.levels[on[u] ? level : a.L - 1];
		uint32_t pg[D];
#pragma unroll
		for (uint32_t d = 0; d < D; ++d) {
			pos_fract_d(x[d], li[u].scale, interp, p[u][d], pd[u][d], pg[d]);
			pdd[u][d] = pos_fract_dd(x[d], li[u].scale, interp);
		}
		const LevelInfo& l = li[u];
		auto index = [&](const uint32_t* local) { return grid_index_primes<D>(hash_grid, l.size, l.res, local, prime); };
		if (interp == Interp::Nearest) v[u][0] = load_fvec<NF>(a.table + (size_t)(l.offset + index(pg)) * F + f0[u], vec);
		else gather_level_f32<D, F, NF>(a.table, l, p[u], pg, f0[u], vec, index, w[u], v[u]);
	}
#pragma unroll
	for (uint32_t u = 0; u < NLV; ++u) {
		if (interp == Interp::Nearest) {
#pragma unroll
			for (uint32_t f = 0; f < NF; ++f) {
				e[0][u * NF + f] = on[u] ? v[u][0].v[f] : 0.0f;
#pragma unroll
				for (int i = 1; i < NQ; ++i) e[i][u * NF + f] = 0.0f;
			}
			continue;
		}
		float val[NF], g[D][NF], u2[NF];
		combine_level_f32<NC, NF>(w[u], v[u], val);
#pragma unroll
		for (uint32_t gd = 0; gd < D; ++gd) level_tangent_f32<D, NF>(gd, li[u].scale, p[u], pd[u], v[u], g[gd]);
		level_second_f32<D, NF>(li[u].scale, p[u], pd[u], pdd[u], v[u], M, diag, mixed, u2);
#pragma unroll
		for (uint32_t f = 0; f < NF; ++f) {
			e[0][u * NF + f] = on[u] ? val[f] : 0.0f;
#pragma unroll
			for (int i = 1; i < NQ - 1; ++i) {
				float t = 0.0f;
				if (!a.V) {
#pragma unroll
					for (uint32_t d = 0; d < D; ++d)
						if (k0 + (i - 1) == d) t = g[d][f];
				} else {
					t = g[0][f] * dir[i - 1][0];
#pragma unroll
					for (uint32_t d = 1; d < D; ++d) t = __builtin_fmaf(g[d][f], dir[i - 1][d], t);
				}
				e[i][u * NF + f] = on[u] ? t : 0.0f;
			}
			e[NQ - 1][u * NF + f] = on[u] ? u2[f] : 0.0f;
		}
	}
}

// ---- shared by the kernels that train through these calls (mlp_f32_jvp_train.hip, mlp_f32_jvp2_train.hip) ----

// f32_act_has_curvature (kernels.h) on the device: wave-uniform, so a network without curvature branches around S
__device__ __forceinline__ bool act_has_curvature(int a) { return a != ACT_NONE && a != ACT_RELU && a != ACT_LEAKY_RELU && a != ACT_SINE; }

// Where the pieces of a context lie (floats), nq quantities: 1 + K, the value and the tangents, or 2 + K with the
// second-order sum last (S_j then holds r_j after the tangents)
struct KeepLayout {
	size_t B, nq, IN, W, NH, OUTP;
	__host__ __device__ size_t x(uint32_t j) const { return j == 0 ? 0 : nq * B * IN + (size_t)(j - 1) * nq * B * W; }  // X_j, j <= NH
	__host__ __device__ size_t y() const { return nq * B * (IN + NH * W); }
	__host__ __device__ size_t s(uint32_t j) const { return y() + B * OUTP + (size_t)j * (nq - 1) * B * W; }  // S_j, j <= NH
	__host__ __device__ size_t total() const { return s((uint32_t)NH) + (nq - 1) * B * OUTP; }
	// the reverse chain's stack: G_j, j <= NH, then [hb_0 | tb_0] [nq][B][IN]
	__host__ __device__ size_t g(uint32_t j) const { return (size_t)j * nq * B * W; }
	__host__ __device__ size_t d0() const { return nq * B * (NH * W + OUTP); }
	__host__ __device__ size_t stack_total() const { return d0() + nq * B * IN; }
};

// quantity i's f4 of row `row` at column col of a [.][B][width] block
__device__ __forceinline__ float* slot(float* base, size_t B, uint32_t width, uint32_t i, uint32_t row, uint32_t col) {
	return base + ((size_t)i * B + row) * width + col;
}

// acc[i][c] += W[16 s + 4 q + j][16 c + r] g[i][s][j]: bwd_from_regs (mlp_f32_fused.hip) for 1 + TG adjoints, each
// weight used by all of them; wp = &W[4 q][r] of the first column tile, K the row length of W
template <int WT, int NQ, int NC>
__device__ __forceinline__ void jvp_bwd_from_regs(const float* __restrict__ wp, uint32_t K, const f4 (&g)[NQ][WT], f4 (&acc)[NQ][NC]) {
#pragma unroll
	for (int s = 0; s < WT; ++s)
#pragma unroll
		for (int c = 0; c < NC; ++c)
#pragma unroll
			for (int j = 0; j < 4; ++j) {
				const float w = wp[(size_t)(16 * s + j) * K + 16 * c];
#pragma unroll
				for (int i = 0; i < NQ; ++i) acc[i][c] = mfma4(w, g[i][s][j], acc[i][c]);
			}
}

}  // namespace
}  // namespace tcnn_amd
