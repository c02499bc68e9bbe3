// mlp_f32_chain.h -- the two steps of the forward-mode register chain, shared by the input Jacobian
// (mlp_f32_jacobian.hip) and the Jacobian-vector product behind a grid (mlp_f32_jvp.hip): a wave's 16-row tile carries
// the value (quantity 0) and NQ - 1 tangents through a matrix and through an activation. The kernels give each
// other's bits where they serve the same module because every product and every factor is these very functions.
// The forward Laplacian (mlp_f32_jvp2.hip) adds one row, the summed second-order quantity, and its gate jac_activate2.
#pragma once

#include "mlp_f32_ops.h"

namespace tcnn_amd {

namespace {

constexpr uint32_t JAC_ROWS_PER_WAVE = 16, JAC_ROWS_PER_BLOCK = 64;

// acc[i][c] += W[16 c + r][16 s + 4 q + j] x[i][s][j] for the value (i = 0) and the tangents, the first nct of NC
// column tiles; wp = &W[r][4 q] of the first tile, K = 16 WT the row length of W. The value's order is
// fwd_from_regs' (mlp_f32_fused.hip).
template <int WT, int NQ, int NC>
__device__ __forceinline__ void jac_from_regs(const float* __restrict__ wp, uint32_t nct, const f4 (&x)[NQ][WT], f4 (&acc)[NQ][NC]) {
	constexpr uint32_t K = 16 * WT;
#pragma unroll
	for (int s = 0; s < WT; ++s)
#pragma unroll
		for (int c = 0; c < NC; ++c) {
			if ((uint32_t)c < nct) {
				const f4 w = *(const f4*)(wp + (size_t)c * 16 * K + 16 * s);
#pragma unroll
				for (int j = 0; j < 4; ++j)
#pragma unroll
					for (int i = 0; i < NQ; ++i) acc[i][c] = mfma4(w[j], x[i][s][j], acc[i][c]);
			}
		}
}

// h <- act(h) and T_d <- act'(h) o T_d, the factor from the post-activation value through the delta chain's function
// (bwd_act with a unit delta is the factor itself)
template <int WT, int NQ>
__device__ __forceinline__ void jac_activate(f4 (&h)[NQ][WT], int act) {
	if (act == ACT_NONE) return;
#pragma unroll
	for (int c = 0; c < WT; ++c)
#pragma unroll
		for (int e = 0; e < 4; ++e) {
			const float y = fwd_act(act, h[0][c][e]);
			const float f = bwd_act(act, 1.0f, y);
			h[0][c][e] = y;
#pragma unroll
			for (int i = 1; i < NQ; ++i) h[i][c][e] *= f;
		}
}

// act'' from the forward value, out of line like the other rare activations; exactly zero for None and ReLU
__device__ __noinline__ float curv_act_ool(int a, float y) { return act_factor2_f32(a, y); }
__device__ __forceinline__ float curv_act(int a, float y) {
	if (a == ACT_NONE || a == ACT_RELU) return 0.0f;
	return curv_act_ool(a, y);
}

// One element through the gate with curvature (the forward Laplacian, mlp_f32_jvp2.hip): q[0] the value, q[1 .. NQ - 2]
// the tangents s_k, q[NQ - 1] the summed second-order quantity r. y = act(z), s_k <- act' s_k exactly as jac_activate
// does it, and U = act' r + act'' sum_k s_k^2: the squares summed in ascending k with one FMA per term after the
// first, the update one multiply and one FMA.
template <int NQ>
__device__ __forceinline__ void jac_gate2(int act, float (&q)[NQ]) {
	const float y = fwd_act(act, q[0]);
	const float f = bwd_act(act, 1.0f, y);
	const float g = curv_act(act, y);
	float ss = q[1] * q[1];
#pragma unroll
	for (int i = 2; i < NQ - 1; ++i) ss = __builtin_fmaf(q[i], q[i], ss);
	q[0] = y;
	q[NQ - 1] = __builtin_fmaf(g, ss, f * q[NQ - 1]);
#pragma unroll
	for (int i = 1; i < NQ - 1; ++i) q[i] *= f;
}

// jac_activate for a tile that carries the second-order quantity as its last row
template <int WT, int NQ>
__device__ __forceinline__ void jac_activate2(f4 (&h)[NQ][WT], int act) {
	if (act == ACT_NONE) return;
#pragma unroll
	for (int c = 0; c < WT; ++c)
#pragma unroll
		for (int e = 0; e < 4; ++e) {
			float q[NQ];
#pragma unroll
			for (int i = 0; i < NQ; ++i) q[i] = h[i][c][e];
			jac_gate2<NQ>(act, q);
#pragma unroll
			for (int i = 0; i < NQ; ++i) h[i][c][e] = q[i];
		}
}

}  // namespace
}  // namespace tcnn_amd
