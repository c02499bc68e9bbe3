// mlp_f32_jvp2_train.hip -- training through the forward Laplacian of an fp32 FullyFusedMLP network module behind a lone
// grid or a lone Identity: the reverse pass of value_jvp_and_second. Given dL/dy, dL/dJv and dL/dq of a loss L(y, Jv, q)
// it produces dL/dparams (NetworkF32Host::jvp_second_forward / jvp_second_backward, tcnn_module_forward_jvp_second /
// tcnn_module_backward_jvp_second). DESIGN.md, "Training through the forward Laplacian".
//
// One batch row, layers j = 0..NH, phi = a', psi = a'', chi = a''' from the stored forward value:
//   forward   z = W h, s_k = W t_k, r = W U;  h' = a(z), t_k' = phi s_k, U' = phi r + psi sum_k s_k^2
//   reverse, from hb', tb_k', Ub' (top: dL/dy, dL/dJv_k, dL/dq)
//     rb   = phi Ub'
//     sb_k = phi tb_k' + 2 psi s_k Ub'
//     zb   = phi hb' + c,  c = psi (sum_k s_k tb_k' + r Ub') + chi (sum_k s_k^2) Ub'
//     dW   = sum_b (zb h^T + sum_k sb_k t_k^T + rb U^T);  hb = W^T zb, tb_k = W^T sb_k, Ub = W^T rb
//
// Three kernels.
//
// 1. The keeping forward, k_f32_grid_mlp_jvp2_keep and k_f32_identity_mlp_jvp2_keep: mlp_f32_jvp2.hip's single pass
//    (K <= 3), the same functions in the same order, so y, Jv and q carry tcnn_module_inference_jvp_second's bits, plus
//    the stores of a context. The context is KeepLayout with nq = 2 + K: X_j = (h_j, t_{j,1..K}, U_j) and
//    S_j = (s_{j,1..K}, r_j), S written and read only where the activation has curvature. Behind an Identity U_0 = 0 is
//    not stored: the first layer's weight gradient runs over the 1 + K leading quantities.
//
// 2. The reverse chain, k_f32_mlp_jvp2_bwd_chain<WT, K>, in k_f32_mlp_jvp_bwd_chain's operand scheme: one wave owns a
//    16-row tile and all W columns, the 2 + K adjoints (hb, tb_1..K, Ub) live in registers, the gate is lane-local, each
//    weight is loaded once and fed to every adjoint's MFMA; no LDS, no barrier. The compiler's resource report decides
//    the shape: the five adjoints of K = 3 fit at W 64 (364 unified registers, 160 of them accumulation registers, no
//    spill, no scratch), so the launch is one chain. The alternative that splits the recurrence into a (tb, Ub)
//    sub-chain and an hb sub-chain would also run one wave per SIMD, with a second walk over the weights and a round
//    trip of the curvature part through memory besides, so it is not built (DESIGN.md has the table).
//    The stack: G_j = (zb_j, sb_{j,1..K}, rb_j) [nq][B][N_j], then (hb_0, tb_{0,1..K}, Ub_0) [nq][B][IN].
//
// 3. The table gradient's tangent and second-order terms in one corner walk, k_grid_jvp2_bwd_f32<D, F>:
//      dL/dtable[idx_c][f] += sum_d (dw_c/dx_d) G_d[f] + (sum_{d,d'} M[d][d'] d^2 w_c/dx_d dx_d') Ub_0[f]
//    G_d = sum_k v_k[d] tb_{0,k}, M = sum_k v_k v_k^T, both in registers; one thread per (point, level), blockIdx.y the
//    level; one fp32 atomic per corner and feature into a zeroed scratch table. jvp2_encode_step's wave-uniform skips:
//    no diagonal part unless Smoothstep, no mixed part for the unit vectors, no launch for Nearest.
#include "grid_dispatch.h"
#include "mlp_f32_jvp_device.h"

namespace tcnn_amd {

namespace {

constexpr int JVP2_TRAIN_TANGENTS = 3;  // mlp_f32_jvp2.hip's T2: one pass

__device__ __noinline__ float act_factor3_f32_ool(int a, float y) { return act_factor3_f32(a, y); }

// ---- 1: the keeping forward ----

// The pass holds NQ = 2 + T2 rows, the call has K <= T2 tangents: row i is quantity i of the context for the value and
// the call's tangents, the last row (U) is quantity K + 1, and the rows between are zero and not kept.
template <int NQ>
__device__ __forceinline__ bool row_kept(int i, uint32_t K) { return (uint32_t)i <= K || i == NQ - 1; }
template <int NQ>
__device__ __forceinline__ uint32_t row_quantity(int i, uint32_t K) { return i == NQ - 1 ? K + 1 : (uint32_t)i; }

// jac_activate2 between two rounds of stores: s_k and r before the gate (an activation with curvature only), then
// h', t_k' and U'. X and S are [.][B][NC 16] blocks.
template <int NC, int NQ>
__device__ __forceinline__ void keep2_activate(f4 (&h)[NQ][NC], int act, float* __restrict__ S, float* __restrict__ Xn, uint32_t B, uint32_t width,
                                               uint32_t K, uint32_t row, uint32_t col) {
	if (act_has_curvature(act)) {
#pragma unroll
		for (int i = 1; i < NQ; ++i)
			if (row_kept<NQ>(i, K))
#pragma unroll
				for (int c = 0; c < NC; ++c) *(f4*)slot(S, B, width, row_quantity<NQ>(i, K) - 1, row, 16 * c + col) = h[i][c];
	}
	jac_activate2<NC, NQ>(h, act);
	if (!Xn) return;
#pragma unroll
	for (int i = 0; i < NQ; ++i)
		if (row_kept<NQ>(i, K))
#pragma unroll
			for (int c = 0; c < NC; ++c) *(f4*)slot(Xn, B, width, row_quantity<NQ>(i, K), row, 16 * c + col) = h[i][c];
}

// jvp2_chain (mlp_f32_jvp2.hip) for its first pass with AoS results, writing the context as it goes
template <int WT, int NQ>
__device__ __forceinline__ void keep2_chain(f4 (&h)[NQ][WT], const Jvp2Args& b, const KeepLayout& kl, float* __restrict__ keep, uint32_t r,
                                            uint32_t q, uint32_t row) {
	const JvpArgs& a = b.j;
	constexpr uint32_t W = 16 * WT;
	const uint32_t nt = (a.NOUT + 15) / 16, K = a.K, B = a.B;
	const float* wl = a.P + (size_t)W * a.IN;
	keep2_activate<WT, NQ>(h, a.act, keep + kl.s(0), keep + kl.x(1), B, W, K, row, 4 * q);
	for (uint32_t l = 1; l < a.NH; ++l, wl += (size_t)W * W) {
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
		keep2_activate<WT, NQ>(h, a.act, keep + kl.s(l), keep + kl.x(l + 1), B, W, K, row, 4 * q);
	}
	for (uint32_t c0 = 0; c0 < nt; ++c0) {
		f4 o[NQ][1];
#pragma unroll
		for (int i = 0; i < NQ; ++i) o[i][0] = f4{0.0f, 0.0f, 0.0f, 0.0f};
		jac_from_regs<WT, NQ, 1>(wl + (size_t)(16 * c0 + r) * W + 4 * q, 1, h, o);
		const uint32_t n0 = 16 * c0 + 4 * q;
		keep2_activate<1, NQ>(o, a.oact, keep + kl.s(a.NH), nullptr, B, a.OUTP, K, row, n0);
		*(f4*)(a.Y + (size_t)row * a.OUTP + n0) = o[0][0];
		*(f4*)(keep + kl.y() + (size_t)row * a.OUTP + n0) = o[0][0];
		float* je = a.J + ((size_t)row * a.NOUT + n0) * K;
		float* qe = b.Q + (size_t)row * a.NOUT + n0;
#pragma unroll
		for (int e = 0; e < 4; ++e, je += K) {
			if (n0 + e < a.NOUT) {
#pragma unroll
				for (int i = 1; i < NQ - 1; ++i)
					if ((uint32_t)(i - 1) < K) je[i - 1] = o[i][0][e];
				qe[e] = o[NQ - 1][0][e];
			}
		}
	}
}

// Grid B / 64, K <= T2. k_f32_grid_mlp_jvp2's first pass with the stores of the context.
template <int WT, uint32_t D, uint32_t F>
__global__ __launch_bounds__(256) void k_f32_grid_mlp_jvp2_keep(const Jvp2Args b, float* __restrict__ keep) {
	const JvpArgs& a = b.j;
	constexpr uint32_t W = 16 * WT;
	constexpr int T2 = JVP2_TRAIN_TANGENTS, NQ = 2 + T2;
	const uint32_t lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;
	const uint32_t row = (blockIdx.x * 4 + (threadIdx.x >> 6)) * JAC_ROWS_PER_WAVE + r;
	if (row >= a.B) return;
	const KeepLayout kl{a.B, 2 + (size_t)a.K, a.IN, W, a.NH, a.OUTP};
	float x[D];
#pragma unroll
	for (uint32_t d = 0; d < D; ++d) x[d] = a.X[(size_t)row * D + d];
	uint32_t prime[D];
	hash_primes<D>((HashType)a.hash, prime);
	const uint32_t ks = a.IN / 16;
	float dir[T2][D];
#pragma unroll
	for (int i = 0; i < T2; ++i)
#pragma unroll
		for (uint32_t d = 0; d < D; ++d) dir[i][d] = a.V && (uint32_t)i < a.K ? a.V[((size_t)row * a.K + i) * D + d] : 0.0f;
	float M[D][D];
#pragma unroll
	for (uint32_t d = 0; d < D; ++d)
#pragma unroll
		for (uint32_t e = 0; e < D; ++e) {
			float m = d == e && d < (uint32_t)T2 ? 1.0f : 0.0f;
			if (a.V) {
				m = dir[0][d] * dir[0][e];
#pragma unroll
				for (int i = 1; i < T2; ++i) m = __builtin_fmaf(dir[i][d], dir[i][e], m);
			}
			M[d][e] = m;
		}
	f4 e[NQ][JVP_MAX_KSTEPS];
#pragma unroll
	for (uint32_t s = 0; s < JVP_MAX_KSTEPS; ++s) {
		if (s < ks) {
			f4 es[NQ];
			jvp2_encode_step<D, F, NQ>(a, s, q, 0, x, dir, M, prime, es);
#pragma unroll
			for (int i = 0; i < NQ; ++i) {
				e[i][s] = es[i];
				if (row_kept<NQ>(i, a.K)) *(f4*)slot(keep, a.B, a.IN, row_quantity<NQ>(i, a.K), row, 16 * s + 4 * q) = es[i];
			}
		}
	}
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
	keep2_chain<WT, NQ>(h, b, kl, keep, r, q, row);
}

// The same behind an Identity row: U_0 = 0 enters the first gate and is not kept; t_{0,k} as
// k_f32_identity_mlp_jvp_keep stores it, the weight gradient's operand
template <int WT>
__global__ __launch_bounds__(256) void k_f32_identity_mlp_jvp2_keep(const Jvp2Args b, float* __restrict__ keep) {
	const JvpArgs& a = b.j;
	constexpr uint32_t W = 16 * WT;
	constexpr int T2 = JVP2_TRAIN_TANGENTS, NQ = 2 + T2;
	const uint32_t lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;
	const uint32_t row = (blockIdx.x * 4 + (threadIdx.x >> 6)) * JAC_ROWS_PER_WAVE + r;
	if (row >= a.B) return;
	const KeepLayout kl{a.B, 2 + (size_t)a.K, a.IN, W, a.NH, a.OUTP};
	for (uint32_t s = 0; s < a.IN; s += 16) {
		f4 v[NQ - 1];
#pragma unroll
		for (int j = 0; j < 4; ++j) {
			const uint32_t k = s + 4 * q + j;
			v[0][j] = k < a.D ? __builtin_fmaf(a.X[(size_t)row * a.D + k], a.scale, a.offset) : 1.0f;
#pragma unroll
			for (int i = 1; i < NQ - 1; ++i) {
				float t = 0.0f;
				if (k < a.D && (uint32_t)i <= a.K) t = a.V ? a.scale * a.V[((size_t)row * a.K + (i - 1)) * a.D + k] : (k == (uint32_t)(i - 1) ? a.scale : 0.0f);
				v[i][j] = t;
			}
		}
#pragma unroll
		for (int i = 0; i < NQ - 1; ++i)
			if ((uint32_t)i <= a.K) *(f4*)slot(keep, a.B, a.IN, i, row, s + 4 * q) = v[i];
	}
	f4 t[NQ - 1][WT], h[NQ][WT];
	jac_identity_layer<WT, NQ - 1>(t, a.P, a.X, false, a.V, a.B, a.D, a.K, a.IN, a.scale, a.offset, r, q, row, 0);
#pragma unroll
	for (int c = 0; c < WT; ++c) {
#pragma unroll
		for (int i = 0; i < NQ - 1; ++i) h[i][c] = t[i][c];
		h[NQ - 1][c] = f4{0.0f, 0.0f, 0.0f, 0.0f};
	}
	keep2_chain<WT, NQ>(h, b, kl, keep, r, q, row);
}

template <int WT>
void keep2_width(hipStream_t st, const Jvp2Args& a, float* keep, bool grid, uint32_t D, uint32_t F) {
	const dim3 blocks(a.j.B / JAC_ROWS_PER_BLOCK), block(256);
	if (!grid) {
		hipLaunchKernelGGL((k_f32_identity_mlp_jvp2_keep<WT>), blocks, block, 0, st, a, keep);
		return;
	}
	switch (D * 16 + F) {
		case 2 * 16 + 2: hipLaunchKernelGGL((k_f32_grid_mlp_jvp2_keep<WT, 2, 2>), blocks, block, 0, st, a, keep); break;
		case 2 * 16 + 4: hipLaunchKernelGGL((k_f32_grid_mlp_jvp2_keep<WT, 2, 4>), blocks, block, 0, st, a, keep); break;
		case 2 * 16 + 8: hipLaunchKernelGGL((k_f32_grid_mlp_jvp2_keep<WT, 2, 8>), blocks, block, 0, st, a, keep); break;
		case 3 * 16 + 2: hipLaunchKernelGGL((k_f32_grid_mlp_jvp2_keep<WT, 3, 2>), blocks, block, 0, st, a, keep); break;
		case 3 * 16 + 4: hipLaunchKernelGGL((k_f32_grid_mlp_jvp2_keep<WT, 3, 4>), blocks, block, 0, st, a, keep); break;
		default: hipLaunchKernelGGL((k_f32_grid_mlp_jvp2_keep<WT, 3, 8>), blocks, block, 0, st, a, keep); break;
	}
}

// ---- 2: the reverse chain ----

struct Jvp2BwdArgs {
	uint32_t B, IN, NH, OUTP, NOUT;
	const float* P;     // [W0 | W1 .. W_{NH-1} | Wout]
	const float* KEEP;  // the keeping forward's context
	const float* DY;    // dL/dy [B][OUTP], nullable: zero; columns past NOUT count as zero
	const float* DJ;    // dL/dJv [B][NOUT][K], nullable: zero
	const float* DQ;    // dL/dq [B][NOUT], nullable: zero
	float* G;           // [G_0 .. G_NH | hb_0, tb_0, Ub_0], KeepLayout::g / d0
	uint32_t want_d0;   // the encoding in front has parameters
	int act, oact;
};

// The gate of one layer on the lane's four neurons: g = (hb, tb_1..K, Ub), the adjoints of the layer's output, come in and
// (zb, sb_1..K, rb) go out.
//   acc = sum_k s_k tb_k + r Ub and ss = sum_k s_k^2 in ascending k, one FMA per term after the first;
//   c = chi (ss Ub) + psi acc;  sb_k = (2 psi Ub) s_k + phi tb_k;  rb = phi Ub;  zb = phi hb + c.
// yv: the layer's forward value; sv = (s_1..K, r) of the context, read only when the activation has curvature.
template <int K>
__device__ __forceinline__ void jvp2_gate(int act, bool curv, const f4& yv, const f4 (&sv)[K + 1], f4 (&g)[K + 2]) {
	if (act == ACT_NONE) return;
#pragma unroll
	for (int e = 0; e < 4; ++e) {
		const float phi = bwd_act(act, 1.0f, yv[e]), ub = g[K + 1][e];
		float c = 0.0f;
		if (curv) {
			const float psi = curv_act_ool(act, yv[e]), chi = act_factor3_f32_ool(act, yv[e]);
			float acc = sv[0][e] * g[1][e], ss = sv[0][e] * sv[0][e];
#pragma unroll
			for (int k = 1; k < K; ++k) {
				acc = __builtin_fmaf(sv[k][e], g[1 + k][e], acc);
				ss = __builtin_fmaf(sv[k][e], sv[k][e], ss);
			}
			acc = __builtin_fmaf(sv[K][e], ub, acc);
			c = __builtin_fmaf(chi, ss * ub, psi * acc);
			const float pu = 2.0f * psi * ub;
#pragma unroll
			for (int k = 0; k < K; ++k) g[1 + k][e] = __builtin_fmaf(pu, sv[k][e], phi * g[1 + k][e]);
		} else {
#pragma unroll
			for (int k = 0; k < K; ++k) g[1 + k][e] *= phi;
		}
		g[K + 1][e] = phi * ub;
		g[0][e] = __builtin_fmaf(phi, g[0][e], c);
	}
}

// Grid B / 64. K is the call's: every quantity is live, nothing is guarded. k_f32_mlp_jvp_bwd_chain's body with Ub as
// the last adjoint.
template <int WT, int K>
__global__ __launch_bounds__(256) void k_f32_mlp_jvp2_bwd_chain(const Jvp2BwdArgs a) {
	constexpr uint32_t W = 16 * WT;
	constexpr int NQ = 2 + K;
	const uint32_t lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;
	const uint32_t row = (blockIdx.x * 4 + (threadIdx.x >> 6)) * JAC_ROWS_PER_WAVE + r;
	if (row >= a.B) return;
	const KeepLayout kl{a.B, NQ, a.IN, W, a.NH, a.OUTP};
	const size_t B = a.B;
	const bool curv = act_has_curvature(a.act), ocurv = act_has_curvature(a.oact);
	const float* wl = a.P + (size_t)W * a.IN + (size_t)(a.NH - 1) * W * W;  // Wout, then W_{NH-1} .. W_1
	f4 d[NQ][WT];
#pragma unroll
	for (int i = 0; i < NQ; ++i)
#pragma unroll
		for (int c = 0; c < WT; ++c) d[i][c] = f4{0.0f, 0.0f, 0.0f, 0.0f};
	{  // output layer: the cotangents come from memory, one k-step of 16 output neurons at a time
		const float* Yv = a.KEEP + kl.y() + (size_t)row * a.OUTP;
		const float* SN = a.KEEP + kl.s(a.NH);
		float* GN = a.G + kl.g(a.NH);
		const float* wp = wl + (size_t)(4 * q) * W + r;
		for (uint32_t s = 0; s < a.OUTP; s += 16) {
			const uint32_t n0 = s + 4 * q;
			f4 g[NQ], sv[K + 1];
#pragma unroll
			for (int j = 0; j < 4; ++j) {
				const bool in = n0 + j < a.NOUT;
				g[0][j] = a.DY && in ? a.DY[(size_t)row * a.OUTP + n0 + j] : 0.0f;
#pragma unroll
				for (int k = 0; k < K; ++k) g[1 + k][j] = a.DJ && in ? a.DJ[((size_t)row * a.NOUT + n0 + j) * K + k] : 0.0f;
				g[K + 1][j] = a.DQ && in ? a.DQ[(size_t)row * a.NOUT + n0 + j] : 0.0f;
			}
			if (a.oact != ACT_NONE) {
				if (ocurv)
#pragma unroll
					for (int k = 0; k <= K; ++k) sv[k] = *(const f4*)(SN + ((size_t)k * B + row) * a.OUTP + n0);
				jvp2_gate<K>(a.oact, ocurv, *(const f4*)(Yv + n0), sv, g);
			}
#pragma unroll
			for (int i = 0; i < NQ; ++i) *(f4*)(GN + ((size_t)i * B + row) * a.OUTP + n0) = g[i];
#pragma unroll
			for (int c = 0; c < WT; ++c)
#pragma unroll
				for (int j = 0; j < 4; ++j) {
					const float w = wp[(size_t)(s + j) * W + 16 * c];
#pragma unroll
					for (int i = 0; i < NQ; ++i) d[i][c] = mfma4(w, g[i][j], d[i][c]);
				}
		}
	}
	for (uint32_t l = a.NH; l-- > 0;) {  // d: the adjoints of layer l's output. Gate with its activation, store, go down
		const float* Hn = a.KEEP + kl.x(l + 1) + (size_t)row * W + 4 * q;  // h_{l+1}: quantity 0 of X_{l+1}
		const float* Sl = a.KEEP + kl.s(l) + (size_t)row * W + 4 * q;
		float* Gl = a.G + kl.g(l) + (size_t)row * W + 4 * q;
#pragma unroll
		for (int c = 0; c < WT; ++c) {
			f4 g[NQ], sv[K + 1];
#pragma unroll
			for (int i = 0; i < NQ; ++i) g[i] = d[i][c];
			if (a.act != ACT_NONE) {
				if (curv)
#pragma unroll
					for (int k = 0; k <= K; ++k) sv[k] = *(const f4*)(Sl + (size_t)k * B * W + 16 * c);
				jvp2_gate<K>(a.act, curv, *(const f4*)(Hn + 16 * c), sv, g);
			}
#pragma unroll
			for (int i = 0; i < NQ; ++i) {
				d[i][c] = g[i];
				*(f4*)(Gl + (size_t)i * B * W + 16 * c) = g[i];
			}
		}
		if (l == 0) break;
		wl -= (size_t)W * W;
		f4 n[NQ][WT];
#pragma unroll
		for (int i = 0; i < NQ; ++i)
#pragma unroll
			for (int c = 0; c < WT; ++c) n[i][c] = f4{0.0f, 0.0f, 0.0f, 0.0f};
		jvp_bwd_from_regs<WT, NQ, WT>(wl + (size_t)(4 * q) * W + r, W, d, n);
#pragma unroll
		for (int i = 0; i < NQ; ++i)
#pragma unroll
			for (int c = 0; c < WT; ++c) d[i][c] = n[i][c];
	}
	if (!a.want_d0) return;
	// first layer: the adjoints of the encoded row, one column tile at a time, each a full contraction from d
	float* D0 = a.G + kl.d0();
	for (uint32_t c0 = 0; c0 < a.IN / 16; ++c0) {
		f4 o[NQ][1];
#pragma unroll
		for (int i = 0; i < NQ; ++i) o[i][0] = f4{0.0f, 0.0f, 0.0f, 0.0f};
		jvp_bwd_from_regs<WT, NQ, 1>(a.P + (size_t)(4 * q) * a.IN + 16 * c0 + r, a.IN, d, o);
#pragma unroll
		for (int i = 0; i < NQ; ++i) *(f4*)(D0 + ((size_t)i * B + row) * a.IN + 16 * c0 + 4 * q) = o[i][0];
	}
}

template <int WT, int K>
void bwd2_chain_launch(hipStream_t st, const Jvp2BwdArgs& a) {
	hipLaunchKernelGGL((k_f32_mlp_jvp2_bwd_chain<WT, K>), dim3(a.B / JAC_ROWS_PER_BLOCK), dim3(256), 0, st, a);
}

template <int WT>
void bwd2_chain_width(hipStream_t st, const Jvp2BwdArgs& a, uint32_t K) {
	if (K == 1) bwd2_chain_launch<WT, 1>(st, a);
	else if (K == 2) bwd2_chain_launch<WT, 2>(st, a);
	else bwd2_chain_launch<WT, 3>(st, a);
}

// ---- 3: the tangent and second-order terms of the table gradient ----

// Grid (B / 256, L). X [B][D]; V [B][K][D], null: the D unit vectors (K = D); T0 = (tb_{0,1..K}, Ub_0) as
// [K + 1][B][IN]; grad: the zeroed scratch table. Linear and Smoothstep only (the host does not launch for Nearest).
template <uint32_t D, uint32_t F>
__global__ __launch_bounds__(256) void k_grid_jvp2_bwd_f32(uint32_t B, uint32_t K, uint32_t IN, const float* __restrict__ X,
                                                           const float* __restrict__ V, const float* __restrict__ T0, float* __restrict__ grad,
                                                           const LevelInfo* __restrict__ levels, uint32_t hash, uint32_t hash_grid,
                                                           uint32_t interp_u) {
	const uint32_t b = blockIdx.x * 256 + threadIdx.x, l = blockIdx.y;
	if (b >= B) return;
	const LevelInfo li = levels[l];
	const Interp interp = (Interp)interp_u;
	const bool diag = interp == Interp::Smoothstep, mixed = V != nullptr;
	uint32_t prime[D];
	hash_primes<D>((HashType)hash, prime);
	float p[D], pd[D], pdd[D];
	uint32_t pg[D];
#pragma unroll
	for (uint32_t d = 0; d < D; ++d) {
		pos_fract_d(X[(size_t)b * D + d], li.scale, interp, p[d], pd[d], pg[d]);
		pdd[d] = pos_fract_dd(X[(size_t)b * D + d], li.scale, interp);
	}
	// G_d = sum_k v_k[d] tb_{0,k} and M = sum_k v_k v_k^T, in ascending k, one FMA per term after the first; the unit
	// vectors select, and their M is the identity
	float G[D][F], M[D][D];
#pragma unroll
	for (uint32_t d = 0; d < D; ++d) {
#pragma unroll
		for (uint32_t f = 0; f < F; ++f) G[d][f] = 0.0f;
#pragma unroll
		for (uint32_t e = 0; e < D; ++e) M[d][e] = !V && d == e ? 1.0f : 0.0f;
	}
#pragma unroll
	for (uint32_t k = 0; k < 3; ++k) {
		if (k < K) {
			const FVec<F> t = load_fvec<F>(T0 + ((size_t)k * B + b) * IN + l * F, true);
			float v[D];
#pragma unroll
			for (uint32_t d = 0; d < D; ++d) v[d] = V ? V[((size_t)b * K + k) * D + d] : 0.0f;
#pragma unroll
			for (uint32_t d = 0; d < D; ++d) {
				if (V) {
#pragma unroll
					for (uint32_t f = 0; f < F; ++f) G[d][f] = k ? __builtin_fmaf(v[d], t.v[f], G[d][f]) : v[d] * t.v[f];
#pragma unroll
					for (uint32_t e = d; e < D; ++e) M[d][e] = k ? __builtin_fmaf(v[d], v[e], M[d][e]) : v[d] * v[e];
				} else if (d == k) {
#pragma unroll
					for (uint32_t f = 0; f < F; ++f) G[d][f] = t.v[f];
				}
			}
		}
	}
	const FVec<F> ub = load_fvec<F>(T0 + ((size_t)K * B + b) * IN + l * F, true);
	const bool second = diag || mixed;
#pragma unroll
	for (uint32_t c = 0; c < (1u << D); ++c) {
		uint32_t local[D];
		float w[D], sg[D];
#pragma unroll
		for (uint32_t d = 0; d < D; ++d) {
			const bool hi = (c >> d) & 1u;
			local[d] = pg[d] + (hi ? 1u : 0u);
			w[d] = hi ? p[d] : 1.0f - p[d];
			sg[d] = hi ? 1.0f : -1.0f;
		}
		float* entry = grad + (size_t)(li.offset + grid_index_primes<D>(hash_grid != 0, li.size, li.res, local, prime)) * F;
		// dw_c / dx_d = scale pd_d (+-1) prod_{o != d} w_o, the product from the scale on as level_tangent_f32 forms it.
		// m2 = sum_{d,d'} M[d][d'] d^2 w_c / dx_d dx_d': the diagonal scale^2 pdd_d (+-1) prod_{o != d} w_o, the mixed
		// parts 2 M[d][e] scale^2 pd_d pd_e (+-1)(+-1) prod_{o != d, e} w_o, as level_second_f32 weighs the corners.
		float a[D], m2 = 0.0f;
#pragma unroll
		for (uint32_t d = 0; d < D; ++d) {
			float pe = li.scale;
#pragma unroll
			for (uint32_t o = 0; o < D; ++o)
				if (o != d) pe *= w[o];
			a[d] = sg[d] * (pe * pd[d]);
			if (diag) m2 = __builtin_fmaf(M[d][d] * li.scale, sg[d] * (pe * pdd[d]), m2);
		}
		if (mixed) {
#pragma unroll
			for (uint32_t d = 0; d < D; ++d)
#pragma unroll
				for (uint32_t e = d + 1; e < D; ++e) {
					float wo = sg[d] * sg[e];
#pragma unroll
					for (uint32_t o = 0; o < D; ++o)
						if (o != d && o != e) wo *= w[o];
					m2 = __builtin_fmaf(2.0f * M[d][e] * ((li.scale * pd[d]) * (li.scale * pd[e])), wo, m2);
				}
		}
#pragma unroll
		for (uint32_t f = 0; f < F; ++f) {
			float v = a[0] * G[0][f];
#pragma unroll
			for (uint32_t d = 1; d < D; ++d) v = __builtin_fmaf(a[d], G[d][f], v);
			if (second) v = __builtin_fmaf(m2, ub.v[f], v);
			unsafeAtomicAdd(entry + f, v);
		}
	}
}

}  // namespace

uint32_t f32_mlp_jvp2_train_max_directions(uint32_t W) { return f32_mlp_jvp2_width_ok(W) ? (uint32_t)JVP2_TRAIN_TANGENTS : 0u; }

size_t f32_mlp_jvp2_keep_floats(uint32_t B, uint32_t K, uint32_t IN, uint32_t W, uint32_t NH, uint32_t OUTP) {
	return KeepLayout{B, 2 + (size_t)K, IN, W, NH, OUTP}.total();
}

size_t f32_mlp_jvp2_stack_floats(uint32_t B, uint32_t K, uint32_t IN, uint32_t W, uint32_t NH, uint32_t OUTP) {
	return KeepLayout{B, 2 + (size_t)K, IN, W, NH, OUTP}.stack_total();
}

size_t f32_mlp_jvp2_keep_x(uint32_t B, uint32_t K, uint32_t IN, uint32_t W, uint32_t NH, uint32_t OUTP, uint32_t j) {
	return KeepLayout{B, 2 + (size_t)K, IN, W, NH, OUTP}.x(j);
}

size_t f32_mlp_jvp2_stack_g(uint32_t B, uint32_t K, uint32_t IN, uint32_t W, uint32_t NH, uint32_t OUTP, uint32_t j) {
	const KeepLayout kl{B, 2 + (size_t)K, IN, W, NH, OUTP};
	return j <= NH ? kl.g(j) : kl.d0();
}

namespace {

void check_jvp2_train_shape(const char* what, uint32_t B, uint32_t IN, uint32_t W, uint32_t NH, uint32_t OUTP, uint32_t n_out, uint32_t K, int act,
                            int out_act) {
	TCNN_CHECK(f32_mlp_jvp2_width_ok(W), std::string(what) + ": the width must be 16, 32 or 64");
	TCNN_CHECK(NH >= 1, std::string(what) + ": at least one hidden layer");
	TCNN_CHECK(IN && OUTP && IN % 16 == 0 && OUTP % 16 == 0, std::string(what) + ": widths must be multiples of 16");
	TCNN_CHECK(B % 256 == 0, std::string(what) + ": batch must be a multiple of 256");
	TCNN_CHECK(n_out && n_out <= OUTP && OUTP - n_out < 16, std::string(what) + ": the padded output width must be the next multiple of 16");
	TCNN_CHECK(act != ACT_SINE && out_act != ACT_SINE, std::string(what) + ": Sine has no backward from its forward value");
	TCNN_CHECK(K >= 1 && K <= f32_mlp_jvp2_train_max_directions(W),
	           std::string(what) + ": " + std::to_string(K) + " directions at width " + std::to_string(W) + " (at most " +
	               std::to_string(f32_mlp_jvp2_train_max_directions(W)) + " are served)");
}

bool jvp2_train_grid_ok(const GridCall& g, uint32_t IN) { return f32_mlp_jvp_grid_ok(g.D, g.F, IN) && g.L && g.L * g.F <= IN && !g.opts.active; }

}  // namespace

void launch_f32_mlp_jvp2_keep(hipStream_t st, uint32_t B, uint32_t D, uint32_t IN, uint32_t W, uint32_t NH, uint32_t OUTP, uint32_t n_out,
                              const float* params, const float* x, const float* directions, uint32_t n_directions, float* y, float* jvp,
                              float* second, int act, int out_act, const GridCall* grid, const float* table, float scale, float offset,
                              float* keep) {
	const char* what = "fp32 forward Laplacian, keeping forward";
	check_jvp2_train_shape(what, B, IN, W, NH, OUTP, n_out, n_directions, act, out_act);
	TCNN_CHECK(directions || n_directions == D, std::string(what) + ": null directions are the unit vectors, as many as inputs");
	Jvp2Args b{};
	JvpArgs& a = b.j;
	if (grid) {
		TCNN_CHECK(grid->D == D && jvp2_train_grid_ok(*grid, IN),
		           std::string(what) + ": a grid of 2 or 3 input dimensions, 2, 4 or 8 features per level and at most 64 columns, without options");
		a.table = table;
		a.levels = grid->levels;
		a.L = grid->L;
		a.hash_grid = grid->hash_grid ? 1u : 0u;
		a.interp = (uint32_t)grid->interp;
		const uint32_t tb = grid->F * 4u < 16u ? grid->F * 4u : 16u;  // FVec loads, as in launch_f32_mlp_jvp2
		a.vec = (uintptr_t)table % tb == 0 ? 1u : 0u;
		a.hash = (uint32_t)grid->hash;
	} else {
		TCNN_CHECK(D && D <= IN, std::string(what) + ": the input width must lie in [1, encoded width]");
	}
	if (!B) return;
	TCNN_CHECK(params && x && y && jvp && second && keep && (!grid || table),
	           std::string(what) + ": the parameters, the inputs, the output, the product, the second-order sum or the context are missing");
	TCNN_CHECK((uintptr_t)keep % 16 == 0 && (uintptr_t)y % 16 == 0, std::string(what) + ": the context and the output must be 16-byte aligned");
	a.B = B, a.D = D, a.IN = IN, a.NH = NH, a.OUTP = OUTP, a.NOUT = n_out, a.K = n_directions;
	a.P = params, a.X = x, a.V = directions, a.Y = y, a.J = jvp;
	b.Q = second;
	a.act = act, a.oact = out_act;
	a.scale = scale, a.offset = offset;
	const uint32_t F = grid ? grid->F : 0;
	switch (W) {
		case 16: keep2_width<1>(st, b, keep, grid != nullptr, D, F); break;
		case 32: keep2_width<2>(st, b, keep, grid != nullptr, D, F); break;
		default: keep2_width<4>(st, b, keep, grid != nullptr, D, F); break;
	}
	TCNN_HIP_CHECK(hipGetLastError());
}

void launch_f32_mlp_jvp2_bwd_chain(hipStream_t st, uint32_t B, uint32_t IN, uint32_t W, uint32_t NH, uint32_t OUTP, uint32_t n_out, uint32_t K,
                                   const float* params, const float* keep, const float* dL_dy, const float* dL_djvp, const float* dL_dsecond,
                                   float* stack, bool want_d0, int act, int out_act) {
	const char* what = "fp32 forward Laplacian, reverse chain";
	check_jvp2_train_shape(what, B, IN, W, NH, OUTP, n_out, K, act, out_act);
	if (!B) return;
	TCNN_CHECK(params && keep && stack, std::string(what) + ": the parameters, the context or the adjoint stack are missing");
	TCNN_CHECK(dL_dy || dL_djvp || dL_dsecond, std::string(what) + ": dL/dy, dL/dJv and dL/dq are all missing");
	TCNN_CHECK((uintptr_t)keep % 16 == 0 && (uintptr_t)stack % 16 == 0, std::string(what) + ": the context and the stack must be 16-byte aligned");
	Jvp2BwdArgs a{};
	a.B = B, a.IN = IN, a.NH = NH, a.OUTP = OUTP, a.NOUT = n_out;
	a.P = params, a.KEEP = keep, a.DY = dL_dy, a.DJ = dL_djvp, a.DQ = dL_dsecond, a.G = stack;
	a.want_d0 = want_d0 ? 1u : 0u;
	a.act = act, a.oact = out_act;
	switch (W) {
		case 16: bwd2_chain_width<1>(st, a, K); break;
		case 32: bwd2_chain_width<2>(st, a, K); break;
		default: bwd2_chain_width<4>(st, a, K); break;
	}
	TCNN_HIP_CHECK(hipGetLastError());
}

void launch_grid_jvp2_bwd_f32(hipStream_t st, const GridCall& g, uint32_t B, uint32_t K, uint32_t IN, const float* x, const float* directions,
                              const float* t0, float* grad) {
	const char* what = "fp32 grid tangent and second-order gradient";
	TCNN_CHECK(jvp2_train_grid_ok(g, IN),
	           std::string(what) + ": a grid of 2 or 3 input dimensions, 2, 4 or 8 features per level and at most 64 columns, without options");
	TCNN_CHECK(K >= 1 && K <= 3 && (directions || K == g.D), std::string(what) + ": one to three directions, or the unit vectors");
	if (!B || g.interp == Interp::Nearest) return;
	TCNN_CHECK(x && t0 && grad && (uintptr_t)t0 % 16 == 0, std::string(what) + ": the inputs, the adjoints or the table are missing");
	const dim3 blocks(div_round_up(B, 256u), g.L), block(256);
	const uint32_t hash = (uint32_t)g.hash, hg = g.hash_grid ? 1u : 0u, interp = (uint32_t)g.interp;
	switch (g.D * 16 + g.F) {
		case 2 * 16 + 2: hipLaunchKernelGGL((k_grid_jvp2_bwd_f32<2, 2>), blocks, block, 0, st, B, K, IN, x, directions, t0, grad, g.levels, hash, hg, interp); break;
		case 2 * 16 + 4: hipLaunchKernelGGL((k_grid_jvp2_bwd_f32<2, 4>), blocks, block, 0, st, B, K, IN, x, directions, t0, grad, g.levels, hash, hg, interp); break;
		case 2 * 16 + 8: hipLaunchKernelGGL((k_grid_jvp2_bwd_f32<2, 8>), blocks, block, 0, st, B, K, IN, x, directions, t0, grad, g.levels, hash, hg, interp); break;
		case 3 * 16 + 2: hipLaunchKernelGGL((k_grid_jvp2_bwd_f32<3, 2>), blocks, block, 0, st, B, K, IN, x, directions, t0, grad, g.levels, hash, hg, interp); break;
		case 3 * 16 + 4: hipLaunchKernelGGL((k_grid_jvp2_bwd_f32<3, 4>), blocks, block, 0, st, B, K, IN, x, directions, t0, grad, g.levels, hash, hg, interp); break;
		default: hipLaunchKernelGGL((k_grid_jvp2_bwd_f32<3, 8>), blocks, block, 0, st, B, K, IN, x, directions, t0, grad, g.levels, hash, hg, interp); break;
	}
	TCNN_HIP_CHECK(hipGetLastError());
}

}  // namespace tcnn_amd
