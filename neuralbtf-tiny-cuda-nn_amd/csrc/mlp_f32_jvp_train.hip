// mlp_f32_jvp_train.hip -- training through the forward-mode path of an fp32 FullyFusedMLP network module behind a lone
// grid or a lone Identity: the reverse pass of value_and_jvp. Given dL/dy and dL/dJv of a loss L(y, Jv) it produces
// dL/dparams for all outputs and all K directions at once (NetworkF32Host::jvp_forward / jvp_backward,
// tcnn_module_forward_jvp / tcnn_module_backward_jvp). DESIGN.md, "Training through value_and_jvp".
//
// One batch row, layers j = 0..NH, a_j the activation (the output activation for j = NH):
//   value     h_0 = e(x), z_j = W_j h_j, h_{j+1} = a_j(z_j), y = h_{NH+1}
//   tangent k t_{0,k} = (de/dx) v_k, s_{j,k} = W_j t_{j,k}, t_{j+1,k} = phi_j o s_{j,k}, Jv_k = t_{NH+1,k}
// with phi_j = a_j' and psi_j = a_j'' from the stored forward value. The reverse pass starts from hb_{NH+1} = dL/dy and
// tb_{NH+1,k} = dL/dJv_k and runs, for j = NH..0,
//   sb_{j,k} = phi_j o tb_{j+1,k}
//   zb_j     = phi_j o hb_{j+1} + psi_j o sum_k s_{j,k} o tb_{j+1,k}
//   dW_j     = sum_b (zb_j h_j^T + sum_k sb_{j,k} t_{j,k}^T)
//   hb_j     = W_j^T zb_j,  tb_{j,k} = W_j^T sb_{j,k}
//
// Three kernels.
//
// 1. The keeping forward: k_f32_grid_mlp_jvp and k_f32_identity_mlp_jvp (mlp_f32_jvp.hip) again, the same functions in
//    the same order (mlp_f32_jvp_device.h, mlp_f32_chain.h), so y and Jv carry tcnn_module_inference_jvp's bits, plus
//    the stores of a context. K <= TG: one pass. The context, nq = 1 + K:
//      X_0 [nq][B][IN] | X_1 .. X_NH [nq][B][W] each | y [B][OUTP] | S_0 .. S_{NH-1} [K][B][W] each | S_NH [K][B][OUTP]
//    X_j holds h_j and t_{j,1..K}, the input side of layer j; S_j holds s_{j,k}, which only the curvature term reads, and
//    is written (and later read) only when a_j has curvature. Both t and s are stored: t is the weight gradient's
//    operand, and s cannot be had back from t = phi o s where phi rounds to zero. Every store is a 16-byte store of
//    registers the chain holds anyway; these are instantiations of their own, so the inference kernels keep their
//    register allocation.
//
// 2. The reverse chain, k_f32_mlp_jvp_bwd_chain<WT, TG>: one wave owns a 16-row tile and all W columns and carries the
//    1 + TG adjoints (hb, tb_1 .. tb_TG) from the output down to the encoded row in registers. In the operand scheme
//    of mlp_f32_fused.hip the accumulators of W_j^T g are the operands of the next product, and the lane that holds
//    hb_{j+1}[n] holds every tb_{j+1,k}[n], so the gate (phi, psi and the curvature sum) is lane-local. Each weight is
//    loaded once per (k-step, column tile) and used by all 1 + TG adjoints, as jac_from_regs does forward. No LDS, no
//    barrier. It stores zb_j and sb_{j,k} stacked like the context, G_j [nq][B][N_j], and hb_0, tb_{0,k} as
//    [nq][B][IN]. A network without curvature (None, ReLU, LeakyReLU) never touches S: the branch is wave-uniform.
//    With the stacked layout dW_j is ONE product over nq B virtual rows, G_j^T X_j, which the unchanged k_f32_wgrad
//    computes in slabs whose order depends on B and K alone.
//
// 3. The tangent term of the grid's table gradient, k_grid_jvp_bwd_f32<D, F>:
//      dL/dtable[idx_c][f] += sum_d (dw_c/dx_d) G_d[l F + f],   G_d = sum_k v_k[d] tb_{0,k}
//    one thread per (point, level), blockIdx.y the level, so the atomics of one instruction fall on one level's slice
//    of the table. G_d is formed in registers; the corner walk is gather_level_f32's index and weight arithmetic and
//    reads no table value; one fp32 atomic add per corner and feature into a zeroed scratch table. The value term
//    w_c hb_0 goes through the bit-reproducible launch_grid_bwd_f32 on the host side.
#include "grid_dispatch.h"
#include "mlp_f32_jvp_device.h"

namespace tcnn_amd {

namespace {

__device__ __noinline__ float act_factor2_f32_ool(int a, float y) { return act_factor2_f32(a, y); }
// ---- 1: the keeping forward ----

// jac_activate between two rounds of stores: s_{j,k} before the gate (an activation with curvature only), then h_{j+1}
// and t_{j+1,k}
template <int WT, int NQ>
__device__ __forceinline__ void keep_activate(f4 (&h)[NQ][WT], int act, float* __restrict__ S, float* __restrict__ Xn, uint32_t B, uint32_t K,
                                              uint32_t row, uint32_t q) {
	constexpr uint32_t W = 16 * WT;
	if (act_has_curvature(act)) {
#pragma unroll
		for (int i = 1; i < NQ; ++i)
			if ((uint32_t)i <= K)
#pragma unroll
				for (int c = 0; c < WT; ++c) *(f4*)slot(S, B, W, i - 1, row, 16 * c + 4 * q) = h[i][c];
	}
	jac_activate<WT, NQ>(h, act);
#pragma unroll
	for (int i = 0; i < NQ; ++i)
		if ((uint32_t)i <= K)
#pragma unroll
			for (int c = 0; c < WT; ++c) *(f4*)slot(Xn, B, W, i, row, 16 * c + 4 * q) = h[i][c];
}

// jac_chain (mlp_f32_jvp.hip) for one pass with AoS results, writing the context as it goes
template <int WT, int NQ>
__device__ __forceinline__ void keep_chain(f4 (&h)[NQ][WT], const JvpArgs& a, const KeepLayout& kl, float* __restrict__ keep, uint32_t r,
                                           uint32_t q, uint32_t row) {
	constexpr uint32_t W = 16 * WT;
	const uint32_t nt = (a.NOUT + 15) / 16, K = a.K, B = a.B;
	const float* wl = a.P + (size_t)W * a.IN;
	keep_activate<WT, NQ>(h, a.act, keep + kl.s(0), keep + kl.x(1), B, K, row, q);
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
		keep_activate<WT, NQ>(h, a.act, keep + kl.s(l), keep + kl.x(l + 1), B, K, row, q);
	}
	const bool ocurv = act_has_curvature(a.oact);
	float* SN = keep + kl.s(a.NH);
	for (uint32_t c0 = 0; c0 < nt; ++c0) {
		f4 o[NQ][1];
#pragma unroll
		for (int i = 0; i < NQ; ++i) o[i][0] = f4{0.0f, 0.0f, 0.0f, 0.0f};
		jac_from_regs<WT, NQ, 1>(wl + (size_t)(16 * c0 + r) * W + 4 * q, 1, h, o);
		const uint32_t n0 = 16 * c0 + 4 * q;
		if (ocurv) {
#pragma unroll
			for (int i = 1; i < NQ; ++i)
				if ((uint32_t)i <= K) *(f4*)slot(SN, B, a.OUTP, i - 1, row, n0) = o[i][0];
		}
		if (a.oact != ACT_NONE) {
#pragma unroll
			for (int e = 0; e < 4; ++e) {
				const float y = fwd_act(a.oact, o[0][0][e]);
				const float f = bwd_act(a.oact, 1.0f, y);
				o[0][0][e] = y;
#pragma unroll
				for (int i = 1; i < NQ; ++i) o[i][0][e] *= f;
			}
		}
		*(f4*)(a.Y + (size_t)row * a.OUTP + n0) = o[0][0];
		*(f4*)(keep + kl.y() + (size_t)row * a.OUTP + n0) = o[0][0];
		float* je = a.J + ((size_t)row * a.NOUT + n0) * K;
#pragma unroll
		for (int e = 0; e < 4; ++e, je += K) {
			if (n0 + e < a.NOUT) {
#pragma unroll
				for (int i = 1; i < NQ; ++i)
					if ((uint32_t)(i - 1) < K) je[i - 1] = o[i][0][e];
			}
		}
	}
}

// Grid B / 64, K <= TG. k_f32_grid_mlp_jvp's single pass with the stores of the context.
template <int WT, uint32_t D, uint32_t F>
__global__ __launch_bounds__(256) void k_f32_grid_mlp_jvp_keep(const JvpArgs a, float* __restrict__ keep) {
	constexpr uint32_t W = 16 * WT;
	constexpr int TG = jvp_tangents(WT), NQ = 1 + TG;
	const uint32_t lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;
	const uint32_t row = (blockIdx.x * 4 + (threadIdx.x >> 6)) * JAC_ROWS_PER_WAVE + r;
	if (row >= a.B) return;
	const KeepLayout kl{a.B, 1 + (size_t)a.K, a.IN, W, a.NH, a.OUTP};
	float x[D];
#pragma unroll
	for (uint32_t d = 0; d < D; ++d) x[d] = a.X[(size_t)row * D + d];
	uint32_t prime[D];
	hash_primes<D>((HashType)a.hash, prime);
	const uint32_t ks = a.IN / 16;
	float dir[TG][D];
#pragma unroll
	for (int i = 0; i < TG; ++i)
#pragma unroll
		for (uint32_t d = 0; d < D; ++d) dir[i][d] = a.V && (uint32_t)i < a.K ? a.V[((size_t)row * a.K + i) * D + d] : 0.0f;
	f4 e[NQ][JVP_MAX_KSTEPS];
#pragma unroll
	for (uint32_t s = 0; s < JVP_MAX_KSTEPS; ++s) {
		if (s < ks) {
			f4 es[NQ];
			jvp_encode_step<D, F, NQ>(a, s, q, 0, x, dir, prime, es);
#pragma unroll
			for (int i = 0; i < NQ; ++i) {
				e[i][s] = es[i];
				if ((uint32_t)i <= a.K) *(f4*)slot(keep, a.B, a.IN, i, row, 16 * s + 4 * q) = es[i];
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
	keep_chain<WT, NQ>(h, a, kl, keep, r, q, row);
}

// The same behind an Identity row. The first layer's tangents need no contraction (jac_identity_layer), but the weight
// gradient needs their operand: t_{0,k} = scale v_k on the D input columns (scale on column k for the unit vectors),
// zero on the padding, stored beside the row x scale + offset, 1.
template <int WT>
__global__ __launch_bounds__(256) void k_f32_identity_mlp_jvp_keep(const JvpArgs a, float* __restrict__ keep) {
	constexpr uint32_t W = 16 * WT;
	constexpr int TG = jvp_tangents(WT), NQ = 1 + TG;
	const uint32_t lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;
	const uint32_t row = (blockIdx.x * 4 + (threadIdx.x >> 6)) * JAC_ROWS_PER_WAVE + r;
	if (row >= a.B) return;
	const KeepLayout kl{a.B, 1 + (size_t)a.K, a.IN, W, a.NH, a.OUTP};
	for (uint32_t s = 0; s < a.IN; s += 16) {
		f4 v[NQ];
#pragma unroll
		for (int j = 0; j < 4; ++j) {
			const uint32_t k = s + 4 * q + j;
			v[0][j] = k < a.D ? __builtin_fmaf(a.X[(size_t)row * a.D + k], a.scale, a.offset) : 1.0f;
#pragma unroll
			for (int i = 1; i < NQ; ++i) {
				float t = 0.0f;
				if (k < a.D && (uint32_t)i <= a.K) t = a.V ? a.scale * a.V[((size_t)row * a.K + (i - 1)) * a.D + k] : (k == (uint32_t)(i - 1) ? a.scale : 0.0f);
				v[i][j] = t;
			}
		}
#pragma unroll
		for (int i = 0; i < NQ; ++i)
			if ((uint32_t)i <= a.K) *(f4*)slot(keep, a.B, a.IN, i, row, s + 4 * q) = v[i];
	}
	f4 h[NQ][WT];
	jac_identity_layer<WT, NQ>(h, a.P, a.X, false, a.V, a.B, a.D, a.K, a.IN, a.scale, a.offset, r, q, row, 0);
	keep_chain<WT, NQ>(h, a, kl, keep, r, q, row);
}

template <int WT>
void keep_width(hipStream_t st, const JvpArgs& a, float* keep, bool grid, uint32_t D, uint32_t F) {
	const dim3 blocks(a.B / JAC_ROWS_PER_BLOCK), block(256);
	if (!grid) {
		hipLaunchKernelGGL((k_f32_identity_mlp_jvp_keep<WT>), blocks, block, 0, st, a, keep);
		return;
	}
	switch (D * 16 + F) {
		case 2 * 16 + 2: hipLaunchKernelGGL((k_f32_grid_mlp_jvp_keep<WT, 2, 2>), blocks, block, 0, st, a, keep); break;
		case 2 * 16 + 4: hipLaunchKernelGGL((k_f32_grid_mlp_jvp_keep<WT, 2, 4>), blocks, block, 0, st, a, keep); break;
		case 2 * 16 + 8: hipLaunchKernelGGL((k_f32_grid_mlp_jvp_keep<WT, 2, 8>), blocks, block, 0, st, a, keep); break;
		case 3 * 16 + 2: hipLaunchKernelGGL((k_f32_grid_mlp_jvp_keep<WT, 3, 2>), blocks, block, 0, st, a, keep); break;
		case 3 * 16 + 4: hipLaunchKernelGGL((k_f32_grid_mlp_jvp_keep<WT, 3, 4>), blocks, block, 0, st, a, keep); break;
		default: hipLaunchKernelGGL((k_f32_grid_mlp_jvp_keep<WT, 3, 8>), blocks, block, 0, st, a, keep); break;
	}
}

// ---- 2: the reverse chain ----

struct JvpBwdArgs {
	uint32_t B, IN, NH, OUTP, NOUT;
	const float* P;     // [W0 | W1 .. W_{NH-1} | Wout]
	const float* KEEP;  // the keeping forward's context
	const float* DY;    // dL/dy [B][OUTP], nullable: zero; columns past NOUT count as zero
	const float* DJ;    // dL/dJv [B][NOUT][TG], nullable: zero
	float* G;           // [G_0 .. G_NH | hb_0, tb_0], KeepLayout::g / d0
	uint32_t want_d0;   // the encoding in front has parameters
	int act, oact;
};

// The gate of one layer on the lane's four neurons: g[0] = hb, g[i] = tb_i come in, zb and sb_i go out.
//   sb_i = phi tb_i,  zb = phi hb + psi sum_i s_i tb_i
// the sum in ascending i, one FMA per term after the first, and one FMA for psi (sum) + phi hb. yv: the layer's forward
// value; sv: s_i of the context, read only when the activation has curvature.
template <int NQ>
__device__ __forceinline__ void jvp_gate(int act, bool curv, const f4& yv, const f4 (&sv)[NQ], f4 (&g)[NQ]) {
	if (act == ACT_NONE) return;
#pragma unroll
	for (int e = 0; e < 4; ++e) {
		const float phi = bwd_act(act, 1.0f, yv[e]);
		float z = phi * g[0][e];
		if (curv) {
			float acc = sv[1][e] * g[1][e];
#pragma unroll
			for (int i = 2; i < NQ; ++i) acc = __builtin_fmaf(sv[i][e], g[i][e], acc);
			z = __builtin_fmaf(act_factor2_f32_ool(act, yv[e]), acc, z);
		}
		g[0][e] = z;
#pragma unroll
		for (int i = 1; i < NQ; ++i) g[i][e] *= phi;
	}
}

// Grid B / 64. TG is the call's K: every quantity is live, nothing is guarded.
template <int WT, int TG>
__global__ __launch_bounds__(256) void k_f32_mlp_jvp_bwd_chain(const JvpBwdArgs a) {
	constexpr uint32_t W = 16 * WT;
	constexpr int NQ = 1 + TG;
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
			f4 g[NQ], sv[NQ];
#pragma unroll
			for (int j = 0; j < 4; ++j) {
				const bool in = n0 + j < a.NOUT;
				g[0][j] = a.DY && in ? a.DY[(size_t)row * a.OUTP + n0 + j] : 0.0f;
#pragma unroll
				for (int i = 1; i < NQ; ++i) g[i][j] = a.DJ && in ? a.DJ[((size_t)row * a.NOUT + n0 + j) * TG + (i - 1)] : 0.0f;
			}
			if (a.oact != ACT_NONE) {
				if (ocurv)
#pragma unroll
					for (int i = 1; i < NQ; ++i) sv[i] = *(const f4*)(SN + ((size_t)(i - 1) * B + row) * a.OUTP + n0);
				jvp_gate<NQ>(a.oact, ocurv, *(const f4*)(Yv + n0), sv, g);
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
	for (uint32_t l = a.NH; l-- > 0;) {  // d = hb_{l+1}, tb_{l+1,.}: gate with layer l's activation, store, go down
		const float* Hn = a.KEEP + kl.x(l + 1) + (size_t)row * W + 4 * q;  // h_{l+1}: quantity 0 of X_{l+1}
		const float* Sl = a.KEEP + kl.s(l) + (size_t)row * W + 4 * q;
		float* Gl = a.G + kl.g(l) + (size_t)row * W + 4 * q;
#pragma unroll
		for (int c = 0; c < WT; ++c) {
			f4 g[NQ], sv[NQ];
#pragma unroll
			for (int i = 0; i < NQ; ++i) g[i] = d[i][c];
			if (a.act != ACT_NONE) {
				if (curv)
#pragma unroll
					for (int i = 1; i < NQ; ++i) sv[i] = *(const f4*)(Sl + (size_t)(i - 1) * B * W + 16 * c);
				jvp_gate<NQ>(a.act, curv, *(const f4*)(Hn + 16 * c), sv, g);
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
	// first layer: hb_0 and tb_{0,.}, one column tile of the encoded row at a time, each a full contraction from d
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

template <int WT, int TG>
void bwd_chain_launch(hipStream_t st, const JvpBwdArgs& a) {
	hipLaunchKernelGGL((k_f32_mlp_jvp_bwd_chain<WT, TG>), dim3(a.B / JAC_ROWS_PER_BLOCK), dim3(256), 0, st, a);
}

template <int WT>
void bwd_chain_width(hipStream_t st, const JvpBwdArgs& a, uint32_t K) {
	if constexpr (WT == 8) {
		bwd_chain_launch<WT, 1>(st, a);
	} else {
		if (K == 1) bwd_chain_launch<WT, 1>(st, a);
		else if (K == 2) bwd_chain_launch<WT, 2>(st, a);
		else bwd_chain_launch<WT, 3>(st, a);
	}
}

// ---- 3: the tangent term of the table gradient ----

// Grid (B / 256, L). X [B][D]; V [B][K][D], null: the D unit vectors (K = D); T0 = tb_{0,k} as [K][B][IN]; grad: the
// zeroed scratch table. Linear and Smoothstep only (Nearest has no tangent term: the host does not launch).
template <uint32_t D, uint32_t F>
__global__ __launch_bounds__(256) void k_grid_jvp_bwd_f32(uint32_t B, uint32_t K, uint32_t IN, const float* __restrict__ X,
                                                          const float* __restrict__ V, const float* __restrict__ T0, float* __restrict__ grad,
                                                          const LevelInfo* __restrict__ levels, uint32_t hash, uint32_t hash_grid,
                                                          uint32_t interp_u) {
	const uint32_t b = blockIdx.x * 256 + threadIdx.x, l = blockIdx.y;
	if (b >= B) return;
	const LevelInfo li = levels[l];
	uint32_t prime[D];
	hash_primes<D>((HashType)hash, prime);
	float p[D], pd[D];
	uint32_t pg[D];
#pragma unroll
	for (uint32_t d = 0; d < D; ++d) pos_fract_d(X[(size_t)b * D + d], li.scale, (Interp)interp_u, p[d], pd[d], pg[d]);
	// G_d = sum_k v_k[d] tb_{0,k}, in ascending k, one FMA per term after the first; the unit vectors select
	float G[D][F];
#pragma unroll
	for (uint32_t d = 0; d < D; ++d)
#pragma unroll
		for (uint32_t f = 0; f < F; ++f) G[d][f] = 0.0f;
#pragma unroll
	for (uint32_t k = 0; k < 3; ++k) {
		if (k < K) {
			const FVec<F> t = load_fvec<F>(T0 + ((size_t)k * B + b) * IN + l * F, true);
#pragma unroll
			for (uint32_t d = 0; d < D; ++d) {
				if (V) {
					const float v = V[((size_t)b * K + k) * D + d];
#pragma unroll
					for (uint32_t f = 0; f < F; ++f) G[d][f] = k ? __builtin_fmaf(v, t.v[f], G[d][f]) : v * t.v[f];
				} else if (d == k) {
#pragma unroll
					for (uint32_t f = 0; f < F; ++f) G[d][f] = t.v[f];
				}
			}
		}
	}
#pragma unroll
	for (uint32_t c = 0; c < (1u << D); ++c) {
		uint32_t local[D];
		float w[D];
#pragma unroll
		for (uint32_t d = 0; d < D; ++d) {
			const bool hi = (c >> d) & 1u;
			local[d] = pg[d] + (hi ? 1u : 0u);
			w[d] = hi ? p[d] : 1.0f - p[d];
		}
		float* entry = grad + (size_t)(li.offset + grid_index_primes<D>(hash_grid != 0, li.size, li.res, local, prime)) * F;
		// dw_c / dx_d = scale pd_d (+-1) prod_{d' != d} w_d', the product from the scale on as level_tangent_f32 forms it
		float a[D];
#pragma unroll
		for (uint32_t d = 0; d < D; ++d) {
			float pe = li.scale;
#pragma unroll
			for (uint32_t o = 0; o < D; ++o)
				if (o != d) pe *= w[o];
			pe *= pd[d];
			a[d] = (c >> d) & 1u ? pe : -pe;
		}
#pragma unroll
		for (uint32_t f = 0; f < F; ++f) {
			float v = a[0] * G[0][f];
#pragma unroll
			for (uint32_t d = 1; d < D; ++d) v = __builtin_fmaf(a[d], G[d][f], v);
			unsafeAtomicAdd(entry + f, v);
		}
	}
}

}  // namespace

uint32_t f32_mlp_jvp_train_max_directions(uint32_t W) { return W == 128 ? 1u : 3u; }

size_t f32_mlp_jvp_keep_floats(uint32_t B, uint32_t K, uint32_t IN, uint32_t W, uint32_t NH, uint32_t OUTP) {
	return KeepLayout{B, 1 + (size_t)K, IN, W, NH, OUTP}.total();
}

size_t f32_mlp_jvp_stack_floats(uint32_t B, uint32_t K, uint32_t IN, uint32_t W, uint32_t NH, uint32_t OUTP) {
	return KeepLayout{B, 1 + (size_t)K, IN, W, NH, OUTP}.stack_total();
}

size_t f32_mlp_jvp_keep_x(uint32_t B, uint32_t K, uint32_t IN, uint32_t W, uint32_t NH, uint32_t OUTP, uint32_t j) {
	return KeepLayout{B, 1 + (size_t)K, IN, W, NH, OUTP}.x(j);
}

size_t f32_mlp_jvp_stack_g(uint32_t B, uint32_t K, uint32_t IN, uint32_t W, uint32_t NH, uint32_t OUTP, uint32_t j) {
	const KeepLayout kl{B, 1 + (size_t)K, IN, W, NH, OUTP};
	return j <= NH ? kl.g(j) : kl.d0();
}

namespace {

void check_jvp_train_shape(const char* what, uint32_t B, uint32_t IN, uint32_t W, uint32_t NH, uint32_t OUTP, uint32_t n_out, uint32_t K, int act,
                           int out_act) {
	TCNN_CHECK(f32_mlp_fused_width_ok(W), std::string(what) + ": the width must be 16, 32, 64 or 128");
	TCNN_CHECK(NH >= 1, std::string(what) + ": at least one hidden layer");
	TCNN_CHECK(IN && OUTP && IN % 16 == 0 && OUTP % 16 == 0, std::string(what) + ": widths must be multiples of 16");
	TCNN_CHECK(B % 256 == 0, std::string(what) + ": batch must be a multiple of 256");
	TCNN_CHECK(n_out && n_out <= OUTP && OUTP - n_out < 16, std::string(what) + ": the padded output width must be the next multiple of 16");
	TCNN_CHECK(act != ACT_SINE && out_act != ACT_SINE, std::string(what) + ": Sine has no backward from its forward value");
	TCNN_CHECK(K >= 1 && K <= f32_mlp_jvp_train_max_directions(W),
	           std::string(what) + ": " + std::to_string(K) + " directions at width " + std::to_string(W) + " (at most " +
	               std::to_string(f32_mlp_jvp_train_max_directions(W)) + " are served)");
}

}  // namespace

void launch_f32_mlp_jvp_keep(hipStream_t st, uint32_t B, uint32_t D, uint32_t IN, uint32_t W, uint32_t NH, uint32_t OUTP, uint32_t n_out,
                             const float* params, const float* x, const float* directions, uint32_t n_directions, float* y, float* jvp,
                             int act, int out_act, const GridCall* grid, const float* table, float scale, float offset, float* keep) {
	const char* what = "fp32 Jacobian-vector product, keeping forward";
	check_jvp_train_shape(what, B, IN, W, NH, OUTP, n_out, n_directions, act, out_act);
	TCNN_CHECK(directions || n_directions == D, std::string(what) + ": null directions are the unit vectors, as many as inputs");
	JvpArgs a{};
	if (grid) {
		TCNN_CHECK(grid->D == D && f32_mlp_jvp_grid_ok(D, grid->F, IN) && grid->L && grid->L * grid->F <= IN && !grid->opts.active,
		           std::string(what) + ": a grid of 2 or 3 input dimensions, 2, 4 or 8 features per level and at most 64 columns, without options");
		a.table = table;
		a.levels = grid->levels;
		a.L = grid->L;
		a.hash_grid = grid->hash_grid ? 1u : 0u;
		a.interp = (uint32_t)grid->interp;
		const uint32_t tb = grid->F * 4u < 16u ? grid->F * 4u : 16u;
		a.vec = (uintptr_t)table % tb == 0 ? 1u : 0u;
		a.hash = (uint32_t)grid->hash;
	} else {
		TCNN_CHECK(D && D <= IN, std::string(what) + ": the input width must lie in [1, encoded width]");
	}
	if (!B) return;
	TCNN_CHECK(params && x && y && jvp && keep && (!grid || table),
	           std::string(what) + ": the parameters, the inputs, the output, the product or the context are missing");
	TCNN_CHECK((uintptr_t)keep % 16 == 0 && (uintptr_t)y % 16 == 0, std::string(what) + ": the context and the output must be 16-byte aligned");
	a.B = B, a.D = D, a.IN = IN, a.NH = NH, a.OUTP = OUTP, a.NOUT = n_out, a.K = n_directions;
	a.P = params, a.X = x, a.V = directions, a.Y = y, a.J = jvp;
	a.act = act, a.oact = out_act;
	a.scale = scale, a.offset = offset;
	const uint32_t F = grid ? grid->F : 0;
	switch (W) {
		case 16: keep_width<1>(st, a, keep, grid != nullptr, D, F); break;
		case 32: keep_width<2>(st, a, keep, grid != nullptr, D, F); break;
		case 64: keep_width<4>(st, a, keep, grid != nullptr, D, F); break;
		default: keep_width<8>(st, a, keep, grid != nullptr, D, F); break;
	}
	TCNN_HIP_CHECK(hipGetLastError());
}

void launch_f32_mlp_jvp_bwd_chain(hipStream_t st, uint32_t B, uint32_t IN, uint32_t W, uint32_t NH, uint32_t OUTP, uint32_t n_out, uint32_t K,
                                  const float* params, const float* keep, const float* dL_dy, const float* dL_djvp, float* stack, bool want_d0,
                                  int act, int out_act) {
	const char* what = "fp32 Jacobian-vector product, reverse chain";
	check_jvp_train_shape(what, B, IN, W, NH, OUTP, n_out, K, act, out_act);
	if (!B) return;
	TCNN_CHECK(params && keep && stack, std::string(what) + ": the parameters, the context or the adjoint stack are missing");
	TCNN_CHECK(dL_dy || dL_djvp, std::string(what) + ": dL/dy and dL/dJv are both missing");
	TCNN_CHECK((uintptr_t)keep % 16 == 0 && (uintptr_t)stack % 16 == 0, std::string(what) + ": the context and the stack must be 16-byte aligned");
	JvpBwdArgs a{};
	a.B = B, a.IN = IN, a.NH = NH, a.OUTP = OUTP, a.NOUT = n_out;
	a.P = params, a.KEEP = keep, a.DY = dL_dy, a.DJ = dL_djvp, a.G = stack;
	a.want_d0 = want_d0 ? 1u : 0u;
	a.act = act, a.oact = out_act;
	switch (W) {
		case 16: bwd_chain_width<1>(st, a, K); break;
		case 32: bwd_chain_width<2>(st, a, K); break;
		case 64: bwd_chain_width<4>(st, a, K); break;
		default: bwd_chain_width<8>(st, a, K); break;
	}
	TCNN_HIP_CHECK(hipGetLastError());
}

void launch_grid_jvp_bwd_f32(hipStream_t st, const GridCall& g, uint32_t B, uint32_t K, uint32_t IN, const float* x, const float* directions,
                             const float* t0, float* grad) {
	const char* what = "fp32 grid tangent gradient";
	TCNN_CHECK(f32_mlp_jvp_grid_ok(g.D, g.F, IN) && g.L * g.F <= IN && !g.opts.active,
	           std::string(what) + ": a grid of 2 or 3 input dimensions, 2, 4 or 8 features per level and at most 64 columns, without options");
	TCNN_CHECK(K >= 1 && K <= 3 && (directions || K == g.D), std::string(what) + ": one to three directions, or the unit vectors");
	if (!B || g.interp == Interp::Nearest) return;
	TCNN_CHECK(x && t0 && grad && (uintptr_t)t0 % 16 == 0, std::string(what) + ": the inputs, the adjoints or the table are missing");
	const dim3 blocks(div_round_up(B, 256u), g.L), block(256);
	const uint32_t hash = (uint32_t)g.hash, hg = g.hash_grid ? 1u : 0u, interp = (uint32_t)g.interp;
	switch (g.D * 16 + g.F) {
		case 2 * 16 + 2: hipLaunchKernelGGL((k_grid_jvp_bwd_f32<2, 2>), blocks, block, 0, st, B, K, IN, x, directions, t0, grad, g.levels, hash, hg, interp); break;
		case 2 * 16 + 4: hipLaunchKernelGGL((k_grid_jvp_bwd_f32<2, 4>), blocks, block, 0, st, B, K, IN, x, directions, t0, grad, g.levels, hash, hg, interp); break;
		case 2 * 16 + 8: hipLaunchKernelGGL((k_grid_jvp_bwd_f32<2, 8>), blocks, block, 0, st, B, K, IN, x, directions, t0, grad, g.levels, hash, hg, interp); break;
		case 3 * 16 + 2: hipLaunchKernelGGL((k_grid_jvp_bwd_f32<3, 2>), blocks, block, 0, st, B, K, IN, x, directions, t0, grad, g.levels, hash, hg, interp); break;
		case 3 * 16 + 4: hipLaunchKernelGGL((k_grid_jvp_bwd_f32<3, 4>), blocks, block, 0, st, B, K, IN, x, directions, t0, grad, g.levels, hash, hg, interp); break;
		default: hipLaunchKernelGGL((k_grid_jvp_bwd_f32<3, 8>), blocks, block, 0, st, B, K, IN, x, directions, t0, grad, g.levels, hash, hg, interp); break;
	}
	TCNN_HIP_CHECK(hipGetLastError());
}

}  // namespace tcnn_amd
