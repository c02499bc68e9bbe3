// mlp_f32_jacobian.hip -- the value f(x) and the input Jacobian df/dx of an fp32 FullyFusedMLP network module behind
// an Identity encoding, in one forward-mode launch (NetworkF32Host::jacobian, tcnn_module_inference_jacobian).
//
// Forward mode in the register chain of mlp_f32_fused.hip. A tangent T_d = dh/dx_d has the shape of h and goes through
// the same matrices: n = W h, T_d <- W T_d, then h = act(n), T_d <- act'(h) o T_d. In the operand scheme of that file
// lane (r = l & 15, q = l >> 4) holds neuron 16 c + 4 q + e of batch row row0 + r as acc[c][e], and the activated
// accumulators of a layer are the operand registers of the next. The lane that holds h[c][e] therefore also holds
// every tangent element it must scale by act'(h[c][e]): the value and TG tangents of a wave's rows run through the
// whole network out of registers. No LDS, no shuffle, no barrier, nothing kept: HBM sees D floats in and
// n_out (1 + D) floats out per sample.
//
// Work split. A wave owns ONE 16-row tile x WT = W / 16 column tiles, and carries the value and TG tangents through it:
// (1 + TG) WT independent accumulators per k-step, which is what the MFMA's dependent-accumulator latency asks for
// (the forward kernel gets them from its second row tile). Every weight f4 is loaded once per (column tile, k-step)
// and used by all 1 + TG quantities. Four waves to a workgroup, 64 rows. An input wider than TG runs
// ceil(D / TG) passes inside the launch; each pass recomputes the value chain (the tangents need act'(h) of every
// layer) and the first stores y. TG per width comes from the compiler's resource report ("Input Jacobian
// of fp32 network modules"): no instantiation uses scratch.
//
// First layer. The value is the K-loop of k_f32_mlp_fwd over the Identity row x scale + offset (ones on the padding
// columns), k-steps ascending and j = 0..3 into one accumulator per element: with the hidden and output products in
// that same order, y carries the bits of tcnn_module_inference. The tangents need no contraction: the pre-activation
// tangent of input d is scale W0[n][d], one load per element.
//
// Layouts, chosen at compile time: x is AoS [B][D] or SoA [D][B]; y is AoS [B][OUTP] rows as the forward writes them
// with J [B][n_out][D], or SoA [n_out][B] with J [n_out D][B] (row o D + d). For a fixed neuron the 16 lanes of a
// quarter hold 16 consecutive batch rows, so every SoA access covers 64-byte runs. J exists only for o < n_out and
// d < D: nothing past those is stored.
#include "mlp_f32_chain.h"

namespace tcnn_amd {

namespace {

// P = [W0 [W][IN] | W1 .. W_{NH-1} [W][W] | Wout [OUTP][W]]; X the caller's inputs, D of them per sample, the Identity
// row being x scale + offset then ones up to IN. Y and J as above. Grid B / 64.
template <int WT, int TG, bool XS, bool YS>
__global__ __launch_bounds__(256) void k_f32_mlp_jacobian(uint32_t B, uint32_t D, uint32_t IN, uint32_t NH, uint32_t OUTP, uint32_t NOUT,
                                                           const float* __restrict__ P, const float* __restrict__ X, float scale, float offset,
                                                           float* __restrict__ Y, float* __restrict__ J, int act, int oact) {
	constexpr uint32_t W = 16 * WT;
	constexpr int NQ = 1 + TG;  // quantity 0 is the value, 1 .. TG the tangents of inputs d0 .. d0 + TG - 1
	const uint32_t lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;
	const uint32_t row = (blockIdx.x * 4 + (threadIdx.x >> 6)) * JAC_ROWS_PER_WAVE + r;
	if (row >= B) return;
	const uint32_t nt = (NOUT + 15) / 16;  // = OUTP / 16: the padded width is the next multiple of 16
	for (uint32_t d0 = 0; d0 < D; d0 += TG) {
		f4 h[NQ][WT];
#pragma unroll
		for (int c = 0; c < WT; ++c) h[0][c] = f4{0.0f, 0.0f, 0.0f, 0.0f};
		{  // first layer, value: the K-loop of k_f32_mlp_fwd over the Identity row
			const float* wp = P + (size_t)r * IN + 4 * q;
			for (uint32_t s = 0; s < IN; s += 16) {
				f4 a;
#pragma unroll
				for (int j = 0; j < 4; ++j) {
					const uint32_t k = s + 4 * q + j;
					a[j] = 1.0f;
					if (k < D) a[j] = __builtin_fmaf(XS ? X[(size_t)k * B + row] : X[(size_t)row * D + k], scale, offset);
				}
#pragma unroll
				for (int c = 0; c < WT; ++c) {
					const f4 w = *(const f4*)(wp + (size_t)c * 16 * IN + s);
#pragma unroll
					for (int j = 0; j < 4; ++j) h[0][c] = mfma4(w[j], a[j], h[0][c]);
				}
			}
		}
		{  // first layer, tangents: d(pre-activation of neuron n) / dx_d = scale W0[n][d], zero past D
			const float* wn = P + (size_t)(4 * q) * IN + d0;
#pragma unroll
			for (int i = 1; i < NQ; ++i) {
				const bool in = d0 + (i - 1) < D;
#pragma unroll
				for (int c = 0; c < WT; ++c)
#pragma unroll
					for (int e = 0; e < 4; ++e) h[i][c][e] = in ? scale * wn[(size_t)(16 * c + e) * IN + (i - 1)] : 0.0f;
			}
		}
		jac_activate<WT, NQ>(h, act);
		const float* wl = P + (size_t)W * IN;
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
			jac_activate<WT, NQ>(h, act);
		}
		// output layer: one column tile at a time, each a full contraction from h and the tangents. The forward's groups
		// of four would keep 16 (1 + TG) more accumulators live across the out-of-line activation calls, which the
		// resource report answers with scratch at W 64; the 1 + TG quantities still give independent chains.
		for (uint32_t c0 = 0; c0 < nt; ++c0) {
			f4 o[NQ][1];
#pragma unroll
			for (int i = 0; i < NQ; ++i) o[i][0] = f4{0.0f, 0.0f, 0.0f, 0.0f};
			jac_from_regs<WT, NQ, 1>(wl + (size_t)(16 * c0 + r) * W + 4 * q, 1, h, o);
			const uint32_t n0 = 16 * c0 + 4 * q;
			// y = oact(o) and J = oact'(y) o (Wout T_d) in place, outside the lane-dependent guards of the stores
			if (oact != ACT_NONE) {
#pragma unroll
				for (int e = 0; e < 4; ++e) {
					const float y = fwd_act(oact, o[0][0][e]);
					const float f = bwd_act(oact, 1.0f, y);
					o[0][0][e] = y;
#pragma unroll
					for (int i = 1; i < NQ; ++i) o[i][0][e] *= f;
				}
			}
			if (d0 == 0) {  // the first pass stores y
				if constexpr (YS) {
#pragma unroll
					for (int e = 0; e < 4; ++e)
						if (n0 + e < NOUT) Y[(size_t)(n0 + e) * B + row] = o[0][0][e];
				} else {
					*(f4*)(Y + (size_t)row * OUTP + n0) = o[0][0];
				}
			}
			// J[.][n0 + e][d0 + i - 1]: one running pointer, stepped by the element strides of o and d
			const size_t so = YS ? (size_t)D * B : D, sd = YS ? B : 1;
			float* je = J + (YS ? ((size_t)n0 * D + d0) * B + row : ((size_t)row * NOUT + n0) * D + d0);
#pragma unroll
			for (int e = 0; e < 4; ++e, je += so) {
				if (n0 + e < NOUT) {
					float* ji = je;
#pragma unroll
					for (int i = 1; i < NQ; ++i, ji += sd)
						if (d0 + (i - 1) < D) *ji = o[i][0][e];
				}
			}
		}
	}
}

template <int WT, int TG>
void jacobian_layout(hipStream_t st, uint32_t B, uint32_t D, uint32_t IN, uint32_t NH, uint32_t OUTP, uint32_t n_out, const float* p,
                     const float* x, bool x_soa, float scale, float offset, float* y, float* j, bool y_soa, int act, int oact) {
	const dim3 grid(B / JAC_ROWS_PER_BLOCK), block(256);
	if (x_soa && y_soa) hipLaunchKernelGGL((k_f32_mlp_jacobian<WT, TG, true, true>), grid, block, 0, st, B, D, IN, NH, OUTP, n_out, p, x, scale, offset, y, j, act, oact);
	else if (x_soa) hipLaunchKernelGGL((k_f32_mlp_jacobian<WT, TG, true, false>), grid, block, 0, st, B, D, IN, NH, OUTP, n_out, p, x, scale, offset, y, j, act, oact);
	else if (y_soa) hipLaunchKernelGGL((k_f32_mlp_jacobian<WT, TG, false, true>), grid, block, 0, st, B, D, IN, NH, OUTP, n_out, p, x, scale, offset, y, j, act, oact);
	else hipLaunchKernelGGL((k_f32_mlp_jacobian<WT, TG, false, false>), grid, block, 0, st, B, D, IN, NH, OUTP, n_out, p, x, scale, offset, y, j, act, oact);
}

}  // namespace

void launch_f32_mlp_jacobian(hipStream_t st, uint32_t B, uint32_t D, uint32_t IN, uint32_t W, uint32_t NH, uint32_t OUTP, uint32_t n_out,
                             const float* params, const float* x, bool x_soa, float scale, float offset, float* y, float* jac, bool y_soa,
                             int act, int out_act) {
	const char* what = "fp32 input Jacobian";
	TCNN_CHECK(f32_mlp_fused_width_ok(W), std::string(what) + ": the width must be 16, 32, 64 or 128");
	TCNN_CHECK(NH >= 1, std::string(what) + ": at least one hidden layer");
	TCNN_CHECK(IN && OUTP && IN % 16 == 0 && OUTP % 16 == 0, std::string(what) + ": widths must be multiples of 16");
	TCNN_CHECK(B % 128 == 0, std::string(what) + ": batch must be a multiple of 128");
	TCNN_CHECK(D && D <= IN, std::string(what) + ": the input width must lie in [1, encoded width]");
	TCNN_CHECK(n_out && n_out <= OUTP && OUTP - n_out < 16, std::string(what) + ": the padded output width must be the next multiple of 16");
	TCNN_CHECK(act != ACT_SINE && out_act != ACT_SINE, std::string(what) + ": Sine has no backward from its forward value");
	if (!B) return;
	TCNN_CHECK(params && x && y && jac, std::string(what) + ": the parameters, the inputs, the output or the Jacobian are missing");
	// tangents per pass, from the resource report: the widest group that keeps W 128 within the register file
	switch (W) {
		case 16: jacobian_layout<1, 3>(st, B, D, IN, NH, OUTP, n_out, params, x, x_soa, scale, offset, y, jac, y_soa, act, out_act); break;
		case 32: jacobian_layout<2, 3>(st, B, D, IN, NH, OUTP, n_out, params, x, x_soa, scale, offset, y, jac, y_soa, act, out_act); break;
		case 64: jacobian_layout<4, 3>(st, B, D, IN, NH, OUTP, n_out, params, x, x_soa, scale, offset, y, jac, y_soa, act, out_act); break;
		default: jacobian_layout<8, 1>(st, B, D, IN, NH, OUTP, n_out, params, x, x_soa, scale, offset, y, jac, y_soa, act, out_act); break;
	}
	TCNN_HIP_CHECK(hipGetLastError());
}

}  // namespace tcnn_amd
