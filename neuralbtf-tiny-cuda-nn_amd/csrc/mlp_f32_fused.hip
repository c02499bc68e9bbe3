// mlp_f32_fused.hip -- the whole fp32 MLP in one launch (an fp32 network module with "otype": "FullyFusedMLP",
// NH >= 1, W in {16, 32, 64, 128}): the forward, and the backward's delta chain D_{NH+1} = dL/dy,
// D_j = (D_{j+1} o act'(h_{j+1})) W_j down to D_0. The weight gradients stay k_f32_wgrad (mlp_f32.hip).
//
// The register chain. mlp_f32.hip's operand scheme leaves lane (r = l & 15, q = l >> 4) of the forward with
// acc[t][c][e] = neuron 16 c + 4 q + e of batch row row0 + 16 t + r, and asks the same lane for X[row][16 s + 4 q + j]
// as the B operand of MFMA j of k-step s. With c = s and e = j these are one element: the activated accumulators of
// a layer ARE the operand registers of the next, tile c feeding k-step c. The backward-data product has the same
// property (gated dY operand, dX accumulators). So a wave that owns all W columns of its 32 rows runs the network
// out of registers: no LDS, no shuffle, no barrier, and HBM sees only the encoded rows, what the caller keeps, and
// the result.
//
// Bit for bit. The f32 MFMA is a k-ordered FMA chain, so an output element's bits are fixed by the order of its
// accumulation. Every product here walks k-steps s ascending and j = 0..3 inside a step into ONE accumulator per
// element, exactly as k_f32_layer_fwd / k_f32_layer_bwd do, and every activation goes through mlp_f32_ops.h: outputs,
// kept activations and every D_j equal the layer kernels' to the bit (tests/test_gpu_mlp_f32_fused.py).
//
// Work split. A wave owns 2 row tiles (32 rows) x WT = W / 16 column tiles: 2 WT independent accumulators per k-step,
// at least two as the MFMA's dependent-accumulator latency asks. The two layers whose other width is not W (the
// output layer of the forward: OUTP columns; the first layer of the chain: IN columns) run in groups of up to four
// column tiles, each group a full contraction from the operand registers. Four waves to a workgroup, 128 rows.
// Weights come through L1 / L2 like the layer kernels' ("Where the weights live").
//
// Layouts. Every batch-side operand a caller sees (the encoded rows of a network alone, the output, dL/dy, dL/de) is
// either AoS [B][width] or batch-contiguous, SoA [width][B], chosen at compile time per operand. For a fixed neuron
// the 16 lanes r = 0 .. 15 of a quarter hold 16 consecutive batch rows, so a SoA access is a 4-byte access per
// (t, c, e) whose lanes cover 64-byte runs: no LDS, no transpose. SoA operands have no padding: neurons at or past the
// true width are neither read nor written (a padded dL/dy element is the exact zero the AoS caller's padding holds).
// The forward's context stays AoS; a SoA forward writes it from the same registers as the caller's SoA output. The
// accumulation order does not depend on the layout, so a SoA result is the AoS result's bits, transposed
// (tests/test_gpu_mlp_f32_layouts.py). DESIGN.md, "Batch-contiguous matrices of fp32 network modules".
#include "mlp_f32_ops.h"

namespace tcnn_amd {

namespace {

constexpr uint32_t ROWS_PER_WAVE = 32, ROWS_PER_BLOCK = 128;

template <int NC>
__device__ __forceinline__ void zero_tiles(f4 (&a)[2][NC]) {
#pragma unroll
	for (int t = 0; t < 2; ++t)
#pragma unroll
		for (int c = 0; c < NC; ++c) a[t][c] = f4{0.0f, 0.0f, 0.0f, 0.0f};
}

// One forward product out of registers: acc[t][c] += W[16 c + r][16 s + 4 q + j] x[t][s][j] for the first nct of NC
// column tiles; wp = &W[r][4 q] of the first tile, K = 16 WT the row length of W.
template <int WT, int NC>
__device__ __forceinline__ void fwd_from_regs(const float* __restrict__ wp, uint32_t nct, const f4 (&x)[2][WT], f4 (&acc)[2][NC]) {
	constexpr uint32_t K = 16 * WT;
#pragma unroll
	for (int s = 0; s < WT; ++s)
#pragma unroll
		for (int c = 0; c < NC; ++c) {
			if ((uint32_t)c < nct) {
				const f4 w = *(const f4*)(wp + (size_t)c * 16 * K + 16 * s);
#pragma unroll
				for (int j = 0; j < 4; ++j) {
					acc[0][c] = mfma4(w[j], x[0][s][j], acc[0][c]);
					acc[1][c] = mfma4(w[j], x[1][s][j], acc[1][c]);
				}
			}
		}
}

// One backward-data product out of registers: acc[t][c] += W[16 s + 4 q + j][16 c + r] g[t][s][j] for the first kct
// of NC column tiles; wp = &W[4 q][r] of the first tile, K the row length of W, the contraction runs over 16 WT rows.
template <int WT, int NC>
__device__ __forceinline__ void bwd_from_regs(const float* __restrict__ wp, uint32_t K, uint32_t kct, const f4 (&g)[2][WT],
                                              f4 (&acc)[2][NC]) {
#pragma unroll
	for (int s = 0; s < WT; ++s)
#pragma unroll
		for (int c = 0; c < NC; ++c) {
			if ((uint32_t)c < kct) {
#pragma unroll
				for (int j = 0; j < 4; ++j) {
					const float w = wp[(size_t)(16 * s + j) * K + 16 * c];
					acc[0][c] = mfma4(w, g[0][s][j], acc[0][c]);
					acc[1][c] = mfma4(w, g[1][s][j], acc[1][c]);
				}
			}
		}
}

// h <- act(h): the accumulators become the next layer's operands; kept (nullable, the lane's &slot[row0 + r][4 q])
// receives them as the layer kernel would have stored them
template <int WT>
__device__ __forceinline__ void activate(f4 (&h)[2][WT], int act, float* __restrict__ kept) {
	constexpr uint32_t W = 16 * WT;
#pragma unroll
	for (int t = 0; t < 2; ++t)
#pragma unroll
		for (int c = 0; c < WT; ++c) {
#pragma unroll
			for (int e = 0; e < 4; ++e) h[t][c][e] = fwd_act(act, h[t][c][e]);
			if (kept) *(f4*)(kept + (size_t)16 * t * W + 16 * c) = h[t][c];
		}
}

// Y = oact(Wout act(W_{NH-1} .. act(W_0 e))), P = [W0 [W][IN] | W1 .. W_{NH-1} [W][W] | Wout [OUTP][W]]. HK (nullable):
// the hidden activations h_1 .. h_NH, [NH][B][W]. Y [B][OUTP], and Y2 (nullable) a second copy of it: a forward that
// keeps a context writes the output into the context and to the caller. Grid B / 128.
// XS: E is [IN][B] (a network alone: the caller's input is the encoded row), and EK (nullable) receives it as AoS
// [B][IN] rows for the context. YS: Y2 is the caller's [NOUT][B], NOUT <= OUTP the unpadded width, and Y (nullable)
// the context's AoS [B][OUTP]; without a context the output tiles past NOUT are not computed at all.
template <int WT, bool XS, bool YS>
__global__ __launch_bounds__(256) void k_f32_mlp_fwd(uint32_t B, uint32_t IN, uint32_t NH, uint32_t OUTP, uint32_t NOUT,
                                                      const float* __restrict__ P, const float* __restrict__ E, float* __restrict__ EK,
                                                      float* __restrict__ HK, float* __restrict__ Y, float* __restrict__ Y2, int act,
                                                      int oact) {
	constexpr uint32_t W = 16 * WT;
	const uint32_t lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;
	const uint32_t row0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * ROWS_PER_WAVE;
	if (row0 >= B) return;
	const size_t lane_w = (size_t)(row0 + r) * W + 4 * q;  // the lane's place in a [B][W] slot
	f4 h[2][WT];
	zero_tiles(h);
	{  // first layer: the K-loop of k_f32_layer_fwd over the encoded row, all WT column tiles
		const float* x0 = E + (size_t)(row0 + r) * IN + 4 * q;  // AoS rows (unused when XS)
		const float* x1 = x0 + (size_t)16 * IN;
		const float* wp = P + (size_t)r * IN + 4 * q;
		for (uint32_t s = 0; s < IN; s += 16) {
			f4 a0, a1;
			if constexpr (XS) {  // four loads per row tile, each a 64-byte run across r; + 0: Identity's x * 1 + 0
				const float* xs = E + (size_t)(s + 4 * q) * B + row0 + r;
#pragma unroll
				for (int j = 0; j < 4; ++j) {
					a0[j] = xs[(size_t)j * B] + 0.0f;
					a1[j] = xs[(size_t)j * B + 16] + 0.0f;
				}
				if (EK) {
					float* ek = EK + (size_t)(row0 + r) * IN + 4 * q + s;
					*(f4*)ek = a0;
					*(f4*)(ek + (size_t)16 * IN) = a1;
				}
			} else {
				a0 = *(const f4*)(x0 + s);
				a1 = *(const f4*)(x1 + s);
			}
#pragma unroll
			for (int c = 0; c < WT; ++c) {
				const f4 w = *(const f4*)(wp + (size_t)c * 16 * IN + s);
#pragma unroll
				for (int j = 0; j < 4; ++j) {
					h[0][c] = mfma4(w[j], a0[j], h[0][c]);
					h[1][c] = mfma4(w[j], a1[j], h[1][c]);
				}
			}
		}
	}
	activate(h, act, HK ? HK + lane_w : nullptr);
	const float* wl = P + (size_t)W * IN;
	for (uint32_t l = 1; l < NH; ++l, wl += (size_t)W * W) {
		f4 n[2][WT];
		zero_tiles(n);
		fwd_from_regs<WT, WT>(wl + (size_t)r * W + 4 * q, WT, h, n);
#pragma unroll
		for (int t = 0; t < 2; ++t)
#pragma unroll
			for (int c = 0; c < WT; ++c) h[t][c] = n[t][c];
		activate(h, act, HK ? HK + (size_t)l * B * W + lane_w : nullptr);
	}
	// output layer: groups of up to four column tiles, each a full contraction from h
	const uint32_t nt = YS && !Y ? (NOUT + 15) / 16 : OUTP / 16;
	for (uint32_t c0 = 0; c0 < nt; c0 += 4) {
		const uint32_t nct = min(4u, nt - c0);
		f4 o[2][4];
		zero_tiles(o);
		fwd_from_regs<WT, 4>(wl + (size_t)(16 * c0 + r) * W + 4 * q, nct, h, o);
#pragma unroll
		for (int t = 0; t < 2; ++t)
#pragma unroll
			for (int c = 0; c < 4; ++c) {
				if ((uint32_t)c < nct) {
					f4 v;
#pragma unroll
					for (int e = 0; e < 4; ++e) v[e] = fwd_act(oact, o[t][c][e]);
					const size_t at = (size_t)(row0 + 16 * t + r) * OUTP + 16 * (c0 + c) + 4 * q;
					if constexpr (YS) {  // one neuron per store, 16 consecutive rows across r; nothing past NOUT
						if (Y) *(f4*)(Y + at) = v;
						const uint32_t n0 = 16 * (c0 + c) + 4 * q;
#pragma unroll
						for (int e = 0; e < 4; ++e)
							if (n0 + e < NOUT) Y2[(size_t)(n0 + e) * B + row0 + 16 * t + r] = v[e];
					} else {
						*(f4*)(Y + at) = v;
						if (Y2) *(f4*)(Y2 + at) = v;
					}
				}
			}
	}
}

// The delta chain from a forward's context KEEP = [e [B][IN] | h_1 .. h_NH [NH][B][W] | y [B][OUTP]] and dL/dy DY
// [B][OUTP]. DH (nullable): D_1 .. D_NH = dL/dh_1 .. dL/dh_NH, [NH][B][W], ungated like the layer kernels' deltas (the
// weight gradient applies the transfer as it loads them); D0 (nullable): dL/de [B][IN]. Grid B / 128.
// GS: DY is [NOUT][B], NOUT <= OUTP the unpadded width (a neuron past it is an exact zero), and DYA (nullable) receives
// it as the AoS [B][OUTP] rows, zero padded, that the output layer's weight gradient reads. DS: D0 is [IN][B].
template <int WT, bool GS, bool DS>
__global__ __launch_bounds__(256) void k_f32_mlp_bwd_chain(uint32_t B, uint32_t IN, uint32_t NH, uint32_t OUTP, uint32_t NOUT,
                                                            const float* __restrict__ P, const float* __restrict__ DY,
                                                            float* __restrict__ DYA, const float* __restrict__ KEEP, float* __restrict__ DH,
                                                            float* __restrict__ D0, int act, int oact) {
	constexpr uint32_t W = 16 * WT;
	const uint32_t lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;
	const uint32_t row0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * ROWS_PER_WAVE;
	if (row0 >= B) return;
	const size_t lane_w = (size_t)(row0 + r) * W + 4 * q;
	const float* H = KEEP + (size_t)B * IN;  // h_{l + 1} at H + l B W
	const float* Yv = H + (size_t)NH * B * W;
	const float* wl = P + (size_t)W * IN + (size_t)(NH - 1) * W * W;  // Wout, then W_{NH-1} .. W_1
	f4 d[2][WT];
	zero_tiles(d);
	{  // output layer: the loop of k_f32_layer_bwd over dL/dy, all WT column tiles
		const size_t g_off0 = (size_t)(row0 + r) * OUTP + 4 * q, g_off1 = g_off0 + (size_t)16 * OUTP;
		const float* wp = wl + (size_t)(4 * q) * W + r;
		for (uint32_t s = 0; s < OUTP; s += 16) {
			f4 g0, g1;
			if constexpr (GS) {  // the forward's stores mirrored: one neuron per load, 16 consecutive rows across r
				const uint32_t n0 = s + 4 * q;
#pragma unroll
				for (int j = 0; j < 4; ++j) {
					const bool in = n0 + j < NOUT;
					const float* gs = DY + (size_t)(n0 + j) * B + row0 + r;
					g0[j] = in ? gs[0] : 0.0f;
					g1[j] = in ? gs[16] : 0.0f;
				}
				if (DYA) {
					*(f4*)(DYA + g_off0 + s) = g0;
					*(f4*)(DYA + g_off1 + s) = g1;
				}
			} else {
				g0 = *(const f4*)(DY + g_off0 + s);
				g1 = *(const f4*)(DY + g_off1 + s);
			}
			g0 = bwd_act4(oact, g0, Yv + g_off0 + s);
			g1 = bwd_act4(oact, g1, Yv + g_off1 + s);
#pragma unroll
			for (int c = 0; c < WT; ++c) {
#pragma unroll
				for (int j = 0; j < 4; ++j) {
					const float w = wp[(size_t)(s + j) * W + 16 * c];
					d[0][c] = mfma4(w, g0[j], d[0][c]);
					d[1][c] = mfma4(w, g1[j], d[1][c]);
				}
			}
		}
	}
	for (uint32_t l = NH; l-- > 0;) {  // d = D_{l + 1}
		const size_t at = (size_t)l * B * W + lane_w;
		if (DH) {
#pragma unroll
			for (int t = 0; t < 2; ++t)
#pragma unroll
				for (int c = 0; c < WT; ++c) *(f4*)(DH + at + (size_t)16 * t * W + 16 * c) = d[t][c];
		}
		if (l == 0 && !D0) return;
#pragma unroll
		for (int t = 0; t < 2; ++t)
#pragma unroll
			for (int c = 0; c < WT; ++c) d[t][c] = bwd_act4(act, d[t][c], H + at + (size_t)16 * t * W + 16 * c);
		if (l == 0) break;
		wl -= (size_t)W * W;
		f4 n[2][WT];
		zero_tiles(n);
		bwd_from_regs<WT, WT>(wl + (size_t)(4 * q) * W + r, W, WT, d, n);
#pragma unroll
		for (int t = 0; t < 2; ++t)
#pragma unroll
			for (int c = 0; c < WT; ++c) d[t][c] = n[t][c];
	}
	if (!D0) return;
	// first layer: groups of up to four column tiles of dL/de, each a full contraction from the gated D_1
	const uint32_t nt = IN / 16;
	for (uint32_t c0 = 0; c0 < nt; c0 += 4) {
		const uint32_t kct = min(4u, nt - c0);
		f4 o[2][4];
		zero_tiles(o);
		bwd_from_regs<WT, 4>(P + (size_t)(4 * q) * IN + 16 * c0 + r, IN, kct, d, o);
#pragma unroll
		for (int t = 0; t < 2; ++t)
#pragma unroll
			for (int c = 0; c < 4; ++c)
				if ((uint32_t)c < kct) {
					if constexpr (DS) {
						float* ds = D0 + (size_t)(16 * (c0 + c) + 4 * q) * B + row0 + 16 * t + r;
#pragma unroll
						for (int e = 0; e < 4; ++e) ds[(size_t)e * B] = o[t][c][e];
					} else {
						*(f4*)(D0 + (size_t)(row0 + 16 * t + r) * IN + 16 * (c0 + c) + 4 * q) = o[t][c];
					}
				}
	}
}

void check_fused_shape(uint32_t B, uint32_t IN, uint32_t W, uint32_t NH, uint32_t OUTP, const char* what) {
	TCNN_CHECK(f32_mlp_fused_width_ok(W), std::string(what) + ": the width must be 16, 32, 64 or 128");
	TCNN_CHECK(NH >= 1, std::string(what) + ": at least one hidden layer");
	TCNN_CHECK(IN && OUTP && IN % 16 == 0 && OUTP % 16 == 0, std::string(what) + ": widths must be multiples of 16");
	TCNN_CHECK(B % ROWS_PER_BLOCK == 0, std::string(what) + ": batch must be a multiple of 128");
}

// dst[c][r] = src[r][c]: the positions and dL/dinput of a SoA call whose encoding keeps AoS kernels (a handful of
// floats per row beside the network's). One thread per element, consecutive threads along r.
__global__ __launch_bounds__(256) void k_f32_transpose(uint32_t R, uint32_t C, const float* __restrict__ src, float* __restrict__ dst) {
	const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (i >= (size_t)R * C) return;
	const size_t c = i / R, r = i % R;
	dst[i] = src[r * C + c];
}

template <bool XS, bool YS>
void fwd_layout(hipStream_t st, uint32_t B, uint32_t IN, uint32_t W, uint32_t NH, uint32_t OUTP, uint32_t n_out, const float* p, const float* e,
                float* ek, float* hk, float* y, float* y2, int act, int oact) {
	const dim3 grid(B / ROWS_PER_BLOCK), block(256);
	switch (W) {
		case 16: hipLaunchKernelGGL((k_f32_mlp_fwd<1, XS, YS>), grid, block, 0, st, B, IN, NH, OUTP, n_out, p, e, ek, hk, y, y2, act, oact); break;
		case 32: hipLaunchKernelGGL((k_f32_mlp_fwd<2, XS, YS>), grid, block, 0, st, B, IN, NH, OUTP, n_out, p, e, ek, hk, y, y2, act, oact); break;
		case 64: hipLaunchKernelGGL((k_f32_mlp_fwd<4, XS, YS>), grid, block, 0, st, B, IN, NH, OUTP, n_out, p, e, ek, hk, y, y2, act, oact); break;
		default: hipLaunchKernelGGL((k_f32_mlp_fwd<8, XS, YS>), grid, block, 0, st, B, IN, NH, OUTP, n_out, p, e, ek, hk, y, y2, act, oact); break;
	}
}

template <bool GS, bool DS>
void chain_layout(hipStream_t st, uint32_t B, uint32_t IN, uint32_t W, uint32_t NH, uint32_t OUTP, uint32_t n_out, const float* p,
                  const float* dy, float* dya, const float* keep, float* dh, float* d0, int act, int oact) {
	const dim3 grid(B / ROWS_PER_BLOCK), block(256);
	switch (W) {
		case 16: hipLaunchKernelGGL((k_f32_mlp_bwd_chain<1, GS, DS>), grid, block, 0, st, B, IN, NH, OUTP, n_out, p, dy, dya, keep, dh, d0, act, oact); break;
		case 32: hipLaunchKernelGGL((k_f32_mlp_bwd_chain<2, GS, DS>), grid, block, 0, st, B, IN, NH, OUTP, n_out, p, dy, dya, keep, dh, d0, act, oact); break;
		case 64: hipLaunchKernelGGL((k_f32_mlp_bwd_chain<4, GS, DS>), grid, block, 0, st, B, IN, NH, OUTP, n_out, p, dy, dya, keep, dh, d0, act, oact); break;
		default: hipLaunchKernelGGL((k_f32_mlp_bwd_chain<8, GS, DS>), grid, block, 0, st, B, IN, NH, OUTP, n_out, p, dy, dya, keep, dh, d0, act, oact); break;
	}
}

}  // namespace

void launch_f32_mlp_fwd(hipStream_t st, uint32_t B, uint32_t IN, uint32_t W, uint32_t NH, uint32_t OUTP, const float* params, const float* e,
                        float* hidden_keep, float* y, float* y2, int act, int out_act) {
	launch_f32_mlp_fwd_layout(st, B, IN, W, NH, OUTP, OUTP, params, e, false, nullptr, hidden_keep, y, y2, false, act, out_act);
}

void launch_f32_mlp_fwd_layout(hipStream_t st, uint32_t B, uint32_t IN, uint32_t W, uint32_t NH, uint32_t OUTP, uint32_t n_out,
                               const float* params, const float* e, bool e_soa, float* e_keep, float* hidden_keep, float* y, float* y2,
                               bool y2_soa, int act, int out_act) {
	check_fused_shape(B, IN, W, NH, OUTP, "fp32 fused forward");
	if (!B) return;
	TCNN_CHECK(params && e && (y2_soa ? y2 : y), "fp32 fused forward: the parameters, the encoded rows or the output are missing");
	TCNN_CHECK(n_out && n_out <= OUTP, "fp32 fused forward: the unpadded output width must lie in [1, padded width]");
	if (e_soa && y2_soa) fwd_layout<true, true>(st, B, IN, W, NH, OUTP, n_out, params, e, e_keep, hidden_keep, y, y2, act, out_act);
	else if (e_soa) fwd_layout<true, false>(st, B, IN, W, NH, OUTP, n_out, params, e, e_keep, hidden_keep, y, y2, act, out_act);
	else if (y2_soa) fwd_layout<false, true>(st, B, IN, W, NH, OUTP, n_out, params, e, e_keep, hidden_keep, y, y2, act, out_act);
	else fwd_layout<false, false>(st, B, IN, W, NH, OUTP, n_out, params, e, e_keep, hidden_keep, y, y2, act, out_act);
	TCNN_HIP_CHECK(hipGetLastError());
}

void launch_f32_mlp_bwd_chain(hipStream_t st, uint32_t B, uint32_t IN, uint32_t W, uint32_t NH, uint32_t OUTP, const float* params,
                              const float* dy, const float* keep, float* d_hidden, float* d0, int act, int out_act) {
	launch_f32_mlp_bwd_chain_layout(st, B, IN, W, NH, OUTP, OUTP, params, dy, false, nullptr, keep, d_hidden, d0, false, act, out_act);
}

void launch_f32_mlp_bwd_chain_layout(hipStream_t st, uint32_t B, uint32_t IN, uint32_t W, uint32_t NH, uint32_t OUTP, uint32_t n_out,
                                     const float* params, const float* dy, bool dy_soa, float* dy_aos, const float* keep, float* d_hidden,
                                     float* d0, bool d0_soa, int act, int out_act) {
	check_fused_shape(B, IN, W, NH, OUTP, "fp32 fused backward");
	TCNN_CHECK(act != ACT_SINE && out_act != ACT_SINE, "fp32 fused backward: Sine has no backward from its forward value");
	if (!B || (!d_hidden && !d0)) return;
	TCNN_CHECK(params && dy && keep, "fp32 fused backward: the parameters, dL/dy or the forward context are missing");
	TCNN_CHECK(n_out && n_out <= OUTP, "fp32 fused backward: the unpadded output width must lie in [1, padded width]");
	if (dy_soa && d0_soa) chain_layout<true, true>(st, B, IN, W, NH, OUTP, n_out, params, dy, dy_aos, keep, d_hidden, d0, act, out_act);
	else if (dy_soa) chain_layout<true, false>(st, B, IN, W, NH, OUTP, n_out, params, dy, dy_aos, keep, d_hidden, d0, act, out_act);
	else if (d0_soa) chain_layout<false, true>(st, B, IN, W, NH, OUTP, n_out, params, dy, dy_aos, keep, d_hidden, d0, act, out_act);
	else chain_layout<false, false>(st, B, IN, W, NH, OUTP, n_out, params, dy, dy_aos, keep, d_hidden, d0, act, out_act);
	TCNN_HIP_CHECK(hipGetLastError());
}

void launch_f32_transpose(hipStream_t st, uint32_t R, uint32_t C, const float* src, float* dst) {
	const size_t n = (size_t)R * C;
	if (!n) return;
	TCNN_CHECK(src && dst, "fp32 transpose: a matrix is missing");
	hipLaunchKernelGGL(k_f32_transpose, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, R, C, src, dst);
	TCNN_HIP_CHECK(hipGetLastError());
}

}  // namespace tcnn_amd
