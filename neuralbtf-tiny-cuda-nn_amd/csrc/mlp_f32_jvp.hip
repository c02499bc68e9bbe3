// mlp_f32_jvp.hip -- the value f(x) and K directional input derivatives J(x) v_k of an fp32 FullyFusedMLP network
// module behind a lone grid (or a lone Identity), in one forward-mode launch that keeps nothing
// (NetworkF32Host::jvp, tcnn_module_inference_jvp). Null directions mean the D unit vectors: the input Jacobian.
//
// Behind the first layer this is the register chain of the Jacobian kernel (mlp_f32_chain.h): one 16-row tile per
// wave, the value and TG tangents through every layer out of registers, one output column tile at a time. What is
// new is the front: the grid is encoded straight into the MFMA operand layout, value and tangents together, so no
// encoded row ever reaches memory.
//
// The lane-to-level map. In the operand scheme lane (r = l & 15, q = l >> 4) supplies columns k = 16 s + 4 q + j,
// j = 0..3, of batch row r for k-step s, and encoded column k is feature k % F of level k / F. A lane's four columns of
// a k-step are therefore
//   F = 2: levels 8 s + 2 q and 8 s + 2 q + 1, both features of each;
//   F = 4: level 4 s + q, its four features;
//   F = 8: level 2 s + (q >> 1), features 4 (q & 1) .. + 3 -- two lanes share the level's index arithmetic and each
//          loads its own 16 bytes of every corner.
// The four quarters of a wave split a row's levels between them and every gathered value is consumed by the lane that
// loaded it: across the encode and the network there is no LDS, no shuffle and no barrier. Columns past L F are the
// forward's padding, zeros for the value and for every tangent.
//
// Value. A column is encode_level_f32's (grid_f32_device.h: the same weight products, corner order and FMA chain), the
// first layer is the K-loop of k_f32_mlp_fwd, and the rest is the chain whose value order is the forward's: y carries
// the bits of tcnn_module_inference.
//
// Tangents. d e_k / d x_d comes from the corners the value already gathered (level_tangent_f32, the arithmetic of
// k_grid_bwd_input): no second gather. Quantity i's operand is e'_k[i] = sum_d (d e_k / d x_d) v_i[d], summed in
// ascending d with one FMA per term after the first; for the unit directions it is the single term, no multiply.
// The first layer is then a real contraction for all 1 + TG quantities, every weight f4 used by each of them.
//
// Registers. A pass encodes its whole operand, (1 + TG) IN / 4 registers, before an accumulator is live -- the
// gathers of a k-step are issued together -- and then contracts. TG is the Jacobian kernel's: 3 up to W 64, 1 at W 128,
// where one direction is one pass. K > TG runs ceil(K / TG) passes inside the launch, each re-encoding; the first
// stores y. The resource report shows no scratch in any instantiation (DESIGN.md has the table).
//
// Instantiations: W, D and F only. The hash's multipliers, the interpolation, and the layouts of x, the directions, y
// and the product are run-time values, all wave-uniform: 24 grid kernels and 4 for the Identity front.
#include "mlp_f32_jvp_device.h"

namespace tcnn_amd {

namespace {

// JvpArgs, the first layer behind an Identity row (jac_identity_layer) and the grid encoded into the operand layout
// (jvp_encode_step) live in mlp_f32_jvp_device.h, which the forward that keeps a context shares.
//
// From the first layer's pre-activations h (value and tangents) to memory: the first activation, the hidden layers
// wl = W1 .. W_{NH-1}, the output layer, and the stores of lane (r, q)'s batch row `row`. Tangent i is number
// d0 + i - 1 of the call's D (the inputs of a Jacobian, the directions of a product); those past D are not stored, and
// the pass with d0 == 0 stores y. ys: Y is [NOUT][B] and J [NOUT D][B] (row o D + d), else Y [B][OUTP] rows as the
// forward writes them and J [B][NOUT][D].
// keep_chain (mlp_f32_jvp_train.hip) is this function's twin with the stores of a context: the two must stay in step,
// operation for operation, or the keeping forward loses this kernel's bits (tests/test_gpu_mlp_f32_jvp_train.py).
template <int WT, int NQ>
__device__ __forceinline__ void jac_chain(f4 (&h)[NQ][WT], const float* __restrict__ wl, uint32_t NH, uint32_t r, uint32_t q, uint32_t row,
                                          uint32_t B, uint32_t OUTP, uint32_t NOUT, uint32_t D, uint32_t d0, bool ys, float* __restrict__ Y,
                                          float* __restrict__ J, int act, int oact) {
	constexpr uint32_t W = 16 * WT;
	const uint32_t nt = (NOUT + 15) / 16;  // = OUTP / 16: the padded width is the next multiple of 16
	jac_activate<WT, NQ>(h, act);
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
	// of four would keep 16 NQ more accumulators live across the out-of-line activation calls, which the
	// resource report answers with scratch at W 64; the NQ quantities still give independent chains.
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
			if (ys) {
#pragma unroll
				for (int e = 0; e < 4; ++e)
					if (n0 + e < NOUT) Y[(size_t)(n0 + e) * B + row] = o[0][0][e];
			} else {
				*(f4*)(Y + (size_t)row * OUTP + n0) = o[0][0];
			}
		}
		// J[.][n0 + e][d0 + i - 1]: one running pointer, stepped by the element strides of o and d
		const size_t so = ys ? (size_t)D * B : D, sd = ys ? B : 1;
		float* je = J + (ys ? ((size_t)n0 * D + d0) * B + row : ((size_t)row * NOUT + n0) * D + d0);
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

// Grid B / 64. W = 16 WT, D input dimensions and F features per level of the grid in front.
template <int WT, uint32_t D, uint32_t F>
__global__ __launch_bounds__(256) void k_f32_grid_mlp_jvp(const JvpArgs a) {
	constexpr uint32_t W = 16 * WT;
	constexpr int TG = jvp_tangents(WT), NQ = 1 + TG;  // quantity 0 is the value, 1 .. TG tangents k0 .. k0 + TG - 1
	const uint32_t lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;
	const uint32_t row = (blockIdx.x * 4 + (threadIdx.x >> 6)) * JAC_ROWS_PER_WAVE + r;
	if (row >= a.B) return;
	float x[D];
#pragma unroll
	for (uint32_t d = 0; d < D; ++d) x[d] = a.x_soa ? a.X[(size_t)d * a.B + row] : a.X[(size_t)row * D + d];
	uint32_t prime[D];
	hash_primes<D>((HashType)a.hash, prime);
	const uint32_t ks = a.IN / 16;
	for (uint32_t k0 = 0; k0 < a.K; k0 += TG) {
		float dir[TG][D];
#pragma unroll
		for (int i = 0; i < TG; ++i)
#pragma unroll
			for (uint32_t d = 0; d < D; ++d) {
				const uint32_t k = k0 + i;
				dir[i][d] = a.V && k < a.K ? (a.x_soa ? a.V[((size_t)k * D + d) * a.B + row] : a.V[((size_t)row * a.K + k) * D + d]) : 0.0f;
			}
		// the pass's whole operand, before an accumulator is live
		f4 e[NQ][JVP_MAX_KSTEPS];
#pragma unroll
		for (uint32_t s = 0; s < JVP_MAX_KSTEPS; ++s) {
			if (s < ks) {
				f4 es[NQ];
				jvp_encode_step<D, F, NQ>(a, s, q, k0, x, dir, prime, es);
#pragma unroll
				for (int i = 0; i < NQ; ++i) e[i][s] = es[i];
			}
		}
		// first layer: the K-loop of k_f32_mlp_fwd for every quantity, each weight f4 used by all of them
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
		jac_chain<WT, NQ>(h, a.P + (size_t)W * a.IN, a.NH, r, q, row, a.B, a.OUTP, a.NOUT, a.K, k0, a.y_soa != 0, a.Y, a.J, a.act, a.oact);
	}
}

// The same call behind an Identity row (or a network alone): the Jacobian kernel's first layer, whose tangents need no
// contraction, with directions when there are any. Null directions give tcnn_module_inference_jacobian's bits.
template <int WT>
__global__ __launch_bounds__(256) void k_f32_identity_mlp_jvp(const JvpArgs a) {
	constexpr uint32_t W = 16 * WT;
	constexpr int TG = jvp_tangents(WT), NQ = 1 + TG;
	const uint32_t lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;
	const uint32_t row = (blockIdx.x * 4 + (threadIdx.x >> 6)) * JAC_ROWS_PER_WAVE + r;
	if (row >= a.B) return;
	for (uint32_t k0 = 0; k0 < a.K; k0 += TG) {
		f4 h[NQ][WT];
		jac_identity_layer<WT, NQ>(h, a.P, a.X, a.x_soa != 0, a.V, a.B, a.D, a.K, a.IN, a.scale, a.offset, r, q, row, k0);
		jac_chain<WT, NQ>(h, a.P + (size_t)W * a.IN, a.NH, r, q, row, a.B, a.OUTP, a.NOUT, a.K, k0, a.y_soa != 0, a.Y, a.J, a.act, a.oact);
	}
}

template <int WT>
void jvp_width(hipStream_t st, const JvpArgs& a, bool grid, uint32_t D, uint32_t F) {
	const dim3 blocks(a.B / JAC_ROWS_PER_BLOCK), block(256);
	if (!grid) {
		hipLaunchKernelGGL((k_f32_identity_mlp_jvp<WT>), blocks, block, 0, st, a);
		return;
	}
	switch (D * 16 + F) {
		case 2 * 16 + 2: hipLaunchKernelGGL((k_f32_grid_mlp_jvp<WT, 2, 2>), blocks, block, 0, st, a); break;
		case 2 * 16 + 4: hipLaunchKernelGGL((k_f32_grid_mlp_jvp<WT, 2, 4>), blocks, block, 0, st, a); break;
		case 2 * 16 + 8: hipLaunchKernelGGL((k_f32_grid_mlp_jvp<WT, 2, 8>), blocks, block, 0, st, a); break;
		case 3 * 16 + 2: hipLaunchKernelGGL((k_f32_grid_mlp_jvp<WT, 3, 2>), blocks, block, 0, st, a); break;
		case 3 * 16 + 4: hipLaunchKernelGGL((k_f32_grid_mlp_jvp<WT, 3, 4>), blocks, block, 0, st, a); break;
		default: hipLaunchKernelGGL((k_f32_grid_mlp_jvp<WT, 3, 8>), blocks, block, 0, st, a); break;
	}
}

}  // namespace

bool f32_mlp_jvp_grid_ok(uint32_t D, uint32_t F, uint32_t IN) { return (D == 2 || D == 3) && (F == 2 || F == 4 || F == 8) && IN <= 16 * JVP_MAX_KSTEPS; }

void launch_f32_mlp_jvp(hipStream_t st, uint32_t B, uint32_t D, uint32_t IN, uint32_t W, uint32_t NH, uint32_t OUTP, uint32_t n_out,
                        const float* params, const float* x, const float* directions, uint32_t n_directions, bool x_soa, float* y, float* jvp,
                        bool y_soa, int act, int out_act, const GridCall* grid, const float* table, float scale, float offset) {
	const char* what = "fp32 Jacobian-vector product";
	TCNN_CHECK(f32_mlp_fused_width_ok(W), std::string(what) + ": the width must be 16, 32, 64 or 128");
	TCNN_CHECK(NH >= 1, std::string(what) + ": at least one hidden layer");
	TCNN_CHECK(IN && OUTP && IN % 16 == 0 && OUTP % 16 == 0, std::string(what) + ": widths must be multiples of 16");
	TCNN_CHECK(B % 128 == 0, std::string(what) + ": batch must be a multiple of 128");
	TCNN_CHECK(n_out && n_out <= OUTP && OUTP - n_out < 16, std::string(what) + ": the padded output width must be the next multiple of 16");
	TCNN_CHECK(act != ACT_SINE && out_act != ACT_SINE, std::string(what) + ": Sine has no backward from its forward value");
	TCNN_CHECK(directions ? n_directions >= 1 : n_directions == D, std::string(what) + ": at least one direction, or the input width for the unit vectors");
	JvpArgs a{};
	if (grid) {
		TCNN_CHECK(grid->D == D && f32_mlp_jvp_grid_ok(D, grid->F, IN) && grid->L && grid->L * grid->F <= IN && !grid->opts.active,
		           std::string(what) + ": a grid of 2 or 3 input dimensions, 2, 4 or 8 features per level and at most 64 columns, without options");
		a.table = table;
		a.levels = grid->levels;
		a.L = grid->L;
		a.hash_grid = grid->hash_grid ? 1u : 0u;
		a.interp = (uint32_t)grid->interp;
		const uint32_t tb = grid->F * 4u < 16u ? grid->F * 4u : 16u;  // FVec loads: entry e sits at table + e F, so the base decides
		a.vec = (uintptr_t)table % tb == 0 ? 1u : 0u;
		a.hash = (uint32_t)grid->hash;
	} else {
		TCNN_CHECK(D && D <= IN, std::string(what) + ": the input width must lie in [1, encoded width]");
	}
	if (!B) return;
	TCNN_CHECK(params && x && y && jvp && (!grid || table), std::string(what) + ": the parameters, the inputs, the output or the product are missing");
	a.B = B, a.D = D, a.IN = IN, a.NH = NH, a.OUTP = OUTP, a.NOUT = n_out, a.K = n_directions;
	a.P = params, a.X = x, a.V = directions, a.Y = y, a.J = jvp;
	a.x_soa = x_soa ? 1u : 0u, a.y_soa = y_soa ? 1u : 0u;
	a.act = act, a.oact = out_act;
	a.scale = scale, a.offset = offset;
	const uint32_t F = grid ? grid->F : 0;
	switch (W) {
		case 16: jvp_width<1>(st, a, grid != nullptr, D, F); break;
		case 32: jvp_width<2>(st, a, grid != nullptr, D, F); break;
		case 64: jvp_width<4>(st, a, grid != nullptr, D, F); break;
		default: jvp_width<8>(st, a, grid != nullptr, D, F); break;
	}
	TCNN_HIP_CHECK(hipGetLastError());
}

}  // namespace tcnn_amd
