// mlp_f32_hessian.hip -- the input Hessian of an fp32 FullyFusedMLP network module behind a lone grid (or a lone
// Identity): the value f(x), K <= 3 directional derivatives J(x) v_k and every v_k^T H(x) v_k' per output, in one
// forward-mode launch that keeps nothing (NetworkF32Host::hessian, tcnn_module_inference_hessian). Null directions mean
// the D unit vectors: the Jacobian and d^2 y_o / dx_d dx_d'.
//
// The scheme. mlp_f32_jvp2.hip carries the SUM over k of the second-order quantity because the Laplacian wants nothing
// else. Here each pair of directions i <= j keeps a row of its own: per layer z = W h, s_k = W t_k, r_ij = W u_ij,
//   h' = a(z), t_k' = a'(z) s_k, u_ij' = a'(z) r_ij + a''(z) s_i s_j,
// which is symmetric in (i, j), so K (K + 1) / 2 rows give both triangles. The launch is one pass that carries the
// value, NT tangents and NP pair rows, 1 + NT + NP rows of a wave's 16-row tile through the Jacobian kernel's register
// chain (jac_from_regs, mlp_f32_chain.h). The pairs are numbered (0,0) (0,1) (1,1) (0,2) (1,2) (2,2): K <= 2 needs the
// first three and runs 2 tangents and 3 pairs (six rows; K = 1 leaves one tangent row zero and stores one pair), K = 3
// runs 3 tangents and all 6 pairs (ten rows). Ten rows fit at every width served: the resource report shows no spilled
// register and no private segment in any instantiation, 468 of the 512 unified registers at W 64 (DESIGN.md has the
// table), so no shape needs a second pass over the network and the grid.
//
// Work split: mlp_f32_jvp.hip's. 64 batch rows per 256-thread workgroup, one 16-row tile per wave, lane (r, q) supplies
// operand columns 16 s + 4 q + j; no LDS, no shuffle, no barrier. Every row sees jac_chain's products in jac_chain's
// order, so y and Jv carry tcnn_module_inference_jvp's bits, and a diagonal pair (k, k) sees jac_gate2's operations
// with one direction -- one product s_k s_k, then fmaf(a'', s_k s_k, a' r) -- so H[k][k] carries the bits of
// tcnn_module_inference_jvp_second's q for direction k alone. All indices of rows are compile-time constants
// (hess_pair_i / hess_pair_j fold after unrolling): nothing indexes a register array at run time.
//
// Fronts. Behind an Identity every u_ij enters the first gate as zero. Behind a grid u_ij[col] =
// sum_{d, d'} M_ij[d][d'] d^2 e_col / dx_d dx_d' with M_ij = (v_i v_j^T + v_j v_i^T) / 2 (v_i v_i^T on the diagonal,
// formed as mlp_f32_jvp2.hip forms it), from the corners the value gathered: one gather per level serves every row
// (hess_encode_step, level_second_f32). For the unit vectors M_dd is a single 1 and M_de a single 1/2; the mixed term
// that jvp2_encode_step skips under null directions is what gives the off-diagonal entries here.
//
// Stores. Each Hessian element and its mirror are stored once, by one lane: no load-add-store, bit-reproducible by
// construction.
//
// Instantiations: W, D and F only, as in mlp_f32_jvp2.hip: 18 grid kernels and 3 for the Identity front.
#include "mlp_f32_jvp_device.h"

namespace tcnn_amd {

namespace {

constexpr int HESS_MAX_DIRECTIONS = 3;
// pair p of (0,0) (0,1) (1,1) (0,2) (1,2) (2,2)
constexpr int hess_pair_i(int p) { return p == 2 || p == 4 ? 1 : p == 5 ? 2 : 0; }
constexpr int hess_pair_j(int p) { return p == 0 ? 0 : p <= 2 ? 1 : 2; }

struct HessArgs {
	JvpArgs j;
	float* H;  // [B][NOUT][K][K], or [NOUT K K][B] when y_soa
};

// The gate with curvature for pair rows: rows 0 the value, 1 .. NT the tangents s_k, 1 + NT + p pair p's r_ij.
// jac_gate2's operations (mlp_f32_chain.h) per pair: y = act(z), u_ij <- fmaf(act'', s_i s_j, act' r_ij) from the
// tangents before they are scaled, then s_k <- act' s_k as jac_activate does it.
template <int WT, int NT, int NP>
__device__ __forceinline__ void hess_activate(f4 (&h)[1 + NT + NP][WT], int act) {
	if (act == ACT_NONE) return;
#pragma unroll
	for (int c = 0; c < WT; ++c)
#pragma unroll
		for (int e = 0; e < 4; ++e) {
			const float y = fwd_act(act, h[0][c][e]);
			const float f = bwd_act(act, 1.0f, y);
			const float g = curv_act(act, y);
			h[0][c][e] = y;
#pragma unroll
			for (int p = 0; p < NP; ++p) {
				const float ss = h[1 + hess_pair_i(p)][c][e] * h[1 + hess_pair_j(p)][c][e];
				h[1 + NT + p][c][e] = __builtin_fmaf(g, ss, f * h[1 + NT + p][c][e]);
			}
#pragma unroll
			for (int i = 1; i <= NT; ++i) h[i][c][e] *= f;
		}
}

// One output tile's four neurons n0 .. n0 + 3 of batch row `row` to memory: y and Jv as jac_chain stores them, and
// every pair whose two directions exist (j < K; i <= j), element and mirror
template <int NT, int NP>
__device__ __forceinline__ void hess_store(const f4 (&o)[1 + NT + NP][1], const JvpArgs& a, float* __restrict__ H, uint32_t n0, uint32_t row) {
	const bool ys = a.y_soa != 0;
	const uint32_t B = a.B, K = a.K, NOUT = a.NOUT;
	if (ys) {
#pragma unroll
		for (int e = 0; e < 4; ++e)
			if (n0 + e < NOUT) a.Y[(size_t)(n0 + e) * B + row] = o[0][0][e];
	} else {
		*(f4*)(a.Y + (size_t)row * a.OUTP + n0) = o[0][0];
	}
	const size_t sk = ys ? B : 1;  // from one direction (or pair element) of an output to the next
#pragma unroll
	for (int e = 0; e < 4; ++e) {
		const uint32_t n = n0 + e;
		if (n < NOUT) {
			float* je = a.J + (ys ? (size_t)n * K * B + row : ((size_t)row * NOUT + n) * K);
#pragma unroll
			for (int i = 0; i < NT; ++i)
				if ((uint32_t)i < K) je[i * sk] = o[1 + i][0][e];
			float* he = H + (ys ? (size_t)n * K * K * B + row : ((size_t)row * NOUT + n) * K * K);
#pragma unroll
			for (int p = 0; p < NP; ++p) {
				const uint32_t i = hess_pair_i(p), j = hess_pair_j(p);
				if (j < K) {
					he[(i * K + j) * sk] = o[1 + NT + p][0][e];
					if (i != j) he[(j * K + i) * sk] = o[1 + NT + p][0][e];
				}
			}
		}
	}
}

// jvp2_chain (mlp_f32_jvp2.hip) with the pair rows: from the first layer's pre-activations to memory
template <int WT, int NT, int NP>
__device__ __forceinline__ void hess_chain(f4 (&h)[1 + NT + NP][WT], const JvpArgs& a, float* __restrict__ H, uint32_t r, uint32_t q, uint32_t row) {
	constexpr uint32_t W = 16 * WT;
	constexpr int NQ = 1 + NT + NP;
	const float* wl = a.P + (size_t)W * a.IN;
	const uint32_t nt = (a.NOUT + 15) / 16;
	hess_activate<WT, NT, NP>(h, a.act);
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
		hess_activate<WT, NT, NP>(h, a.act);
	}
	// output layer: one column tile at a time, as in jac_chain
	for (uint32_t c0 = 0; c0 < nt; ++c0) {
		f4 o[NQ][1];
#pragma unroll
		for (int i = 0; i < NQ; ++i) o[i][0] = f4{0.0f, 0.0f, 0.0f, 0.0f};
		jac_from_regs<WT, NQ, 1>(wl + (size_t)(16 * c0 + r) * W + 4 * q, 1, h, o);
		hess_activate<1, NT, NP>(o, a.oact);
		hess_store<NT, NP>(o, a, H, 16 * c0 + 4 * q, row);
	}
}

// jvp2_encode_step (mlp_f32_jvp_device.h) with one second-order operand per pair: e[0] the value and e[1 .. NT] the
// tangents, jvp_encode_step's operations in its order, and e[1 + NT + p] the column's
// sum_{d, d'} M[p][d][d'] d^2 e / dx_d dx_d' (level_second_f32), all from the level's one gather. Without directions
// tangent i is unit vector i - 1, and a pair needs only its own term -- the diagonal one for (d, d), the mixed one for
// (d, e) -- the other being exactly zero. Zero on the padding columns.
template <uint32_t D, uint32_t F, int NT, int NP>
__device__ __forceinline__ void hess_encode_step(const JvpArgs& a, uint32_t s, uint32_t q, const float (&x)[D], const float (&dir)[NT][D],
                                                 const float (&M)[NP][D][D], const uint32_t (&prime)[D], f4 (&e)[1 + NT + NP]) {
	constexpr uint32_t NF = F == 2 ? 2 : 4, NLV = 4 / NF, NC = 1u << D;
	constexpr int NQ = 1 + NT + NP;
	const Interp interp = (Interp)a.interp;
	const bool vec = a.vec != 0, hash_grid = a.hash_grid != 0, given = a.V != nullptr;
	const bool diag = interp == Interp::Smoothstep, mixed = interp != Interp::Nearest;
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
		float val[NF], g[D][NF], u2[NP][NF];
		combine_level_f32<NC, NF>(w[u], v[u], val);
#pragma unroll
		for (uint32_t gd = 0; gd < D; ++gd) level_tangent_f32<D, NF>(gd, li[u].scale, p[u], pd[u], v[u], g[gd]);
#pragma unroll
		for (int pr = 0; pr < NP; ++pr) {
			const bool same = hess_pair_i(pr) == hess_pair_j(pr);
			level_second_f32<D, NF>(li[u].scale, p[u], pd[u], pdd[u], v[u], M[pr], diag && (given || same), mixed && (given || !same), u2[pr]);
		}
#pragma unroll
		for (uint32_t f = 0; f < NF; ++f) {
			e[0][u * NF + f] = on[u] ? val[f] : 0.0f;
#pragma unroll
			for (int i = 1; i <= NT; ++i) {
				float t = 0.0f;
				if (!given) {  // unit direction i - 1: selected, so that no register array is indexed at run time
#pragma unroll
					for (uint32_t d = 0; d < D; ++d)
						if ((uint32_t)(i - 1) == d) t = g[d][f];
				} else {
					t = g[0][f] * dir[i - 1][0];
#pragma unroll
					for (uint32_t d = 1; d < D; ++d) t = __builtin_fmaf(g[d][f], dir[i - 1][d], t);
				}
				e[i][u * NF + f] = on[u] ? t : 0.0f;
			}
#pragma unroll
			for (int pr = 0; pr < NP; ++pr) e[1 + NT + pr][u * NF + f] = on[u] ? u2[pr][f] : 0.0f;
		}
	}
}

// The launch behind a grid for NT tangents (directions 0 .. NT - 1, zero past K) and pairs 0 .. NP - 1:
// k_f32_grid_mlp_jvp2's body with a row per pair
template <int WT, uint32_t D, uint32_t F, int NT, int NP>
__device__ __forceinline__ void hess_grid_pass(const HessArgs& b, const float (&x)[D], const uint32_t (&prime)[D], uint32_t r, uint32_t q,
                                               uint32_t row) {
	const JvpArgs& a = b.j;
	constexpr int NQ = 1 + NT + NP;
	const uint32_t ks = a.IN / 16;
	float dir[NT][D];
#pragma unroll
	for (int i = 0; i < NT; ++i)
#pragma unroll
		for (uint32_t d = 0; d < D; ++d)
			dir[i][d] = a.V && (uint32_t)i < a.K ? (a.x_soa ? a.V[((size_t)i * D + d) * a.B + row] : a.V[((size_t)row * a.K + i) * D + d]) : 0.0f;
	// M of pair (i, j), its upper triangle: v_i v_i^T as the Laplacian kernel forms it, else the symmetric part of
	// v_i v_j^T; for the unit vectors a single 1 at (i, i) or a single 1/2 at (i, j)
	float M[NP][D][D];
#pragma unroll
	for (int p = 0; p < NP; ++p) {
		const int i = hess_pair_i(p), j = hess_pair_j(p);
#pragma unroll
		for (uint32_t d = 0; d < D; ++d)
#pragma unroll
			for (uint32_t e = 0; e < D; ++e) {
				float m = (uint32_t)i == d && (uint32_t)j == e ? (i == j ? 1.0f : 0.5f) : 0.0f;
				if (a.V) m = i == j ? dir[i][d] * dir[i][e] : 0.5f * (dir[i][d] * dir[j][e] + dir[j][d] * dir[i][e]);
				M[p][d][e] = m;
			}
	}
	// the whole operand, before an accumulator is live
	f4 e[NQ][JVP_MAX_KSTEPS];
#pragma unroll
	for (uint32_t s = 0; s < JVP_MAX_KSTEPS; ++s) {
		if (s < ks) {
			f4 es[NQ];
			hess_encode_step<D, F, NT, NP>(a, s, q, x, dir, M, prime, es);
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
	hess_chain<WT, NT, NP>(h, a, b.H, r, q, row);
}

// The same behind an Identity row (or for a network alone): the encoding is linear, so every pair row enters the first
// gate as zero
template <int WT, int NT, int NP>
__device__ __forceinline__ void hess_identity_pass(const HessArgs& b, uint32_t r, uint32_t q, uint32_t row) {
	const JvpArgs& a = b.j;
	constexpr int NQ = 1 + NT + NP;
	f4 t[1 + NT][WT], h[NQ][WT];
	jac_identity_layer<WT, 1 + NT>(t, a.P, a.X, a.x_soa != 0, a.V, a.B, a.D, a.K, a.IN, a.scale, a.offset, r, q, row, 0);
#pragma unroll
	for (int c = 0; c < WT; ++c) {
#pragma unroll
		for (int i = 0; i <= NT; ++i) h[i][c] = t[i][c];
#pragma unroll
		for (int i = 1 + NT; i < NQ; ++i) h[i][c] = f4{0.0f, 0.0f, 0.0f, 0.0f};
	}
	hess_chain<WT, NT, NP>(h, a, b.H, r, q, row);
}

// Grid B / 64. W = 16 WT, D input dimensions and F features per level of the grid in front. K is wave-uniform.
template <int WT, uint32_t D, uint32_t F>
__global__ __launch_bounds__(256) void k_f32_grid_mlp_hessian(const HessArgs b) {
	const JvpArgs& a = b.j;
	const uint32_t lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;
	const uint32_t row = (blockIdx.x * 4 + (threadIdx.x >> 6)) * JAC_ROWS_PER_WAVE + r;
	if (row >= a.B) return;
	float x[D];
#pragma unroll
	for (uint32_t d = 0; d < D; ++d) x[d] = a.x_soa ? a.X[(size_t)d * a.B + row] : a.X[(size_t)row * D + d];
	uint32_t prime[D];
	hash_primes<D>((HashType)a.hash, prime);
	if (a.K <= 2) hess_grid_pass<WT, D, F, 2, 3>(b, x, prime, r, q, row);
	else hess_grid_pass<WT, D, F, 3, 6>(b, x, prime, r, q, row);
}

template <int WT>
__global__ __launch_bounds__(256) void k_f32_identity_mlp_hessian(const HessArgs b) {
	const JvpArgs& a = b.j;
	const uint32_t lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;
	const uint32_t row = (blockIdx.x * 4 + (threadIdx.x >> 6)) * JAC_ROWS_PER_WAVE + r;
	if (row >= a.B) return;
	if (a.K <= 2) hess_identity_pass<WT, 2, 3>(b, r, q, row);
	else hess_identity_pass<WT, 3, 6>(b, r, q, row);
}

template <int WT>
void hessian_width(hipStream_t st, const HessArgs& a, bool grid, uint32_t D, uint32_t F) {
	const dim3 blocks(a.j.B / JAC_ROWS_PER_BLOCK), block(256);
	if (!grid) {
		hipLaunchKernelGGL((k_f32_identity_mlp_hessian<WT>), blocks, block, 0, st, a);
		return;
	}
	switch (D * 16 + F) {
		case 2 * 16 + 2: hipLaunchKernelGGL((k_f32_grid_mlp_hessian<WT, 2, 2>), blocks, block, 0, st, a); break;
		case 2 * 16 + 4: hipLaunchKernelGGL((k_f32_grid_mlp_hessian<WT, 2, 4>), blocks, block, 0, st, a); break;
		case 2 * 16 + 8: hipLaunchKernelGGL((k_f32_grid_mlp_hessian<WT, 2, 8>), blocks, block, 0, st, a); break;
		case 3 * 16 + 2: hipLaunchKernelGGL((k_f32_grid_mlp_hessian<WT, 3, 2>), blocks, block, 0, st, a); break;
		case 3 * 16 + 4: hipLaunchKernelGGL((k_f32_grid_mlp_hessian<WT, 3, 4>), blocks, block, 0, st, a); break;
		default: hipLaunchKernelGGL((k_f32_grid_mlp_hessian<WT, 3, 8>), blocks, block, 0, st, a); break;
	}
}

}  // namespace

uint32_t f32_mlp_hessian_max_directions(uint32_t W) { return f32_mlp_jvp2_width_ok(W) ? (uint32_t)HESS_MAX_DIRECTIONS : 0u; }

void launch_f32_mlp_hessian(hipStream_t st, uint32_t B, uint32_t D, uint32_t IN, uint32_t W, uint32_t NH, uint32_t OUTP, uint32_t n_out,
                            const float* params, const float* x, const float* directions, uint32_t n_directions, bool x_soa, float* y, float* jvp,
                            float* hessian, bool y_soa, int act, int out_act, const GridCall* grid, const float* table, float scale,
                            float offset) {
	const char* what = "fp32 input Hessian";
	TCNN_CHECK(f32_mlp_jvp2_width_ok(W), std::string(what) + ": the width must be 16, 32 or 64");
	TCNN_CHECK(NH >= 1, std::string(what) + ": at least one hidden layer");
	TCNN_CHECK(IN && OUTP && IN % 16 == 0 && OUTP % 16 == 0, std::string(what) + ": widths must be multiples of 16");
	TCNN_CHECK(B % 128 == 0, std::string(what) + ": batch must be a multiple of 128");
	TCNN_CHECK(n_out && n_out <= OUTP && OUTP - n_out < 16, std::string(what) + ": the padded output width must be the next multiple of 16");
	TCNN_CHECK(act != ACT_SINE && out_act != ACT_SINE, std::string(what) + ": Sine has no backward from its forward value");
	TCNN_CHECK(directions ? n_directions >= 1 : n_directions == D, std::string(what) + ": at least one direction, or the input width for the unit vectors");
	TCNN_CHECK(n_directions <= (uint32_t)HESS_MAX_DIRECTIONS, std::string(what) + ": at most 3 directions");
	HessArgs b{};
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
	TCNN_CHECK(params && x && y && jvp && hessian && (!grid || table),
	           std::string(what) + ": the parameters, the inputs, the output, the product or the Hessian are missing");
	a.B = B, a.D = D, a.IN = IN, a.NH = NH, a.OUTP = OUTP, a.NOUT = n_out, a.K = n_directions;
	a.P = params, a.X = x, a.V = directions, a.Y = y, a.J = jvp;
	b.H = hessian;
	a.x_soa = x_soa ? 1u : 0u, a.y_soa = y_soa ? 1u : 0u;
	a.act = act, a.oact = out_act;
	a.scale = scale, a.offset = offset;
	const uint32_t F = grid ? grid->F : 0;
	switch (W) {
		case 16: hessian_width<1>(st, b, grid != nullptr, D, F); break;
		case 32: hessian_width<2>(st, b, grid != nullptr, D, F); break;
		default: hessian_width<4>(st, b, grid != nullptr, D, F); break;
	}
	TCNN_HIP_CHECK(hipGetLastError());
}

}  // namespace tcnn_amd
