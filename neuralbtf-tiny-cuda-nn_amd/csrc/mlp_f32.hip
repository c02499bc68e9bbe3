// mlp_f32.hip -- layer-wise fp32 MLP engine for gfx950 (an fp32 network module: Network /
// NetworkWithInputEncoding dtype = float32). Parameters, activations, dL/dy, dL/dparams and dL/dinput are
// fp32; the products run on the f32 MFMA v_mfma_f32_16x16x4_f32 (exact f32 inputs, f32 accumulation) and
// nothing is narrowed to fp16. Every width is a multiple of 16, so every matrix is whole 16 x 16 tiles.
//
// Operand scheme. The MFMA takes A[i][k] in lane (i = l & 15, k = l >> 4) and B[k][j] in lane
// (k = l >> 4, j = l & 15), one float each, and leaves D[4 (l >> 4) + e][l & 15] in register e. Lane
// (r = l & 15, q = l >> 4) therefore feeds FOUR consecutive MFMAs from one 16-byte load of a row that
// is contiguous along the contraction index: it loads elements [r][16 s + 4 q .. + 3] of both operands
// and MFMA j takes element j of each, which sums k = 16 s + 4 q + j over q -- a permuted but complete
// order of the 16 indices of step s. The forward has both operands in that form (X [B][K] and W [N][K]);
// the backward kernels have one (dY rows, along n) or none (the weight gradient contracts over the
// batch) and read the other operand as four 4-byte loads that are contiguous across the 16 lanes r.
// All three kernels put the matrix whose rows become the OUTPUT's contiguous index into A's place, so a
// lane's four accumulator registers are four consecutive elements of one output row: 16-byte stores for
// the forward and the backward-data kernel.
//
// Weights are read through the vector L1 / L2, not staged in LDS: a workgroup's four waves read the
// same <= 64 KiB tile columns of a matrix that every other workgroup reads too, so after first touch
// they are L2 (and mostly L1) hits, and no kernel here uses LDS or a barrier at all.
//
// Each wave owns 2 row tiles x up to 4 column tiles (forward, backward data) or 2 x 2 tiles (weight
// gradient): at least two independent accumulators, as the MFMA's dependent-accumulator latency asks.
//
// The second-order input gradient (backward_backward_input) adds two kernels on the same scheme: the tangent
// layer is the forward product with a gating epilogue, the curvature layer the backward-data product with a fused
// epilogue; its weight gradients run k_f32_wgrad as it is.
#include "act_f32.h"
#include "kernels.h"

namespace tcnn_amd {

static_assert(AF32_NONE == ACT_NONE && AF32_RELU == ACT_RELU && AF32_LEAKY_RELU == ACT_LEAKY_RELU && AF32_EXPONENTIAL == ACT_EXPONENTIAL &&
                  AF32_SINE == ACT_SINE && AF32_SIGMOID == ACT_SIGMOID && AF32_SQUAREPLUS == ACT_SQUAREPLUS &&
                  AF32_SOFTPLUS == ACT_SOFTPLUS && AF32_TANH == ACT_TANH,
              "act_f32.h restates the activation codes of kernels.h");

namespace {

__device__ __forceinline__ f4 mfma4(float a, float b, f4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// The rare activations stay out of line, as in the fp16 layer-wise engine: the MFMA loops inline None / ReLU only.
__device__ __noinline__ float act_fwd_f32_ool(int a, float x) { return act_fwd_f32(a, x); }
__device__ __noinline__ float act_bwd_f32_ool(int a, float g, float y) { return act_bwd_f32(a, g, y); }
__device__ __noinline__ float act_factor2_f32_ool(int a, float y) { return act_factor2_f32(a, y); }

__device__ __forceinline__ float fwd_act(int a, float x) {
	if (a == ACT_NONE) return x;
	if (a == ACT_RELU) return x > 0.0f ? x : 0.0f;
	return act_fwd_f32_ool(a, x);
}
__device__ __forceinline__ float bwd_act(int a, float g, float y) {
	if (a == ACT_NONE) return g;
	if (a == ACT_RELU) return y > 0.0f ? g : 0.0f;
	return act_bwd_f32_ool(a, g, y);
}
__device__ __forceinline__ f4 bwd_act4(int a, f4 g, const float* __restrict__ y) {
	if (a == ACT_NONE) return g;
	const f4 yv = *(const f4*)y;
	f4 o;
#pragma unroll
	for (int e = 0; e < 4; ++e) o[e] = bwd_act(a, g[e], yv[e]);
	return o;
}

constexpr uint32_t ROWS_PER_WAVE = 32, ROWS_PER_BLOCK = 128, COLS_PER_BLOCK = 64;

// Y[B][N] = act(X[B][K] W^T), W [N][K]. Grid (B / 128, ceil(N / 64)); wave: rows [row0, row0 + 32), up to 4 column tiles.
__global__ __launch_bounds__(256) void k_f32_layer_fwd(uint32_t B, uint32_t N, uint32_t K, const float* __restrict__ W,
                                                        const float* __restrict__ X, float* __restrict__ Y, int act) {
	const uint32_t lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;
	const uint32_t row0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * ROWS_PER_WAVE;
	const uint32_t n0 = blockIdx.y * COLS_PER_BLOCK;
	if (row0 >= B || n0 >= N) return;
	const uint32_t nct = min(4u, (N - n0) / 16);
	f4 acc[2][4];
#pragma unroll
	for (int t = 0; t < 2; ++t)
#pragma unroll
		for (int c = 0; c < 4; ++c) acc[t][c] = f4{0.0f, 0.0f, 0.0f, 0.0f};
	const float* x0 = X + (size_t)(row0 + r) * K + 4 * q;
	const float* x1 = x0 + (size_t)16 * K;
	const float* wp = W + (size_t)(n0 + r) * K + 4 * q;
	for (uint32_t s = 0; s < K; s += 16) {
		const f4 a0 = *(const f4*)(x0 + s), a1 = *(const f4*)(x1 + s);
#pragma unroll
		for (int c = 0; c < 4; ++c) {
			if ((uint32_t)c < nct) {
				const f4 w = *(const f4*)(wp + (size_t)c * 16 * K + s);
#pragma unroll
				for (int j = 0; j < 4; ++j) {
					acc[0][c] = mfma4(w[j], a0[j], acc[0][c]);
					acc[1][c] = mfma4(w[j], a1[j], acc[1][c]);
				}
			}
		}
	}
	// D[neuron 4 q + e][row r]: four consecutive neurons of one row per lane
#pragma unroll
	for (int t = 0; t < 2; ++t)
#pragma unroll
		for (int c = 0; c < 4; ++c) {
			if ((uint32_t)c < nct) {
				f4 o;
#pragma unroll
				for (int e = 0; e < 4; ++e) o[e] = fwd_act(act, acc[t][c][e]);
				*(f4*)(Y + (size_t)(row0 + 16 * t + r) * N + n0 + 16 * c + 4 * q) = o;
			}
		}
}

// dX[B][K] = (dY o act'(Yv)) W, W [N][K]; Yv: the forward value beside dY (unread for act None). The
// transfer is applied to the dY operand as it is loaded. Grid (B / 128, ceil(K / 64)).
__global__ __launch_bounds__(256) void k_f32_layer_bwd(uint32_t B, uint32_t N, uint32_t K, const float* __restrict__ W,
                                                        const float* __restrict__ dY, const float* __restrict__ Yv, int act,
                                                        float* __restrict__ dX) {
	const uint32_t lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;
	const uint32_t row0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * ROWS_PER_WAVE;
	const uint32_t k0 = blockIdx.y * COLS_PER_BLOCK;
	if (row0 >= B || k0 >= K) return;
	const uint32_t kct = min(4u, (K - k0) / 16);
	f4 acc[2][4];
#pragma unroll
	for (int t = 0; t < 2; ++t)
#pragma unroll
		for (int c = 0; c < 4; ++c) acc[t][c] = f4{0.0f, 0.0f, 0.0f, 0.0f};
	const size_t g_off0 = (size_t)(row0 + r) * N + 4 * q, g_off1 = g_off0 + (size_t)16 * N;
	const float* wp = W + (size_t)(4 * q) * K + k0 + r;  // W[16 s + 4 q + j][k0 + 16 c + r]
	for (uint32_t s = 0; s < N; s += 16) {
		const f4 g0 = bwd_act4(act, *(const f4*)(dY + g_off0 + s), Yv + g_off0 + s);
		const f4 g1 = bwd_act4(act, *(const f4*)(dY + g_off1 + s), Yv + g_off1 + s);
#pragma unroll
		for (int c = 0; c < 4; ++c) {
			if ((uint32_t)c < kct) {
#pragma unroll
				for (int j = 0; j < 4; ++j) {
					const float w = wp[(size_t)(s + j) * K + 16 * c];
					acc[0][c] = mfma4(w, g0[j], acc[0][c]);
					acc[1][c] = mfma4(w, g1[j], acc[1][c]);
				}
			}
		}
	}
#pragma unroll
	for (int t = 0; t < 2; ++t)
#pragma unroll
		for (int c = 0; c < 4; ++c)
			if ((uint32_t)c < kct) *(f4*)(dX + (size_t)(row0 + 16 * t + r) * K + k0 + 16 * c + 4 * q) = acc[t][c];
}

// partial[slab][N][K] = sum over the slab's rows b of (dY o act'(Yv))[b][n] X[b][k]. Grid (ceil(N / 64) *
// ceil(K / 64), slabs); wave (wn, wk) of a workgroup owns the 32 x 32 tile (2 x 2 accumulators) at
// (64 bn + 32 wn, 64 bk + 32 wk) and runs over the slab's rows alone: no cross-wave sum, no atomics.
__global__ __launch_bounds__(256) void k_f32_wgrad(uint32_t B, uint32_t N, uint32_t K, const float* __restrict__ dY,
                                                    const float* __restrict__ Yv, int act, const float* __restrict__ X,
                                                    float* __restrict__ partial, uint32_t rows_per_slab) {
	const uint32_t lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4, wave = threadIdx.x >> 6;
	const uint32_t kb = (K + 63) / 64;
	const uint32_t n0 = (blockIdx.x / kb) * 64 + (wave & 1) * 32, k0 = (blockIdx.x % kb) * 64 + (wave >> 1) * 32;
	if (n0 >= N || k0 >= K) return;
	const uint32_t nnt = min(2u, (N - n0) / 16), nkt = min(2u, (K - k0) / 16);
	const uint32_t b0 = blockIdx.y * rows_per_slab, b1 = min(B, b0 + rows_per_slab);
	f4 acc[2][2];
#pragma unroll
	for (int t = 0; t < 2; ++t)
#pragma unroll
		for (int c = 0; c < 2; ++c) acc[t][c] = f4{0.0f, 0.0f, 0.0f, 0.0f};
	for (uint32_t b = b0; b < b1; b += 16) {
		float g[2][4], x[2][4];
#pragma unroll
		for (int t = 0; t < 2; ++t)
#pragma unroll
			for (int j = 0; j < 4; ++j) {
				g[t][j] = 0.0f;
				if ((uint32_t)t < nnt) {
					const size_t o = (size_t)(b + 4 * q + j) * N + n0 + 16 * t + r;
					g[t][j] = act == ACT_NONE ? dY[o] : bwd_act(act, dY[o], Yv[o]);
				}
			}
#pragma unroll
		for (int c = 0; c < 2; ++c)
#pragma unroll
			for (int j = 0; j < 4; ++j) x[c][j] = (uint32_t)c < nkt ? X[(size_t)(b + 4 * q + j) * K + k0 + 16 * c + r] : 0.0f;
#pragma unroll
		for (int j = 0; j < 4; ++j)
#pragma unroll
			for (int t = 0; t < 2; ++t)
#pragma unroll
				for (int c = 0; c < 2; ++c) acc[t][c] = mfma4(g[t][j], x[c][j], acc[t][c]);
	}
	float* out = partial + (size_t)blockIdx.y * N * K;
#pragma unroll
	for (int t = 0; t < 2; ++t)
#pragma unroll
		for (int c = 0; c < 2; ++c)
			if ((uint32_t)t < nnt && (uint32_t)c < nkt) {
#pragma unroll
				for (int e = 0; e < 4; ++e) out[(size_t)(n0 + 16 * t + 4 * q + e) * K + k0 + 16 * c + r] = acc[t][c][e];
			}
}

// ---- the second-order input gradient (NetworkF32Host::backward_backward_input) ----
// The two products again as helpers (the first-order kernels above keep their loops as they are: their register
// allocation is the recorded one).
// The forward product of one wave: acc[t][c] = D[neuron 4 q + e][row r] of X W^T for rows 16 t + r of x0 and
// neurons 16 c + .. of wp (both already offset to the lane's row and its 4 q), nct column tiles.
__device__ __forceinline__ void fwd_tiles(uint32_t K, uint32_t nct, const float* __restrict__ x0, const float* __restrict__ wp, f4 (&acc)[2][4]) {
#pragma unroll
	for (int t = 0; t < 2; ++t)
#pragma unroll
		for (int c = 0; c < 4; ++c) acc[t][c] = f4{0.0f, 0.0f, 0.0f, 0.0f};
	const float* x1 = x0 + (size_t)16 * K;
	for (uint32_t s = 0; s < K; s += 16) {
		const f4 a0 = *(const f4*)(x0 + s), a1 = *(const f4*)(x1 + s);
#pragma unroll
		for (int c = 0; c < 4; ++c) {
			if ((uint32_t)c < nct) {
				const f4 w = *(const f4*)(wp + (size_t)c * 16 * K + s);
#pragma unroll
				for (int j = 0; j < 4; ++j) {
					acc[0][c] = mfma4(w[j], a0[j], acc[0][c]);
					acc[1][c] = mfma4(w[j], a1[j], acc[1][c]);
				}
			}
		}
	}
}

// The backward-data product of one wave: acc[t][c] = D[column 4 q + e][row r] of (dY o act'(Yv)) W for rows
// 16 t + r at g_off0 (the lane's row and its 4 q) and columns 16 c + .. of wp = &W[4 q][k0 + r], kct column tiles.
__device__ __forceinline__ void bwd_tiles(uint32_t N, uint32_t K, uint32_t kct, size_t g_off0, const float* __restrict__ wp,
                                          const float* __restrict__ dY, const float* __restrict__ Yv, int act, f4 (&acc)[2][4]) {
#pragma unroll
	for (int t = 0; t < 2; ++t)
#pragma unroll
		for (int c = 0; c < 4; ++c) acc[t][c] = f4{0.0f, 0.0f, 0.0f, 0.0f};
	const size_t g_off1 = g_off0 + (size_t)16 * N;
	for (uint32_t s = 0; s < N; s += 16) {  // W[16 s + 4 q + j][k0 + 16 c + r]
		const f4 g0 = bwd_act4(act, *(const f4*)(dY + g_off0 + s), Yv + g_off0 + s);
		const f4 g1 = bwd_act4(act, *(const f4*)(dY + g_off1 + s), Yv + g_off1 + s);
#pragma unroll
		for (int c = 0; c < 4; ++c) {
			if ((uint32_t)c < kct) {
#pragma unroll
				for (int j = 0; j < 4; ++j) {
					const float w = wp[(size_t)(s + j) * K + 16 * c];
					acc[0][c] = mfma4(w, g0[j], acc[0][c]);
					acc[1][c] = mfma4(w, g1[j], acc[1][c]);
				}
			}
		}
	}
}

// Tangent layer: the forward kernel with a gating epilogue. With T = X W^T (never stored), Y = T o act'(Yv) and, for an
// activation with curvature (R given), R = (T o D) o act''(Yv): Yv the layer's forward value, D the first-order
// dL/d(that value). Grid and tile ownership are the forward's.
__global__ __launch_bounds__(256) void k_f32_layer_tangent(uint32_t B, uint32_t N, uint32_t K, const float* __restrict__ W,
                                                            const float* __restrict__ X, const float* __restrict__ Yv, int act,
                                                            float* __restrict__ Y, const float* __restrict__ D, float* __restrict__ R) {
	const uint32_t lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;
	const uint32_t row0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * ROWS_PER_WAVE;
	const uint32_t n0 = blockIdx.y * COLS_PER_BLOCK;
	if (row0 >= B || n0 >= N) return;
	const uint32_t nct = min(4u, (N - n0) / 16);
	f4 acc[2][4];
	fwd_tiles(K, nct, X + (size_t)(row0 + r) * K + 4 * q, W + (size_t)(n0 + r) * K + 4 * q, acc);
#pragma unroll
	for (int t = 0; t < 2; ++t)
#pragma unroll
		for (int c = 0; c < 4; ++c) {
			if ((uint32_t)c < nct) {
				const size_t o = (size_t)(row0 + 16 * t + r) * N + n0 + 16 * c + 4 * q;
				*(f4*)(Y + o) = bwd_act4(act, acc[t][c], Yv + o);
				if (R) {
					const f4 yv = *(const f4*)(Yv + o), d = *(const f4*)(D + o);
					f4 rr;
#pragma unroll
					for (int e = 0; e < 4; ++e) rr[e] = (acc[t][c][e] * d[e]) * act_factor2_f32_ool(act, yv[e]);
					*(f4*)(R + o) = rr;
				}
			}
		}
}

// Curvature layer: the backward-data kernel with a fused epilogue, Qb = (Q W) o act'(Yb) + Rb (Yb: the forward value
// of the layer below, unread for act None; Rb nullable). Qb may be Rb: a lane reads and writes its own elements only,
// so neither is __restrict__. Grid and tile ownership are the backward-data kernel's.
__global__ __launch_bounds__(256) void k_f32_layer_curvature(uint32_t B, uint32_t N, uint32_t K, const float* __restrict__ W,
                                                              const float* __restrict__ Q, const float* __restrict__ Yb, int act,
                                                              const float* Rb, float* Qb) {
	const uint32_t lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;
	const uint32_t row0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * ROWS_PER_WAVE;
	const uint32_t k0 = blockIdx.y * COLS_PER_BLOCK;
	if (row0 >= B || k0 >= K) return;
	const uint32_t kct = min(4u, (K - k0) / 16);
	f4 acc[2][4];
	bwd_tiles(N, K, kct, (size_t)(row0 + r) * N + 4 * q, W + (size_t)(4 * q) * K + k0 + r, Q, Q, ACT_NONE, acc);
#pragma unroll
	for (int t = 0; t < 2; ++t)
#pragma unroll
		for (int c = 0; c < 4; ++c)
			if ((uint32_t)c < kct) {
				const size_t o = (size_t)(row0 + 16 * t + r) * K + k0 + 16 * c + 4 * q;
				f4 v = bwd_act4(act, acc[t][c], Yb + o);
				if (Rb) {
					const f4 rb = *(const f4*)(Rb + o);
#pragma unroll
					for (int e = 0; e < 4; ++e) v[e] += rb[e];
				}
				*(f4*)(Qb + o) = v;
			}
}

// Identity in front: dL2/dD_0 = scale * dL2/d(dx) in the value columns, 0 in the padding
__global__ __launch_bounds__(256) void k_f32_identity_tangent(uint32_t B, uint32_t D, uint32_t width, float scale,
                                                               const float* __restrict__ ux, float* __restrict__ u0) {
	const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= (size_t)B * width) return;
	const uint32_t b = (uint32_t)(i / width), j = (uint32_t)(i % width);
	u0[i] = j < D ? ux[(size_t)b * D + j] * scale : 0.0f;
}

__global__ __launch_bounds__(256) void k_f32_add(size_t n, float* __restrict__ dst, const float* __restrict__ src) {
	const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n) dst[i] += src[i];
}

void check_shape(uint32_t B, uint32_t N, uint32_t K, const char* what) {
	TCNN_CHECK(N && K && N % 16 == 0 && K % 16 == 0, std::string(what) + ": widths must be multiples of 16");
	TCNN_CHECK(B % ROWS_PER_BLOCK == 0, std::string(what) + ": batch must be a multiple of 128");
}

}  // namespace

void launch_f32_layer_fwd(hipStream_t st, uint32_t B, uint32_t N, uint32_t K, const float* w, const float* x, float* y, int act) {
	check_shape(B, N, K, "fp32 layer forward");
	if (!B) return;
	hipLaunchKernelGGL(k_f32_layer_fwd, dim3(B / ROWS_PER_BLOCK, div_round_up(N, COLS_PER_BLOCK)), dim3(256), 0, st, B, N, K, w, x, y, act);
	TCNN_HIP_CHECK(hipGetLastError());
}

void launch_f32_layer_bwd(hipStream_t st, uint32_t B, uint32_t N, uint32_t K, const float* w, const float* dy, const float* yv, int act,
                          float* dx) {
	check_shape(B, N, K, "fp32 layer backward");
	TCNN_CHECK(act != ACT_SINE, "fp32 layer backward: Sine has no backward from its forward value");
	TCNN_CHECK(act == ACT_NONE || yv, "fp32 layer backward: the forward value is missing");
	if (!B) return;
	hipLaunchKernelGGL(k_f32_layer_bwd, dim3(B / ROWS_PER_BLOCK, div_round_up(K, COLS_PER_BLOCK)), dim3(256), 0, st, B, N, K, w, dy,
	                   act == ACT_NONE ? dy : yv, act, dx);
	TCNN_HIP_CHECK(hipGetLastError());
}

void launch_f32_layer_tangent(hipStream_t st, uint32_t B, uint32_t N, uint32_t K, const float* w, const float* x, const float* yv, int act,
                              float* y, const float* d, float* r) {
	check_shape(B, N, K, "fp32 tangent layer");
	TCNN_CHECK(act != ACT_SINE, "fp32 tangent layer: Sine has no backward from its forward value");
	TCNN_CHECK(act == ACT_NONE || yv, "fp32 tangent layer: the forward value is missing");
	TCNN_CHECK(!r || (d && yv && f32_act_has_curvature(act)), "fp32 tangent layer: the curvature output needs dL/dy and an activation that has one");
	if (!B) return;
	hipLaunchKernelGGL(k_f32_layer_tangent, dim3(B / ROWS_PER_BLOCK, div_round_up(N, COLS_PER_BLOCK)), dim3(256), 0, st, B, N, K, w, x,
	                   act == ACT_NONE ? x : yv, act, y, d, r);
	TCNN_HIP_CHECK(hipGetLastError());
}

void launch_f32_layer_curvature(hipStream_t st, uint32_t B, uint32_t N, uint32_t K, const float* w, const float* q, const float* yv_below,
                                int act_below, const float* r_below, float* q_below) {
	check_shape(B, N, K, "fp32 curvature layer");
	TCNN_CHECK(act_below != ACT_SINE, "fp32 curvature layer: Sine has no backward from its forward value");
	TCNN_CHECK(act_below == ACT_NONE || yv_below, "fp32 curvature layer: the forward value is missing");
	if (!B) return;
	hipLaunchKernelGGL(k_f32_layer_curvature, dim3(B / ROWS_PER_BLOCK, div_round_up(K, COLS_PER_BLOCK)), dim3(256), 0, st, B, N, K, w, q,
	                   act_below == ACT_NONE ? q : yv_below, act_below, r_below, q_below);
	TCNN_HIP_CHECK(hipGetLastError());
}

void launch_f32_identity_tangent(hipStream_t st, uint32_t B, uint32_t D, uint32_t width, float scale, const float* u_x, float* u0) {
	TCNN_CHECK(D <= width, "fp32 identity tangent: the row is narrower than the input");
	if (!B || !width) return;
	hipLaunchKernelGGL(k_f32_identity_tangent, dim3((uint32_t)div_round_up((size_t)B * width, (size_t)256)), dim3(256), 0, st, B, D, width,
	                   scale, u_x, u0);
	TCNN_HIP_CHECK(hipGetLastError());
}

void launch_f32_add(hipStream_t st, size_t n, float* dst, const float* src) {
	if (!n) return;
	hipLaunchKernelGGL(k_f32_add, dim3((uint32_t)div_round_up(n, (size_t)256)), dim3(256), 0, st, n, dst, src);
	TCNN_HIP_CHECK(hipGetLastError());
}

// Rows of one slab: 256 (one batch granule) while that gives at most 256 slabs, else the next multiple
// of 256 that does; the slab count, not the device, decides the order of every sum.
uint32_t f32_wgrad_slab_rows(uint32_t B) {
	const uint32_t granules = div_round_up(B, 256);
	return div_round_up(granules, 256) * 256;
}
uint32_t f32_wgrad_n_slabs(uint32_t B) { return B ? div_round_up(B, f32_wgrad_slab_rows(B)) : 0; }

void launch_f32_wgrad(hipStream_t st, uint32_t B, uint32_t N, uint32_t K, const float* dy, const float* yv, int act, const float* x,
                      float* partial) {
	check_shape(B, N, K, "fp32 weight gradient");
	TCNN_CHECK(act != ACT_SINE, "fp32 weight gradient: Sine has no backward from its forward value");
	TCNN_CHECK(act == ACT_NONE || yv, "fp32 weight gradient: the forward value is missing");
	if (!B) return;
	const uint32_t tiles = div_round_up(N, 64) * div_round_up(K, 64);
	hipLaunchKernelGGL(k_f32_wgrad, dim3(tiles, f32_wgrad_n_slabs(B)), dim3(256), 0, st, B, N, K, dy, act == ACT_NONE ? dy : yv, act, x,
	                   partial, f32_wgrad_slab_rows(B));
	TCNN_HIP_CHECK(hipGetLastError());
}

}  // namespace tcnn_amd
