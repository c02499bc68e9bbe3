// optimizers.hip -- the elementwise optimizers beside Adam (reference optimizers/sgd.h, ema.h,
// lookahead.h, batched.h) and the torch optimizer's Adam on a caller's tensors (k_adam_torch) as
// streaming passes over the parameter vector; the arithmetic is in optim_device.h and adam_device.h. Every kernel: 256 threads, 8 consecutive parameters per thread (one 16-byte access
// per fp16 array, two per fp32 array), so a workgroup spans OPT_SPAN = 2048 parameters; the last
// thread with work finishes a count that is no multiple of 8 one parameter at a time. fp32
// arithmetic, no LDS, no atomics, nothing that depends on the batch. Buffers are whole allocations
// (16-byte aligned).
#include "adam_device.h"
#include "optim_device.h"
#include "optimizers.h"

namespace tcnn_amd {

namespace {

constexpr uint32_t OPT_PER_THREAD = 8;
constexpr uint32_t OPT_THREADS = 256;
constexpr uint32_t OPT_SPAN = OPT_PER_THREAD * OPT_THREADS;

struct F8 {
	float v[8];
};
__device__ __forceinline__ F8 load_f8(const float* p) {
	const f4 a = *(const f4*)p, b = *(const f4*)(p + 4);
	return F8{{a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w}};
}
__device__ __forceinline__ void store_f8(float* p, const F8& x) {
	*(f4*)p = f4{x.v[0], x.v[1], x.v[2], x.v[3]};
	*(f4*)(p + 4) = f4{x.v[4], x.v[5], x.v[6], x.v[7]};
}
__device__ __forceinline__ h8 round_h8(const F8& x) {
	h8 h;
#pragma unroll
	for (int r = 0; r < 8; ++r) h[r] = f16_rn(x.v[r]);
	return h;
}

// this thread's parameters [i0, i0 + 8): `full` when all of them exist, else [i0, n) one at a time
#define OPT_RANGE                                                                             \
	const size_t i0 = ((size_t)blockIdx.x * OPT_THREADS + threadIdx.x) * OPT_PER_THREAD; \
	if (i0 >= n) return;                                                                  \
	const bool full = i0 + OPT_PER_THREAD <= n;

// fp32 gradient sums -> the fp16 gradients the optimizers read
__global__ __launch_bounds__(256) void k_grad_f16(const float* __restrict__ g32, _Float16* __restrict__ g16, float grad_scale, size_t n) {
	OPT_RANGE
	if (full) {
		F8 g = load_f8(g32 + i0);
#pragma unroll
		for (int r = 0; r < 8; ++r) g.v[r] = g.v[r] * grad_scale;
		*(h8*)(g16 + i0) = round_h8(g);
	} else {
		for (size_t i = i0; i < n; ++i) g16[i] = optim_grad16(g32[i], grad_scale);
	}
}

__global__ __launch_bounds__(256) void k_sgd(float* __restrict__ w32, _Float16* __restrict__ w16, const _Float16* __restrict__ g16,
                                              float loss_scale, float lr, float l2_reg, size_t n) {
	OPT_RANGE
	if (full) {
		F8 w = load_f8(w32 + i0);
		const h8 g = *(const h8*)(g16 + i0);
#pragma unroll
		for (int r = 0; r < 8; ++r) w.v[r] = sgd_update(w.v[r], g[r], loss_scale, lr, l2_reg);
		store_f8(w32 + i0, w);
		*(h8*)(w16 + i0) = round_h8(w);
	} else {
		for (size_t i = i0; i < n; ++i) {
			const float nw = sgd_update(w32[i], g16[i], loss_scale, lr, l2_reg);
			w32[i] = nw;
			w16[i] = f16_rn(nw);
		}
	}
}

// FULL: tmp carries the average in fp32 and weights_ema is its rounding; else (tmp unused) the previous
// value is the fp16 weights_ema itself. Two kernels, so a profile tells the two precisions apart.
template <bool FULL>
__global__ __launch_bounds__(256) void k_ema(const _Float16* __restrict__ w16, _Float16* __restrict__ ema, float* __restrict__ tmp,
                                              float decay, float debias_old, float debias_new, size_t n) {
	OPT_RANGE
	if (full) {
		const h8 w = *(const h8*)(w16 + i0);
		F8 p;
		if (FULL) {
			p = load_f8(tmp + i0);
		} else {
			const h8 e = *(const h8*)(ema + i0);
#pragma unroll
			for (int r = 0; r < 8; ++r) p.v[r] = (float)e[r];
		}
#pragma unroll
		for (int r = 0; r < 8; ++r) p.v[r] = ema_update(p.v[r], w[r], decay, debias_old, debias_new);
		if (FULL) store_f8(tmp + i0, p);
		*(h8*)(ema + i0) = round_h8(p);
	} else {
		for (size_t i = i0; i < n; ++i) {
			const float v = ema_update(FULL ? tmp[i] : (float)ema[i], w16[i], decay, debias_old, debias_new);
			if (FULL) tmp[i] = v;
			ema[i] = f16_rn(v);
		}
	}
}

__global__ __launch_bounds__(256) void k_lookahead(float* __restrict__ w32, _Float16* __restrict__ w16, _Float16* __restrict__ look,
                                                    float alpha, size_t n) {
	OPT_RANGE
	if (full) {
		F8 w = load_f8(w32 + i0);
		const h8 l = *(const h8*)(look + i0);
#pragma unroll
		for (int r = 0; r < 8; ++r) w.v[r] = lookahead_blend(l[r], w.v[r], alpha);
		store_f8(w32 + i0, w);
		const h8 h = round_h8(w);
		*(h8*)(look + i0) = h;
		*(h8*)(w16 + i0) = h;
	} else {
		for (size_t i = i0; i < n; ++i) {
			const float nw = lookahead_blend(look[i], w32[i], alpha);
			w32[i] = nw;
			look[i] = w16[i] = f16_rn(nw);
		}
	}
}

__global__ __launch_bounds__(256) void k_batched_pool(const _Float16* __restrict__ g16, float* __restrict__ pool, float multiplier,
                                                       int first, size_t n) {
	OPT_RANGE
	if (full) {
		const h8 g = *(const h8*)(g16 + i0);
		F8 p{};
		if (!first) p = load_f8(pool + i0);
#pragma unroll
		for (int r = 0; r < 8; ++r) p.v[r] = batched_pool(p.v[r], g[r], multiplier, first != 0);
		store_f8(pool + i0, p);
	} else {
		for (size_t i = i0; i < n; ++i) pool[i] = batched_pool(first ? 0.0f : pool[i], g16[i], multiplier, first != 0);
	}
}

__global__ __launch_bounds__(256) void k_pool_cast(const float* __restrict__ pool, _Float16* __restrict__ pool16, size_t n) {
	OPT_RANGE
	if (full) {
		*(h8*)(pool16 + i0) = round_h8(load_f8(pool + i0));
	} else {
		for (size_t i = i0; i < n; ++i) pool16[i] = f16_rn(pool[i]);
	}
}

// Adam of the torch optimizer (tinycudann.optim.Adam) on one parameter tensor: adam_tail on the
// caller's gradient as it is (G = float or _Float16; no loss scale, no fp16 rounding), fp32 masters
// only. a.n parameters, the first a.n_matrix of them matrix parameters (the boundary may fall inside
// a thread's 8). The five loads of a thread are independent; a thread none of whose parameters is
// updated (frozen class, untouched grid entries) stores nothing, else its skipped parameters are
// rewritten with their unchanged values.
template <typename G>
__global__ __launch_bounds__(256) void k_adam_torch(const AdamArgs a, float* __restrict__ w32, const G* __restrict__ grad,
                                                     float* __restrict__ m1, float* __restrict__ m2, uint32_t* __restrict__ steps) {
	const size_t n = a.n;
	OPT_RANGE
	if (full) {
		F8 w = load_f8(w32 + i0), v1 = load_f8(m1 + i0), v2 = load_f8(m2 + i0), g;
		const uint4 sa = *(const uint4*)(steps + i0), sb = *(const uint4*)(steps + i0 + 4);
		uint32_t st[8] = {sa.x, sa.y, sa.z, sa.w, sb.x, sb.y, sb.z, sb.w};
		if constexpr (sizeof(G) == 4) {
			g = load_f8((const float*)grad + i0);
		} else {
			const h8 gh = *(const h8*)((const _Float16*)grad + i0);
#pragma unroll
			for (int r = 0; r < 8; ++r) g.v[r] = (float)gh[r];
		}
		bool any = false;
#pragma unroll
		for (int r = 0; r < 8; ++r) any = adam_tail(a, (uint32_t)i0 + r, g.v[r], w.v[r], v1.v[r], v2.v[r], st[r]) || any;
		if (!any) return;
		store_f8(w32 + i0, w);
		store_f8(m1 + i0, v1);
		store_f8(m2 + i0, v2);
		*(uint4*)(steps + i0) = make_uint4(st[0], st[1], st[2], st[3]);
		*(uint4*)(steps + i0 + 4) = make_uint4(st[4], st[5], st[6], st[7]);
	} else {
		for (size_t i = i0; i < n; ++i) {
			float w = w32[i], v1 = m1[i], v2 = m2[i];
			uint32_t st = steps[i];
			if (!adam_tail(a, (uint32_t)i, (float)grad[i], w, v1, v2, st)) continue;
			w32[i] = w;
			m1[i] = v1;
			m2[i] = v2;
			steps[i] = st;
		}
	}
}

#undef OPT_RANGE

inline dim3 opt_grid(size_t n) { return dim3(div_round_up(n, OPT_SPAN)); }

}  // namespace

uint32_t optimizer_kernel_span() { return OPT_SPAN; }

void launch_grad_f16(hipStream_t st, const float* g32, void* g16, float grad_scale, size_t n) {
	if (!n) return;
	hipLaunchKernelGGL(k_grad_f16, opt_grid(n), dim3(OPT_THREADS), 0, st, g32, (_Float16*)g16, grad_scale, n);
	TCNN_HIP_CHECK(hipGetLastError());
}

void launch_sgd(hipStream_t st, float* w32, void* w16, const void* g16, float loss_scale, float lr, float l2_reg, size_t n) {
	if (!n) return;
	hipLaunchKernelGGL(k_sgd, opt_grid(n), dim3(OPT_THREADS), 0, st, w32, (_Float16*)w16, (const _Float16*)g16, loss_scale, lr, l2_reg, n);
	TCNN_HIP_CHECK(hipGetLastError());
}

void launch_ema(hipStream_t st, const void* w16, void* ema16, float* tmp, float decay, float debias_old, float debias_new, size_t n) {
	if (!n) return;
	if (tmp)
		hipLaunchKernelGGL(k_ema<true>, opt_grid(n), dim3(OPT_THREADS), 0, st, (const _Float16*)w16, (_Float16*)ema16, tmp, decay, debias_old,
		                   debias_new, n);
	else
		hipLaunchKernelGGL(k_ema<false>, opt_grid(n), dim3(OPT_THREADS), 0, st, (const _Float16*)w16, (_Float16*)ema16, tmp, decay,
		                   debias_old, debias_new, n);
	TCNN_HIP_CHECK(hipGetLastError());
}

void launch_lookahead(hipStream_t st, float* w32, void* w16, void* look16, float alpha, size_t n) {
	if (!n) return;
	hipLaunchKernelGGL(k_lookahead, opt_grid(n), dim3(OPT_THREADS), 0, st, w32, (_Float16*)w16, (_Float16*)look16, alpha, n);
	TCNN_HIP_CHECK(hipGetLastError());
}

void launch_batched_pool(hipStream_t st, const void* g16, float* pool, uint32_t multiplier, bool first, size_t n) {
	if (!n) return;
	hipLaunchKernelGGL(k_batched_pool, opt_grid(n), dim3(OPT_THREADS), 0, st, (const _Float16*)g16, pool, (float)multiplier, first ? 1 : 0,
	                   n);
	TCNN_HIP_CHECK(hipGetLastError());
}

void launch_adam_torch(hipStream_t st, const AdamArgs& a, float* w32, const void* grad, bool grad_f16, float* m1, float* m2, uint32_t* steps) {
	if (!a.n) return;
	if (grad_f16)
		hipLaunchKernelGGL(k_adam_torch<_Float16>, opt_grid(a.n), dim3(OPT_THREADS), 0, st, a, w32, (const _Float16*)grad, m1, m2, steps);
	else
		hipLaunchKernelGGL(k_adam_torch<float>, opt_grid(a.n), dim3(OPT_THREADS), 0, st, a, w32, (const float*)grad, m1, m2, steps);
	TCNN_HIP_CHECK(hipGetLastError());
}

void launch_pool_cast(hipStream_t st, const float* pool, void* pool16, size_t n) {
	if (!n) return;
	hipLaunchKernelGGL(k_pool_cast, opt_grid(n), dim3(OPT_THREADS), 0, st, pool, (_Float16*)pool16, n);
	TCNN_HIP_CHECK(hipGetLastError());
}

}  // namespace tcnn_amd
