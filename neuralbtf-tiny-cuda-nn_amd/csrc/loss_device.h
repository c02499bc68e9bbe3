// The nine training losses of the reference (src/loss.cu:57-65), one device definition shared by the
// stand-alone kernel (mlp_layers.hip), the register-resident fused kernel (mlp_fused.h) and the tile
// kernels (mlp_tile.h), so that the three agree bit for bit.
//
// The arithmetic is the reference's, term for term and in its operation order
// (include/tiny-cuda-nn/losses/*.h, the lines between `const float prediction` and `gradients[i] =`).
// The library is built with -ffp-contract=off: nothing here is left for the compiler to contract. The
// three reference expressions of the form a*b + c are written as explicit FMAs, the project's
// restatement of nvcc's contraction (as the RelativeL2 `p*p + 0.01f` always was):
//   relative_l2.h:67            p*p + 0.01f                      -> fmaf(p, p, 0.01f)
//   relative_l2_luminance.h:79  luminance*luminance + 0.01f      -> fmaf(lum, lum, 0.01f)
//   smape.h:66                  0.5f*(|t| + |p|) + 1e-2f         -> fmaf(0.5f, |t| + |p|, 1e-2f)
//   relative_l2_luminance.h:77  0.299f*r + 0.587f*g + 0.114f*b   -> fmaf(0.114f, b, fmaf(0.587f, g, 0.299f*r))
// The last one is a CHOICE: the association (left to right, each addition fused with the product to
// its right) is what a left-to-right contraction gives, but what nvcc emits for it was not checked.
#pragma once

#include "common.h"

namespace tcnn_amd {

// RelativeL2 = 0 and L2 = 1 are the values of the former one-bit `loss_l2` switch.
enum LossType : uint32_t {
	LOSS_RELATIVE_L2 = 0,
	LOSS_L2 = 1,
	LOSS_RELATIVE_L2_LUMINANCE = 2,
	LOSS_L1 = 3,
	LOSS_RELATIVE_L1 = 4,
	LOSS_MAPE = 5,
	LOSS_SMAPE = 6,
	LOSS_CROSS_ENTROPY = 7,
	LOSS_VARIANCE = 8,
	LOSS_N_TYPES = 9,
};

// relative_l2_luminance.h:68-77: r, g, b are outputs 0, 1, 2 of the sample's padded row; outputs
// 3, 4, 5 are added by the caller when dims >= 6
__device__ __forceinline__ float loss_luminance(float r, float g, float b) {
	return __builtin_fmaf(0.114f, b, __builtin_fmaf(0.587f, g, 0.299f * r));
}

// How a kernel selects the loss (the LOSS template argument of loss_eval and of the training kernels'
// bodies): a LossType value fixes it at compile time; LOSS_ANY switches on the run-time type (wave-
// uniform); LOSS_L2_FAMILY is the run-time choice between RelativeL2 and L2 only -- the code of the
// default training kernels, which sit at their register bounds ("Losses").
constexpr int LOSS_ANY = -1;
constexpr int LOSS_L2_FAMILY = -2;

// One output element: the loss value (already divided by n_total) and the loss-scaled gradient.
// PDF: data_pdf is present (false: pdf = 1, and the divisions by it, exact, are left out).
// lum is read for RelativeL2Luminance only.
// G: the type the gradient is stored in -- _Float16 (rounded once from the fp32 result) or float (the
// fp32 result itself: the torch loss on fp32 predictions, loss_torch.hip).
template <typename G>
__device__ __forceinline__ G loss_grad_store(float g);
template <>
__device__ __forceinline__ _Float16 loss_grad_store<_Float16>(float g) { return f16_rn(g); }
template <>
__device__ __forceinline__ float loss_grad_store<float>(float g) { return g; }

template <bool PDF, int LOSS = LOSS_ANY, typename G = _Float16>
__device__ __forceinline__ void loss_eval(uint32_t type_rt, float p, float t, float pdf, float n_total, float loss_scale, float lum,
                                          float& value, G& grad) {
	const uint32_t type = LOSS >= 0 ? (uint32_t)LOSS : type_rt;
	const float d = p - t;
	if (LOSS == LOSS_L2_FAMILY || type <= LOSS_RELATIVE_L2_LUMINANCE) {  // relative_l2.h:66-75, l2.h:66-74, relative_l2_luminance.h:66-86
		float pse;
		if constexpr (LOSS == LOSS_L2_FAMILY) pse = type ? 1.0f : __builtin_fmaf(p, p, 0.01f);
		else pse = type == LOSS_L2 ? 1.0f : type == LOSS_RELATIVE_L2 ? __builtin_fmaf(p, p, 0.01f) : __builtin_fmaf(lum, lum, 0.01f);
		if constexpr (PDF) {
			value = d * d / pse / pdf / n_total;
			grad = loss_grad_store<G>(loss_scale * (2.0f * d / pse / pdf) / n_total);
		} else {
			value = d * d / pse / n_total;
			grad = loss_grad_store<G>(loss_scale * (2.0f * d / pse) / n_total);
		}
	} else if (type == LOSS_L1) {  // l1.h:66-74
		if constexpr (PDF) {
			value = fabsf(d) / pdf / n_total;
			grad = loss_grad_store<G>(loss_scale * copysignf(1.0f / pdf, d) / n_total);
		} else {
			value = fabsf(d) / n_total;
			grad = loss_grad_store<G>(loss_scale * copysignf(1.0f, d) / n_total);
		}
	} else if (type <= LOSS_SMAPE) {  // relative_l1.h:66-76, mape.h:66-77, smape.h:66-77
		const float den = type == LOSS_RELATIVE_L1 ? fabsf(p) + 1e-2f
		                  : type == LOSS_MAPE      ? fabsf(t) + 1e-2f
		                                           : __builtin_fmaf(0.5f, fabsf(t) + fabsf(p), 1e-2f);
		float scale = 1.0f / den;
		if constexpr (PDF) scale = scale / pdf;
		value = fabsf(d) * scale / n_total;
		grad = loss_grad_store<G>(loss_scale * copysignf(scale, d) / n_total);  // d == 0: +scale, as copysignf gives
	} else if (type == LOSS_CROSS_ENTROPY) {  // cross_entropy.h:66-76: 1 / n_total is inside factor
		float factor = -t;
		if constexpr (PDF) factor = factor / pdf;
		factor = factor / n_total;
		value = factor * logf(p);
		grad = loss_grad_store<G>(loss_scale * (factor / p));
	} else {  // variance_is.h:66-76: the pdf divides twice
		float factor = t * t;
		if constexpr (PDF) factor = factor / pdf;
		factor = factor / n_total;
		value = PDF ? factor / p - factor / pdf : factor / p - factor;
		grad = loss_grad_store<G>(loss_scale * (-factor / (p * p)));
	}
}

// The luminance of the sample in lane column c from the 16-output fragment y of an MFMA result, by
// ds_bpermute (no LDS memory; it reads the source lane's register). The WHOLE wave must execute this:
// a lane outside EXEC reads as 0. Every lane computes its sample's luminance, redundantly.
//   OP  (out_row order: register r of lane group q = output 4r + q): outputs 0..3 are y[0] of lanes
//       c, 16 + c, 32 + c, 48 + c; outputs 4, 5 are y[1] of lanes c, 16 + c.
//   !OP (one lane holds outputs 4q .. 4q + 3): outputs 0..3 are y[0..3] of lane c, outputs 4, 5 are
//       y[0], y[1] of lane 16 + c.
// One term of the sum at a time (fetch, add, FMA), the stages fenced against the scheduler: the fused
// kernel has no register to spare for four fetches in flight ("Losses").
template <bool OP>
__device__ __forceinline__ float loss_luminance_xlane(h4 y, int c, uint32_t dims) {
	// output k of the sample, fp16 -> fp32, from the lane that holds it
	auto out = [&](int k) {
		const int lane = OP ? 16 * (k & 3) + c : 16 * (k >> 2) + c;
		const int reg = OP ? k >> 2 : k & 3;
		const _Float16 mine = y[reg];  // a copy: bit-casting the vector element itself reads element 0
		const int bits = __builtin_amdgcn_ds_bpermute(4 * lane, (int)__builtin_bit_cast(uint16_t, mine));
		return (float)__builtin_bit_cast(_Float16, (uint16_t)bits);
	};
	const bool six = dims >= 6;  // wave-uniform
	float r = out(0);
	if (six) r += out(3);
	float lum = 0.299f * r;
	__builtin_amdgcn_sched_barrier(0);
	float g = out(1);
	if (six) g += out(4);
	lum = __builtin_fmaf(0.587f, g, lum);
	__builtin_amdgcn_sched_barrier(0);
	float b = out(2);
	if (six) b += out(5);
	return __builtin_fmaf(0.114f, b, lum);  // = loss_luminance(r, g, b)
}

}  // namespace tcnn_amd
