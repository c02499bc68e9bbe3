// grid_bwd_scale.h -- the fixed-point exponent of the LDS grid backward (grid_bwd_lds.h) and the
// guard that decides whether a cheaply summed bound may stand in for the exact one. Host and device:
// tests/cpp/grid_bwd_scale_check.cpp runs this very code against emulations of both summation orders.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TCNN_SCALE_HD __host__ __device__ __forceinline__
#else
#define TCNN_SCALE_HD inline
#endif

namespace tcnn_amd {

// lim = the largest factor that keeps m (1.01: the rounding of every add) plus half a unit per corner
// update of the chunk's P points below 2^31. D <= 4, P <= 2^26: the numerator stays positive.
TCNN_SCALE_HD float grid_bwd_scale_lim(float m, float P, uint32_t D) {
	return (2147483647.0f - (float)(1u << D) * P) / (m * 1.01f);
}

// e = floor(log2(lim)), clamped to [-126, e_max]; 0 for an empty or non-finite sum (the caller turns a
// non-finite sum into a NaN gradient). e_max: the precision trait's EXP_MAX (grid_bwd_lds.h); the default
// is the fp16 kernel's, which fp16 dL/dy never reaches (a non-zero sum is >= 2^-24, so lim < 2^55).
constexpr int GRID_BWD_EXP_MAX_F16 = 100;
TCNN_SCALE_HD int grid_bwd_scale_exp(float m, float P, uint32_t D, int e_max = GRID_BWD_EXP_MAX_F16) {
	int e = 0;
	if (m > 0.0f && std::isfinite(m)) {
		e = ilogbf(grid_bwd_scale_lim(m, P, D));
		e = e < e_max ? e : e_max;
		e = e > -126 ? e : -126;
	}
	return e;
}

// Guard of the streaming path. The exact pre-pass sums the chunk's s_i = max_f |dL/dy_i| (all >= 0)
// in fp32 as: 32 sequential adds per thread, a 6-step butterfly, 16 sequential adds over the waves
// -- at most 32 + 6 + 16 = 54 roundings on the path of any term. The streaming path sums the same
// terms as: 1 add of a lane's two samples, a 4-step tree over the 16 lanes (the fused kernel's slice
// sum), the 6-step butterfly, the 16 wave adds -- at most 27. With u = 2^-24 and only non-negative
// terms, a sum with k roundings per path lies within [(1-u)^k, (1+u)^k] of the real sum S (no term
// underflows: the smallest fp16 magnitude is 2^-24; none overflows: 2^15 x 65504 < 2^31), so
//   m / mh in [(1-u)^54 (1+u)^-27, (1+u)^54 (1-u)^-27]  -> |m / mh - 1| < 82 u.
// lim(m) rounds twice more (the product m * 1.01f and the quotient; the numerator is the same
// number on both paths), each monotonic in m, so |lim(m) / lim(mh) - 1| < 82 u + 4 u + O(u^2) < 87 u
// ~ 2^-17.6. The guard band is 2^-14 = 1024 u relative, twelve times that: when lim(mh) = f 2^e with
// 1 + 2^-14 <= f <= 2 - 2^-13, lim(m) lies in the same binade and floor(log2) agrees. A uniformly
// distributed mantissa falls in the band with probability 3 x 2^-14 < 0.02 %.
// mh = 0 means every term is 0, so m = 0 as well (e = 0 on both paths); a non-finite mh is rejected.
constexpr uint32_t GRID_BWD_GUARD_BITS = 1u << 9;  // 2^-14 of the 23-bit mantissa
TCNN_SCALE_HD bool grid_bwd_scale_guard(float mh, float P, uint32_t D) {
	if (!std::isfinite(mh)) return false;
	if (!(mh > 0.0f)) return true;
	const float lim = grid_bwd_scale_lim(mh, P, D);
	uint32_t b;
	memcpy(&b, &lim, 4);
	const uint32_t ex = (b >> 23) & 0xffu, mant = b & 0x7fffffu;
	if (ex == 0u || ex == 0xffu) return false;  // denormal or non-finite lim: take the exact path
	return mant >= GRID_BWD_GUARD_BITS && mant <= 0x800000u - 2u * GRID_BWD_GUARD_BITS;
}

}  // namespace tcnn_amd
