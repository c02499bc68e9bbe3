// sh_device.h -- real spherical harmonics as polynomials in three independent variables (x, y, z),
// the form of the reference's SphericalHarmonics encoding (the direction is NOT normalised, so off
// the sphere the polynomial form matters). Output l^2 + l + m (0 <= l < DEG, -l <= m <= l):
//   m = 0:  Y(l, 0)  = K(l, 0) P(l, 0)
//   m > 0:  Y(l, m)  = sqrt(2) K(l, m) Re((x + iy)^m) P(l, m)
//           Y(l, -m) = sqrt(2) K(l, m) Im((x + iy)^m) P(l, m)
//   K(l, m) = sqrt((2l + 1) (l - m)! / (4 pi (l + m)!))
//   P(m, m) = (-1)^m (2m - 1)!!,  P(m + 1, m) = (2m + 1) z P(m, m),
//   P(l, m) = ((2l - 1) z P(l - 1, m) - (l + m - 1) P(l - 2, m)) / (l - m)      (a polynomial in z)
// evaluated by these recurrences in fp32, m outermost, every l and m a template parameter: the
// constants fold at compile time and each output goes to its sink as soon as it exists, so even
// degree 8 (64 outputs per sample) keeps a handful of live registers and nothing in scratch.
// The gradient differentiates exactly these recurrences:
//   d Re((x+iy)^m) / dx =  m Re((x+iy)^(m-1)),  d Re / dy = -m Im((x+iy)^(m-1)),
//   d Im((x+iy)^m) / dx =  m Im((x+iy)^(m-1)),  d Im / dy =  m Re((x+iy)^(m-1)),
//   P'(m, m) = 0, P'(m + 1, m) = (2m + 1) P(m, m),
//   P'(l, m) = ((2l - 1) (P(l - 1, m) + z P'(l - 1, m)) - (l + m - 1) P'(l - 2, m)) / (l - m).
// Rounding: an output passes through at most 2m + 5 (l - m) + 3 <= 38 fp32 roundings, each relative
// to a partial result that the same recurrence with every subtraction turned into an addition at
// (|x|, |y|, |z|) bounds.
#pragma once

#include "common.h"

namespace tcnn_amd {

constexpr double sh_const_sqrt(double v) {
	double r = v > 1.0 ? v : 1.0;
	for (int i = 0; i < 64; ++i) r = 0.5 * (r + v / r);
	return r;
}
// K(l, m), times sqrt(2) for m > 0
constexpr float sh_norm(uint32_t l, uint32_t m) {
	double v = (2.0 * l + 1.0) / (4.0 * 3.14159265358979323846);
	for (uint32_t i = l - m + 1; i <= l + m; ++i) v /= (double)i;
	if (m) v *= 2.0;
	return (float)sh_const_sqrt(v);
}
// P(m, m) = (-1)^m (2m - 1)!!
constexpr float sh_pmm(uint32_t m) {
	double v = 1.0;
	for (uint32_t i = 1; i <= m; ++i) v *= -(2.0 * i - 1.0);
	return (float)v;
}

// P(L, M) from p1 = P(L - 1, M), p2 = P(L - 2, M)
template <uint32_t M, uint32_t L>
__device__ __forceinline__ float sh_legendre(float z, float p1, float p2) {
	if constexpr (L == M) return sh_pmm(M);
	else if constexpr (L == M + 1) return ((float)(2 * M + 1) * sh_pmm(M)) * z;
	else return __builtin_fmaf((float)(2 * L - 1) * z, p1, -((float)(L + M - 1) * p2)) * (1.0f / (float)(L - M));
}
// dP(L, M)/dz from p1 = P(L - 1, M), d1 = P'(L - 1, M), d2 = P'(L - 2, M)
template <uint32_t M, uint32_t L>
__device__ __forceinline__ float sh_legendre_dz(float z, float p1, float d1, float d2) {
	if constexpr (L == M) return 0.0f;
	else if constexpr (L == M + 1) return (float)(2 * M + 1) * sh_pmm(M);
	else return __builtin_fmaf((float)(2 * L - 1), __builtin_fmaf(z, d1, p1), -((float)(L + M - 1) * d2)) * (1.0f / (float)(L - M));
}

template <uint32_t DEG, uint32_t M, uint32_t L, typename Out>
__device__ __forceinline__ void sh_fwd_l(float z, float a, float b, float p1, float p2, Out&& out) {
	const float p = sh_legendre<M, L>(z, p1, p2);
	constexpr float k = sh_norm(L, M);
	const float kp = k * p;
	if constexpr (M == 0) out(L * L + L, kp);
	else {
		out(L * L + L + M, kp * a);
		out(L * L + L - M, kp * b);
	}
	if constexpr (L + 1 < DEG) sh_fwd_l<DEG, M, L + 1>(z, a, b, p, p1, out);
}
// a + ib = (x + iy)^M
template <uint32_t DEG, uint32_t M, typename Out>
__device__ __forceinline__ void sh_fwd_m(float x, float y, float z, float a, float b, Out&& out) {
	sh_fwd_l<DEG, M, M>(z, a, b, 0.0f, 0.0f, out);
	if constexpr (M + 1 < DEG) sh_fwd_m<DEG, M + 1>(x, y, z, __builtin_fmaf(a, x, -(b * y)), __builtin_fmaf(a, y, b * x), out);
}
// all DEG^2 outputs at (x, y, z): out(index, value)
template <uint32_t DEG, typename Out>
__device__ __forceinline__ void sh_forward(float x, float y, float z, Out&& out) {
	sh_fwd_m<DEG, 0>(x, y, z, 1.0f, 0.0f, out);
}

// sums over l of g(l, +-M) K P and g(l, +-M) K P' for one M
template <uint32_t DEG, uint32_t M, uint32_t L, typename Grad>
__device__ __forceinline__ void sh_bwd_l(float z, float p1, float p2, float d1, float d2, Grad&& g, float& sa, float& sb, float& za,
                                         float& zb) {
	const float p = sh_legendre<M, L>(z, p1, p2);
	const float d = sh_legendre_dz<M, L>(z, p1, d1, d2);
	constexpr float k = sh_norm(L, M);
	const float kp = k * p, kd = k * d;
	const float ga = g(L * L + L + M);
	sa = __builtin_fmaf(ga, kp, sa);
	za = __builtin_fmaf(ga, kd, za);
	if constexpr (M > 0) {
		const float gb = g(L * L + L - M);
		sb = __builtin_fmaf(gb, kp, sb);
		zb = __builtin_fmaf(gb, kd, zb);
	}
	if constexpr (L + 1 < DEG) sh_bwd_l<DEG, M, L + 1>(z, p, p1, d, d1, g, sa, sb, za, zb);
}
// a + ib = (x + iy)^M, ap + i bp = (x + iy)^(M - 1)
template <uint32_t DEG, uint32_t M, typename Grad>
__device__ __forceinline__ void sh_bwd_m(float x, float y, float z, float a, float b, float ap, float bp, Grad&& g, float& gx, float& gy,
                                         float& gz) {
	float sa = 0.0f, sb = 0.0f, za = 0.0f, zb = 0.0f;
	sh_bwd_l<DEG, M, M>(z, 0.0f, 0.0f, 0.0f, 0.0f, g, sa, sb, za, zb);
	if constexpr (M == 0) gz += za;
	else {
		gx = __builtin_fmaf((float)M, __builtin_fmaf(sa, ap, sb * bp), gx);
		gy = __builtin_fmaf((float)M, __builtin_fmaf(sb, ap, -(sa * bp)), gy);
		gz += __builtin_fmaf(a, za, b * zb);
	}
	if constexpr (M + 1 < DEG)
		sh_bwd_m<DEG, M + 1>(x, y, z, __builtin_fmaf(a, x, -(b * y)), __builtin_fmaf(a, y, b * x), a, b, g, gx, gy, gz);
}
// sum_j g(j) dY_j/d(x, y, z)
template <uint32_t DEG, typename Grad>
__device__ __forceinline__ void sh_backward(float x, float y, float z, Grad&& g, float& gx, float& gy, float& gz) {
	gx = gy = gz = 0.0f;
	sh_bwd_m<DEG, 0>(x, y, z, 1.0f, 0.0f, 0.0f, 0.0f, g, gx, gy, gz);
}

}  // namespace tcnn_amd
