// act_f32_ulps -- accuracy of the fp32 network engine's activation functions (csrc/act_f32.h: the very
// device functions mlp_f32.hip calls) against host double, over a dense grid. Stand-alone:
//
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=off -Ineuralbtf-tiny-cuda-nn_amd/csrc \
//         tools/act_f32_ulps.hip -o tools/act_f32_ulps && tools/act_f32_ulps > profiles/act_f32_ulps.json
//
// For every smooth activation: the forward act(z) over z in [-8, 8] (Exponential: [-8, 32], which covers
// the wide-range test's pre-activations of ~30), and the transfer factor phi(y) over the stored forward
// values y = float(act(z)) of the same grid. Error unit: 2^-24 * max(|exact|, 1) -- relative to the value
// where it is above 1, absolute below (Softplus' log(exp(10 z) + 1) and 1 - exp(-10 y) cancel near 0, so a
// purely relative measure would not be bounded). None, ReLU and LeakyReLU are exact selections / one
// multiplication and are not measured. tests/mlp_f32_reference.py doubles these figures for its bound.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <vector>

#include "act_f32.h"

using namespace tcnn_amd;

#define HIP_OK(x)                                                            \
	do {                                                                     \
		if ((x) != hipSuccess) {                                             \
			std::fprintf(stderr, "HIP error at %s:%d\n", __FILE__, __LINE__); \
			return 1;                                                        \
		}                                                                    \
	} while (0)

constexpr uint32_t N = 1u << 22;

__global__ void k_eval(int act, float lo, float step, uint32_t n, float* __restrict__ z_out, float* __restrict__ y_out,
                       float* __restrict__ f_out) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const float z = lo + step * (float)i;
	const float y = act_fwd_f32(act, z);
	z_out[i] = z;
	y_out[i] = y;
	f_out[i] = act_factor_f32(act, y);
}

static double fwd64(int a, double z) {
	switch (a) {
		case AF32_EXPONENTIAL: return std::exp(z);
		case AF32_SIGMOID: return 1.0 / (1.0 + std::exp(-z));
		case AF32_SQUAREPLUS: return 0.5 * (10.0 * z + std::sqrt(100.0 * z * z + 4.0)) / 10.0;
		case AF32_SOFTPLUS: return (z > 0 ? 10.0 * z + std::log1p(std::exp(-10.0 * z)) : std::log1p(std::exp(10.0 * z))) / 10.0;
		case AF32_TANH: return std::tanh(z);
		default: return z;
	}
}
static double factor64(int a, double y) {
	switch (a) {
		case AF32_EXPONENTIAL: return y;
		case AF32_SIGMOID: return y * (1.0 - y);
		case AF32_SQUAREPLUS: return 100.0 * y * y / (100.0 * y * y + 1.0);
		case AF32_SOFTPLUS: return -std::expm1(-10.0 * y);
		case AF32_TANH: return 1.0 - y * y;
		default: return 1.0;
	}
}

int main() {
	const struct { int a; const char* name; float lo, hi; } acts[] = {
	    {AF32_EXPONENTIAL, "Exponential", -8.0f, 32.0f}, {AF32_SIGMOID, "Sigmoid", -8.0f, 8.0f}, {AF32_SQUAREPLUS, "Squareplus", -8.0f, 8.0f},
	    {AF32_SOFTPLUS, "Softplus", -8.0f, 8.0f},        {AF32_TANH, "Tanh", -8.0f, 8.0f}};
	float *dz, *dy, *df;
	HIP_OK(hipMalloc(&dz, N * 4));
	HIP_OK(hipMalloc(&dy, N * 4));
	HIP_OK(hipMalloc(&df, N * 4));
	std::vector<float> z(N), y(N), f(N);
	const double unit = std::ldexp(1.0, -24);
	std::printf("{\"grid_points\": %u, \"unit\": \"2^-24 * max(|exact|, 1)\", \"activations\": {", N);
	bool first = true;
	for (const auto& c : acts) {
		const float step = (c.hi - c.lo) / (float)N;
		hipLaunchKernelGGL(k_eval, dim3(N / 256), dim3(256), 0, nullptr, c.a, c.lo, step, N, dz, dy, df);
		HIP_OK(hipGetLastError());
		HIP_OK(hipDeviceSynchronize());
		HIP_OK(hipMemcpy(z.data(), dz, N * 4, hipMemcpyDeviceToHost));
		HIP_OK(hipMemcpy(y.data(), dy, N * 4, hipMemcpyDeviceToHost));
		HIP_OK(hipMemcpy(f.data(), df, N * 4, hipMemcpyDeviceToHost));
		double worst_fwd = 0, worst_fac = 0;
		for (uint32_t i = 0; i < N; ++i) {
			const double ey = fwd64(c.a, (double)z[i]), ef = factor64(c.a, (double)y[i]);
			worst_fwd = std::max(worst_fwd, std::fabs((double)y[i] - ey) / (unit * std::max(std::fabs(ey), 1.0)));
			worst_fac = std::max(worst_fac, std::fabs((double)f[i] - ef) / (unit * std::max(std::fabs(ef), 1.0)));
		}
		std::printf("%s\n  \"%s\": {\"range\": [%g, %g], \"forward\": %.4f, \"factor\": %.4f}", first ? "" : ",", c.name, (double)c.lo,
		            (double)c.hi, worst_fwd, worst_fac);
		first = false;
	}
	std::printf("\n}}\n");
	return 0;
}
