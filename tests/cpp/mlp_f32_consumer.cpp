// A caller of fp32-precision network modules through the runtime C++ API: tcnn::cpp::create_network(...,
// Precision::Fp32) and create_network_with_input_encoding(..., Precision::Fp32)
// (include/tiny-cuda-nn/cpp_api.h). Built against the headers + libtcnn_mi355x.so and run by
// tests/test_gpu_mlp_f32_cpp.py: a W = 16 network (16 inputs, one hidden ReLU layer, 16 outputs) runs forward
// and backward on fp32 buffers and is compared with a host double loop.
#include <tiny-cuda-nn/cpp_api.h>

#include <cmath>
#include <cstdio>
#include <memory>
#include <vector>

using namespace tcnn;

#define REQUIRE(c)                                                     \
	do {                                                               \
		if (!(c)) {                                                    \
			std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
			return 1;                                                  \
		}                                                              \
	} while (0)
#define HIP_OK(x) REQUIRE((x) == hipSuccess)

int main() {
	const uint32_t W = 16, IN = 16, OUT = 16, n = 256;
	const json net = {{"otype", "CutlassMLP"}, {"n_neurons", W}, {"n_hidden_layers", 1}, {"activation", "ReLU"}, {"output_activation", "None"}};
	std::unique_ptr<cpp::Module> m{cpp::create_network(IN, OUT, net, cpp::Precision::Fp32)};
	REQUIRE(m->param_precision() == cpp::Precision::Fp32);
	REQUIRE(m->output_precision() == cpp::Precision::Fp32);
	REQUIRE(m->n_params() == W * IN + OUT * W);
	REQUIRE(m->n_input_dims() == IN && m->n_output_dims() == OUT);
	// the fp16 module of the same call keeps its precision, and so does the constructor without one
	std::unique_ptr<cpp::Module> h{cpp::create_network(IN, OUT, net, cpp::Precision::Fp16)};
	std::unique_ptr<cpp::Module> h0{cpp::create_network(IN, OUT, net)};
	REQUIRE(h->param_precision() == cpp::Precision::Fp16 && h0->param_precision() == cpp::Precision::Fp16);
	REQUIRE(h->n_params() == m->n_params());
	const json enc = {{"otype", "OneBlob"}, {"n_bins", 4}};
	std::unique_ptr<cpp::Module> e{cpp::create_network_with_input_encoding(2, 3, enc, net, cpp::Precision::Fp32)};
	REQUIRE(e->param_precision() == cpp::Precision::Fp32 && e->n_output_dims() == 16);
	REQUIRE(e->name() == "NetworkWithInputEncoding");

	const size_t np = m->n_params();
	std::vector<float> p(np), x((size_t)n * IN), dy((size_t)n * OUT);
	for (size_t i = 0; i < np; ++i) p[i] = 0.5f * std::sin(0.37f * (float)(i + 1));
	for (size_t i = 0; i < x.size(); ++i) x[i] = std::fmod(0.6180339887f * (float)(i + 1), 1.0f) - 0.3f;
	for (size_t i = 0; i < dy.size(); ++i) dy[i] = std::cos(0.11f * (float)(i + 3));
	float *dp, *dx, *dout, *ddy, *dgp, *dgx;
	HIP_OK(hipMalloc(&dp, np * 4));
	HIP_OK(hipMalloc(&dx, x.size() * 4));
	HIP_OK(hipMalloc(&dout, dy.size() * 4));
	HIP_OK(hipMalloc(&ddy, dy.size() * 4));
	HIP_OK(hipMalloc(&dgp, np * 4));
	HIP_OK(hipMalloc(&dgx, x.size() * 4));
	HIP_OK(hipMemcpy(dp, p.data(), np * 4, hipMemcpyHostToDevice));
	HIP_OK(hipMemcpy(dx, x.data(), x.size() * 4, hipMemcpyHostToDevice));
	HIP_OK(hipMemcpy(ddy, dy.data(), dy.size() * 4, hipMemcpyHostToDevice));
	cpp::Context ctx = m->forward(nullptr, n, dx, dout, dp, true);
	m->backward(nullptr, ctx, n, dgx, ddy, dgp, dx, dout, dp);
	HIP_OK(hipDeviceSynchronize());
	std::vector<float> out(dy.size()), gp(np), gx(x.size());
	HIP_OK(hipMemcpy(out.data(), dout, out.size() * 4, hipMemcpyDeviceToHost));
	HIP_OK(hipMemcpy(gp.data(), dgp, np * 4, hipMemcpyDeviceToHost));
	HIP_OK(hipMemcpy(gx.data(), dgx, gx.size() * 4, hipMemcpyDeviceToHost));

	// host double: y = Wout relu(W0 x); magnitudes (sums of |terms|) size the fp32 bounds
	std::vector<double> rgp(np, 0.0), mgp(np, 0.0);
	const float* W0 = p.data();
	const float* Wo = p.data() + W * IN;
	const double u = std::ldexp(1.0, -24);
	for (uint32_t b = 0; b < n; ++b) {
		double a[16], am[16], d[16], dm[16];
		for (uint32_t i = 0; i < W; ++i) {
			double s = 0, sm = 0;
			for (uint32_t k = 0; k < IN; ++k) {
				s += (double)W0[i * IN + k] * x[b * IN + k];
				sm += std::fabs((double)W0[i * IN + k] * x[b * IN + k]);
			}
			a[i] = s > 0 ? s : 0;
			am[i] = sm;
		}
		for (uint32_t o = 0; o < OUT; ++o) {
			double s = 0, sm = 0;
			for (uint32_t i = 0; i < W; ++i) {
				s += (double)Wo[o * W + i] * a[i];
				sm += std::fabs((double)Wo[o * W + i]) * am[i];
			}
			// two chains of 16 fp32 FMAs and one stored fp32 activation in between
			REQUIRE(std::fabs(out[b * OUT + o] - s) <= 40 * u * sm + 1e-30);
		}
		for (uint32_t i = 0; i < W; ++i) {
			double s = 0, sm = 0;
			for (uint32_t o = 0; o < OUT; ++o) {
				s += (double)Wo[o * W + i] * dy[b * OUT + o];
				sm += std::fabs((double)Wo[o * W + i] * dy[b * OUT + o]);
				rgp[W * IN + o * W + i] += (double)dy[b * OUT + o] * a[i];
				mgp[W * IN + o * W + i] += std::fabs((double)dy[b * OUT + o]) * am[i];
			}
			// ReLU's mask comes from the stored forward value; a pre-activation within rounding of 0 may fall either way
			const bool on = a[i] > 0;
			if (std::fabs(a[i]) <= 20 * u * am[i]) d[i] = std::nan("");
			else d[i] = on ? s : 0;
			dm[i] = sm;
		}
		for (uint32_t k = 0; k < IN; ++k) {
			double s = 0, sm = 0;
			bool unsure = false;
			for (uint32_t i = 0; i < W; ++i) {
				if (std::isnan(d[i])) { unsure = true; continue; }
				s += (double)W0[i * IN + k] * d[i];
				sm += std::fabs((double)W0[i * IN + k]) * dm[i];
			}
			if (!unsure) REQUIRE(std::fabs(gx[b * IN + k] - s) <= 40 * u * sm + 1e-30);
		}
		for (uint32_t i = 0; i < W; ++i)
			for (uint32_t k = 0; k < IN; ++k) {
				if (std::isnan(d[i])) { mgp[i * IN + k] = INFINITY; continue; }
				rgp[i * IN + k] += d[i] * x[b * IN + k];
				mgp[i * IN + k] += dm[i] * std::fabs((double)x[b * IN + k]);
			}
	}
	double sum = 0;
	for (size_t i = 0; i < np; ++i) {
		REQUIRE(std::isfinite(gp[i]));
		// a chain of n products over the batch on top of the deltas' own error
		REQUIRE(!(std::fabs(gp[i] - rgp[i]) > (n + 60) * u * mgp[i] + 1e-30));
		sum += std::fabs(gp[i]);
	}
	REQUIRE(sum > 1.0);
	std::printf("mlp f32 api ok\n");
	return 0;
}
