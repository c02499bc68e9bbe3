// A caller of fp32-precision encodings through both C++ interfaces: the template API
// (create_encoding<float>, include/tiny-cuda-nn/encoding.h) and the runtime API
// (tcnn::cpp::create_encoding(..., Precision::Fp32), include/tiny-cuda-nn/cpp_api.h). Built against the
// headers + libtcnn_mi355x.so and run by tests/test_gpu_encoding_f32.py: both create an fp32 module of
// the same D = 2 hash grid, and inference on the same parameters gives the same finite fp32 output.
#include <tiny-cuda-nn/cpp_api.h>
#include <tiny-cuda-nn/encoding.h>

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

int main() {
	const json enc = {{"otype", "HashGrid"}, {"n_levels", 8}, {"n_features_per_level", 2}, {"log2_hashmap_size", 12},
	                  {"base_resolution", 8}, {"per_level_scale", 1.5}};
	const uint32_t n = 512;  // the template API's inference takes multiples of 256
	std::unique_ptr<Encoding<float>> a{create_encoding<float>(2, enc)};
	std::unique_ptr<cpp::Module> b{cpp::create_encoding(2, enc, cpp::Precision::Fp32)};
	REQUIRE(a->param_precision() == TCNN_PRECISION_FP32);
	REQUIRE(b->param_precision() == cpp::Precision::Fp32);
	REQUIRE(b->output_precision() == cpp::Precision::Fp32);
	REQUIRE(a->n_params() == b->n_params() && a->n_params() > 0);
	REQUIRE(a->padded_output_width() == 16 && b->n_output_dims() == 16);
	// an fp16 module beside them keeps its precision
	std::unique_ptr<cpp::Module> h{cpp::create_encoding(2, enc, cpp::Precision::Fp16)};
	REQUIRE(h->param_precision() == cpp::Precision::Fp16);

	// parameters large enough to see (the initial ones are +-1e-4): a ramp, the same for both
	std::vector<float> table(a->n_params());
	for (size_t i = 0; i < table.size(); ++i) table[i] = 0.001f * (float)(i % 1999) - 1.0f;
	HIP_CHECK_THROW(hipMemcpy(a->params(), table.data(), table.size() * 4, hipMemcpyHostToDevice));
	std::vector<float> x(2 * n);
	for (uint32_t i = 0; i < 2 * n; ++i) x[i] = std::fmod(0.6180339887f * (float)(i + 1), 1.0f);
	GPUMatrix<float> in(2, n), out_a(16, n), out_b(16, n);
	HIP_CHECK_THROW(hipMemcpy(in.data(), x.data(), x.size() * 4, hipMemcpyHostToDevice));
	a->inference(nullptr, in, out_a);
	b->inference(nullptr, n, in.data(), out_b.data(), a->params());
	HIP_CHECK_THROW(hipDeviceSynchronize());
	std::vector<float> ra(16 * n), rb(16 * n);
	HIP_CHECK_THROW(hipMemcpy(ra.data(), out_a.data(), ra.size() * 4, hipMemcpyDeviceToHost));
	HIP_CHECK_THROW(hipMemcpy(rb.data(), out_b.data(), rb.size() * 4, hipMemcpyDeviceToHost));
	double sum = 0;
	for (size_t i = 0; i < ra.size(); ++i) {
		REQUIRE(std::isfinite(ra[i]));
		REQUIRE(ra[i] == rb[i]);
		sum += std::fabs(ra[i]);
	}
	REQUIRE(sum > 1.0);  // not all zeros
	std::printf("encoding f32 api ok\n");
	return 0;
}
