// A caller of the reference's loss interface (reference include/tiny-cuda-nn/loss.h, src/loss.cu:57-65)
// over the engine: create_loss<T> for the nine otypes, Loss<T>::evaluate on the output of
// Trainer::forward (its gradients must be the context's dL_doutput, bit for bit), and
// create_from_config with a loss the engine once refused. Built against include/tiny-cuda-nn/*.h +
// libtcnn_mi355x.so and run by tests/test_gpu_losses.py. Every check prints "FAIL ..." and exits nonzero.
#include <tiny-cuda-nn/common_device.h>

#include <tiny-cuda-nn/config.h>
#include <tiny-cuda-nn/loss.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <memory>
#include <vector>

using namespace tcnn;

static int g_fail = 0;
#define EXPECT(c)                                                           \
	do {                                                                    \
		if (!(c)) {                                                         \
			std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c);        \
			++g_fail;                                                       \
		}                                                                   \
	} while (0)

__global__ void field(uint32_t n, const float* __restrict__ xy, float* __restrict__ rgb) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const float x = xy[2 * i], y = xy[2 * i + 1];
	rgb[3 * i + 0] = 0.5f + 0.5f * sinf(9.0f * x) * cosf(7.0f * y);
	rgb[3 * i + 1] = 0.5f + 0.4f * sinf(23.0f * x * y + 1.0f);
	rgb[3 * i + 2] = 0.5f + 0.3f * cosf(31.0f * x) * sinf(17.0f * y);
}

int main(int argc, char** argv) {
	if (argc < 2) {
		std::printf("usage: %s <config_hash.json>\n", argv[0]);
		return 2;
	}
	try {
		std::ifstream f{argv[1]};
		json config = json::parse(std::string{std::istreambuf_iterator<char>{f}, std::istreambuf_iterator<char>{}});
		const char* const otypes[] = {"L2", "RelativeL2", "RelativeL2Luminance", "L1", "RelativeL1", "Mape", "Smape", "CrossEntropy", "Variance"};

		// create_loss: the nine otypes in any letter case; anything else throws and names the nine
		for (const char* o : otypes) {
			std::unique_ptr<Loss<network_precision_t>> l{create_loss<network_precision_t>({{"otype", o}})};
			EXPECT(l->hyperparams()["otype"] == o);
		}
		{
			std::unique_ptr<Loss<network_precision_t>> l{create_loss<network_precision_t>({{"otype", "crossentropy"}})};
			EXPECT(l != nullptr);
		}
		for (const char* o : {"Huber", ""}) {
			bool threw = false;
			try {
				std::unique_ptr<Loss<network_precision_t>> l{create_loss<network_precision_t>({{"otype", o}})};
			} catch (const std::runtime_error& e) {
				threw = std::strstr(e.what(), "RelativeL2Luminance") && std::strstr(e.what(), "Variance");
			}
			EXPECT(threw);
		}

		hipStream_t stream;
		HIP_CHECK_THROW(hipStreamCreate(&stream));
		const uint32_t B = 1024;
		default_rng_t rng{1337};
		GPUMatrix<float> batch(2, B), target(3, B);
		generate_random_uniform<float>(stream, rng, batch.n_elements(), batch.data());
		linear_kernel(field, 0, stream, B, batch.data(), target.data());

		// Loss::evaluate on the forward's own output gives the forward's dL_doutput
		for (const char* o : otypes) {
			config["loss"] = {{"otype", o}};
			TrainableModel model = create_from_config(2, 3, config);
			auto ctx = model.trainer->forward(stream, 128.0f, batch, target);
			const uint32_t w = model.trainer->padded_output_width();
			GPUMatrix<float> values(w, B);
			GPUMatrix<network_precision_t> gradients(w, B);
			model.loss->evaluate(stream, 128.0f, ctx->output, target, values, gradients);
			HIP_CHECK_THROW(hipStreamSynchronize(stream));
			std::vector<uint16_t> got((size_t)w * B), want((size_t)w * B);
			HIP_CHECK_THROW(hipMemcpy(got.data(), gradients.data(), got.size() * 2, hipMemcpyDeviceToHost));
			HIP_CHECK_THROW(hipMemcpy(want.data(), ctx->dL_doutput.data(), want.size() * 2, hipMemcpyDeviceToHost));
			EXPECT(got == want);
			bool any = false;
			for (uint16_t g : got) any = any || (g & 0x7fff) != 0;
			EXPECT(any);
			// the context's loss is the sum of the values
			const std::vector<float> v = values.to_cpu_vector();
			double sum = 0.0, mag = 0.0;
			for (float x : v) sum += x, mag += std::fabs(x);
			// (a fresh network's outputs are about 1e-5 and of either sign: CrossEntropy and Variance then give the
			// NaN / inf of the reference's unclamped formulas, in the values and in the sum alike)
			const float loss = model.trainer->loss(stream, *ctx);
			if (std::isfinite(sum)) {
				if (!(std::fabs(loss - sum) <= 1e-5 * mag)) std::printf("%s: loss %g, sum of values %g\n", o, loss, sum);
				EXPECT(std::fabs(loss - sum) <= 1e-5 * mag);
			} else {
				EXPECT(!std::isfinite(loss));
			}
		}

		// create_from_config with Smape trains
		{
			config["loss"] = {{"otype", "Smape"}};
			TrainableModel model = create_from_config(2, 3, config);
			EXPECT(model.trainer->engine() == "fused");
			const uint32_t TB = 1 << 14;
			GPUMatrix<float> tb(2, TB), tt(3, TB);
			float first = 0.0f, last = 0.0f;
			for (int i = 0; i < 100; ++i) {
				generate_random_uniform<float>(stream, rng, tb.n_elements(), tb.data());
				linear_kernel(field, 0, stream, TB, tb.data(), tt.data());
				auto ctx = model.trainer->training_step(stream, tb, tt);
				if (i == 0) first = model.trainer->loss(stream, *ctx);
				if (i == 99) last = model.trainer->loss(stream, *ctx);
			}
			std::printf("Smape loss first=%g last=%g\n", first, last);
			EXPECT(std::isfinite(first) && std::isfinite(last) && last < first);
		}
		HIP_CHECK_THROW(hipStreamDestroy(stream));
	} catch (const std::exception& e) {
		std::printf("FAIL exception: %s\n", e.what());
		return 1;
	}
	if (g_fail) return 1;
	std::printf("loss api ok\n");
	return 0;
}
