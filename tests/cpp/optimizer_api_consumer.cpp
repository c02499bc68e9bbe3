// A caller of the stacked optimizers through the C++ template API (create_optimizer with "nested"
// blocks, Trainer::params_inference, use_inference_params) and of the optimizer kernels themselves on
// parameter counts that are no multiple of 8 (which no trainable model has), built against
// include/tiny-cuda-nn/*.h + libtcnn_mi355x.so and run by tests/test_gpu_optimizer_cpp.py. Every check
// prints "FAIL ..." and exits nonzero on mismatch.
#include <tiny-cuda-nn/common_device.h>

#include <tiny-cuda-nn/config.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <vector>

#include "optimizers.h"  // csrc: the kernels' launchers

using namespace tcnn;

static int g_fail = 0;
#define EXPECT(c)                                                    \
	do {                                                             \
		if (!(c)) {                                                  \
			std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
			++g_fail;                                                \
		}                                                            \
	} while (0)

__global__ void field(uint32_t n, const float* __restrict__ xy, float* __restrict__ rgb) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const float x = xy[2 * i], y = xy[2 * i + 1];
	rgb[3 * i + 0] = 0.5f + 0.5f * sinf(9.0f * x) * cosf(7.0f * y);
	rgb[3 * i + 1] = 0.5f + 0.4f * sinf(23.0f * x * y + 1.0f);
	rgb[3 * i + 2] = 0.5f + 0.3f * cosf(31.0f * x) * sinf(17.0f * y);
}

template <typename F>
static std::string thrown(F&& f) {
	try {
		f();
	} catch (const std::exception& e) {
		return e.what();
	}
	return "";
}
static bool contains(const std::string& s, const char* what) { return s.find(what) != std::string::npos; }

template <typename T>
static std::vector<T> d2h(const void* p, size_t n) {
	std::vector<T> h(n);
	HIP_CHECK_THROW(hipMemcpy(h.data(), p, n * sizeof(T), hipMemcpyDeviceToHost));
	return h;
}
template <typename T>
static GPUMemory<T> h2d(const std::vector<T>& h) {
	GPUMemory<T> d(h.size());
	HIP_CHECK_THROW(hipMemcpy(d.data(), h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
	return d;
}
static double ulp16(double x) { return std::ldexp(1.0, (int)std::floor(std::log2(std::fmax(std::fabs(x), std::ldexp(1.0, -14)))) - 10); }

// ---- the kernels on n parameters, against their expressions in double:
// |got - ref| <= (n_ops + 2) 2^-24 A + 2^-149 for fp32 results (A: the expression with every term's
// magnitude), fp16 results bit-equal to the rounding of the fp32 result next to them ----
static void kernel_checks(hipStream_t st, size_t n) {
	std::vector<float> w(n), g32(n), pool(n), tmp(n);
	std::vector<_Float16> g(n), look(n), ema(n), w16(n);
	default_rng_t r{(uint64_t)n};
	for (size_t i = 0; i < n; ++i) {
		w[i] = (r.next_float() - 0.5f) * 3.0f;
		g32[i] = (r.next_float() - 0.5f) * 40.0f;
		pool[i] = (r.next_float() - 0.5f) * 2.0f;
		tmp[i] = (r.next_float() - 0.5f) * 3.0f;
		g[i] = (_Float16)((r.next_float() - 0.5f) * 30.0f);
		look[i] = (_Float16)((r.next_float() - 0.5f) * 3.0f);
		ema[i] = (_Float16)tmp[i];
		w16[i] = (_Float16)w[i];
	}
	auto bound = [](double A, int n_ops) { return (n_ops + 2) * std::ldexp(1.0, -24) * A + std::ldexp(1.0, -149); };
	int bad = 0;
	{  // fp16 gradients
		auto d32 = h2d(g32);
		GPUMemory<_Float16> d16(n);
		tcnn_amd::launch_grad_f16(st, d32.data(), d16.data(), 0.5f, n);
		const auto h = d2h<_Float16>(d16.data(), n);
		for (size_t i = 0; i < n; ++i) bad += h[i] != (_Float16)(g32[i] * 0.5f);
	}
	{  // SGD
		const float ls = 128.0f, lr = 0.05f, l2 = 1e-4f;
		auto dw = h2d(w);
		auto dg = h2d(g);
		GPUMemory<_Float16> dh(n);
		tcnn_amd::launch_sgd(st, dw.data(), dh.data(), dg.data(), ls, lr, l2, n);
		const auto hw = d2h<float>(dw.data(), n);
		const auto hh = d2h<_Float16>(dh.data(), n);
		for (size_t i = 0; i < n; ++i) {
			const double gr = (double)g[i] / ls + (double)l2 * w[i], ref = w[i] - (double)lr * gr;
			const double A = std::fabs(w[i]) + lr * (std::fabs((double)g[i] / ls) + std::fabs((double)l2 * w[i]));
			bad += !(std::fabs(hw[i] - ref) <= bound(A, 5)) || hh[i] != (_Float16)hw[i];
		}
	}
	for (int full = 0; full < 2; ++full) {  // EMA, half and full precision
		const float d = 0.95f, o = 0.3f, nw = 2.5f;
		auto dw = h2d(w16);
		auto de = h2d(ema);
		auto dt = h2d(tmp);
		tcnn_amd::launch_ema(st, dw.data(), de.data(), full ? dt.data() : nullptr, d, o, nw, n);
		const auto he = d2h<_Float16>(de.data(), n);
		const auto ht = d2h<float>(dt.data(), n);
		for (size_t i = 0; i < n; ++i) {
			const double prev = full ? (double)tmp[i] : (double)ema[i];
			const double a = prev * d * o, b = (double)w16[i] * (1.0 - (double)d), ref = (a + b) * nw, A = (std::fabs(a) + std::fabs(b)) * nw;
			if (full) bad += !(std::fabs(ht[i] - ref) <= bound(A, 6)) || he[i] != (_Float16)ht[i];
			else bad += !(std::fabs((double)he[i] - ref) <= bound(A, 6) + ulp16(ref)) || ht[i] != tmp[i];
		}
	}
	{  // Lookahead
		const float alpha = 0.25f;
		auto dw = h2d(w);
		auto dl = h2d(look);
		GPUMemory<_Float16> dh(n);
		tcnn_amd::launch_lookahead(st, dw.data(), dh.data(), dl.data(), alpha, n);
		const auto hw = d2h<float>(dw.data(), n);
		const auto hh = d2h<_Float16>(dh.data(), n), hl = d2h<_Float16>(dl.data(), n);
		for (size_t i = 0; i < n; ++i) {
			const double a = (double)look[i] * (1.0 - (double)alpha), b = (double)w[i] * alpha;
			bad += !(std::fabs(hw[i] - (a + b)) <= bound(std::fabs(a) + std::fabs(b), 4)) || hh[i] != (_Float16)hw[i] || hl[i] != hh[i];
		}
	}
	for (int first = 0; first < 2; ++first) {  // the Batched pool and its cast
		auto dg = h2d(g);
		auto dp = h2d(pool);
		GPUMemory<_Float16> dh(n);
		tcnn_amd::launch_batched_pool(st, dg.data(), dp.data(), 3, first != 0, n);
		tcnn_amd::launch_pool_cast(st, dp.data(), dh.data(), n);
		const auto hp = d2h<float>(dp.data(), n);
		const auto hh = d2h<_Float16>(dh.data(), n);
		for (size_t i = 0; i < n; ++i) {
			const double p = first ? 0.0 : (double)pool[i], q = (double)g[i] / 3.0;
			bad += !(std::fabs(hp[i] - (p + q)) <= bound(std::fabs(p) + std::fabs(q), 2)) || hh[i] != (_Float16)hp[i];
		}
	}
	if (bad) std::printf("FAIL optimizer kernels on %zu parameters: %d mismatches\n", n, bad);
	g_fail += bad != 0;
}

int main() {
	try {
		hipStream_t stream;
		HIP_CHECK_THROW(hipStreamCreate(&stream));

		// ---- create_optimizer: the otypes, their nesting, the refusals (optimizer.cu:49-80) ----
		for (const char* otype : {"Average", "Novograd", "Composite", "Shampoo", "Nope"}) {
			const std::string direct = thrown([&] { delete create_optimizer<network_precision_t>({{"otype", otype}}); });
			json nested = {{"otype", "Ema"}};
			nested["nested"] = {{"otype", otype}};
			const std::string inner = thrown([&] { delete create_optimizer<network_precision_t>(nested); });
			EXPECT(contains(direct, otype) && contains(direct, "supported: Adam, SGD, ExponentialDecay, Ema, Lookahead, Batched"));
			EXPECT(inner == direct);
		}
		EXPECT(contains(thrown([] { delete create_optimizer<network_precision_t>({{"otype", "Shampoo"}}); }),
		                "Cannot create `ShampooOptimizer` because tiny-cuda-nn was not compiled with cuBLAS and cuSolver."));
		EXPECT(contains(thrown([] { delete create_optimizer<network_precision_t>({{"otype", "Nope"}}); }), "Invalid optimizer type: Nope"));

		json opt = {{"otype", "Ema"}, {"decay", 0.9f}};
		opt["nested"] = {{"otype", "ExponentialDecay"}, {"decay_start", 1}, {"decay_interval", 1}, {"decay_end", 2}, {"decay_base", 0.5f}};
		opt["nested"]["nested"] = {{"otype", "adam"}, {"learning_rate", 1e-2f}, {"beta2", 0.99f}, {"epsilon", 1e-15f}};
		std::shared_ptr<Optimizer<network_precision_t>> po{create_optimizer<network_precision_t>(opt)};
		EXPECT(po->learning_rate() == 1e-2f && po->step() == 0 && po->custom_weights() == nullptr);  // not attached yet

		const json enc = {{"otype", "HashGrid"}, {"n_levels", 16}, {"n_features_per_level", 2}, {"log2_hashmap_size", 10},
		                  {"base_resolution", 16}, {"per_level_scale", 1.5f}};
		const json net = {{"otype", "FullyFusedMLP"}, {"activation", "ReLU"}, {"output_activation", "None"}, {"n_neurons", 64},
		                  {"n_hidden_layers", 2}};
		std::shared_ptr<NetworkWithInputEncoding<network_precision_t>> model{new NetworkWithInputEncoding<network_precision_t>(2, 3, enc, net)};
		std::shared_ptr<Loss<network_precision_t>> loss{create_loss<network_precision_t>({{"otype", "RelativeL2"}})};
		Trainer<float, network_precision_t, network_precision_t> tr(model, po, loss, 1337);
		const size_t np = tr.n_params();
		EXPECT(tr.params_inference() != tr.params() && po->custom_weights() == tr.params_inference());
		// initialize_params: the custom weights start as the fp16 parameters
		EXPECT(d2h<uint16_t>(tr.params_inference(), np) == d2h<uint16_t>(tr.params(), np));

		const uint32_t n = 512;
		default_rng_t rng{1337};
		GPUMatrix<float> batch(2, n), target(3, n);
		generate_random_uniform<float>(stream, rng, 2 * n, batch.data());
		hipLaunchKernelGGL(field, dim3(n / 256), dim3(256), 0, stream, n, batch.data(), target.data());

		// 4 steps: the learning rate halves before steps 2 and 3 (nested counts 1 and 2) and then stays;
		// the averaged weights follow ema.h:57-59 on the fp16 parameters of every step
		const float rates[4] = {1e-2f, 1e-2f * 0.5f, 1e-2f * 0.5f * 0.5f, 1e-2f * 0.5f * 0.5f};
		// beside the average in double: its absolute-mode value (every term's magnitude) and the bound of what
		// the half-precision steps add -- each step rounds its fp32 result ((6 + 2) 2^-24 A) once to fp16 (one
		// ulp of A at the most) and carries the earlier steps' error on, scaled by decay x debias_old x debias_new
		std::vector<double> avg(np, 0.0), mag(np, 0.0), err(np, 0.0);
		for (uint32_t s = 1; s <= 4; ++s) {
			auto ctx = tr.training_step(stream, batch, target);
			EXPECT(std::isfinite(tr.loss(stream, *ctx)));
			EXPECT(po->step() == s && po->learning_rate() == rates[s - 1]);
			const auto w16 = d2h<_Float16>(tr.params(), np);
			const float old = 1 - (float)std::pow((double)0.9f, (double)(s - 1)), nw = 1.0f / (1 - (float)std::pow((double)0.9f, (double)s));
			for (size_t i = 0; i < np; ++i) {
				avg[i] = (avg[i] * 0.9f * old + (double)w16[i] * (1.0 - (double)0.9f)) * nw;
				mag[i] = (mag[i] * 0.9f * old + std::fabs((double)w16[i]) * (1.0 - (double)0.9f)) * nw;
				err[i] = err[i] * 0.9f * old * nw + ulp16(mag[i]) + 8 * std::ldexp(mag[i], -24);
			}
		}
		{
			const auto ema = d2h<_Float16>(tr.params_inference(), np);
			const auto w16 = d2h<_Float16>(tr.params(), np);
			int bad = 0, differ = 0;
			for (size_t i = 0; i < np; ++i) {
				bad += !(std::fabs((double)ema[i] - avg[i]) <= err[i]);
				differ += ema[i] != w16[i];
			}
			EXPECT(bad == 0);
			EXPECT(differ > 0);
		}
		// hyperparams echo the tree; each level takes its own keys
		json hp = tr.hyperparams()["optimizer"];
		EXPECT(hp["otype"] == "EMA" && hp["nested"]["otype"] == "ExponentialDecay" && hp["nested"]["nested"]["otype"] == "Adam");
		json upd = {{"decay", 0.5f}};
		upd["nested"] = {{"decay_end", 100}};
		tr.update_hyperparams({{"optimizer", upd}});
		hp = po->hyperparams();
		EXPECT(hp["decay"] == 0.5f && hp["nested"]["decay_end"] == 100 && hp["nested"]["decay_base"] == 0.5f);
		EXPECT(po->config()["nested"]["decay_end"] == 100 && po->config()["nested"]["decay_start"] == 1);
		po->set_learning_rate(8e-3f);  // stored as value / factor, reported as the value
		EXPECT(po->learning_rate() == (8e-3f / 0.25f) * 0.25f);

		// inference and a forward with use_inference_params read the averaged weights; a backward does not
		GPUMatrix<float> out(3, n);
		model->inference(stream, batch, out);
		auto fi = tr.forward(stream, 128.0f, batch, target, nullptr, /*use_inference_params=*/true);
		auto ft = tr.forward(stream, 128.0f, batch, target);
		HIP_CHECK_THROW(hipStreamSynchronize(stream));
		const auto ho = out.to_cpu_vector();
		const auto oi = d2h<_Float16>(fi->output.data(), (size_t)16 * n), ot = d2h<_Float16>(ft->output.data(), (size_t)16 * n);
		int diff_i = 0, diff_t = 0;
		for (uint32_t i = 0; i < n; ++i)
			for (uint32_t k = 0; k < 3; ++k) {
				diff_i += (float)oi[(size_t)i * 16 + k] != ho[(size_t)i * 3 + k];
				diff_t += (float)ot[(size_t)i * 16 + k] != ho[(size_t)i * 3 + k];
			}
		EXPECT(diff_i == 0);
		EXPECT(diff_t > 0);  // the training parameters give another output
		EXPECT(std::isfinite(tr.loss(stream, *fi)));
		EXPECT(contains(thrown([&] { tr.backward(stream, *fi, batch); }), "use_inference_params"));
		EXPECT(contains(thrown([&] { tr.backward(stream, *ft, batch, nullptr, /*use_inference_params=*/true); }), "use_inference_params"));
		EXPECT(contains(thrown([&] { tr.training_step(stream, batch, target, nullptr, true, nullptr, /*use_inference_params=*/true); }),
		                "use_inference_params"));
		tr.backward(stream, *ft, batch);  // the ordinary halves still step the tree
		tr.optimizer_step(stream, 128.0f);
		EXPECT(po->step() == 5);

		// snapshot: params_binary holds the averaged weights; deserialize sets both parameter sets from it
		const auto ema = d2h<uint16_t>(tr.params_inference(), np);
		const json snap = tr.serialize(true);
		EXPECT(snap["optimizer"].count("weights_ema_binary") && snap["optimizer"]["nested"].count("learning_rate_factor") &&
		       snap["optimizer"]["nested"]["nested"].count("first_moments_binary"));
		tr.deserialize(snap);
		EXPECT(d2h<uint16_t>(tr.params(), np) == ema && d2h<uint16_t>(tr.params_inference(), np) == ema && po->step() == 5);

		// an optimizer without custom weights: one parameter set
		std::shared_ptr<Optimizer<network_precision_t>> sgd{create_optimizer<network_precision_t>({{"otype", "SGD"}, {"learning_rate", 0.02f}})};
		std::shared_ptr<NetworkWithInputEncoding<network_precision_t>> m2{new NetworkWithInputEncoding<network_precision_t>(2, 3, enc, net)};
		Trainer<float, network_precision_t, network_precision_t> ts(m2, sgd, loss, 1337);
		EXPECT(ts.params_inference() == ts.params() && sgd->custom_weights() == nullptr && sgd->learning_rate() == 0.02f);
		auto c0 = ts.training_step(stream, batch, target, nullptr, true, nullptr, /*use_inference_params=*/true);  // the same set: allowed
		EXPECT(sgd->step() == 1 && std::isfinite(ts.loss(stream, *c0)));

		// ---- the kernels on counts that are no multiple of 8, of the workgroup span, or both ----
		EXPECT(tcnn_amd::optimizer_kernel_span() == 2048);
		for (size_t cnt : {(size_t)5, (size_t)8, (size_t)2048, (size_t)2 * 2048 + 13}) kernel_checks(stream, cnt);

		HIP_CHECK_THROW(hipStreamSynchronize(stream));
		HIP_CHECK_THROW(hipStreamDestroy(stream));
	} catch (const std::exception& e) {
		std::printf("FAIL exception: %s\n", e.what());
		return 1;
	}
	if (g_fail) return 1;
	std::printf("optimizer_api ok: Ema / ExponentialDecay / Adam through tcnn::Trainer, kernels on odd counts\n");
	return 0;
}
