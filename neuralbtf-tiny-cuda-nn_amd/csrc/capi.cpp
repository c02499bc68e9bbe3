// capi.cpp -- extern "C" boundary (include/tcnn_mi355x.h). Exceptions stop here and become return
// codes + tcnn_last_error().
#include "../../include/tcnn_mi355x.h"
#include "debug_api.h"  // test-only diagnostics, not in the product header
#include "debug_adam.h"
#include "debug_grid_bwd.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <mutex>

#include "loss_device.h"
#include "loss_torch.h"
#include "optimizers.h"
#include "runtime.h"

using namespace tcnn_amd;

namespace {
thread_local std::string g_last_error;
thread_local std::string g_str;

std::mutex g_log_mutex;
tcnn_log_callback_t g_log_cb = nullptr;
void* g_log_user = nullptr;

template <typename F>
int guard(F&& f) {
	try {
		f();
		return 0;
	} catch (const std::exception& e) {
		g_last_error = e.what();
	} catch (...) {
		g_last_error = "unknown C++ exception";
	}
	return 1;
}

template <typename T, typename F>
T* guard_ptr(F&& f) {
	try {
		return f();
	} catch (const std::exception& e) {
		g_last_error = e.what();
	} catch (...) {
		g_last_error = "unknown C++ exception";
	}
	return nullptr;
}

json parse_json(const char* s) {
	if (!s || !*s) return json::object();
	return json::parse(std::string(s));
}

// ---- runtime module (cpp_api.cu:64-140) ----
// What a forward keeps for its backward (the reference's tcnn::Context, cpp_api.cu:84-94). Buffers come
// from a pool the module and its contexts share, so a context may outlive its module, and steady-state
// training allocates nothing. Like the reference's stream arenas, a context's buffer is stream-ordered:
// the backward must run on the forward's stream (or after it).
struct KeepPool {
	std::mutex mu;
	std::vector<std::unique_ptr<DevBuf>> free;
	std::unique_ptr<DevBuf> get() {
		std::lock_guard<std::mutex> lk(mu);
		if (free.empty()) return std::make_unique<DevBuf>();
		auto b = std::move(free.back());
		free.pop_back();
		return b;
	}
	void put(std::unique_ptr<DevBuf> b) {
		std::lock_guard<std::mutex> lk(mu);
		if (free.size() < 4) free.push_back(std::move(b));  // keeps two forwards in flight without allocating
	}
};

struct ModuleCtx {
	virtual ~ModuleCtx() = default;
};

struct NwieCtx : ModuleCtx {
	std::shared_ptr<KeepPool> pool;
	std::unique_ptr<DevBuf> keep;
	int layout = 0;
	const float* in = nullptr;
	const void* params = nullptr;
	~NwieCtx() override {
		if (pool && keep) pool->put(std::move(keep));
	}
};

struct ModuleBase {
	virtual ~ModuleBase() = default;
	virtual void inference(hipStream_t st, uint32_t n, const float* in, void* out, const void* params) = 0;
	virtual std::unique_ptr<ModuleCtx> forward(hipStream_t st, uint32_t n, const float* in, void* out, const void* params, bool prep) = 0;
	virtual void backward(hipStream_t st, const ModuleCtx* ctx, uint32_t n, float* dL_din, const void* dL_dout, void* dL_dparams,
	                      const float* in, const void* out, const void* params) = 0;
	// tcnn_module_backward_scaled specialised by the module (false: the generic scale / backward /
	// divide sequence runs instead)
	virtual bool backward_scaled(hipStream_t, const ModuleCtx*, uint32_t, float*, const void*, void*, const float*, const void*,
	                             const void*, float, bool) {
		return false;
	}
	// object.h:278-288: only encodings that define it (the grid) support second-order gradients; beyond the
	// reference, an fp32 network module does too (ModuleNWIEF32)
	virtual void backward_backward_input(hipStream_t, const ModuleCtx*, uint32_t, const float*, const float*, const void*, void*, void*,
	                                     float*, const void*) {
		throw std::runtime_error("DifferentiableObject::backward_backward_input_impl: not implemented error");
	}
	virtual GridEncodingHost* grid_encoding() { return nullptr; }
	// precision of the parameters, the output, dL/doutput and dL/dparams (TCNN_PRECISION_*): fp16 for
	// every module but an encoding or a network created with Fp32
	virtual int precision() const { return TCNN_PRECISION_FP16; }
	size_t elem_bytes() const { return precision() == TCNN_PRECISION_FP32 ? 4 : 2; }
	virtual const char* engine() const { return "encoding"; }
	virtual const char* inference_engine() const { return "encoding"; }
	virtual const char* backward_kernel(bool) const { return "encoding"; }
	virtual uint32_t n_input_dims() const = 0;
	virtual uint32_t n_output_dims() const = 0;
	virtual uint64_t n_params() const = 0;
	virtual uint64_t n_network_params() const { return 0; }  // the matrix parameters, which come first
	virtual void initialize_params(uint64_t seed, float* params_fp32, float scale) = 0;
	virtual json hyperparams() const = 0;
	virtual std::string name() const = 0;
	std::string scratch;
};

void check_batch(uint32_t n) {
	TCNN_CHECK(n % BATCH_GRANULARITY == 0, "Batch size must be a multiple of " + std::to_string(BATCH_GRANULARITY));
}

struct ModuleNWIE : ModuleBase {
	NetworkHost model;
	StepWorkspace ws;
	DevBuf grad32;
	std::shared_ptr<KeepPool> pool = std::make_shared<KeepPool>();
	ModuleNWIE(uint32_t n_in, uint32_t n_out, const json& enc, const json& net) : model(n_in, n_out, enc, net, LOSS_RELATIVE_L2) {}
	void inference(hipStream_t st, uint32_t n, const float* in, void* out, const void* params) override {
		check_batch(n);
		model.inference(st, ws, n, in, params, out);
	}
	// The context keeps the encoding of this batch in the layout the backward reads, so the backward
	// does not encode again (the fused grid kernel skips its gathers; the tile engine its encoding pass).
	std::unique_ptr<ModuleCtx> forward(hipStream_t st, uint32_t n, const float* in, void* out, const void* params, bool prep) override {
		check_batch(n);
		auto c = std::make_unique<NwieCtx>();
		c->pool = pool;
		if (model.sw.no_forward_keep) {  // A/B switch (read when the module is built): the backward recomputes the forward
			model.inference(st, ws, n, in, params, out);
			c->layout = NetworkHost::KEEP_NONE;
			return c;
		}
		c->keep = pool->get();
		c->layout = model.forward_keep(st, ws, n, in, params, out, prep, *c->keep);
		c->in = in;
		c->params = params;
		return c;
	}
	void backward(hipStream_t st, const ModuleCtx* ctx, uint32_t n, float* dL_din, const void* dL_dout, void* dL_dparams, const float* in,
	              const void*, const void* params) override {
		check_batch(n);
		if (!dL_dparams && !dL_din) return;
		model.fwd_bwd(st, ws, pass(ctx, n, in, params, dL_dout, dL_din));
		if (dL_dparams) launch_cast_f32_f16(st, grad32.as<float>(), dL_dparams, n_params());
	}
	// the backward of a batch as the engine takes it: external dL/dy, gradients into grad32
	TrainPass pass(const ModuleCtx* ctx, uint32_t n, const float* in, const void* params, const void* dL_dout, float* dL_din) {
		grad32.reserve(n_params() * 4);
		TrainPass p;
		p.B = n;
		p.pos = in;
		p.params16 = params;
		p.dims = model.n_output_dims;
		p.dout16 = dL_dout;
		p.grad32 = grad32.as<float>();
		p.dL_dinput = dL_din;
		// the kept encoding describes this batch only if the backward sees the forward's input and parameters
		const NwieCtx* c = dynamic_cast<const NwieCtx*>(ctx);
		if (c && c->keep && c->layout != NetworkHost::KEEP_NONE && c->in == in && c->params == params) {
			p.kept = c->keep->p;
			p.kept_layout = c->layout;
		}
		return p;
	}
	// the torch binding's backward in as few launches as the engine allows: the loss scale folded
	// into the fused kernel's dL/dy load (or one scaling pass for the other engines), the gradient
	// finalised as fp16(fp16(g) / s) in one pass (launch_grad_finalize) instead of a cast and a division
	bool backward_scaled(hipStream_t st, const ModuleCtx* ctx, uint32_t n, float* dL_din, const void* dL_dout, void* dL_dparams,
	                     const float* in, const void*, const void* params, float s, bool dparams_f32) override {
		check_batch(n);
		if (!dL_dparams && !dL_din) return true;
		TrainPass p = pass(ctx, n, in, params, dL_dout, dL_din);
		p.dout_scale = s;
		if (dL_dparams) p.fin = GradFinalize{dL_dparams, s, dparams_f32 ? 1 : 0};
		const bool finalised = model.fwd_bwd(st, ws, p);
		if (dL_din) launch_div_f32(st, dL_din, s, (size_t)n * model.n_input_dims);
		if (dL_dparams && !finalised) launch_grad_finalize(st, grad32.as<float>(), dL_dparams, s, n_params(), dparams_f32);
		return true;
	}
	GridEncodingHost* grid_encoding() override { return model.grid; }
	const char* engine() const override { return model.engine(); }
	const char* inference_engine() const override { return model.inference_engine(); }
	const char* backward_kernel(bool with_dinput) const override { return model.backward_kernel(with_dinput); }
	uint32_t n_input_dims() const override { return model.n_input_dims; }
	uint32_t n_output_dims() const override { return model.mlp.padded_output; }
	uint64_t n_params() const override { return model.n_params(); }
	uint64_t n_network_params() const override { return model.mlp.n_params(); }
	void initialize_params(uint64_t seed, float* p, float scale) override {
		Pcg32 rng{seed};
		std::vector<float> host(n_params());
		model.initialize_params(rng, host.data(), scale);
		TCNN_HIP_CHECK(hipMemcpy(p, host.data(), host.size() * 4, hipMemcpyHostToDevice));
	}
	json hyperparams() const override { return model.hyperparams(); }
	std::string name() const override { return "NetworkWithInputEncoding"; }
};

// NetworkWithInputEncoding at fp32 precision (tcnn_create_network*_precision with Fp32): parameters, output,
// dL/doutput, dL/dparams fp32, on the f32-MFMA layer kernels behind the fp32 encoding. The forward's context
// keeps the encoded rows, every hidden activation and the output; TCNN_NO_FORWARD_KEEP (or a backward that sees
// other inputs or parameters than the forward) recomputes them.
struct NwieF32Ctx : ModuleCtx {
	std::shared_ptr<KeepPool> pool;
	std::unique_ptr<DevBuf> keep;
	const float* in = nullptr;
	const void* params = nullptr;
	~NwieF32Ctx() override {
		if (pool && keep) pool->put(std::move(keep));
	}
};

struct ModuleNWIEF32 : ModuleBase {
	NetworkF32Host model;
	DevBuf rekeep;
	std::shared_ptr<KeepPool> pool = std::make_shared<KeepPool>();
	ModuleNWIEF32(uint32_t n_in, uint32_t n_out, const json& enc, const json& net) : model(n_in, n_out, enc, net) {}
	int precision() const override { return TCNN_PRECISION_FP32; }
	void inference(hipStream_t st, uint32_t n, const float* in, void* out, const void* params) override {
		check_batch(n);
		model.forward(st, n, in, (const float*)params, (float*)out, nullptr);
	}
	std::unique_ptr<ModuleCtx> forward(hipStream_t st, uint32_t n, const float* in, void* out, const void* params, bool) override {
		check_batch(n);
		TCNN_CHECK(!model.has_sine(), "Sine has no backward from its forward value: a forward that keeps a context is refused (use inference)");
		auto c = std::make_unique<NwieF32Ctx>();
		if (model.sw.no_forward_keep) {  // A/B switch (read when the module is built): the backward recomputes the forward
			model.forward(st, n, in, (const float*)params, (float*)out, nullptr);
			return c;
		}
		c->pool = pool;
		c->keep = pool->get();
		c->keep->reserve(model.keep_floats(n) * 4);
		model.forward(st, n, in, (const float*)params, (float*)out, c->keep->as<float>());
		c->in = in;
		c->params = params;
		return c;
	}
	void backward(hipStream_t st, const ModuleCtx* ctx, uint32_t n, float* dL_din, const void* dL_dout, void* dL_dparams, const float* in,
	              const void*, const void* params) override {
		check_batch(n);
		if (!dL_dparams && !dL_din) return;
		model.backward(st, n, in, (const float*)params, (const float*)dL_dout, kept(st, ctx, n, in, params), (float*)dL_dparams, dL_din);
	}
	// the context's activations if they describe this batch (the backward sees the forward's input and parameters),
	// else the forward again into the module's own buffer
	const float* kept(hipStream_t st, const ModuleCtx* ctx, uint32_t n, const float* in, const void* params) {
		const NwieF32Ctx* c = dynamic_cast<const NwieF32Ctx*>(ctx);
		if (c && c->keep && c->in == in && c->params == params) return c->keep->as<float>();
		rekeep.reserve(model.keep_floats(n) * 4);
		model.forward(st, n, in, (const float*)params, nullptr, rekeep.as<float>());
		return rekeep.as<float>();
	}
	// Second order with respect to the input (beyond the reference, whose networks have none): every non-null
	// output is overwritten; dL_dout may be null only for the tangent pass alone (dL_ddLdout)
	void backward_backward_input(hipStream_t st, const ModuleCtx* ctx, uint32_t n, const float* dL_ddLdin, const float* in,
	                             const void* dL_dout, void* dL_dparams, void* dL_ddLdout, float* dL_din, const void* params) override {
		check_batch(n);
		model.check_second_order();
		if (!dL_dparams && !dL_ddLdout && !dL_din) return;
		TCNN_CHECK(dL_dout || (!dL_dparams && !dL_din),
		           "backward_backward_input: dL_doutput may be null only when dL_dparams and dL_dinput are (the tangent pass alone)");
		TCNN_CHECK(params && in && dL_ddLdin, "backward_backward_input needs the input, the parameters and dL_ddLdinput");
		model.backward_backward_input(st, n, in, (const float*)params, dL_ddLdin, (const float*)dL_dout, kept(st, ctx, n, in, params),
		                              (float*)dL_dparams, (float*)dL_ddLdout, dL_din);
	}
	GridEncodingHost* grid_encoding() override { return model.enc->lone_grid(); }
	const char* engine() const override { return "layered"; }
	const char* inference_engine() const override { return "layered"; }
	const char* backward_kernel(bool) const override { return "layered"; }
	uint32_t n_input_dims() const override { return model.n_input_dims; }
	uint32_t n_output_dims() const override { return model.mlp.padded_output; }
	uint64_t n_params() const override { return model.n_params(); }
	uint64_t n_network_params() const override { return model.mlp.n_params(); }
	void initialize_params(uint64_t seed, float* p, float scale) override {
		Pcg32 rng{seed};
		std::vector<float> host(n_params());
		model.initialize_params(rng, host.data(), scale);
		TCNN_HIP_CHECK(hipMemcpy(p, host.data(), host.size() * 4, hipMemcpyHostToDevice));
	}
	json hyperparams() const override { return model.hyperparams(); }
	std::string name() const override { return "NetworkWithInputEncoding"; }
};

// Every encoding as a module (cpp_api.cu:145-149); its grids make it own parameters and a gradient
// buffer. Encoding modules take any batch size (per-point kernels with bounds checks, like the
// reference); networks keep the 256 rule.
struct ModuleEncoding : ModuleBase {
	EncodingHost enc;
	DevBuf grad32;
	ModuleEncoding(uint32_t n_in, const json& j, uint32_t alignment, bool f32) : enc(n_in, j, f32) {
		if (alignment > 0) enc.set_alignment(alignment);
	}
	int precision() const override { return enc.f32 ? TCNN_PRECISION_FP32 : TCNN_PRECISION_FP16; }
	void inference(hipStream_t st, uint32_t n, const float* in, void* out, const void* params) override {
		enc.forward_aos(st, n, in, params, out);
	}
	std::unique_ptr<ModuleCtx> forward(hipStream_t st, uint32_t n, const float* in, void* out, const void* params, bool) override {
		inference(st, n, in, out, params);  // nothing to keep: the backward recomputes dy/dx
		return nullptr;
	}
	void backward(hipStream_t st, const ModuleCtx*, uint32_t n, float* dL_din, const void* dL_dout, void* dL_dparams, const float* in,
	              const void*, const void* params) override {
		if (dL_din) enc.backward_input(st, n, in, dL_dout, dL_din, params);
		if (!dL_dparams || !enc.n_params()) return;
		if (enc.f32) return enc.backward_params(st, n, in, dL_dout, 2, (float*)dL_dparams);  // fp32 dL/dparams: the sums themselves
		grad32.reserve((size_t)enc.n_params() * 4);
		enc.backward_params(st, n, in, dL_dout, 2, grad32.as<float>());
		launch_cast_f32_f16(st, grad32.as<float>(), dL_dparams, enc.n_params());
	}
	// a grid standing alone; grids nested in a composite keep ModuleBase's "not implemented"
	void backward_backward_input(hipStream_t st, const ModuleCtx* ctx, uint32_t n, const float* dL_ddLdin, const float* in,
	                             const void* dL_dout, void* dL_dparams, void* dL_ddLdout, float* dL_din, const void* params) override {
		const GridEncodingHost* grid = enc.lone_grid();
		if (!grid) return ModuleBase::backward_backward_input(st, ctx, n, dL_ddLdin, in, dL_dout, dL_dparams, dL_ddLdout, dL_din, params);
		if (!dL_ddLdout && !dL_dparams) return;  // grid.h:913-915
		TCNN_CHECK(params, "backward_backward_input needs the grid parameters");
		const uint32_t W = enc.padded_output_width();
		if (enc.f32) {  // fp32 module: the fp32 atomics accumulate straight into dL/dparams
			if (dL_dparams) TCNN_HIP_CHECK(hipMemsetAsync(dL_dparams, 0, (size_t)grid->n_params * 4, st));  // GradientMode::Overwrite
			return grid->backward_backward_input(st, n, in, enc.n_dims, (const float*)params, dL_ddLdin, (const float*)dL_dout, W,
			                                     (float*)dL_dparams, (float*)dL_ddLdout, W, dL_din);
		}
		if (dL_dparams) {
			grad32.reserve((size_t)grid->n_params * 4);
			TCNN_HIP_CHECK(hipMemsetAsync(grad32.p, 0, (size_t)grid->n_params * 4, st));  // GradientMode::Overwrite
		}
		grid->backward_backward_input(st, n, in, enc.n_dims, (const _Float16*)params, dL_ddLdin, (const _Float16*)dL_dout, W,
		                              dL_dparams ? grad32.as<float>() : nullptr, (_Float16*)dL_ddLdout, W, dL_din);
		if (dL_dparams) launch_cast_f32_f16(st, grad32.as<float>(), dL_dparams, grid->n_params);
	}
	// the lone grid (nullptr: a lone OneBlob / Identity); max_level does not go through the composite kernels yet
	GridEncodingHost* grid_encoding() override {
		if (!enc.lone_part()) throw std::runtime_error(enc.name() + ": max_level is not implemented by the MI355X engine yet");
		return enc.lone_grid();
	}
	uint32_t n_input_dims() const override { return enc.n_dims; }
	uint32_t n_output_dims() const override { return enc.padded_output_width(); }
	uint64_t n_params() const override { return enc.n_params(); }
	void initialize_params(uint64_t seed, float* p, float scale) override {
		if (!enc.n_params()) return;
		Pcg32 rng{seed};
		std::vector<float> host(enc.n_params());
		enc.initialize_params(rng, host.data(), scale);
		TCNN_HIP_CHECK(hipMemcpy(p, host.data(), host.size() * 4, hipMemcpyHostToDevice));
	}
	json hyperparams() const override { return enc.hyperparams(); }
	std::string name() const override { return enc.name(); }
};
}  // namespace

struct tcnn_module {
	std::unique_ptr<ModuleBase> m;
	DevBuf dout_scaled, dparams16;  // tcnn_module_backward_scaled's temporaries
};
struct tcnn_context {
	uint32_t n = 0;
	std::unique_ptr<ModuleCtx> impl;  // what the forward kept (nullptr: nothing)
};
struct tcnn_trainer {
	std::unique_ptr<TrainerHost> t;
};
struct tcnn_dp_comm {
	std::unique_ptr<DpComm> c;
};

extern "C" {

const char* tcnn_last_error(void) { return g_last_error.c_str(); }
const char* tcnn_version(void) { return "tcnn-mi355x 0.1 (gfx950)"; }
uint32_t tcnn_batch_size_granularity(void) { return BATCH_GRANULARITY; }
int tcnn_cuda_device(void) {
	int d = -1;
	if (hipGetDevice(&d) != hipSuccess) return -1;
	return d;
}
int tcnn_set_cuda_device(int device) {
	return guard([&] { TCNN_HIP_CHECK(hipSetDevice(device)); });
}
void tcnn_free_temporary_memory(void) {  // free_all_gpu_memory_arenas (gpu_memory.h:751-754)
	try {
		tcnn_amd::workspace_arena_free_all();
	} catch (...) {
	}
}
int tcnn_has_networks(void) { return 1; }

int tcnn_generate_random_logistic(void* stream, uint64_t* rng_state, uint64_t* rng_inc, uint64_t n, float* out, float mean, float stddev) {
	return guard([&] {
		TCNN_CHECK(rng_state && rng_inc, "generate_random_logistic: rng state missing");
		launch_generate_logistic((hipStream_t)stream, n, *rng_state, *rng_inc, out, mean, stddev);
		Pcg32 r;
		r.state = *rng_state;
		r.inc = *rng_inc;
		r.advance((int64_t)n);  // random.h:64
		*rng_state = r.state;
	});
}
int tcnn_generate_random_uniform(void* stream, uint64_t* rng_state, uint64_t* rng_inc, uint64_t n, float* out, float lower, float upper) {
	return guard([&] {
		TCNN_CHECK(rng_state && rng_inc, "generate_random_uniform: rng state missing");
		launch_generate_uniform((hipStream_t)stream, n, *rng_state, *rng_inc, out, lower, upper);
		Pcg32 r;
		r.state = *rng_state;
		r.inc = *rng_inc;
		r.advance((int64_t)n);  // rng.advance(n_elements), random.h:64
		*rng_state = r.state;
	});
}

void tcnn_set_log_callback(tcnn_log_callback_t cb, void* user) {
	std::lock_guard<std::mutex> lk(g_log_mutex);
	g_log_cb = cb;
	g_log_user = user;
}
float tcnn_default_loss_scale(int precision) { return precision == TCNN_PRECISION_FP32 ? 1.0f : 128.0f; }
int tcnn_preferred_precision(void) { return TCNN_PRECISION_FP16; }

tcnn_module* tcnn_create_network_with_input_encoding(uint32_t n_in, uint32_t n_out, const char* enc, const char* net) {
	return guard_ptr<tcnn_module>([&] {
		auto* r = new tcnn_module;
		r->m = std::make_unique<ModuleNWIE>(n_in, n_out, parse_json(enc), parse_json(net));
		return r;
	});
}

// create_network = Identity encoding + network (cpp_api.cu:151-153)
tcnn_module* tcnn_create_network(uint32_t n_in, uint32_t n_out, const char* net) {
	return guard_ptr<tcnn_module>([&] {
		auto* r = new tcnn_module;
		r->m = std::make_unique<ModuleNWIE>(n_in, n_out, json{{"otype", "Identity"}}, parse_json(net));
		return r;
	});
}

// The two constructors with the module's precision: Fp16 is the module the constructors above create, Fp32
// an fp32 network module (ModuleNWIEF32).
tcnn_module* tcnn_create_network_with_input_encoding_precision(uint32_t n_in, uint32_t n_out, const char* enc, const char* net,
                                                               int precision) {
	return guard_ptr<tcnn_module>([&] {
		TCNN_CHECK(precision == TCNN_PRECISION_FP16 || precision == TCNN_PRECISION_FP32,
		           "create_network_with_input_encoding: precision must be Fp16 or Fp32");
		auto r = std::make_unique<tcnn_module>();
		if (precision == TCNN_PRECISION_FP32) r->m = std::make_unique<ModuleNWIEF32>(n_in, n_out, parse_json(enc), parse_json(net));
		else r->m = std::make_unique<ModuleNWIE>(n_in, n_out, parse_json(enc), parse_json(net));
		return r.release();
	});
}

tcnn_module* tcnn_create_network_precision(uint32_t n_in, uint32_t n_out, const char* net, int precision) {
	return guard_ptr<tcnn_module>([&] {
		TCNN_CHECK(precision == TCNN_PRECISION_FP16 || precision == TCNN_PRECISION_FP32, "create_network: precision must be Fp16 or Fp32");
		auto r = std::make_unique<tcnn_module>();
		const json identity = json{{"otype", "Identity"}};
		if (precision == TCNN_PRECISION_FP32) r->m = std::make_unique<ModuleNWIEF32>(n_in, n_out, identity, parse_json(net));
		else r->m = std::make_unique<ModuleNWIE>(n_in, n_out, identity, parse_json(net));
		return r.release();
	});
}

// create_encoding<T>(n_dims, encoding, alignment) (encoding.cu:131-145); alignment 0: none. A grid
// standing alone takes no alignment here.
tcnn_module* tcnn_create_encoding_aligned(uint32_t n_in, const char* enc, int precision, uint32_t alignment) {
	return guard_ptr<tcnn_module>([&] {
		TCNN_CHECK(precision == TCNN_PRECISION_FP16 || precision == TCNN_PRECISION_FP32, "create_encoding: precision must be Fp16 or Fp32");
		json j = parse_json(enc);
		const std::string ot = j.is_object() && j.find("otype") != j.end() ? j["otype"].get<std::string>() : "OneBlob";
		TCNN_CHECK(EncodingHost::known(ot), "Encoding '" + ot + "' is not implemented by the MI355X engine yet");
		TCNN_CHECK(alignment == 0 || !EncodingHost::is_grid_otype(ot), "create_encoding: a grid encoding module takes no alignment");
		auto r = std::make_unique<tcnn_module>();
		r->m = std::make_unique<ModuleEncoding>(n_in, j, alignment, precision == TCNN_PRECISION_FP32);
		return r.release();
	});
}

tcnn_module* tcnn_create_encoding(uint32_t n_in, const char* enc, int precision) {
	return tcnn_create_encoding_aligned(n_in, enc, precision, 0);
}

void tcnn_module_destroy(tcnn_module* m) { delete m; }

int tcnn_module_inference(tcnn_module* m, void* stream, uint32_t n, const float* in, void* out, const void* params) {
	if (n == 0) return 0;  // empty batch: nothing to do (every kernel would be a zero-size launch)
	return guard([&] { m->m->inference((hipStream_t)stream, n, in, out, params); });
}

tcnn_context* tcnn_module_forward(tcnn_module* m, void* stream, uint32_t n, const float* in, void* out, const void* params, int prep) {
	return guard_ptr<tcnn_context>([&] {
		auto* c = new tcnn_context;
		c->n = n;
		if (n) c->impl = m->m->forward((hipStream_t)stream, n, in, out, params, prep != 0);
		return c;
	});
}

int tcnn_module_backward(tcnn_module* m, void* stream, const tcnn_context* ctx, uint32_t n, float* dL_din, const void* dL_dout,
                         void* dL_dparams, const float* in, const void* out, const void* params) {
	return guard([&] {
		TCNN_CHECK(ctx != nullptr, "backward: null context");
		if (n == 0) {  // empty batch: Overwrite-mode gradients are all zero
			if (dL_dparams) TCNN_HIP_CHECK(hipMemsetAsync(dL_dparams, 0, m->m->n_params() * m->m->elem_bytes(), (hipStream_t)stream));
			return;
		}
		TCNN_CHECK(ctx->n == n, "backward: batch size differs from the forward's");
		m->m->backward((hipStream_t)stream, ctx->impl.get(), n, dL_din, dL_dout, dL_dparams, in, out, params);
	});
}

int tcnn_module_backward_scaled(tcnn_module* m, void* stream, const tcnn_context* ctx, uint32_t n, float* dL_din, const void* dL_dout,
                                void* dL_dparams, const float* in, const void* out, const void* params, float loss_scale,
                                int dparams_fp32) {
	return guard([&] {
		TCNN_CHECK(ctx != nullptr, "backward: null context");
		TCNN_CHECK(loss_scale != 0.0f, "backward: loss scale must be nonzero");
		const hipStream_t st = (hipStream_t)stream;
		const uint64_t np = m->m->n_params();
		const bool f32 = m->m->precision() == TCNN_PRECISION_FP32;  // fp32 module: dL/dparams is fp32 whatever dparams_fp32 says
		if (n == 0) {
			if (dL_dparams) TCNN_HIP_CHECK(hipMemsetAsync(dL_dparams, 0, np * ((dparams_fp32 || f32) ? 4 : 2), st));
			return;
		}
		TCNN_CHECK(ctx->n == n, "backward: batch size differs from the forward's");
		if (m->m->backward_scaled(st, ctx->impl.get(), n, dL_din, dL_dout, dL_dparams, in, out, params, loss_scale, dparams_fp32 != 0))
			return;
		const size_t n_out = (size_t)n * m->m->n_output_dims();
		if (f32) {  // the same three steps in fp32: dL/dy * s, backward, dL/dinput and dL/dparams divided by s
			m->dout_scaled.reserve(n_out * 4);
			launch_scale_f32(st, (const float*)dL_dout, m->dout_scaled.as<float>(), loss_scale, n_out);
			m->m->backward(st, ctx->impl.get(), n, dL_din, m->dout_scaled.p, dL_dparams, in, out, params);
			if (dL_din) launch_div_f32(st, dL_din, loss_scale, (size_t)n * m->m->n_input_dims());
			if (dL_dparams) launch_div_f32(st, (float*)dL_dparams, loss_scale, np);
			return;
		}
		m->dout_scaled.reserve(n_out * 2);
		launch_scale_f16(st, dL_dout, m->dout_scaled.p, loss_scale, n_out);  // modules.py:135 doutput * loss_scale
		void* g16 = dL_dparams;
		if (dL_dparams && dparams_fp32) {
			m->dparams16.reserve(np * 2);
			g16 = m->dparams16.p;
		}
		m->m->backward(st, ctx->impl.get(), n, dL_din, m->dout_scaled.p, g16, in, out, params);
		if (dL_din) launch_div_f32(st, dL_din, loss_scale, (size_t)n * m->m->n_input_dims());  // modules.py:137
		if (dL_dparams) launch_div_f16(st, g16, dL_dparams, loss_scale, np, dparams_fp32 != 0);  // modules.py:138
	});
}

int tcnn_module_backward_backward_input(tcnn_module* m, void* stream, const tcnn_context* ctx, uint32_t n, const float* dL_ddLdin,
                                        const float* in, const void* dL_dout, void* dL_dparams, void* dL_ddLdout, float* dL_din,
                                        const void* params) {
	return guard([&] {
		TCNN_CHECK(ctx != nullptr, "backward_backward_input: null context");
		if (n == 0) {
			if (dL_dparams) TCNN_HIP_CHECK(hipMemsetAsync(dL_dparams, 0, m->m->n_params() * m->m->elem_bytes(), (hipStream_t)stream));
			return;
		}
		m->m->backward_backward_input((hipStream_t)stream, ctx->impl.get(), n, dL_ddLdin, in, dL_dout, dL_dparams, dL_ddLdout, dL_din, params);
	});
}

void tcnn_context_destroy(tcnn_context* c) { delete c; }

static GridEncodingHost& module_grid(tcnn_module* m) {
	GridEncodingHost* g = m->m->grid_encoding();
	TCNN_CHECK(g != nullptr, "module has no grid encoding");
	return *g;
}
int tcnn_module_set_max_level(tcnn_module* m, float max_level) {
	return guard([&] { module_grid(m).max_level = max_level; });
}
float tcnn_module_max_level(tcnn_module* m) {
	float v = -1.0f;
	guard([&] { v = module_grid(m).max_level; });
	return v;
}
int tcnn_module_set_max_level_gpu(tcnn_module* m, const float* max_level_per_point) {
	return guard([&] { module_grid(m).max_level_gpu = max_level_per_point; });
}
uint32_t tcnn_module_n_input_dims(const tcnn_module* m) { return m->m->n_input_dims(); }
uint32_t tcnn_module_n_output_dims(const tcnn_module* m) { return m->m->n_output_dims(); }
uint64_t tcnn_module_n_params(const tcnn_module* m) { return m->m->n_params(); }
uint64_t tcnn_module_n_network_params(const tcnn_module* m) { return m->m->n_network_params(); }
int tcnn_module_param_precision(const tcnn_module* m) { return m->m->precision(); }
int tcnn_module_output_precision(const tcnn_module* m) { return m->m->precision(); }
int tcnn_module_initialize_params(tcnn_module* m, uint64_t seed, float* p, float scale) {
	return guard([&] { m->m->initialize_params(seed, p, scale); });
}
const char* tcnn_module_hyperparams(tcnn_module* m) {
	m->m->scratch = m->m->hyperparams().dump();
	return m->m->scratch.c_str();
}
const char* tcnn_module_name(tcnn_module* m) {
	m->m->scratch = m->m->name();
	return m->m->scratch.c_str();
}

tcnn_trainer* tcnn_trainer_create(uint32_t n_in, uint32_t n_out, const char* cfg, uint32_t seed) {
	return guard_ptr<tcnn_trainer>([&] {
		auto* r = new tcnn_trainer;
		r->t = std::make_unique<TrainerHost>(n_in, n_out, parse_json(cfg), seed);
		return r;
	});
}
void tcnn_trainer_destroy(tcnn_trainer* t) { delete t; }
int tcnn_trainer_training_step(tcnn_trainer* t, void* stream, uint32_t n, const float* in, const float* target, int run_opt) {
	return guard([&] {
		TCNN_CHECK(n > 0, "training_step: empty batch");
		t->t->training_step((hipStream_t)stream, n, in, target, run_opt != 0);
	});
}
int tcnn_trainer_training_step_part(tcnn_trainer* t, void* stream, uint32_t n, const float* in, const float* target, int part) {
	return guard([&] { t->t->training_step_part((hipStream_t)stream, n, in, target, part); });
}
int tcnn_trainer_optimizer_step(tcnn_trainer* t, void* stream) {
	return guard([&] { t->t->optimizer_step((hipStream_t)stream); });
}
void* tcnn_workspace_allocate(void* stream, uint64_t n_bytes) {
	void* p = nullptr;
	guard([&] { p = workspace_allocate((hipStream_t)stream, n_bytes); });
	return p;
}
int tcnn_workspace_free(void* stream, void* ptr) {
	return guard([&] { workspace_free((hipStream_t)stream, ptr); });
}
int tcnn_free_workspace_arena(void* stream) {
	return guard([&] { workspace_arena_free((hipStream_t)stream); });
}
int tcnn_workspace_arena_info(void* stream, uint64_t* mapped_bytes, int* virtual_memory) {
	return guard([&] { workspace_arena_info((hipStream_t)stream, mapped_bytes, virtual_memory); });
}

struct tcnn_trainer_context {
	std::unique_ptr<TrainerFwdCtx> c;
};
tcnn_trainer_context* tcnn_trainer_forward(tcnn_trainer* t, void* stream, uint32_t n, const float* in, const float* target, const float* pdf,
                                           const void* ext, int prep) {
	tcnn_trainer_context* r = nullptr;
	const int rc = guard([&] {
		TCNN_CHECK(n > 0, "forward: empty batch");
		auto c = t->t->forward((hipStream_t)stream, n, in, target, pdf, ext, prep != 0);
		r = new tcnn_trainer_context{std::move(c)};
	});
	return rc == 0 ? r : nullptr;
}
tcnn_trainer_context* tcnn_trainer_forward_perturbed(tcnn_trainer* t, void* stream, uint32_t n, const float* in, const float* target,
                                                     const float* pdf, const float* perturbation, int prep) {
	tcnn_trainer_context* r = nullptr;
	const int rc = guard([&] {
		TCNN_CHECK(n > 0, "forward: empty batch");
		TCNN_CHECK(target != nullptr, "forward_perturbed: a target is required");
		auto c = t->t->forward((hipStream_t)stream, n, in, target, pdf, nullptr, prep != 0, perturbation);
		r = new tcnn_trainer_context{std::move(c)};
	});
	return rc == 0 ? r : nullptr;
}
tcnn_trainer_context* tcnn_trainer_forward_inference_params(tcnn_trainer* t, void* stream, uint32_t n, const float* in, const float* target,
                                                            const float* pdf, const void* ext) {
	tcnn_trainer_context* r = nullptr;
	const int rc = guard([&] {
		TCNN_CHECK(n > 0, "forward: empty batch");
		auto c = t->t->forward((hipStream_t)stream, n, in, target, pdf, ext, false, nullptr, true);
		r = new tcnn_trainer_context{std::move(c)};
	});
	return rc == 0 ? r : nullptr;
}
int tcnn_trainer_backward(tcnn_trainer* t, void* stream, const tcnn_trainer_context* ctx, uint32_t n, const float* in, float* dL_din,
                          int gradient_mode) {
	return guard([&] {
		TCNN_CHECK(ctx != nullptr, "backward: null context");
		TCNN_CHECK(gradient_mode >= 0 && gradient_mode <= 2, "backward: gradient_mode must be 0 (Overwrite), 1 (Accumulate) or 2 (Ignore)");
		t->t->backward((hipStream_t)stream, *ctx->c, n, in, dL_din, gradient_mode);
	});
}
float tcnn_trainer_context_loss(tcnn_trainer* t, void* stream, const tcnn_trainer_context* ctx) {
	float v = -1.0f;
	guard([&] {
		TCNN_CHECK(ctx != nullptr, "loss: null context");
		v = t->t->ctx_loss((hipStream_t)stream, *ctx->c);
	});
	return v;
}
int tcnn_trainer_context_loss_value(tcnn_trainer* t, void* stream, const tcnn_trainer_context* ctx, float* out) {
	return guard([&] {
		TCNN_CHECK(ctx != nullptr, "loss: null context");
		TCNN_CHECK(out != nullptr, "loss: null result pointer");
		*out = t->t->ctx_loss((hipStream_t)stream, *ctx->c);
	});
}
const void* tcnn_trainer_context_output(const tcnn_trainer_context* ctx) { return ctx ? ctx->c->out16.p : nullptr; }
const void* tcnn_trainer_context_doutput(const tcnn_trainer_context* ctx) { return ctx ? ctx->c->dLdy() : nullptr; }
void tcnn_trainer_context_destroy(tcnn_trainer_context* ctx) { delete ctx; }
uint32_t tcnn_trainer_padded_output_width(const tcnn_trainer* t) { return t->t->model->mlp.padded_output; }
int tcnn_trainer_optimizer_step_range(tcnn_trainer* t, void* stream, uint64_t begin, uint64_t end) {
	return guard([&] { t->t->optimizer_step_range((hipStream_t)stream, begin, end); });
}
int tcnn_dp_unique_id(void* id) {
	return guard([&] { dp_unique_id(id); });
}
tcnn_dp_comm* tcnn_dp_comm_create(const void* id, int nranks, int rank) {
	return guard_ptr<tcnn_dp_comm>([&] {
		auto* r = new tcnn_dp_comm;
		r->c = std::make_unique<DpComm>(id, nranks, rank);
		return r;
	});
}
void tcnn_dp_comm_destroy(tcnn_dp_comm* c) { delete c; }
int tcnn_trainer_set_dp(tcnn_trainer* t, tcnn_dp_comm* c, int sharded) {
	return guard([&] {
		if (c) t->t->require_plain_adam("A data-parallel communicator");
		t->t->set_dp(c ? c->c.get() : nullptr, sharded != 0);
	});
}
uint64_t tcnn_dp_peer_blob_bytes(void) { return tcnn_amd::dp_peer_blob_bytes(); }
int tcnn_trainer_dp_peer_export(tcnn_trainer* t, int nranks, int rank, void* blob) {
	return guard([&] {
		t->t->require_plain_adam("The data-parallel peer exchange");
		t->t->dp_peer_export(nranks, rank, blob);
	});
}
int tcnn_trainer_dp_peer_attach(tcnn_trainer* t, const void* blobs) {
	return guard([&] {
		t->t->require_plain_adam("The data-parallel peer exchange");
		t->t->dp_peer_attach(blobs);
	});
}
int tcnn_trainer_dp_peer_detach(tcnn_trainer* t) {
	return guard([&] { t->t->dp_peer_detach(); });
}
int tcnn_trainer_dp_peer_set_timeout(tcnn_trainer* t, double seconds) {
	return guard([&] { t->t->dp_peer_set_timeout(seconds); });
}
int tcnn_debug_peer_loopback(tcnn_trainer* t, int nranks) {
	return guard([&] {
		t->t->require_plain_adam("The data-parallel peer exchange");
		t->t->dp_peer_loopback(nranks);
	});
}
int tcnn_debug_adam_uniform_blocks(tcnn_trainer* t, uint32_t* n_uniform, uint32_t* n_blocks) {
	return guard([&] {
		if (n_blocks) *n_blocks = t->t->n_step_blocks();
		if (n_uniform) *n_uniform = t->t->uniform_step_blocks();
	});
}
int tcnn_trainer_dp_peer_abandon(tcnn_trainer* t) {
	return guard([&] { t->t->dp_peer_abandon(); });
}
int tcnn_trainer_dp_gather_state(tcnn_trainer* t, void* stream) {
	return guard([&] { t->t->dp_gather_state((hipStream_t)stream); });
}
float tcnn_trainer_loss(tcnn_trainer* t, void* stream) {
	float v = -1.0f;
	if (guard([&] { v = t->t->loss((hipStream_t)stream); }) != 0) return -1.0f;
	return v;
}
int tcnn_trainer_loss_value(tcnn_trainer* t, void* stream, float* out) {
	return guard([&] {
		TCNN_CHECK(out != nullptr, "loss: null result pointer");
		*out = t->t->loss((hipStream_t)stream);
	});
}
int tcnn_loss_evaluate(const char* otype, void* stream, uint32_t n, uint32_t stride, uint32_t dims, float loss_scale, const void* pred16,
                       const float* target, float* values, void* grads16, const float* pdf) {
	return guard([&] {
		TCNN_CHECK(otype != nullptr, "loss_evaluate: null otype");
		const int type = loss_type_from_otype(otype);
		TCNN_CHECK(type >= 0, std::string("Loss '") + otype + "' is not implemented by the MI355X engine (" + loss_otype_list() + ")");
		TCNN_CHECK(dims >= 1 && dims <= stride, "loss_evaluate: dims must be in [1, stride]");
		TCNN_CHECK(pred16 && target && grads16, "loss_evaluate: null predictions, targets or gradients");
		TCNN_CHECK((uint64_t)n * stride < (1ull << 32), "loss_evaluate: n * stride must be below 2^32");
		if (!n) return;
		// the per-workgroup sums are not part of this interface: scratch, freed after the kernel (hipFree waits)
		DevBuf part;
		part.reserve((size_t)relative_l2_n_blocks(n, stride) * sizeof(float));
		launch_relative_l2_partial((hipStream_t)stream, n, stride, dims, loss_scale, pred16, target, grads16, part.as<float>(), (uint32_t)type, pdf,
		                           values);
	});
}
int tcnn_loss_type(const char* otype) {
	int type = -1;
	guard([&] {
		TCNN_CHECK(otype != nullptr, "loss: null otype");
		type = loss_type_from_otype(otype);
		TCNN_CHECK(type >= 0, std::string("Loss '") + otype + "' is not implemented by the MI355X engine (" + loss_otype_list() + ")");
	});
	return type;
}
uint32_t tcnn_loss_workspace_floats(uint64_t n, uint32_t dims) { return loss_torch_n_partials(n, dims); }
int tcnn_loss_forward(int loss_type, void* stream, uint64_t n, uint32_t dims, const void* pred, int pred_f32, uint64_t row_stride,
                      const float* target, const float* pdf, float* workspace, uint32_t workspace_floats, float* value) {
	return guard([&] {
		launch_loss_torch_value((hipStream_t)stream, (uint32_t)loss_type, n, dims, pred, pred_f32 != 0, row_stride, target, pdf, workspace,
		                        workspace_floats, value);
	});
}
int tcnn_loss_backward(int loss_type, void* stream, uint64_t n, uint32_t dims, const void* pred, int pred_f32, uint64_t row_stride,
                       const float* target, const float* pdf, const float* grad_output, void* gradients) {
	return guard([&] {
		launch_loss_torch_grad((hipStream_t)stream, (uint32_t)loss_type, n, dims, pred, pred_f32 != 0, row_stride, target, pdf, grad_output,
		                       gradients);
	});
}
int tcnn_adam_step_buffers(void* stream, const tcnn_adam_options* o, uint64_t n, uint64_t n_matrix, uint32_t step, float* params,
                           const void* grad, int grad_f16, float* m1, float* m2, uint32_t* steps, const float* bias_factors,
                           uint32_t n_bias_factors) {
	return guard([&] {
		TCNN_CHECK(o != nullptr, "adam_step_buffers: null options");
		TCNN_CHECK(n < (1ull << 32), "adam_step_buffers: a parameter tensor must hold fewer than 2^32 elements");
		if (!n) return;
		TCNN_CHECK(params && grad && m1 && m2 && steps, "adam_step_buffers: null parameters, gradients or state");
		for (const void* p : {(const void*)params, grad, (const void*)m1, (const void*)m2, (const void*)steps})
			TCNN_CHECK((uintptr_t)p % 16 == 0, "adam_step_buffers: parameters, gradients and state must be aligned to 16 bytes");
		AdamArgs a{};
		a.n = (uint32_t)n;
		a.n_matrix = (uint32_t)std::min<uint64_t>(n_matrix, n);
		a.loss_scale = a.grad_scale = a.inv_loss_scale = 1.0f;  // unused: the gradient is taken as it is
		a.lr = o->learning_rate;
		a.beta1 = o->beta1;
		a.beta2 = o->beta2;
		a.eps = o->epsilon;
		a.l2_reg = o->l2_reg;
		a.rel_decay = o->relative_decay;
		a.abs_decay = o->absolute_decay;
		a.clip = o->clipping_magnitude;
		a.nonmat_lr_factor = o->non_matrix_learning_rate_factor;
		a.lower_lr_bound = 0.0f;
		a.upper_lr_bound = std::numeric_limits<float>::max();
		if (o->adabound) {  // adam.h:156-159, as TrainerHost::adam_args
			a.lower_lr_bound = 0.1f - 0.1f / ((1 - o->beta2) * (float)step + 1);
			a.upper_lr_bound = 0.1f + 0.1f / ((1 - o->beta2) * (float)step);
		}
		a.opt_matrix = o->optimize_matrix_params;
		a.opt_nonmatrix = o->optimize_non_matrix_params;
		a.factor_table = bias_factors;
		a.factor_n = bias_factors ? n_bias_factors : 0u;
		launch_adam_torch((hipStream_t)stream, a, params, grad, grad_f16 != 0, m1, m2, steps);
	});
}
int tcnn_adam_bias_factors(float beta1, float beta2, uint32_t first_step, uint32_t n, float* out) {
	return guard([&] {
		TCNN_CHECK(out != nullptr || n == 0, "adam_bias_factors: null result pointer");
		for (uint32_t k = 0; k < n; ++k) {  // as TrainerHost::adam_args_table
			const float t = (float)(first_step + k);
			out[k] = std::sqrt(1.0f - std::pow(beta2, t)) / (1.0f - std::pow(beta1, t));
		}
	});
}
const float* tcnn_trainer_loss_device(tcnn_trainer* t) { return t->t->d_loss.as<float>(); }
int tcnn_trainer_inference(tcnn_trainer* t, void* stream, uint32_t n, const float* in, float* out) {
	return guard([&] {
		if (n) t->t->inference((hipStream_t)stream, n, in, out);
	});
}
uint64_t tcnn_trainer_n_params(const tcnn_trainer* t) { return t->t->n_params; }
uint64_t tcnn_trainer_n_network_params(const tcnn_trainer* t) { return t->t->n_mlp; }
float* tcnn_trainer_params_fp32(tcnn_trainer* t) { return t->t->w32.as<float>(); }
void* tcnn_trainer_params(tcnn_trainer* t) { return t->t->w16.p; }
void* tcnn_trainer_params_inference(tcnn_trainer* t) { return t->t->params_inference(); }
int tcnn_trainer_optimizer_buffer(tcnn_trainer* t, const char* name, void** ptr, uint32_t* elem_bytes) {
	return guard([&] {
		TCNN_CHECK(name && ptr, "optimizer_buffer: null name or result pointer");
		*ptr = t->t->optimizer_buffer(name, elem_bytes);
	});
}
int tcnn_trainer_learning_rate(const tcnn_trainer* t, float* learning_rate) {
	return guard([&] {
		TCNN_CHECK(learning_rate != nullptr, "learning_rate: null result pointer");
		*learning_rate = t->t->learning_rate();
	});
}
const char* tcnn_trainer_optimizer_schedule(const tcnn_trainer* t) { return !t->t->opt ? "adam" : t->t->opt_inline ? "inline" : "staged"; }
int tcnn_trainer_set_learning_rate(tcnn_trainer* t, float learning_rate) {
	return guard([&] { t->t->set_learning_rate(learning_rate); });
}
// The raw gradient / step-count pointers may be cached by the caller: the first request makes the
// buffers current (on the stream of the last step) and the trainer keeps them so from then on
// (TrainerHost::lean_settle, LeanUse::Caller).
void* tcnn_trainer_param_gradients(tcnn_trainer* t) {
	if (guard([&] { t->t->lean_settle(TrainerHost::LeanUse::Caller); }) != 0) return nullptr;
	return t->t->g16.p;
}
float* tcnn_trainer_gradients_fp32(tcnn_trainer* t) {
	if (guard([&] { t->t->lean_settle(TrainerHost::LeanUse::Caller); }) != 0) return nullptr;
	return t->t->g32.as<float>();
}
int tcnn_trainer_optimizer_state(tcnn_trainer* t, float** m1, float** m2, uint32_t** steps) {
	if (int rc = guard([&] { t->t->lean_settle(TrainerHost::LeanUse::Caller); })) return rc;
	if (m1) *m1 = t->t->m1.as<float>();
	if (m2) *m2 = t->t->m2.as<float>();
	if (steps) *steps = t->t->steps.as<uint32_t>();
	return 0;
}
int tcnn_trainer_set_gradient_scale(tcnn_trainer* t, float s) {
	TrainerHost& h = *t->t;
	h.grad_scale_user = s;
	h.grad_scale = s / (float)h.dp_nranks();  // the RCCL communicator's or the peer exchange's N
	return 0;
}
int tcnn_trainer_set_loss_scale(tcnn_trainer* t, float loss_scale) {
	return guard([&] {
		TCNN_CHECK(loss_scale > 0.0f && std::isfinite(loss_scale), "set_loss_scale: the loss scale must be positive and finite");
		t->t->loss_scale = loss_scale;
	});
}
int tcnn_trainer_set_graph(tcnn_trainer* t, int on) {
	return guard([&] { t->t->set_graph(on != 0); });
}
int tcnn_trainer_graph_stats(const tcnn_trainer* t, uint64_t* captures, uint64_t* replays) {
	if (captures) *captures = t->t->graph_captures;
	if (replays) *replays = t->t->graph_replays;
	return 0;
}
int tcnn_trainer_serialize(tcnn_trainer* t, int with_optimizer, void* buf, uint64_t capacity, uint64_t* size) {
	return guard([&] {
		const std::vector<uint8_t> b = t->t->serialize(with_optimizer != 0);
		if (size) *size = b.size();
		if (buf) {
			TCNN_CHECK(capacity >= b.size(), "tcnn_trainer_serialize: buffer too small");
			std::memcpy(buf, b.data(), b.size());
		}
	});
}
int tcnn_trainer_serialize_json(tcnn_trainer* t, int with_optimizer, char* buf, uint64_t capacity, uint64_t* size) {
	return guard([&] {
		const std::string j = t->t->serialize_json(with_optimizer != 0);
		if (size) *size = j.size() + 1;
		if (buf) {
			TCNN_CHECK(capacity >= j.size() + 1, "tcnn_trainer_serialize_json: buffer too small");
			std::memcpy(buf, j.c_str(), j.size() + 1);
		}
	});
}
int tcnn_trainer_deserialize(tcnn_trainer* t, const void* buf, uint64_t size) {
	return guard([&] { t->t->deserialize(buf, (size_t)size); });
}
int tcnn_trainer_set_params_full_precision(tcnn_trainer* t, const float* host, uint64_t n) {
	return guard([&] { t->t->set_params_full_precision(host, n); });
}
uint32_t tcnn_trainer_optimizer_step_count(const tcnn_trainer* t) { return t->t->optimizer_step_count(); }
int tcnn_trainer_update_hyperparams(tcnn_trainer* t, const char* params_json) {
	return guard([&] {
		const json p = json::parse(params_json);
		if (p.count("optimizer")) t->t->update_optimizer_hyperparams(p["optimizer"]);  // Trainer::update_hyperparams, trainer.h:213-216
		// the reference forwards "loss" to Loss::update_hyperparams, which holds no hyperparameters
		// (relative_l2.h, l2.h): the loss type is fixed at construction there too -- say so instead of
		// ignoring a request to change it
		if (p.count("loss") && p["loss"].is_object() && p["loss"].count("otype")) {
			const std::string o = p["loss"]["otype"].get<std::string>();
			TCNN_CHECK(ieq(o, t->t->loss_otype), "update_hyperparams: the loss type is fixed at construction ('" + t->t->loss_otype +
			                                         "'), cannot change it to '" + o + "'");
		}
	});
}
const char* tcnn_trainer_hyperparams(tcnn_trainer* t) {
	g_str.clear();
	if (guard([&] {
		    json h = json::object();
		    h["optimizer"] = t->t->optimizer_hyperparams();
		    h["loss"] = json::object();
		    h["loss"]["otype"] = t->t->loss_otype;
		    g_str = h.dump();
	    }) != 0)
		return nullptr;
	return g_str.c_str();
}
int tcnn_trainer_initialize_params_rng(tcnn_trainer* t, uint64_t* state, uint64_t inc) {
	return guard([&] {
		TCNN_CHECK(state != nullptr, "initialize_params_rng: null state");
		Pcg32 rng;
		rng.state = *state;
		rng.inc = inc;
		t->t->initialize_params_rng(rng);
		*state = rng.state;
	});
}
int tcnn_trainer_initialize_params(tcnn_trainer* t, uint32_t seed) {
	return guard([&] { t->t->initialize_params(seed); });
}
const char* tcnn_trainer_engine(const tcnn_trainer* t) { return t->t->model->engine(); }
const char* tcnn_trainer_inference_engine(const tcnn_trainer* t) { return t->t->model->inference_engine(); }
const char* tcnn_module_engine(const tcnn_module* m) { return m->m->engine(); }
const char* tcnn_module_inference_engine(const tcnn_module* m) { return m->m->inference_engine(); }
const char* tcnn_module_backward_kernel(const tcnn_module* m, int with_dinput) { return m->m->backward_kernel(with_dinput != 0); }
int tcnn_trainer_set_max_level(tcnn_trainer* t, float max_level) {
	return guard([&] {
		TCNN_CHECK(t->t->model->grid != nullptr, "trainer model has no grid encoding");
		t->t->model->grid->max_level = max_level;
	});
}

int tcnn_trainer_profile_begin(tcnn_trainer* t) { return tcnn_trainer_profile_begin_sampled(t, 1); }
int tcnn_trainer_profile_begin_sampled(tcnn_trainer* t, uint32_t every) {
	return guard([&] {
		t->t->timer.reset();
		t->t->timer.every = every ? every : 1;
		t->t->timer.counter = 0;
		t->t->timer.enabled = true;
	});
}
int tcnn_trainer_profile_end(tcnn_trainer* t, double* ms, uint32_t n_phases, uint32_t* n_steps) {
	return guard([&] { t->t->profile_end(ms, n_phases, n_steps); });
}

int tcnn_debug_fused_phase_cycles(tcnn_trainer* t, void* stream, uint32_t n, const float* input, const float* target,
                                  uint64_t* host_cycles8) {
	return guard([&] {
		auto& tr = *t->t;
		auto& m = *tr.model;
		TCNN_CHECK(m.mlp.width == 64 && m.mlp.n_input == 32 && m.mlp.n_hidden_layers == 2 && m.grid->desc.n_pos_dims == 2,
		           "phase profile: config_hash shape only");
		hipStream_t st = (hipStream_t)stream;
		// run one normal step first so the workspace is sized
		tr.training_step(st, n, input, target, false);
		const uint32_t nb = fused_train_n_blocks(64, 32, 2, 2, tr.n_output_dims, false, n);
		const size_t WV = fused_train_waves();  // waves per workgroup of the fused kernel
		DevBuf prof;
		prof.reserve((size_t)nb * WV * 16 * 8);
		TCNN_HIP_CHECK(hipMemsetAsync(prof.p, 0, (size_t)nb * WV * 16 * 8, st));
		launch_fused_train_profile(st, n, tr.n_output_dims, tr.w16.p, (const uint8_t*)tr.w16.p + tr.n_mlp * 2, input, target,
		                           tr.ws.dLdenc.p, tr.ws.wgrad_partial.as<float>(), tr.ws.loss_partial.as<float>(),
		                           m.grid->dev_levels(), nb, tr.ws.wimage.p, prof.as<unsigned long long>());
		std::vector<unsigned long long> h((size_t)nb * WV * 16);
		TCNN_HIP_CHECK(hipMemcpyAsync(h.data(), prof.p, h.size() * 8, hipMemcpyDeviceToHost, st));
		TCNN_HIP_CHECK(hipStreamSynchronize(st));
		for (int k = 0; k < 16; ++k) {
			unsigned long long sum = 0;
			for (size_t w = 0; w < (size_t)nb * WV; ++w) sum += h[w * 16 + k];
			host_cycles8[k] = sum;
		}
	});
}

int tcnn_debug_grid_bwd_count_fallbacks(int on) {
	return guard([&] { grid_bwd_debug_count_fallbacks(on != 0); });
}
int tcnn_debug_grid_bwd_fallbacks(uint32_t* count) {
	return guard([&] { *count = grid_bwd_debug_fallbacks(); });
}
int tcnn_debug_step_dldenc(tcnn_trainer* t, void* host_dldenc, size_t dldenc_bytes, float* host_bound, size_t bound_bytes,
                           int* bound_live) {
	return guard([&] {
		auto& ws = t->t->ws;
		TCNN_HIP_CHECK(hipDeviceSynchronize());
		TCNN_CHECK(dldenc_bytes <= ws.dLdenc.bytes, "debug: dL/d(encoding) read past the workspace");
		TCNN_HIP_CHECK(hipMemcpy(host_dldenc, ws.dLdenc.p, dldenc_bytes, hipMemcpyDeviceToHost));
		*bound_live = ws.dy_bound_live ? 1 : 0;
		if (ws.dy_bound_live) {
			TCNN_CHECK(bound_bytes <= ws.dy_bound.bytes, "debug: slice sums read past the workspace");
			TCNN_HIP_CHECK(hipMemcpy(host_bound, ws.dy_bound.p, bound_bytes, hipMemcpyDeviceToHost));
		}
	});
}
int tcnn_debug_grid_backward_items(tcnn_trainer* t, void* stream, uint32_t n, const float* input, const void* dldy_pairs,
                                   const float* dy_bound, float* host_slabs, size_t slab_floats, uint32_t* n_chunks,
                                   uint32_t* slab_stride) {
	return guard([&] {
		auto& tr = *t->t;
		TCNN_CHECK(tr.model->grid != nullptr, "debug: trainer model has no grid encoding");
		TCNN_CHECK(n % 32 == 0, "debug: batch must be a multiple of 32");
		GridEncodingHost& g = *tr.model->grid;
		hipStream_t st = (hipStream_t)stream;
		GridBwdBufs w;
		g.backward_items(st, w, n, input, g.desc.n_pos_dims, dldy_pairs, 0, 0, nullptr, 0, dy_bound);
		TCNN_HIP_CHECK(hipStreamSynchronize(st));
		*n_chunks = w.n_chunks;
		*slab_stride = g.n_lds_params;
		const size_t nfl = (size_t)w.n_chunks * g.n_lds_params;
		TCNN_CHECK(nfl <= slab_floats, "debug: slab buffer too small");
		TCNN_HIP_CHECK(hipMemcpy(host_slabs, w.partial.p, nfl * 4, hipMemcpyDeviceToHost));
	});
}

int tcnn_debug_hfma(void* stream, const void* a, const void* b, const void* c, void* out, uint32_t n_pairs) {
	return guard([&] { launch_probe_hfma((hipStream_t)stream, a, b, c, out, n_pairs); });
}

int tcnn_debug_probe(void* stream, float* mfma_out, int16_t* tr_out) {
	return guard([&] { launch_probe((hipStream_t)stream, mfma_out, tr_out); });
}

}  // extern "C"

namespace tcnn_amd {
void log_msg(LogSeverity s, const std::string& msg) {
	std::lock_guard<std::mutex> lk(g_log_mutex);
	if (g_log_cb) g_log_cb((int)s, msg.c_str(), g_log_user);
}
}  // namespace tcnn_amd
