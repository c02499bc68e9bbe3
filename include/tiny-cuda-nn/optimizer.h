// tiny-cuda-nn/optimizer.h -- Optimizer<T> / create_optimizer<T> (reference
// include/tiny-cuda-nn/optimizer.h, src/optimizer.cu) for the MI355X engine. The optimizers -- Adam
// (optimizers/adam.h), SGD, and the ExponentialDecay / Ema / Lookahead / Batched wrappers with their
// "nested" blocks -- run inside the engine's training step; this object carries the configuration into
// the Trainer and forwards later hyper-parameter and learning-rate changes to it.
#pragma once

#include "loss.h"

namespace tcnn {

namespace detail {
// src/optimizer.cu:49-80 as the engine implements it: the otypes it runs, and its refusals
inline bool optimizer_otype_has_nested(const std::string& otype) {
	for (const char* w : {"ExponentialDecay", "Ema", "Lookahead", "Batched"})
		if (equals_case_insensitive(otype, w)) return true;
	return false;
}
inline void validate_optimizer_config(const json& optimizer) {
	static const char* supported = " (supported: Adam, SGD, ExponentialDecay, Ema, Lookahead, Batched)";
	if (!optimizer.is_object()) throw std::runtime_error{"Optimizer: the configuration (and every 'nested' block) must be an object"};
	const std::string otype = optimizer.value("otype", std::string{"Adam"});
	if (equals_case_insensitive(otype, "Adam") || equals_case_insensitive(otype, "SGD")) return;
	if (optimizer_otype_has_nested(otype)) {
		validate_optimizer_config(optimizer.count("nested") ? optimizer["nested"] : json::object());
		return;
	}
	if (equals_case_insensitive(otype, "Shampoo"))
		throw std::runtime_error{std::string{"Cannot create `ShampooOptimizer` because tiny-cuda-nn was not compiled with cuBLAS and cuSolver."} +
		                         supported};
	for (const char* refused : {"Average", "Novograd", "Composite"})
		if (equals_case_insensitive(otype, refused))
			throw std::runtime_error{"Optimizer '" + std::string{refused} + "' is not implemented by the MI355X engine" + supported};
	throw std::runtime_error{"Invalid optimizer type: " + otype + supported};
}
// each level takes its own keys and passes "nested" down (Optimizer::update_hyperparams of the wrappers)
inline void merge_optimizer_config(json& config, const json& params) {
	for (auto it = params.begin(); it != params.end(); ++it) {
		if (it.key() == "nested" && it.value().is_object() && config.count("nested") && config["nested"].is_object())
			merge_optimizer_config(config["nested"], it.value());
		else
			config[it.key()] = it.value();
	}
}
// the innermost block (Adam or SGD), which holds the learning rate
inline json& innermost_optimizer_config(json& config) {
	json* c = &config;
	while (optimizer_otype_has_nested(c->value("otype", std::string{"Adam"}))) {
		if (!c->count("nested")) (*c)["nested"] = json::object();
		c = &(*c)["nested"];
	}
	return *c;
}
}  // namespace detail

template <typename T>
class Optimizer {
public:
	explicit Optimizer(json config) : m_config(std::move(config)) {}
	virtual ~Optimizer() {}

	// adam.h:235-283 / 200-210; the wrappers' update_hyperparams (e.g. ema.h:167-179)
	void update_hyperparams(const json& params) {
		detail::merge_optimizer_config(m_config, params);
		if (m_trainer) {
			json p = json::object();
			p["optimizer"] = params;
			detail::check_rc(tcnn_trainer_update_hyperparams(m_trainer, p.dump().c_str()));
		}
	}
	json hyperparams() const {
		if (m_trainer) return json::parse(tcnn_trainer_hyperparams(m_trainer))["optimizer"];
		return m_config;
	}
	// Optimizer::learning_rate(): the wrappers report their nested optimizer's, ExponentialDecay base x factor
	// (exponential_decay.h:73-75; the factor is 1 before the first step)
	float learning_rate() const {
		if (m_trainer) {
			float lr = 0.0f;
			detail::check_rc(tcnn_trainer_learning_rate(m_trainer, &lr));
			return lr;
		}
		json c = m_config;
		return detail::innermost_optimizer_config(c).value("learning_rate", 1e-3f);
	}
	// set_learning_rate(): an ExponentialDecay stores value / factor and hands the value down
	// (exponential_decay.h:77-80)
	void set_learning_rate(float lr) {
		detail::innermost_optimizer_config(m_config)["learning_rate"] = lr;
		if (m_trainer) detail::check_rc(tcnn_trainer_set_learning_rate(m_trainer, lr));
	}
	// Optimizer::step() of the outermost optimizer (Batched: its own counter)
	uint32_t step() const { return m_trainer ? tcnn_trainer_optimizer_step_count(m_trainer) : 0u; }
	// Optimizer::custom_weights(): the Ema / Lookahead weights inference reads, nullptr without any
	T* custom_weights() const {
		if (!m_trainer) return nullptr;
		void* p = tcnn_trainer_params_inference(m_trainer);
		return p == tcnn_trainer_params(m_trainer) ? nullptr : (T*)p;
	}
	const json& config() const { return m_config; }

	// set by the Trainer that runs this optimizer
	void attach(tcnn_trainer* t) { m_trainer = t; }

private:
	json m_config;
	tcnn_trainer* m_trainer = nullptr;
};

template <typename T>
Optimizer<T>* create_optimizer(const json& optimizer) {
	detail::validate_optimizer_config(optimizer);
	json c = optimizer;
	c["otype"] = optimizer.value("otype", std::string{"Adam"});
	return new Optimizer<T>(c);
}

}  // namespace tcnn
