// tiny-cuda-nn/loss.h -- Loss<T> / create_loss<T> (reference include/tiny-cuda-nn/loss.h,
// src/loss.cu) for the MI355X engine. The loss is evaluated inside the engine's training step
// (fused into the MLP kernel); this object carries its configuration into the Trainer, and
// evaluate() runs the engine's stand-alone loss kernel on caller matrices.
// Implemented losses, the reference's nine (src/loss.cu:57-65, include/tiny-cuda-nn/losses/*.h): L2,
// RelativeL2, RelativeL2Luminance, L1, RelativeL1, Mape, Smape, CrossEntropy, Variance; any other
// otype throws. Predictions <= 0 are not clamped (CrossEntropy / Variance then give the reference's
// inf / NaN), and those two losses can be negative.
#pragma once

#include <algorithm>
#include <cctype>

#include "common.h"
#include "gpu_matrix.h"

namespace tcnn {

namespace detail {
inline bool equals_case_insensitive(const std::string& a, const std::string& b) {
	if (a.size() != b.size()) return false;
	for (size_t i = 0; i < a.size(); ++i)
		if (std::tolower((unsigned char)a[i]) != std::tolower((unsigned char)b[i])) return false;
	return true;
}
}  // namespace detail

template <typename T>
class Loss {
public:
	// (json members are initialised with parentheses: braces would wrap the value in an array)
	explicit Loss(json config) : m_config(std::move(config)) {}
	virtual ~Loss() {}
	void update_hyperparams(const json& params) {
		for (auto it = params.begin(); it != params.end(); ++it) m_config[it.key()] = it.value();
	}
	json hyperparams() const { return m_config; }
	const json& config() const { return m_config; }

	// loss.h of the reference: per-element loss values (already divided by the number of target elements)
	// and loss-scaled gradients of fp16 predictions [stride x n]; targets and data_pdf are [dims x n],
	// values and gradients [stride x n] with zeros in the padded rows. Returns once the work has finished.
	void evaluate(hipStream_t stream, const float loss_scale, const GPUMatrix<T>& prediction, const GPUMatrix<float>& target,
	              GPUMatrix<float>& values, GPUMatrix<T>& gradients, const GPUMatrix<float>* data_pdf = nullptr) const {
		if constexpr (sizeof(T) != 2) {
			throw std::runtime_error{"Loss::evaluate: fp32 predictions are not implemented by the MI355X engine"};
		} else {
			const uint32_t dims = target.m(), stride = prediction.m();
			CHECK_THROW(prediction.n() == target.n());
			CHECK_THROW(values.m() == stride && gradients.m() == stride);
			CHECK_THROW(values.n() == prediction.n() && gradients.n() == prediction.n());
			CHECK_THROW(prediction.is_contiguous() && target.is_contiguous() && values.is_contiguous() && gradients.is_contiguous());
			if (data_pdf) CHECK_THROW(data_pdf->m() == dims && data_pdf->n() == target.n() && data_pdf->is_contiguous());
			const std::string otype = m_config.value("otype", std::string{"RelativeL2"});
			detail::check_rc(tcnn_loss_evaluate(otype.c_str(), stream, prediction.n(), stride, dims, loss_scale, prediction.data(), target.data(),
			                                    values.data(), gradients.data(), data_pdf ? data_pdf->data() : nullptr));
		}
	}

private:
	json m_config;
};

// loss.cu: create_loss<T>(json) -- unknown otypes throw as the reference's factory does
template <typename T>
Loss<T>* create_loss(const json& loss) {
	const std::string otype = loss.value("otype", std::string{"RelativeL2"});
	static const char* const k_otypes[] = {"L2", "RelativeL2", "RelativeL2Luminance", "L1", "RelativeL1", "Mape", "Smape", "CrossEntropy", "Variance"};
	bool known = false;
	std::string list;
	for (const char* o : k_otypes) {
		known = known || detail::equals_case_insensitive(otype, o);
		list += (list.empty() ? "" : ", ") + std::string{o};
	}
	if (!known) throw std::runtime_error{"Loss: type '" + otype + "' is not implemented by the MI355X engine (" + list + ")"};
	json c = loss;
	c["otype"] = otype;
	return new Loss<T>(c);
}

}  // namespace tcnn
