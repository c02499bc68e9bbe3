// grid_dispatch.h -- run-time grid shape (input dims, features per level, hash type) to the template
// arguments of the grid kernels: each helper calls fn with the value as a std::integral_constant, so a
// launcher writes its launch once, inside a generic lambda, and names the kernel's arguments with
// decltype(tag)::value. Every grid launcher dispatches through these; the set of kernels a launcher
// instantiates is the product of the helpers it nests.
#pragma once

#include <type_traits>

#include "common.h"

namespace tcnn_amd {

template <typename Fn>
void with_grid_dims(uint32_t D, Fn&& fn) {
	switch (D) {
		case 2: return fn(std::integral_constant<uint32_t, 2>{});
		case 3: return fn(std::integral_constant<uint32_t, 3>{});
		case 4: return fn(std::integral_constant<uint32_t, 4>{});
		default: throw std::runtime_error("GridEncoding: number of input dims must be 2, 3 or 4");
	}
}

template <typename Fn>
void with_grid_features(uint32_t F, Fn&& fn) {
	switch (F) {
		case 1: return fn(std::integral_constant<uint32_t, 1>{});
		case 2: return fn(std::integral_constant<uint32_t, 2>{});
		case 4: return fn(std::integral_constant<uint32_t, 4>{});
		case 8: return fn(std::integral_constant<uint32_t, 8>{});
		default: throw std::runtime_error("GridEncoding: n_features_per_level must be 1, 2, 4 or 8");
	}
}

template <typename Fn>
void with_grid_hash(HashType h, Fn&& fn) {
	switch (h) {
		case HashType::Prime: return fn(std::integral_constant<HashType, HashType::Prime>{});
		case HashType::ReversedPrime: return fn(std::integral_constant<HashType, HashType::ReversedPrime>{});
		default: return fn(std::integral_constant<HashType, HashType::CoherentPrime>{});
	}
}

// fn(d, f, h): dims, then features, then hash (an unsupported D is reported before an unsupported F)
template <typename Fn>
void with_grid_shape(uint32_t D, uint32_t F, HashType h, Fn&& fn) {
	with_grid_dims(D, [&](auto d) { with_grid_features(F, [&](auto f) { with_grid_hash(h, [&](auto hh) { fn(d, f, hh); }); }); });
}

}  // namespace tcnn_amd
