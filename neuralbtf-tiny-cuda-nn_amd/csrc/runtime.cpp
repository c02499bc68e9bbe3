// runtime.cpp -- host runtime: JSON config surface, parameter init, trainer orchestration.
#include "runtime.h"
#include "loss_device.h"

#include <algorithm>
#include <cctype>
#include <cmath>
#include <cstring>
#include <limits>
#include <random>

namespace tcnn_amd {

// ------------------------------------------------------------------------------------------
// PCG32 (stream semantics of dependencies/pcg32/pcg32.h)
// ------------------------------------------------------------------------------------------
static constexpr uint64_t PCG32_MULT = 0x5851f42d4c957f2dULL;

void Pcg32::seed(uint64_t initstate, uint64_t initseq) {
	state = 0u;
	inc = (initseq << 1u) | 1u;
	next_uint();
	state += initstate;
	next_uint();
}

uint32_t Pcg32::next_uint() {
	uint64_t old = state;
	state = old * PCG32_MULT + inc;
	uint32_t xorshifted = (uint32_t)(((old >> 18u) ^ old) >> 27u);
	uint32_t rot = (uint32_t)(old >> 59u);
	return (xorshifted >> rot) | (xorshifted << ((~rot + 1u) & 31));
}

float Pcg32::next_float() {
	uint32_t u = (next_uint() >> 9) | 0x3f800000u;
	float f;
	std::memcpy(&f, &u, 4);
	return f - 1.0f;
}

void Pcg32::advance(int64_t delta_) {
	uint64_t cur_mult = PCG32_MULT, cur_plus = inc, acc_mult = 1u, acc_plus = 0u;
	uint64_t delta = (uint64_t)delta_;
	while (delta > 0) {
		if (delta & 1) {
			acc_mult *= cur_mult;
			acc_plus = acc_plus * cur_mult + cur_plus;
		}
		cur_plus = (cur_mult + 1) * cur_plus;
		cur_mult *= cur_mult;
		delta /= 2;
	}
	state = acc_mult * state + acc_plus;
}

// generate_random_uniform's strided order (reference random.h:39-70), evaluated on the host.
static void strided_uniform(Pcg32& rng, size_t n, float* out, float lo, float hi) {
	const size_t n_gen = 4;
	const size_t n_thr = (n + n_gen - 1) / n_gen;
	const size_t n_threads = (n_thr + 127) / 128 * 128;
	const float range = hi - lo;
	for (size_t i = 0; i < n_threads; ++i) {  // all launched threads write, also those past n_thr (random.h:41-54)
		Pcg32 r = rng;
		r.advance((int64_t)(i * n_gen));
		for (size_t j = 0; j < n_gen; ++j) {
			size_t idx = i + n_threads * j;
			if (idx >= n) break;
			out[idx] = std::fma(r.next_float(), range, lo);
		}
	}
	rng.advance((int64_t)n);
}

// ------------------------------------------------------------------------------------------
// DevBuf
// ------------------------------------------------------------------------------------------
DevBuf::~DevBuf() { release(); }

void DevBuf::release() {
	if (p) (void)hipFree(p);
	p = nullptr;
	bytes = 0;
}

void DevBuf::reserve(size_t n) {
	if (n <= bytes && p) return;
	release();
	if (n == 0) n = 16;
	TCNN_HIP_CHECK(hipMalloc(&p, n));
	bytes = n;
	static const bool poison = std::getenv("TCNN_DEBUG_POISON") != nullptr;  // NaN-fill new buffers (finds reads of unwritten memory)
	if (poison) TCNN_HIP_CHECK(hipMemset(p, 0xff, n));
}

EngineSwitches EngineSwitches::from_env() {
	EngineSwitches s;
	auto on = [](const char* n) { return std::getenv(n) != nullptr; };
	s.no_fused_grid = on("TCNN_NO_FUSED_GRID");
	s.no_tile_engine = on("TCNN_NO_TILE_ENGINE");
	s.no_inrange_index = on("TCNN_NO_INRANGE_INDEX");
	s.no_forward_keep = on("TCNN_NO_FORWARD_KEEP");
	s.split_forward = on("TCNN_SPLIT_FORWARD");
	const char* bin = std::getenv("TCNN_GRID_BIN");
	s.grid_bin_all = bin && std::string(bin) == "all";
	if (const char* e = std::getenv("TCNN_GRID_BWD_CHUNKS"))
		if (std::atoi(e) > 0) s.grid_bwd_chunks = (uint32_t)std::atoi(e);
	if (const char* e = std::getenv("TCNN_GRID_BWD_RANGES"))
		if (std::atoi(e) > 0) s.grid_bwd_ranges = (uint32_t)std::atoi(e);
	if (const char* e = std::getenv("TCNN_GRID_BWD_STREAM")) s.no_grid_bwd_stream = std::string(e) == "0";
	if (const char* e = std::getenv("TCNN_WT_STORES")) s.wt_stores = (uint32_t)std::strtoul(e, nullptr, 0) & WT_STORES_ALL;
	if (const char* e = std::getenv("TCNN_ADAM_LEAN")) s.adam_lean = (uint32_t)std::strtoul(e, nullptr, 0) & ADAM_LEAN_ALL;
	if (const char* e = std::getenv("TCNN_GRID_BWD_PLAN")) s.grid_bwd_plan = std::string(e) == "feature" ? 1 : (std::string(e) == "range" ? 0 : -1);
	return s;
}

bool ieq(const std::string& a, const std::string& b) {
	if (a.size() != b.size()) return false;
	for (size_t i = 0; i < a.size(); ++i)
		if (std::tolower((unsigned char)a[i]) != std::tolower((unsigned char)b[i])) return false;
	return true;
}

// the reference's loss factory (src/loss.cu:57-65)
static const struct { const char* name; uint32_t type; } k_loss_otypes[] = {
	{"L2", LOSS_L2},
	{"RelativeL2", LOSS_RELATIVE_L2},
	{"RelativeL2Luminance", LOSS_RELATIVE_L2_LUMINANCE},
	{"L1", LOSS_L1},
	{"RelativeL1", LOSS_RELATIVE_L1},
	{"Mape", LOSS_MAPE},
	{"Smape", LOSS_SMAPE},
	{"CrossEntropy", LOSS_CROSS_ENTROPY},
	{"Variance", LOSS_VARIANCE},
};
int loss_type_from_otype(const std::string& otype) {
	for (const auto& e : k_loss_otypes)
		if (ieq(otype, e.name)) return (int)e.type;
	return -1;
}
std::string loss_otype_list() {
	std::string r;
	for (const auto& e : k_loss_otypes) r += (r.empty() ? "" : ", ") + std::string(e.name);
	return r;
}

template <typename T>
static T jval(const json& j, const char* key, T dflt) {
	auto it = j.find(key);
	if (it == j.end() || it->is_null()) return dflt;
	return it->get<T>();
}

static bool jhas(const json& j, const char* key) { return j.is_object() && j.find(key) != j.end(); }

// ------------------------------------------------------------------------------------------
// Grid encoding (reference grid.h:652-1208)
// ------------------------------------------------------------------------------------------
static uint32_t powi_u32(uint32_t base, uint32_t exp) {
	uint32_t r = 1;
	for (uint32_t i = 0; i < exp; ++i) r *= base;
	return r;
}

// The items of a backward plan must tile [0, size) x [0, F) of each of its levels exactly. An entry in no
// item is never written by k_grid_bwd_lds, and whatever its slab element held is summed into the
// gradient. The kernel's IDX_HASH_RANGE index and write_slab's one contiguous run per item assume one
// of two splits per level: entry ranges holding all F features, or feature groups holding every entry.
// Either must run 0 -> size (or 0 -> F) without gap or overlap.
static void check_items_tile_levels(const std::vector<GridSlice>& items, const std::vector<LevelInfo>& levels, uint32_t n_levels, uint32_t F) {
	std::vector<std::vector<std::pair<uint32_t, uint32_t>>> runs(n_levels);  // [lo, hi) along the level's split axis
	std::vector<int> by_feature(n_levels, -1);
	for (const GridSlice& s : items) {
		TCNN_CHECK(s.level < n_levels && s.begin < s.end && s.end <= levels[s.level].size && s.nf >= 1 && s.f0 + s.nf <= F,
		           "GridEncoding: backward item outside its level");
		const bool all_features = s.f0 == 0 && s.nf == F;
		TCNN_CHECK(all_features || (s.begin == 0 && s.end == levels[s.level].size), "GridEncoding: backward item splits entries and features");
		TCNN_CHECK(by_feature[s.level] < 0 || by_feature[s.level] == (all_features ? 0 : 1), "GridEncoding: level split two ways");
		by_feature[s.level] = all_features ? 0 : 1;
		runs[s.level].push_back(all_features ? std::make_pair(s.begin, s.end) : std::make_pair(s.f0, s.f0 + s.nf));
	}
	for (uint32_t l = 0; l < n_levels; ++l) {
		std::sort(runs[l].begin(), runs[l].end());
		uint32_t at = 0;
		for (const auto& r : runs[l]) {
			TCNN_CHECK(r.first == at, "GridEncoding: backward items of level " + std::to_string(l) + " leave a gap or overlap at " + std::to_string(at));
			at = r.second;
		}
		TCNN_CHECK(at == (by_feature[l] == 1 ? F : levels[l].size), "GridEncoding: backward items do not cover level " + std::to_string(l));
	}
}

GridEncodingHost::GridEncodingHost(uint32_t n_dims, const json& enc) {
	const std::string otype = jval<std::string>(enc, "otype", "Grid");
	const std::string default_type = ieq(otype, "TiledGrid") ? "Tiled" : (ieq(otype, "DenseGrid") ? "Dense" : "Hash");
	const uint32_t F = jval<uint32_t>(enc, "n_features_per_level", 2u);
	TCNN_CHECK(F == 1 || F == 2 || F == 4 || F == 8, "GridEncoding: n_features_per_level must be 1, 2, 4, or 8.");
	uint32_t n_feat;
	if (jhas(enc, "n_features") || jhas(enc, "n_grid_features")) {
		n_feat = jhas(enc, "n_features") ? enc["n_features"].get<uint32_t>() : enc["n_grid_features"].get<uint32_t>();
		TCNN_CHECK(!jhas(enc, "n_levels"), "GridEncoding: may not specify n_features and n_levels simultaneously (one determines the other)");
	} else {
		n_feat = F * jval<uint32_t>(enc, "n_levels", 16u);
	}
	TCNN_CHECK(n_feat % F == 0, "GridEncoding: n_features must be a multiple of n_features_per_level");
	const uint32_t L = n_feat / F;
	TCNN_CHECK(L >= 1 && L <= MAX_LEVELS, "GridEncoding: too many levels");
	const std::string type = jval<std::string>(enc, "type", default_type);
	GridType gt;
	if (ieq(type, "Hash")) gt = GridType::Hash;
	else if (ieq(type, "Dense")) gt = GridType::Dense;
	else if (ieq(type, "Tiled")) gt = GridType::Tiled;
	else throw std::runtime_error("GridEncoding: invalid grid type " + type);
	const uint32_t base = jval<uint32_t>(enc, "base_resolution", 16u);
	const float default_scale = gt == GridType::Dense ? std::exp(std::log(256.0f / (float)base) / (float)(L - 1)) : 2.0f;
	const std::string interp = jval<std::string>(enc, "interpolation", "Linear");
	const std::string hash = jval<std::string>(enc, "hash", "CoherentPrime");
	TCNN_CHECK(n_dims >= 2 && n_dims <= 4, "GridEncoding: number of input dims must be 2, 3 or 4.");

	desc.n_pos_dims = n_dims;
	desc.n_features_per_level = F;
	desc.n_levels = L;
	desc.log2_hashmap_size = jval<uint32_t>(enc, "log2_hashmap_size", 19u);
	desc.base_resolution = base;
	desc.per_level_scale = jval<float>(enc, "per_level_scale", default_scale);
	desc.grid_type = gt;
	if (ieq(hash, "Prime")) desc.hash_type = HashType::Prime;
	else if (ieq(hash, "CoherentPrime")) desc.hash_type = HashType::CoherentPrime;
	else if (ieq(hash, "ReversedPrime")) desc.hash_type = HashType::ReversedPrime;
	else throw std::runtime_error("GridEncoding: unsupported hash type " + hash);
	if (ieq(interp, "Nearest")) desc.interp = Interp::Nearest;
	else if (ieq(interp, "Linear")) desc.interp = Interp::Linear;
	else if (ieq(interp, "Smoothstep")) desc.interp = Interp::Smoothstep;
	else throw std::runtime_error("GridEncoding: invalid interpolation " + interp);
	stochastic = jval<bool>(enc, "stochastic_interpolation", false);
	n_features = n_feat;

	// offset table, grid.h:688-719 (host log2/exp2 in float, as the reference's host code)
	const float log2_scale = std::log2(desc.per_level_scale);
	uint32_t offset = 0;
	levels.resize(L);
	for (uint32_t l = 0; l < L; ++l) {
		const float scale = exp2f((float)l * log2_scale) * (float)base - 1.0f;
		const uint32_t res = (uint32_t)ceilf(scale) + 1;
		const uint32_t max_params = std::numeric_limits<uint32_t>::max() / 2;
		uint32_t params = std::pow((float)res, (float)n_dims) > (float)max_params ? max_params : powi_u32(res, n_dims);
		params = (params + 7u) / 8u * 8u;
		if (gt == GridType::Tiled) params = std::min(params, powi_u32(base, n_dims));
		else if (gt == GridType::Hash) params = std::min(params, 1u << desc.log2_hashmap_size);
		levels[l] = LevelInfo{scale, res, offset, params};
		log_debug("GridEncoding at level " + std::to_string(l) + ": resolution=" + std::to_string(res) +
		          " params_in_level=" + std::to_string(params));  // grid.h:717
		offset += params;
	}
	n_params = offset * F;

	// Backward plan. A level whose F features fit the LDS budget is one LDS item; else, when one
	// feature fits, one item per feature group (config_hash's 2^15-entry hashed levels: two items);
	// levels with even one feature over the budget -- and every level after them, so the binned
	// levels are a suffix of the parameter vector -- go through the binned backward (grid_bin.hip).
	// TCNN_GRID_BIN=all bins every level that does not fit whole (tuning switch).
	const uint32_t S = grid_bwd_slot_budget();
	const bool bin_all = sw.grid_bin_all;
	first_binned = L;
	for (uint32_t l = 0; l < L; ++l) {
		const uint64_t need = bin_all ? (uint64_t)levels[l].size * F : (uint64_t)levels[l].size;
		if (need > S) { first_binned = l; break; }
	}
	n_lds_params = (first_binned < L ? levels[first_binned].offset : offset) * F;
	// Two work plans for the LDS levels (r06), chosen per launch (plan_for). Both: a level whose F
	// features fit the budget is one item; the others split --
	//   PLAN_RANGE:   a hashed power-of-two level into entry ranges holding all F features: the chunk
	//                 slabs are in parameter order (Adam and the slab sums read them without the map),
	//                 the packed-pair LDS adds of MODE 0 apply for F = 2;
	//   PLAN_FEATURE: into feature groups (r05): each writes a feature-group-major run, read back
	//                 through GridSlabMap.
	// Measured (profiles/r06_grid_plan_ab.json): the range plan takes 2^15 / 2^18-point steps 2 us /
	// 1.4 % faster (Adam 15.0 -> 13.0 us at 2^18), the feature plan is 25 % faster in configs[3]'s
	// 2^20-point backward, whose chunks run in several rounds.
	GridSlabMap map{};
	map.n_levels = std::max(1u, first_binned);
	while ((1u << map.log2F) < F) ++map.log2F;
	for (int plan = 0; plan < 2; ++plan) {
		std::vector<GridSlice>& out = plans[plan].slices;
		std::vector<GridSlice> single;
		for (uint32_t l = 0; l < first_binned; ++l) {
			const uint32_t size = levels[l].size;
			map.pbase[l] = levels[l].offset * F;
			map.size[l] = size;
			if (plan == PLAN_FEATURE) map.nf[l] = F;
			if ((uint64_t)size * F <= S) {
				out.push_back(GridSlice{l, 0, size, 0, F});
				continue;
			}
			uint32_t full = 1;
			for (uint32_t d = 0; d < desc.n_pos_dims && full <= size; ++d) full *= levels[l].res;
			const bool hashed_pow2 = gt == GridType::Hash && (size & (size - 1)) == 0 && full > size;
			if (plan == PLAN_RANGE && hashed_pow2) {
				uint32_t R = 1;
				while ((uint64_t)size * F / R > S) R *= 2;
				// tuning override (TCNN_GRID_BWD_RANGES), rounded up to a power of two: R must divide the
				// (power-of-two) size, or the entries [R * len, size) would be in no item
				// (clamped to size / 256 first, itself a power of two: the doubling cannot wrap)
				const uint32_t most = size / 256;
				uint32_t want = 1;
				while (want < std::min(sw.grid_bwd_ranges, most)) want *= 2;
				R = std::max(R, want);
				const uint32_t len = size / R;
				for (uint32_t r = 0; r < R; ++r) single.push_back(GridSlice{l, r * len, (r + 1) * len, 0, F});
				continue;
			}
			uint32_t nf = F;
			while (nf > 1 && ((uint64_t)size * nf > S || F % nf)) --nf;
			if (plan == PLAN_FEATURE) map.nf[l] = nf;
			else plans[plan].identity = false;  // a non-hashed level split by features: the range plan needs the map too
			for (uint32_t f = 0; f < F; f += nf) single.push_back(GridSlice{l, 0, size, f, nf});
		}
		out.insert(out.end(), single.begin(), single.end());
	}
	plans[PLAN_FEATURE].identity = true;
	for (uint32_t l = 0; l < first_binned; ++l) plans[PLAN_FEATURE].identity = plans[PLAN_FEATURE].identity && map.nf[l] == F;
	if (!plans[PLAN_RANGE].identity) plans[PLAN_RANGE] = plans[PLAN_FEATURE];  // (no hashed split: one plan)
	for (const GridPlan& pl : plans) check_items_tile_levels(pl.slices, levels, first_binned, F);
	map.pbase[first_binned] = n_lds_params;
	d_slab_map.reserve(sizeof(GridSlabMap));
	TCNN_HIP_CHECK(hipMemcpy(d_slab_map.p, &map, sizeof(GridSlabMap), hipMemcpyHostToDevice));

	// binned levels: slices of 2^s entries, ~128 per level (one workgroup each in the accumulate
	// pass), within the accumulator budget and GRID_BIN_MAX_SLICES
	const uint32_t max_entries = GRID_ACC_LDS_BYTES / 4 / F;
	for (uint32_t l = first_binned; l < L; ++l) {
		const uint32_t size = levels[l].size;
		uint32_t lg = 0;
		while ((1ull << lg) < size) ++lg;
		uint32_t s = lg > 7 ? lg - 7 : 0;
		s = std::max(s, 9u);
		while ((1u << s) > max_entries) --s;
		TCNN_CHECK(div_round_up(size, 1u << s) <= GRID_BIN_MAX_SLICES,
		           "GridEncoding: level of " + std::to_string(size) + " entries exceeds the binned backward's capacity");
		GridBinLevel b{l, s, div_round_up(size, 1u << s), n_buckets};
		n_buckets += b.n_slices;
		acc_lds_bytes = std::max(acc_lds_bytes, (1u << s) * F * 4);
		bin_levels.push_back(b);
	}
	if (!bin_levels.empty()) {
		d_bin_levels.reserve(bin_levels.size() * sizeof(GridBinLevel));
		TCNN_HIP_CHECK(hipMemcpy(d_bin_levels.p, bin_levels.data(), bin_levels.size() * sizeof(GridBinLevel), hipMemcpyHostToDevice));
	}

	// grid_index_inrange (grid_device.h: the reference stride loop, then a mask or ONE conditional
	// subtraction) is exact for positions in [0, 1] on every level iff hashed levels have
	// power-of-two sizes and the others hold res^D entries (their index is then < 2 size)
	inrange_index_ok = true;
	for (const LevelInfo& li : levels) {
		uint32_t stride = 1;
		for (uint32_t d = 0; d < desc.n_pos_dims; ++d)
			if (stride <= li.size) stride *= li.res;
		uint64_t full = 1;
		for (uint32_t d = 0; d < desc.n_pos_dims; ++d) full = std::min<uint64_t>(full * li.res, 1ull << 40);
		const bool hashed = hash_grid() && li.size < stride;
		if (hashed ? (li.size & (li.size - 1)) != 0 : full > li.size) inrange_index_ok = false;
		if (li.res < 2) inrange_index_ok = false;
	}
	d_levels.reserve(levels.size() * sizeof(LevelInfo));
	TCNN_HIP_CHECK(hipMemcpy(d_levels.p, levels.data(), levels.size() * sizeof(LevelInfo), hipMemcpyHostToDevice));
	for (GridPlan& pl : plans) {
		pl.d_slices.reserve(pl.slices.size() * sizeof(GridSlice));
		TCNN_HIP_CHECK(hipMemcpy(pl.d_slices.p, pl.slices.data(), pl.slices.size() * sizeof(GridSlice), hipMemcpyHostToDevice));
	}
}

void GridEncodingHost::initialize_params(Pcg32& rng, float* out, float scale) const {
	strided_uniform(rng, n_params, out, -1e-4f * scale, 1e-4f * scale);
}

GridBinArgs GridEncodingHost::bin_args(GridBwdBufs& w, uint32_t B) const {
	GridBinArgs a{};
	a.lv = d_bin_levels.as<GridBinLevel>();
	a.n_slots = (uint32_t)bin_levels.size();
	a.n_buckets = n_buckets;
	a.pts_per_chunk = GRID_BIN_RECS >> desc.n_pos_dims;
	a.n_chunks = div_round_up(std::max(B, 1u), a.pts_per_chunk);
	a.acc_lds_bytes = acc_lds_bytes;
	if (a.n_slots) {
		w.recs.reserve((size_t)a.n_slots * a.n_chunks * GRID_BIN_RECS * sizeof(uint2));
		w.dir.reserve((size_t)a.n_buckets * a.n_chunks * sizeof(uint2));
		w.dysum.reserve((size_t)a.n_slots * a.n_chunks * desc.n_features_per_level * sizeof(float));
	}
	a.recs = w.recs.as<uint2>();
	a.dir = w.dir.as<uint2>();
	a.dysum = w.dysum.as<float>();
	return a;
}

void GridEncodingHost::backward_items(hipStream_t st, GridBwdBufs& w, uint32_t B, const float* pos, uint32_t pstride, const void* dy,
                                      int layout, uint32_t dy_stride, const GridBwdEpilogue* ep, uint32_t reserved, const float* dy_bound) const {
	const uint32_t n_chunks = bwd_chunks(B, reserved);
	w.n_chunks = n_chunks;
	w.plan = plan_for(B, reserved);
	const GridPlan& pl = plans[w.plan];
	if (!pl.slices.empty()) w.partial.reserve((size_t)n_chunks * n_lds_params * 4);
	launch_grid_bwd(st, call(), B, pos, pstride, dy, layout, dy_stride, pl.d_slices.as<GridSlice>(), (uint32_t)pl.slices.size(), n_chunks,
	                w.partial.as<float>(), n_lds_params, ep, pl.slices.data(), levels.data(), dy_bound, sw.wt_stores);
}

void GridEncodingHost::backward_bin(hipStream_t st, GridBwdBufs& w, uint32_t B, const float* pos, uint32_t pstride, const void* dy,
                                    int layout, uint32_t dy_stride) const {
	if (bin_levels.empty() || B == 0) return;
	const GridBinArgs a = bin_args(w, B);
	launch_grid_bin(st, call(), B, pos, pstride, dy, layout, dy_stride, a);
}

void GridEncodingHost::backward_acc(hipStream_t st, GridBwdBufs& w, uint32_t B, const void* dy, int layout, uint32_t dy_stride,
                                    float* grad32, const GridAccAdam* adam) const {
	if (bin_levels.empty()) return;
	if (B == 0) {  // no points: zero gradient (Overwrite)
		if (!adam) TCNN_HIP_CHECK(hipMemsetAsync(grad32 + n_lds_params, 0, (size_t)(n_params - n_lds_params) * 4, st));
		return;
	}
	const GridBinArgs a = bin_args(w, B);
	launch_grid_acc(st, call(), B, dy, layout, dy_stride, a, grad32, adam);
}

void GridEncodingHost::reduce_items(hipStream_t st, GridBwdBufs& w, float* grad32, GradFinalize fin) const {
	if (plans[0].slices.empty()) return;
	launch_grid_slab_reduce(st, w.partial.as<float>(), w.n_chunks, n_lds_params, n_lds_params, grad32, slab_map(w.plan), fin);
}

void GridEncodingHost::backward(hipStream_t st, GridBwdBufs& w, uint32_t B, const float* pos, uint32_t pstride, const void* dy,
                                int layout, uint32_t dy_stride, float* grad32) const {
	backward_items(st, w, B, pos, pstride, dy, layout, dy_stride);
	backward_bin(st, w, B, pos, pstride, dy, layout, dy_stride);
	backward_acc(st, w, B, dy, layout, dy_stride, grad32);
	reduce_items(st, w, grad32);
}

// fp32 modules: every level as LDS items with all F features. A level whose F features fit the LDS
// budget is one item; a larger hashed power-of-two level splits into power-of-two entry ranges
// (IDX_HASH_RANGE), any other large level (dense, tiled) into ranges of S / F entries (the generic index,
// corners outside the range skipped). Every item of a split level walks all of the chunk's points.
void GridEncodingHost::build_plan_f32() {
	if (!plan_f32.slices.empty()) return;
	const uint32_t S = grid_bwd_slot_budget(), F = desc.n_features_per_level;
	std::vector<GridSlice>& out = plan_f32.slices;
	for (uint32_t l = 0; l < desc.n_levels; ++l) {
		const uint32_t size = levels[l].size;
		if ((uint64_t)size * F <= S) {
			out.push_back(GridSlice{l, 0, size, 0, F});
			continue;
		}
		uint32_t len = S / F;  // entries of one range (S and F are powers of two)
		if ((size & (size - 1)) == 0) len = std::min(len, size);
		for (uint32_t b = 0; b < size; b += len) out.push_back(GridSlice{l, b, std::min(size, b + len), 0, F});
	}
	for (const GridSlice& s : out) TCNN_CHECK((uint64_t)(s.end - s.begin) * F <= S, "GridEncoding: fp32 backward item exceeds the LDS");
	check_items_tile_levels(out, levels, desc.n_levels, F);
	plan_f32.identity = true;
	plan_f32.d_slices.reserve(out.size() * sizeof(GridSlice));
	TCNN_HIP_CHECK(hipMemcpy(plan_f32.d_slices.p, out.data(), out.size() * sizeof(GridSlice), hipMemcpyHostToDevice));
}

void GridEncodingHost::backward_f32(hipStream_t st, GridBwdBufs& w, uint32_t B, const float* pos, uint32_t pstride, const float* dy32,
                                    uint32_t dy_stride, float* grad32) const {
	TCNN_CHECK(!plan_f32.slices.empty(), "GridEncoding: the fp32 backward plan was not built");
	if (B == 0) {  // no points: zero gradient (Overwrite)
		TCNN_HIP_CHECK(hipMemsetAsync(grad32, 0, (size_t)n_params * 4, st));
		return;
	}
	const uint32_t n_chunks = bwd_chunks_f32(B);
	// one chunk: its slab is the gradient (every parameter belongs to exactly one item, which writes it)
	float* partial = grad32;
	if (n_chunks > 1) {
		w.partial.reserve((size_t)n_chunks * n_params * 4);
		partial = w.partial.as<float>();
	}
	launch_grid_bwd_f32(st, call(), B, pos, pstride, dy32, dy_stride, plan_f32.d_slices.as<GridSlice>(), (uint32_t)plan_f32.slices.size(),
	                    n_chunks, partial, n_params);
	if (n_chunks > 1) launch_grid_slab_reduce(st, partial, n_chunks, n_params, n_params, grad32, nullptr);
}

static const char* grid_type_str(GridType t) { return t == GridType::Hash ? "Hash" : t == GridType::Dense ? "Dense" : "Tiled"; }
static const char* hash_str(HashType t) { return t == HashType::Prime ? "Prime" : t == HashType::ReversedPrime ? "ReversedPrime" : "CoherentPrime"; }
static const char* interp_str(Interp t) { return t == Interp::Nearest ? "Nearest" : t == Interp::Smoothstep ? "Smoothstep" : "Linear"; }

json GridEncodingHost::hyperparams() const {  // grid.h:1096-1114
	json r = {
		{"otype", "Grid"}, {"type", grid_type_str(desc.grid_type)}, {"n_levels", desc.n_levels},
		{"n_features_per_level", desc.n_features_per_level}, {"base_resolution", desc.base_resolution},
		{"per_level_scale", desc.per_level_scale}, {"interpolation", interp_str(desc.interp)}, {"hash", hash_str(desc.hash_type)},
	};
	if (desc.grid_type == GridType::Hash) r["log2_hashmap_size"] = desc.log2_hashmap_size;
	return r;
}

// ------------------------------------------------------------------------------------------
// MLP (reference src/network.cu:48-138, fully_fused_mlp.cu:635-678, 865-891)
// ------------------------------------------------------------------------------------------
static const char* const ACT_NAMES[] = {"None", "ReLU", "LeakyReLU", "Exponential", "Sine", "Sigmoid", "Squareplus", "Softplus", "Tanh"};

static int parse_activation(const std::string& s) {  // string_to_activation (common.cu)
	for (int a = 0; a <= ACT_TANH; ++a)
		if (ieq(s, ACT_NAMES[a])) return a;
	throw std::runtime_error("Invalid activation name: " + s);
}

MlpHost::MlpHost(uint32_t n_input_dims, uint32_t n_output_dims, const json& net) {
	otype = jval<std::string>(net, "otype", "MLP");
	TCNN_CHECK(ieq(otype, "FullyFusedMLP") || ieq(otype, "MegakernelMLP") || ieq(otype, "MLP") || ieq(otype, "CutlassMLP"),
	           "Invalid network type: " + otype);
	width = jval<uint32_t>(net, "n_neurons", 128u);
	n_hidden_layers = jval<uint32_t>(net, "n_hidden_layers", 5u);
	if (ieq(otype, "FullyFusedMLP") || ieq(otype, "MegakernelMLP")) {
		TCNN_CHECK(n_hidden_layers >= 1, "FullyFusedMLP requires at least 1 hidden layer (3 layers in total).");
		TCNN_CHECK(width == 16 || width == 32 || width == 64 || width == 128,
		           "FullyFusedMLP only supports 16, 32, 64, and 128 neurons, but got " + std::to_string(width) + ". Use CutlassMLP instead if this is a requirement.");
	}
	// CutlassMLP (cutlass_mlp.cu:41-81): any width; 0 hidden layers = one [padded_output][input] matrix
	activation = parse_activation(jval<std::string>(net, "activation", "ReLU"));
	output_activation = parse_activation(jval<std::string>(net, "output_activation", "None"));
	n_input = n_input_dims;
	n_output = n_output_dims;
	padded_output = (n_output + 15) / 16 * 16;  // REQUIRED_ALIGNMENT 16 (fully_fused_mlp.h:108-110)
}

static void xavier(Pcg32& rnd, uint32_t rows, uint32_t cols, float* out, float scale) {
	scale *= std::sqrt(6.0f / (float)(cols + rows));
	const size_t n = (size_t)rows * cols;
	for (size_t i = 0; i < n; ++i) {
		float t = rnd.next_float() * 2.0f;
		t = t * scale;
		out[i] = t - scale;
	}
}

void MlpHost::initialize_params(Pcg32& rng, float* out, float scale) const {
	if (n_hidden_layers == 0) {  // one matrix (cutlass_mlp.cu:64-67)
		xavier(rng, padded_output, n_input, out, scale);
		return;
	}
	xavier(rng, width, n_input, out, scale);
	out += (size_t)width * n_input;
	for (uint32_t i = 1; i < n_hidden_layers; ++i) {
		xavier(rng, width, width, out, scale);
		out += (size_t)width * width;
	}
	xavier(rng, padded_output, width, out, scale);
}

static const char* act_str(int a) { return a >= 0 && a <= ACT_TANH ? ACT_NAMES[a] : "None"; }

json MlpHost::hyperparams() const {
	return {{"otype", ieq(otype, "CutlassMLP") || ieq(otype, "MLP") ? "CutlassMLP" : "FullyFusedMLP"},
	        {"n_neurons", width}, {"n_hidden_layers", n_hidden_layers},
	        {"activation", act_str(activation)}, {"output_activation", act_str(output_activation)}};
}

void AdamHost::update(const json& p) {  // adam.h:235-283
	if (jhas(p, "beta1")) beta1 = p["beta1"].get<float>();
	if (jhas(p, "beta2")) beta2 = p["beta2"].get<float>();
	if (jhas(p, "epsilon")) epsilon = p["epsilon"].get<float>();
	if (jhas(p, "learning_rate")) learning_rate = p["learning_rate"].get<float>();
	if (jhas(p, "l2_reg")) l2_reg = p["l2_reg"].get<float>();
	if (jhas(p, "adabound")) adabound = p["adabound"].get<bool>();
	if (jhas(p, "relative_decay")) relative_decay = p["relative_decay"].get<float>();
	if (jhas(p, "absolute_decay")) absolute_decay = p["absolute_decay"].get<float>();
	if (jhas(p, "clipping_magnitude")) clipping_magnitude = p["clipping_magnitude"].get<float>();
	if (jhas(p, "non_matrix_learning_rate_factor")) non_matrix_learning_rate_factor = p["non_matrix_learning_rate_factor"].get<float>();
	if (jhas(p, "optimize_matrix_params")) optimize_matrix_params = p["optimize_matrix_params"].get<bool>();
	if (jhas(p, "optimize_non_matrix_params")) optimize_non_matrix_params = p["optimize_non_matrix_params"].get<bool>();
}

json AdamHost::hyperparams() const {
	return {{"otype", "Adam"}, {"beta1", beta1}, {"beta2", beta2}, {"epsilon", epsilon}, {"learning_rate", learning_rate},
	        {"l2_reg", l2_reg}, {"adabound", adabound}, {"relative_decay", relative_decay}, {"absolute_decay", absolute_decay},
	        {"clipping_magnitude", clipping_magnitude}, {"non_matrix_learning_rate_factor", non_matrix_learning_rate_factor},
	        {"optimize_matrix_params", optimize_matrix_params}, {"optimize_non_matrix_params", optimize_non_matrix_params}};
}

// ------------------------------------------------------------------------------------------
// Encodings (reference src/encoding.cu:77-150)
// ------------------------------------------------------------------------------------------
bool EncodingHost::is_grid_otype(const std::string& eo) {
	return ieq(eo, "HashGrid") || ieq(eo, "Grid") || ieq(eo, "TiledGrid") || ieq(eo, "DenseGrid");
}
static bool is_composite_otype(const std::string& eo) { return ieq(eo, "Composite") || ieq(eo, "NRC") || ieq(eo, "OneBlobFrequency"); }

bool EncodingHost::known(const std::string& eo) {
	return is_grid_otype(eo) || ieq(eo, "OneBlob") || ieq(eo, "Identity") || ieq(eo, "SphericalHarmonics") || ieq(eo, "TriangleWave") ||
	       is_composite_otype(eo);
}

EncodingHost::EncodingHost(uint32_t n_dims_to_encode, const json& enc, bool fp32) : n_dims(n_dims_to_encode), f32(fp32) {
	const std::string eo = jval<std::string>(enc, "otype", "OneBlob");  // encoding.cu:133
	TCNN_CHECK(known(eo), "Encoding '" + eo + "' is not implemented by the MI355X engine yet");
	if (ieq(eo, "Composite")) {
		parse_composite(enc);
	} else if (is_composite_otype(eo)) {  // NRC / OneBlobFrequency, encoding.cu:93-115
		const json tri = {{"n_dims_to_encode", 3}, {"otype", "TriangleWave"}, {"n_frequencies", jval<uint32_t>(enc, "n_frequencies", 12u)}};
		const json blob = {{"n_dims_to_encode", 5}, {"otype", "OneBlob"}, {"n_bins", jval<uint32_t>(enc, "n_bins", 4u)}};
		const json rest = {{"otype", "Identity"}};
		parse_composite(json{{"otype", "Composite"}, {"nested", json::array({tri, blob, rest})}});
	} else {  // standing alone: one part over every input column
		add_part(n_dims_to_encode, 0, enc);
	}
	otype = is_composite_otype(eo) ? "Composite" : parts[0].hyperparams()["otype"].get<std::string>();
	layout(1);
}

// CompositeEncoding::CompositeEncoding (composite.h:138-186)
void EncodingHost::parse_composite(const json& enc) {
	TCNN_CHECK(jhas(enc, "nested") && enc["nested"].is_array(), "Must provide an array of nested encodings to CompositeEncoding.");
	const std::string red = jval<std::string>(enc, "reduction", "Concatenation");
	TCNN_CHECK(ieq(red, "Concatenation") || ieq(red, "Sum") || ieq(red, "Product"), "Invalid reduction type: " + red);
	TCNN_CHECK(ieq(red, "Concatenation"),
	           "CompositeEncoding: reduction '" + red + "' is not implemented by the MI355X engine yet (only Concatenation)");
	const json& nested = enc["nested"];
	uint32_t total = 0;
	for (size_t i = 0; i < nested.size(); ++i) {
		total += jval<uint32_t>(nested[i], "n_dims_to_encode", 0u);
		if (jhas(nested[i], "dims_to_encode_begin")) {
			total = 0xFFFFFFFFu;
			break;
		}
	}
	TCNN_CHECK(total == 0xFFFFFFFFu || total <= n_dims, "CompositeEncoding: nested encodings must not encode more dims " +
	                                                        std::to_string(total) + " than composite " + std::to_string(n_dims));
	uint32_t unspecified = total == 0xFFFFFFFFu ? 0xFFFFFFFFu : n_dims - total;
	uint32_t off = 0;
	for (size_t i = 0; i < nested.size(); ++i) {
		uint32_t n;
		if (jhas(nested[i], "n_dims_to_encode")) {
			// dims_to_encode_begin counts only beside n_dims_to_encode (composite.h:166-171)
			if (jhas(nested[i], "dims_to_encode_begin")) off = nested[i]["dims_to_encode_begin"].get<uint32_t>();
			n = nested[i]["n_dims_to_encode"].get<uint32_t>();
		} else {
			TCNN_CHECK(unspecified != 0xFFFFFFFFu, "CompositeEncoding: may only leave 'n_dims_to_encode' unspecified for a single nested encoding");
			n = unspecified;
			unspecified = 0xFFFFFFFFu;
		}
		if (n > 0) add_part(n, off, nested[i]);
		off += n;
	}
	// nested encodings that share an input column are refused: the reference's dL/dinput is then
	// whatever the last of them wrote (order-dependent), and the plain stores here rely on it
	std::vector<int> owner(n_dims, -1);
	for (size_t i = 0; i < parts.size(); ++i) {
		const Part& p = parts[i];
		TCNN_CHECK(p.in_col + p.n_in <= n_dims, "CompositeEncoding: nested encoding " + std::to_string(i) + " reads input dims [" +
		                                            std::to_string(p.in_col) + ", " + std::to_string(p.in_col + p.n_in) +
		                                            ") beyond the composite's " + std::to_string(n_dims));
		for (uint32_t c = p.in_col; c < p.in_col + p.n_in; ++c) {
			TCNN_CHECK(owner[c] < 0, "CompositeEncoding: nested encodings " + std::to_string(owner[c]) + " and " + std::to_string(i) +
			                             " overlap in input dim " + std::to_string(c) + "; overlapping ranges are not supported");
			owner[c] = (int)i;
		}
	}
}

void EncodingHost::add_part(uint32_t n_in, uint32_t in_col, const json& enc) {
	const std::string eo = jval<std::string>(enc, "otype", "OneBlob");
	TCNN_CHECK(!ieq(eo, "Composite") && !ieq(eo, "NRC") && !ieq(eo, "OneBlobFrequency"),
	           "CompositeEncoding: a nested Composite encoding is not implemented by the MI355X engine yet");
	TCNN_CHECK(known(eo), "Encoding '" + eo + "' is not implemented by the MI355X engine yet");
	Part p;
	p.n_in = n_in;
	p.in_col = in_col;
	if (ieq(eo, "SphericalHarmonics")) {  // spherical_harmonics.h:105-120
		p.kind = COMP_SH;
		p.p0 = jval<uint32_t>(enc, "degree", 4u);
		TCNN_CHECK(n_in == 3, "Can only encode 3D directions in spherical harmonics.");
		TCNN_CHECK(p.p0 > 0, "Spherical harmonics must have positive degree.");
		TCNN_CHECK(p.p0 <= 8, "Spherical harmonics are only implemented up to degree 8.");
		p.n_values = p.p0 * p.p0;
	} else if (ieq(eo, "TriangleWave")) {
		p.kind = COMP_TRIANGLE;
		p.p0 = jval<uint32_t>(enc, "n_frequencies", 12u);
		p.n_values = n_in * p.p0;
	} else if (ieq(eo, "OneBlob")) {
		p.kind = COMP_ONEBLOB;
		p.p0 = jval<uint32_t>(enc, "n_bins", 16u);
		TCNN_CHECK(p.p0 > 0 && (p.p0 & (p.p0 - 1)) == 0, "Number of bins must be a power of 2");
		p.n_values = n_in * p.p0;
	} else if (ieq(eo, "Identity")) {
		p.kind = COMP_IDENTITY;
		p.f0 = jval<float>(enc, "scale", 1.0f);
		p.f1 = jval<float>(enc, "offset", 0.0f);
		p.n_values = n_in;
	} else {
		p.kind = COMP_GRID;
		p.grid = std::make_unique<GridEncodingHost>(n_in, enc);
		p.bufs = std::make_unique<GridBwdBufs>();
		p.n_values = p.grid->n_features;
		if (f32) p.grid->build_plan_f32();
	}
	p.f32 = f32;
	parts.push_back(std::move(p));
}

// composite.h:188-198 (each part's output alignment), then Encoding::set_alignment on the composite
// (encoding.h:70, composite.h:380-384: the last part takes the rest)
void EncodingHost::layout(uint32_t alignment) {
	uint32_t col = 0, n_par = 0;
	for (size_t i = 0; i < parts.size(); ++i) {
		Part& p = parts[i];
		const uint32_t a = i + 1 < parts.size() ? parts[i + 1].required_alignment() : std::max(alignment, 1u);
		p.out_col = col;
		p.width = (col + p.n_values + a - 1) / a * a - col;
		col += p.width;
		p.param_offset = n_par;
		if (p.grid) {
			p.grid->n_to_pad = p.width - p.n_values;
			n_par += p.grid->n_params;
		}
	}
	n_grid_params = n_par;
	if (!lone_part()) build_table();
}

// The limits are the table's (a kernel argument, and LDS rows of `width`): they do not bind a part
// that stands alone with its own kernel.
void EncodingHost::build_table() {
	const uint32_t width = padded_output_width();
	TCNN_CHECK(n_dims <= COMP_MAX_INPUTS, "CompositeEncoding: at most " + std::to_string(COMP_MAX_INPUTS) + " input dims");
	TCNN_CHECK(parts.size() <= COMP_MAX_PARTS, "CompositeEncoding: at most " + std::to_string(COMP_MAX_PARTS) + " nested encodings");
	TCNN_CHECK(width <= COMP_MAX_WIDTH, "CompositeEncoding: encoded width " + std::to_string(width) + " exceeds " + std::to_string(COMP_MAX_WIDTH));
	table = CompTable{};
	table.n_parts = (uint32_t)parts.size();
	table.n_in = n_dims;
	table.width = width;
	std::vector<bool> read(n_dims, false);
	for (size_t i = 0; i < parts.size(); ++i) {
		const Part& p = parts[i];
		CompPart& c = table.parts[i];
		c.kind = p.kind;
		c.in_col = p.in_col;
		c.n_in = p.n_in;
		c.out_col = p.out_col;
		c.width = p.width;
		c.n_values = p.n_values;
		c.p0 = p.p0;
		c.p1 = 0;
		while (p.kind == COMP_ONEBLOB && (1u << c.p1) < p.p0) ++c.p1;
		c.f0 = p.f0;
		c.f1 = p.f1;
		for (uint32_t d = 0; d < p.n_in; ++d) read[p.in_col + d] = true;
		if (p.kind == COMP_GRID) {
			for (uint32_t j = p.out_col; j < p.out_col + p.n_values; ++j) table.grid_cols[j / 32] |= 1u << (j % 32);
			if (p.width > p.n_values) table.fwd_work = 1;
			continue;
		}
		table.fwd_work = 1;
		for (uint32_t d = 0; d < (p.kind == COMP_SH ? 1u : p.n_in); ++d) {
			table.slot_part[table.n_slots] = (uint8_t)i;
			table.slot_col[table.n_slots++] = (uint8_t)(p.in_col + d);
		}
	}
	for (uint32_t c = 0; c < n_dims; ++c)
		if (!read[c]) {
			table.slot_part[table.n_slots] = (uint8_t)COMP_SLOT_ZERO;
			table.slot_col[table.n_slots++] = (uint8_t)c;
		}
}

void EncodingHost::initialize_params(Pcg32& rng, float* out, float s) const {
	// composite.h:422-427: the nested encodings in order, one generator
	for (const Part& p : parts)
		if (p.grid) p.grid->initialize_params(rng, out + p.param_offset, s);
}

json EncodingHost::Part::hyperparams() const {
	switch (kind) {
		case COMP_SH: return {{"otype", "SphericalHarmonics"}, {"degree", p0}};
		case COMP_TRIANGLE: return {{"otype", "TriangleWave"}, {"n_frequencies", p0}};
		case COMP_ONEBLOB: return {{"otype", "OneBlob"}, {"n_bins", p0}};
		case COMP_IDENTITY: return {{"otype", "Identity"}, {"scale", f0}, {"offset", f1}};
		default: return grid->hyperparams();
	}
}

json EncodingHost::hyperparams() const {
	if (otype != "Composite") return parts[0].hyperparams();
	json nested = json::array();
	for (const Part& p : parts) nested.push_back(p.hyperparams());
	return {{"otype", "Composite"}, {"nested", nested}};  // composite.h:437-447
}

// fn(T{}) with T the element type of an encoding's precision: one body for the fp16 and the fp32 module
template <typename Fn>
static void with_precision(bool f32, Fn&& fn) {
	if (f32) fn(float{});
	else fn(_Float16{});
}

void EncodingHost::Part::forward(hipStream_t st, uint32_t B, const float* x, uint32_t x_stride, const void* params16, void* out16,
                                 uint32_t stride, bool alone) const {
	with_precision(f32, [&](auto zero) {
		using T = decltype(zero);
		T* out = (T*)out16 + out_col;
		if (kind == COMP_ONEBLOB) return launch_oneblob_fwd(st, B, n_in, p0, x + in_col, x_stride, out, stride, width - n_values);
		if (kind == COMP_IDENTITY) return launch_identity_fwd(st, B, n_in, f0, f1, x + in_col, x_stride, out, stride, width - n_values);
		TCNN_CHECK(kind == COMP_GRID, "this encoding has no kernel of its own");
		TCNN_CHECK(params16, "grid forward needs the grid parameters");
		if (alone && width > n_values) TCNN_HIP_CHECK(hipMemsetAsync(out16, 0, (size_t)B * stride * sizeof(T), st));
		const T* table = (const T*)params16 + param_offset;
		// the fp32 forward writes its value columns only; the fp16 one whole rows, or the part's columns
		if constexpr (sizeof(T) == 4) grid->forward_f32(st, B, x + in_col, x_stride, table, out, stride);
		else grid->forward(st, B, x + in_col, x_stride, table, out, false, stride, alone ? 0u : n_values);
	});
}

void EncodingHost::Part::backward_input(hipStream_t st, uint32_t B, const float* x, uint32_t x_stride, const void* params16,
                                        const void* dy16, int dy_layout, uint32_t stride, float* dx) const {
	TCNN_CHECK(!f32 || dy_layout == 2, "an fp32 encoding reads dL/d(encoding) as AoS rows");
	with_precision(f32, [&](auto zero) {
		using T = decltype(zero);
		const T* dy = (const T*)dy16 + out_col;
		if (kind == COMP_ONEBLOB) return launch_oneblob_bwd(st, B, n_in, p0, x + in_col, x_stride, dy, stride, dx + in_col, x_stride);
		if (kind == COMP_IDENTITY) return launch_identity_bwd(st, B, n_in, f0, dy, stride, dx + in_col, x_stride);
		TCNN_CHECK(kind == COMP_GRID, "this encoding has no kernel of its own");
		TCNN_CHECK(params16, "grid backward_input needs the grid parameters");
		grid->backward_input(st, B, x + in_col, x_stride, (const T*)params16 + param_offset, dy, dy_layout, stride, dx + in_col, x_stride);
	});
}

void EncodingHost::forward_aos(hipStream_t st, uint32_t B, const float* x, const void* params16, void* out16) const {
	const uint32_t W = padded_output_width();
	if (const Part* p = lone_part()) return p->forward(st, B, x, n_dims, params16, out16, W, true);
	// one launch for every parameter-free value and all padding; each grid its own column slice
	with_precision(f32, [&](auto zero) { launch_composite_fwd(st, B, x, (decltype(zero)*)out16, table); });
	for (const Part& p : parts)
		if (p.grid) p.forward(st, B, x, n_dims, params16, out16, W, false);
}

void EncodingHost::backward_input(hipStream_t st, uint32_t B, const float* x, const void* dy16, float* dx, const void* params16,
                                  int dy_layout) const {
	const uint32_t W = padded_output_width();
	TCNN_CHECK(dy_layout == 2 || lone_grid(), "backward_input reads dL/d(encoding) as AoS rows");
	if (const Part* p = lone_part()) return p->backward_input(st, B, x, n_dims, params16, dy16, dy_layout, W, dx);
	with_precision(f32, [&](auto zero) { launch_composite_bwd_input(st, B, x, (const decltype(zero)*)dy16, W, dx, table); });
	for (const Part& p : parts)
		if (p.grid) p.backward_input(st, B, x, n_dims, params16, dy16, 2, W, dx);
}

void EncodingHost::backward_params(hipStream_t st, uint32_t B, const float* x, const void* dy16, int dy_layout, float* grad32) const {
	const uint32_t W = padded_output_width();
	TCNN_CHECK(dy_layout == 2 || lone_grid(), "backward_params reads dL/d(encoding) as AoS rows");
	for (const Part& p : parts) {
		if (!p.grid) continue;
		if (f32) p.grid->backward_f32(st, *p.bufs, B, x + p.in_col, n_dims, (const float*)dy16 + p.out_col, W, grad32 + p.param_offset);
		else p.grid->backward(st, *p.bufs, B, x + p.in_col, n_dims, (const _Float16*)dy16 + p.out_col, dy_layout, W, grad32 + p.param_offset);
	}
}

// ------------------------------------------------------------------------------------------
// NetworkWithInputEncoding
// ------------------------------------------------------------------------------------------
NetworkHost::NetworkHost(uint32_t n_in, uint32_t n_out, const json& e, const json& net, uint32_t loss)
	: n_input_dims(n_in), n_output_dims(n_out), loss_type(loss) {
	enc = std::make_unique<EncodingHost>(n_in, e);
	grid = enc->lone_grid();
	enc->set_alignment(16);  // minimum_alignment(network): 16 for FullyFusedMLP and CutlassMLP (network.cu:76-95)
	mlp = MlpHost(enc->padded_output_width(), n_out, net);
	TCNN_CHECK(fused_ok() || layered_ok(), "network shape (n_neurons = " + std::to_string(mlp.width) + ", input width " +
	                                           std::to_string(mlp.n_input) + ") is not supported by the MI355X engine");
	log_debug(std::string("NetworkWithInputEncoding: ") + mlp.otype + " (n_neurons=" + std::to_string(mlp.width) +
	          ", n_hidden_layers=" + std::to_string(mlp.n_hidden_layers) + ") runs on the " + engine() + " engine");
}

bool NetworkHost::fused_ok() const {
	// CutlassMLP / "MLP" run on the layer-wise engine (the reference's separate GEMM-per-layer network)
	const bool ff = ieq(mlp.otype, "FullyFusedMLP") || ieq(mlp.otype, "MegakernelMLP");
	if (sw.no_fused_grid) return false;  // A/B switch: the tile engine instead
	if (!fused_train_loss_supported(mlp.width, mlp.n_hidden_layers, loss_type)) return false;  // the tile engine instead
	return ff && grid && grid->n_to_pad == 0 && !grid->opts().active && mlp.output_activation == 0 &&
	       (mlp.activation == ACT_NONE || mlp.activation == ACT_RELU) &&
	       fused_train_supported(mlp.width, mlp.n_input, mlp.n_hidden_layers, grid->desc.n_pos_dims,
	                             grid->desc.n_features_per_level, mlp.padded_output, mlp.activation, grid->desc.hash_type);
}

bool NetworkHost::tile_shape_ok() const {
	const bool ff = ieq(mlp.otype, "FullyFusedMLP") || ieq(mlp.otype, "MegakernelMLP");
	if (!ff || mlp.output_activation == ACT_SINE) return false;  // Sine has no post-activation backward (common_device.h:271-275)
	if (sw.no_tile_engine) return false;  // A/B switch: the layer-wise engine instead
	return tile_train_supported(mlp.width, mlp.n_input, mlp.n_hidden_layers, mlp.padded_output, mlp.activation);
}

bool NetworkHost::tile_ok() const { return !fused_ok() && tile_shape_ok(); }

bool NetworkHost::tile_infer_ok() const {
	return tile_shape_ok() && tile_infer_supported(mlp.width, mlp.n_input, mlp.n_hidden_layers, mlp.padded_output, mlp.activation);
}

const char* NetworkHost::inference_engine() const {
	if (fused_ok() && mlp_infer_supported(mlp.width, mlp.n_input, mlp.n_hidden_layers, mlp.padded_output, mlp.activation)) return "fused";
	if (tile_infer_ok()) return "fused";
	return layered_ok() ? "layered" : "unsupported";
}

// any width / input width / padded output that is a multiple of 16 (layers above 128 run k_wide_layer)
bool NetworkHost::layered_ok() const {
	return layered_width_supported(mlp.width) && mlp.n_input % 16 == 0 && layered_width_supported(mlp.n_input) &&
	       layered_width_supported(mlp.padded_output) && mlp.activation != ACT_SINE &&
	       mlp.output_activation != ACT_SINE;  // Sine has no post-activation backward
}

void NetworkHost::initialize_params(Pcg32& rng, float* out, float scale) const {
	mlp.initialize_params(rng, out, scale);
	enc->initialize_params(rng, out + mlp.n_params(), scale);
}

json NetworkHost::hyperparams() const {
	return {{"otype", "NetworkWithInputEncoding"}, {"encoding", enc->hyperparams()}, {"network", mlp.hyperparams()}};
}

void NetworkHost::forward_layers(hipStream_t st, StepWorkspace& ws, uint32_t B, const void* params16, void* out16, bool keep) {
	const uint32_t W = mlp.width, IN = mlp.n_input, NH = mlp.n_hidden_layers, OUTP = mlp.padded_output;
	const _Float16* p = (const _Float16*)params16;
	ws.acts.reserve((size_t)(keep ? NH : 2) * B * W * 2);
	auto act_buf = [&](uint32_t j) { return ws.acts.as<_Float16>() + (size_t)(keep ? j : (j & 1)) * B * W; };
	const void* x = ws.enc16.p;
	uint32_t K = IN;
	for (uint32_t j = 0; j < NH; ++j) {
		launch_layer_fwd(st, B, W, K, p, x, act_buf(j), mlp.activation);
		p += (size_t)W * K;
		x = act_buf(j);
		K = W;
	}
	launch_layer_fwd(st, B, OUTP, K, p, x, out16, mlp.output_activation);
}

void NetworkHost::inference(hipStream_t st, StepWorkspace& ws, uint32_t B, const float* pos, const void* params16, void* out16,
                            bool trust_image) {
	TCNN_CHECK(B % 32 == 0, "inference: batch must be a multiple of 32");
	const uint32_t IN = mlp.n_input;
	const void* eparams = enc_params(params16);
	if (fused_ok() && mlp_infer_supported(mlp.width, IN, mlp.n_hidden_layers, mlp.padded_output, mlp.activation)) {
		// the trainer's packed image when it matches its parameters, else the kernel builds its LDS
		// image from the parameters themselves (no pack launch)
		fused_forward(st, ws, B, pos, params16, trust_image && ws.wimage_valid, nullptr, out16);
		return;
	}
	ws.enc16.reserve((size_t)IN * B * 2);
	if (tile_infer_ok()) {  // the whole network in one launch (mlp_tile.h k_mlp_tile_infer)
		enc->forward_aos(st, B, pos, eparams, ws.enc16.p);
		launch_mlp_tile_infer(st, mlp.width, IN, mlp.n_hidden_layers, mlp.activation, mlp.output_activation, B, params16, ws.enc16.p, out16);
		return;
	}
	TCNN_CHECK(layered_ok(), "inference: network shape not supported by the MI355X engine");
	enc->forward_aos(st, B, pos, eparams, ws.enc16.p);
	forward_layers(st, ws, B, params16, out16, false);
}

// grid encoding + MLP forward on the packed weight image (ws.wimage): one kernel (k_fused_fwd_grid),
// or under TCNN_SPLIT_FORWARD the SoA grid forward then k_mlp_infer. enc_soa (nullable) receives the
// encoding [IN][B] for a training context's backward.
void NetworkHost::fused_forward(hipStream_t st, StepWorkspace& ws, uint32_t B, const float* pos, const void* params16, bool use_image,
                                void* enc_soa, void* out16) {
	const uint32_t IN = mlp.n_input;
	const void* eparams = enc_params(params16);
	if (sw.split_forward) {
		if (!use_image) {
			ws.wimage.reserve(fused_weight_image_bytes(mlp.width, IN, mlp.n_hidden_layers));
			launch_pack_weights(st, mlp.width, IN, mlp.n_hidden_layers, params16, ws.wimage.p);
			ws.wimage_valid = false;  // packed from these parameters, which need not be the trainer's
		}
		void* enc = enc_soa;
		if (!enc) {
			ws.enc16.reserve((size_t)IN * B * 2);
			enc = ws.enc16.p;
		}
		grid->forward(st, B, pos, grid->desc.n_pos_dims, eparams, enc, true, 0);
		launch_mlp_infer(st, mlp.width, IN, mlp.n_hidden_layers, mlp.activation, true, B, ws.wimage.p, enc, out16);
		return;
	}
	launch_fused_fwd(st, grid->call(), mlp.width, IN, mlp.n_hidden_layers, mlp.activation, B, weight_image(st, ws, params16, use_image),
	                 params16, eparams, pos, enc_soa, out16);
}

const void* NetworkHost::weight_image(hipStream_t st, StepWorkspace& ws, const void* params16, bool have_image) {
	if (have_image) return ws.wimage.p;
	if (((uintptr_t)params16 & 15) == 0) return nullptr;  // the kernel's 16-byte loads build the image
	ws.wimage.reserve(fused_weight_image_bytes(mlp.width, mlp.n_input, mlp.n_hidden_layers));
	launch_pack_weights(st, mlp.width, mlp.n_input, mlp.n_hidden_layers, params16, ws.wimage.p);
	ws.wimage_valid = false;  // packed from these parameters, which need not be the trainer's
	return ws.wimage.p;
}

int NetworkHost::backward_engine_keep(bool with_dinput) const {
	if (fused_ok() && !with_dinput) return KEEP_FUSED_SOA;
	if (tile_shape_ok()) return KEEP_TILE_AOS;
	return KEEP_NONE;
}

int NetworkHost::forward_keep(hipStream_t st, StepWorkspace& ws, uint32_t B, const float* pos, const void* params16, void* out16,
                              bool with_dinput, DevBuf& keep) {
	const int layout = backward_engine_keep(with_dinput);
	const uint32_t IN = mlp.n_input;
	const void* eparams = enc_params(params16);
	if (layout == KEEP_FUSED_SOA && mlp_infer_supported(mlp.width, IN, mlp.n_hidden_layers, mlp.padded_output, mlp.activation)) {
		keep.reserve((size_t)IN * B * 2);
		fused_forward(st, ws, B, pos, params16, false, keep.p, out16);
		return KEEP_FUSED_SOA;
	}
	if (layout == KEEP_TILE_AOS && tile_infer_ok()) {
		keep.reserve((size_t)IN * B * 2);
		enc->forward_aos(st, B, pos, eparams, keep.p);
		launch_mlp_tile_infer(st, mlp.width, IN, mlp.n_hidden_layers, mlp.activation, mlp.output_activation, B, params16, keep.p, out16);
		return KEEP_TILE_AOS;
	}
	inference(st, ws, B, pos, params16, out16);
	return KEEP_NONE;
}

NetworkHost::BackwardKernel NetworkHost::backward_kernel_kind(bool with_dinput) const {
	if (fused_ok() && !with_dinput) return BackwardKernel::Register;
	if (tile_shape_ok()) return BackwardKernel::Tile;
	return layered_ok() ? BackwardKernel::Layered : BackwardKernel::Unsupported;
}

const char* NetworkHost::backward_kernel(bool with_dinput) const {
	switch (backward_kernel_kind(with_dinput)) {
		case BackwardKernel::Register: return "register";
		case BackwardKernel::Tile: return "tile";
		case BackwardKernel::Layered: return "layered";
		default: return "unsupported";
	}
}

bool NetworkHost::fwd_bwd(hipStream_t st, StepWorkspace& ws, const TrainPass& p) {
	switch (backward_kernel_kind(p.dL_dinput != nullptr)) {
		case BackwardKernel::Register: return fwd_bwd_fused(st, ws, p);
		case BackwardKernel::Tile: fwd_bwd_tile(st, ws, p); return false;
		default: fwd_bwd_layered(st, ws, p); return false;
	}
}

void NetworkHost::pack_weights(hipStream_t st, StepWorkspace& ws, const void* params16) {
	ws.wimage.reserve(fused_weight_image_bytes(mlp.width, mlp.n_input, mlp.n_hidden_layers));
	launch_pack_weights(st, mlp.width, mlp.n_input, mlp.n_hidden_layers, params16, ws.wimage.p);
	ws.wimage_valid = true;
}

void NetworkHost::fused_kernel(hipStream_t st, StepWorkspace& ws, const TrainPass& p, bool pack, bool emit_dy_bound) {
	const uint32_t B = p.B;
	TCNN_CHECK(B % 32 == 0, "training: batch must be a multiple of 32");
	const uint32_t n_mlp = mlp.n_params();
	const uint32_t L = grid->desc.n_levels, F = grid->desc.n_features_per_level;
	const void* enc_soa = p.kept_as(KEEP_FUSED_SOA);
	const uint32_t nb = fused_train_n_blocks(mlp.width, mlp.n_input, mlp.n_hidden_layers, grid->desc.n_pos_dims, p.dims,
	                                         p.dout16 != nullptr, B);
	ws.n_fused_blocks = nb;
	ws.n_loss_partials = nb;
	ws.dLdenc.reserve((size_t)L * F * B * 2);
	// slice sums for the grid backward's streaming pre-pass (D == 2, F == 2: the shapes it exists for)
	// (the kernel variants with an external dL/dy or an encoding read from memory do not emit them)
	ws.dy_bound_live = emit_dy_bound && !sw.no_grid_bwd_stream && !p.dout16 && !enc_soa && grid->desc.n_pos_dims == 2 && F == 2;
	if (ws.dy_bound_live) ws.dy_bound.reserve((size_t)L * (B / 32) * 4);
	ws.wgrad_partial.reserve((size_t)nb * n_mlp * 4);
	ws.loss_partial.reserve((size_t)nb * 4);
	// without a packed image that matches params16, every workgroup builds its LDS image from the
	// parameters (load_weights_lds_v) -- no k_pack_weights launch; the Adam tail of the grid backward
	// still writes the next step's image into ws.wimage
	ws.wimage.reserve(fused_weight_image_bytes(mlp.width, mlp.n_input, mlp.n_hidden_layers));
	FusedTrainArgs a{};
	a.wimage = (const _Float16*)weight_image(st, ws, p.params16, !pack && ws.wimage_valid);
	a.B = B;
	a.dims = p.dims;
	a.loss_scale = p.loss_scale;
	a.loss_type = loss_type;
	a.params = (const _Float16*)p.params16;
	a.table = (const uint32_t*)enc_params(p.params16);
	a.pos = p.pos;
	a.target = p.target;
	a.out = (_Float16*)p.out16;
	a.dLdenc = ws.dLdenc.as<uint32_t>();
	a.wgrad_partial = ws.wgrad_partial.as<float>();
	a.loss_partial = ws.loss_partial.as<float>();
	a.dout = (const _Float16*)p.dout16;
	a.dout_scale = p.dout16 && p.dout_scale != 0.0f ? p.dout_scale : 1.0f;
	a.enc = (const _Float16*)enc_soa;
	a.dy_bound = ws.dy_bound_live ? ws.dy_bound.as<float>() : nullptr;
	a.wt_stores = sw.wt_stores;
	launch_fused_train(st, grid->call(), mlp.width, mlp.n_input, mlp.n_hidden_layers, mlp.activation, a, nb);
}

void NetworkHost::grid_backward(hipStream_t st, StepWorkspace& ws, uint32_t B, const float* pos, GridBwdEpilogue* ep) {
	if (ep) {
		ep->wimage = ws.wimage.as<_Float16>();
		ep->W = mlp.width;
		ep->IN = mlp.n_input;
		ep->NH = mlp.n_hidden_layers;
		fused_image_layout(mlp.width, mlp.n_input, mlp.n_hidden_layers, &ep->RSI, &ep->RSW, &ep->oWh, &ep->oWo);
		ep->wpart = ws.wgrad_partial.as<float>();
		ep->n_wparts = ws.n_fused_blocks;
		ep->lpart = ws.loss_partial.as<float>();
	}
	grid->backward_items(st, ws.gbw, B, pos, grid->desc.n_pos_dims, ws.dLdenc.p, 0, 0, ep, ep ? ep->n_mlp_groups : 0u,
	                     ws.dy_bound_live ? ws.dy_bound.as<float>() : nullptr);
	grid->backward_bin(st, ws.gbw, B, pos, grid->desc.n_pos_dims, ws.dLdenc.p, 0, 0);
	if (ep && ep->apply_adam) ws.wimage_valid = true;  // the epilogue wrote the image of the updated weights
}

bool NetworkHost::fwd_bwd_fused(hipStream_t st, StepWorkspace& ws, const TrainPass& p) {
	const uint32_t n_mlp = mlp.n_params();
	fused_kernel(st, ws, p, true);
	p.mark(st, 1);
	// the network-gradient column sums run in the grid backward's spare workgroups (the epilogue
	// without Adam: block_column_sums, the order of launch_column_sums), not as a launch of their own
	GridBwdEpilogue ep{};
	ep.enabled = 1;
	ep.apply_adam = 0;
	ep.buf.g32 = p.grad32;
	ep.n_mlp_groups = mlp_tail_groups();
	ep.n_mlp = n_mlp;
	ws.loss_sum.reserve(16);
	ep.d_loss = ws.loss_sum.as<float>();
	TCNN_CHECK(n_mlp % 4 == 0, "network parameter count must be a multiple of 4");
	// the torch binding's finalised gradient straight from the two reductions (no k_grad_finalize
	// pass) when every grid level goes through the slabs
	const bool fin = p.fin.out && grid->bin_levels.empty();
	GradFinalize fin_grid{};
	if (fin) {
		ep.fin = p.fin;
		fin_grid = p.fin;
		fin_grid.out = (char*)p.fin.out + (size_t)n_mlp * (p.fin.out_f32 ? 4 : 2);
	}
	grid_backward(st, ws, p.B, p.pos, &ep);
	grid->backward_acc(st, ws.gbw, p.B, ws.dLdenc.p, 0, 0, p.grad32 + n_mlp);
	p.mark(st, 2);
	grid->reduce_items(st, ws.gbw, p.grad32 + n_mlp, fin_grid);
	p.mark(st, 3);
	return fin;
}

const void* NetworkHost::scaled_dout(hipStream_t st, StepWorkspace& ws, const TrainPass& p) {
	if (!p.dout16 || p.dout_scale == 0.0f) return p.dout16;
	const size_t n_out = (size_t)p.B * mlp.padded_output;
	ws.dout_scaled.reserve(n_out * 2);
	launch_scale_f16(st, p.dout16, ws.dout_scaled.p, p.dout_scale, n_out);
	return ws.dout_scaled.p;
}

// Tile-engine training pass (mlp_tile.hip): encoding forward (AoS fp16), one fused kernel for the
// whole network over 32-sample tiles (forward, loss, backward, weight-gradient partials, dL/d(enc)),
// the partial reduction, then the encoding's backward.
void NetworkHost::fwd_bwd_tile(hipStream_t st, StepWorkspace& ws, const TrainPass& p) {
	const uint32_t B = p.B;
	TCNN_CHECK(B % 32 == 0, "training: batch must be a multiple of 32");
	const uint32_t W = mlp.width, IN = mlp.n_input, NH = mlp.n_hidden_layers;
	const uint32_t n_mlp = mlp.n_params();
	const void* eparams = enc_params(p.params16);
	const void* dout16 = scaled_dout(st, ws, p);
	const void* enc_aos = p.kept_as(KEEP_TILE_AOS);
	if (!enc_aos) {
		ws.enc16.reserve((size_t)B * IN * 2);
		enc->forward_aos(st, B, p.pos, eparams, ws.enc16.p);
		enc_aos = ws.enc16.p;
	}
	const uint32_t nb = tile_train_blocks(B, W, IN, NH);
	ws.wgrad_partial.reserve((size_t)nb * n_mlp * 4);
	ws.loss_partial.reserve((size_t)nb * 4);
	const bool enc_grad = enc->n_params() > 0 || p.dL_dinput;
	const int dy_layout = enc->dy_layout();
	if (enc_grad) ws.delta0.reserve((size_t)B * IN * 2);
	const uint32_t wT_bytes = tile_train_wT_bytes(W, IN, NH);
	if (wT_bytes) ws.tile_wT.reserve(wT_bytes);
	TileTrainArgs a{};
	a.B = B;
	a.dims = p.dims;
	a.loss_type = loss_type;
	a.loss_scale = p.loss_scale;
	a.out_act = mlp.output_activation;
	a.params = (const _Float16*)p.params16;
	a.wT = wT_bytes ? ws.tile_wT.as<_Float16>() : nullptr;
	a.enc = (const _Float16*)enc_aos;
	a.target = p.target;
	a.dout = (const _Float16*)dout16;
	a.out = (_Float16*)p.out16;
	a.dldenc = enc_grad ? ws.delta0.p : nullptr;
	a.dldenc_pairs = dy_layout == 0 ? 1 : 0;
	a.wgrad_partial = ws.wgrad_partial.as<float>();
	a.loss_partial = ws.loss_partial.as<float>();
	launch_mlp_tile_train(st, W, IN, NH, mlp.activation, a);
	ws.n_loss_partials = dout16 ? 0 : nb;
	const size_t tf = reduce_partials_tmp_floats(nb, n_mlp);
	if (tf) ws.red_tmp.reserve(tf * 4);
	launch_reduce_partials(st, ws.wgrad_partial.as<float>(), nb, n_mlp, n_mlp, p.grad32, ws.red_tmp.as<float>());
	p.mark(st, 1);
	if (p.dL_dinput) enc->backward_input(st, B, p.pos, ws.delta0.p, p.dL_dinput, eparams, dy_layout);
	enc->backward_params(st, B, p.pos, ws.delta0.p, dy_layout, p.grad32 + n_mlp);
	p.mark(st, 2);
	p.mark(st, 3);
}

// Layer-wise training pass (reference FullyFusedMLP::forward_impl/backward_impl dataflow,
// fully_fused_mlp.cu:680-836; CutlassMLP cutlass_mlp.cu:120-315).
void NetworkHost::fwd_bwd_layered(hipStream_t st, StepWorkspace& ws, const TrainPass& p) {
	const uint32_t B = p.B, dims = p.dims;
	const float* pos = p.pos;
	const float* target = p.target;
	const void* params16 = p.params16;
	void* out16 = p.out16;
	float* grad32 = p.grad32;
	float* dL_dinput = p.dL_dinput;
	TCNN_CHECK(layered_ok(), "training: network/encoding configuration not supported by the MI355X engine");
	TCNN_CHECK(B % 32 == 0, "training: batch must be a multiple of 32");
	const uint32_t W = mlp.width, IN = mlp.n_input, NH = mlp.n_hidden_layers, OUTP = mlp.padded_output;
	const uint32_t n_mlp = mlp.n_params();
	const _Float16* p16 = (const _Float16*)params16;
	const void* eparams = enc_params(params16);
	const uint32_t nck = wgrad_n_chunks(B);
	const uint32_t maxK = std::max(W, IN);
	ws.enc16.reserve((size_t)B * IN * 2);
	ws.out16.reserve((size_t)B * OUTP * 2);
	ws.dout16.reserve((size_t)B * OUTP * 2);
	ws.delta0.reserve((size_t)B * std::max(W, IN) * 2);
	ws.delta1.reserve((size_t)B * std::max(W, IN) * 2);
	ws.wgrad_partial.reserve((size_t)nck * std::max(W, OUTP) * maxK * 4);

	const void* dout16 = scaled_dout(st, ws, p);

	// forward
	enc->forward_aos(st, B, pos, eparams, ws.enc16.p);
	void* out = out16 ? out16 : ws.out16.p;
	forward_layers(st, ws, B, params16, out, true);
	auto act = [&](uint32_t j) { return ws.acts.as<_Float16>() + (size_t)j * B * W; };

	// loss / external dL/dout (loss-scaled by the caller) -> G fp16 [B][OUTP]
	if (dout16) {
		TCNN_HIP_CHECK(hipMemcpyAsync(ws.dout16.p, dout16, (size_t)B * OUTP * 2, hipMemcpyDeviceToDevice, st));
		ws.n_loss_partials = 0;
	} else {
		const uint32_t nl = relative_l2_n_blocks(B, OUTP);
		ws.loss_partial.reserve((size_t)nl * 4);
		launch_relative_l2_partial(st, B, OUTP, dims, p.loss_scale, out, target, ws.dout16.p, ws.loss_partial.as<float>(), loss_type);
		ws.n_loss_partials = nl;
	}
	launch_act_bwd_inplace(st, B * OUTP, mlp.output_activation, out, ws.dout16.p);

	// backward: weight offsets [W0 | W1..W_{NH-1} | Wout] ([Wout] alone for 0 hidden layers)
	auto w_off = [&](uint32_t j) -> size_t { return j == 0 ? 0 : (size_t)W * IN + (size_t)(j - 1) * W * W; };
	auto wgrad = [&](uint32_t N, uint32_t K, const void* dy, const void* x, size_t off) {
		launch_wgrad(st, B, N, K, dy, x, ws.wgrad_partial.as<float>(), nck);
		const size_t tf = reduce_partials_tmp_floats(nck, N * K);
		if (tf) ws.red_tmp.reserve(tf * 4);
		launch_reduce_partials(st, ws.wgrad_partial.as<float>(), nck, N * K, N * K, grad32 + off, ws.red_tmp.as<float>());
	};
	_Float16* dcur = ws.delta0.as<_Float16>();
	_Float16* dnext = ws.delta1.as<_Float16>();
	const bool enc_grad = enc->n_params() > 0 || dL_dinput;
	const int dy_layout = enc->dy_layout();
	const bool pairs = dy_layout == 0;
	const _Float16* denc = dnext;  // dL/d(encoding), when enc_grad
	if (NH == 0) {  // one matrix: dWout = dout^T enc, dL/d(encoding) = Wout^T dout (no transfer)
		wgrad(OUTP, IN, ws.dout16.p, ws.enc16.p, 0);
		p.mark(st, 1);
		if (enc_grad) launch_layer_bwd(st, B, OUTP, IN, p16, ws.dout16.p, nullptr, dnext, ACT_NONE, pairs);
	} else {
		// output layer
		wgrad(OUTP, W, ws.dout16.p, act(NH - 1), w_off(NH));
		launch_layer_bwd(st, B, OUTP, W, p16 + w_off(NH), ws.dout16.p, act(NH - 1), dcur, mlp.activation);
		for (uint32_t j = NH - 1; j >= 1; --j) {
			wgrad(W, W, dcur, act(j - 1), w_off(j));
			launch_layer_bwd(st, B, W, W, p16 + w_off(j), dcur, act(j - 1), dnext, mlp.activation);
			std::swap(dcur, dnext);
		}
		wgrad(W, IN, dcur, ws.enc16.p, 0);
		p.mark(st, 1);
		// dL/d(encoding) = W0^T delta_0 (no transfer), AoS [B][IN] or level-major pairs
		if (enc_grad) launch_layer_bwd(st, B, W, IN, p16, dcur, nullptr, dnext, ACT_NONE, pairs);
		denc = dnext;
	}
	if (dL_dinput) enc->backward_input(st, B, pos, denc, dL_dinput, eparams, dy_layout);
	enc->backward_params(st, B, pos, denc, dy_layout, grad32 + n_mlp);
	p.mark(st, 2);
	p.mark(st, 3);
}

// ------------------------------------------------------------------------------------------
// NetworkWithInputEncoding<float> (an fp32 network module; mlp_f32.hip)
// ------------------------------------------------------------------------------------------
NetworkF32Host::NetworkF32Host(uint32_t n_in, uint32_t n_out, const json& e, const json& net) : n_input_dims(n_in), n_output_dims(n_out) {
	enc = std::make_unique<EncodingHost>(n_in, e, true);
	enc->set_alignment(16);
	mlp = MlpHost(enc->padded_output_width(), n_out, net);
	TCNN_CHECK(mlp.width % 16 == 0 && mlp.width > 0, "fp32 network: n_neurons must be a multiple of 16, got " + std::to_string(mlp.width));
}

void NetworkF32Host::initialize_params(Pcg32& rng, float* out, float scale) const {
	mlp.initialize_params(rng, out, scale);
	enc->initialize_params(rng, out + mlp.n_params(), scale);
}

json NetworkF32Host::hyperparams() const {
	return {{"otype", "NetworkWithInputEncoding"}, {"encoding", enc->hyperparams()}, {"network", mlp.hyperparams()}};
}

void NetworkF32Host::forward(hipStream_t st, uint32_t B, const float* pos, const float* params, float* out32, float* keep) {
	const uint32_t W = mlp.width, IN = mlp.n_input, NH = mlp.n_hidden_layers, OUTP = mlp.padded_output;
	if (!keep) acts.reserve(((size_t)B * IN + 2 * (size_t)B * W) * 4);
	float* e = keep ? keep : acts.as<float>();
	float* h = e + (size_t)B * IN;
	auto act_buf = [&](uint32_t j) { return h + (size_t)(keep ? j : (j & 1)) * B * W; };
	enc->forward_aos(st, B, pos, params + mlp.n_params(), e);
	const float* p = params;
	const float* x = e;
	uint32_t K = IN;
	for (uint32_t j = 0; j < NH; ++j) {
		launch_f32_layer_fwd(st, B, W, K, p, x, act_buf(j), mlp.activation);
		p += (size_t)W * K;
		x = act_buf(j);
		K = W;
	}
	// with a keep the output lands there (the backward's output-activation transfer reads it) and is copied out
	float* y = keep ? h + (size_t)NH * B * W : out32;
	launch_f32_layer_fwd(st, B, OUTP, K, p, x, y, mlp.output_activation);
	if (keep && out32) TCNN_HIP_CHECK(hipMemcpyAsync(out32, y, (size_t)B * OUTP * 4, hipMemcpyDeviceToDevice, st));
}

void NetworkF32Host::backward(hipStream_t st, uint32_t B, const float* pos, const float* params, const float* dout32, const float* keep,
                              float* dL_dparams, float* dL_dinput) {
	TCNN_CHECK(!has_sine(), "Sine has no backward from its forward value: the MI355X engine serves it through inference only");
	const uint32_t W = mlp.width, IN = mlp.n_input, NH = mlp.n_hidden_layers, OUTP = mlp.padded_output;
	const uint32_t n_mlp = mlp.n_params();
	const float* e = keep;
	const float* h = e + (size_t)B * IN;
	auto act = [&](uint32_t j) { return h + (size_t)j * B * W; };
	const float* y = h + (size_t)NH * B * W;
	const float* eparams = params + n_mlp;
	const uint32_t nsl = f32_wgrad_n_slabs(B);
	const uint32_t maxK = std::max(W, IN);
	delta0.reserve((size_t)B * maxK * 4);
	delta1.reserve((size_t)B * maxK * 4);
	if (dL_dparams) wgrad_partial.reserve((size_t)nsl * std::max(W, OUTP) * maxK * 4);
	// weight offsets [W0 | W1 .. W_{NH-1} | Wout] ([Wout] alone for 0 hidden layers)
	auto w_off = [&](uint32_t j) -> size_t { return j == 0 ? 0 : (size_t)W * IN + (size_t)(j - 1) * W * W; };
	// dW = (dy o act'(yv))^T x: per-slab partial sums, then their fixed-order sum
	auto wgrad = [&](uint32_t N, uint32_t K, const float* dy, const float* yv, int a, const float* x, size_t off) {
		if (!dL_dparams) return;
		launch_f32_wgrad(st, B, N, K, dy, yv, a, x, wgrad_partial.as<float>());
		const size_t tf = reduce_partials_tmp_floats(nsl, N * K);
		if (tf) red_tmp.reserve(tf * 4);
		launch_reduce_partials(st, wgrad_partial.as<float>(), nsl, N * K, N * K, dL_dparams + off, red_tmp.as<float>());
	};
	float* dcur = delta0.as<float>();
	float* dnext = delta1.as<float>();
	const bool enc_grad = (dL_dparams && enc->n_params() > 0) || dL_dinput;
	// a delta here is dL/d(post-activation value): both of its readers apply the transfer as they load it
	if (NH == 0) {
		wgrad(OUTP, IN, dout32, y, mlp.output_activation, e, 0);
		if (enc_grad) launch_f32_layer_bwd(st, B, OUTP, IN, params, dout32, y, mlp.output_activation, dnext);
	} else {
		wgrad(OUTP, W, dout32, y, mlp.output_activation, act(NH - 1), w_off(NH));
		launch_f32_layer_bwd(st, B, OUTP, W, params + w_off(NH), dout32, y, mlp.output_activation, dcur);
		for (uint32_t j = NH - 1; j >= 1; --j) {
			wgrad(W, W, dcur, act(j), mlp.activation, act(j - 1), w_off(j));
			launch_f32_layer_bwd(st, B, W, W, params + w_off(j), dcur, act(j), mlp.activation, dnext);
			std::swap(dcur, dnext);
		}
		wgrad(W, IN, dcur, act(0), mlp.activation, e, 0);
		if (enc_grad) launch_f32_layer_bwd(st, B, W, IN, params, dcur, act(0), mlp.activation, dnext);
	}
	if (dL_dinput) enc->backward_input(st, B, pos, dnext, dL_dinput, eparams, 2);
	if (dL_dparams && enc->n_params() > 0) enc->backward_params(st, B, pos, dnext, 2, dL_dparams + n_mlp);
}

void NetworkF32Host::check_second_order() const {
	TCNN_CHECK(!has_sine(), "Sine has no backward from its forward value: the MI355X engine serves it through inference only");
	const EncodingHost::Part* lone = enc->lone_part();
	if (!lone || (lone->kind != COMP_IDENTITY && lone->kind != COMP_GRID))
		throw std::runtime_error("NetworkWithInputEncoding<float>::backward_backward_input behind " + enc->name() +
		                         ": not implemented error (Identity or a grid standing alone only)");
}

// Second order ("Second-order input gradients of fp32 network modules"). Layer j = 0..NH maps h_j (width
// K_j) to h_{j+1} = a_j(W_j h_j) (width N_j); D_j = dL/dh_j is the first-order delta, U_j = dL2/dD_j the tangent,
// R_j = T_j o D_{j+1} o a_j''(h_{j+1}) the curvature source and Q_j = dL2/d(pre-activation of layer j).
void NetworkF32Host::backward_backward_input(hipStream_t st, uint32_t B, const float* pos, const float* params, const float* dL_ddLdinput,
                                             const float* dout32, const float* keep, float* dL_dparams, float* dL_ddLdoutput,
                                             float* dL_dinput) {
	check_second_order();
	const EncodingHost::Part* lone = enc->lone_part();
	const GridEncodingHost* grid = enc->lone_grid();
	const bool identity = !grid;
	if (!dL_dparams && !dL_ddLdoutput && !dL_dinput) return;
	const bool need_d = dL_dparams || dL_dinput;  // everything but the tangent pass reads the first-order deltas
	TCNN_CHECK(dout32 || !need_d, "backward_backward_input: dL_dparams and dL_dinput need dL_doutput");
	TCNN_CHECK(dL_ddLdinput, "backward_backward_input: dL_ddLdinput is missing");
	const uint32_t W = mlp.width, IN = mlp.n_input, NH = mlp.n_hidden_layers, OUTP = mlp.padded_output;
	const uint32_t n_mlp = mlp.n_params(), n_enc = enc->n_params(), D = n_input_dims;
	const float* eparams = params + n_mlp;
	auto a = [&](uint32_t j) { return j < NH ? mlp.activation : mlp.output_activation; };
	auto Nj = [&](uint32_t j) { return j < NH ? W : OUTP; };
	auto Kj = [&](uint32_t j) { return j == 0 ? IN : W; };
	auto w_off = [&](uint32_t j) -> size_t { return j == 0 ? 0 : (size_t)W * IN + (size_t)(j - 1) * W * W; };
	// h_0 .. h_{NH+1} of the keep, and the same offsets for the chains kept here
	auto chain = [&](uint32_t j) -> size_t { return j == 0 ? 0 : (size_t)B * IN + (size_t)(j - 1) * B * W; };
	const size_t n_chain = chain(NH + 1), n_out = (size_t)B * OUTP;
	// [D_0 .. D_NH | U_0 .. U_NH | U_{NH+1} | R_0 .. R_NH (Q_j in place) | P_0 | dx of P_0]
	second.reserve((2 * n_chain + n_out + ((size_t)NH * B * W + n_out) + (size_t)B * IN + (size_t)B * D) * 4);
	float* Dc = second.as<float>();
	float* Uc = Dc + n_chain;
	float* Uout = Uc + n_chain;
	float* Rc = Uout + n_out;
	float* P0 = Rc + (size_t)NH * B * W + n_out;
	float* dx_tmp = P0 + (size_t)B * IN;
	auto hv = [&](uint32_t j) { return keep + chain(j); };
	auto Dv = [&](uint32_t j) -> const float* { return j == NH + 1 ? dout32 : Dc + chain(j); };
	auto Rv = [&](uint32_t j) { return Rc + (size_t)j * B * W; };

	// the first-order delta chain again (the forward context does not hold it); D_0 only a grid reads
	if (need_d)
		for (uint32_t j = NH + 1; j-- > (grid ? 0u : 1u);)
			launch_f32_layer_bwd(st, B, Nj(j), Kj(j), params + w_off(j), Dv(j + 1), hv(j + 1), a(j), Dc + chain(j));

	// 1: the encoding. U_0 = dL2/dD_0; a grid also gives its own dL2/dtable (atomic adds onto zeros) and dL2/dx
	if (grid) {
		if (dL_dparams) TCNN_HIP_CHECK(hipMemsetAsync(dL_dparams + n_mlp, 0, (size_t)n_enc * 4, st));
		grid->backward_backward_input(st, B, pos, enc->n_dims, eparams, dL_ddLdinput, need_d ? Dv(0) : nullptr, IN,
		                              dL_dparams ? dL_dparams + n_mlp : nullptr, Uc, IN, dL_dinput);
	} else {
		launch_f32_identity_tangent(st, B, lone->n_in, IN, lone->f0, dL_ddLdinput, Uc);
	}

	// 2: the tangent pass, bottom up; a layer with curvature leaves R_j beside U_{j+1}
	int top = -1;  // the highest layer with curvature: Q_j = 0 above it
	for (uint32_t j = 0; j <= NH; ++j) {
		float* r = need_d && f32_act_has_curvature(a(j)) ? Rv(j) : nullptr;
		if (r) top = (int)j;
		if (j == NH && !dL_ddLdoutput && !r) break;
		float* y = j < NH ? Uc + chain(j + 1) : dL_ddLdoutput ? dL_ddLdoutput : Uout;
		launch_f32_layer_tangent(st, B, Nj(j), Kj(j), params + w_off(j), Uc + chain(j), hv(j + 1), a(j), y, r ? Dv(j + 1) : nullptr, r);
	}
	if (!need_d) return;

	// 3: the curvature pass, top down, with both weight-gradient terms of a matrix in one fixed-order sum:
	// A = sum_b (D_{j+1} o a_j'(h_{j+1})) U_j^T in slabs [0, nsl), B = sum_b Q_j h_j^T in slabs [nsl, 2 nsl)
	const uint32_t nsl = f32_wgrad_n_slabs(B);
	if (dL_dparams) wgrad_partial.reserve((size_t)2 * nsl * std::max(W, OUTP) * std::max(W, IN) * 4);
	for (uint32_t j = NH + 1; j-- > 0;) {
		const uint32_t N = Nj(j), K = Kj(j);
		const bool have_q = (int)j <= top;
		if (dL_dparams) {
			float* part = wgrad_partial.as<float>();
			launch_f32_wgrad(st, B, N, K, Dv(j + 1), hv(j + 1), a(j), Uc + chain(j), part);
			if (have_q) launch_f32_wgrad(st, B, N, K, Rv(j), nullptr, ACT_NONE, hv(j), part + (size_t)nsl * N * K);
			const uint32_t n_parts = have_q ? 2 * nsl : nsl;
			const size_t tf = reduce_partials_tmp_floats(n_parts, N * K);
			if (tf) red_tmp.reserve(tf * 4);
			launch_reduce_partials(st, part, n_parts, N * K, N * K, dL_dparams + w_off(j), red_tmp.as<float>());
		}
		if (!have_q) continue;
		if (j > 0) {  // Q_{j-1} = R_{j-1} + (Q_j W_j) o a_{j-1}'(h_j), in R_{j-1}'s place
			const bool r_below = f32_act_has_curvature(a(j - 1));
			launch_f32_layer_curvature(st, B, N, K, params + w_off(j), Rv(j), hv(j), a(j - 1), r_below ? Rv(j - 1) : nullptr, Rv(j - 1));
		} else if (dL_dinput || (dL_dparams && n_enc)) {  // P_0 = Q_0 W_0 = dL2/d(encoded row)
			launch_f32_layer_bwd(st, B, N, K, params, Rv(0), nullptr, ACT_NONE, P0);
		}
	}
	// P_0 through the encoding's first-order backward, added to the grid's own terms
	if (top < 0) {
		if (identity && dL_dinput) TCNN_HIP_CHECK(hipMemsetAsync(dL_dinput, 0, (size_t)B * D * 4, st));
		return;
	}
	if (identity) {
		if (dL_dinput) enc->backward_input(st, B, pos, P0, dL_dinput, eparams, 2);
		return;
	}
	if (dL_dinput) {
		enc->backward_input(st, B, pos, P0, dx_tmp, eparams, 2);
		launch_f32_add(st, (size_t)B * D, dL_dinput, dx_tmp);
	}
	if (dL_dparams) {
		grid_tmp.reserve((size_t)n_enc * 4);
		enc->backward_params(st, B, pos, P0, 2, grid_tmp.as<float>());
		launch_f32_add(st, n_enc, dL_dparams + n_mlp, grid_tmp.as<float>());
	}
}

// ------------------------------------------------------------------------------------------
// Trainer (reference trainer.h:47-361, config.h:46-63)
// ------------------------------------------------------------------------------------------
TrainerHost::TrainerHost(uint32_t n_in, uint32_t n_out, const json& cfg, uint32_t seed)
	: n_input_dims(n_in), n_output_dims(n_out), config(cfg) {
	const json enc = jhas(cfg, "encoding") ? cfg["encoding"] : json::object();
	const json net = jhas(cfg, "network") ? cfg["network"] : json::object();
	const json opt = jhas(cfg, "optimizer") ? cfg["optimizer"] : json::object();
	const json los = jhas(cfg, "loss") ? cfg["loss"] : json::object();
	loss_otype = jval<std::string>(los, "otype", "RelativeL2");
	const int loss_type = loss_type_from_otype(loss_otype);
	TCNN_CHECK(loss_type >= 0, "Loss '" + loss_otype + "' is not implemented by the MI355X engine (" + loss_otype_list() + ")");
	const std::string oo = jval<std::string>(opt, "otype", "Adam");
	if (ieq(oo, "Adam")) {
		adam.update(opt);
	} else {  // a stacked optimizer or SGD (optimizer_tree.cpp); throws for the otypes the engine refuses
		this->opt = opt_build(opt);
		opt_inline = true;
		for (const OptNode* n = this->opt.get(); n; n = n->nested.get())
			if (n->kind != OptKind::Adam && n->kind != OptKind::ExponentialDecay && n->kind != OptKind::Ema) opt_inline = false;
	}
	model = std::make_unique<NetworkHost>(n_in, n_out, enc, net, (uint32_t)loss_type);
	TCNN_CHECK(loss_type != LOSS_RELATIVE_L2_LUMINANCE || model->mlp.padded_output >= 6,
	           "RelativeL2Luminance reads 6 columns of the padded output row");
	n_params = model->n_params();
	n_mlp = model->mlp.n_params();
	initialize_params(seed);
}

void TrainerHost::initialize_params(uint32_t seed) {
	// trainer.h:52-55: pcg32{seed_seq{seed}.generate()[0]}
	std::seed_seq seq{seed};
	std::vector<uint32_t> seeds(2);
	seq.generate(seeds.begin(), seeds.end());
	Pcg32 rng{seeds.front()};
	initialize_params_rng(rng);
}

void TrainerHost::initialize_params_rng(Pcg32& rng) {
	log_debug("Trainer: initializing " + std::to_string(n_params) + " params and resetting training.");  // trainer.h:70
	TCNN_HIP_CHECK(hipDeviceSynchronize());  // queued steps on the caller's stream must not race the reset
	std::vector<float> host(n_params);
	model->initialize_params(rng, host.data());
	w32.reserve(n_params * 4);
	w16.reserve(n_params * 2);
	g16.reserve(n_params * 2);
	g32.reserve(n_params * 4);
	m1.reserve(n_params * 4);
	m2.reserve(n_params * 4);
	steps.reserve(n_params * 4);
	d_loss.reserve(16);
	TCNN_HIP_CHECK(hipMemcpy(w32.p, host.data(), n_params * 4, hipMemcpyHostToDevice));
	TCNN_HIP_CHECK(hipMemset(g16.p, 0, n_params * 2));
	TCNN_HIP_CHECK(hipMemset(g32.p, 0, n_params * 4));
	TCNN_HIP_CHECK(hipMemset(m1.p, 0, n_params * 4));
	TCNN_HIP_CHECK(hipMemset(m2.p, 0, n_params * 4));
	TCNN_HIP_CHECK(hipMemset(steps.p, 0, n_params * 4));
	TCNN_HIP_CHECK(hipMemset(d_loss.p, 0, 16));
	if (n_step_blocks()) {  // every block uniform at count 0, like steps[]
		step_blocks.reserve((size_t)n_step_blocks() * 4);
		TCNN_HIP_CHECK(hipMemset(step_blocks.p, 0, (size_t)n_step_blocks() * 4));
	}
	grads_stale = false;
	steps_current = true;
	step_blocks_diverged = false;
	launch_cast_f32_f16(nullptr, w32.as<float>(), w16.p, n_params);
	TCNN_HIP_CHECK(hipDeviceSynchronize());
	adam_step = 0;
	ws.wimage_valid = false;
	if (this->opt) {
		opt_allocate();
		opt_reset_weights();
		TCNN_HIP_CHECK(hipDeviceSynchronize());
	}
}

void TrainerHost::set_params_full_precision(const float* host, uint64_t n) {
	TCNN_CHECK(n == n_params, "Can't set fp params because buffer has the wrong size.");
	TCNN_HIP_CHECK(hipDeviceSynchronize());  // queued training work must not race the upload
	TCNN_HIP_CHECK(hipMemcpy(w32.p, host, n * 4, hipMemcpyHostToDevice));
	launch_cast_f32_f16(nullptr, w32.as<float>(), w16.p, n_params);
	ws.wimage_valid = false;
	TCNN_HIP_CHECK(hipDeviceSynchronize());
	opt_reset_weights();
}

void TrainerHost::training_step(hipStream_t st, uint32_t B, const float* input, const float* target, bool run_optimizer) {
	TCNN_CHECK(B % BATCH_GRANULARITY == 0, "training_step: batch size must be a multiple of 256");
	// only the one-call step carries lean state on; every other schedule reads or overwrites g32 / g16 /
	// steps[] / the slabs
	if (!(run_optimizer && lean_mask() != 0)) lean_settle(LeanUse::Write);
	if (timer.enabled) {
		timer.sampling = (timer.counter++ % timer.every) == 0;
		if (timer.sampling) timer.marks.push_back({-1, -1, -1, -1, -1});
	}
	// a whole step with the optimizer replays as a hipGraph when enabled (not on the steps that record
	// phase events, not with AdaBound, whose bounds depend on the step)
	// (nor with a stacked optimizer, whose host-side schedule depends on the step: it steps eagerly)
	if (run_optimizer && use_graph && !opt && !(timer.enabled && timer.sampling) && !adam.adabound &&
	    training_step_graph(st, B, input, target))
		return;
	if (run_optimizer && opt) {
		opt_training_step(st, B, input, target);
		return;
	}
	if (run_optimizer) step_eager(st, B, input, target);
	else gradient_pass(st, B, input, target);
}

// the eager step with the optimizer, on whichever schedule is attached
void TrainerHost::step_eager(hipStream_t st, uint32_t B, const float* input, const float* target) {
	if (dp) training_step_dp(st, B, input, target);
	else if (peer_attached) training_step_peer(st, B, input, target);
	else step_adam(st, B, input, target);
}

void TrainerHost::step_adam(hipStream_t st, uint32_t B, const float* input, const float* target) {
	if (overlapped_ok()) training_step_overlapped(st, B, input, target, true);
	else training_step_sequential(st, B, input, target, true);
}

void TrainerHost::gradient_pass(hipStream_t st, uint32_t B, const float* input, const float* target, float* grad_out) {
	if (overlapped_ok()) training_step_overlapped(st, B, input, target, false, grad_out);
	else training_step_sequential(st, B, input, target, false, grad_out);
}

TrainPass TrainerHost::loss_pass(uint32_t B, const float* input, const float* target, float* grad32) const {
	TrainPass p;
	p.B = B;
	p.pos = input;
	p.params16 = w16.p;
	p.target = target;
	p.dims = n_output_dims;
	p.loss_scale = loss_scale;
	p.grad32 = grad32;
	return p;
}

// tile and layer-wise engines: the pass, the loss sum, then Adam (reference trainer.h:163-190)
void TrainerHost::training_step_sequential(hipStream_t st, uint32_t B, const float* input, const float* target, bool run_optimizer,
                                           float* grad_out) {
	timer.mark(st, 0);
	TrainPass p = loss_pass(B, input, target, (grad_out && !run_optimizer) ? grad_out : g32.as<float>());
	p.timer = &timer;
	model->fwd_bwd(st, ws, p);
	launch_sum(st, ws.loss_partial.as<float>(), ws.n_loss_partials, d_loss.as<float>());
	timer.mark(st, 4);
	last_B = B;
	if (run_optimizer) adam_apply(st, g32.as<float>(), grad_scale, g16.p);
}

// Training step of the fused engine in three launches on one stream (the reference's step is ~10
// kernels plus side streams, trainer.h:163-190): the fused grid+MLP kernel; the grid backward,
// whose 16 extra workgroups (on CUs the grid items leave free) reduce the fused kernel's
// network-gradient slabs and the loss and -- with the optimizer -- run Adam on the network and
// write the next step's weight image; then either Adam over the grid parameters summing the grid
// backward's chunk slabs on the fly, or (run_optimizer = false: the multi-GPU path, whose
// all-reduce sits between the gradients and Adam) the slab reduction into the fp32 gradient.
// Summation orders are the same either way (bit-identical parameters).
void TrainerHost::training_step_overlapped(hipStream_t st, uint32_t B, const float* input, const float* target, bool run_optimizer,
                                           float* grad_out) {
	NetworkHost& m = *model;
	float* const gsum = (grad_out && !run_optimizer) ? grad_out : g32.as<float>();
	timer.mark(st, 0);
	m.fused_kernel(st, ws, loss_pass(B, input, target, gsum), false, true);
	timer.mark(st, 1);
	if (run_optimizer) ++adam_step;
	GridBwdEpilogue ep{};
	ep.enabled = 1;
	ep.apply_adam = run_optimizer ? 1 : 0;
	ep.adam_mlp = run_optimizer ? adam_args_table(st, adam_step) : adam_args();
	ep.adam_mlp.n = (uint32_t)n_mlp;
	ep.buf = AdamBuffers{w32.as<float>(), w16.as<_Float16>(), gsum, g16.as<_Float16>(), m1.as<float>(), m2.as<float>(),
	                     steps.as<uint32_t>()};
	ep.n_mlp_groups = mlp_tail_groups();
	ep.n_mlp = (uint32_t)n_mlp;
	ep.d_loss = d_loss.as<float>();
	TCNN_CHECK(n_mlp % 4 == 0, "network parameter count must be a multiple of 4");
	m.grid_backward(st, ws, B, input, &ep);
	GridEncodingHost& g = *m.grid;
	if (run_optimizer) {
		// binned levels: Adam applied by the accumulate pass; LDS levels: Adam summing their slabs
		GridAccAdam ga{};
		ga.a = adam_args_table(st, adam_step);
		ga.buf = ep.buf;
		ga.param_base = (uint32_t)n_mlp;
		ga.write_grad32 = 0;  // the fp16 gradients (reference m_param_gradients) are written; the fp32 sums are not needed
		g.backward_acc(st, ws.gbw, B, ws.dLdenc.p, 0, 0, g32.as<float>() + n_mlp, &ga);
		timer.mark(st, 2);
		AdamArgs ag = adam_args_table(st, adam_step);
		ag.n = (uint32_t)n_mlp + g.n_lds_params;
		ag.begin = (uint32_t)n_mlp;
		ag.part = ws.gbw.partial.as<float>();
		ag.n_parts = ws.gbw.n_chunks;
		ag.part_stride = g.n_lds_params;
		ag.part_map = g.slab_map(ws.gbw.plan);
		// nothing in the step reads the grid range of g32 / g16, and blocks of parameters that were all
		// hit share one step count: both are settled when somebody asks (lean_settle)
		ag.lean = lean_mask();
		ag.step_blocks = step_blocks.as<uint32_t>();
		TCNN_CHECK(steps_current || (ag.lean & ADAM_LEAN_STEPS), "training step: block step counts were not expanded");
		if (!g.plans[0].slices.empty())
			launch_adam(st, ag, w32.as<float>(), w16.p, g32.as<float>(), g16.p, m1.as<float>(), m2.as<float>(), steps.as<uint32_t>());
		lean_note_step(st, ag.lean);
	} else {
		g.backward_acc(st, ws.gbw, B, ws.dLdenc.p, 0, 0, gsum + n_mlp);
		timer.mark(st, 2);
		g.reduce_items(st, ws.gbw, gsum + n_mlp);
	}
	timer.mark(st, 3);
	last_B = B;
}

// Captured step graphs, keyed by everything the step's kernels read (graph_key); a few are kept so
// a caller cycling through a handful of batch buffers replays one graph per buffer.
struct TrainerHost::StepGraph {
	static constexpr size_t MAX_GRAPHS = 8;
	hipStream_t cs = nullptr;  // capture / replay stream (the caller's may be the legacy null stream)
	hipEvent_t e0 = nullptr, e1 = nullptr;
	std::vector<std::pair<std::vector<uint64_t>, hipGraphExec_t>> execs;  // most recently used last
	StepGraph() {
		TCNN_HIP_CHECK(hipStreamCreateWithFlags(&cs, hipStreamNonBlocking));
		TCNN_HIP_CHECK(hipEventCreateWithFlags(&e0, hipEventDisableTiming));
		TCNN_HIP_CHECK(hipEventCreateWithFlags(&e1, hipEventDisableTiming));
	}
	~StepGraph() {
		for (auto& e : execs) (void)hipGraphExecDestroy(e.second);
		(void)hipEventDestroy(e0);
		(void)hipEventDestroy(e1);
		(void)hipStreamDestroy(cs);
	}
	hipGraphExec_t find(const std::vector<uint64_t>& key) {
		for (size_t i = 0; i < execs.size(); ++i)
			if (execs[i].first == key) {
				auto e = execs[i];
				execs.erase(execs.begin() + i);
				execs.push_back(e);
				return e.second;
			}
		return nullptr;
	}
};

TrainerHost::~TrainerHost() {
	if (graph) (void)hipDeviceSynchronize();  // replays may still run on the graph's stream
}

void TrainerHost::set_graph(bool on) {
	if (!on && graph) {
		TCNN_HIP_CHECK(hipDeviceSynchronize());  // replays run on the callers' streams
		graph.reset();
	}
	use_graph = on;
}

std::vector<uint64_t> TrainerHost::graph_key(uint32_t B, const float* input, const float* target) const {
	std::vector<uint64_t> k = {B, (uint64_t)(uintptr_t)input, (uint64_t)(uintptr_t)target, (uint64_t)ftable_valid,
	                           (uint64_t)(uintptr_t)w32.p, (uint64_t)(uintptr_t)w16.p, (uint64_t)(uintptr_t)g16.p,
	                           (uint64_t)(uintptr_t)g32.p, (uint64_t)(uintptr_t)m1.p, (uint64_t)(uintptr_t)m2.p,
	                           (uint64_t)(uintptr_t)steps.p, (uint64_t)(uintptr_t)d_loss.p, (uint64_t)(uintptr_t)d_ftable.p,
	                           (uint64_t)(uintptr_t)ws.dLdenc.p, (uint64_t)(uintptr_t)ws.dy_bound.p, (uint64_t)(uintptr_t)ws.wgrad_partial.p,
	                           (uint64_t)(uintptr_t)ws.loss_partial.p, (uint64_t)(uintptr_t)ws.wimage.p,
	                           (uint64_t)(uintptr_t)ws.gbw.partial.p, (uint64_t)(uintptr_t)ws.gbw.recs.p,
	                           (uint64_t)(uintptr_t)ws.gbw.dir.p, (uint64_t)(uintptr_t)ws.gbw.dysum.p, ws.n_fused_blocks,
	                           ws.gbw.n_chunks, (uint64_t)overlapped_ok(), (uint64_t)(uintptr_t)dp, (uint64_t)dp_sharded, dp_per,
	                           (uint64_t)(uintptr_t)ws.enc16.p, (uint64_t)(uintptr_t)ws.acts.p, (uint64_t)(uintptr_t)ws.delta0.p,
	                           (uint64_t)(uintptr_t)ws.delta1.p, (uint64_t)(uintptr_t)ws.dout16.p, (uint64_t)(uintptr_t)ws.out16.p,
	                           (uint64_t)(uintptr_t)ws.red_tmp.p, (uint64_t)(uintptr_t)ws.tile_wT.p, (uint64_t)(uintptr_t)ws.loss_sum.p,
	                           ws.n_loss_partials, (uint64_t)(uintptr_t)peer.get(), (uint64_t)peer_attached,
	                           // which k_adam variant the capture holds (the sticky switches re-capture)
	                           (uint64_t)lean_mask(), (uint64_t)(uintptr_t)step_blocks.p};
	// every scalar the step's kernels take from the trainer (AdamArgs holds no pointer here)
	const AdamArgs a = adam_args();
	const size_t n = sizeof(AdamArgs) / 8 + 1;
	std::vector<uint64_t> ab(n, 0);
	std::memcpy(ab.data(), &a, sizeof(AdamArgs));
	k.insert(k.end(), ab.begin(), ab.end());
	const GridOpts o = model->grid ? model->grid->opts() : GridOpts{};  // OneBlob / Identity encodings: no grid
	uint32_t ml = 0;
	std::memcpy(&ml, &o.max_level, 4);
	k.insert(k.end(), {(uint64_t)ml, (uint64_t)(uintptr_t)o.max_level_gpu, o.stochastic, o.n_features, o.active, o.inrange_index});
	uint32_t ls = 0, gs = 0;
	std::memcpy(&ls, &loss_scale, 4);
	std::memcpy(&gs, &grad_scale, 4);
	k.insert(k.end(), {(uint64_t)ls, (uint64_t)gs});
	return k;
}

bool TrainerHost::training_step_graph(hipStream_t st, uint32_t B, const float* input, const float* target) {
	// the single-GPU fused step's first step builds the weight image eagerly (the replays then read it)
	const bool image_step = overlapped_ok() && !dp && !peer_attached;
	if (adam_step + 1 >= GRAPH_STEPS || (image_step && !ws.wimage_valid)) return false;
	if (peer_attached) peer_check();
	if (ftable_valid < GRAPH_STEPS || ftable_b1 != adam.beta1 || ftable_b2 != adam.beta2)
		(void)adam_args_table(st, GRAPH_STEPS, GRAPH_STEPS);
	if (!graph) graph = std::make_unique<StepGraph>();
	std::vector<uint64_t> key = graph_key(B, input, target);
	hipGraphExec_t exec = graph->find(key);
	if (!exec) {
		// eager step first (sizes every workspace for this B, so the capture allocates nothing)
		step_eager(st, B, input, target);
		key = graph_key(B, input, target);
		TCNN_HIP_CHECK(hipStreamSynchronize(st));
		TCNN_HIP_CHECK(hipStreamSynchronize(graph->cs));
		if (graph->execs.size() >= StepGraph::MAX_GRAPHS) {
			(void)hipGraphExecDestroy(graph->execs.front().second);
			graph->execs.erase(graph->execs.begin());
		}
		const uint32_t step0 = adam_step, ftv0 = ftable_valid, lb0 = last_B;
		const bool wv0 = ws.wimage_valid, dps0 = dp_state_partial;
		const bool gst0 = grads_stale, sc0 = steps_current, sbd0 = step_blocks_diverged;
		const float sgs0 = stale_grad_scale;
		hipStream_t const lst0 = lean_st;
		hipGraph_t g = nullptr;
		const bool tim = timer.enabled;
		timer.enabled = false;  // no phase events inside the graph
		TCNN_HIP_CHECK(hipStreamBeginCapture(graph->cs, hipStreamCaptureModeThreadLocal));
		step_eager(graph->cs, B, input, target);
		TCNN_HIP_CHECK(hipStreamEndCapture(graph->cs, &g));
		timer.enabled = tim;
		adam_step = step0;  // the capture ran nothing
		ftable_valid = ftv0;
		last_B = lb0;
		ws.wimage_valid = wv0;
		dp_state_partial = dps0;
		grads_stale = gst0;
		steps_current = sc0;
		step_blocks_diverged = sbd0;
		stale_grad_scale = sgs0;
		lean_st = lst0;
		hipGraphExec_t e = nullptr;
		const hipError_t err = hipGraphInstantiate(&e, g, nullptr, nullptr, 0);
		(void)hipGraphDestroy(g);
		TCNN_HIP_CHECK(err);
		graph->execs.emplace_back(key, e);
		++graph_captures;
		return true;
	}
	// replayed straight on the caller's stream (the legacy null stream included): no private stream,
	// no event joins -- captured on graph->cs only because a capture needs a non-null stream
	TCNN_HIP_CHECK(hipGraphLaunch(exec, st));
	// the host-side effects of the eager step
	++adam_step;
	ws.wimage_valid = image_step;  // the data-parallel steps leave the weight image to be rebuilt by the next step
	if ((dp && dp_sharded) || peer_attached) dp_state_partial = true;
	if (image_step) lean_note_step(st, lean_mask());  // the captured k_adam is the key's variant
	last_B = B;
	++graph_replays;
	return true;
}

hipEvent_t PhaseTimer::get() {
	if (next == pool.size()) {
		hipEvent_t e;
		TCNN_HIP_CHECK(hipEventCreate(&e));
		pool.push_back(e);
	}
	return pool[next++];
}

PhaseTimer::~PhaseTimer() {
	for (auto e : pool) (void)hipEventDestroy(e);
}

void PhaseTimer::mark(hipStream_t st, int phase) {
	if (!enabled || !sampling || marks.empty()) return;
	const int idx = (int)next;
	TCNN_HIP_CHECK(hipEventRecord(get(), st));
	marks.back()[phase] = idx;
}

void TrainerHost::profile_end(double* ms, uint32_t n_phases, uint32_t* n_steps) {
	TCNN_HIP_CHECK(hipDeviceSynchronize());
	const uint32_t P = std::min<uint32_t>(n_phases, PhaseTimer::N_PHASES);
	for (uint32_t p = 0; p < n_phases; ++p) ms[p] = 0.0;
	std::vector<uint32_t> cnt(P, 0);
	for (auto& m : timer.marks) {
		for (uint32_t p = 0; p < P; ++p) {
			if (m[p] < 0 || m[p + 1] < 0) continue;
			float t = 0.0f;
			TCNN_HIP_CHECK(hipEventElapsedTime(&t, timer.pool[m[p]], timer.pool[m[p + 1]]));
			ms[p] += t;
			++cnt[p];
		}
	}
	for (uint32_t p = 0; p < P; ++p)
		if (cnt[p]) ms[p] /= cnt[p];
	if (n_steps) *n_steps = P ? cnt[0] : 0;
	timer.enabled = false;
	timer.reset();
}

AdamArgs TrainerHost::adam_args() const {
	AdamArgs a{};
	a.n = (uint32_t)n_params;
	a.n_matrix = (uint32_t)n_mlp;  // layer_sizes() of the network only (grid.h:1084-1088)
	a.loss_scale = loss_scale;
	a.grad_scale = grad_scale;
	a.lr = adam.learning_rate;
	a.beta1 = adam.beta1;
	a.beta2 = adam.beta2;
	a.eps = adam.epsilon;
	a.l2_reg = adam.l2_reg;
	a.rel_decay = adam.relative_decay;
	a.abs_decay = adam.absolute_decay;
	a.clip = adam.clipping_magnitude;
	a.nonmat_lr_factor = adam.non_matrix_learning_rate_factor;
	a.lower_lr_bound = 0.0f;
	a.upper_lr_bound = std::numeric_limits<float>::max();
	if (adam.adabound) {
		a.lower_lr_bound = 0.1f - 0.1f / ((1 - adam.beta2) * (float)adam_step + 1);
		a.upper_lr_bound = 0.1f + 0.1f / ((1 - adam.beta2) * (float)adam_step);
	}
	a.opt_matrix = adam.optimize_matrix_params;
	a.opt_nonmatrix = adam.optimize_non_matrix_params;
	int e = 0;
	a.inv_loss_scale = (std::frexp(loss_scale, &e) == 0.5f) ? 1.0f / loss_scale : 0.0f;  // exact for powers of two
	return a;
}

// Data-parallel step in two parts, so the caller can all-reduce the network gradients while the
// grid backward runs (fused_gradient_half). Same kernels and summation orders as
// training_step(run_optimizer = false). The tile and layer-wise engines do their whole pass in part 0.
void TrainerHost::training_step_part(hipStream_t st, uint32_t B, const float* input, const float* target, int part) {
	TCNN_CHECK(B % BATCH_GRANULARITY == 0, "training_step: batch size must be a multiple of 256");
	TCNN_CHECK(part == 0 || part == 1, "training_step_part: part must be 0 or 1");
	lean_settle(LeanUse::Write);
	if (!overlapped_ok()) {
		if (part == 0) training_step(st, B, input, target, false);
		return;
	}
	TCNN_CHECK(part == 0 || last_B == B, "training_step_part: part 1 must follow part 0 of the same batch");
	fused_gradient_half(st, B, input, target, part);
}

void TrainerHost::fused_gradient_half(hipStream_t st, uint32_t B, const float* input, const float* target, int half) {
	NetworkHost& m = *model;
	float* g = g32.as<float>();
	if (half == 0) {
		m.fused_kernel(st, ws, loss_pass(B, input, target, g), false, true);
		launch_column_sums(st, ws.wgrad_partial.as<float>(), ws.n_fused_blocks, (uint32_t)n_mlp, g);
		launch_sum(st, ws.loss_partial.as<float>(), ws.n_loss_partials, d_loss.as<float>());
		last_B = B;
		return;
	}
	m.grid_backward(st, ws, B, input);
	m.grid->backward_acc(st, ws.gbw, B, ws.dLdenc.p, 0, 0, g + n_mlp);
	m.grid->reduce_items(st, ws.gbw, g + n_mlp);
}

AdamArgs TrainerHost::adam_args_table(hipStream_t st, uint32_t upto, uint32_t reserve) {
	AdamArgs a = adam_args();
	if (ftable_b1 != adam.beta1 || ftable_b2 != adam.beta2) {  // hyper-parameters changed: recompute all
		ftable_valid = 0;
		ftable_b1 = adam.beta1;
		ftable_b2 = adam.beta2;
	}
	if (std::max(upto, reserve) > ftable_cap) {
		ftable_cap = std::max((std::max(upto, reserve) + 1023u) / 1024u * 1024u, std::max(1024u, 2 * ftable_cap));
		TCNN_HIP_CHECK(hipStreamSynchronize(st));  // the old table may still be read by queued work
		d_ftable.reserve((size_t)ftable_cap * 4);
		ftable_valid = 0;
	}
	if (std::max(upto, reserve) > ftable_valid) {
		// the factors depend only on t and the betas, sqrt(1 - b2^t) / (1 - b1^t) (adam.h:110-113),
		// computed 1024 steps ahead on the host with the C library's powf / sqrtf -- one libm for
		// every step, the same one the CPU restatement uses, so the Adam update is bit-exact against it
		// (a device powf differs from glibc's in the last bit for some t)
		const uint32_t ahead = std::min(ftable_cap, (std::max(upto, reserve) + 1023u) / 1024u * 1024u);
		h_ftable.resize(ahead);
		for (uint32_t t = ftable_valid + 1; t <= ahead; ++t)
			h_ftable[t - 1] = std::sqrt(1.0f - std::pow(adam.beta2, (float)t)) / (1.0f - std::pow(adam.beta1, (float)t));
		TCNN_HIP_CHECK(hipMemcpyAsync(d_ftable.as<float>() + ftable_valid, h_ftable.data() + ftable_valid, (size_t)(ahead - ftable_valid) * 4,
		                              hipMemcpyHostToDevice, st));
		TCNN_HIP_CHECK(hipStreamSynchronize(st));  // h_ftable may grow (reallocate) before the next fill
		ftable_valid = ahead;
	}
	a.factor_table = d_ftable.as<float>();
	a.factor_n = ftable_valid;
	return a;
}

void TrainerHost::optimizer_step(hipStream_t st) {
	lean_settle(LeanUse::Write);  // the gradients of a one-call step, and per-parameter counts for adam_apply
	if (opt) {  // the tree on the gradient buffers: the fp16 gradients first (Adam's own rounding of the sums)
		launch_grad_f16(st, g32.as<float>(), g16.p, grad_scale, n_params);
		OptStep s;
		s.st = st;
		s.g32 = g32.as<float>();
		s.gscale = grad_scale;
		s.g16 = g16.p;
		opt_step(*opt, s);
		return;
	}
	adam_apply(st, g32.as<float>(), grad_scale, g16.p);
}

// ---- lean Adam over the grid slabs: what the one-call step leaves undone, settled on request ----
uint32_t TrainerHost::n_step_blocks() const {
	return model->grid ? div_round_up(model->grid->n_lds_params, ADAM_STEP_BLOCK) : 0u;
}

uint32_t TrainerHost::lean_mask() const {
	if (opt || dp || peer_attached || !overlapped_ok() || !model->grid || model->grid->plans[0].slices.empty()) return 0;
	uint32_t m = adam_lean;
	if (grads_eager) m &= ~ADAM_LEAN_GRADS;
	if (steps_per_param) m &= ~ADAM_LEAN_STEPS;
	return m;
}

void TrainerHost::lean_note_step(hipStream_t st, uint32_t lean) {
	lean_st = st;
	grads_stale = (lean & ADAM_LEAN_GRADS) != 0;
	stale_grad_scale = grad_scale;
	if (lean & ADAM_LEAN_STEPS) {
		steps_current = false;
		step_blocks_diverged = false;
	}
}

// g32 / g16 of the grid range from the last step's slabs, which nothing has overwritten since (every
// backward settles first): plan, chunk count and slab buffer are still the step's in ws.gbw
void TrainerHost::grads_materialize() {
	if (!grads_stale) return;
	const GridEncodingHost& g = *model->grid;
	launch_grid_slab_gradients(lean_st, ws.gbw.partial.as<float>(), ws.gbw.n_chunks, g.n_lds_params, g.n_lds_params, g.slab_map(ws.gbw.plan),
	                           stale_grad_scale, g32.as<float>() + n_mlp, g16.as<_Float16>() + n_mlp);
	grads_stale = false;
}

void TrainerHost::steps_expand(LeanUse use) {
	if (!n_step_blocks()) return;
	if (!steps_current) {
		launch_adam_steps_expand(lean_st, step_blocks.as<uint32_t>(), model->grid->n_lds_params, steps.as<uint32_t>() + n_mlp);
		steps_current = true;
	}
	if (use != LeanUse::Read && !step_blocks_diverged) {
		TCNN_HIP_CHECK(hipMemsetAsync(step_blocks.p, 0xFF, (size_t)n_step_blocks() * 4, lean_st));
		step_blocks_diverged = true;
	}
}

void TrainerHost::lean_settle(LeanUse use) {
	grads_materialize();
	steps_expand(use);
	if (use == LeanUse::Caller) grads_eager = steps_per_param = true;
}

uint32_t TrainerHost::uniform_step_blocks() {
	const uint32_t n = n_step_blocks();
	if (!n) return 0;
	std::vector<uint32_t> h(n);
	TCNN_HIP_CHECK(hipStreamSynchronize(lean_st));
	TCNN_HIP_CHECK(hipMemcpy(h.data(), step_blocks.p, (size_t)n * 4, hipMemcpyDeviceToHost));
	uint32_t u = 0;
	for (uint32_t w : h) u += w != ADAM_STEPS_DIVERGED ? 1u : 0u;
	return u;
}

std::unique_ptr<TrainerFwdCtx> TrainerHost::forward(hipStream_t st, uint32_t B, const float* input, const float* target, const float* pdf,
                                                    const void* ext_dLdy16, bool prep_dinput, const float* perturbation,
                                                    bool use_inference_params) {
	TCNN_CHECK(B % BATCH_GRANULARITY == 0, "forward: batch size must be a multiple of 256");
	TCNN_CHECK(ext_dLdy16 || target, "forward: a target (or an external dL/dy) is required");
	NetworkHost& m = *model;
	const uint32_t OUTP = m.mlp.padded_output;
	auto c = std::make_unique<TrainerFwdCtx>();
	c->B = B;
	c->out16.reserve((size_t)B * OUTP * 2);
	// use_inference_params (trainer.h:97-112): the forward and its loss on the optimizer's custom weights
	const void* params16 = use_inference_params ? params_inference() : w16.p;
	c->inference_params = params16 != w16.p;
	c->layout = m.forward_keep(st, ws, B, input, params16, c->out16.p, prep_dinput, c->keep);
	if (ext_dLdy16) {  // trainer.h:126-130: the caller's dL/dy replaces the loss
		c->ext = ext_dLdy16;
	} else {
		c->dLdy16.reserve((size_t)B * OUTP * 2);
		c->n_lpart = relative_l2_n_blocks(B, OUTP);
		c->lpart.reserve((size_t)c->n_lpart * 4);
		const void* loss_in = c->out16.p;
		if (perturbation) {  // trainer.h:114-123: the loss (and its dL/dy) on the perturbed output
			c->pert16.reserve((size_t)B * OUTP * 2);
			launch_add_perturbation(st, B * OUTP, c->out16.p, perturbation, c->pert16.p);
			loss_in = c->pert16.p;
		}
		launch_relative_l2_partial(st, B, OUTP, n_output_dims, loss_scale, loss_in, target, c->dLdy16.p, c->lpart.as<float>(),
		                           m.loss_type, pdf);
	}
	ws.wimage_valid = false;  // forward_keep may have packed the image in place
	return c;
}

void TrainerHost::backward(hipStream_t st, const TrainerFwdCtx& c, uint32_t B, const float* input, float* dL_dinput, int gradient_mode) {
	TCNN_CHECK(B == c.B, "backward: batch size differs from the forward's");
	lean_settle(LeanUse::Write);  // Accumulate adds to g32; the backward overwrites the slabs
	TCNN_CHECK(!c.inference_params,
	           "backward: use_inference_params is honoured by inference and by a forward without a backward only; this context's "
	           "forward read the optimizer's custom weights, and gradients are taken at the training parameters");
	// Accumulate: this backward's gradients into a scratch sum, added afterwards (trainer.h:146-153).
	// Ignore: the same scratch, never added -- the parameter gradients stay as they were and only
	// dL/dinput is delivered (the engine's fused backward computes both in one pass).
	float* dst = g32.as<float>();
	if (gradient_mode != 0) {
		g32_acc.reserve(n_params * 4);
		dst = g32_acc.as<float>();
	}
	TrainPass p;
	p.B = B;
	p.pos = input;
	p.params16 = w16.p;
	p.dims = n_output_dims;
	p.dout16 = c.dLdy();
	p.grad32 = dst;
	p.dL_dinput = dL_dinput;
	p.kept = c.keep.p;
	p.kept_layout = c.layout;
	model->fwd_bwd(st, ws, p);
	if (gradient_mode == 1) launch_add_f32(st, dst, g32.as<float>(), n_params);
	ws.wimage_valid = false;
	last_B = B;
}

float TrainerHost::ctx_loss(hipStream_t st, const TrainerFwdCtx& c) {  // trainer.h:205-211
	if (c.ext) return 0.0f;  // no loss was evaluated (the reference's L stays unwritten)
	launch_sum(st, c.lpart.as<float>(), c.n_lpart, d_loss.as<float>());
	return loss(st);
}

void TrainerHost::optimizer_step_range(hipStream_t st, uint64_t begin, uint64_t end) {
	require_plain_adam("optimizer_step_range");
	lean_settle(LeanUse::Write);
	TCNN_CHECK(begin <= end && end <= n_params, "optimizer_step_range: range outside the parameter vector");
	++adam_step;
	AdamArgs a = adam_args_table(st, adam_step);
	a.begin = (uint32_t)begin;
	a.n = (uint32_t)end;
	launch_adam(st, a, w32.as<float>(), w16.p, g32.as<float>(), g16.p, m1.as<float>(), m2.as<float>(), steps.as<uint32_t>());
	ws.wimage_valid = false;
}

float TrainerHost::loss(hipStream_t st) {
	float v = 0.0f;
	TCNN_HIP_CHECK(hipMemcpyAsync(&v, d_loss.p, 4, hipMemcpyDeviceToHost, st));
	TCNN_HIP_CHECK(hipStreamSynchronize(st));
	return v;
}

void TrainerHost::inference(hipStream_t st, uint32_t B, const float* input, float* out) {
	const uint32_t OUTP = model->mlp.padded_output;
	ws.out16.reserve((size_t)B * OUTP * 2);
	// the inference parameters (trainer.h:330-335); the weight image tracks the training parameters only
	const void* p = params_inference();
	model->inference(st, ws, B, input, p, ws.out16.p, /*trust_image=*/p == w16.p);
	launch_trim_cast(st, B, OUTP, n_output_dims, ws.out16.p, out);
}

}  // namespace tcnn_amd
