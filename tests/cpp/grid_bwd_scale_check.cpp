// grid_bwd_scale_check.cpp -- host check of csrc/grid_bwd_scale.h: over random multisets of fp16
// magnitudes it emulates, in fp32, the two orders in which the grid backward sums a chunk's
// max_f |dL/dy| -- the exact pre-pass and the streaming path's slice sums (grid_bwd_lds.h,
// mlp_fused.h) -- and checks that whenever grid_bwd_scale_guard accepts the streaming sum, its exponent
// equals the exact one, and that the guard rejects fewer than 1 % of uniformly random cases.
// Prints "cases N accepted A rejected R mismatches M uniform_cases U uniform_rejected V"; exit 0 iff
// M == 0 and V < 1 % of U.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../neuralbtf-tiny-cuda-nn_amd/csrc/grid_bwd_scale.h"

using namespace tcnn_amd;

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {  // splitmix64
	uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
	z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
	z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
	return (uint32_t)((z ^ (z >> 31)) >> 16);
}

// a non-negative finite fp16 bit pattern (<= 0x7bff) as float, exactly
static float h2f(uint32_t h) {
	const uint32_t ex = h >> 10, mant = h & 0x3ffu;
	if (ex == 0) return (float)mant * (1.0f / 16777216.0f);  // denormal: mant * 2^-24
	uint32_t b = ((ex + 112u) << 23) | (mant << 13);
	float f;
	memcpy(&f, &b, 4);
	return f;
}

// the exact pre-pass: thread t sums its points t, t + 1024, ... in order (32 slots, absent ones 0),
// 6-step xor butterfly over the 64 lanes of a wave, the 16 wave sums added in order
static float butterfly_red(const float* per_thread) {
	float red[16];
	for (int w = 0; w < 16; ++w) {
		float v[64];
		for (int l = 0; l < 64; ++l) v[l] = per_thread[64 * w + l];
		for (int o = 32; o > 0; o >>= 1) {
			float n[64];
			for (int l = 0; l < 64; ++l) n[l] = v[l] + v[l ^ o];
			memcpy(v, n, sizeof v);
		}
		red[w] = v[0];
	}
	float m = red[0];
	for (int w = 1; w < 16; ++w) m += red[w];
	return m;
}

static float sum_exact(const std::vector<float>& s) {
	static float th[1024];
	const size_t n = s.size();
	for (size_t t = 0; t < 1024; ++t) {
		float m = 0.0f;
		for (size_t p = 0; p < 32; ++p) {
			const size_t i = t + p * 1024;
			m += i < n ? s[i] : 0.0f;
		}
		th[t] = m;
	}
	return butterfly_red(th);
}

// the streaming path: per 32-point slice, lane c adds its samples c and 16 + c, then a balanced tree
// over the 16 lanes (pairs, quads, half rows, the row); thread t of the grid backward takes slice t
static float sum_stream(const std::vector<float>& s) {
	static float th[1024];
	const size_t ns = s.size() / 32;
	for (size_t t = 0; t < 1024; ++t) {
		if (t >= ns) { th[t] = 0.0f; continue; }
		float v[16];
		for (int c = 0; c < 16; ++c) v[c] = s[32 * t + c] + s[32 * t + 16 + c];
		static const int perm[4][16] = {
			{1, 0, 3, 2, 5, 4, 7, 6, 9, 8, 11, 10, 13, 12, 15, 14},   // quad_perm [1, 0, 3, 2]
			{2, 3, 0, 1, 6, 7, 4, 5, 10, 11, 8, 9, 14, 15, 12, 13},   // quad_perm [2, 3, 0, 1]
			{7, 6, 5, 4, 3, 2, 1, 0, 15, 14, 13, 12, 11, 10, 9, 8},   // row_half_mirror
			{15, 14, 13, 12, 11, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1, 0}};  // row_mirror
		for (int st = 0; st < 4; ++st) {
			float n[16];
			for (int c = 0; c < 16; ++c) n[c] = v[c] + v[perm[st][c]];
			memcpy(v, n, sizeof v);
		}
		th[t] = v[0];
	}
	return butterfly_red(th);
}

int main(int argc, char** argv) {
	const int rounds = argc > 1 ? atoi(argv[1]) : 300;
	static const uint32_t sizes[] = {32, 64, 256, 1024, 4096, 8224, 16384, 32768};
	uint64_t cases = 0, accepted = 0, rejected = 0, mismatches = 0, uni = 0, uni_rej = 0;
	std::vector<float> s;
	for (int r = 0; r < rounds; ++r) {
		for (uint32_t n : sizes) {
			for (int kind = 0; kind < 5; ++kind) {
				s.assign(n, 0.0f);
				// 0 uniform random fp16 bit patterns (log-uniform magnitudes, denormals included)
				// 1 a narrow random exponent band (gradient-like)   2 sparse: ~1 in 64 non-zero
				// 3 one large outlier over small values              4 denormals only
				const uint32_t band = 1 + rnd() % 26, top = (band + 4) << 10;
				for (uint32_t i = 0; i < n; ++i) {
					uint32_t h;
					switch (kind) {
						case 0: h = rnd() % 0x7c00u; break;
						case 1: h = (band << 10) + rnd() % (4u << 10); if (h >= top) h = top - 1; break;
						case 2: h = (rnd() % 64 == 0) ? rnd() % 0x7c00u : 0u; break;
						case 3: h = rnd() % 0x0c00u; break;
						default: h = rnd() % 0x0400u; break;
					}
					s[i] = h2f(h);
				}
				if (kind == 3) s[rnd() % n] = h2f(0x7800u + rnd() % 0x3ffu);
				const float P = (float)n;
				const float m = sum_exact(s), mh = sum_stream(s);
				const bool ok = grid_bwd_scale_guard(mh, P, 2);
				++cases;
				if (kind == 0) ++uni;
				if (ok) {
					++accepted;
					if (grid_bwd_scale_exp(mh, P, 2) != grid_bwd_scale_exp(m, P, 2)) {
						++mismatches;
						fprintf(stderr, "mismatch: n %u kind %d m %.9g mh %.9g\n", n, kind, m, mh);
					}
				} else {
					++rejected;
					if (kind == 0) ++uni_rej;
				}
			}
		}
	}
	// sums placed on purpose at binade edges of lim: the guard must reject or agree there too
	for (int k = 0; k < 20000; ++k) {
		const float P = (float)sizes[rnd() % 8];
		float x = ldexpf(1.0f, (int)(rnd() % 40) - 20);
		x = grid_bwd_scale_lim(x, P, 2);  // m with lim(m) near a power of two: m ~ C / (1.01 2^j)
		uint32_t b;
		memcpy(&b, &x, 4);
		b += (rnd() % 4097) - 2048;  // around the band (2^-14 relative = 512 .. 1024 ulps)
		float mh;
		memcpy(&mh, &b, 4);
		b += (rnd() % 181) - 90;  // an "exact" sum up to 90 ulps (>= 90 u, beyond the derived 87 u) from it
		float m;
		memcpy(&m, &b, 4);
		++cases;
		if (grid_bwd_scale_guard(mh, P, 2)) {
			++accepted;
			if (grid_bwd_scale_exp(mh, P, 2) != grid_bwd_scale_exp(m, P, 2)) ++mismatches;
		} else {
			++rejected;
		}
	}
	// degenerate sums
	if (!grid_bwd_scale_guard(0.0f, 32.0f, 2) || grid_bwd_scale_exp(0.0f, 32.0f, 2) != 0) ++mismatches;
	if (grid_bwd_scale_guard(__builtin_inff(), 32.0f, 2) || grid_bwd_scale_guard(__builtin_nanf(""), 32.0f, 2)) ++mismatches;
	printf("cases %llu accepted %llu rejected %llu mismatches %llu uniform_cases %llu uniform_rejected %llu\n",
	       (unsigned long long)cases, (unsigned long long)accepted, (unsigned long long)rejected, (unsigned long long)mismatches,
	       (unsigned long long)uni, (unsigned long long)uni_rej);
	return (mismatches == 0 && uni_rej * 100 < uni) ? 0 : 1;
}
