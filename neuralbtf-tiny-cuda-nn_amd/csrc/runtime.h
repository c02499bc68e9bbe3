// runtime.h -- host-side objects of the engine: JSON config -> grid encoding / fused MLP /
// NetworkWithInputEncoding / Trainer, device buffers, workspace. The C-ABI (capi.cpp) and the
// C++ template API (include/tiny-cuda-nn/*.h) are thin layers over these classes.
#pragma once

#include <json.hpp>

#include <array>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "common.h"
#include "grid_device.h"
#include "kernels.h"
#include "optimizer_tree.h"
#include "wt_store.h"

namespace tcnn_amd {

using json = nlohmann::json;

// ---- host PCG32 (same stream semantics as the reference's dependencies/pcg32/pcg32.h) ----
struct Pcg32 {
	uint64_t state = 0x853c49e6748fea9bULL, inc = 0xda3e39cb94b95bdbULL;
	Pcg32() = default;
	explicit Pcg32(uint64_t initstate, uint64_t initseq = 1u) { seed(initstate, initseq); }
	void seed(uint64_t initstate, uint64_t initseq = 1u);
	uint32_t next_uint();
	float next_float();
	void advance(int64_t delta);
};

// ---- grow-only device allocation ----
struct DevBuf {
	void* p = nullptr;
	size_t bytes = 0;
	DevBuf() = default;
	DevBuf(const DevBuf&) = delete;
	DevBuf& operator=(const DevBuf&) = delete;
	~DevBuf();
	void reserve(size_t n);  // contents are not preserved
	void release();
	template <typename T> T* as() const { return (T*)p; }
};

bool ieq(const std::string& a, const std::string& b);
// LossType (loss_device.h) of a loss otype, compared case-insensitively; -1: not one of the nine
int loss_type_from_otype(const std::string& otype);
std::string loss_otype_list();  // "L2, RelativeL2, ..." for error messages

// Scratch of one grid backward (grow-only).
struct GridBwdBufs {
	DevBuf partial, recs, dir, dysum;
	uint32_t n_chunks = 0;  // LDS items: point chunks = slabs in `partial`
	int plan = 0;           // the LDS work plan the slabs in `partial` follow (GridEncodingHost::plans)
};
// LDS work plan of the grid backward: items, their device copy, and whether the chunk slabs are in
// parameter order (no GridSlabMap needed to read them)
struct GridPlan {
	std::vector<GridSlice> slices;
	DevBuf d_slices;
	bool identity = true;
	GridPlan() = default;
	GridPlan& operator=(const GridPlan& o) {
		slices = o.slices;
		identity = o.identity;
		return *this;
	}
};
enum : int { PLAN_RANGE = 0, PLAN_FEATURE = 1 };

// ---- multiresolution grid (reference encodings/grid.h:652-1208) ----
// The engine's A/B and tuning switches (TCNN_* environment variables). Read once when an engine
// object is built -- never per step -- so an experiment sets them before creating its trainer or
// module. Process-wide debug switches (TCNN_DEBUG_POISON, TCNN_DEBUG_GRID_TIMES, TCNN_TILE_REG_A,
// TCNN_TILE_WG_PER_CU) are read once per process where they are used.
struct EngineSwitches {
	bool no_fused_grid = false;     // TCNN_NO_FUSED_GRID: grid models train on the tile engine
	bool no_tile_engine = false;    // TCNN_NO_TILE_ENGINE: FullyFusedMLP shapes train on the layer-wise engine
	bool no_inrange_index = false;  // TCNN_NO_INRANGE_INDEX: the generic grid index in every kernel
	bool no_forward_keep = false;   // TCNN_NO_FORWARD_KEEP: Module backward recomputes the forward
	bool split_forward = false;     // TCNN_SPLIT_FORWARD: grid forward + k_mlp_infer instead of k_fused_fwd_grid
	bool grid_bin_all = false;      // TCNN_GRID_BIN=all: bin every grid level that does not fit whole
	uint32_t grid_bwd_chunks = 0;   // TCNN_GRID_BWD_CHUNKS: grid backward point chunks (0: automatic)
	uint32_t grid_bwd_ranges = 0;   // TCNN_GRID_BWD_RANGES: at least this many entry ranges per hashed level (tuning)
	int grid_bwd_plan = -1;         // TCNN_GRID_BWD_PLAN=range|feature: force one work plan (A/B; -1: by batch)
	bool no_grid_bwd_stream = false;  // TCNN_GRID_BWD_STREAM=0: no dy_bound from the fused kernel, exact pre-pass everywhere (A/B)
	// TCNN_WT_STORES=<mask>: the training step's hand-off stores that write through L2 (wt_store.h:
	// WT_WGRAD_SLAB 1, WT_GRID_SLAB 2); 0: all plain (A/B). Results do not depend on it.
	uint32_t wt_stores = WT_STORES_DEFAULT;
	// TCNN_ADAM_LEAN=<mask>: what the trainer's Adam over the grid slabs leaves out of its traffic
	// (kernels.h: ADAM_LEAN_GRADS 1 the gradient stores, produced when a caller asks; ADAM_LEAN_STEPS 2
	// per-parameter step counts of blocks that agree, off by default: measured slower); 0: every store and
	// count (A/B). Results do not depend on it.
	uint32_t adam_lean = ADAM_LEAN_DEFAULT;
	static EngineSwitches from_env();
};

struct GridEncodingHost {
	EngineSwitches sw = EngineSwitches::from_env();
	GridDesc desc{};
	uint32_t n_features = 0;     // L * F
	uint32_t n_to_pad = 0;       // alignment padding (reference set_padded_output_width)
	uint32_t n_params = 0;       // offset[L] * F
	bool stochastic = false;
	float max_level = 1000.0f;              // GridEncoding::set_max_level (grid_interface.h:101-107)
	const float* max_level_gpu = nullptr;   // set_max_level_gpu: [B] per point (grid_interface.h:109-123)
	std::vector<LevelInfo> levels;
	// backward plan: levels [0, first_binned) are LDS work items (`slices`, per-chunk slabs), levels
	// [first_binned, L) go through the binned backward (grid_bin.hip), one slot each
	GridPlan plans[2];  // PLAN_RANGE, PLAN_FEATURE (ctor); both have the same items when no level splits
	uint32_t first_binned = 0;
	bool inrange_index_ok = false;  // grid_index_inrange is exact for in-range positions (ctor)
	uint32_t n_lds_params = 0;  // offset[first_binned] * F
	std::vector<GridBinLevel> bin_levels;
	uint32_t n_buckets = 0, acc_lds_bytes = 0;
	DevBuf d_levels, d_slab_map, d_bin_levels;

	GridEncodingHost(uint32_t n_dims_to_encode, const json& enc);
	uint32_t padded_output_width() const { return n_features + n_to_pad; }
	void set_alignment(uint32_t a) { n_to_pad = (n_features + a - 1) / a * a - n_features; }
	bool hash_grid() const { return desc.grid_type == GridType::Hash; }
	// GridEncodingTemplated::initialize_params (grid.h:1059-1062) -> host fp32
	void initialize_params(Pcg32& rng, float* host_out, float scale = 1.0f) const;
	json hyperparams() const;
	const LevelInfo* dev_levels() const { return d_levels.as<LevelInfo>(); }
	GridOpts opts() const {
		GridOpts o;
		o.max_level = max_level;
		o.max_level_gpu = max_level_gpu;
		o.stochastic = stochastic ? 1u : 0u;
		o.n_features = n_features;
		const float t = (max_level * (float)n_features) / (float)desc.n_features_per_level + 1e-3f;
		o.active = (stochastic || max_level_gpu || (float)(desc.n_levels - 1) >= t) ? 1u : 0u;
		o.inrange_index = (inrange_index_ok && desc.interp == Interp::Linear && !sw.no_inrange_index) ? 1u : 0u;
		return o;
	}
	// this grid as every grid launcher takes it (kernels.h)
	GridCall call() const {
		return GridCall{desc.n_pos_dims, desc.n_features_per_level, desc.n_levels, desc.hash_type, hash_grid(), desc.interp, dev_levels(), opts()};
	}
	// the slabs' element order under a plan; nullptr when it is the parameter order (every LDS item holds
	// all F features of its entries: the readers then index the slabs directly, no dependent map load)
	const GridSlabMap* slab_map(int plan) const { return plans[plan].identity ? nullptr : d_slab_map.as<GridSlabMap>(); }
	// the plan of a launch: TCNN_GRID_BWD_PLAN=range|feature, else the range plan while the items x
	// chunks run in one round on the CUs (2^15 .. 2^18 points), the feature plan beyond (configs[3])
	int plan_for(uint32_t B, uint32_t reserved = 0) const {
		if (sw.grid_bwd_plan >= 0) return sw.grid_bwd_plan;
		const uint32_t n_items = (uint32_t)plans[PLAN_RANGE].slices.size();
		return (uint64_t)bwd_chunks(B, reserved) * n_items + reserved <= 256 ? PLAN_RANGE : PLAN_FEATURE;
	}
	// point chunks of the backward: items x chunks workgroups of 1024 threads (one per CU: 128 KiB
	// of LDS each) fit the CUs left after `reserved` other workgroups in ONE round, with one chunk of
	// slack (config_hash, 26 items + 16 tail workgroups: 7 / 8 / 9 / 10 chunks -> 68.8 / 65.8 /
	// 67.5 / 109 us, the last spilling into a second round); >= 4096 points each
	uint32_t bwd_chunks(uint32_t B, uint32_t reserved = 0) const {
		const std::vector<GridSlice>& slices = plans[PLAN_RANGE].slices;  // (both plans: the same count for F = 2)
		if (slices.empty()) return 1;
		const uint32_t n_cu = 256;
		const uint32_t fit = (n_cu > reserved ? n_cu - reserved : 1u) / (uint32_t)slices.size();
		uint32_t c = std::max(1u, fit > 2 ? fit - 1 : fit);
		// large batches: chunks small enough for the register-resident path, over several rounds
		// (configs[3], 2^20 points: 8 -> 32 chunks, grid backward 170 -> 99 us, step -4 %,
		// profiles/r04_grid_bwd_chunks.txt); config_hash at 2^18 keeps its 8
		c = std::max(c, (B + GRID_BWD_REG_POINTS - 1) / GRID_BWD_REG_POINTS);
		if (sw.grid_bwd_chunks) return std::max(1u, std::min(std::min(sw.grid_bwd_chunks, 32u), B / 1024));  // tuning override
		// >= 8192 points per chunk: below that the per-chunk slab (written here, read by Adam or the
		// slab reduction) costs more than the parallelism gains (2^15 points, one rank of N = 8:
		// 4 chunks 46.6 us per step vs 8 chunks 48.0, profiles/r05_chunk_sweep.txt)
		return std::max(1u, std::min(std::min(c, 32u), B / 8192));
	}
	// bin-pass geometry for B points (reserves the record / directory buffers in w)
	GridBinArgs bin_args(GridBwdBufs& w, uint32_t B) const;
	// The backward pieces. dy: dL/d(encoding) fp16 in launch_grid_bwd layout `layout` (stride for AoS).
	//   backward_items  LDS items -> per-chunk slabs in w.partial (+ the trainer's epilogue workgroups)
	//   backward_bin    bin pass of the binned levels
	//   backward_acc    accumulate pass: fp32 gradient of the binned levels into grad32 (grid
	//                   parameter order, whole grid vector) or Adam on them (adam != nullptr)
	//   reduce_items    fixed-order slab sums of the LDS levels into grad32[0, n_lds_params)
	// backward() = all four: the fp32 gradient of every grid parameter into grad32 [n_params].
	// dy_bound: launch_grid_bwd's (layout 0, written by the fused kernel beside dy)
	void backward_items(hipStream_t st, GridBwdBufs& w, uint32_t B, const float* pos, uint32_t pstride, const void* dy, int layout,
	                    uint32_t dy_stride, const GridBwdEpilogue* ep = nullptr, uint32_t reserved = 0, const float* dy_bound = nullptr) const;
	void backward_bin(hipStream_t st, GridBwdBufs& w, uint32_t B, const float* pos, uint32_t pstride, const void* dy, int layout,
	                  uint32_t dy_stride) const;
	void backward_acc(hipStream_t st, GridBwdBufs& w, uint32_t B, const void* dy, int layout, uint32_t dy_stride, float* grad32,
	                  const GridAccAdam* adam = nullptr) const;
	void reduce_items(hipStream_t st, GridBwdBufs& w, float* grad32, GradFinalize fin = {}) const;
	void backward(hipStream_t st, GridBwdBufs& w, uint32_t B, const float* pos, uint32_t pstride, const void* dy, int layout,
	              uint32_t dy_stride, float* grad32) const;
	// launch_grid_fwd / launch_grid_bwd_input / launch_grid_bwd_bwd (kernels.h) on this grid (call()).
	// T: the module's precision (_Float16, or float for an fp32 encoding module)
	void forward(hipStream_t st, uint32_t B, const float* pos, uint32_t pos_stride, const void* table16, void* out16, bool soa,
	             uint32_t out_stride, uint32_t aos_row_cols = 0) const {
		launch_grid_fwd(st, call(), B, pos, pos_stride, table16, out16, soa, out_stride, aos_row_cols);
	}
	template <typename T>
	void backward_input(hipStream_t st, uint32_t B, const float* pos, uint32_t pos_stride, const T* table, const T* dy, int dy_layout,
	                    uint32_t dy_stride, float* dx, uint32_t dx_stride) const {
		launch_grid_bwd_input(st, call(), B, pos, pos_stride, table, dy, dy_layout, dy_stride, dx, dx_stride);
	}
	template <typename T>
	void backward_backward_input(hipStream_t st, uint32_t B, const float* pos, uint32_t pos_stride, const T* table, const float* dL_ddLdx,
	                             const T* dy, uint32_t dy_stride, float* grad32, T* dLddLdy, uint32_t ddy_stride, float* dx) const {
		launch_grid_bwd_bwd(st, call(), B, pos, pos_stride, table, dL_ddLdx, dy, dy_stride, grad32, dLddLdy, ddy_stride, dx);
	}

	// ---- fp32 precision (an fp32 encoding module: fp32 table, AoS fp32 rows and dL/dy; grid_f32.hip) ----
	// The backward's work plan: EVERY level as LDS items holding all F features -- whole levels, or entry
	// ranges of the levels too large for the LDS (those the fp16 path bins: the binned backward packs fp16
	// into its records and has no fp32 form). Slabs are in parameter order. Built by build_plan_f32().
	GridPlan plan_f32;
	void build_plan_f32();
	// point chunks: items x chunks in one round on the CUs, >= 8192 points each (as bwd_chunks)
	uint32_t bwd_chunks_f32(uint32_t B) const {
		const uint32_t n_items = std::max<uint32_t>(1u, (uint32_t)plan_f32.slices.size());
		return std::max(1u, std::min(std::min(std::max(256u / n_items, 1u), 32u), B / 8192));
	}
	void forward_f32(hipStream_t st, uint32_t B, const float* pos, uint32_t pos_stride, const float* table32, float* out32,
	                 uint32_t out_stride) const {
		launch_grid_fwd_f32(st, call(), B, pos, pos_stride, table32, out32, out_stride);
	}
	// the fp32 gradient of every grid parameter into grad32 [n_params], bit-reproducible
	void backward_f32(hipStream_t st, GridBwdBufs& w, uint32_t B, const float* pos, uint32_t pstride, const float* dy32, uint32_t dy_stride,
	                  float* grad32) const;
};

// ---- fully fused MLP shape (reference networks/fully_fused_mlp.h) ----
struct MlpHost {
	uint32_t width = 64, n_input = 32, n_hidden_layers = 2, n_output = 16, padded_output = 16;
	int activation = 1, output_activation = 0;
	std::string otype = "FullyFusedMLP";
	MlpHost() = default;
	MlpHost(uint32_t n_input_dims, uint32_t n_output_dims, const json& net);
	uint32_t n_params() const {
		return n_hidden_layers == 0 ? padded_output * n_input
		                            : width * n_input + (n_hidden_layers - 1) * width * width + padded_output * width;
	}
	void initialize_params(Pcg32& rng, float* host_out, float scale = 1.0f) const;  // Xavier (gpu_matrix.h:284-299)
	json hyperparams() const;
};

struct AdamHost {
	float learning_rate = 1e-3f, beta1 = 0.9f, beta2 = 0.999f, epsilon = 1e-8f, l2_reg = 1e-8f;
	float relative_decay = 0.0f, absolute_decay = 0.0f, clipping_magnitude = 0.0f, non_matrix_learning_rate_factor = 1.0f;
	bool adabound = false, optimize_matrix_params = true, optimize_non_matrix_params = true;
	void update(const json& p);
	json hyperparams() const;
};

// One optimizer of a stacked "optimizer" block (optimizer_tree.h): its hyper-parameters, its host-side
// state and its device buffers (allocated by TrainerHost::opt_allocate). An Adam node holds nothing:
// Adam's hyper-parameters, step count and moments are the Trainer's (adam, adam_step, m1, m2, steps).
struct OptNode {
	OptKind kind = OptKind::Adam;
	std::unique_ptr<OptNode> nested;
	// SGD (sgd.h:146-152)
	float sgd_lr = 1e-3f, sgd_l2_reg = 1e-8f;
	uint32_t sgd_step = 0;
	// ExponentialDecay (exponential_decay.h:153-159): the nested learning rate is base_lr * lr_factor
	float decay_base = 0.1f, lr_factor = 1.0f, base_lr = 0.0f;
	uint32_t decay_interval = 10000, decay_start = 10000, decay_end = 10000000;
	// Ema (ema.h:209-214): weights_ema fp16 [n] (the inference parameters); tmp fp32 [n] with full_precision
	float ema_decay = 0.99f;
	bool full_precision = false;
	DevBuf weights_ema, tmp;
	// Lookahead (lookahead.h:163-167): weights_lookahead fp16 [n] (the inference parameters)
	float alpha = 0.5f;
	uint32_t n_steps = 16;
	DevBuf weights_lookahead;
	// Batched (batched.h:155-161): pool fp32 [n], its fp16 cast, own step counter
	uint32_t multiplier = 16, batched_step = 0;
	DevBuf pool, pool16;
};

// Encodings of the network input (reference encodings/*.h). An encoding is its list of parts, each
// over its own input columns (composite.h, Concatenation): the multiresolution grid (parametric),
// OneBlob (oneblob.h), Identity (identity.h), SphericalHarmonics and TriangleWave. An encoding that is
// not spelled as a Composite is one part over every input column. Grid, OneBlob and Identity parts
// have kernels of their own, which a part that stands alone runs (rows of any width); every other
// encoding runs the composite kernels (composite.hip), then each nested grid on its column slice.
struct EncodingHost {
	uint32_t n_dims = 0;  // input dims encoded
	// Precision of the parameters, the encoded rows and dL/dy (create_encoding<T>): fp16, or fp32 for an
	// fp32 encoding module, whose every buffer named "16" below then holds fp32 and whose kernels are the
	// fp32 ones (nothing narrowed to fp16). Layout, widths, alignment, parameter offsets, initial
	// parameters, hyperparams() and name() do not depend on it. fp16 networks and the Trainer build fp16 encodings,
	// an fp32 network module (NetworkF32Host) an fp32 one.
	bool f32 = false;

	// Widths follow composite.h:188-198: every part is created with alignment 1, part i is widened so
	// that part i + 1 starts at a multiple of its required alignment (a grid's n_features_per_level,
	// else 1), and the encoding's own alignment widens the last part. Parameters are the grids' tables
	// in order.
	struct Part {
		uint32_t kind = 0;  // COMP_* (kernels.h)
		uint32_t in_col = 0, n_in = 0, out_col = 0, width = 0, n_values = 0;
		uint32_t p0 = 0;             // SH degree | TriangleWave n_frequencies | OneBlob n_bins
		float f0 = 1.0f, f1 = 0.0f;  // Identity scale, offset
		uint32_t param_offset = 0;   // of a grid's table inside the encoding's parameters
		std::unique_ptr<GridEncodingHost> grid;
		std::unique_ptr<GridBwdBufs> bufs;  // scratch of this grid's backward
		bool f32 = false;                   // the encoding's precision (EncodingHost::f32)
		uint32_t required_alignment() const { return grid ? grid->desc.n_features_per_level : 1u; }
		bool own_kernel() const { return kind == COMP_GRID || kind == COMP_ONEBLOB || kind == COMP_IDENTITY; }
		json hyperparams() const;
		// This part's own kernel on its column slice. x, params16, out16 / dy16 and dx are the
		// encoding's: fp32 [B][x_stride], the parameters, AoS rows of `stride` columns (fp16; fp32 when
		// f32, like the parameters), fp32 [B][x_stride]. alone: the part owns the whole row (a grid then zeroes it for its padding).
		void forward(hipStream_t st, uint32_t B, const float* x, uint32_t x_stride, const void* params16, void* out16, uint32_t stride,
		             bool alone) const;
		void backward_input(hipStream_t st, uint32_t B, const float* x, uint32_t x_stride, const void* params16, const void* dy16,
		                    int dy_layout, uint32_t stride, float* dx) const;
	};
	std::vector<Part> parts;
	std::string otype;  // as spelled: "Composite", or the lone part's own ("Grid", "OneBlob", "SphericalHarmonics", ...)
	CompTable table{};  // the parts as the composite kernels read them (encodings that run them only)
	uint32_t n_grid_params = 0;

	EncodingHost(uint32_t n_dims_to_encode, const json& enc, bool fp32 = false);
	static bool known(const std::string& otype);
	static bool is_grid_otype(const std::string& otype);
	// the part that stands alone and runs its own kernel; nullptr: the composite kernels run
	const Part* lone_part() const { return otype != "Composite" && parts[0].own_kernel() ? &parts[0] : nullptr; }
	GridEncodingHost* lone_grid() const { return lone_part() ? parts[0].grid.get() : nullptr; }
	uint32_t padded_output_width() const { return parts.empty() ? 0u : parts.back().out_col + parts.back().width; }
	void set_alignment(uint32_t a) { layout(a); }  // Encoding::set_alignment (encoding.h)
	uint32_t n_params() const { return n_grid_params; }
	void initialize_params(Pcg32& rng, float* host_out, float scale = 1.0f) const;
	json hyperparams() const;
	// the reference's class name (SphericalHarmonicsEncoding, CompositeEncoding, ...)
	std::string name() const { return otype + "Encoding"; }
	// encoded output AoS fp16 (fp32 when f32) [B][padded_output_width()] (padding: grid 0, OneBlob / Identity /
	// TriangleWave 1 after the values, SphericalHarmonics 1 before them)
	void forward_aos(hipStream_t st, uint32_t B, const float* x, const void* params16, void* out16) const;
	// The layout the backward reads dL/d(encoding) fp16 in (launch_grid_bwd): AoS [B][padded width]
	// (2), or for a lone grid with feature pairs and no padding level-major pairs [L][B] (0), which
	// its backward reads coalesced (AoS rows would cost one 64-byte line per 4-byte read)
	int dy_layout() const {
		const GridEncodingHost* g = lone_grid();
		return !f32 && g && g->desc.n_features_per_level == 2 && g->n_to_pad == 0 ? 0 : 2;
	}
	// dL/dx fp32 [B][n_dims]; params16 = the encoding's parameters (grids). dy_layout: 2, or what
	// dy_layout() allows
	void backward_input(hipStream_t st, uint32_t B, const float* x, const void* dy16, float* dx, const void* params16 = nullptr,
	                    int dy_layout = 2) const;
	// the fp32 gradient of every grid's table into grad32 [n_params()] (each grid's slice in order),
	// each grid with its own scratch (an fp32 encoding: this is its dL/dparams, written in place)
	void backward_params(hipStream_t st, uint32_t B, const float* x, const void* dy16, int dy_layout, float* grad32) const;

private:
	void parse_composite(const json& enc);
	void add_part(uint32_t n_in, uint32_t in_col, const json& enc);
	void layout(uint32_t alignment);  // widths, columns, parameter offsets (+ build_table)
	void build_table();               // the composite kernels' argument, within its COMP_MAX_* limits
};

// Per-phase hipEvent timing of the training step (bench.py's live per-kernel roofline source).
// Phases on the trainer's stream: [0] fused grid+MLP kernel (fwd, loss, bwd, dW), [1] grid backward
// (two-launch step: with the reduction + Adam epilogue), [2] reductions, [3] loss sum / optimizer
// (sequential path only; phases a step does not have are skipped). Events are recorded
// only on every `every`-th step (each record is a barrier packet that idles the GPU for a few us).
struct PhaseTimer {
	static constexpr int N_PHASES = 4;
	bool enabled = false;
	uint32_t every = 1, counter = 0;
	bool sampling = false;  // this step records events
	std::vector<hipEvent_t> pool;
	std::vector<std::array<int, N_PHASES + 1>> marks;  // event indices per step (-1 = not recorded)
	size_t next = 0;
	hipEvent_t get();
	void mark(hipStream_t st, int phase);  // records the phase boundary on a sampled step
	void reset() { next = 0; marks.clear(); }
	~PhaseTimer();
};

// One forward+backward over a batch: what NetworkHost::fwd_bwd reads and writes. The gradient comes
// from the loss on `target` or, with dout16, from the caller's dL/d(output).
struct TrainPass {
	uint32_t B = 0;
	const float* pos = nullptr;      // fp32 [B][n_input_dims]
	const void* params16 = nullptr;  // [mlp | encoding] fp16
	const float* target = nullptr;   // fp32 [B][dims]: the network's loss, its dL/d(output) times loss_scale
	uint32_t dims = 0;
	float loss_scale = 1.0f;
	const void* dout16 = nullptr;  // external dL/d(output) fp16 [B][padded_output] instead of the loss
	// 0: dout16 as given; else fp16(dout16 * dout_scale), the torch binding's loss scale: folded into the
	// fused kernel's load, one scaling launch into ws.dout_scaled ahead of the other engines' pass
	float dout_scale = 0.0f;
	void* out16 = nullptr;       // optional network output fp16 [B][padded_output]
	float* grad32 = nullptr;     // fp32 gradient sums [mlp | encoding]
	float* dL_dinput = nullptr;  // optional fp32 [B][n_input_dims]
	// a forward_keep encoding of this batch and its layout (NetworkHost::KEEP_*); used when the layout is
	// the one the engine that runs reads
	const void* kept = nullptr;
	int kept_layout = 0;
	const void* kept_as(int layout) const { return kept_layout == layout ? kept : nullptr; }
	// the torch binding's finalised parameter gradient: written from the reductions where the engine can
	// (fwd_bwd then returns true), instead of a pass over grad32 afterwards
	GradFinalize fin{};
	PhaseTimer* timer = nullptr;  // phase marks 1..3 (nullable)
	void mark(hipStream_t st, int phase) const {
		if (timer) timer->mark(st, phase);
	}
};

// Workspace for one fwd/bwd over a batch of B (sizes grow only).
struct StepWorkspace {
	DevBuf dLdenc, wgrad_partial, loss_partial, grad32_tmp, out16, enc16, wimage;
	// the fused kernel's slice sums of max_f |dL/denc| ([L][B/32] floats) for the grid backward's
	// streaming pre-pass; dy_bound_live: the last fused_kernel wrote them beside dLdenc
	DevBuf dy_bound;
	bool dy_bound_live = false;
	GridBwdBufs gbw;
	DevBuf acts, delta0, delta1, dout16, red_tmp;  // layer-wise engine
	DevBuf dout_scaled;  // tile and layer-wise engines: TrainPass::dout16 x dout_scale
	DevBuf tile_wT;  // tile engine: transposed copy of the streamed hidden matrices
	DevBuf loss_sum;  // the grid backward epilogue's loss sum where nobody reads it (fwd_bwd_fused)
	uint32_t n_fused_blocks = 0, n_loss_partials = 0;
	bool wimage_valid = false;  // fused weight image matches the current fp16 params (trainer fast path)
};

// NetworkWithInputEncoding<__half> (reference network_with_input_encoding.h:41-190) over two engines:
//   "fused"   grid encoding + W in {32, 64} FullyFusedMLP: one register-resident kernel
//             (mlp_fused.h) + the LDS-privatised grid backward;
//   "fused"   (tile) W in {16, 32, 64, 128} FullyFusedMLP with any encoding (mlp_tile.h), training
//             and inference;
//   "layered" everything else (CutlassMLP, other widths, output activations):
//             per-layer MFMA kernels (mlp_layers.hip) with fp16 activations in HBM.
struct NetworkHost {
	EngineSwitches sw = EngineSwitches::from_env();
	std::unique_ptr<EncodingHost> enc;
	GridEncodingHost* grid = nullptr;  // enc->lone_grid(), cached: the fused path reads it every step
	MlpHost mlp;
	uint32_t n_input_dims = 0, n_output_dims = 0;
	const uint32_t loss_type;  // training loss: LossType (loss_device.h), 0 RelativeL2, 1 L2, ...
	NetworkHost(uint32_t n_in, uint32_t n_out, const json& enc, const json& net, uint32_t loss_type);
	uint64_t n_params() const { return (uint64_t)mlp.n_params() + enc->n_params(); }
	// the encoding's parameters inside params16 ([mlp | encoding] fp16)
	const void* enc_params(const void* params16) const { return (const uint8_t*)params16 + (size_t)mlp.n_params() * 2; }
	bool fused_ok() const;   // register-resident kernel (mlp_fused.h): grid input, W <= 64
	bool tile_shape_ok() const;  // tile kernels (mlp_tile.h): FullyFusedMLP W in {16..128}, any encoding, IN <= 128, H <= 5
	bool tile_ok() const;        // the training engine is the tile kernel (tile_shape_ok and not fused_ok)
	bool tile_infer_ok() const;  // inference runs the tile inference kernel
	bool layered_ok() const;
	const char* engine() const { return (fused_ok() || tile_ok()) ? "fused" : layered_ok() ? "layered" : "unsupported"; }
	const char* inference_engine() const;  // "fused" (one MLP launch) or "layered"
	// the kernel family fwd_bwd dispatches to (with_dinput: the caller wants dL/dinput): the register-resident
	// kernel (mlp_fused.h), the tile kernel (mlp_tile.h) or one kernel per layer; backward_kernel names it
	// "register" / "tile" / "layered" / "unsupported"
	enum class BackwardKernel { Register, Tile, Layered, Unsupported };
	BackwardKernel backward_kernel_kind(bool with_dinput) const;
	const char* backward_kernel(bool with_dinput) const;
	void initialize_params(Pcg32& rng, float* host_out, float scale = 1.0f) const;  // network first (nwie.h:124-130)

	// params16: [mlp | encoding] fp16. out16: fp16 [B][padded_output].
	// trust_image: ws.wimage_valid tracks params16 (the Trainer's own parameters, whose every writer
	// clears it), so a valid fused weight image is reused instead of re-packed
	void inference(hipStream_t st, StepWorkspace& ws, uint32_t B, const float* pos, const void* params16, void* out16,
	               bool trust_image = false);
	// Forward that keeps what the backward needs (the reference's forward context, cpp_api.cu:84-109,
	// network_with_input_encoding.h:70-81): the encoding, in the layout of the engine the backward will
	// run (with_dinput: the caller wants dL/dinput) -- SoA [IN][B] for the register-resident grid kernel,
	// AoS [B][IN] for the tile kernel -- into keep (grown here). Returns the layout kept (KEEP_*); the
	// layer-wise engine keeps nothing (its backward recomputes the forward).
	enum : int { KEEP_NONE = 0, KEEP_FUSED_SOA = 1, KEEP_TILE_AOS = 2 };
	int backward_engine_keep(bool with_dinput) const;
	void fused_forward(hipStream_t st, StepWorkspace& ws, uint32_t B, const float* pos, const void* params16, bool use_image, void* enc_soa,
	                   void* out16);
	int forward_keep(hipStream_t st, StepWorkspace& ws, uint32_t B, const float* pos, const void* params16, void* out16, bool with_dinput,
	                 DevBuf& keep);
	// forward+backward of one pass (TrainPass): the fp32 gradient sums into p.grad32 ([mlp | encoding]),
	// the loss partials into ws.loss_partial[0 .. ws.n_loss_partials), dL/dinput when asked for. Returns
	// whether the parameter gradient also went out finalised (p.fin).
	bool fwd_bwd(hipStream_t st, StepWorkspace& ws, const TrainPass& p);
	json hyperparams() const;

	// pieces of the fused engine for the trainer's overlapped step
	// pack: do not reuse ws.wimage (the parameters need not be the ones it was packed from);
	// emit_dy_bound: write the grid backward's slice sums beside dL/d(encoding) where the kernel can
	void fused_kernel(hipStream_t st, StepWorkspace& ws, const TrainPass& p, bool pack, bool emit_dy_bound = false);
	void grid_backward(hipStream_t st, StepWorkspace& ws, uint32_t B, const float* pos, GridBwdEpilogue* ep = nullptr);
	void pack_weights(hipStream_t st, StepWorkspace& ws, const void* params16);

private:
	bool fwd_bwd_fused(hipStream_t st, StepWorkspace& ws, const TrainPass& p);
	void fwd_bwd_tile(hipStream_t st, StepWorkspace& ws, const TrainPass& p);
	void fwd_bwd_layered(hipStream_t st, StepWorkspace& ws, const TrainPass& p);
	// p.dout16 as the tile and layer-wise engines read it (scaled into ws.dout_scaled when p.dout_scale is set)
	const void* scaled_dout(hipStream_t st, StepWorkspace& ws, const TrainPass& p);
	// The weight image a fused launch reads: ws.wimage when have_image (a packed image the caller
	// trusts); nullptr for 16-byte aligned parameters (every workgroup builds its LDS image from them, no
	// pack launch); else -- a parameter view with an odd offset, e.g. a slice of a flat torch buffer --
	// the image packed here
	const void* weight_image(hipStream_t st, StepWorkspace& ws, const void* params16, bool have_image);
	// forward through the layers from ws.enc16; hidden activations kept in ws.acts when `keep`
	void forward_layers(hipStream_t st, StepWorkspace& ws, uint32_t B, const void* params16, void* out16, bool keep);
};

// NetworkWithInputEncoding<float>: an fp32 network module (Network / NetworkWithInputEncoding dtype = float32).
// The fp32 EncodingHost in front, its rows handed to the first layer as they are, then one f32-MFMA kernel per
// layer (mlp_f32.hip). Parameters [mlp | encoding], rows, dL/dy, dL/dparams and dL/dinput are all fp32; layout,
// parameter count, initial values, hyperparams() follow NetworkHost for the same config. FullyFusedMLP and
// CutlassMLP run the same kernels. Sine (no backward from its forward value) is served by inference() only.
struct NetworkF32Host {
	EngineSwitches sw = EngineSwitches::from_env();
	std::unique_ptr<EncodingHost> enc;
	MlpHost mlp;
	uint32_t n_input_dims = 0, n_output_dims = 0;
	DevBuf acts, delta0, delta1, wgrad_partial, red_tmp;  // grow-only scratch
	NetworkF32Host(uint32_t n_in, uint32_t n_out, const json& enc, const json& net);
	uint64_t n_params() const { return (uint64_t)mlp.n_params() + enc->n_params(); }
	bool has_sine() const { return mlp.activation == ACT_SINE || mlp.output_activation == ACT_SINE; }
	void initialize_params(Pcg32& rng, float* host_out, float scale = 1.0f) const;
	json hyperparams() const;
	// what a forward keeps for its backward: [enc B x IN | NH hidden activations B x W | output B x OUTP] floats
	size_t keep_floats(uint32_t B) const {
		return (size_t)B * ((size_t)mlp.n_input + (size_t)mlp.n_hidden_layers * mlp.width + mlp.padded_output);
	}
	// out32 fp32 [B][padded_output]; keep (nullable): keep_floats(B) floats, else two ping-pong buffers of the scratch
	void forward(hipStream_t st, uint32_t B, const float* pos, const float* params, float* out32, float* keep);
	// from a forward's keep: dL/dparams fp32 [n_params()] (nullable), dL/dinput fp32 [B][n_input_dims] (nullable)
	void backward(hipStream_t st, uint32_t B, const float* pos, const float* params, const float* dout32, const float* keep,
	              float* dL_dparams, float* dL_dinput);
	// Second order with respect to the input, from a forward's keep: dL_ddLdinput = dL2/d(dL/dinput) fp32
	// [B][n_input_dims] -> dL2/dparams [n_params()], dL2/d(dL/doutput) [B][padded_output], dL2/dinput
	// [B][n_input_dims] (each nullable, each overwritten). dout32, the first-order dL/doutput, may be null when only
	// dL_ddLdoutput is asked for. The encoding in front is Identity or a lone grid; any other throws. The network's part
	// of dL2/dparams is bit-reproducible, the grid's (fp32 atomics) is not.
	void backward_backward_input(hipStream_t st, uint32_t B, const float* pos, const float* params, const float* dL_ddLdinput,
	                             const float* dout32, const float* keep, float* dL_dparams, float* dL_ddLdoutput, float* dL_dinput);
	void check_second_order() const;  // throws for Sine and for an encoding that is neither Identity nor a lone grid
	DevBuf second, grid_tmp;  // grow-only scratch of backward_backward_input: its delta / tangent / curvature chains; a grid's second table gradient
};

// One RCCL communicator of a data-parallel job (dp.cpp): rank `rank` of `nranks`, one process per
// GPU; collectives run on its own stream `cs`, joined to the trainer's stream with events.
struct DpComm {
	void* comm = nullptr;  // ncclComm_t
	int nranks = 1, rank = 0;
	hipStream_t cs = nullptr;
	hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
	DpComm(const void* unique_id, int nranks, int rank);
	~DpComm();
	DpComm(const DpComm&) = delete;
	DpComm& operator=(const DpComm&) = delete;
	void all_reduce_f32(float* buf, size_t n, hipStream_t st);
	// in place: rank r receives the sum of [r per, (r + 1) per) at buf + r per
	void reduce_scatter_f32(float* buf, size_t per, hipStream_t st);
	// in place: rank r's [r per, (r + 1) per) elements of elem_bytes (2 or 4) to every rank
	void all_gather(void* buf, size_t per_elems, int elem_bytes, hipStream_t st);
};
void dp_unique_id(void* id128);  // ncclGetUniqueId (one rank; the caller broadcasts it)

// Trainer::forward's context (reference trainer.h:89-95, 97-144): the network output, the loss-scaled
// dL/d(output) (from the loss, or the caller's external dL/dy), the loss partial sums and the encoding
// kept for the backward (NetworkHost::forward_keep).
struct TrainerFwdCtx {
	uint32_t B = 0;
	DevBuf keep;
	int layout = 0;
	DevBuf out16, dLdy16, lpart;
	DevBuf pert16;              // output + perturbation, what the loss saw (trainer.h:114-123)
	const void* ext = nullptr;  // external dL/dy (not owned)
	bool inference_params = false;  // the forward read the optimizer's custom weights: no backward
	uint32_t n_lpart = 0;
	const void* dLdy() const { return ext ? ext : dLdy16.p; }
};

// Stream-ordered workspace arena (arena.cpp; reference gpu_memory.h:426-754)
void* workspace_allocate(hipStream_t st, size_t n_bytes);
void workspace_free(hipStream_t st, void* p);
void workspace_arena_free(hipStream_t st);
void workspace_arena_free_all();
uint64_t dp_peer_blob_bytes();  // bytes of one rank's peer-exchange blob (dp_peer.hip)
double peer_default_timeout_s();  // TCNN_PEER_TIMEOUT_S or 300 s
void workspace_arena_info(hipStream_t st, uint64_t* mapped_bytes, int* vmm);

struct TrainerHost {
	uint32_t n_input_dims, n_output_dims;
	PhaseTimer timer;
	json config;
	std::unique_ptr<NetworkHost> model;
	AdamHost adam;
	std::string loss_otype;
	uint64_t n_params = 0, n_mlp = 0;
	DevBuf w32, w16, g16, g32, m1, m2, steps, d_loss;
	// Adam bias-correction factors of steps 1 .. ftable_valid (AdamArgs::factor_table), for the betas
	// they were computed with; grown by doubling
	DevBuf d_ftable;
	std::vector<float> h_ftable;  // host staging of the table (computed on the host, see adam_args_table)
	uint32_t ftable_cap = 0, ftable_valid = 0;
	float ftable_b1 = 0.0f, ftable_b2 = 0.0f;
	// makes the table cover steps 1 .. upto (computing what is missing, 1024 steps ahead) and
	// returns args with factor_table / factor_n set
	// (capacity for at least `reserve` entries)
	AdamArgs adam_args_table(hipStream_t st, uint32_t upto, uint32_t reserve = 0);
	StepWorkspace ws;
	uint32_t adam_step = 0;
	float grad_scale = 1.0f;       // what Adam multiplies the fp32 gradient sum by
	float grad_scale_user = 1.0f;  // the caller's factor (tcnn_trainer_set_gradient_scale); x 1/N under set_dp
	float loss_scale = 128.0f;  // default_loss_scale<__half> (common.h:232)
	uint32_t last_B = 0;

	// ---- lean Adam over the grid slabs (EngineSwitches::adam_lean; k_adam<LEAN>, kernels.hip) ----
	// The one-call single-GPU step (training_step_overlapped with the optimizer, eager or replayed) may
	// leave two things undone in the grid range [n_mlp, n_mlp + n_lds_params); every other reader or
	// writer of that state goes through lean_settle first.
	//  * ADAM_LEAN_GRADS: g32 / g16 are not stored. grads_stale says so; the step's chunk slabs stay
	//    intact in ws.gbw until the next backward, so grads_materialize() sums them again (same slab
	//    order, same f16_rn(sum * grad_scale)) on the stream of that step.
	//  * ADAM_LEAN_STEPS: step_blocks holds one count per 256 parameters (AdamArgs::step_blocks);
	//    steps[] is current only for the diverged blocks until steps_expand() writes the others out.
	// A caller who asked for the raw pointers (tcnn_trainer_param_gradients / _gradients_fp32 /
	// _optimizer_state) may cache them, so that switches the trainer to the eager stores / per-parameter
	// counts for good (LeanUse::Caller); so does attaching a data-parallel exchange.
	uint32_t adam_lean = EngineSwitches::from_env().adam_lean;
	bool grads_eager = false, steps_per_param = false;  // sticky (LeanUse::Caller)
	bool grads_stale = false;                           // the grid range of g32 / g16 is one step behind the slabs
	float stale_grad_scale = 1.0f;                      // grad_scale of the step whose slabs they are
	hipStream_t lean_st = nullptr;                      // the stream of the last lean step
	DevBuf step_blocks;                                 // uint32 [n_step_blocks()], 0 after initialize_params
	bool steps_current = true;                          // steps[] holds every count
	bool step_blocks_diverged = false;                  // every word is ADAM_STEPS_DIVERGED (nothing to expand or mark)
	uint32_t n_step_blocks() const;
	// the AdamArgs::lean bits of a one-call step taken now (0: not on that path, or all switched off)
	uint32_t lean_mask() const;
	// Read: g32 / g16 / steps[] are made current and stay so until the next lean step. Write: also
	// marks every block diverged, for whoever updates steps[] itself (the next lean steps vote the
	// blocks uniform again). Caller: Write, and the trainer stays eager / per-parameter from now on.
	enum class LeanUse { Read, Write, Caller };
	void lean_settle(LeanUse use);
	void grads_materialize();
	void steps_expand(LeanUse use);
	void lean_note_step(hipStream_t st, uint32_t lean);  // host-side state after a one-call step (eager or replayed)
	uint32_t uniform_step_blocks();  // debug_adam.h: blocks whose word is a count (synchronises)

	// two-launch single-GPU step: reductions + Adam fused into the grid backward's epilogue
	bool overlapped_ok() const { return model->fused_ok(); }
	// The two schedules of a step. grad_out (run_optimizer = false only): where the fp32 gradient sums go
	// (default g32)
	void training_step_overlapped(hipStream_t st, uint32_t B, const float* input, const float* target, bool run_optimizer,
	                              float* grad_out = nullptr);
	void training_step_sequential(hipStream_t st, uint32_t B, const float* input, const float* target, bool run_optimizer,
	                              float* grad_out = nullptr);
	// the trainer's own pass: the loss on `target` at the training parameters, gradients into grad32
	TrainPass loss_pass(uint32_t B, const float* input, const float* target, float* grad32) const;
	// this rank's fp32 gradient sums (into grad_out, default g32) and the loss sum, no optimizer, on the
	// engine's schedule
	void gradient_pass(hipStream_t st, uint32_t B, const float* input, const float* target, float* grad_out = nullptr);
	// the same gradients from the fused engine in two halves, so that a caller can send the network
	// gradients off while the grid backward runs: 0 the fused kernel, the network-gradient column sums into
	// g32[0, n_mlp) and the loss sum; 1 the grid backward and its reductions into g32[n_mlp, n)
	void fused_gradient_half(hipStream_t st, uint32_t B, const float* input, const float* target, int half);
	// one single-GPU step with Adam inside, on the engine's schedule
	void step_adam(hipStream_t st, uint32_t B, const float* input, const float* target);
	AdamArgs adam_args() const;

	// ---- stacked optimizers (optimizer_tree.cpp). opt == nullptr: plain Adam, whose every path below
	// is untouched. Otherwise opt owns the step: opt_inline (only ExponentialDecay / Ema above Adam)
	// keeps Adam's schedule -- the learning rate is set on the host before it, one EMA launch follows --
	// and every other tree runs the gradient pass of run_optimizer = false, then steps on the gradient
	// buffers. ----
	std::unique_ptr<OptNode> opt;
	bool opt_inline = false;
	// what one level's step reads: the fp32 gradient sums x gscale (Adam's input), their fp16 rounding
	// (everybody else's); whole: the Adam leaf runs the engine's whole step with the optimizer on the batch
	struct OptStep {
		hipStream_t st = nullptr;
		const float* g32 = nullptr;
		float gscale = 1.0f;
		void* g16 = nullptr;
		bool whole = false;
		uint32_t B = 0;
		const float* input = nullptr;
		const float* target = nullptr;
	};
	std::unique_ptr<OptNode> opt_build(const json& p);
	void opt_allocate();      // (re)allocates and zeroes the tree's buffers and counters (initialize_params)
	void opt_reset_weights();  // the custom-weights buffer <- the fp16 parameters (trainer.h:248-265)
	void opt_update(OptNode& n, const json& p);
	json opt_hyperparams(const OptNode& n) const;
	uint32_t opt_count(const OptNode& n) const;  // Optimizer::step()
	float opt_lr(const OptNode& n) const;
	void opt_set_lr(OptNode& n, float v);
	void* opt_custom_weights(const OptNode& n) const;
	void opt_step(OptNode& n, const OptStep& s);
	void opt_training_step(hipStream_t st, uint32_t B, const float* input, const float* target);
	// Adam on the fp32 sums grad32 x gscale (fp16 gradients written to grad16)
	void adam_apply(hipStream_t st, const float* grad32, float gscale, void* grad16);
	void update_optimizer_hyperparams(const json& p);  // Trainer::update_hyperparams' "optimizer" block
	json optimizer_hyperparams() const;
	uint32_t optimizer_step_count() const { return opt ? opt_count(*opt) : adam_step; }
	float learning_rate() const { return opt ? opt_lr(*opt) : adam.learning_rate; }
	void set_learning_rate(float v);
	// Trainer::params_inference(): the optimizer's custom weights, else the training parameters
	void* params_inference() const;
	// a named state buffer of the tree ("weights_ema", "tmp", "weights_lookahead", "averaged_gradients",
	// "averaged_gradients_half"), outermost first; nullptr when the tree has none
	void* optimizer_buffer(const std::string& name, uint32_t* elem_bytes) const;
	// the data-parallel schedules and optimizer_step_range apply Adam themselves
	void require_plain_adam(const char* what) const;

	TrainerHost(uint32_t n_in, uint32_t n_out, const json& cfg, uint32_t seed);
	void initialize_params(uint32_t seed);
	void initialize_params_rng(Pcg32& rng);  // from the caller's generator (advanced by n_params draws)
	void training_step(hipStream_t st, uint32_t B, const float* input, const float* target, bool run_optimizer);
	void step_eager(hipStream_t st, uint32_t B, const float* input, const float* target);  // with the optimizer
	void training_step_part(hipStream_t st, uint32_t B, const float* input, const float* target, int part);
	void optimizer_step(hipStream_t st);
	// Trainer::forward / backward (trainer.h:97-153): the two halves of training_step with the
	// reference's options -- data_pdf (fp32 [B][n_output_dims]), external dL/dy (fp16 [B][padded
	// output], loss-scaled like the loss's own), dL/dinput (fp32 [B][n_input_dims]) and Accumulate
	// gradients (added to gradients_fp32() instead of overwriting it). Gradients land in the buffer
	// optimizer_step() reads.
	// perturbation (nullable): fp32 [B][padded output] noise added to the output before the loss
	std::unique_ptr<TrainerFwdCtx> forward(hipStream_t st, uint32_t B, const float* input, const float* target, const float* pdf,
	                                       const void* ext_dLdy16, bool prep_dinput, const float* perturbation = nullptr,
	                                       bool use_inference_params = false);
	// gradient_mode: 0 Overwrite, 1 Accumulate, 2 Ignore (GradientMode, common.h)
	void backward(hipStream_t st, const TrainerFwdCtx& c, uint32_t B, const float* input, float* dL_dinput, int gradient_mode);
	float ctx_loss(hipStream_t st, const TrainerFwdCtx& c);
	DevBuf g32_acc;  // Accumulate mode: this backward's gradients before they are added
	// data-parallel exchange inside the step (dp.cpp): with a communicator attached every
	// training_step(run_optimizer = true) sums the gradients across the ranks (all-reduce, or
	// reduce-scatter + Adam on this rank's shard + all-gather of the fp16 parameters when sharded)
	DpComm* dp = nullptr;
	bool dp_sharded = false, dp_state_partial = false;
	uint64_t dp_per = 0;  // parameters per shard (sharded: buffers padded to nranks * dp_per)
	void set_dp(DpComm* c, bool sharded);
	void training_step_dp(hipStream_t st, uint32_t B, const float* input, const float* target);
	void dp_gather_state(hipStream_t st);
	// data-parallel exchange over peer-mapped device memory, no collective library (dp_peer.hip):
	// export IPC handles of this rank's buffers, attach every rank's, then each training_step exchanges
	// through the peers' memory (sharded Adam, fp16 parameter gather)
	struct PeerDp;
	std::shared_ptr<PeerDp> peer;
	bool peer_attached = false;
	void dp_peer_export(int nranks, int rank, void* blob);
	void dp_peer_attach(const void* blobs);
	void dp_peer_detach();
	void dp_peer_loopback(int nranks);  // measurement only: an N-rank attachment whose peers are all this rank
	void dp_peer_abandon();  // local, no barrier: only before any exchange step (a failed attach on some rank)
	double peer_timeout_s = peer_default_timeout_s();
	void dp_peer_set_timeout(double seconds);
	void peer_check() const;  // throws if a wait of an earlier step failed
	int peer_nranks = 1;  // ranks of the attached peer exchange
	// ranks whose gradients Adam's input sums (RCCL communicator or peer exchange): grad_scale = user / N
	int dp_nranks() const { return dp ? dp->nranks : (peer_attached ? peer_nranks : 1); }
	void dp_peer_gather_state(hipStream_t st);
	void training_step_peer(hipStream_t st, uint32_t B, const float* input, const float* target);
	void peer_wait(hipStream_t st, int c, int slot, int signal_bump = -1, long long timeout_ticks = -1);  // -1: the peer timeout
	void peer_gather(hipStream_t st, int what, bool poll);
	// Adam on parameters [begin, end) only (data-parallel sharded optimizer: each rank updates its
	// shard of the reduce-scattered gradient, then the fp16 parameters are all-gathered)
	void optimizer_step_range(hipStream_t st, uint64_t begin, uint64_t end);
	float loss(hipStream_t st);
	void inference(hipStream_t st, uint32_t B, const float* input, float* out);
	void set_params_full_precision(const float* host, uint64_t n);
	// snapshot in the reference's msgpack format (Trainer::serialize / deserialize, trainer.h:275-315)
	std::vector<uint8_t> serialize(bool with_optimizer);
	// the same object as JSON text, binaries as {"bytes": [...], "subtype": null} (json serialize(bool))
	std::string serialize_json(bool with_optimizer);
	void deserialize(const void* data, size_t size);
	void profile_end(double* ms, uint32_t n_phases, uint32_t* n_steps);

	// hipGraph replay of the single-GPU training step (the reference Trainer's CUDA graph,
	// trainer.h:163-190, cuda_graph.h:52-178). Opt-in (tcnn_trainer_set_graph). A graph is replayed
	// while every scalar and device pointer the step's kernels read is unchanged (graph_key); any
	// change (batch size, input / target buffers, hyper-parameters, scales, workspace growth) runs
	// the step eagerly and re-captures. The Adam bias-factor table is filled GRAPH_STEPS steps ahead
	// first, so a replayed step carries no step-dependent kernel argument.
	static constexpr uint32_t GRAPH_STEPS = 1u << 20;
	bool use_graph = false;
	struct StepGraph;
	std::unique_ptr<StepGraph> graph;
	uint64_t graph_replays = 0, graph_captures = 0;
	std::vector<uint64_t> graph_key(uint32_t B, const float* input, const float* target) const;
	bool training_step_graph(hipStream_t st, uint32_t B, const float* input, const float* target);
	void set_graph(bool on);
	~TrainerHost();
};

}  // namespace tcnn_amd
