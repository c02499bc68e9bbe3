// kernels.h -- host-side launchers of the gfx950 kernels (defined in kernels.hip).
#pragma once

#include "common.h"

namespace tcnn_amd {

struct LevelInfo;

// What every grid launcher needs to know about the grid it runs on (GridEncodingHost::call()): the
// shape that selects the kernel (grid_dispatch.h), the device level table and the options.
struct GridCall {
	uint32_t D, F, L;  // input dims, features per level, levels
	HashType hash;
	bool hash_grid;    // GridType::Hash (dense and tiled grids index without hashing)
	Interp interp;
	const LevelInfo* levels;  // device [L]
	GridOpts opts;
};

// Work plan of the LDS-privatised grid backward: one item per (level, entry range, feature range);
// the item's int32 accumulators (end-begin) x nf fit in grid_bwd_slot_budget() LDS slots.
struct GridSlice {
	uint32_t level;
	uint32_t begin;  // entry range within the level
	uint32_t end;
	uint32_t f0;     // feature range [f0, f0 + nf)
	uint32_t nf;
};

// Binned backward of the grid levels whose accumulators do not fit the LDS (grid_bin.hip): the
// level's entries are cut into slices of 2^slice_log2 entries; every (point, corner) update is
// counting-sorted by slice into per-chunk record runs, then one workgroup per slice ("bucket")
// accumulates its records in LDS and writes (or applies Adam to) the slice's gradient.
struct GridBinLevel {
	uint32_t level;
	uint32_t slice_log2;
	uint32_t n_slices;
	uint32_t bucket_base;  // first global bucket of the level
};

struct GridBinArgs {
	const GridBinLevel* lv;  // [n_slots]
	uint32_t n_slots, n_buckets;
	uint32_t n_chunks, pts_per_chunk;  // point chunks of the bin pass (pts_per_chunk = GRID_BIN_RECS >> D)
	uint32_t acc_lds_bytes;            // accumulator bytes of the largest slice
	uint2* recs;     // [n_slots][n_chunks][GRID_BIN_RECS] {(w16 << 16) | entry-in-slice, dL/dy bits or point index}
	uint2* dir;      // [n_buckets][n_chunks] {first record of the bucket's run in the chunk, count}
	float* dysum;    // [n_slots][n_chunks][F] sum of |dL/dy| (fixed-point range of the level)
};
constexpr uint32_t GRID_BIN_RECS = 4096;        // records per (level, chunk) run
constexpr uint32_t GRID_BIN_MAX_SLICES = 2048;  // slices per level
constexpr uint32_t GRID_ACC_LDS_BYTES = 64 * 1024;  // accumulator budget of one slice

// Runtime activation codes of the layer-wise engine (reference Activation, common.h:126-136).
enum : int {
	ACT_NONE = 0, ACT_RELU = 1, ACT_LEAKY_RELU = 2, ACT_EXPONENTIAL = 3, ACT_SINE = 4, ACT_SIGMOID = 5,
	ACT_SQUAREPLUS = 6, ACT_SOFTPLUS = 7, ACT_TANH = 8,
};

// Layout of the grid backward's per-chunk fp32 partial slabs: level-major like the parameters, but
// within a level whose work items hold nf < F features the slab is feature-group-major
// ([F/nf][size][nf]) so every item writes one contiguous range. slab index of grid parameter p,
// level l, entry e, feature f (f0 = f - f % nf):  pbase[l] + f0 * size[l] + e * nf[l] + (f - f0).
// Points per chunk up to which the LDS grid backward keeps a chunk's dL/dy in registers
// (GRID_BWD_THREADS x GRID_BWD_PR, grid_bwd_lds.h): the faster path, so large batches take more chunks.
constexpr uint32_t GRID_BWD_REG_POINTS = 1024u * 32u;

struct GridSlabMap {
	uint32_t n_levels, log2F;
	uint32_t pbase[MAX_LEVELS + 1];  // offset_l * F
	uint32_t size[MAX_LEVELS];
	uint32_t nf[MAX_LEVELS];
};

__device__ __forceinline__ uint32_t grid_slab_index(const GridSlabMap* __restrict__ m, uint32_t p) {
	uint32_t l = 0;
	while (l + 1 < m->n_levels && p >= m->pbase[l + 1]) ++l;
	const uint32_t r = p - m->pbase[l];
	const uint32_t e = r >> m->log2F, f = r & ((1u << m->log2F) - 1u);
	const uint32_t nf = m->nf[l];
	const uint32_t f0 = f & ~(nf - 1u);
	return m->pbase[l] + f0 * m->size[l] + e * nf + (f - f0);
}

struct AdamArgs {
	uint32_t n, n_matrix;
	float loss_scale, grad_scale;  // grad_scale multiplies the fp32 gradient before fp16 rounding (1/N for N-rank sums)
	float lr, beta1, beta2, eps, l2_reg, rel_decay, abs_decay, clip, nonmat_lr_factor;
	float lower_lr_bound, upper_lr_bound;
	int opt_matrix, opt_nonmatrix;
	float inv_loss_scale;  // 1 / loss_scale when that is exact (power of two), else 0
	// parameter range [begin, n) of this launch; when part != nullptr the gradient of parameter i is
	// the fixed-order sum of n_parts partial slabs part[j * part_stride + (i - begin)] (written back
	// to grad32[i]) instead of grad32[i] (reduction fused into the optimizer)
	uint32_t begin;
	const float* part;
	uint32_t n_parts, part_stride;
	// bias-correction factors sqrt(1 - beta2^t) / (1 - beta1^t) precomputed on the device by the
	// same adam_bias_factor for t = 1 .. factor_n (factor_table[t - 1]); other t are computed per
	// parameter. Parameters carry their own step counts (adam.h:110-113), so without the table every
	// grid entry paid two powf -- the Adam epilogue of the binned backward was VALU-bound on them.
	const float* factor_table;
	uint32_t factor_n;
	// grid slabs: parameter i reads slab element grid_slab_index(part_map, i - begin) (nullptr: i - begin)
	const GridSlabMap* part_map;
	// Slab-summing launches only (part != nullptr), EngineSwitches::adam_lean:
	// ADAM_LEAN_GRADS: grad32[i] and grad16[i] are not stored (the slabs stay intact after the step; the
	// trainer sums them again when a caller asks for the gradients).
	// ADAM_LEAN_STEPS: step_blocks[b] is the common step count of parameters [begin + 256 b, begin + 256 b +
	// 256) and steps[] is neither read nor written for them, or ADAM_STEPS_DIVERGED: steps[] is
	// authoritative. After every launch a block's word is a count exactly when its counts are all equal.
	uint32_t lean;
	uint32_t* step_blocks;
};

// Default: the gradient stores only. The block counts measured slower at 2^18 (k_adam 11.2 against 10.2 us): a
// block that once diverged stays so, and after 220 bench steps 3 of 2768 blocks were still uniform (DESIGN (f) 5).
enum : uint32_t { ADAM_LEAN_GRADS = 1u, ADAM_LEAN_STEPS = 2u, ADAM_LEAN_ALL = 3u, ADAM_LEAN_DEFAULT = ADAM_LEAN_GRADS };
constexpr uint32_t ADAM_STEPS_DIVERGED = 0xFFFFFFFFu;
constexpr uint32_t ADAM_STEP_BLOCK = 256;

// Optimizer state buffers (full parameter vector [network | encoding]).
struct AdamBuffers {
	float* w32;
	_Float16* w16;
	float* g32;      // fp32 gradient sums (written by fused-reduction epilogues)
	_Float16* g16;   // fp16 gradients (reference m_param_gradients)
	float* m1;
	float* m2;
	uint32_t* steps;
};

// Work carried by the grid backward launch (single-GPU trainer step): n_mlp_groups extra
// workgroups, on CUs the grid items leave free, each reduce one column block of the fused kernel's
// network-gradient slabs, run Adam on those network parameters and write them into the next step's
// fused weight image; workgroup 0 also sums the loss partials.
// Where a reduction writes the torch binding's finalised parameter gradient (grad_finalize_store,
// common.h) instead of fp32 sums: out (nullable; fp16, or fp32 if out_f32) at the parameter's index.
struct GradFinalize {
	void* out = nullptr;
	float s = 1.0f;
	int out_f32 = 0;
};

struct GridBwdEpilogue {
	int enabled;
	int apply_adam;          // 0: only the reduction (network gradients -> buf.g32, loss), for the
	                         // multi-GPU path where the all-reduce sits between reduction and Adam
	AdamArgs adam_mlp;       // range [0, n_mlp)
	AdamBuffers buf;
	// network-gradient tail
	uint32_t n_mlp_groups;   // extra workgroups (0 = none)
	const float* wpart;      // fused kernel slabs [n_wparts][n_mlp]
	uint32_t n_wparts, n_mlp;
	const float* lpart;      // loss partials [n_wparts]
	float* d_loss;
	// fused weight image (mlp_fused.h FusedLayout): W0 rows of RSI halves at 0, hidden rows of RSW
	// at oWh, output rows of RSW at oWo
	_Float16* wimage;
	uint32_t W, IN, NH, RSI, RSW, oWh, oWo;
	GradFinalize fin;        // apply_adam == 0: network gradients finalised into fin.out instead of buf.g32
};

bool fused_train_loss_supported(uint32_t W, uint32_t NH, uint32_t loss_type);  // loss_type: LossType (loss_device.h)
// Fused train step (grid encoding -> MLP fwd -> RelativeL2 -> MLP bwd -> dW partials, dL/denc).
// With dout16 != NULL the loss is skipped and dL/d(output) fp16 [B][16] is read instead (Module::backward).
// Returns false if no fused kernel exists for this shape.
bool fused_train_supported(uint32_t W, uint32_t IN, uint32_t NH, uint32_t D, uint32_t F, uint32_t OUTP, int act, HashType h);
// Workgroups the fused launch uses (= partial slabs it writes) for this shape and batch.
uint32_t fused_train_waves();  // waves per workgroup of k_fused_train_grid
uint32_t fused_train_n_blocks(uint32_t W, uint32_t IN, uint32_t NH, uint32_t D, uint32_t dims, bool ext_dout, uint32_t B);
// The kernel argument of the fused train step, filled by the host that launches it (value-initialise
// it: what is not set is null / 0); launch_fused_train sets the fields marked (launcher).
struct FusedTrainArgs {
	const _Float16* wimage; // packed LDS weight image (k_pack_weights), or null: built from params
	uint32_t B;
	uint32_t dims;          // target width (n_output_dims)
	float loss_scale;
	float n_total;          // (launcher) (float)(B * dims) as in relative_l2.h:64
	uint32_t loss_type;     // LossType (loss_device.h): 0 RelativeL2, 1 L2, ... (wave-uniform switch)
	uint32_t inrange_index; // (launcher) 1: grid_index_inrange is exact for in-range positions (Linear interpolation)
	const _Float16* params; // MLP weights fp16 [W0 | hidden | Wout]
	const uint32_t* table;  // grid params as half2 entries (F == 2)
	const float* pos;       // [B][D]
	const float* target;    // [B][dims]
	_Float16* out;          // optional network output [B][16]
	uint32_t* dLdenc;       // [L][B] half2 (level-major feature pairs)
	float* wgrad_partial;   // [gridDim.x][N_MLP]
	float* loss_partial;    // [gridDim.x]
	const LevelInfo* levels;  // (launcher)
	uint32_t hash_grid;       // (launcher)
	uint32_t interp;          // (launcher)
	const _Float16* dout;   // EXT_DOUT: external dL/d(output) fp16 [B][16] (loss-scaled by the caller)
	float dout_scale;       // EXT_DOUT: dL/dy = fp16(dout * dout_scale) (the torch binding's loss scale; 1: as given)
	const _Float16* enc;    // ENC_MEM: the encoding kept by the forward, SoA [IN][B] (no gathers; with dout only)
	unsigned long long* prof;  // diagnostic build only: per-wave phase cycle sums [waves][8]
	// optional [L][B/32]: per (level, 32-sample slice) the fp32 sum of max_f |dL/denc| as stored -- the
	// grid backward's fixed-point range without its pass over dLdenc (grid_bwd_lds.h); null: not emitted
	float* dy_bound;
	uint32_t wt_stores;     // WT_WGRAD_SLAB (wt_store.h): the slab store writes through L2 (wave-uniform)
};
// g: the grid (D, hash, levels, hash_grid, interp and opts.inrange_index are read); n_blocks: fused_train_n_blocks
void launch_fused_train(hipStream_t st, const GridCall& g, uint32_t W, uint32_t IN, uint32_t NH, int act, FusedTrainArgs a,
                        uint32_t n_blocks);
// LDS weight image of the fused kernels, built once per parameter update.
size_t fused_weight_image_bytes(uint32_t W, uint32_t IN, uint32_t NH);
void launch_pack_weights(hipStream_t st, uint32_t W, uint32_t IN, uint32_t NH, const void* params16, void* image);

// Forward-only MLP (inference): in fp16 SoA [IN][B] or AoS [B][IN] -> out fp16 [B][16].
bool mlp_infer_supported(uint32_t W, uint32_t IN, uint32_t NH, uint32_t OUTP, int act);
// grid encoding + MLP forward in one kernel (k_fused_fwd_grid); wimage null: the LDS image is built from
// params16 (16-byte aligned); enc16 (nullable) receives the SoA encoding
void launch_fused_fwd(hipStream_t st, const GridCall& g, uint32_t W, uint32_t IN, uint32_t NH, int act, uint32_t B,
                      const void* wimage, const void* params16, const void* table16, const float* pos, void* enc16, void* out16);
void launch_mlp_infer(hipStream_t st, uint32_t W, uint32_t IN, uint32_t NH, int act, bool soa, uint32_t B,
                      const void* wimage, const void* in16, void* out16);
// out[b*n_out + o] = (float)in[b*in_stride + o]  (reference trim_and_cast_from, object.cu:60-67)
void launch_trim_cast(hipStream_t st, uint32_t B, uint32_t in_stride, uint32_t n_out, const void* in16, float* out);

// Grid forward (standalone; reference kernel_grid layout): out SoA [(l*F+f)*B + i] when soa, else
// AoS [i*out_stride + l*F + f].
void launch_grid_fwd(hipStream_t st, const GridCall& g, uint32_t B, const float* pos, uint32_t pos_stride, const void* table16,
                     void* out16, bool soa, uint32_t out_stride, uint32_t aos_row_cols = 0);

// Grid backward: dLdy layout 0 = level-major pairs ([l][i][F] halves), 1 = SoA ([(l*F+f)*B + i]),
// 2 = AoS ([i*dy_stride + l*F + f]).
uint32_t grid_bwd_slot_budget();
// host_slices / host_levels: the host copies of the work plan and of the g.L levels, passed by value as
// kernel arguments when they fit (grid_bwd_lds.h GridBwdTables)
void launch_grid_bwd(hipStream_t st, const GridCall& g, uint32_t B, const float* pos, uint32_t pos_stride, const void* dLdy16,
                     int dy_layout, uint32_t dy_stride, const GridSlice* slices, uint32_t n_slices, uint32_t n_chunks, float* partial,
                     uint32_t partial_stride, const GridBwdEpilogue* ep = nullptr, const GridSlice* host_slices = nullptr,
                     const LevelInfo* host_levels = nullptr,
                     // dy_bound (layout 0 only): [L][B/32] slice sums of max_f |dL/dy| written by the fused kernel that
                     // wrote dLdy16 (launch_fused_train) -- the streaming pre-pass of grid_bwd_lds.h; null: the exact one
                     const float* dy_bound = nullptr,
                     uint32_t wt_stores = 0);  // WT_GRID_SLAB (wt_store.h): the chunk slabs are written through L2
// Debug (debug_api.h): count the workgroups of every following launch_grid_bwd that were given
// dy_bound but took the exact pre-pass; the count of the last launch (synchronises the device).
void grid_bwd_debug_count_fallbacks(bool on);
uint32_t grid_bwd_debug_fallbacks();
// Binned backward, pass 1: counting-sort the updates of the binned levels by slice (GridBinArgs).
void launch_grid_bin(hipStream_t st, const GridCall& g, uint32_t B, const float* pos, uint32_t pos_stride, const void* dLdy16,
                     int dy_layout, uint32_t dy_stride, const GridBinArgs& a);
// Binned backward, pass 2: one workgroup per slice sums its records in LDS (int32 fixed point scaled
// by the level's sum of |dL/dy|) and writes the fp32 gradient of grid parameter p to grad32[p] (grid
// parameter order) or, with adam != nullptr, applies Adam to parameter param_base + p.
struct GridAccAdam {
	AdamArgs a;
	AdamBuffers buf;
	uint32_t param_base;
	int write_grad32;  // also store the fp32 sum into buf.g32
};
void launch_grid_acc(hipStream_t st, const GridCall& g, uint32_t B, const void* dLdy16, int dy_layout, uint32_t dy_stride,
                     const GridBinArgs& a, float* grad32, const GridAccAdam* adam);

// The launchers below are typed on the module's precision T (_Float16, or float for an fp32 encoding
// module: Encoding dtype = float32): the type of the table / the encoded rows / dL/dy. Both forms are
// instantiated where the kernels are; the arithmetic in between is fp32 in both.

// dL/dx fp32 [B][dx_stride] through the grid (reference grid.h:171-211 + 322-349), dy_dx recomputed
// from the table; dLdy in the launch_grid_bwd layouts (fp32: AoS rows only, dy_layout 2).
template <typename T>
void launch_grid_bwd_input(hipStream_t st, const GridCall& g, uint32_t B, const float* pos, uint32_t pos_stride, const T* table,
                           const T* dLdy, int dy_layout, uint32_t dy_stride, float* dx, uint32_t dx_stride);
// Second-order grid gradients (reference grid.h:351-627, 902-1026): from dL/d(dL/dx) fp32 [B][D]
// and dL/dy (AoS [B][dy_stride], nullable) -> grad32 += dL/dgrid (fp32 atomics, nullable),
// dL/d(dL/dy) AoS [B][ddy_stride] (nullable), dL/dx fp32 [B][D] (nullable).
template <typename T>
void launch_grid_bwd_bwd(hipStream_t st, const GridCall& g, uint32_t B, const float* pos, uint32_t pos_stride, const T* table,
                         const float* dL_ddLdx, const T* dLdy, uint32_t dy_stride, float* grad32, T* dLddLdy, uint32_t ddy_stride,
                         float* dx);
// fused weight-image geometry (FusedLayout) for the epilogue
void fused_image_layout(uint32_t W, uint32_t IN, uint32_t NH, uint32_t* RSI, uint32_t* RSW, uint32_t* oWh, uint32_t* oWo);

// out[c] = sum_j in[j*N + c] in block_column_sums order (G = 16 column blocks of 1024 threads):
// the network-gradient reduction of the sequential path, identical to the grid-backward tail's
void launch_column_sums(hipStream_t st, const float* in, uint32_t n_parts, uint32_t N, float* out);
// workgroups of the grid backward's network-gradient tail = column blocks of launch_column_sums (the
// same G in both keeps the two reductions' summation order identical); TCNN_MLP_TAIL_GROUPS overrides
uint32_t mlp_tail_groups();
// out[p] = sum_j in[j*stride + grid_slab_index(map, p)] (the grid backward's slabs, fixed order)
void launch_grid_slab_reduce(hipStream_t st, const float* in, uint32_t n_parts, uint32_t stride, uint32_t n, float* out,
                             const GridSlabMap* map, GradFinalize fin = {});
// out[p] = sum_j in[j*stride + p] (p < n). tmp: caller-owned device scratch of
// reduce_partials_tmp_floats(n_parts, n) floats (per workspace, so concurrent modules / streams /
// devices never share it)
size_t reduce_partials_tmp_floats(uint32_t n_parts, uint32_t n);
void launch_reduce_partials(hipStream_t st, const float* in, uint32_t n_parts, uint32_t stride, uint32_t n,
                            float* out, float* tmp);

// ---- tile engine (mlp_tile.h): fused MLP for W in {16, 32, 64, 128}, IN in {16, 32, 64, 128},
// 1..5 hidden layers, hidden activation None / ReLU, any output activation; encoded input fp16 [B][IN] ----
uint32_t tile_train_lds_bytes(uint32_t W, uint32_t IN, uint32_t NH);
bool tile_train_supported(uint32_t W, uint32_t IN, uint32_t NH, uint32_t outp, int act);
uint32_t tile_train_blocks(uint32_t B, uint32_t W, uint32_t IN, uint32_t NH);
// hidden matrices whose weights do not fit the LDS beside the rest (e.g. W128/H5/IN128: 2) are read from
// L2; their transposed copy needs tile_train_wT_bytes of device memory (0: every matrix is staged)
uint32_t tile_train_n_streamed(uint32_t W, uint32_t IN, uint32_t NH);
uint32_t tile_train_wT_bytes(uint32_t W, uint32_t IN, uint32_t NH);
// The kernel argument of the tile train step, filled by the host that launches it (value-initialise it);
// launch_mlp_tile_train sets n_total.
struct TileTrainArgs {
	uint32_t B, dims, loss_type;  // loss_type: LossType (loss_device.h)
	float loss_scale, n_total;
	int out_act;             // output activation (ACT_*), applied after the output layer, transfer before the backward
	const _Float16* params;  // [W0 | hidden | Wout] fp16 (unpadded width WR)
	// streamed hidden matrices 1..NS transposed, [NS][W (in)][W (out)] fp16: tile_train_wT_bytes of scratch
	// (nullptr when 0), rewritten from params by the launch
	const _Float16* wT;
	const _Float16* enc;     // encoded input fp16 [B][IN]
	const float* target;     // [B][dims] (loss)
	const _Float16* dout;    // external dL/d(output) fp16 [B][16] (loss-scaled by the caller; nullptr: the loss)
	_Float16* out;           // optional network output fp16 [B][16]
	void* dldenc;            // optional dL/d(encoding): pairs [IN/2][B] (uint32) or AoS fp16 [B][IN]
	int dldenc_pairs;
	float* wgrad_partial;    // [gridDim.x][N_MLP] (tile_train_blocks slabs)
	float* loss_partial;     // [gridDim.x]
};
void launch_mlp_tile_train(hipStream_t st, uint32_t W, uint32_t IN, uint32_t NH, int act, TileTrainArgs a);
// forward only (the reference's INFERENCE instantiation): enc16 fp16 [B][IN] -> out16 fp16 [B][16]
bool tile_infer_supported(uint32_t W, uint32_t IN, uint32_t NH, uint32_t outp, int act);
uint32_t tile_infer_blocks(uint32_t B, uint32_t W, uint32_t IN, uint32_t NH);
void launch_mlp_tile_infer(hipStream_t st, uint32_t W, uint32_t IN, uint32_t NH, int act, int out_act, uint32_t B, const void* params16,
                           const void* enc16, void* out16);

// generate_random_uniform<float> (random.h:57-70) from pcg32 {state, inc} (not advanced here)
void launch_generate_uniform(hipStream_t st, uint64_t n, uint64_t state, uint64_t inc, float* out, float lo, float hi);
void launch_generate_logistic(hipStream_t st, uint64_t n, uint64_t state, uint64_t inc, float* out, float mean, float stddev);
// pert16[i] = fp16(out16[i] + noise[i]) (the Trainer's output perturbation)
void launch_add_perturbation(hipStream_t st, uint32_t n, const void* out16, const float* noise, void* pert16);
void launch_adam(hipStream_t st, const AdamArgs& a, float* w32, void* w16, const float* grad32, void* grad16,
                 float* m1, float* m2, uint32_t* steps);
// What a lean launch_adam (ADAM_LEAN_GRADS) left out, from the slabs it summed: grad32[p] = the fixed-order
// slab sum, grad16[p] = f16_rn(sum * grad_scale), p < n -- the values and bits k_adam stores.
void launch_grid_slab_gradients(hipStream_t st, const float* in, uint32_t n_parts, uint32_t stride, uint32_t n, const GridSlabMap* map,
                                float grad_scale, float* grad32, void* grad16);
// steps[256 b + k] = step_blocks[b] for every block b < n_blocks whose word is a count (k < 256, 256 b + k < n)
void launch_adam_steps_expand(hipStream_t st, const uint32_t* step_blocks, uint32_t n, uint32_t* steps);

void launch_cast_f32_f16(hipStream_t st, const float* in, void* out, size_t n);
void launch_cast_f16_f32(hipStream_t st, const void* in, float* out, size_t n);
// loss-scale arithmetic of the torch binding (modules.py:128-137): out = fp16(in * s); x /= s (fp32);
// out = fp16(in / s), stored as fp16 or widened to fp32
void launch_scale_f16(hipStream_t st, const void* in, void* out, float s, size_t n);
void launch_div_f32(hipStream_t st, float* x, float s, size_t n);
// out = in * s in fp32: dL/dy * loss_scale of an fp32 encoding module (its gradients take launch_div_f32)
void launch_scale_f32(hipStream_t st, const float* in, float* out, float s, size_t n);
void launch_div_f16(hipStream_t st, const void* in, void* out, float s, size_t n, bool out_f32);
void launch_grad_finalize(hipStream_t st, const float* g, void* out, float s, size_t n, bool out_f32);

// RelativeL2 (standalone, reference relative_l2.h:40-76): pred fp16 [B][stride] -> values, grads
void launch_relative_l2(hipStream_t st, uint32_t B, uint32_t stride, uint32_t dims, float loss_scale,
                        const void* pred16, const float* target, float* values, void* grads16);

void launch_sum(hipStream_t st, const float* in, uint32_t n, float* out);

// ---- layer-wise MFMA MLP (mlp_layers.hip); activations sample-major fp16 [B][width] ----
bool layered_width_supported(uint32_t w);
// y[B][N] = act(x[B][K] w^T), w row-major [N][K]
void launch_layer_fwd(hipStream_t st, uint32_t B, uint32_t N, uint32_t K, const void* w16, const void* x16, void* y16, int act);
// dx[B][K] = act'(h) * (dy[B][N] w); h == nullptr: no transfer
// pairs = true (no transfer only): dX written as level-major fp16 pairs [K/2][B] (grid F = 2 encodings)
void launch_layer_bwd(hipStream_t st, uint32_t B, uint32_t N, uint32_t K, const void* w16, const void* dy16, const void* h16,
                      void* dx16, int act, bool pairs = false);
// in-place output-activation transfer: g[i] = act'(y[i]) g[i] over n elements
void launch_act_bwd_inplace(hipStream_t st, uint32_t n, int act, const void* y16, void* g16);
// partial[chunk][N][K] = sum over the chunk's samples of dy[i][n] x[i][k]
uint32_t wgrad_n_chunks(uint32_t B);
void launch_wgrad(hipStream_t st, uint32_t B, uint32_t N, uint32_t K, const void* dy16, const void* x16, float* partial,
                  uint32_t n_chunks);
uint32_t relative_l2_n_blocks(uint32_t B, uint32_t stride);
void launch_relative_l2_partial(hipStream_t st, uint32_t B, uint32_t stride, uint32_t dims, float loss_scale, const void* pred16,
                                const float* target, void* grads16, float* loss_partial, uint32_t loss_type = 0,
                                const float* pdf = nullptr, float* values = nullptr);  // loss_type: LossType (loss_device.h)
// out[i] += in[i] (Accumulate-mode gradients)
void launch_add_f32(hipStream_t st, const float* in, float* out, size_t n);

// ---- OneBlob / Identity encodings (encodings.hip); output AoS [B][out_stride] of T (_Float16 / float), padding = 1 ----
template <typename T>
void launch_oneblob_fwd(hipStream_t st, uint32_t B, uint32_t D, uint32_t n_bins, const float* x, uint32_t x_stride, T* out,
                        uint32_t out_stride, uint32_t n_pad);
// dL/dx fp32 [B][x_stride] from dL/dy AoS (kernel_one_blob_backward, oneblob.h:116-147)
template <typename T>
void launch_oneblob_bwd(hipStream_t st, uint32_t B, uint32_t D, uint32_t n_bins, const float* x, uint32_t x_stride, const T* dy,
                        uint32_t dy_stride, float* dx, uint32_t dx_stride);
template <typename T>
void launch_identity_fwd(hipStream_t st, uint32_t B, uint32_t D, float scale, float offset, const float* x, uint32_t x_stride, T* out,
                         uint32_t out_stride, uint32_t n_pad);
template <typename T>
void launch_identity_bwd(hipStream_t st, uint32_t B, uint32_t D, float scale, const T* dy, uint32_t dy_stride, float* dx,
                         uint32_t dx_stride);

// Composite encodings (composite.hip; reference encodings/composite.h with Concatenation, and
// spherical_harmonics.h / triangle_wave.h): the parts of one encoded AoS row [B][width]. A part reads
// input columns [in_col, in_col + n_in) and owns output columns [out_col, out_col + width): n_values
// encoded values and width - n_values padding columns (SphericalHarmonics: 1, before the values;
// TriangleWave / OneBlob / Identity: 1, after them; grid: 0, after them). The table travels by value.
enum : uint32_t { COMP_SH = 0, COMP_TRIANGLE = 1, COMP_ONEBLOB = 2, COMP_IDENTITY = 3, COMP_GRID = 4 };
constexpr uint32_t COMP_MAX_PARTS = 16, COMP_MAX_INPUTS = 64, COMP_MAX_WIDTH = 256;
constexpr uint32_t COMP_SLOT_ZERO = 0xFF;
struct CompPart {
	uint32_t kind, in_col, n_in, out_col, width, n_values;
	uint32_t p0;     // SH degree | TriangleWave n_frequencies | OneBlob n_bins
	uint32_t p1;     // OneBlob log2(n_bins)
	float f0, f1;    // Identity scale, offset
};
struct CompTable {
	uint32_t n_parts, n_in, width;
	uint32_t fwd_work;  // any column that k_composite_fwd writes
	CompPart parts[COMP_MAX_PARTS];
	uint32_t grid_cols[COMP_MAX_WIDTH / 32];  // bit c: column c holds a nested grid's value (its own launch writes it)
	// backward work: slot s is (part, input column) -- one per SH part, one per input column of the other
	// parameter-free parts, and (COMP_SLOT_ZERO, column) for every input column that no part reads
	uint32_t n_slots;
	uint8_t slot_part[COMP_MAX_INPUTS], slot_col[COMP_MAX_INPUTS];
};
// every column of every row that no nested grid's own forward writes (values of the parameter-free
// parts and all padding, the grids' included): one launch; out AoS [B][t.width] of T (_Float16 / float)
template <typename T>
void launch_composite_fwd(hipStream_t st, uint32_t B, const float* x, T* out, const CompTable& t);
// dL/dx fp32 [B][n_in] of the parameter-free parts' columns and zeros in the unread columns (plain
// stores); dy AoS [B][dy_stride]
template <typename T>
void launch_composite_bwd_input(hipStream_t st, uint32_t B, const float* x, const T* dy, uint32_t dy_stride, float* dx,
                                const CompTable& t);

// ---- fp32-precision encoding modules (Encoding dtype = float32): the float forms of the typed
// launchers above, and in grid_f32.hip the grid forward and parameter backward, which are kernels of
// their own (the fp16 forward is packed-fp16 arithmetic, the fp16 backward reads three dL/dy layouts).
// Tables, encoded rows AoS [B][stride], dL/dy and dL/d(dL/dy) are fp32 and nothing in between is
// narrowed to fp16; dL/dy is always AoS rows. ----
// only the value columns [0, L * F) of each row are written
void launch_grid_fwd_f32(hipStream_t st, const GridCall& g, uint32_t B, const float* pos, uint32_t pos_stride, const float* table32,
                         float* out32, uint32_t out_stride);
// LDS-privatised backward: items with all F features (slabs in parameter order), partial [n_chunks][partial_stride]
void launch_grid_bwd_f32(hipStream_t st, const GridCall& g, uint32_t B, const float* pos, uint32_t pos_stride, const float* dLdy32,
                         uint32_t dy_stride, const GridSlice* slices, uint32_t n_slices, uint32_t n_chunks, float* partial,
                         uint32_t partial_stride);

// ---- fp32 network modules (Network / NetworkWithInputEncoding dtype = float32; mlp_f32.hip): the layer-wise
// engine on the f32 MFMA. Weights [N][K], rows AoS [B][width], all fp32; N and K multiples of 16, B of 128. ----
// y[B][N] = act(x[B][K] w^T)
void launch_f32_layer_fwd(hipStream_t st, uint32_t B, uint32_t N, uint32_t K, const float* w, const float* x, float* y, int act);
// dx[B][K] = (dy[B][N] o act'(yv)) w; yv: the forward value beside dy (unread for ACT_NONE). The transfer runs in the operand load.
void launch_f32_layer_bwd(hipStream_t st, uint32_t B, uint32_t N, uint32_t K, const float* w, const float* dy, const float* yv, int act,
                          float* dx);
// partial[slab][N][K] = sum over the slab's rows of (dy o act'(yv))^T x; f32_wgrad_n_slabs(B) slabs of
// f32_wgrad_slab_rows(B) rows, which launch_reduce_partials sums in a fixed order
uint32_t f32_wgrad_slab_rows(uint32_t B);
uint32_t f32_wgrad_n_slabs(uint32_t B);
void launch_f32_wgrad(hipStream_t st, uint32_t B, uint32_t N, uint32_t K, const float* dy, const float* yv, int act, const float* x,
                      float* partial);
// The second-order input gradient (NetworkF32Host::backward_backward_input). An activation has curvature when
// act'' is not identically zero: None, ReLU and LeakyReLU have none.
inline bool f32_act_has_curvature(int act) {
	return act == ACT_EXPONENTIAL || act == ACT_SIGMOID || act == ACT_SQUAREPLUS || act == ACT_SOFTPLUS || act == ACT_TANH;
}
// tangent layer: with t = x[B][K] w^T, y[B][N] = t o act'(yv) and, when r is given (an activation with curvature),
// r[B][N] = t o d o act''(yv); yv: the layer's forward value, d: dL/d(that value) of the first-order backward
void launch_f32_layer_tangent(hipStream_t st, uint32_t B, uint32_t N, uint32_t K, const float* w, const float* x, const float* yv, int act,
                              float* y, const float* d, float* r);
// curvature layer: q_below[B][K] = (q[B][N] w) o act'(yv_below) + r_below (r_below nullable; q_below may be r_below)
void launch_f32_layer_curvature(hipStream_t st, uint32_t B, uint32_t N, uint32_t K, const float* w, const float* q, const float* yv_below,
                                int act_below, const float* r_below, float* q_below);
// Identity in front: u0[B][width] = scale * u_x[B][D] in the first D columns, 0 in the padding
void launch_f32_identity_tangent(hipStream_t st, uint32_t B, uint32_t D, uint32_t width, float scale, const float* u_x, float* u0);
// dst[i] += src[i], i < n
void launch_f32_add(hipStream_t st, size_t n, float* dst, const float* src);

void launch_probe_hfma(hipStream_t st, const void* a, const void* b, const void* c, void* out, uint32_t n_pairs);
// Diagnostic: the config_hash fused (pipelined) kernel with s_memtime phase stamps (prof: [blocks*8][8] u64).
void launch_fused_train_profile(hipStream_t st, uint32_t B, uint32_t dims, const void* params16, const void* table16,
                                const float* pos, const float* target, void* dLdenc, float* wgrad_partial,
                                float* loss_partial, const LevelInfo* levels, uint32_t n_blocks, const void* wimage,
                                unsigned long long* prof);
// Debug probe: runs one MFMA 16x16x32 f16 and two ds_read_b64_tr_b16 with known data.
void launch_probe(hipStream_t st, float* mfma_out, int16_t* tr_out);

}  // namespace tcnn_amd
