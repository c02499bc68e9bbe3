/* debug_grid_bwd.h -- TEST-ONLY entry points of libtcnn_mi355x.so around the grid backward's streaming
 * pre-pass (grid_bwd_lds.h), a companion of debug_api.h: not part of the product C-ABI
 * (include/tcnn_mi355x.h), no product code path calls them, they may change without notice. Used by
 * tests/test_gpu_grid_bwd_stream.py. */
#ifndef TCNN_DEBUG_GRID_BWD_H
#define TCNN_DEBUG_GRID_BWD_H
#include "../../include/tcnn_mi355x.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Counting on: every following grid backward launch of the process counts its workgroups that were
 * given slice sums (dy_bound) but took the exact pre-pass -- inside the guard band, or a non-finite
 * sum. tcnn_debug_grid_bwd_fallbacks returns the count of the last launch (synchronises the device). */
int tcnn_debug_grid_bwd_count_fallbacks(int on);
int tcnn_debug_grid_bwd_fallbacks(uint32_t* count);
/* The last step's dL/d(encoding) (device [L][n] half2, as the fused kernel stored it) and slice sums
 * ([L][n/32] floats) copied to host buffers of dldenc_bytes / bound_bytes bytes; *bound_live = 0 when
 * the step emitted no slice sums (host_bound is then untouched). */
int tcnn_debug_step_dldenc(tcnn_trainer* t, void* host_dldenc, size_t dldenc_bytes, float* host_bound, size_t bound_bytes,
                           int* bound_live);
/* The LDS items of the trainer's grid backward on caller-supplied device buffers: dL/dy as level-major
 * pairs [L][n] half2 and (nullable) slice sums [L][n/32]; the chunk slabs ([*n_chunks][*slab_stride]
 * floats) are copied to host_slabs (slab_floats floats of room). */
int tcnn_debug_grid_backward_items(tcnn_trainer* t, void* stream, uint32_t n, const float* input, const void* dldy_pairs,
                                   const float* dy_bound, float* host_slabs, size_t slab_floats, uint32_t* n_chunks,
                                   uint32_t* slab_stride);

#ifdef __cplusplus
}
#endif
#endif /* TCNN_DEBUG_GRID_BWD_H */
