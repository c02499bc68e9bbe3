/* debug_adam.h -- TEST-ONLY diagnostic of the trainer's lean grid Adam (TCNN_ADAM_LEAN), a companion of
 * debug_api.h like debug_grid_bwd.h: not part of the product C-ABI (include/tcnn_mi355x.h), no product code
 * path calls it and it may change without notice. Used by tests/test_gpu_adam_lean.py, which declares the
 * ctypes signature itself. */
#ifndef TCNN_DEBUG_ADAM_H
#define TCNN_DEBUG_ADAM_H
#include "../../include/tcnn_mi355x.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Block step counts of the trainer's Adam over the grid slabs (TCNN_ADAM_LEAN bit 2; kernels.h AdamArgs):
 * n_blocks = 256-parameter blocks of that range, n_uniform = those whose parameters share one count kept in
 * the block's word (the others keep per-parameter counts). Waits for the stream of the last step; changes
 * nothing. A trainer that keeps per-parameter counts (the bit off, or after tcnn_trainer_optimizer_state)
 * reports the words as the last step with block counts left them. */
int tcnn_debug_adam_uniform_blocks(tcnn_trainer* t, uint32_t* n_uniform, uint32_t* n_blocks);

#ifdef __cplusplus
}
#endif
#endif /* TCNN_DEBUG_ADAM_H */
