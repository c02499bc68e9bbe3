// fused training kernels with the LOSS_RELATIVE_L2_LUMINANCE loss inside (see fused_loss_tu.h).
// Not W64 with two hidden layers: that kernel uses all 256 registers and the luminance's cross-lane
// fetch made it spill 2-8 of them, however the fetch was arranged; such a network trains on the tile
// engine (fused_train_loss_supported, NetworkHost::fused_ok).
#define TCNN_FUSED_LOSS LOSS_RELATIVE_L2_LUMINANCE
#define TCNN_FUSED_LOSS_SHAPES(X) X(64, 32, 1) X(32, 32, 2) X(32, 32, 1)
#include "fused_loss_tu.h"
