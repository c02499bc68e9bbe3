// fused training kernels with the LOSS_CROSS_ENTROPY loss inside (see fused_loss_tu.h)
#define TCNN_FUSED_LOSS LOSS_CROSS_ENTROPY
#include "fused_loss_tu.h"
