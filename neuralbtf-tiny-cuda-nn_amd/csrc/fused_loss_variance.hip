// fused training kernels with the LOSS_VARIANCE loss inside (see fused_loss_tu.h)
#define TCNN_FUSED_LOSS LOSS_VARIANCE
#include "fused_loss_tu.h"
