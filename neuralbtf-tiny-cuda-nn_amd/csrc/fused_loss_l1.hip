// fused training kernels with the LOSS_L1 loss inside (see fused_loss_tu.h)
#define TCNN_FUSED_LOSS LOSS_L1
#include "fused_loss_tu.h"
