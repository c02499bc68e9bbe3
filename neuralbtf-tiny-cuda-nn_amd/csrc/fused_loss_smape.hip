// fused training kernels with the LOSS_SMAPE loss inside (see fused_loss_tu.h)
#define TCNN_FUSED_LOSS LOSS_SMAPE
#include "fused_loss_tu.h"
