// fused training kernels with the LOSS_MAPE loss inside (see fused_loss_tu.h)
#define TCNN_FUSED_LOSS LOSS_MAPE
#include "fused_loss_tu.h"
