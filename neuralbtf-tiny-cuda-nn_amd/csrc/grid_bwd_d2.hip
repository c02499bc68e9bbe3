// grid_bwd_d2.hip -- LDS-privatised grid backward instantiated for D = 2 (grid_bwd_lds.h)
#include "grid_bwd_lds.h"

namespace tcnn_amd {
template void grid_bwd_d<2>(hipStream_t, uint32_t, HashType, const GridBwdLaunch&);
}  // namespace tcnn_amd
