// The fused training kernel for one of the seven losses beyond RelativeL2 / L2
// (k_fused_train_grid_loss, mlp_fused.h): its instantiations and their launcher, one translation unit
// per loss (fused_loss_*.hip define TCNN_FUSED_LOSS and include this) so they compile in parallel.
#include "kernels.h"

#include "grid_device.h"
#include "grid_dispatch.h"
#include "mlp_fused.h"

// the shapes instantiated for this loss (fused_train_loss_supported in fused.hip says the same)
#ifndef TCNN_FUSED_LOSS_SHAPES
#define TCNN_FUSED_LOSS_SHAPES(X) TCNN_FUSED_SHAPES(X)
#endif

namespace tcnn_amd {

template <int W, int IN, int NH, uint32_t D, HashType H, Act A>
static void launch_fused_loss_t(hipStream_t st, const FusedTrainArgs& args, uint32_t n_blocks) {
	constexpr size_t bytes = RegKernelLayout<W, IN, NH>::BYTES;
	static uint64_t done = 0;
	set_dyn_lds((const void*)k_fused_train_grid_loss<W, IN, NH, D, H, A, TCNN_FUSED_LOSS>, (int)bytes, done);
	hipLaunchKernelGGL((k_fused_train_grid_loss<W, IN, NH, D, H, A, TCNN_FUSED_LOSS>), dim3(n_blocks), dim3(64 * FUSED_WAVES), bytes, st, args);
	TCNN_HIP_CHECK(hipGetLastError());
}

template <int W, int IN, int NH>
static void launch_fused_loss_shape(hipStream_t st, uint32_t D, HashType h, int act, const FusedTrainArgs& a, uint32_t nb) {
	with_grid_hash(h, [&](auto hh) {
		constexpr HashType H = decltype(hh)::value;
		if (D == 2) {
			if (act == 1) launch_fused_loss_t<W, IN, NH, 2, H, Act::ReLU>(st, a, nb);
			else launch_fused_loss_t<W, IN, NH, 2, H, Act::None>(st, a, nb);
		} else {
			if (act == 1) launch_fused_loss_t<W, IN, NH, 3, H, Act::ReLU>(st, a, nb);
			else launch_fused_loss_t<W, IN, NH, 3, H, Act::None>(st, a, nb);
		}
	});
}

template <>
bool launch_fused_train_loss<TCNN_FUSED_LOSS>(hipStream_t st, uint32_t W, uint32_t IN, uint32_t NH, uint32_t D, HashType h, int act,
                                              const FusedTrainArgs& a, uint32_t n_blocks) {
	TCNN_CHECK(!a.dout && !a.enc && a.loss_type == (uint32_t)TCNN_FUSED_LOSS, "fused train: loss kernel launched with the wrong arguments");
	TCNN_CHECK(D == 2 || D == 3, "fused train: 2 or 3 input dimensions");
#define X(w, in, nh) if (W == w && IN == in && NH == nh) { launch_fused_loss_shape<w, in, nh>(st, D, h, act, a, n_blocks); return true; }
	TCNN_FUSED_LOSS_SHAPES(X)
#undef X
	return false;
}

}  // namespace tcnn_amd
