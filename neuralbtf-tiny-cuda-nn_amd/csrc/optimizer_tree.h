// optimizer_tree.h -- the optimizers that wrap or replace Adam (reference optimizers/sgd.h,
// exponential_decay.h, ema.h, lookahead.h, batched.h) as a host-side tree over the Trainer's
// buffers, and the launchers of their kernels (optimizers.hip). The innermost node is Adam (whose
// state and hyper-parameters stay where they are, in TrainerHost) or SGD. A trainer whose optimizer is
// plain Adam has no tree.
#pragma once

#include <string>

#include "common.h"
#include "optimizers.h"

namespace tcnn_amd {

enum class OptKind : int { Adam, SGD, ExponentialDecay, Ema, Lookahead, Batched };

// "Adam, SGD, ..." for error messages
std::string optimizer_otype_list();
// create_optimizer (src/optimizer.cu:49-80): the kind of an otype (case-insensitive); throws for the
// otypes the engine refuses (Average, Novograd, Composite, Shampoo) and for unknown ones
OptKind optimizer_kind_from_otype(const std::string& otype);

}  // namespace tcnn_amd
