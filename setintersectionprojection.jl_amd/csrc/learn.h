// Constraint learning from training images (the reference's constraint_learning_by_obseration,
// src/constraint_learning_by_observation.jl:8-163): a standalone batched pipeline over chunks of images, no engine context.
// See learn.hip and include/sipx.h (sipx_learn_observations) for the keys and their conventions.
#pragma once
#include <stdint.h>

#include "../../include/sipx.h"

namespace sipx {

void learn_observations_host(int dtype, const int64_t* n, const double* h, int64_t n_train, const void* m_train,
                             const int64_t* strides, int64_t max_batch, sipx_observations* out, int device);

}  // namespace sipx
