// dqn_slots_internal.hpp -- the image form of uavenv_dqn_act_slots, shared by learner.hip and the slots loop (loop.hip); like the
// entry points of dqn_internal.hpp it is NOT part of the C ABI (include/uavenv.h), whose entry forwards here with no images.
#pragma once
#include <stdint.h>

#include "../../include/uavenv.h"

extern "C" {

// uavenv_dqn_act_slots with the images of the nets as they are now: images[j] (host array; nullable as a whole and per net) =
// uavenv_dqn_split_image's output for nets[j], of which the q_local half is staged.
int uavenv_dqn_act_slots_img(const UavDqnNet *const *nets, int32_t n_nets, const void *obs_dev, int32_t obs_dtype, int32_t n_envs,
                             float eps, uint64_t seed, uint64_t counter, int32_t *index_out_dev, float *q_out_dev,
                             const float *const *images, void *stream);

}  // extern "C"
