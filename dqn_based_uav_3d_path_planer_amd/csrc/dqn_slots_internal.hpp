// dqn_slots_internal.hpp -- the image forms of uavenv_dqn_act_slots, uavenv_dqn_grad_slots and uavenv_dqn_reduce_adam_slots, shared by
// learner.hip and the slots loop (loop.hip); like the entry points of dqn_internal.hpp they are NOT part of the C ABI
// (include/uavenv.h), whose entries forward here with no images.
#pragma once
#include <stdint.h>

#include "../../include/uavenv.h"

extern "C" {

// uavenv_dqn_act_slots with the images of the nets as they are now: images[j] (host array; nullable as a whole and per net) =
// uavenv_dqn_split_image's output for nets[j], of which the q_local half is staged.
int uavenv_dqn_act_slots_img(const UavDqnNet *const *nets, int32_t n_nets, const void *obs_dev, int32_t obs_dtype, int32_t n_envs,
                             float eps, uint64_t seed, uint64_t counter, int32_t *index_out_dev, float *q_out_dev,
                             const float *const *images, void *stream);

// uavenv_dqn_grad_slots with the images of the nets as they are now (images[j] as above): with one for EVERY slot both layer-1
// images of every slot come in by LDS-DMA, as uavenv_dqn_grad_img stages them; otherwise a slot without one converts fc1 itself.
int uavenv_dqn_grad_slots_img(const UavReplayRing *ring, int32_t head, int32_t filled, int32_t batch, uint64_t seed, uint64_t counter,
                              const int32_t *pairs_dev, const UavDqnNet *const *nets, int32_t n_nets, int32_t kind, float gamma,
                              int32_t huber, float *const *partials, const float *const *images, void *stream);

// uavenv_dqn_grad_slots_w with the images of the nets as they are now (images[j] as above).
int uavenv_dqn_grad_slots_w_img(const UavReplayRing *ring, int32_t head, int32_t filled, int32_t batch, uint64_t seed, uint64_t counter,
                                const int32_t *pairs_dev, const UavDqnNet *const *nets, int32_t n_nets, int32_t kind, float gamma,
                                int32_t huber, const float *is_weights_dev, float *abs_td_out_dev, float *const *partials,
                                const float *const *images, void *stream);

// uavenv_dqn_reduce_adam_slots that keeps images[j] current with the new parameters (uavenv_dqn_reduce_adam_img per slot), and
// writes slot j's column sums to raw_out[j] (host array, nullable as a whole and per net) as uavenv_dqn_reduce_adam's raw_out.
int uavenv_dqn_reduce_adam_slots_img(const UavDqnNet *const *nets, int32_t n_nets, float *const *partials, int32_t n_partials,
                                     float lr, float beta1, float beta2, float eps, const int32_t *step_t, const int32_t *hard_update,
                                     float *const *loss_out, float *const *raw_out, const uint32_t *go_word_dev, uint32_t go_value,
                                     float *const *images, void *stream);

}  // extern "C"
