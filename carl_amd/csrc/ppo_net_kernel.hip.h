// ppo_net_kernel.hip.h -- ppo_net_kernel<H>, the network kernel of the PPO update on the device: the classic unit's actor
// and critic, the Brax unit's critic.  Each of the two units instantiates it through ppo_host.hpp's launch_ppo_net (the
// Brax unit's instances are compiled beside its actor kernel: profiles/ppo_refactor_identity.txt on why they stay).  The
// device functions of policy_kernels.hip.h (dense_layer, head_layer, activate, tanh_fast, normalize_input) are called,
// none is changed, so every earlier kernel compiles to the code it had (profiles/ppo_isa_identity.txt).
//
// ppo_net_kernel<H> runs ONE network (the actor or the critic: `kind`) over a minibatch.  H is the padded hidden width
// (0: a linear network, 32, 64); nothing depends on the family: input slot i is packed input i (the context inputs,
// then the observation), padded with zeros to kPpoK = CARL_POLICY_MAX_IN slots.  The rollout's layout keeps the
// observation at slot F + d instead; the zero weights between the two halves there add fma(0, 0, acc) = acc, so the
// arithmetic per output is the same sequence of fmas and the forward pass has the rollout's bits (up to the sign of a
// zero sum).  Per tile: the forward pass, the loss and dL/dy, the backward pass (ppo_device.hip.h's header comment).
// The body is ppo_net_body.inc, which the population kernel (ppo_sets_kernels.hip.h) includes too.
#pragma once

#include "ppo_device.hip.h"

namespace carl {

// Preconditions (host, ppo_host.hpp): the batch and both networks validated; H the padded width of THIS network
// (0 iff it has no hidden layer); gridDim.x <= n_tiles; the dynamic LDS is ppo_lds_bytes(H).
template <int H>
__global__ void __launch_bounds__(kPpoThreads) ppo_net_kernel(const PpoNetArgs a) {
#define PPO_MB_LANE_WINDOW false  // (one learner: every lane of the buffer is its own)
#define PPO_MB_LANE_LO 0
#define PPO_MB_LANE_HI 0
#define PPO_MB_PARAMS a.params
#define PPO_MB_XFORM a.xform
#define PPO_MB_LOG_STD a.log_std
#define PPO_MB_SLAB a.slab
#define PPO_MB_NEW_OUT a.new_out
#define PPO_MB_IDX b.idx
#define PPO_MB_ADV_NORM b.adv_norm
#define PPO_MB_CLIP_RANGE b.clip_range
#define PPO_MB_VF_COEF b.vf_coef
#define PPO_MB_ENT_COEF b.ent_coef
#include "ppo_net_body.inc"
#include "ppo_net_body_undef.inc"
}

}  // namespace carl
