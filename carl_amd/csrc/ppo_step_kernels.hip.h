// ppo_step_kernels.hip.h -- the kernels of PPO's minibatch step (include/carl_amd.h: carl_ppo_adv_stats, carl_adam_step).
// Included by carl_ppo_step.hip only, so the library holds one definition of each.  The constants, the workgroup sum and the
// argument structs are ppo_step_device.hip.h's; each kernel's body is a file of its own (ppo_adv_stats_body.inc,
// adam_step_body.inc) that the population kernels (ppo_sets_kernels.hip.h) include too.
//
// Both kernels sum in float64 in an order that is a fixed function of the launch shape: a thread chains its own elements
// in index order, a wavefront adds its 64 values by a shuffle tree, thread 0 adds the wavefronts' sums from LDS in
// wavefront order.  No floating-point atomics, no hand-over between workgroups: the same call twice gives the same bits.
// Floating-point contraction is off in both, so every product and every sum is rounded on its own.
#pragma once

#include "ppo_step_device.hip.h"

namespace carl {

// Preconditions (host, carl_ppo_step.hip): n_total >= 1, batch_size >= 1, gridDim.x == ceil(n_total / batch_size)
__global__ void __launch_bounds__(kAdvThreads) ppo_adv_stats_kernel(const PpoAdvStatsArgs a) {
#pragma clang fp contract(off)
#define ADV_MB_IDX a.idx
#define ADV_MB_ADV_NORM a.adv_norm
#include "ppo_adv_stats_body.inc"
#undef ADV_MB_IDX
#undef ADV_MB_ADV_NORM
}

// Preconditions (host): gridDim.x == 1; the tensors' elements together <= kAdamMaxFloats
__global__ void __launch_bounds__(kAdamThreads) adam_step_kernel(const AdamArgs a) {
#pragma clang fp contract(off)
#define ADAM_MB_ROW(first_row, t) first_row
#define ADAM_MB_STEP a.step
#define ADAM_MB_BETA_POW a.beta_pow
#define ADAM_MB_NORM_OUT a.norm_out
#define ADAM_MB_LR a.lr
#define ADAM_MB_MAX_GRAD_NORM a.max_grad_norm
#include "adam_step_body.inc"
#include "adam_step_body_undef.inc"
}

}  // namespace carl
