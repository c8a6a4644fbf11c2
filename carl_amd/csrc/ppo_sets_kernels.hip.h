// ppo_sets_kernels.hip.h -- the kernels of a POPULATION of PPO learners (include/carl_amd.h: carl_ppo_grad_sets,
// carl_ppo_adv_stats_sets, carl_adam_step_sets).  Included by carl_ppo_sets.hip only.  Each kernel is an existing body run
// once per member: ppo_net_body.inc (ppo_net_kernel<H>'s), ppo_reduce_body.inc (ppo_reduce_kernel's), ppo_adv_stats_body.inc
// and adam_step_body.inc, included textually with the member's values in the place of the launch's arguments.  No body is
// restated and no existing kernel is instantiated here; the layout, the argument structs and the helpers are
// ppo_device.hip.h's and ppo_step_device.hip.h's.
//
// The grid is dim3(what ONE learner's launch has, n_sets): inside the body blockIdx.x / gridDim.x keep their meaning, so
// member s gets the workgroup count, the tile-to-workgroup mapping, the slab order and the sums of the one-set call on
// its n_samples samples, and blockIdx.y picks the member.  Everything read per member -- the hyper row, the packed
// parameters, log_std, the idx and adv_norm rows, the slabs -- is addressed from kernel arguments and blockIdx.y alone:
// wavefront-uniform and read-only, so the row's scalars arrive by scalar loads, once per workgroup, and cost no LDS.
#pragma once

#include "ppo_net_kernel.hip.h"
#include "ppo_step_device.hip.h"

namespace carl {

// what a population launch adds to one learner's arguments
struct PpoSetsArgs {
  const double* hyper;     // [n_sets][CARL_PPO_HYPER]
  const int32_t* idx;      // [n_sets][idx_stride]
  const float* adv_norm;   // row s at adv_norm + s * adv_stride: [2]; nullable
  long long idx_stride;
  long long adv_stride;
  long long slab_stride;   // floats between two members' slabs of THIS network: gridDim.x slabs
  int lanes_per_set;
  int xform_stride;        // floats between two members' packed ACTOR blocks (PpoNetArgs.xform is member 0's)
};

// float32 of a hyperparameter, rounded once: what carl_ppo_grad takes as a float
__device__ __forceinline__ float ppo_hyper_f32(const double* __restrict__ row, int col) { return (float)row[col]; }

// Preconditions (host, carl_ppo_sets.hip): ppo_net_kernel<H>'s for every member; `a` holds member 0's params, xform,
// log_std and slab; gridDim.y == n_sets; n_sets * lanes_per_set == a.b.n_lanes; the dynamic LDS is ppo_lds_bytes(H).
template <int H>
__global__ void __launch_bounds__(kPpoThreads) ppo_net_sets_kernel(const PpoNetArgs a, const PpoSetsArgs ps) {
  const int set = (int)blockIdx.y;
  const double* const hyper = ps.hyper + (size_t)set * CARL_PPO_HYPER;
  const float set_clip_range = ppo_hyper_f32(hyper, CARL_PPO_HYPER_CLIP_RANGE);
  const float set_vf_coef = ppo_hyper_f32(hyper, CARL_PPO_HYPER_VF_COEF);
  const float set_ent_coef = ppo_hyper_f32(hyper, CARL_PPO_HYPER_ENT_COEF);
  const float* const set_params = a.params + (size_t)set * a.shape.set_floats;
  const float* const set_xform = a.xform + (size_t)set * ps.xform_stride;
  const float* const set_log_std = a.log_std + set;  // (read by the Gaussian actor only)
  float* const set_slab = a.slab + (size_t)set * ps.slab_stride;
  const int32_t* const set_idx = ps.idx + (size_t)set * ps.idx_stride;
  const float* const set_adv_norm = ps.adv_norm != nullptr ? ps.adv_norm + (size_t)set * ps.adv_stride : nullptr;
  const int set_lane_lo = set * ps.lanes_per_set, set_lane_hi = set_lane_lo + ps.lanes_per_set;
#define PPO_MB_LANE_WINDOW true
#define PPO_MB_LANE_LO set_lane_lo
#define PPO_MB_LANE_HI set_lane_hi
#define PPO_MB_PARAMS set_params
#define PPO_MB_XFORM set_xform
#define PPO_MB_LOG_STD set_log_std
#define PPO_MB_SLAB set_slab
#define PPO_MB_NEW_OUT static_cast<float*>(nullptr)
#define PPO_MB_IDX set_idx
#define PPO_MB_ADV_NORM set_adv_norm
#define PPO_MB_CLIP_RANGE set_clip_range
#define PPO_MB_VF_COEF set_vf_coef
#define PPO_MB_ENT_COEF set_ent_coef
#include "ppo_net_body.inc"
#include "ppo_net_body_undef.inc"
}

// The slabs of every member, in workgroup order: ppo_reduce_kernel's rule per member.  `a0` holds member 0's pointers.
struct PpoReduceSetsArgs {
  long long slab_actor_stride, slab_critic_stride;  // floats between two members' slabs
};

// Preconditions (host): gridDim.y == n_sets; grad_actor / grad_critic [n_sets][set_floats], grad_log_std [n_sets],
// stats [n_sets][6]
__global__ void __launch_bounds__(256) ppo_reduce_sets_kernel(const PpoReduceArgs a0, const PpoReduceSetsArgs p) {
  const size_t set = blockIdx.y;
  PpoReduceArgs a = a0;
  a.slab_actor += set * p.slab_actor_stride;
  a.slab_critic += set * p.slab_critic_stride;
  a.grad_actor += set * a0.actor.set_floats;
  a.grad_critic += set * a0.critic.set_floats;
  a.grad_log_std += set;  // (written by a Gaussian actor only)
  a.stats += set * 6;
#include "ppo_reduce_body.inc"
}

// ---- one epoch's advantage statistics of every member: workgroup (k, s) takes minibatch k of member s's epoch
// Preconditions (host): ppo_adv_stats_kernel's per row; gridDim.y == n_sets; a.idx [n_sets][idx_stride], a.adv_norm
// [n_sets][gridDim.x][2]
__global__ void __launch_bounds__(kAdvThreads) ppo_adv_stats_sets_kernel(const PpoAdvStatsArgs a, const long long idx_stride) {
#pragma clang fp contract(off)
  const int32_t* const set_idx = a.idx + (size_t)blockIdx.y * idx_stride;
  float* const set_adv_norm = a.adv_norm + (size_t)blockIdx.y * gridDim.x * 2;
#define ADV_MB_IDX set_idx
#define ADV_MB_ADV_NORM set_adv_norm
#include "ppo_adv_stats_body.inc"
#undef ADV_MB_IDX
#undef ADV_MB_ADV_NORM
}

// ---- the global-norm clip and Adam of every member: workgroup s takes row s of every [n_sets][n] tensor, step [n_sets],
// beta_pow / norm_out [n_sets][2]; lr and max_grad_norm from member s's hyper row (a.lr, a.max_grad_norm are not read)
// Preconditions (host): adam_step_kernel's per member; gridDim.x == n_sets
__global__ void __launch_bounds__(kAdamThreads) adam_step_sets_kernel(const AdamArgs a, const double* __restrict__ hyper) {
#pragma clang fp contract(off)
  const size_t set = blockIdx.x;
  const double set_lr = hyper[set * CARL_PPO_HYPER + CARL_PPO_HYPER_LR];
  const double set_max_grad_norm = hyper[set * CARL_PPO_HYPER + CARL_PPO_HYPER_MAX_GRAD_NORM];
  int64_t* const set_step = a.step + set;
  double* const set_beta_pow = a.beta_pow + 2 * set;
  double* const set_norm_out = a.norm_out != nullptr ? a.norm_out + 2 * set : nullptr;
#define ADAM_MB_ROW(first_row, t) (first_row + set * (size_t)a.n[t])
#define ADAM_MB_STEP set_step
#define ADAM_MB_BETA_POW set_beta_pow
#define ADAM_MB_NORM_OUT set_norm_out
#define ADAM_MB_LR set_lr
#define ADAM_MB_MAX_GRAD_NORM set_max_grad_norm
#include "adam_step_body.inc"
#include "adam_step_body_undef.inc"
}

}  // namespace carl
