// ppo_host.hpp -- the one host path of the PPO update on the device, shared by its two translation units (carl_ppo.hip,
// carl_brax_ppo.hip): the shape and grid rules, the batch, workspace and critic checks with their messages
// (ppo_host_checks.hpp, which a population's unit includes without the launches), and the launch sequence actor -> critic
// -> reduction.  Each rule is written once; a unit adds its network, family and row-pitch
// checks, its workspace size and its own kernels.  Host code; launch_ppo_net instantiates ppo_net_kernel<H> in the unit
// that includes this file.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/carl_amd.h"
#include "host_common.hpp"
#include "policy_host.hpp"
#include "policy_launch.hpp"
#include "ppo_host_checks.hpp"
#include "ppo_net_kernel.hip.h"

namespace carl_host {

// The library's one instance of context_trace_kernel (defined in carl_ppo.hip): the walk over a validated batch with at
// least one lane and one step; pitch is never 0
int launch_context_trace(const char* who, const carl_batch_t& b, const int32_t* ctx_idx0, const uint32_t* episode0,
                         const uint8_t* terminated, const uint8_t* truncated, int n_steps, int pitch, int32_t* context_id,
                         hipStream_t s);

// a network kernel instance with its dynamic LDS
inline int launch_ppo_kernel(const char* who, void (*fn)(carl::PpoNetArgs), size_t lds, const carl::PpoNetArgs& a, int grid,
                             hipStream_t s) {
  if (int e = ensure_dynamic_lds(reinterpret_cast<const void*>(fn), lds, who)) return e;
  hipLaunchKernelGGL(fn, dim3(grid), dim3(carl::kPpoThreads), lds, s, a);
  return check_launch(who);
}

// ppo_net_kernel<H> for a network of padded hidden width H
inline int launch_ppo_net(const char* who, int H, const carl::PpoNetArgs& a, int grid, hipStream_t s) {
  return with_padded_hidden(H, [&](auto h) {
    constexpr int kH = decltype(h)::value;
    static_assert(carl::ppo_lds_bytes(kH) <= carl::kCuLdsBytes, "a PPO network launch's LDS does not fit a compute unit");
    return launch_ppo_kernel(who, carl::ppo_net_kernel<kH>, carl::ppo_lds_bytes(kH), a, grid, s);
  });
}

// what differs between the units' launch sequences
struct PpoUnit {
  int (*set_floats)(const carl_policy_t*);  // ppo_shape_of's
  int (*actor_slab_floats)(int H);          // floats of one workgroup's slab of the actor
  void (*reduce)(carl::PpoReduceArgs);      // the unit's reduction kernel
  int reduce_extra;                         // its outputs behind the two gradients: the statistics and grad_log_std
};

// The three launches of a validated call: the actor through launch_actor(H, args, grid), the critic on the actor's
// transformed inputs through launch_ppo_net, then the slabs in workgroup order.  actor_kind: kPpoCategorical / kPpoGaussian
template <class LaunchActor>
int launch_ppo_update(const char* who, const PpoUnit& unit, const carl_ppo_batch_t* ppo, int pitch, int actor_kind,
                      const carl_policy_t* policy, const carl_policy_t* critic, const float* log_std,
                      const carl_ppo_out_t* out, hipStream_t s, LaunchActor&& launch_actor) {
  const int grid = ppo_workgroups(ppo->n_samples);
  const int ha = policy_padded_hidden(policy), hc = policy_padded_hidden(critic);
  carl::PpoNetArgs a{};
  a.b = *ppo;
  a.b.row_pitch = pitch;
  a.n_ctx = policy->n_ctx;
  for (int k = 0; k < policy->n_ctx; ++k) a.ctx_rows[k] = policy->ctx_rows[k];
  a.xform = policy->params + policy_transform_offset(policy);
  a.log_std = log_std;
  a.n_tiles = (ppo->n_samples + carl::kPpoTile - 1) / carl::kPpoTile;
  // the actor
  a.shape = ppo_shape_of(policy, unit.set_floats);
  a.kind = actor_kind;
  a.params = policy->params;
  a.slab = out->workspace;
  a.new_out = out->new_log_prob;
  if (int e = launch_actor(ha, a, grid)) return e;
  // the critic, on the actor's transformed inputs
  carl::PpoNetArgs c = a;
  c.shape = ppo_shape_of(critic, unit.set_floats);
  c.kind = carl::kPpoValue;
  c.params = critic->params;
  c.slab = out->workspace + (size_t)grid * unit.actor_slab_floats(ha);
  c.new_out = out->new_value;
  if (int e = launch_ppo_net(who, hc, c, grid, s)) return e;
  // the slabs, in workgroup order
  carl::PpoReduceArgs r{};
  r.actor = a.shape, r.critic = c.shape;
  r.h_actor = ha, r.h_critic = hc;
  r.n_workgroups = grid;
  r.gaussian = actor_kind == carl::kPpoGaussian ? 1 : 0;
  r.inv_m = 1.0 / (double)ppo->n_samples;
  r.n_samples = (float)ppo->n_samples;
  r.slab_actor = a.slab, r.slab_critic = c.slab;
  r.grad_actor = out->grad_actor, r.grad_critic = out->grad_critic, r.grad_log_std = out->grad_log_std;
  r.stats = out->stats;
  const int outputs = r.actor.set_floats + r.critic.set_floats + unit.reduce_extra;
  hipLaunchKernelGGL(unit.reduce, dim3((outputs + 255) / 256), dim3(256), 0, s, r);
  return check_launch(who);
}

}  // namespace carl_host
