// ppo_kernels.hip.h -- the kernels of the PPO update on the device (include/carl_amd.h: carl_policy_context_trace,
// carl_ppo_grad): ppo_net_kernel<H> (ppo_net_kernel.hip.h), and here the two that are not templates, the slab reduction
// and the trace walk.  Included by carl_ppo.hip only, so the library holds one definition of each of the two: the Brax
// unit runs its trace through carl_ppo.hip's launch_context_trace (ppo_host.hpp) and has a reduction of its own.  The
// layout, the argument structs and the tile helpers are ppo_device.hip.h's; carl_device.hip.h's select_context is
// called, not changed.
#pragma once

#include "ppo_net_kernel.hip.h"

namespace carl {

// One thread per output: the packed gradient entries of the actor, then of the critic, then the 6 statistics and
// grad_log_std.  Every sum is a fixed function of the slabs.
__global__ void __launch_bounds__(256) ppo_reduce_kernel(const PpoReduceArgs a) {
  const int n_a = a.actor.set_floats, n_c = a.critic.set_floats;
  const int sa = ppo_slab_floats(a.h_actor), sc = ppo_slab_floats(a.h_critic);
  const int ka = ppo_offsets(a.h_actor).kNet, kc = ppo_offsets(a.h_critic).kNet;
  for (int e = (int)(blockIdx.x * blockDim.x + threadIdx.x); e < n_a + n_c + 8; e += (int)(gridDim.x * blockDim.x)) {
    if (e < n_a) {
      a.grad_actor[e] = e < a.actor.weight_floats
          ? (float)(ppo_slab_sum(a.slab_actor, sa, a.n_workgroups, ppo_slab_index(a.h_actor, a.actor, e)) * a.inv_m) : 0.0f;
    } else if (e < n_a + n_c) {
      const int k = e - n_a;
      a.grad_critic[k] = k < a.critic.weight_floats
          ? (float)(ppo_slab_sum(a.slab_critic, sc, a.n_workgroups, ppo_slab_index(a.h_critic, a.critic, k)) * a.inv_m) : 0.0f;
    } else {
      const int q = e - n_a - n_c;
      if (q < 4) a.stats[q == 0 ? 0 : q + 1] = (float)(ppo_slab_sum(a.slab_actor, sa, a.n_workgroups, ka + q) * a.inv_m);
      else if (q == 4) a.stats[1] = (float)(ppo_slab_sum(a.slab_critic, sc, a.n_workgroups, kc + 4) * a.inv_m);
      else if (q == 5) a.stats[5] = a.n_samples;
      else if (q == 6 && a.gaussian) a.grad_log_std[0] = (float)(ppo_slab_sum(a.slab_actor, sa, a.n_workgroups, ka + 5) * a.inv_m);
    }
  }
}

// ---- the context each step ran in (include/carl_amd.h: carl_policy_context_trace).  One thread owns one lane's column
// and walks it forward; the flag loads of kTraceRows rows are issued before the dependent chain of those rows, as
// gae_kernel's.  pitch is never 0 here.
constexpr int kTraceRows = 8;

__global__ void __launch_bounds__(kTraceThreads)
    context_trace_kernel(const carl_batch_t b, const int32_t* __restrict__ ctx_idx0, const uint32_t* __restrict__ episode0,
                         const uint8_t* __restrict__ terminated, const uint8_t* __restrict__ truncated, const int n_steps,
                         const int pitch, int32_t* __restrict__ context_id) {
  const int lane = (int)blockIdx.x * kTraceThreads + (int)threadIdx.x;
  if (lane >= b.n_lanes) return;
  const size_t n = (size_t)pitch;
  const uint64_t glane = (uint64_t)(b.lane_offset + lane);
  const bool autoreset = (b.flags & CARL_FLAG_AUTORESET) != 0;
  int c = ctx_idx0[lane];
  uint32_t e = episode0[lane];
#pragma unroll 1
  for (int t0 = 0; t0 < n_steps; t0 += kTraceRows) {
    uint8_t te[kTraceRows], tr[kTraceRows];
#pragma unroll
    for (int k = 0; k < kTraceRows; ++k) {
      if (t0 + k < n_steps) {  // (uniform)
        const size_t i = (size_t)(t0 + k) * n + lane;
        te[k] = terminated[i];
        tr[k] = truncated[i];
      }
    }
#pragma unroll
    for (int k = 0; k < kTraceRows; ++k) {
      if (t0 + k < n_steps) {
        context_id[(size_t)(t0 + k) * n + lane] = c;
        if (autoreset && (te[k] | tr[k]) != 0) {  // reset_lane's order: the selector, then the episode counter
          c = select_context(b, c, glane, e);
          e += 1u;
        }
      }
    }
  }
}

}  // namespace carl
